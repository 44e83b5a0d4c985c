"""Pressure-Poisson initialisation on the host (CPU, no GPU needed): ``util.torch_jacobi``, ``pressure_poisson`` and
``Flow.initialize`` with ``initialize_pressure`` against vectors produced by the reference's own CPU path
(tests/golden/jacobi_*.npz and pressure_decay_16x16.npz, made by tools/gen_golden_jacobi.py), and the reference's own
two checks of the solver restated.

Bounds.  The Jacobi iterates and the density of ``pressure_poisson`` in fp64: bit for bit -- the torch expressions are
the reference's, operation for operation.  The constructed populations: 2e-14 in fp64 and 2e-6 in fp32, the bounds
tests/test_host_api.py and tests/test_spectrum_host.py hold initial states of the mirror to.  The physical checks: the
reference's 0.05 (absolute, pressure in PU) and 5 % (L1 against the uninitialised state)."""
import numpy as np
import pytest
import torch

import lettuce_amd as lt
from lettuce_amd._flow import pressure_poisson, initialize_pressure_poisson
from conftest import golden, TORCH_DT
from test_host_api import ctx

SHAPES = [[1, 7], [2, 3], [5, 7], [12, 20], [33, 17], [64, 66], [2, 3, 1], [6, 10, 7], [17, 5, 33]]
STOPS = [[12, 20], [6, 10, 7]]
COUNTS = (1, 2, 3, 8)
IDS = ["x".join(map(str, s)) for s in SHAPES]
ATOL = {"f64": 2e-14, "f32": 2e-6}


def jacobi_fixture(shape):
    return golden("jacobi_" + "x".join(str(n) for n in shape))


def same_bits(got, want):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def test_exports():
    assert lt.util.torch_jacobi is lt.torch_jacobi
    assert lt.pressure_poisson is pressure_poisson and lt.initialize_pressure_poisson is initialize_pressure_poisson


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_torch_jacobi_fixed_counts_bit_for_bit(shape, dt):
    g = jacobi_fixture(shape)
    rhs, p0 = (torch.as_tensor(g[k]).to(TORCH_DT[dt]) for k in ("rhs", "p0"))
    before = p0.clone()
    assert torch.equal(lt.util.torch_jacobi(rhs, p0, float(g["dx"]), len(shape), tol_abs=0.0, max_num_steps=0), p0)
    for n in COUNTS:
        got = lt.util.torch_jacobi(rhs, p0, float(g["dx"]), len(shape), tol_abs=0.0, max_num_steps=n)
        assert same_bits(got, g[f"p{n}_{dt}"]), f"{shape} {dt}: iterate {n}"
    assert torch.equal(p0, before)


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("shape", STOPS, ids=["12x20", "6x10x7"])
def test_torch_jacobi_tolerance_stop_bit_for_bit(shape, dt):
    g = jacobi_fixture(shape)
    rhs, p0 = (torch.as_tensor(g[k]).to(TORCH_DT[dt]) for k in ("rhs", "p0"))
    got = lt.util.torch_jacobi(rhs, p0, float(g["dx"]), len(shape), tol_abs=float(g[f"tol_{dt}"]), max_num_steps=100)
    assert same_bits(got, g[f"stop_{dt}"])
    assert int(g[f"stop_it_{dt}"]) == 6
    # the iterate that stopped is the sixth of the fixed-count sequence: neither the fifth nor the seventh
    for n in (5, 6, 7):
        it = lt.util.torch_jacobi(rhs, p0, float(g["dx"]), len(shape), tol_abs=0.0, max_num_steps=n)
        assert torch.equal(it, got) == (n == 6)
    # a tolerance of 1 or more ends the reference before its first sweep (its error starts at 1)
    assert torch.equal(lt.util.torch_jacobi(rhs, p0, float(g["dx"]), len(shape), tol_abs=1.0), p0)


def decay(context, **kwargs):
    return lt.DecayingTurbulence(context, [16, 16], 1000, 0.05, k0=2, randseed=1, **kwargs)


def test_pressure_poisson_density_bit_for_bit():
    g = golden("pressure_decay_16x16")
    flow = decay(ctx("f64"), initialize_pressure=False)
    p0, u0 = flow.initial_pu()
    rho0 = flow.context.convert_to_tensor(flow.units.convert_pressure_pu_to_density_lu(p0))
    u0 = flow.context.convert_to_tensor(flow.units.convert_velocity_to_lu(u0))
    rho = pressure_poisson(flow.units, u0, rho0)
    assert float(np.abs(g["rho_f64"] - 1).max()) > 1e-4           # the solver moved the density
    assert same_bits(rho, g["rho_f64"])


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_decaying_turbulence_constructs_with_its_defaults(dt):
    g = golden("pressure_decay_16x16")
    flow = decay(ctx(dt))
    assert flow.initialize_pressure and flow.initialize_fneq
    err = float(np.abs(flow.f.numpy().astype(np.float64) - g[f"f_{dt}"]).max())
    print(f"decay 16x16 {dt}: max |f - reference| {err:.3e} (bound {ATOL[dt]:.0e})")
    assert err <= ATOL[dt]
    # ... and the density of the constructed state is the solver's, not 1 (the non-equilibrium part moves it by 3e-10)
    assert float(np.abs(flow.rho().numpy().astype(np.float64) - g["rho_f64"]).max()) <= 1e-6
    assert float(np.abs(flow.rho().numpy().astype(np.float64) - 1).max()) >= 1e-4
    # 3-D switches the option off, as the reference does
    assert not lt.DecayingTurbulence(ctx(dt), [8, 8, 6], 100, 0.05, k0=2, randseed=1).initialize_pressure


def test_initialize_pressure_poisson_reinitialises_the_equilibrium():
    flow = decay(ctx("f64"), initialize_pressure=False, initialize_fneq=False)
    u = flow.u().clone()
    f = initialize_pressure_poisson(flow, max_num_steps=1000, tol_pressure=1e-6)
    assert f.shape == flow.f.shape
    rho = pressure_poisson(flow.units, u, flow.rho(), tol_abs=1e-6, max_num_steps=1000)
    assert torch.equal(f, flow.equilibrium(flow, rho=rho, u=u))
    assert float((rho - 1).abs().max()) > 1e-4


# ------------------------------------------------------------------ the reference's own checks, restated
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_taylor_green_2d_pressure_within_005_of_the_analytic(dt):
    """tests/flow/test_pressure_poisson.py of the reference: TGV 32^2, rho0 = 1"""
    context = ctx(dt)
    flow = lt.TaylorGreenVortex(context, 32, 100, 0.05, lt.D2Q9())
    p0, u = flow.initial_pu()
    u = flow.units.convert_velocity_to_lu(u)
    rho = pressure_poisson(flow.units, u, torch.ones_like(flow.units.convert_pressure_pu_to_density_lu(p0)))
    p_final = flow.units.convert_density_lu_to_pressure_pu(rho).numpy()
    err = float(np.abs(p_final - p0.numpy()).max())
    print(f"TGV 32^2 {dt}: max |p - analytic| {err:.4f} (bound 0.05)")
    assert p_final.shape == tuple(p0.shape) and err <= 0.05


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_taylor_green_2d_l1_pressure_error_falls_below_5_percent(dt):
    """tests/flow/test_initialize_pressure.py of the reference: tol_abs = 1e-6, max_num_steps = 1000"""
    context = ctx(dt)
    flow = lt.TaylorGreenVortex(context, [32] * 2, 10, 0.05, initialize_fneq=False)
    p0, u0 = flow.analytic_solution(t=0)
    u_lu = flow.units.convert_velocity_to_lu(u0)
    rho_lu = torch.ones_like(p0)
    f_before = flow.equilibrium(flow, rho=rho_lu, u=u_lu)
    p_before = flow.units.convert_density_lu_to_pressure_pu(flow.rho(f_before))
    rho_poisson = pressure_poisson(flow.units, u_lu, rho_lu, tol_abs=1e-6, max_num_steps=1000)
    f_after = flow.equilibrium(flow, rho=rho_poisson, u=u_lu)
    p_after = flow.units.convert_density_lu_to_pressure_pu(flow.rho(f_after))
    before, after = float((p_before - p0).abs().sum()), float((p_after - p0).abs().sum())
    print(f"TGV 32^2 {dt}: L1 pressure error {after:.4e}, uninitialised {before:.4e}, ratio {after / before:.4f}")
    assert after < 5e-2 * before
    assert float((p_after - p0).abs().max()) <= 5e-2


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_taylor_green_3d_pressure_within_005_of_the_analytic(dt):
    """the same check on TGV 32^3 with the Laplacian of all three axes (dim = 3: the documented departure; 16^3 gives
    0.055 and is too coarse)"""
    context = ctx(dt)
    flow = lt.TaylorGreenVortex(context, 32, 100, 0.05, lt.D3Q27(), initialize_fneq=False)
    p0, u = flow.initial_pu()
    u = flow.units.convert_velocity_to_lu(u)
    rho = pressure_poisson(flow.units, u, torch.ones_like(flow.units.convert_pressure_pu_to_density_lu(p0)))
    p_final = flow.units.convert_density_lu_to_pressure_pu(rho).numpy()
    err = float(np.abs(p_final - p0.numpy()).max())
    print(f"TGV 32^3 {dt}: max |p - analytic| {err:.4f} (bound 0.05)")
    assert err <= 0.05


def test_torch_jacobi_takes_the_torch_expression_off_the_engines_ground():
    """CPU tensors never reach the engine, whatever the context; a dim that is not the field's rolls only the first dim
    axes, as the reference does"""
    from lettuce_amd import util
    g = jacobi_fixture([6, 10, 7])
    rhs, p0 = (torch.as_tensor(g[k]).double() for k in ("rhs", "p0"))
    assert util._jacobi_engine(rhs, p0, 3) is None
    planes = util.torch_jacobi(rhs, p0, 0.37, 2, tol_abs=0.0, max_num_steps=2)
    each = torch.stack([util.torch_jacobi(rhs[..., k], p0[..., k], 0.37, 2, tol_abs=0.0, max_num_steps=2)
                        for k in range(7)], dim=-1)
    assert torch.equal(planes, each)
    with pytest.raises(lt.LettuceException):
        util.torch_jacobi(rhs, p0, 0.37, 1)


def test_lt_jacobi_refuses_bad_arguments_before_any_hip_call(engine_library):
    """null pointers, dims outside 2-3, an extent < 1, an unknown dtype and a negative max: code 1 and a message, with no
    device in the machine -- the pointers handed over here are never followed.  max_num_steps = 0 returns at once too."""
    import ctypes
    from lettuce_amd import _native
    lib = _native.load_library()
    assert _native.SYMBOLS["lt_jacobi"][1][5] == ctypes.POINTER(ctypes.c_int64)
    fake = ctypes.c_void_p(4096)

    def call(p=fake, scratch=ctypes.c_void_p(8192), rhs=fake, dtype=0, dims=2, shape=(5, 7, 0), steps=3, batch=0, work=fake):
        it, err = ctypes.c_int64(-1), ctypes.c_double(-1.0)
        code = lib.lt_jacobi(p, scratch, rhs, dtype, dims, (ctypes.c_int64 * 3)(*shape), 0.37, 0.0, steps, batch, work,
                             ctypes.byref(it), ctypes.byref(err), None)
        return code, lib.lt_last_error().decode(), it.value, err.value

    for kwargs, text in ((dict(p=None), "null"), (dict(scratch=None), "null"), (dict(rhs=None), "null"),
                         (dict(work=None), "null"), (dict(dims=1), "1 dimensions"), (dict(dims=4), "4 dimensions"),
                         (dict(shape=(5, 0, 0)), "shape[1] = 0"), (dict(shape=(-2, 7, 0)), "shape[0] = -2"),
                         (dict(dims=3), "shape[2] = 0"), (dict(dtype=2), "unknown dtype 2"),
                         (dict(steps=-1), "max_num_steps = -1"), (dict(batch=-1), "batch = -1")):
        code, message, it, _ = call(**kwargs)
        assert code == 1 and text in message and it == -1, (kwargs, code, message)
    assert call(steps=0)[::2] == (0, 0) and call(steps=0)[3] == 1.0
