"""Pressure-Poisson initialisation on the HIP path: ``lt_jacobi`` alone against the reference's iterates
(tests/golden/jacobi_*.npz, made by tools/gen_golden_jacobi.py), its stopping rule, its refusals, and
``lt.DecayingTurbulence`` with its defaults on a native context (tests/golden/pressure_decay_16x16.npz).

Bounds.  Iterates, and the density of ``pressure_poisson`` in fp64: bit for bit.  The reported error: within
(N + 1) * 2^-53 relative of the golden mean square (math.fsum over the fp64 squares of the reference's residuum, divided
by N): (N - 1) * 2^-53 is the worst case of any summation order of N non-negative terms, and the division by N rounds
once on either side.  The constructed populations in fp64: 2e-14, the bound
tests/test_gpu_spectrum.py and tests/test_spectrum_host.py hold this flow's initial state to.  fp32, the project's
error-budget convention (tests/test_gpu_fp32_error_budget.py): with E(x) = max |x - the reference's fp64 result|,
E(engine) <= FACTOR * E(the reference's own fp32 result), FACTOR = 4; from the golden E_ref = 5.85e-8 for the density
and 1.06e-7 for the populations."""
import ctypes

import numpy as np
import pytest
import torch

import lettuce_amd as lt
from conftest import golden, TORCH_DT
from test_gpu_fp32_error_budget import FACTOR
from test_jacobi_kernel_host import sum_bound
from test_pressure_poisson_host import SHAPES, IDS, STOPS, jacobi_fixture, same_bits, decay

pytestmark = pytest.mark.gpu

FP64 = 2e-14
DEVICE = "cuda:0"


def native(dt):
    return lt.Context(device=DEVICE, dtype=TORCH_DT[dt], use_native=True)


def fields(g, dt):
    return tuple(torch.as_tensor(g[k]).to(TORCH_DT[dt]).to(DEVICE) for k in ("rhs", "p0"))


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_fixed_counts_bit_for_bit(shape, dt):
    from lettuce_amd import _native
    g = jacobi_fixture(shape)
    rhs, p0 = fields(g, dt)
    before = p0.clone()
    n = int(np.prod(shape))
    for steps in (0, 1, 2, 3, 8):
        p, iterations, error = _native.jacobi(rhs, p0, float(g["dx"]), 0.0, steps)
        again = _native.jacobi(rhs, p0, float(g["dx"]), 0.0, steps)
        assert iterations == steps and again[1] == steps
        assert torch.equal(p0, before)
        if steps == 0:
            assert torch.equal(p, p0) and error == 1.0
            continue
        assert same_bits(p, g[f"p{steps}_{dt}"]), f"{shape} {dt}: iterate {steps}"
        assert torch.equal(again[0], p) and np.float64(again[2]).tobytes() == np.float64(error).tobytes()
        want = float(g[f"err_{dt}"][steps - 1])
        if steps == 8:                # the stored residuum gives the stored error
            assert sum_bound(g[f"r8_{dt}"])[0] / n == want
        bound = (n + 1) * 2.0 ** -53 * want
        print(f"{shape} {dt} after {steps}: error {error:.17e}, reference {want:.17e}, |difference| "
              f"{abs(error - want):.3e} (bound {bound:.3e})")
        assert abs(error - want) <= bound


@pytest.mark.parametrize("batch", [1, 64], ids=["batch1", "batch64"])
@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("shape", STOPS, ids=["12x20", "6x10x7"])
def test_tolerance_stop_is_the_references(shape, dt, batch):
    """the count and the iterate of the reference; with a batch above the count the sweeps enqueued behind the stop find
    the flag up and must leave p alone"""
    from lettuce_amd import _native
    g = jacobi_fixture(shape)
    rhs, p0 = fields(g, dt)
    p, iterations, error = _native.jacobi(rhs, p0, float(g["dx"]), float(g[f"tol_{dt}"]), 100, batch=batch)
    assert iterations == int(g[f"stop_it_{dt}"]) == 6
    assert same_bits(p, g[f"stop_{dt}"])
    assert error <= float(g[f"tol_{dt}"]) and error == pytest.approx(float(g[f"err_{dt}"][5]), rel=1e-12)
    # through the public function too
    assert same_bits(lt.util.torch_jacobi(rhs, p0, float(g["dx"]), len(shape), tol_abs=float(g[f"tol_{dt}"]),
                                          max_num_steps=100), g[f"stop_{dt}"])


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_a_nan_stops_after_one_iteration(dt):
    from lettuce_amd import _native
    g = jacobi_fixture([12, 20])
    rhs, p0 = fields(g, dt)
    rhs[3, 4] = float("nan")
    p, iterations, error = _native.jacobi(rhs, p0, float(g["dx"]), 0.0, 50)
    assert iterations == 1 and np.isnan(error)
    want = lt.util.torch_jacobi(rhs.cpu(), p0.cpu(), float(g["dx"]), 2, tol_abs=0.0, max_num_steps=50)
    assert int(torch.isnan(want).sum()) == 1
    assert torch.equal(torch.isnan(p).cpu(), torch.isnan(want))
    assert torch.equal(torch.nan_to_num(p).cpu(), torch.nan_to_num(want))


def test_decaying_turbulence_defaults_fp64():
    g = golden("pressure_decay_16x16")
    flow = decay(native("f64"), initialize_pressure=False)
    p0, u0 = flow.initial_pu()
    rho0 = flow.context.convert_to_tensor(flow.units.convert_pressure_pu_to_density_lu(p0))
    u0 = flow.context.convert_to_tensor(flow.units.convert_velocity_to_lu(u0))
    rho = lt.pressure_poisson(flow.units, u0, rho0)
    assert rho.is_cuda and same_bits(rho, g["rho_f64"])
    flow = decay(native("f64"))
    assert flow.initialize_pressure and flow.initialize_fneq and flow.f.is_cuda
    err = float(np.abs(flow.f.cpu().numpy() - g["f_f64"]).max())
    print(f"decay 16x16 f64: max |f - reference| {err:.3e} (bound {FP64:.0e})")
    assert err <= FP64


def test_decaying_turbulence_defaults_fp32_within_the_reference_error_budget():
    g = golden("pressure_decay_16x16")
    flow = decay(native("f32"), initialize_pressure=False)
    p0, u0 = flow.initial_pu()
    rho0 = flow.context.convert_to_tensor(flow.units.convert_pressure_pu_to_density_lu(p0))
    u0 = flow.context.convert_to_tensor(flow.units.convert_velocity_to_lu(u0))
    rho = lt.pressure_poisson(flow.units, u0, rho0).cpu().numpy().astype(np.float64)
    f = decay(native("f32")).f.cpu().numpy().astype(np.float64)
    for what, got, ref32, ref64 in (("rho", rho, g["rho_f32"], g["rho_f64"]), ("f", f, g["f_f32"], g["f_f64"])):
        e_ref = float(np.abs(ref32.astype(np.float64) - ref64).max())
        e = float(np.abs(got - ref64).max())
        print(f"decay 16x16 f32 {what}: E_ref {e_ref:.3e}, E {e:.3e}, ratio {e / e_ref:.3f} (bound {FACTOR})")
        assert e_ref > 0 and e <= FACTOR * e_ref


def test_refusals_and_a_valid_call_behind_them():
    from lettuce_amd import _native
    lib = _native.load_library()
    g = jacobi_fixture([5, 7])
    rhs, p0 = fields(g, "f64")
    p, scratch = p0.clone(), torch.empty_like(p0)
    work = torch.empty(_native.JACOBI_WORK_BYTES // 8, dtype=torch.float64, device=DEVICE)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())

    def call(p_=p, scratch_=scratch, rhs_=rhs, dtype=1, dims=2, shape=(5, 7, 0), steps=3, batch=0, work_=work):
        it, err = ctypes.c_int64(-1), ctypes.c_double(-1.0)
        code = lib.lt_jacobi(None if p_ is None else ptr(p_), None if scratch_ is None else ptr(scratch_),
                             None if rhs_ is None else ptr(rhs_), dtype, dims, (ctypes.c_int64 * 3)(*shape), 0.37, 0.0,
                             steps, batch, None if work_ is None else ptr(work_), ctypes.byref(it), ctypes.byref(err),
                             torch.cuda.current_stream().cuda_stream)
        return code, lib.lt_last_error().decode(), it.value

    for kwargs, text in ((dict(p_=None), "null"), (dict(scratch_=None), "null"), (dict(rhs_=None), "null"),
                         (dict(work_=None), "null"), (dict(dims=1), "1 dimensions"), (dict(dims=4), "4 dimensions"),
                         (dict(shape=(5, 0, 0)), "shape[1] = 0"), (dict(dims=3), "shape[2] = 0"),
                         (dict(dtype=2), "unknown dtype 2"), (dict(steps=-1), "max_num_steps = -1")):
        code, message, it = call(**kwargs)
        assert code == 1 and text in message and it == -1, (kwargs, code, message)
    assert torch.equal(p, p0)
    code, message, it = call()
    assert code == 0 and it == 3
    assert same_bits(p, g["p3_f64"])


@pytest.mark.parametrize("kind", ["view", "fp16"])
def test_other_tensors_take_the_torch_expression(kind):
    from lettuce_amd import util
    g = jacobi_fixture([12, 20])
    rhs, p0 = fields(g, "f32")
    if kind == "view":
        rhs, p0 = rhs.t(), p0.t()
        assert not p0.is_contiguous()
    else:
        rhs, p0 = rhs.half(), p0.half()
    assert util._jacobi_engine(rhs, p0, 2) is None
    got = util.torch_jacobi(rhs, p0, 0.37, 2, tol_abs=0.0, max_num_steps=3)
    assert got.dtype == p0.dtype and got.is_cuda
    want = util.torch_jacobi(rhs.cpu().float(), p0.cpu().float(), 0.37, 2, tol_abs=0.0, max_num_steps=3)
    tol = 2e-6 if kind == "view" else 2e-2
    assert float((got.cpu().float() - want).abs().max()) <= tol * float(want.abs().max())
    # ... while their contiguous fp32 forms go to the engine and give the reference's bits
    if kind == "view":
        assert util._jacobi_engine(rhs.contiguous(), p0.contiguous(), 2) is not None
        assert torch.equal(util.torch_jacobi(rhs.contiguous(), p0.contiguous(), 0.37, 2, tol_abs=0.0, max_num_steps=3).cpu(),
                           want)
