"""The TRT and the regularised collision on the host (CPU, no GPU needed): the mirror's torch path against vectors
produced by the reference's own CPU path (tests/golden/trt_*.npz, regularized_*.npz, made by
tools/gen_golden_relaxations.py), the properties that define the two operators, and the plumbing that hands them to
the HIP engine (descriptors, binding, header, exported symbol, refusals).

Bounds: those of test_smagorinsky_host.py and test_force_host.py -- fp64 the project's 2e-14, fp32 8e-7 -- for the
collided field and every stepped snapshot alike."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import lettuce_amd as lt
from conftest import golden, TORCH_DT, ROOT
from test_host_api import ctx

ATOL = {"f64": 2e-14, "f32": 8e-7}
LATTICES = {"d2q9": lt.D2Q9, "d3q15": lt.D3Q15, "d3q19": lt.D3Q19, "d3q27": lt.D3Q27}
FIXTURES = [f"{operator}_{lat}_{dt}" for operator in ("trt", "regularized") for lat in LATTICES for dt in ("f64", "f32")]
ENGINE_F32 = 1e-5       # the engine tests' fp32 bound, which the fixtures must separate from


def close(got, want, dt):
    got, want = np.asarray(got), np.asarray(want)
    err = float(np.abs(got - want).max())
    print(f"max |difference| {err:.3e} (bound {ATOL[dt]:.1e})")
    np.testing.assert_allclose(got, want, rtol=0, atol=ATOL[dt])


def fixture_flow(g, name):
    operator, lat, dt = name.split("_")
    flow = lt.TaylorGreenVortex(ctx(dt), [int(r) for r in g["resolution"]], float(g["reynolds"]), float(g["mach"]),
                                LATTICES[lat]())
    flow.f = torch.tensor(g["f0"])
    return flow, operator, dt


def make_collision(g, operator):
    if operator == "trt":
        return lt.TRTCollision(float(g["tau"]), float(g["tau_minus"]))
    return lt.RegularizedCollision()           # takes the flow's tau on its first call


def noisy(dt, res, stencil, seed=7, noise=0.05):
    flow = lt.TaylorGreenVortex(ctx(dt), res, 1600, 0.1, stencil())
    g = torch.Generator().manual_seed(seed)
    factor = 1 + noise * (2 * torch.rand(flow.f.shape, generator=g, dtype=torch.float64) - 1)
    flow.f = (flow.f.double() * factor).to(TORCH_DT[dt])
    return flow


SHAPES = [(lt.D2Q9, [8, 6]), (lt.D3Q15, [4, 6, 5]), (lt.D3Q19, [4, 6, 5]), (lt.D3Q27, [4, 6, 5])]


@pytest.mark.parametrize("name", FIXTURES)
def test_torch_path_matches_the_reference(name):
    """collision(flow) and f after 1, 2, 3 and 10 steps"""
    g = golden(name)
    flow, operator, dt = fixture_flow(g, name)
    assert flow.f.dtype == TORCH_DT[dt]
    collision = make_collision(g, operator)
    f0 = flow.f.clone()
    close(collision(flow).numpy(), g["collided"], dt)
    assert torch.equal(flow.f, f0)
    if operator == "regularized":
        assert collision.tau == float(g["tau"]) == float(g["flow_tau"])
    sim = lt.Simulation(flow, collision, [])
    for i in range(1, 11):
        sim(1)
        if i in (1, 2, 3, 10):
            close(flow.f.numpy(), g[f"f{i}"], dt)


@pytest.mark.parametrize("name", FIXTURES)
def test_fixtures_tell_the_operator_from_wrong_ones(name):
    """what the generator asserted when it wrote them, checked again on the mirror: these vectors would catch BGK at
    the same tau in place of either operator and TRT with its two relaxation times swapped -- by 10 engine tolerances
    (fp32: 1e-5) at the collision and 100 after 10 steps"""
    g = golden(name)
    _, operator, dt = fixture_flow(g, name)
    tau = float(g["tau"])
    wrong = {"BGK at the same tau": lt.BGKCollision(tau)}
    if operator == "trt":
        wrong["relaxation times swapped"] = lt.TRTCollision(float(g["tau_minus"]), tau)
    for what, collision in wrong.items():
        flow = fixture_flow(g, name)[0]
        collided = collision(flow).numpy()
        lt.Simulation(flow, collision, [])(10)
        gaps = np.abs(collided - g["collided"]).max(), np.abs(flow.f.numpy() - g["f10"]).max()
        print(f"{what}: {gaps[0]:.2e} / {gaps[1]:.2e}")
        assert gaps[0] >= 10 * ENGINE_F32 and gaps[1] >= 100 * ENGINE_F32, what


@pytest.mark.parametrize("stencil,res", SHAPES)
def test_trt_with_equal_relaxation_times_is_bgk(stencil, res):
    """(sp + sm) / (2 tau) = (f - feq) / tau up to rounding: fp64 rounding level (measured 1.4e-17 on these states)"""
    flow = noisy("f64", res, stencil)
    for tau in (0.51, 0.8, 1.7):
        err = float((lt.TRTCollision(tau, tau)(flow) - lt.BGKCollision(tau)(flow)).abs().max())
        print(f"tau {tau}: {err:.2e}")
        assert err <= 2e-16


@pytest.mark.parametrize("stencil,res", SHAPES)
def test_regularized_at_tau_one_returns_the_equilibrium(stencil, res):
    flow = noisy("f64", res, stencil)
    collision = lt.RegularizedCollision()
    collision(flow)
    collision.tau = 1.0
    assert torch.equal(collision(flow), flow.equilibrium(flow))


@pytest.mark.parametrize("stencil,res", SHAPES)
def test_regularized_forgets_the_higher_moments(stencil, res):
    """two states with equal rho, u and Pi collide to the same result: a perturbation g with sum g = sum e g =
    sum e e g = 0 (the null space of the ten / six moments, from an SVD) changes f by 1e-3 and the result by rounding"""
    flow = noisy("f64", res, stencil)
    e = flow.torch_stencil.e.double()
    d, q = flow.stencil.d, flow.stencil.q
    rows = [torch.ones(q, dtype=torch.float64)] + [e[:, a] for a in range(d)]
    rows += [e[:, a] * e[:, b] for a in range(d) for b in range(a, d)]
    m = torch.stack(rows)
    _, s, vh = torch.linalg.svd(m, full_matrices=True)
    rank = int((s > 1e-10).sum())
    ghost = vh[rank]                                            # a unit vector of the null space
    assert float((m @ ghost).abs().max()) < 1e-14
    collision = lt.RegularizedCollision()
    collision(flow)
    collision.tau = 0.7
    first = collision(flow)
    amplitude = 1e-3 * torch.cos(torch.arange(flow.f[0].numel(), dtype=torch.float64)).reshape(flow.f[0].shape)
    flow.f = flow.f + ghost.reshape([-1] + [1] * d) * amplitude
    second = collision(flow)
    err = float((first - second).abs().max())
    print(f"max |difference| {err:.2e}")
    assert err <= 1e-15
    bgk = float((lt.BGKCollision(0.7)(flow) - first).abs().max())
    assert bgk > 1e-4                                           # BGK keeps them


@pytest.mark.parametrize("stencil,res", SHAPES)
@pytest.mark.parametrize("operator", ["trt", "regularized"])
def test_mass_and_momentum_are_conserved(operator, stencil, res):
    flow = noisy("f64", res, stencil)
    if operator == "trt":
        collision = lt.TRTCollision(0.6, 1.9)
    else:
        collision = lt.RegularizedCollision()
        collision(flow)
        collision.tau = 0.7
    rho, j = flow.rho().clone(), flow.j().clone()
    flow.f = collision(flow)
    # exact in real arithmetic; in fp64 each of the q collided populations is off by a few roundings of 2^-53 |f_q| and
    # the two sums over q add q - 1 roundings of at most 2^-53 rho each: q 2^-52 max(rho) bounds both
    bound = flow.stencil.q * 2.0 ** -52 * float(rho.abs().max())
    errs = float((flow.rho() - rho).abs().max()), float((flow.j() - j).abs().max())
    print(f"mass {errs[0]:.2e}, momentum {errs[1]:.2e} (bound {bound:.2e})")
    assert errs[0] <= bound and errs[1] <= bound


def test_reference_attributes_and_exports():
    trt = lt.TRTCollision(0.8)
    assert (trt.tau_plus, trt.tau_minus) == (0.8, 1.0)                # the reference's default
    assert lt.TRTCollision(0.6, tau_minus=1.4).tau_minus == 1.4
    assert lt.ext.TRTCollision is lt.TRTCollision and lt.ext.RegularizedCollision is lt.RegularizedCollision
    assert isinstance(trt, lt.Collision) and isinstance(lt.RegularizedCollision(), lt.Collision)
    assert trt.native_available() and lt.RegularizedCollision().native_available()
    assert lt.RegularizedCollision().tau is None and lt.RegularizedCollision().Q_matrix is None


def test_regularized_takes_the_flows_tau_on_its_first_call():
    """whatever the constructor got (regularized_collision.py:18-19); later assignments hold"""
    flow = noisy("f64", [8, 6], lt.D2Q9)
    own = flow.units.relaxation_parameter_lu
    collision = lt.RegularizedCollision(0.9)
    assert collision.tau == 0.9
    first = collision(flow)
    assert collision.tau == own and collision.Q_matrix is not None
    assert list(collision.Q_matrix.shape) == [9, 2, 2]
    collision.tau = 0.9
    second = collision(flow)
    assert collision.tau == 0.9
    assert float((first - second).abs().max()) > 1e-4
    feq = flow.equilibrium(flow)
    # f - feq scales with 1 - 1 / tau
    ratio = (1 - 1 / 0.9) / (1 - 1 / own)
    assert float(((second - feq) - ratio * (first - feq)).abs().max()) < 1e-15
    # the descriptor's tau does the same on a fresh object
    fresh = lt.RegularizedCollision(0.9)
    desc = fresh.native_generator()
    assert desc.kind == "regularized" and desc.tau(flow) == own and fresh.tau == own
    fresh.tau = 0.75
    assert desc.tau(flow) == 0.75


def test_descriptors_read_their_values_late():
    flow = noisy("f64", [8, 6], lt.D2Q9)
    trt = lt.TRTCollision(0.8, 1.1)
    desc = trt.native_generator()
    assert isinstance(desc, lt.native_desc.NativeCollision) and desc.kind == "trt"
    assert (desc.tau(flow), desc.tau_minus(flow)) == (0.8, 1.1)
    assert desc.constant is None and desc.force is None
    trt.tau_plus, trt.tau_minus = 0.6, 19.25
    assert (desc.tau(flow), desc.tau_minus(flow)) == (0.6, 19.25)
    assert lt.RegularizedCollision().native_generator().tau_minus is None
    assert lt.BGKCollision(0.6).native_generator().tau_minus is None
    assert lt.SmagorinskyCollision(0.6).native_generator().tau_minus is None


def test_binding_header_and_library(engine_library):
    from lettuce_amd import _native
    assert _native.SYMBOLS["lt_plan_set_trt"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_double])
    assert hasattr(_native.Plan, "set_trt")
    assert _native.COLLISION_IDS == {"none": 0, "bgk": 1, "kbc": 2, "smagorinsky": 3}     # unchanged
    assert _native.MORE_COLLISION_IDS == {"trt": 8, "regularized": 9}
    header = open(os.path.join(ROOT, "include", "lettuce_hip.h")).read()
    assert re.search(r"\bLT_COLLISION_TRT\s*=\s*8\b", header)
    assert re.search(r"\bLT_COLLISION_REGULARIZED\s*=\s*9\b", header)
    assert re.search(r"\bLT_COLLISION_SMAGORINSKY\s*=\s*3\b", header)
    assert re.search(r"int\s+lt_plan_set_trt\s*\(\s*lt_plan\s*\*\s*plan\s*,\s*double\s+tau_minus\s*\)\s*;", header)
    assert re.search(r"#define\s+LT_ABI_VERSION\s+2\b", header)      # two enum values and one function only
    lib = ctypes.CDLL(engine_library)
    assert hasattr(lib, "lt_plan_set_trt")
    lib.lt_plan_set_trt.restype = ctypes.c_int
    lib.lt_plan_set_trt.argtypes = [ctypes.c_void_p, ctypes.c_double]
    lib.lt_abi_version.restype = ctypes.c_int
    assert lib.lt_abi_version() == 2
    assert lib.lt_plan_set_trt(None, 1.1) == 1                       # LT_ERR_INVALID: refused, not dereferenced
    lib.lt_last_error.restype = ctypes.c_char_p
    assert b"null plan" in lib.lt_last_error()


def test_slab_driver_refuses_an_engine_without_set_trt():
    """as it treats set_smagorinsky: a stand-in engine that cannot take tau_minus must not run TRT as something else"""
    class Engine:                                                    # no set_trt
        def set_smagorinsky(self, constant):
            pass

    context = ctx("f32")
    slab = lt.ZSlab([8, 8, 8], 0, 1)
    flow = lt.TaylorGreenVortex(context, slab.extended_resolution, 100, 0.05, lt.D3Q19(), slab=slab)
    with pytest.raises(lt.LettuceException, match="has no trt collision"):
        lt.SlabSimulation(flow, lt.TRTCollision(0.8, 1.1), slab, engine=Engine())


# --------------------------------------------------------------------------- densities far from 1
@pytest.mark.parametrize("lat", ["D2Q9", "D3Q19", "D3Q27"])
@pytest.mark.parametrize("operator", ["trt", "regularized"])
def test_mirror_on_the_asymmetric_states_against_the_reference(operator, lat):
    """rho in 0.5 .. 1.5 at tau = 0.501 (1 and 5 steps) and in 1 / 20 .. 20 at tau = 0.7 and 1.7 (tests/golden/asymmetric_*,
    oracle/gen_golden.py): the CPU path the engine tests of these states compare with"""
    from test_gpu_asymmetric_operators import _op, fixture_runs
    for what, got, want in fixture_runs(_op(operator, "relaxation", lat, operator=operator), operator):
        print(what, end=": ")
        close(got, want, "f64")
