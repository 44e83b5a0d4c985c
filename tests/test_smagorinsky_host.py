"""SmagorinskyCollision on the host (CPU, no GPU needed): the mirror's torch path against vectors produced by the
reference's own CPU path (tests/golden/smagorinsky_*.npz, made by tools/gen_golden_smagorinsky.py), and the plumbing
that hands the operator to the HIP engine (descriptor, binding, header, exported symbol, refusals).

Bounds: fp64 the project's 2e-14, fp32 the 8e-7 KBC is held to against the reference, for the collided field, tau_eff
and every stepped snapshot alike."""
import os
import re

import numpy as np
import pytest
import torch

import lettuce_amd as lt
from conftest import golden, unpack_nsm, TORCH_DT, ROOT
from test_host_api import UniformFlow, ctx

ATOL = {"f64": 2e-14, "f32": 8e-7}
LATTICES = {"d2q9": lt.D2Q9, "d3q15": lt.D3Q15, "d3q19": lt.D3Q19, "d3q27": lt.D3Q27}
PERIODIC = [f"smagorinsky_{lat}_{kind}_{dt}" for lat in LATTICES for kind in ("default", "strong")
            for dt in ("f64", "f32")]


def close(got, want, dt):
    got, want = np.asarray(got), np.asarray(want)
    err = float(np.abs(got - want).max())
    print(f"max |difference| {err:.3e} (bound {ATOL[dt]:.1e})")
    np.testing.assert_allclose(got, want, rtol=0, atol=ATOL[dt])


def fixture_flow(g, name):
    _, lat, _, dt = name.split("_")
    flow = lt.TaylorGreenVortex(ctx(dt), [int(r) for r in g["resolution"]], float(g["reynolds"]), float(g["mach"]),
                                LATTICES[lat]())
    flow.f = torch.tensor(g["f0"])
    return flow, dt


@pytest.mark.parametrize("name", PERIODIC)
def test_torch_path_matches_the_reference(name):
    """collision(flow), its tau_eff field, f after 1, 2, 3 and 10 steps and the kinetic-energy series"""
    g = golden(name)
    flow, dt = fixture_flow(g, name)
    assert flow.f.dtype == TORCH_DT[dt]
    collision = lt.SmagorinskyCollision(float(g["tau"]), float(g["constant"]))
    assert collision.tau_eff == collision.tau                      # until the first call
    f0 = flow.f.clone()
    close(collision(flow).numpy(), g["collided"], dt)
    assert torch.equal(flow.f, f0)
    assert collision.tau_eff.shape == tuple(g["tau_eff"].shape)
    close(collision.tau_eff.numpy(), g["tau_eff"], dt)
    sim = lt.Simulation(flow, collision, [])
    energy = [float(lt.IncompressibleKineticEnergy(flow)())]
    for i in range(1, 11):
        sim(1)
        energy.append(float(lt.IncompressibleKineticEnergy(flow)()))
        if i in (1, 2, 3, 10):
            close(flow.f.numpy(), g[f"f{i}"], dt)
    np.testing.assert_allclose(energy, g["energy_pu"], rtol=1e-12 if dt == "f64" else 2e-6, atol=0)


@pytest.mark.parametrize("name", [n for n in PERIODIC if "strong" in n])
def test_strong_fixtures_tell_the_operator_from_bgk_and_from_one_iteration(name):
    """what the generator asserted when it wrote them, checked again on the mirror: these vectors would catch an
    operator that is plain BGK, or one that stops after the first iteration"""
    g = golden(name)
    flow, dt = fixture_flow(g, name)
    tau, constant = float(g["tau"]), float(g["constant"])
    need = 50 * (1e-12 if dt == "f64" else 3.5e-6)
    assert np.abs(lt.BGKCollision(tau)(flow).numpy() - g["collided"]).max() >= need
    once = lt.SmagorinskyCollision(tau, constant)
    once.iterations = 1
    assert np.abs(once(flow).numpy() - g["collided"]).max() >= need


OBSTACLES = [("smagorinsky_obstacle2d_d2q9_f64", lt.D2Q9, "f64"), ("smagorinsky_obstacle3d_d3q19_f32", lt.D3Q19, "f32")]


def obstacle_from(g, stencil, context):
    flow = lt.Obstacle(context, [int(r) for r in g["resolution"]], 100, 0.1, float(g["domain_length_x"]),
                       stencil=stencil())
    flow.mask = g["obstacle_mask"]
    flow.initialize()
    collision = lt.SmagorinskyCollision(flow.units.relaxation_parameter_lu, float(g["constant"]))
    return flow, lt.Simulation(flow, collision, [])


@pytest.mark.parametrize("name,stencil,dt", OBSTACLES, ids=[o[0] for o in OBSTACLES])
def test_obstacle_with_inlet_outlet_and_body_matches_the_reference(name, stencil, dt):
    g = golden(name)
    flow, sim = obstacle_from(g, stencil, ctx(dt))
    close(flow.f.numpy(), g["f0"], dt)
    assert sim.collision.tau == pytest.approx(float(g["tau"]), rel=1e-15)
    assert [type(b).__name__ for b in sim.boundaries[1:]] == list(g["boundary_order"])
    np.testing.assert_array_equal(sim.no_collision_mask.numpy(), g["no_collision_mask"])
    np.testing.assert_array_equal(sim.no_streaming_mask.numpy(), unpack_nsm(g))
    done = 0
    for n in (1, 2, 10):
        sim(n - done)
        done = n
        close(flow.f.numpy(), g[f"f{n}"], dt)


def test_d1q3_conserves_mass_and_momentum():
    """the reference has no 1-D fixture flow: invariants of the torch path on D1Q3"""
    flow = UniformFlow(ctx(), [32], 1, 0.01, lt.D1Q3())
    torch.manual_seed(4)
    flow.f = flow.f * (1 + 0.1 * torch.rand_like(flow.f))
    rho0, j0 = flow.rho(), flow.j()
    collision = lt.SmagorinskyCollision(0.51, 1.0)
    out = collision(flow)
    assert torch.allclose(flow.rho(out), rho0, atol=1e-13) and torch.allclose(flow.j(out), j0, atol=1e-13)
    assert collision.tau_eff.shape == (32,) and float(collision.tau_eff.min()) >= 0.51
    assert not torch.allclose(out, lt.BGKCollision(0.51)(flow), atol=1e-6)


def test_fix_point_at_equilibrium():
    flow = UniformFlow(ctx(), [8, 8, 8], 1, 0.01, lt.D3Q19())
    out = lt.SmagorinskyCollision(0.51)(flow)
    assert torch.allclose(out, flow.f, atol=1e-14)


def test_reference_attributes_and_native_availability():
    c = lt.SmagorinskyCollision(0.6)
    assert (c.tau, c.constant, c.iterations, c.force, c.tau_eff) == (0.6, 0.17, 2, None, 0.6)
    assert lt.SmagorinskyCollision(0.6, 0.3).constant == 0.3 and lt.ext.SmagorinskyCollision is lt.SmagorinskyCollision
    assert c.native_available()
    c.iterations = 1
    assert not c.native_available()
    c.iterations = 3
    assert not c.native_available()
    assert not lt.SmagorinskyCollision(0.6, force=object()).native_available()


def test_descriptor_names_the_kind_and_reads_tau_and_constant_late():
    c = lt.SmagorinskyCollision(0.6, 0.2)
    desc = c.native_generator()
    assert desc.kind == "smagorinsky" and desc.arithmetic == "exact"
    assert (desc.tau(None), desc.constant(None)) == (0.6, 0.2)
    c.tau, c.constant = 0.7, 0.4                                  # re-read per batch, like tau
    assert (desc.tau(None), desc.constant(None)) == (0.7, 0.4)
    assert lt.BGKCollision(0.6).native_generator().constant is None
    assert lt.NoCollision().native_generator().constant is None


def test_binding_header_and_library(engine_library):
    import ctypes
    from lettuce_amd import _native
    assert _native.COLLISION_IDS == {"none": 0, "bgk": 1, "kbc": 2, "smagorinsky": 3}
    assert _native.SYMBOLS["lt_plan_set_smagorinsky"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_double])
    assert hasattr(_native.Plan, "set_smagorinsky")
    header = open(os.path.join(ROOT, "include", "lettuce_hip.h")).read()
    assert re.search(r"LT_COLLISION_SMAGORINSKY\s*=\s*3\b", header)
    assert re.search(r"int\s+lt_plan_set_smagorinsky\s*\(\s*lt_plan\s*\*\s*plan\s*,\s*double\s+constant\s*\)\s*;", header)
    assert re.search(r"#define\s+LT_ABI_VERSION\s+2\b", header)    # a new enum value and one new function only
    lib = ctypes.CDLL(engine_library)
    assert hasattr(lib, "lt_plan_set_smagorinsky")
    lib.lt_plan_set_smagorinsky.restype = ctypes.c_int
    lib.lt_plan_set_smagorinsky.argtypes = [ctypes.c_void_p, ctypes.c_double]
    assert lib.lt_plan_set_smagorinsky(None, 0.17) != 0            # a null plan is refused, not dereferenced


def test_native_context_refuses_a_force_or_another_iteration_count():
    """Context(use_native=True) with something the engine has no kernel for raises the usual NativeEngineError (a
    CPU context told it is native: the refusal comes before anything touches a device)"""
    from lettuce_amd._native import NativeEngineError
    context = ctx("f32")
    context.use_native = True
    flow = lt.TaylorGreenVortex(context, [8, 8], 100, 0.05, lt.D2Q9())
    with pytest.raises(NativeEngineError, match="no kernel for: collision 'SmagorinskyCollision'"):
        lt.Simulation(flow, lt.SmagorinskyCollision(0.6, force=object()), [])
    once = lt.SmagorinskyCollision(0.6)
    once.iterations = 1
    with pytest.raises(NativeEngineError, match="SmagorinskyCollision"):
        lt.Simulation(flow, once, [])


# --------------------------------------------------------------------------- densities far from 1
@pytest.mark.parametrize("lat", ["D2Q9", "D3Q19", "D3Q27"])
@pytest.mark.parametrize("kind,constant", [("default", 0.17), ("strong", 1.0)])
def test_mirror_on_the_asymmetric_states_against_the_reference(kind, constant, lat):
    """rho in 0.5 .. 1.5 at tau = 0.501 (1 and 5 steps) and in 1 / 20 .. 20 at tau = 0.7 and 1.7 (tests/golden/asymmetric_*,
    oracle/gen_golden.py): the CPU path the engine tests of these states compare with"""
    from test_gpu_asymmetric_operators import _op, fixture_runs
    op = _op(f"smagorinsky-{kind}", "smagorinsky", lat, constant=constant)
    for what, got, want in fixture_runs(op, f"smagorinsky_{kind}"):
        print(what, end=": ")
        close(got, want, "f64")
