"""The incompressible and the LessMemory equilibrium on the host (CPU, no GPU needed): the mirror's torch path against
vectors produced by the reference's own CPU path (tests/golden/incompressible_*.npz, lessmemory_*.npz, made by
tools/gen_golden_equilibria.py), the descriptors that hand the equilibrium to the HIP engine, and the refusals that need
no device.

Bounds: those of test_relaxations_host.py -- fp64 the project's 2e-14, fp32 8e-7 -- for feq, the initial populations,
the collided field and every stepped snapshot alike."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import lettuce_amd as lt
from lettuce_amd import moments
from conftest import golden, unpack_nsm, TORCH_DT, ROOT
from test_host_api import ctx
from test_relaxations_host import ATOL, LATTICES, ENGINE_F32, close

OPERATORS = ("bgk", "trt", "regularized", "guo")
FIXTURES = [f"incompressible_{operator}_{lat}_{dt}" for operator in OPERATORS for lat in LATTICES for dt in ("f64", "f32")]
OBSTACLES = [f"incompressible_obstacle_{lat}_{dt}" for lat in ("d2q9", "d3q19") for dt in ("f64", "f32")]
LESS_MEMORY = "lessmemory_bgk_d2q9_f64"


def fixture_flow(g, name, equilibrium=None, context=None):
    """the fixture's Taylor-Green vortex with its equilibrium (rho0 as stored), before the noise"""
    _, operator, lat, dt = name.split("_")
    if equilibrium is None:
        equilibrium = lt.IncompressibleQuadraticEquilibrium(float(g["rho0"])) if "rho0" in g else lt.QuadraticEquilibriumLessMemory()
    flow = lt.TaylorGreenVortex(context or ctx(dt), [int(r) for r in g["resolution"]], float(g["reynolds"]), float(g["mach"]),
                                LATTICES[lat](), equilibrium)
    return flow, operator, dt


def make_collision(g, operator, flow):
    if operator == "bgk":
        return lt.BGKCollision(float(g["tau"]))
    if operator == "trt":
        return lt.TRTCollision(float(g["tau"]), float(g["tau_minus"]))
    if operator == "regularized":
        return lt.RegularizedCollision()           # takes the flow's tau on its first call
    acceleration = [float(g["acceleration"])] + [0.0] * (flow.stencil.d - 1)
    return lt.BGKCollision(float(g["tau"]), force=lt.Guo(flow, float(g["tau"]), acceleration))


def obstacle_flow(g, name, context=None, equilibrium=None):
    _, _, lat, dt = name.split("_")
    if equilibrium is None:
        equilibrium = lt.IncompressibleQuadraticEquilibrium(float(g["rho0"]))
    flow = lt.Obstacle(context or ctx(dt), [int(r) for r in g["resolution"]], float(g["reynolds"]), float(g["mach"]),
                       float(g["domain_length_x"]), stencil=LATTICES[lat](), equilibrium=equilibrium)
    flow.mask = g["obstacle_mask"]
    flow.initialize()
    return flow, dt


@pytest.mark.parametrize("name", FIXTURES + [LESS_MEMORY])
def test_torch_path_matches_the_reference(name):
    """Flow.initialize with initialize_f_neq, equilibrium(flow), collision(flow) and f after 1, 2, 3 and 10 steps"""
    g = golden(name)
    flow, operator, dt = fixture_flow(g, name)
    assert flow.f.dtype == TORCH_DT[dt]
    close(flow.f.numpy(), g["finit"], dt)
    flow.f = torch.tensor(g["f0"])
    close(flow.equilibrium(flow).numpy(), g["feq"], dt)
    collision = make_collision(g, operator, flow)
    f0 = flow.f.clone()
    close(collision(flow).numpy(), g["collided"], dt)
    assert torch.equal(flow.f, f0)
    sim = lt.Simulation(flow, collision, [])
    for i in range(1, 11):
        sim(1)
        if i in (1, 2, 3, 10):
            close(flow.f.numpy(), g[f"f{i}"], dt)


@pytest.mark.parametrize("name", FIXTURES)
def test_fixtures_tell_the_equilibrium_from_wrong_ones(name):
    """what the generator asserted when it wrote them, checked again on the mirror: these vectors would catch the
    quadratic equilibrium in place of the incompressible one, and rho0 = 1.0 in place of 1.1 -- by 10 engine tolerances
    (fp32: 1e-5) at the collision and 100 after 10 steps"""
    g = golden(name)
    for what, equilibrium in (("QuadraticEquilibrium", lt.QuadraticEquilibrium()),
                              ("rho0 = 1.0", lt.IncompressibleQuadraticEquilibrium(1.0))):
        flow, operator, _ = fixture_flow(g, name, equilibrium)
        flow.f = torch.tensor(g["f0"])
        collision = make_collision(g, operator, flow)
        collided = collision(flow).numpy()
        lt.Simulation(flow, collision, [])(10)
        gaps = np.abs(collided - g["collided"]).max(), np.abs(flow.f.numpy() - g["f10"]).max()
        print(f"{what}: {gaps[0]:.2e} / {gaps[1]:.2e}")
        assert gaps[0] >= 10 * ENGINE_F32 and gaps[1] >= 100 * ENGINE_F32, what


@pytest.mark.parametrize("name", OBSTACLES)
def test_obstacle_with_the_incompressible_equilibrium_matches_the_reference(name):
    """inlet (its populations are the incompressible equilibrium's), bounce-back block, anti-bounce-back outlet"""
    g = golden(name)
    flow, dt = obstacle_flow(g, name)
    close(flow.f.numpy(), g["f0"], dt)
    sim = lt.Simulation(flow, lt.BGKCollision(flow.units.relaxation_parameter_lu), [])
    assert [type(b).__name__ for b in sim.boundaries[1:]] == list(g["boundary_order"])
    np.testing.assert_array_equal(sim.no_collision_mask.numpy(), g["no_collision_mask"])
    np.testing.assert_array_equal(sim.no_streaming_mask.numpy(), unpack_nsm(g))
    for i in range(1, 11):
        sim(1)
        if i in (1, 2, 3, 10):
            close(flow.f.numpy(), g[f"f{i}"], dt)


@pytest.mark.parametrize("lat,res", [("d2q9", [12, 10]), ("d3q15", [10, 8, 6]), ("d3q19", [10, 8, 6]), ("d3q27", [6, 8, 6])])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_less_memory_is_the_quadratic_equilibrium_bit_for_bit(lat, res, dt):
    """as in the reference: feq, the initial populations, the collided field and 10 steps, BGK and the regularised collision"""
    g = golden(f"incompressible_bgk_{lat}_{dt}")
    results = []
    for equilibrium in (lt.QuadraticEquilibrium(), lt.QuadraticEquilibriumLessMemory()):
        flow = lt.TaylorGreenVortex(ctx(dt), res, 1600, 0.1, LATTICES[lat](), equilibrium)
        out = [flow.f.clone()]
        flow.f = torch.tensor(g["f0"])
        out += [flow.equilibrium(flow), lt.BGKCollision(0.8)(flow), lt.RegularizedCollision()(flow)]
        lt.Simulation(flow, lt.BGKCollision(0.8), [])(10)
        results.append(out + [flow.f.clone()])
    for a, b in zip(*results):
        assert torch.equal(a, b)


def test_reference_attributes_and_exports():
    eq = lt.IncompressibleQuadraticEquilibrium()
    assert eq.rho0 == 1.0                                             # the reference's default
    assert lt.IncompressibleQuadraticEquilibrium(rho0=1.25).rho0 == 1.25
    assert lt.ext.IncompressibleQuadraticEquilibrium is lt.IncompressibleQuadraticEquilibrium
    assert lt.ext.QuadraticEquilibriumLessMemory is lt.QuadraticEquilibriumLessMemory
    for e in (eq, lt.QuadraticEquilibriumLessMemory(), lt.QuadraticEquilibrium()):
        assert isinstance(e, lt.Equilibrium) and e.native_available()


def test_descriptors_read_rho0_late_and_name_the_kind():
    eq = lt.IncompressibleQuadraticEquilibrium(1.1)
    desc = eq.native_generator()
    assert isinstance(desc, lt.native_desc.NativeEquilibrium) and desc.kind == "incompressible"
    assert desc.rho0() == 1.1 and desc.plan_args() == ("incompressible", 1.1)
    eq.rho0 = 0.9
    assert desc.rho0() == 0.9 and desc.plan_args() == ("incompressible", 0.9)
    for e in (lt.QuadraticEquilibrium(), lt.QuadraticEquilibriumLessMemory()):
        d = e.native_generator()
        assert d.kind == "quadratic" and d.rho0 is None and d.plan_args() == ("quadratic", 1.0)
    assert lt.native_desc.NativeEquilibrium().kind == "quadratic"


def test_the_flow_hands_its_equilibrium_to_the_engine_or_steps_aside():
    """Flow._engine_equilibrium: what the plans get (and what joins the steppers' carry key), read on every use; None for
    an equilibrium the engine has no kernel for, a subclass of the library's classes included"""
    class Scaled(lt.QuadraticEquilibrium):
        def __call__(self, flow, rho=None, u=None):
            return 1.01 * super().__call__(flow, rho, u)

    class Own(lt.Equilibrium):
        def __call__(self, flow, rho=None, u=None):
            return 1.01 * lt.QuadraticEquilibrium()(flow, rho, u)

        def native_available(self):
            return False

        def native_generator(self):
            return None

    flow = lt.TaylorGreenVortex(ctx(), [8, 6], 100, 0.05, lt.D2Q9(), lt.IncompressibleQuadraticEquilibrium(1.1))
    assert flow._engine_equilibrium() == ("incompressible", 1.1)
    flow.equilibrium.rho0 = 1.3
    assert flow._engine_equilibrium() == ("incompressible", 1.3)
    flow.equilibrium = lt.QuadraticEquilibriumLessMemory()
    assert flow._engine_equilibrium() == ("quadratic", 1.0)
    for other in (Scaled(), Own()):
        flow.equilibrium = other
        assert flow._engine_equilibrium() is None
        assert not (isinstance(other, Scaled) and other.native_available())


def test_simulation_on_a_native_context_names_what_has_no_kernel():
    """before any plan is made: an equilibrium of the caller's, and the incompressible equilibrium under a collision that
    has no kernel for it (both named)"""
    class Own(lt.Equilibrium):
        def __call__(self, flow, rho=None, u=None):
            return 1.01 * lt.QuadraticEquilibrium()(flow, rho, u)

        def native_available(self):
            return False

        def native_generator(self):
            return None

    flow = lt.TaylorGreenVortex(ctx(), [8, 6], 100, 0.05, lt.D2Q9(), Own())
    flow.context.use_native = True                    # as if a GPU context had been requested
    with pytest.raises(lt.NativeEngineError, match="equilibrium 'Own'"):
        lt.Simulation(flow, lt.BGKCollision(0.8), [])
    flow.equilibrium = lt.IncompressibleQuadraticEquilibrium(1.1)
    collisions = [lt.KBCCollision(), lt.SmagorinskyCollision(0.8),
                  lt.MRTCollision(moments.D2Q9Dellar(lt.D2Q9(), flow.context), [1.0] * 9, flow.context)]
    for collision in collisions:
        with pytest.raises(lt.NativeEngineError) as info:
            lt.Simulation(flow, collision, [])
        assert "equilibrium 'IncompressibleQuadraticEquilibrium'" in str(info.value)
        assert f"collision '{type(collision).__name__}'" in str(info.value)


@pytest.mark.parametrize("driver", ["SlabSimulation", "TwoStepSlabSimulation"])
def test_slab_simulations_refuse_a_non_quadratic_equilibrium_by_name(driver):
    context = ctx("f32")
    slab = lt.ZSlab([8, 8, 8], 0, 1)
    flow = lt.TaylorGreenVortex(context, slab.extended_resolution, 100, 0.05, lt.D3Q19(),
                                lt.IncompressibleQuadraticEquilibrium(1.1), slab=slab)
    with pytest.raises(lt.LettuceException, match="equilibrium 'IncompressibleQuadraticEquilibrium' has no slab kernel"):
        getattr(lt, driver)(flow, lt.BGKCollision(0.8), slab)


def test_binding_header_and_library(engine_library):
    from lettuce_amd import _native
    assert _native.SYMBOLS["lt_plan_set_equilibrium"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_double])
    assert hasattr(_native.Plan, "set_equilibrium")
    assert _native.EQUILIBRIUM_IDS == {"quadratic": 0, "incompressible": 1}
    header = open(os.path.join(ROOT, "include", "lettuce_hip.h")).read()
    assert re.search(r"enum\s+lt_equilibrium_kind\s*\{\s*LT_EQUILIBRIUM_QUADRATIC\s*=\s*0\s*,\s*LT_EQUILIBRIUM_INCOMPRESSIBLE\s*=\s*1\s*\}", header)
    assert re.search(r"int\s+lt_plan_set_equilibrium\s*\(\s*lt_plan\s*\*\s*plan\s*,\s*int\s+kind\s*,\s*double\s+rho0\s*\)\s*;", header)
    assert re.search(r"#define\s+LT_ABI_VERSION\s+2\b", header)      # one enum and one function only
    lib = ctypes.CDLL(engine_library)
    lib.lt_plan_set_equilibrium.restype = ctypes.c_int
    lib.lt_plan_set_equilibrium.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_double]
    lib.lt_abi_version.restype = ctypes.c_int
    assert lib.lt_abi_version() == 2
    assert lib.lt_plan_set_equilibrium(None, 1, 1.1) == 1            # LT_ERR_INVALID: refused, not dereferenced
    lib.lt_last_error.restype = ctypes.c_char_p
    assert b"null plan" in lib.lt_last_error()
