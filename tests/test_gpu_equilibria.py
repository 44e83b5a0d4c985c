"""The incompressible and the LessMemory equilibrium on the HIP engine (lt_plan_set_equilibrium; the kernels' COLL | 16),
in the manner of test_gpu_relaxations.py.

The references are the vectors of tests/golden/incompressible_*.npz and lessmemory_*.npz (the reference's own CPU path,
tools/gen_golden_equilibria.py) and, where the fixtures have no such grid, the mirror's torch path on a CPU context in
float64, which test_equilibria_host.py pins to those vectors.

Tolerances are the project's own: test_gpu_engine.ATOL 1e-12 / 1e-5 times max(1, |f|max), times max(1, n / 10) in fp32,
times 10 with an anti-bounce-back outlet.  One engine kernel against another is bit for bit.  Every comparison prints
its largest difference before it asserts.
"""
import numpy as np
import pytest
import torch

import lettuce_amd as lt
from lettuce_amd._kept import Phase
from conftest import golden, TORCH_DT
from test_gpu_engine import ATOL, dev
from test_gpu_paths_vs_oracle import perturbed_state
from test_gpu_smagorinsky import assert_close, run
from test_host_api import UniformFlow
from test_equilibria_host import FIXTURES, OBSTACLES, LESS_MEMORY, fixture_flow, make_collision, obstacle_flow

pytestmark = pytest.mark.gpu

RHO0 = 1.1
TAU, TAU_MINUS, ACCELERATION = 0.8, 3.0, 1e-4
KIND = {"bgk": "bgk", "trt": "trt", "regularized": "regularized", "guo": "bgk"}
COLL = {"bgk": 17, "guo": 21, "trt": 24, "regularized": 25}          # the kernels' COLL: 16 + the collision (+ 4: force)
STENCILS = {"D1Q3": lt.D1Q3, "D2Q9": lt.D2Q9, "D3Q15": lt.D3Q15, "D3Q19": lt.D3Q19, "D3Q27": lt.D3Q27}


def native(dt):
    return lt.Context(device="cuda:0", dtype=TORCH_DT[dt], use_native=True)


def make_plan(operator, lat, dt, res, entries=(), rho0=RHO0, tau=TAU, tau_minus=TAU_MINUS, acceleration=ACCELERATION,
              equilibrium="incompressible", **kwargs):
    from lettuce_amd._native import Plan
    plan = Plan(lat, TORCH_DT[dt], KIND[operator], res, entries, **kwargs)
    if operator == "trt":
        plan.set_trt(tau_minus)
    if operator == "guo":
        plan.set_force([acceleration] + [0.0] * (len(res) - 1), 0.5, 1.0 - 1.0 / (2.0 * tau))
    if equilibrium is not None:
        plan.set_equilibrium(equilibrium, rho0)
    return plan


def fixture_plan(g, name, **kwargs):
    _, operator, lat, dt = name.split("_")
    return make_plan(operator, lat.upper(), dt, [int(r) for r in g["resolution"]], rho0=float(g["rho0"]),
                     tau=float(g["tau"]), tau_minus=float(g["tau_minus"]) or 1.0, acceleration=float(g["acceleration"]),
                     **kwargs)


def cpu_collision(operator, flow, tau=TAU):
    if operator == "bgk":
        return lt.BGKCollision(tau)
    if operator == "trt":
        return lt.TRTCollision(tau, TAU_MINUS)
    if operator == "regularized":
        collision = lt.RegularizedCollision()
        collision.native_generator().tau(flow)         # the first use takes the flow's tau ...
        collision.tau = tau                            # ... which an assignment replaces
        return collision
    return lt.BGKCollision(tau, force=lt.Guo(flow, tau, [ACCELERATION] + [0.0] * (flow.stencil.d - 1)))


def cpu_run(operator, lat, f0, steps, tau=TAU, dtype=torch.float64, rho0=RHO0):
    """the mirror's torch path on the CPU in `dtype` from f0: (collided, {n: f after n steps}), float64 arrays"""
    context = lt.Context("cpu", dtype, use_native=False)
    flow = UniformFlow(context, list(f0.shape[1:]), 1, 0.01, STENCILS[lat](), lt.IncompressibleQuadraticEquilibrium(rho0))
    flow.f = f0.to(dtype).clone()
    collision = cpu_collision(operator, flow, tau)
    collided = collision(flow).double().numpy().copy()
    sim, out, done = lt.Simulation(flow, collision, []), {}, 0
    for n in steps:
        sim(n - done)
        done = n
        out[n] = flow.f.double().numpy().copy()
    return collided, out


# --------------------------------------------------------------------------- the plan: lt_collide, lt_run
@pytest.mark.parametrize("name", FIXTURES)
def test_collide_and_steps_against_the_reference_vectors(name):
    """the reference's collided field, and its populations after 1, 2, 3 and 10 steps through lt_run"""
    g = golden(name)
    _, operator, lat, dt = name.split("_")
    plan = fixture_plan(g, name)
    tau = float(g["tau"])
    assert f"lt::{lat}, 0, {COLL[operator]}," in plan.kernel_name(), plan.kernel_name()
    f0 = torch.tensor(g["f0"])
    got = plan.collide(dev(f0), torch.empty_like(dev(f0)), tau).cpu().numpy()
    assert_close(got, g["collided"], dt, what=f"{name} collided")
    # periodic BGK mirrors the reference's operations one for one: bit for bit on the 3-D lattices, fp32 and fp64.  (Not
    # on the D2Q9 fixture, 5.6e-17 / 8.9e-8: ATen's sum over q of a [9, 12, 10] tensor is not the sequential one.)
    exact = operator == "bgk" and lat != "d2q9"
    if exact:
        np.testing.assert_array_equal(got, g["collided"])
    for n in (1, 2, 3, 10):
        stepped = run(plan, f0, n, tau)
        assert_close(stepped, g[f"f{n}"], dt, n, what=f"{name} f{n}")
        assert plan.last_run_info() == {"single_step_launches": n - 1, "two_step_launches": 0, "many_step_launches": 0}
        if exact:
            np.testing.assert_array_equal(stepped, g[f"f{n}"])


@pytest.mark.parametrize("name", [n for n in FIXTURES if "_bgk_" in n])
def test_equilibrium_and_init_fneq_kernels_against_the_reference_vectors(name):
    """plan.equilibrium on the moments of the noisy state, and plan.init_fneq on the moments of the flow's equilibrium
    populations (what initialize_f_neq hands it)"""
    from lettuce_amd._native import Plan
    g = golden(name)
    _, _, lat, dt = name.split("_")
    res = [int(r) for r in g["resolution"]]
    plan = Plan(lat.upper(), TORCH_DT[dt], "none", res)
    plan.set_equilibrium("incompressible", float(g["rho0"]))
    rho, u = plan.macroscopic(dev(torch.tensor(g["f0"])))
    assert_close(plan.equilibrium(rho, u).cpu().numpy(), g["feq"], dt, what=f"{name} feq")
    # the quadratic plan returns something else, by more than ten fp32 tolerances
    plan.set_equilibrium("quadratic")
    assert float(np.abs(plan.equilibrium(rho, u).cpu().numpy() - g["feq"]).max()) > 10 * ATOL["f32"]
    plan.set_equilibrium("incompressible", float(g["rho0"]))
    # Flow.initialize: feq(rho, u) of the initial fields, then initialize_f_neq from its moments
    cpu = fixture_flow(g, name)[0]
    p0, u0 = cpu.initial_pu()
    rho0 = dev(cpu.context.convert_to_tensor(cpu.units.convert_pressure_pu_to_density_lu(p0)))
    u0 = dev(cpu.context.convert_to_tensor(cpu.units.convert_velocity_to_lu(u0)))
    feq0 = plan.equilibrium(rho0, u0)
    rho1, u1 = plan.macroscopic(feq0)
    eye_cs2 = float(torch.tensor(cpu.stencil.cs ** 2, dtype=torch.get_default_dtype()))
    got = plan.init_fneq(rho1, u1, cpu.units.relaxation_parameter_lu, eye_cs2).cpu().numpy()
    assert_close(got, g["finit"], dt, what=f"{name} finit")


@pytest.mark.parametrize("name", OBSTACLES)
def test_obstacle_through_the_python_api_against_the_reference_vectors(name):
    """inlet (its populations come from the Python class), bounce-back block and anti-bounce-back outlet, whose
    neighbour's moments are those AFTER the collision: this equilibrium does not conserve momentum"""
    g = golden(name)
    flow, dt = obstacle_flow(g, name, native(dt=name.split("_")[-1]))
    assert_close(flow.f.cpu().numpy(), g["f0"], dt, what=f"{name} f0")
    sim = lt.Simulation(flow, lt.BGKCollision(flow.units.relaxation_parameter_lu), [])
    assert sim._native is not None
    done = 0
    for n in (1, 2, 3, 10):
        sim(n - done)
        done = n
        assert_close(flow.f.cpu().numpy(), g[f"f{n}"], dt, n, outlet=True, what=f"{name} f{n}")
    assert ", 17," in sim._native.plan.kernel_name(), sim._native.plan.kernel_name()


# --------------------------------------------------------------------------- the Python API on a native context
@pytest.mark.parametrize("name", FIXTURES + [LESS_MEMORY])
def test_flow_collision_and_simulation_through_the_python_api(name):
    """Flow construction (Flow.initialize and initialize_f_neq reach the plan's equilibrium), equilibrium(flow),
    collision(flow) and Simulation, against the reference's vectors"""
    g = golden(name)
    dt = name.split("_")[-1]
    flow, operator, _ = fixture_flow(g, name, context=native(dt))
    assert flow.f.is_cuda and flow._engine_plan(flow.f) is not None
    assert_close(flow.f.cpu().numpy(), g["finit"], dt, what=f"{name} finit")
    flow.f = dev(torch.tensor(g["f0"]))
    assert_close(flow.equilibrium(flow).cpu().numpy(), g["feq"], dt, what=f"{name} feq")
    collision = make_collision(g, operator, flow)
    assert_close(collision(flow).cpu().numpy(), g["collided"], dt, what=f"{name} collided")
    assert flow._collision_plans, "collision(flow) did not go through the engine"
    sim = lt.Simulation(flow, collision, [])
    done = 0
    for n in (1, 2, 3, 10):
        sim(n - done)
        done = n
        assert_close(flow.f.cpu().numpy(), g[f"f{n}"], dt, n, what=f"{name} f{n}")


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_a_change_of_rho0_between_two_batches_restarts_from_flow_f(dt):
    """rho0 is read per batch and is part of the carry key: 3 steps at 1.1, then 2 at 1.0, as the torch path does it"""
    g = golden(f"incompressible_bgk_d3q19_{dt}")
    flows = []
    for context in (native(dt), lt.Context("cpu", torch.float64, use_native=False)):
        flow = fixture_flow(g, f"incompressible_bgk_d3q19_{dt}", context=context)[0]
        flow.f = context.convert_to_tensor(torch.tensor(g["f0"]), dtype=context.dtype)
        sim = lt.Simulation(flow, lt.BGKCollision(float(g["tau"])), [])
        sim(3)
        if context.use_native:
            kept = sim._native.kept                   # something is kept that the next batch could carry on from
            assert kept.phase is Phase.PENDING and kept.valid and kept.resume(kept.key) is not None
        flow.equilibrium.rho0 = 1.0
        sim(2)
        flows.append(flow)
    got, want = flows[0].f.cpu().numpy(), flows[1].f.numpy()
    assert_close(got, want, dt, 5, what=f"3 steps at rho0 1.1 + 2 at 1.0, {dt}")
    assert float(np.abs(want - g["f3"]).max()) > 10 * ATOL["f32"]
    # five steps at 1.1 are something else
    assert float(np.abs(got - cpu_run("bgk", "D3Q19", torch.tensor(g["f0"]), (5,))[1][5]).max()) > 10 * ATOL["f32"]


GRIDS = [("D1Q3", [16]), ("D1Q3", [301]), ("D2Q9", [13, 67]), ("D3Q15", [5, 7, 67]), ("D3Q19", [5, 7, 67]), ("D3Q27", [3, 5, 67])]


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("lat,res", GRIDS, ids=[f"{lat}-{'x'.join(map(str, res))}" for lat, res in GRIDS])
@pytest.mark.parametrize("operator", list(COLL))
def test_small_and_ragged_grids_against_the_cpu_path(operator, lat, res, dt):
    """D1Q3, and extents that are no multiple of a workgroup, a wave or a tile: more than one workgroup, a partial last
    one.  The CPU path runs in float64 from the same (fp32: the same fp32) state."""
    f0 = perturbed_state(lat, res, TORCH_DT[dt], 23)
    want_collided, want = cpu_run(operator, lat, f0, (1, 3))
    plan = make_plan(operator, lat, dt, res)
    got = plan.collide(dev(f0), torch.empty_like(dev(f0)), TAU).cpu().numpy()
    assert_close(got, want_collided, dt, what=f"{operator} {lat} {res} {dt} collided")
    for n in (1, 3):
        assert_close(run(plan, f0, n, TAU), want[n], dt, n, what=f"{operator} {lat} {res} {dt} n = {n}")


@pytest.mark.parametrize("operator", list(COLL))
def test_fused_is_bit_identical_to_stream_then_collide(operator):
    lat, res = "D3Q19", [6, 5, 8]
    plan = make_plan(operator, lat, "f32", res)
    f = dev(perturbed_state(lat, res, torch.float32, 7))
    a, b, c = torch.empty_like(f), torch.empty_like(f), torch.empty_like(f)
    plan.stream(f, a)
    plan.collide(a, b, TAU)
    plan.stream_collide(f, c, TAU)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(c.cpu().numpy(), b.cpu().numpy())


# --------------------------------------------------------------------------- which kernel, how many launches
def test_kernel_name_and_one_update_per_launch_where_the_quadratic_plan_pairs():
    """D3Q19 fp32 on a grid the two-step sweep tiles: the quadratic plan pairs its fused steps when told to, the same
    plan with the incompressible equilibrium keeps one update per launch, says so, and names another kernel"""
    lat, res = "D3Q19", [6, 24, 192]
    f0 = perturbed_state(lat, res, torch.float32, 3)
    plan = make_plan("bgk", lat, "f32", res, equilibrium=None)
    plan.set_two_step(1)
    quadratic_name = plan.kernel_name()
    assert quadratic_name.startswith("lbm2_kernel<float, lt::d3q19, 0, 1,") and plan.two_step_admitted() is None
    run(plan, f0, 9, TAU)
    assert plan.last_run_info() == {"single_step_launches": 0, "two_step_launches": 4, "many_step_launches": 0}
    plan.set_equilibrium("incompressible", RHO0)
    name = plan.kernel_name()
    assert name != quadratic_name and name.startswith("lbm_kernel<float, lt::d3q19, 0, 17,"), name
    why = plan.two_step_admitted()
    assert why is not None and "incompressible equilibrium" in why, why
    assert plan.resident_enabled()[0] is False
    got = run(plan, f0, 9, TAU)
    assert plan.last_run_info() == {"single_step_launches": 8, "two_step_launches": 0, "many_step_launches": 0}
    fresh = make_plan("bgk", lat, "f32", res)                     # a plan that never knew the two-step switch
    assert fresh.kernel_name() == name
    np.testing.assert_array_equal(got, run(fresh, f0, 9, TAU))
    assert_close(got, cpu_run("bgk", lat, f0, (9,))[1][9], "f32", 9, what="9 steps, one update per launch")
    # ... and back: kind 0 launches what the plan launched before
    plan.set_equilibrium("quadratic")
    assert plan.kernel_name() == quadratic_name and plan.two_step_admitted() is None


def test_a_plan_that_set_kind_zero_is_a_plan_that_never_called_the_setter():
    for lat, dt, res, operator in (("D3Q19", "f32", [6, 5, 8], "bgk"), ("D2Q9", "f64", [12, 10], "trt"),
                                   ("D3Q27", "f32", [4, 6, 5], "guo")):
        f0 = perturbed_state(lat, res, TORCH_DT[dt], 5)
        never = make_plan(operator, lat, dt, res, equilibrium=None)
        zero = make_plan(operator, lat, dt, res, equilibrium="quadratic", rho0=1.1)     # rho0 is not read
        back = make_plan(operator, lat, dt, res)
        back.set_equilibrium("quadratic")
        assert never.kernel_name() == zero.kernel_name() == back.kernel_name()
        want = run(never, f0, 4, TAU)
        np.testing.assert_array_equal(run(zero, f0, 4, TAU), want)
        np.testing.assert_array_equal(run(back, f0, 4, TAU), want)
        a = dev(f0)
        want = never.collide(a, torch.empty_like(a), TAU).cpu().numpy()
        np.testing.assert_array_equal(zero.collide(a, torch.empty_like(a), TAU).cpu().numpy(), want)
        rho, u = never.macroscopic(a)
        np.testing.assert_array_equal(zero.equilibrium(rho, u).cpu().numpy(), never.equilibrium(rho, u).cpu().numpy())


# --------------------------------------------------------------------------- refusals
def _refused(call, code, *words):
    from lettuce_amd._native import NativeEngineError
    with pytest.raises(NativeEngineError) as info:
        call()
    assert info.value.code == code, (info.value.code, str(info.value))
    for word in words:
        assert word in str(info.value), str(info.value)


def test_refusals_leave_the_plan_as_it_was():
    from lettuce_amd._native import Plan, LAYOUT_SLAB
    lat, res = "D2Q9", [16, 24]
    f0 = dev(perturbed_state(lat, res, torch.float64, 9))

    def collided(plan, tau=TAU):
        return plan.collide(f0, torch.empty_like(f0), tau).cpu().numpy()

    # LT_ERR_INVALID: an unknown kind, a non-finite rho0 -- on a quadratic and on an incompressible plan
    for equilibrium in (None, "incompressible"):
        plan = make_plan("bgk", lat, "f64", res, equilibrium=equilibrium)
        name, before = plan.kernel_name(), collided(plan)
        for kind in (2, -1):
            assert plan.lib.lt_plan_set_equilibrium(plan._handle, kind, 1.0) == 1
            assert b"equilibrium kind" in plan.lib.lt_last_error()
        for rho0 in (float("nan"), float("inf")):
            _refused(lambda: plan.set_equilibrium("incompressible", rho0), 1, "rho0")
        assert plan.kernel_name() == name
        np.testing.assert_array_equal(collided(plan), before)
    # LT_ERR_UNSUPPORTED: the collisions without such kernels
    plans = {"KBC": Plan(lat, torch.float64, "kbc", res), "Smagorinsky": Plan(lat, torch.float64, "smagorinsky", res),
             "forced Smagorinsky": Plan(lat, torch.float64, "smagorinsky", res), "MRT": Plan(lat, torch.float64, "mrt", res)}
    plans["forced Smagorinsky"].set_force([1e-4, 0.0], 0.5, 0.4)
    plans["MRT"].set_mrt("D2Q9Dellar", [1.0, 1.0, 1.0] + [1.3] * 6)
    for what, plan in plans.items():
        name, before = plan.kernel_name(), collided(plan)
        _refused(lambda: plan.set_equilibrium("incompressible", RHO0), 2, "incompressible equilibrium",
                 "MRT" if what == "MRT" else what.split()[-1])
        assert plan.kernel_name() == name
        np.testing.assert_array_equal(collided(plan), before)
    # ... a slab-layout plan, with and without ghost planes
    for ghosts in (0, 1):
        slab = Plan("D3Q19", torch.float32, "bgk", [8, 6, 4], layout=LAYOUT_SLAB, ghost_planes=ghosts)
        name = slab.kernel_name()
        _refused(lambda: slab.set_equilibrium("incompressible", RHO0), 2, "incompressible equilibrium", "slab")
        assert slab.kernel_name() == name
    # ... a plan with a constant-pressure outlet
    entries = [{"kind": "pressure_outlet", "axis": 0, "side": 1, "rho_outlet": 1.0}]
    outlet = Plan(lat, torch.float64, "bgk", res, entries)
    _refused(lambda: outlet.set_equilibrium("incompressible", RHO0), 2, "incompressible equilibrium", "constant-pressure outlet")
    outlet.set_equilibrium("quadratic")                              # kind 0 is always taken
    # a kind-1 plan: no launch of several steps, by name
    plan = make_plan("bgk", lat, "f64", [16, 64])
    f = dev(perturbed_state(lat, [16, 64], torch.float64, 9))
    name = plan.kernel_name()
    _refused(lambda: plan.set_two_step(1), 2, "two steps per launch", "incompressible equilibrium")
    _refused(lambda: plan.set_many_step(1), 2, "several steps per launch", "incompressible equilibrium")
    _refused(lambda: plan.stream_collide_twice(f, torch.empty_like(f), TAU), 2, "incompressible equilibrium")
    _refused(lambda: plan.stream_collide_many(f, torch.empty_like(f), TAU, 4), 2, "incompressible equilibrium")
    plan.set_two_step(0); plan.set_two_step(-1); plan.set_many_step(0); plan.set_many_step(-1)
    assert plan.kernel_name() == name
    # the same grid with the quadratic equilibrium has both launches
    plan.set_equilibrium("quadratic")
    plan.set_many_step(1)
    assert plan.kernel_name().startswith("lbm_many_kernel")
    # Simulation names the pair that has no kernel (the texts without a device: test_equilibria_host.py)
    flow = lt.TaylorGreenVortex(native("f32"), [8, 8], 100, 0.05, lt.D2Q9(), lt.IncompressibleQuadraticEquilibrium(RHO0))
    with pytest.raises(lt.NativeEngineError, match="equilibrium 'IncompressibleQuadraticEquilibrium' with collision 'KBCCollision'"):
        lt.Simulation(flow, lt.KBCCollision(), [])


# --------------------------------------------------------------------------- the other equilibria
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_less_memory_runs_the_quadratic_kernels(dt):
    """bit for bit what QuadraticEquilibrium gives on the engine, and within the bounds of its own fixture"""
    g = golden(LESS_MEMORY)
    results = []
    for equilibrium in (lt.QuadraticEquilibriumLessMemory(), lt.QuadraticEquilibrium()):
        flow = fixture_flow(g, LESS_MEMORY, equilibrium, native(dt))[0]
        out = [flow.f.clone()]
        flow.f = dev(torch.tensor(g["f0"]).to(TORCH_DT[dt]))
        out += [flow.equilibrium(flow), lt.BGKCollision(float(g["tau"]))(flow)]
        sim = lt.Simulation(flow, lt.BGKCollision(float(g["tau"])), [])
        assert ", 0, 1," in sim._native.plan.kernel_name()
        sim(10)
        results.append([t.cpu().numpy() for t in out + [flow.f]])
    for a, b in zip(*results):
        np.testing.assert_array_equal(a, b)
    for got, key in zip(results[0], ("finit", "feq", "collided", "f10")):
        assert_close(got, g[key], dt, what=f"{LESS_MEMORY} as {dt}: {key}")


class Scaled(lt.Equilibrium):
    """an equilibrium of the caller's: 1.01 times the quadratic one"""

    def __call__(self, flow, rho=None, u=None):
        return 1.01 * lt.QuadraticEquilibrium()(flow, rho, u)

    def native_available(self):
        return False

    def native_generator(self):
        return None


@pytest.mark.parametrize("lat,res", [("D2Q9", [12, 10]), ("D3Q19", [6, 5, 8])])
def test_an_equilibrium_of_the_callers_is_not_replaced_by_the_quadratic_kernel(lat, res):
    """BGKCollision(tau)(flow), TRT, the regularised collision and initialize_f_neq(flow) on a native context: the torch
    expressions with the caller's equilibrium, not the engine's quadratic result"""
    results = {}
    for where, context in (("engine", native("f64")), ("cpu", lt.Context("cpu", torch.float64, use_native=False))):
        for equilibrium in (Scaled(), lt.QuadraticEquilibrium()):
            flow = UniformFlow(context, res, 10, 0.05, STENCILS[lat](), equilibrium)
            flow.f = context.convert_to_tensor(perturbed_state(lat, res, torch.float64, 31))
            out = {"bgk": lt.BGKCollision(0.8)(flow), "trt": lt.TRTCollision(0.8, 1.4)(flow),
                   "regularized": lt.RegularizedCollision()(flow), "fneq": lt.initialize_f_neq(flow)}
            results[where, type(equilibrium).__name__] = {k: v.cpu().numpy() for k, v in out.items()}
    for key in ("bgk", "trt", "regularized", "fneq"):
        got, want = results["engine", "Scaled"][key], results["cpu", "Scaled"][key]
        assert_close(got, want, "f64", what=f"{key} with the caller's equilibrium")
        gap = float(np.abs(got - results["engine", "QuadraticEquilibrium"][key]).max())
        print(f"{key}: distance from the engine's quadratic result {gap:.2e}")
        assert gap > 10 * ATOL["f32"]
    # Simulation refuses it by name
    flow = UniformFlow(native("f64"), res, 10, 0.05, STENCILS[lat](), Scaled())
    with pytest.raises(lt.NativeEngineError, match="equilibrium 'Scaled'"):
        lt.Simulation(flow, lt.BGKCollision(0.8), [])
