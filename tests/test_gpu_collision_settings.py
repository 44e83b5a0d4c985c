"""The per-batch settings of a collision on the engine: which ``Plan.set_*`` calls ``lt.Simulation`` makes per batch and
``collision(flow)`` per call, in which order and with which arguments, and the carry-key contract of the stepper -- a
batch after a changed setting starts again from ``flow.f`` on the same plan, a batch after an unchanged one carries on.

The plan's four collision setters and ``set_equilibrium`` are wrapped with recorders that log and delegate; the launch
counts come from ``plan.last_run_info()`` (fused stream-collide launches; the collide pass of a batch that starts from
``flow.f`` is not among them).  Nothing here compares populations with a reference: the operators' own test files do."""
import warnings

import pytest
import torch

import lettuce_amd as lt
from lettuce_amd import moments
from lettuce_amd._native import Plan

pytestmark = pytest.mark.gpu

SETTERS = ("set_smagorinsky", "set_trt", "set_mrt", "set_force", "set_equilibrium")
QUADRATIC = ("set_equilibrium", ("quadratic", 1.0))
TAU, FORCE_TAU = 0.8, 0.6
ACCELERATION = (1e-3, -2e-3)
GUO = (0.5, 1 - 1 / (2 * FORCE_TAU))        # ueq_scale, source_scale
RATES = [1.0, 1.0, 1.0, 0.7, 0.7, 0.7, 1.05, 1.1, 1.15]
GRIDS = {"d2q9": (lt.D2Q9, [16, 16], torch.float64), "d3q19": (lt.D3Q19, [8, 8, 8], torch.float32)}
# the launch paths of a batch: the caller's dense tensors, the engine's resident populations; one fused step per launch
PATHS = {"dense": 0, "resident": 1}


@pytest.fixture
def calls(monkeypatch):
    """[(plan, setter, positional arguments)] of every call from here on, construction included"""
    log = []
    for name in SETTERS:
        def recorder(self, *args, _name=name, _original=getattr(Plan, name)):
            log.append((self, _name, args))
            return _original(self, *args)
        monkeypatch.setattr(Plan, name, recorder)
    return log


def taken(log, plan):
    """the calls on ``plan`` since the last look (the flow's moment plan gets its equilibrium too: not meant here)"""
    mine = [(name, args) for p, name, args in log if p is plan]
    log.clear()
    return mine


def native_flow(grid="d2q9"):
    stencil, res, dtype = GRIDS[grid]
    context = lt.Context("cuda:0", dtype, use_native=True)
    return lt.TaylorGreenVortex(context, res, 100, 0.05, stencil())


def mrt_collision(flow):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                     # the D2Q9 transforms say that they are experimental
        return lt.MRTCollision(moments.D2Q9Dellar(flow.stencil, flow.context), RATES, flow.context)


def guo(flow, acceleration=ACCELERATION):
    return lt.Guo(flow, FORCE_TAU, list(acceleration))


def rates_of(collision):
    return tuple(float(s) for s in collision.relaxation_parameters.tolist())


def acceleration_of(collision):
    return tuple(float(a) for a in collision.force.acceleration.tolist())


def set_rate(collision):
    collision.relaxation_parameters[3] = 0.9


def set_acceleration(collision):
    collision.force.acceleration = collision.force.acceleration * 2


# name -> (collision of a flow, its setter calls now, a change of one setting or of tau, or None)
SIMULATION_CASES = {
    "bgk": (lambda flow: lt.BGKCollision(TAU), lambda c: [], lambda c: setattr(c, "tau", 0.9)),
    "kbc": (lambda flow: lt.KBCCollision(), lambda c: [], None),
    "regularized": (lambda flow: lt.RegularizedCollision(), lambda c: [], lambda c: setattr(c, "tau", 0.9)),
    "none": (lambda flow: lt.NoCollision(), lambda c: [], None),
    "bgk-guo": (lambda flow: lt.BGKCollision(TAU, force=guo(flow)),
                lambda c: [("set_force", (acceleration_of(c), *GUO))], set_acceleration),
    "smagorinsky": (lambda flow: lt.SmagorinskyCollision(TAU, 0.2),
                    lambda c: [("set_smagorinsky", (c.constant,))], lambda c: setattr(c, "constant", 0.3)),
    "trt": (lambda flow: lt.TRTCollision(TAU, 1.4),
            lambda c: [("set_trt", (c.tau_minus,))], lambda c: setattr(c, "tau_minus", 1.1)),
    "mrt": (mrt_collision, lambda c: [("set_mrt", ("D2Q9Dellar", rates_of(c)))], set_rate),
}
RUNS = [(name, "d2q9", "dense") for name in SIMULATION_CASES] + [("smagorinsky", "d2q9", "resident"),
                                                                 ("trt", "d3q19", "resident"), ("trt", "d3q19", "dense")]


@pytest.mark.parametrize("name,grid,path", RUNS, ids=["-".join(r) for r in RUNS])
def test_simulation_hands_the_settings_over_once_per_batch_and_keys_the_carry_on_them(calls, name, grid, path):
    make, expected, change = SIMULATION_CASES[name]
    flow = native_flow(grid)
    collision = make(flow)
    sim = lt.Simulation(flow, collision, [])
    plan = sim._native.plan
    assert taken(calls, plan) == []                         # the quadratic equilibrium is the plan's own default
    plan.set_resident(PATHS[path])
    plan.set_many_step(0)
    plan.set_two_step(0)

    def batch(fused):
        sim(2)
        got, info = taken(calls, plan), plan.last_run_info()
        print(f"{name} {path}: {got} {info}")
        assert got == expected(collision) + [QUADRATIC]
        assert sim._native.plan is plan and plan.resident_enabled()[0] == (path == "resident")
        assert info == {"single_step_launches": fused, "two_step_launches": 0, "many_step_launches": 0}

    batch(1)                # from flow.f: the collide pass and one fused step
    batch(2)                # nothing changed and nobody looked: carries on with two fused steps
    if change is not None:
        before = expected(collision)
        change(collision)
        assert expected(collision) != before or not before
        batch(1)            # the same plan with the new value, and from flow.f again
        batch(2)


# --------------------------------------------------------------------------- collision(flow)
# name -> (collision of a flow, its plan's kind, the calls of one collision(flow))
def forced_calls(collision):
    return ("set_force", (acceleration_of(collision), collision.force.ueq_scaling_factor,
                          GUO[1] if isinstance(collision.force, lt.Guo) else 0.0))


UNFORCED = ("set_force", (None,))
CALL_CASES = {
    "bgk": (lambda flow: lt.BGKCollision(TAU), "bgk", lambda c: [QUADRATIC, UNFORCED]),
    "bgk-guo": (lambda flow: lt.BGKCollision(TAU, force=guo(flow)), "bgk", lambda c: [QUADRATIC, forced_calls(c)]),
    "smagorinsky": (lambda flow: lt.SmagorinskyCollision(TAU, 0.2), "smagorinsky",
                    lambda c: [QUADRATIC, ("set_smagorinsky", (0.2,)), UNFORCED]),
    "smagorinsky-shan-chen": (lambda flow: lt.SmagorinskyCollision(TAU, 0.2, force=lt.ShanChen(flow, 0.7, list(ACCELERATION))),
                              "smagorinsky", lambda c: [QUADRATIC, ("set_smagorinsky", (0.2,)), forced_calls(c)]),
    "trt": (lambda flow: lt.TRTCollision(TAU, 1.4), "trt", lambda c: [QUADRATIC, ("set_trt", (1.4,))]),
    "kbc": (lambda flow: lt.KBCCollision(), "kbc", lambda c: [QUADRATIC]),
    "regularized": (lambda flow: lt.RegularizedCollision(), "regularized", lambda c: [QUADRATIC]),
    "mrt": (mrt_collision, "mrt", lambda c: [("set_mrt", ("D2Q9Dellar", rates_of(c)))]),
}


@pytest.mark.parametrize("name", CALL_CASES)
def test_collision_of_a_flow_hands_the_settings_to_the_kinds_plan_before_every_call(calls, name):
    make, kind, expected = CALL_CASES[name]
    flow = native_flow()
    collision = make(flow)
    for _ in range(2):
        out = collision(flow)
        assert set(flow._collision_plans) == {kind}
        got = taken(calls, flow._collision_plans[kind])
        print(f"{name}: {got}")
        assert got == expected(collision)                   # set_equilibrium first where the collision evaluates feq
        assert out.shape == flow.f.shape and out.data_ptr() != flow.f.data_ptr()
    if name in ("kbc", "regularized"):
        assert collision.tau == flow.units.relaxation_parameter_lu     # fixed at the first call, before it was used


@pytest.mark.parametrize("kind", ["bgk", "smagorinsky"])
def test_collisions_with_and_without_a_force_share_the_kinds_plan_and_do_not_leak_the_force(calls, kind):
    flow = native_flow()

    def make(flow, force):
        return lt.BGKCollision(TAU, force=force) if kind == "bgk" else lt.SmagorinskyCollision(TAU, 0.2, force=force)

    plain, forced = make(flow, None), make(flow, guo(flow))
    results = [collision(flow).clone() for collision in (plain, forced, plain, forced)]
    assert set(flow._collision_plans) == {kind}
    forces = [args for name, args in taken(calls, flow._collision_plans[kind]) if name == "set_force"]
    assert forces == [(None,), (ACCELERATION, *GUO), (None,), (ACCELERATION, *GUO)]
    assert torch.equal(results[0], results[2]) and torch.equal(results[1], results[3])
    assert not torch.equal(results[0], results[1])
    # each is what a flow gives that never saw the other
    for collision_of, want in ((lambda f: make(f, None), results[0]), (lambda f: make(f, guo(f)), results[1])):
        fresh = native_flow()
        assert torch.equal(collision_of(fresh)(fresh), want)
