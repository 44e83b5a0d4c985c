"""The per-batch settings of a collision on the host (CPU, no GPU needed): ``CollisionSettings`` -- what
``NativeCollision.settings(flow)`` reads and what ``apply(engine)`` calls -- and ``SlabSimulation`` on one rank with a
stand-in engine that records the setter calls: which are made at construction and which per batch."""
import inspect
import warnings

import pytest
import torch

import lettuce_amd as lt
from lettuce_amd import moments
from lettuce_amd.native_desc import CollisionSettings, NativeCollision, NativeForce
from slab_cpu_engine import OracleSlabEngine
from test_host_api import ctx

GUO_SOURCE = 1 - 1 / (2 * 0.6)            # Guo's source scale at its tau = 0.6
RATES_D2Q9 = [1.0, 1.0, 1.0, 0.7, 0.7, 0.7, 1.05, 1.1, 1.15]


def mrt(transform, stencil, context, rates):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                     # the D2Q9 transforms say that they are experimental
        return lt.MRTCollision(transform(stencil, context), rates, context)


def flow_2d():
    return lt.TaylorGreenVortex(ctx("f64"), [8, 6], 100, 0.05, lt.D2Q9())


def set_rate(collision):
    collision.relaxation_parameters[3] = 0.9


def set_acceleration(collision):
    collision.force.acceleration = collision.force.acceleration * 2


def set_force_tau(collision):
    collision.force.tau = 0.8


# name -> (collision of a flow, the record its attributes give, the changes after which the record differs)
def bgk(flow):
    return lt.BGKCollision(0.8), CollisionSettings(), []


def bgk_guo(flow):
    collision = lt.BGKCollision(0.8, force=lt.Guo(flow, 0.6, [1e-3, 0.0]))
    return collision, CollisionSettings(force=((1e-3, 0.0), 0.5, GUO_SOURCE)), [set_acceleration, set_force_tau]


def smagorinsky_shan_chen(flow):
    collision = lt.SmagorinskyCollision(0.6, 0.2, force=lt.ShanChen(flow, 0.7, [0.0, 2e-3]))
    want = CollisionSettings(smagorinsky=0.2, force=((0.0, 2e-3), 0.7, 0.0))
    return collision, want, [lambda c: setattr(c, "constant", 0.3), set_acceleration, set_force_tau]


def trt(flow):
    return lt.TRTCollision(0.6, 1.4), CollisionSettings(tau_minus=1.4), [lambda c: setattr(c, "tau_minus", 1.1)]


def regularized(flow):
    return lt.RegularizedCollision(), CollisionSettings(), []


def kbc(flow):
    return lt.KBCCollision(), CollisionSettings(), []


def mrt_dellar(flow):
    collision = mrt(moments.D2Q9Dellar, flow.stencil, flow.context, RATES_D2Q9)
    return collision, CollisionSettings(mrt=("D2Q9Dellar", tuple(RATES_D2Q9))), [set_rate]


def no_collision(flow):
    return lt.NoCollision(), CollisionSettings(), []


CASES = [bgk, bgk_guo, smagorinsky_shan_chen, trt, regularized, kbc, mrt_dellar, no_collision]


@pytest.mark.parametrize("case", CASES, ids=[c.__name__ for c in CASES])
def test_the_record_holds_the_values_of_the_collisions_attributes(case):
    flow = flow_2d()
    collision, want, changes = case(flow)
    got = collision.native_generator().settings(flow)
    assert got == want
    for name in ("smagorinsky", "tau_minus", "mrt", "force"):          # the very values, not something close to them
        assert getattr(got, name) == getattr(want, name) and type(getattr(got, name)) is type(getattr(want, name))
    assert hash(got) == hash(want) and len({got, want}) == 1
    assert collision.native_generator().settings(flow) == got          # a second read
    for change in changes:
        before = collision.native_generator().settings(flow)
        change(collision)
        after = collision.native_generator().settings(flow)
        assert after != before and len({before, after}) == 2
    # tau is not part of the record, and reading the record does not fix it: KBC and the regularised collision still
    # take theirs from the flow at the first read of tau
    if case in (regularized, kbc):
        assert collision.tau is None
        assert collision.native_generator().tau(flow) == flow.units.relaxation_parameter_lu


def test_settings_reads_every_callable_once_and_in_order():
    reads = []

    def counting(name, value):
        def read(*args):
            reads.append(name)
            return value
        return read

    force = NativeForce("guo", acceleration=counting("acceleration", (1e-3, 0.0)), ueq_scale=counting("ueq_scale", 0.5),
                        source_scale=counting("source_scale", 0.25))
    desc = NativeCollision("bgk", tau=counting("tau", 0.8), constant=counting("constant", 0.2),
                           tau_minus=counting("tau_minus", 1.4), transform="D2Q9Dellar",
                           rates=counting("rates", list(RATES_D2Q9)), force=force)
    got = desc.settings(None)
    assert reads == ["constant", "tau_minus", "rates", "acceleration", "ueq_scale", "source_scale"]
    assert got == CollisionSettings(0.2, 1.4, ("D2Q9Dellar", tuple(RATES_D2Q9)), ((1e-3, 0.0), 0.5, 0.25))


class Recorder:
    def __init__(self):
        self.log = []

    def set_smagorinsky(self, *args):
        self.log.append(("set_smagorinsky", args))

    def set_trt(self, *args):
        self.log.append(("set_trt", args))

    def set_mrt(self, *args):
        self.log.append(("set_mrt", args))

    def set_force(self, *args):
        self.log.append(("set_force", args))


def test_apply_calls_the_setters_in_one_order_with_the_plans_arguments():
    from lettuce_amd._native import Plan
    force = ((1e-3, 0.0), 0.5, GUO_SOURCE)
    full = CollisionSettings(0.2, 1.4, ("D2Q9Dellar", tuple(RATES_D2Q9)), force)
    engine = Recorder()
    full.apply(engine)
    assert engine.log == [("set_smagorinsky", (0.2,)), ("set_trt", (1.4,)),
                          ("set_mrt", ("D2Q9Dellar", tuple(RATES_D2Q9))), ("set_force", force)]
    assert full.setters == ("set_smagorinsky", "set_trt", "set_mrt", "set_force")
    # the arguments are those of Plan.set_*, by position
    names = {"set_smagorinsky": ["constant"], "set_trt": ["tau_minus"], "set_mrt": ["transform_name", "rates"],
             "set_force": ["acceleration", "ueq_scale", "source_scale"]}
    for setter, args in engine.log:
        bound = inspect.signature(getattr(Plan, setter)).bind(None, *args)
        assert list(bound.arguments)[1:] == names[setter]
    # a value that is None is no call
    for record, setters in ((CollisionSettings(), ()), (CollisionSettings(tau_minus=1.1), ("set_trt",)),
                            (CollisionSettings(smagorinsky=0.2, force=force), ("set_smagorinsky", "set_force"))):
        engine = Recorder()
        record.apply(engine)
        assert tuple(name for name, _ in engine.log) == setters == record.setters


# --------------------------------------------------------------------------- SlabSimulation on one rank
class RecordingSlabEngine(OracleSlabEngine, Recorder):
    """collides as BGK whatever the collision object; the four setters log and do nothing else"""

    def __init__(self, lattice):
        OracleSlabEngine.__init__(self, lattice, torch.float64, "bgk")
        Recorder.__init__(self)

    def taken(self):
        log, self.log = self.log, []
        return log


def slab_flow(stencil):
    slab = lt.ZSlab([8, 4, 6], 0, 1)
    return slab, lt.TaylorGreenVortex(ctx("f64"), slab.extended_resolution, 400, 0.1, stencil(), slab=slab)


def test_slab_driver_hands_smagorinsky_and_force_over_once_per_batch():
    slab, flow = slab_flow(lt.D3Q19)
    collision = lt.SmagorinskyCollision(0.6, 0.2, force=lt.Guo(flow, 0.6, [1e-3, 0.0, 0.0]))
    engine = RecordingSlabEngine("D3Q19")
    sim = lt.SlabSimulation(flow, collision, slab, engine=engine)
    force = ("set_force", ((1e-3, 0.0, 0.0), 0.5, GUO_SOURCE))
    # construction: the force, so that the two-step driver can ask the engine; the constant of the first batch may come too
    assert engine.taken() in ([force], [("set_smagorinsky", (0.2,)), force])
    sim(2)
    assert engine.taken() == [("set_smagorinsky", (0.2,)), force]
    collision.constant = 0.3
    collision.force.acceleration = flow.context.convert_to_tensor([0.0, 2e-3, 0.0])
    sim(3)                                                             # a batch of three steps: one call per setter
    assert engine.taken() == [("set_smagorinsky", (0.3,)), ("set_force", ((0.0, 2e-3, 0.0), 0.5, GUO_SOURCE))]


def test_slab_driver_hands_tau_minus_over_once_per_batch():
    slab, flow = slab_flow(lt.D3Q19)
    collision = lt.TRTCollision(0.6, 1.4)
    engine = RecordingSlabEngine("D3Q19")
    sim = lt.SlabSimulation(flow, collision, slab, engine=engine)
    assert engine.taken() in ([], [("set_trt", (1.4,))])
    sim(2)
    assert engine.taken() == [("set_trt", (1.4,))]
    collision.tau_minus = 1.1
    sim(3)
    assert engine.taken() == [("set_trt", (1.1,))]


def test_slab_driver_sets_nothing_for_bgk():
    slab, flow = slab_flow(lt.D3Q19)
    engine = RecordingSlabEngine("D3Q19")
    sim = lt.SlabSimulation(flow, lt.BGKCollision(0.6), slab, engine=engine)
    sim(2)
    sim(3)
    assert engine.taken() == []


def test_slab_driver_reads_and_hands_over_the_mrt_rates_once_per_batch():
    slab, flow = slab_flow(lt.D3Q27)
    rates = [1.0] * 4 + [0.7] * 6 + [1.05 + 0.05 * k for k in range(17)]
    collision = mrt(moments.D3Q27Hermite, flow.stencil, flow.context, rates)
    reads, read_rates = [], collision._rates

    def counted():
        reads.append(1)
        return read_rates()
    collision._rates = counted                                         # one call is one copy from the device
    engine = RecordingSlabEngine("D3Q27")
    sim = lt.SlabSimulation(flow, collision, slab, engine=engine)
    assert engine.taken() == [("set_mrt", ("D3Q27Hermite", tuple(rates)))] and len(reads) == 1
    sim(2)
    assert engine.taken() == [("set_mrt", ("D3Q27Hermite", tuple(rates)))] and len(reads) == 2
    collision.relaxation_parameters[5] = 0.9
    rates[5] = 0.9
    sim(3)
    assert engine.taken() == [("set_mrt", ("D3Q27Hermite", tuple(rates)))] and len(reads) == 3


def engine_without(setter):
    """a stand-in with three of the four setters (construction refuses it before it is asked for anything else)"""
    methods = {name: getattr(Recorder, name) for name in ("set_smagorinsky", "set_trt", "set_mrt", "set_force")
               if name != setter}
    return type("Engine", (), dict(methods, log=[]))()


@pytest.mark.parametrize("setter,message", [("set_smagorinsky", "engine Engine has no smagorinsky collision"),
                                            ("set_trt", "engine Engine has no trt collision"),
                                            ("set_mrt", "engine Engine has no mrt collision"),
                                            ("set_force", "engine Engine has no body force")])
def test_slab_driver_refuses_an_engine_that_lacks_a_setter(setter, message):
    stencil = lt.D3Q27 if setter == "set_mrt" else lt.D3Q19
    slab, flow = slab_flow(stencil)
    if setter == "set_trt":
        collision = lt.TRTCollision(0.6, 1.4)
    elif setter == "set_mrt":
        collision = mrt(moments.D3Q27Hermite, flow.stencil, flow.context, [1.0] * 27)
    else:
        collision = lt.SmagorinskyCollision(0.6, 0.2, force=lt.Guo(flow, 0.6, [1e-3, 0.0, 0.0]))
    with pytest.raises(lt.LettuceException, match=message):
        lt.SlabSimulation(flow, collision, slab, engine=engine_without(setter))
