"""The kept-state record (lettuce_amd/_kept.py) by itself, with CPU tensors and a recording completion / release --
every phase x every operation -- and the slab drivers on it: one rank, the oracle-backed engine, a list of events (a
look, an assignment, an in-place edit, a changed tau) against a twin that never carries on."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__))))

from lettuce_amd._kept import KeptState, Phase  # noqa: E402

KEY, OTHER_KEY = (0.8, "settings", ("quadratic", 1.0)), (0.9, "settings", ("quadratic", 1.0))
PHASES = list(Phase)
ENGINE = [False, True]


class Pass:
    """a deferred pass: f* and scratch (or the engine's buffers), a completion and a release that count their calls"""

    def __init__(self, engine=False):
        self.fstar, self.scratch = torch.zeros(3), torch.ones(3)
        self.where = KeptState.ENGINE if engine else (self.fstar, self.scratch)
        self.completed = self.released = 0

    def complete(self):
        self.completed += 1
        return self.scratch, self.fstar                     # f, f_next

    def release(self):
        self.released += 1


def kept_in(phase, engine=False):
    """(record in ``phase``, its pass, the (f, f_next) that were shown or None)"""
    kept, owed, shown = KeptState(), Pass(engine), None
    if phase is not Phase.NOTHING:
        kept.defer(owed.where, KEY, owed.complete, owed.release)
    if phase is Phase.SHOWN:
        shown = kept.present()
    assert kept.phase is phase
    return kept, owed, shown


OPERATIONS = {
    "defer": lambda kept: kept.defer((torch.zeros(2), torch.zeros(2)), KEY, lambda: None),
    "present": lambda kept: kept.present(),
    "resume": lambda kept: kept.resume(KEY),
    "drop": lambda kept: kept.drop(),
    "invalidate": lambda kept: kept.invalidate(),
}
AFTER = {"defer": lambda phase: Phase.PENDING, "present": lambda phase: Phase.SHOWN, "resume": lambda phase: phase,
         "drop": lambda phase: Phase.NOTHING, "invalidate": lambda phase: phase}


@pytest.mark.parametrize("engine", ENGINE, ids=["tensors", "engine"])
@pytest.mark.parametrize("operation", list(OPERATIONS))
@pytest.mark.parametrize("phase", PHASES, ids=[p.name for p in PHASES])
def test_phase_completion_and_release_after_every_operation_in_every_phase(phase, operation, engine):
    kept, owed, _ = kept_in(phase, engine)
    completed = owed.completed
    if operation == "present" and phase is not Phase.PENDING:
        with pytest.raises(AssertionError):                 # there is no pass to run: nobody may ask for one
            kept.present()
        assert kept.phase is phase
    else:
        OPERATIONS[operation](kept)
        assert kept.phase is AFTER[operation](phase)
    # the completion runs exactly once, when somebody looks; the release on a drop from pending and never otherwise
    assert owed.completed == completed + (operation == "present" and phase is Phase.PENDING)
    assert completed == (phase is Phase.SHOWN)
    assert owed.released == (operation == "drop" and phase is Phase.PENDING)


@pytest.mark.parametrize("engine", ENGINE, ids=["tensors", "engine"])
def test_resume_while_pending(engine):
    kept, owed, _ = kept_in(Phase.PENDING, engine)
    assert kept.resume(KEY) is owed.where                   # equal key, nothing touched
    assert kept.resume(KEY, (torch.zeros(3), torch.ones(3))) is owed.where    # nobody can reach f*: ``now`` is not asked
    assert kept.resume(OTHER_KEY) is None and kept.resume(None) is None
    assert kept.resume(KEY) is owed.where                   # asking changes nothing
    if not engine:
        owed.scratch.add_(0)                                # an edited witness, values unchanged
        assert kept.resume(KEY) is None
    assert owed.completed == 0 and owed.released == 0


def test_resume_once_shown_with_two_tensors():
    kept, owed, (f, f_next) = kept_in(Phase.SHOWN)
    assert f is owed.scratch and f_next is owed.fstar
    assert kept.resume(KEY, (f, f_next)) is owed.where      # f* is still in f_next: (f*, scratch) = (f_next, f)
    assert kept.resume(OTHER_KEY, (f, f_next)) is None
    assert kept.resume(KEY) is None and kept.resume(KEY, (f,)) is None        # nothing stands where the witness stood
    assert kept.resume(KEY, (f.clone(), f_next)) is None    # a replaced witness
    assert kept.resume(KEY, (f, f_next.clone())) is None
    assert kept.resume(KEY, (f_next, f)) is None
    assert kept.resume(KEY, (f, f_next)) is owed.where
    f_next.mul_(1)                                          # an edited witness
    assert kept.resume(KEY, (f, f_next)) is None
    assert owed.completed == 1 and owed.released == 0


def test_resume_once_shown_with_the_populations_in_the_engine():
    kept, owed, (f, f_next) = kept_in(Phase.SHOWN, engine=True)
    assert kept.resume(KEY, (f,)) == KeptState.ENGINE and kept.resume(KEY, (f,)) is not None
    assert kept.resume(OTHER_KEY, (f,)) is None and kept.resume(KEY) is None
    # the other buffer is scratch space: replaced or edited, the engine still holds what f shows
    f_next.mul_(1)
    assert kept.resume(KEY, (f, torch.empty(3))) is not None and kept.resume(KEY, (f, f_next)) is not None
    assert kept.resume(KEY, (f.clone(),)) is None
    f.mul_(1)
    assert kept.resume(KEY, (f,)) is None


def test_nothing_kept_resumes_nothing():
    kept = KeptState()
    assert kept.resume(None) is None and kept.resume(KEY, (torch.zeros(3), torch.zeros(3))) is None
    kept, owed, _ = kept_in(Phase.PENDING)
    kept.drop()
    assert kept.resume(KEY) is None and kept.resume(KEY, owed.where) is None


@pytest.mark.parametrize("engine", ENGINE, ids=["tensors", "engine"])
@pytest.mark.parametrize("phase", PHASES, ids=[p.name for p in PHASES])
def test_invalidate_holds_until_the_next_batch_whether_or_not_somebody_looks(phase, engine):
    kept, owed, shown = kept_in(phase, engine)
    kept.invalidate()
    assert kept.phase is phase and kept.resume(KEY) is None
    if phase is Phase.PENDING:
        shown = kept.present()                              # the pass is still owed to whoever looks ...
        assert owed.completed == 1 and shown[0] is owed.scratch
    if shown is not None:
        assert kept.resume(KEY, shown) is None              # ... and the look does not bring the carry back
    again = Pass(engine)
    kept.defer(again.where, KEY, again.complete, again.release)     # the batch that started from f
    assert kept.resume(KEY) is again.where
    assert owed.released == 0 and again.completed == 0


def test_the_key_of_the_slab_drivers_is_none():
    kept, owed = KeptState(), Pass()
    kept.defer(owed.where, None, owed.complete)
    assert kept.resume(None) is owed.where and kept.resume(KEY) is None
    assert kept.resume(None, kept.present()) is owed.where
    kept.drop()                                             # from shown: nothing to release (and no release given)
    assert kept.phase is Phase.NOTHING


# --------------------------------------------------------------------------- the slab drivers on the record
RESOLUTION = [6, 4, 5]
DRIVERS = [("SlabSimulation", {}), ("TwoStepSlabSimulation", {"direct": True}), ("TwoStepSlabSimulation", {"direct": False})]


class Counting:
    """the oracle-backed engine with its ``collide_planes`` calls counted"""

    def __init__(self, inner):
        self.__dict__["inner"], self.__dict__["collides"] = inner, 0

    def __getattr__(self, name):
        return getattr(self.inner, name)

    def __setattr__(self, name, value):
        setattr(self.inner, name, value)

    def collide_planes(self, *args):
        self.__dict__["collides"] += 1
        return self.inner.collide_planes(*args)


def planewise_engine():
    """The oracle-backed engine, colliding plane by plane.  The oracle's momentum is a matrix product, whose last bit
    depends on how many nodes share the call (one plane in an edge launch, all planes in ``collide_planes``); a plane
    collided by itself, from a fresh copy, gives the same bits in whichever launch it falls -- as a node does on the
    GPU -- and only then can a run that carries on equal one that starts from ``f`` bit for bit."""
    from slab_cpu_engine import OracleSlabEngine

    class Planewise(OracleSlabEngine):
        def _collide(self, f, tau):
            collide = super()._collide
            return torch.cat([collide(f[:, z:z + 1].clone(), tau) for z in range(f.shape[1])], dim=1)
    return Planewise("D3Q19", torch.float64, "bgk")


def slab_simulation(driver, kwargs):
    import lettuce_amd as lt
    ctx = lt.Context("cpu", torch.float64, use_native=False)
    slab = lt.ZSlab(RESOLUTION, rank=0, world_size=1)
    flow = lt.TaylorGreenVortex(ctx, slab.extended_resolution, 100, 0.1, lt.D3Q19(), slab=slab)
    return getattr(lt, driver)(flow, lt.BGKCollision(flow.units.relaxation_parameter_lu), slab,
                               engine=Counting(planewise_engine()), **kwargs)




@pytest.mark.parametrize("driver,kwargs", DRIVERS, ids=["single-step", "two-step-direct", "two-step-edges"])
def test_slab_drivers_against_a_twin_that_never_carries_on(driver, kwargs):
    """Each event is followed by a batch; the twin gets the same events but assigns ``f = f.clone()`` before every
    batch.  ``collide_planes`` runs once per batch that starts from ``f`` and never in one that carries on."""
    sim, twin = slab_simulation(driver, kwargs), slab_simulation(driver, kwargs)
    assert driver != "TwoStepSlabSimulation" or sim._direct_ok() == kwargs["direct"]

    def both(event):
        event(sim)
        event(twin)

    def batch(steps, what, starts_from_f):
        before = sim.engine.collides
        sim(steps)
        twin.f = twin.f.clone()
        twin(steps)
        print(f"{driver} {kwargs} after '{what}': {steps} steps, collide_planes calls {sim.engine.collides - before}")
        assert sim.engine.collides - before == int(starts_from_f), what
        assert sim._kept.phase is Phase.PENDING

    def look(what):
        assert torch.equal(sim.local_f(), twin.local_f()), f"after '{what}': the populations differ from the twin's"
        assert sim._kept.phase is Phase.SHOWN

    batch(2, "construction", True)
    batch(3, "nobody looked", False)
    look("nobody looked")
    batch(2, "a look", False)
    # assignments and edits use other values, so that a batch that carried on from the kept f* would show
    both(lambda s: setattr(s, "f", s.f * 0.999))
    batch(3, "f read and assigned while pending", True)
    kept = [s.local_f().clone() for s in (sim, twin)]
    look("f read and assigned while pending")
    batch(2, "a look", False)
    both(lambda s: setattr(s, "f", torch.full_like(s._f, 0.05)))
    batch(3, "f assigned while pending, unread", True)
    look("f assigned while pending, unread")
    assert not torch.equal(sim.local_f(), kept[0])
    batch(2, "a look", False)
    both(lambda s: setattr(s, "f_next", torch.zeros_like(s._f)))
    batch(3, "f_next assigned while pending", True)
    look("f_next assigned while pending")
    both(lambda s: s.f.mul_(1.001))
    batch(2, "f edited in place while shown", True)
    both(lambda s: s.f.mul_(0.999))
    batch(3, "f edited in place while pending", True)
    look("f edited in place")
    batch(2, "a look", False)
    # a changed tau: the slab drivers carry on across it (the record's key is None), pending or shown
    both(lambda s: setattr(s.collision, "tau", s.collision.tau + 0.05))
    batch(3, "tau changed while pending", False)
    look("tau changed while pending")
    both(lambda s: setattr(s.collision, "tau", s.collision.tau - 0.02))
    batch(2, "tau changed while shown", False)
    look("tau changed while shown")
    assert twin.engine.collides == 13                       # the twin started every batch from f
