"""What a time-step driver keeps between two batches: one record for ``Simulation``'s stepper, ``Flow`` and the slabs."""
import enum


def _version(t):
    return None if t is None else (id(t), t.data_ptr(), t._version, tuple(t.shape))


class Phase(enum.Enum):
    NOTHING = 0     # the next batch starts from ``f``
    PENDING = 1     # f* is held and the pass is not done
    SHOWN = 2       # the pass was done; f* still sits in the other buffer, or in the engine


class KeptState:
    """A batch ends one streaming pass short: the post-collision populations f* of its last step stay where the engine
    left them, the pass runs when somebody looks at ``f``, and the next batch carries on from f* if nothing was touched.
    ``where``: (f*, scratch), the tensors a batch that carries on is launched with, or ``ENGINE``; the pass streams f*
    into scratch, so after it ``f`` is scratch, ``f_next`` is f* and ``where`` stays.  ``key``: what two batches must
    share, (tau, settings, equilibrium) for ``Simulation``; None for the slab drivers, which carry on even when tau or a
    setting changed between two batches -- the last collide of the batch before then ran with the earlier values.
    ``witness``: the tensors whose (id, data_ptr, _version, shape) must be as they were -- f* and scratch while pending,
    ``f`` and ``f_next`` once shown (f* in the engine: ``f`` alone, the other buffer is scratch space).  ``completion``
    runs the pass and returns (f, f_next); ``release`` gives back what an abandoned pass holds, or is None."""
    ENGINE = ()     # ``where`` of populations in the engine's resident buffers: no tensor to launch with or to watch

    def __init__(self):
        self.phase, self.valid = Phase.NOTHING, True
        self.where = self.key = self.witness = self.completion = self.release = None

    def defer(self, where, key, completion, release=None):
        """a batch ended one pass short"""
        self.phase, self.valid = Phase.PENDING, True
        self.where, self.key, self.completion, self.release = where, key, completion, release
        self.witness = tuple(map(_version, where))

    def present(self):
        """somebody looked: run the pass, once, and return (f, f_next)"""
        assert self.phase is Phase.PENDING
        shown, self.completion, self.phase = self.completion(), None, Phase.SHOWN
        self.witness = tuple(map(_version, shown if self.where else shown[:1]))
        return shown

    def resume(self, key, now=()):
        """``where`` if the next batch may carry on from it, else None.  ``now``: the tensors that stand where the
        witness stood (``f``, ``f_next``); not asked while pending -- nobody reaches f* and scratch but through a look"""
        if self.phase is Phase.NOTHING or not self.valid or key != self.key:
            return None
        if self.phase is Phase.PENDING:
            now = self.where
        return self.where if tuple(map(_version, now))[:len(self.witness)] == self.witness else None

    def drop(self):
        """``f`` was assigned: a pending pass is abandoned and what it holds released"""
        release = self.release if self.phase is Phase.PENDING else None
        self.__init__()
        if release is not None:
            release()

    def invalidate(self):
        """masks, boundary parameters or link lists were replaced: the next batch starts from ``f``, whatever the phase
        and whether or not somebody looks before it (a pending pass is still owed to whoever looks)"""
        self.valid = False
