"""Call traces of the single-GPU stepper: which ``Plan`` calls ``lt.Simulation`` issues for a script of events (a look,
an assignment, an in-place edit, a changed setting between two batches), in which order and on which buffers.  Test
infrastructure for ``test_gpu_stepper_call_trace.py``, modelled on ``slab_schedule_trace.py``.

A case builds one simulation (D2Q9, [16, 8], fp64, BGK; one step per launch) on the caller's dense tensors or on the
engine's resident populations, records every call of its plan from then on and plays a script; every event of a script
is followed by a batch of two steps.  Every call is one line:

    <method> <arguments> [-> <result>] [| <last_run_info>]

Tensor arguments appear as the role of their buffer (resolved through ``data_ptr``): ``f`` / ``f_next`` are the flow's two
buffers as they were when the trace began, ``f_clone`` / ``f_next_new`` what the script assigned later; the trace keeps
every named tensor alive, so that no later allocation can take a named address.  After ``run`` and ``resident_advance``
the line ends with the launch counts of ``plan.last_run_info()``.  Lines that begin with ``#`` name the event.

A twin simulation receives the same events but assigns ``flow.f = flow.f.clone()`` before every batch, so it never
carries on from kept state; after every look the populations of the two are compared with ``torch.equal``.

The fixtures under ``stepper_call_traces/`` are recorded output: ``python tests/stepper_call_trace.py`` rewrites them,
which is only right at a commit whose launches are the intended ones.
"""
import contextlib
import io
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FIXTURES = os.path.join(ROOT, "tests", "stepper_call_traces")
RESOLUTION = [16, 8]
TAU, OTHER_TAU = 0.8, 0.9
K = 2
PATHS = {"dense": 0, "resident": 1}
# name -> (script, launch path)
CASES = {"events-dense": ("events", "dense"), "events-resident": ("events", "resident"),
         "masks-dense": ("masks", "dense"), "masks-resident": ("masks_shown", "resident")}
_TRACED = ("run", "stream", "resident_load", "resident_advance", "resident_store", "resident_free", "set_masks",
           "update_boundary", "set_links")


class Trace:
    """records the calls of one plan; ``Plan``'s methods are patched for the length of ``patched()``"""

    def __init__(self, plan):
        self.plan, self.lines, self.named, self.depth = plan, [], {}, 0

    def name(self, tensor, role):
        self.named[tensor.data_ptr()] = (role, tensor)

    def _show(self, value):
        if torch.is_tensor(value):
            return self.named.get(value.data_ptr(), ("other",))[0]
        if value is None:
            return "-"
        if isinstance(value, float):
            return f"{value:.6g}"
        if isinstance(value, dict):
            return "{" + " ".join(f"{k}={self._show(v)}" for k, v in sorted(value.items())) + "}"
        if isinstance(value, (list, tuple)):
            return "(" + " ".join(self._show(v) for v in value) + ")"
        return str(value)

    def note(self, text):
        self.lines.append("# " + text)

    def calls(self, since=0):
        """the method names of the recorded calls from line ``since`` on"""
        return [line.split()[0] for line in self.lines[since:] if not line.startswith("#")]

    @contextlib.contextmanager
    def patched(self):
        from lettuce_amd._native import Plan
        trace, undo = self, []
        names = [n for n in vars(Plan) if n in _TRACED or n.startswith("set_")]

        def traced(name, original):
            def call(plan, *args, **kwargs):
                if plan is not trace.plan or trace.depth:
                    return original(plan, *args, **kwargs)
                trace.depth += 1
                try:
                    out = original(plan, *args, **kwargs)
                finally:
                    trace.depth -= 1
                parts = [name] + [trace._show(a) for a in args]
                parts += [f"{k}={trace._show(v)}" for k, v in sorted(kwargs.items())]
                if name in ("run", "stream", "resident_store"):
                    parts.append("-> " + trace._show(out))
                if name in ("run", "resident_advance"):
                    parts.append("| " + trace._show(plan.last_run_info()))
                trace.lines.append(" ".join(parts))
                return out
            return call
        for name in sorted(names):
            undo.append((name, vars(Plan)[name]))
            setattr(Plan, name, traced(name, getattr(Plan, name)))
        try:
            yield
        finally:
            for name, old in undo:
                setattr(Plan, name, old)


def _simulation(lt, with_block):
    context = lt.Context("cuda:0", torch.float64, use_native=True)
    if not with_block:
        flow = lt.TaylorGreenVortex(context, RESOLUTION, 100, 0.05, lt.D2Q9())
    else:
        block = torch.zeros(RESOLUTION, dtype=torch.bool)
        block[5:8, 2:5] = True

        class WithBlock(lt.TaylorGreenVortex):
            @property
            def boundaries(self):
                return [lt.BounceBackBoundary(block)]
        flow = WithBlock(context, RESOLUTION, 100, 0.05, lt.D2Q9())
    sim = lt.Simulation(flow, lt.BGKCollision(TAU), [])
    return sim


class Pair:
    """the traced simulation and its twin, which never carries on"""

    def __init__(self, lt, script, path):
        self.lt = lt
        with_block = script.startswith("masks")
        self.sim, self.twin = _simulation(lt, with_block), _simulation(lt, with_block)
        for s in (self.sim, self.twin):
            s._native.plan.set_two_step(0)
            s._native.plan.set_many_step(0)
            s._native.plan.set_resident(PATHS[path])
        self.trace = Trace(self.sim._native.plan)
        self.trace.name(self.sim.flow.f, "f")
        self.trace.name(self.sim.flow.f_next, "f_next")

    def both(self, action):
        for s in (self.sim, self.twin):
            action(s)

    def batch(self, k=K):
        self.trace.note(f"batch {k}")
        self.sim(k)
        self.twin.flow.f = self.twin.flow.f.clone()
        self.twin(k)

    def look(self):
        self.trace.note("look")
        mine, other = self.sim.flow.f, self.twin.flow.f
        assert torch.equal(mine, other), "the populations differ from the twin's, which never carries on"
        return mine


def _events(p):
    t, lt = p.trace, p.lt
    t.note("1 a first batch")
    p.batch()
    t.note("2 nobody looked")
    p.batch()
    t.note("3 flow.f was read")
    p.look()
    p.batch()
    t.note("4 flow.f *= 1 after a look")
    p.look()

    def edit(s):
        s.flow.f *= 1
    p.both(edit)
    p.batch()
    t.note("5 flow.f = flow.f.clone() while pending")
    assert p.sim.flow._pending is not None

    def assign(s):
        s.flow.f = s.flow.f.clone()
    p.both(assign)
    t.name(p.sim.flow.f, "f_clone")
    p.batch()
    t.note("6 flow.f_next = torch.empty_like(flow.f) while pending")
    assert p.sim.flow._pending is not None
    fresh = []

    def assign_next(s):
        fresh.append(_like(s))
        s.flow.f_next = fresh[-1]
    p.both(assign_next)
    t.name(fresh[0], "f_next_new")
    p.batch()
    t.note("7 collision.tau changed while pending")
    assert p.sim.flow._pending is not None
    p.both(lambda s: setattr(s.collision, "tau", OTHER_TAU))
    p.batch()
    t.note("8 collision.tau changed while shown")
    p.look()
    p.both(lambda s: setattr(s.collision, "tau", TAU))
    p.batch()
    t.note("9 six steps with an ObservableReporter of interval 2")
    series = []
    for s in (p.sim, p.twin):
        with contextlib.redirect_stdout(io.StringIO()):
            s.reporter.append(lt.ObservableReporter(lt.IncompressibleKineticEnergy(s.flow), interval=2, out=None))
        series.append(s.reporter[-1].out)
    t.note("batch 6")
    p.sim(6)
    for _ in range(3):
        p.twin.flow.f = p.twin.flow.f.clone()
        p.twin(2)
    assert series[0] == series[1] and len(series[0]) == 3, series
    p.look()


def _like(sim):
    """a tensor of the populations' shape and kind, without looking at them"""
    flow = sim.flow
    return torch.empty([flow.stencil.q, *flow.resolution], dtype=flow.context.dtype, device=flow.context.device)


def _edit_mask(node):
    def edit(s):
        s.no_collision_mask[node] = 1               # one more bounce-back node, in place
    return edit


def _masks_shown(p):
    t = p.trace
    t.note("1 a first batch")
    p.batch()
    t.note("10 no_collision_mask edited in place while shown")
    p.look()
    p.both(_edit_mask((2, 6)))
    p.batch()
    p.look()


def _masks(p):
    t = p.trace
    _masks_shown(p)
    p.batch()
    t.note("11 no_collision_mask edited in place while pending")
    assert p.sim.flow._pending is not None
    p.both(_edit_mask((12, 1)))
    p.batch()
    p.look()


SCRIPTS = {"events": _events, "masks": _masks, "masks_shown": _masks_shown}


def run_case(name, script=None):
    """the trace of one case, as a list of lines; ``script``: a function of the pair, played in place of the case's"""
    import lettuce_amd as lt
    which, path = CASES[name]
    pair = Pair(lt, which, path)
    with pair.trace.patched():
        (script or SCRIPTS[which])(pair)
    torch.cuda.synchronize()
    return pair.trace.lines


def recorded(name):
    with open(os.path.join(FIXTURES, name + ".txt")) as fh:
        return fh.read().splitlines()


def assert_same_trace(name):
    got, want = run_case(name), recorded(name)
    for k, (g, w) in enumerate(zip(got, want), start=1):
        assert g == w, f"{name}, line {k}: issued '{g}', recorded '{w}'"
    assert len(got) == len(want), f"{name}: {len(got)} lines issued, {len(want)} recorded"


if __name__ == "__main__":
    out_dir = sys.argv[1] if len(sys.argv) > 1 else FIXTURES
    os.makedirs(out_dir, exist_ok=True)
    for case in CASES:
        with open(os.path.join(out_dir, case + ".txt"), "w") as out:
            out.write("\n".join(run_case(case)) + "\n")
        print("recorded", case)
