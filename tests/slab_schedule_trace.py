"""Schedule traces of the slab drivers: which engine launch, which transport operation and which stream operation a
driver issues, in which order, on which stream and on which buffers.  Test infrastructure for
``test_slab_schedule_trace.py`` (CPU, oracle-backed engine) and ``test_gpu_slab_schedule_trace.py`` (HIP plan).

A case builds one driver on one rank (D3Q19, BGK, grid [64, 8, 8]: the smallest slab the two-step driver takes with
its overlapped branch live), wraps its engine in a recording proxy, hooks its transport and the stream operations, runs
three batches (3 steps, then 4, then 3 again: a batch that starts from ``f``, batches that carry on from the one
before, double steps and -- in the last batch -- the odd single step behind them) and reads ``f`` once at the end.
Every call is one line:

    <event> <arguments> [@<stream>]

``event`` names what happened, not the Python method: ``pack``, ``unpack``, ``send``, ``wait``, ``launch:<entry
point>``, ``engine:<other call>``, ``stream:<operation>``.  Tensor arguments appear as the role of their buffer
(resolved through ``data_ptr``): ``f`` / ``f_next`` (the two population buffers as they were when the trace began),
``send_down`` / ``send_up``, ``send2_down`` / ``send2_up`` (the second pair of the direct schedule), ``recv_from_below``
/ ``recv_from_above``, ``slot<parity>_from_below`` / ``slot<parity>_from_above`` (receive windows).  The last line is the
number of tensors on the driver's device that the driver and its transport hold after the run.

The transports are hooked through whichever of their method names exists -- ``send`` / ``wait`` or ``signal`` /
``wait`` (the windows' names before they shared one interface) or ``start`` / ``finish`` -- so the same helper
traces the commit the fixtures were recorded at and every later one.  The fixtures under ``slab_schedule_traces/``
are recorded output: ``python tests/slab_schedule_trace.py cpu|gpu`` rewrites them, which is only right at a commit
whose schedules are the intended ones.
"""
import contextlib
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

FIXTURES = os.path.join(ROOT, "tests", "slab_schedule_traces")
RESOLUTION = [64, 8, 8]
BATCHES = (3, 4, 3)

# name -> (driver, constructor arguments, bounce-back block?)
CPU_CASES = {
    "cpu-single-step": ("SlabSimulation", {}, False),
    "cpu-two-step-direct": ("TwoStepSlabSimulation", {"direct": True}, False),
    "cpu-two-step-edges": ("TwoStepSlabSimulation", {"direct": False}, False),
    "cpu-two-step-masked": ("TwoStepSlabSimulation", {}, True),
}
GPU_CASES = {
    "gpu-single-step-rccl-overlap": ("SlabSimulation", {"transport": "rccl", "overlap": True}, False),
    "gpu-single-step-rccl-serial": ("SlabSimulation", {"transport": "rccl", "overlap": False}, False),
    "gpu-single-step-copy-overlap": ("SlabSimulation", {"transport": "copy", "overlap": True}, False),
    "gpu-single-step-copy-serial": ("SlabSimulation", {"transport": "copy", "overlap": False}, False),
    "gpu-two-step-rccl-direct": ("TwoStepSlabSimulation", {"transport": "rccl", "direct": True}, False),
    "gpu-two-step-rccl-edges": ("TwoStepSlabSimulation", {"transport": "rccl", "direct": False}, False),
    "gpu-two-step-rccl-signalled": ("TwoStepSlabSimulation", {"transport": "rccl", "signalled": True}, False),
    "gpu-two-step-copy-direct": ("TwoStepSlabSimulation", {"transport": "copy", "direct": True}, False),
    "gpu-two-step-copy-edges": ("TwoStepSlabSimulation", {"transport": "copy", "direct": False}, False),
    "gpu-two-step-copy-direct-2streams": ("TwoStepSlabSimulation", {"transport": "copy", "direct": True,
                                                                    "copy_streams": 2}, False),
}

_EVENT = {"pack": "pack", "pack_two_step": "pack", "unpack": "unpack", "unpack_two_step": "unpack"}
_LAUNCHES = ("stream_collide", "collide_planes", "stream_planes", "wait_edges")


def _transports(sim):
    """the objects that hold transport state: the driver itself where it keeps the message buffers, and its windows"""
    seen, out = set(), []
    for obj in (sim, getattr(sim, "_halo", None), sim._cw, sim._window):
        if obj is not None and id(obj) not in seen:
            seen.add(id(obj))
            out.append(obj)
    return out


class Trace:
    def __init__(self, sim):
        self.sim, self.lines, self.depth = sim, [], 0
        self.cuda = sim._f.is_cuda
        self.fixed = {sim._f.data_ptr(): "f", sim._f_next.data_ptr(): "f_next"}
        self.compute = torch.cuda.current_stream() if self.cuda else None

    # ---- roles of the buffers ----------------------------------------------------------------------
    def _roles(self):
        roles = dict(self.fixed)
        names = {"send_down": ("send_down", "_send_down"), "send_up": ("send_up", "_send_up"),
                 "recv_from_above": ("from_above", "_recv_down"), "recv_from_below": ("from_below", "_recv_up")}
        for obj in _transports(self.sim):
            for role, attributes in names.items():
                for a in attributes:
                    t = vars(obj).get(a)
                    if torch.is_tensor(t):
                        roles[t.data_ptr()] = role
            local = vars(obj).get("_local")                       # copy window: [parity][direction]
            if local is not None:
                for p in (0, 1):
                    roles[local[p][0].data_ptr()] = f"slot{p}_from_below"
                    roles[local[p][1].data_ptr()] = f"slot{p}_from_above"
        send2 = getattr(self.sim, "_send2", None)
        if send2 is not None:
            roles[send2[0].data_ptr()], roles[send2[1].data_ptr()] = "send2_down", "send2_up"
        return roles

    def _show(self, value, roles):
        if torch.is_tensor(value):
            return roles.get(value.data_ptr(), "other")
        if value is None:
            return "-"
        if isinstance(value, float):
            return f"{value:.6g}"
        if isinstance(value, (list, tuple)):
            return "(" + " ".join(self._show(v, roles) for v in value) + ")"
        return str(value)

    def _stream(self, stream=None):
        if not self.cuda:
            return ""
        stream = torch.cuda.current_stream() if stream is None else stream
        if stream == self.compute:
            return "compute"
        return "comm" if self.sim._comm is not None and stream == self.sim._comm else "other"

    def event(self, what, args=(), kwargs=None, result=None):
        if self.depth:
            return                                               # what an operation issues inside itself is its own
        roles = self._roles()
        parts = [what] + [self._show(a, roles) for a in args]
        parts += [f"{k}={self._show(v, roles)}" for k, v in sorted((kwargs or {}).items())]
        if result is not None:                                   # received messages: named by role, whatever their order
            parts.append("-> " + " ".join(sorted(self._show(r, roles) for r in result)))
        if self.cuda:
            parts.append("@" + self._stream())
        self.lines.append(" ".join(parts))

    # ---- hooks -------------------------------------------------------------------------------------
    def wrap(self, what, fn, returns=False):
        def traced(*args, **kwargs):
            if returns:
                self.depth += 1
                try:
                    out = fn(*args, **kwargs)
                finally:
                    self.depth -= 1
                self.event(what, args, kwargs, result=out)
                return out
            self.event(what, args, kwargs)
            self.depth += 1
            try:
                return fn(*args, **kwargs)
            finally:
                self.depth -= 1
        return traced

    def hook_transport(self, obj):
        for event, candidates in (("send", ("send", "signal", "start")), ("wait", ("wait", "finish"))):
            for name in candidates:
                if hasattr(type(obj), name):
                    setattr(obj, name, self.wrap(event, getattr(obj, name), returns=event == "wait"))
                    break

    @contextlib.contextmanager
    def patched(self):
        """the process group's batched point-to-point call and the stream operations, for the length of a run"""
        trace, undo = self, []

        def replace(owner, name, new):
            undo.append((owner, name, getattr(owner, name)))
            setattr(owner, name, new)

        batch = dist.batch_isend_irecv

        class Request:
            def __init__(self, inner, k):
                self.inner, self.k = inner, k

            def wait(self):
                trace.event("wait", (f"request{self.k}",))
                return self.inner.wait()

        def traced_batch(ops):
            trace.event("send", [f"{op.op.__name__}:{trace._show(op.tensor, trace._roles())}:peer{op.peer}:tag{op.tag}"
                                 for op in ops])
            return [Request(r, k) for k, r in enumerate(batch(ops))]
        replace(dist, "batch_isend_irecv", traced_batch)
        if self.cuda:
            def stream_operation(name, original):
                def traced(this, other=None, *rest):
                    if trace.depth == 0:
                        about = trace._stream(other) if isinstance(other, torch.cuda.Stream) else "event"
                        subject = trace._stream(this) if isinstance(this, torch.cuda.Stream) else "event"
                        trace.lines.append(f"stream:{name} {subject} {about}")
                    trace.depth += 1
                    try:
                        return original(this, *(() if other is None else (other,)), *rest)
                    finally:
                        trace.depth -= 1
                return traced
            for owner, name in ((torch.cuda.Stream, "wait_stream"), (torch.cuda.Stream, "wait_event"),
                                (torch.cuda.Event, "record")):
                replace(owner, name, stream_operation(name, getattr(owner, name)))
        try:
            yield
        finally:
            for owner, name, old in reversed(undo):
                setattr(owner, name, old)

    def held_tensors(self):
        """distinct tensors on the driver's device that the driver and its transport hold"""
        device, found = self.sim._f.device, {}

        def walk(value, depth):
            if torch.is_tensor(value):
                if value.device == device and value.numel():
                    found[(value.data_ptr(), tuple(value.shape))] = True
            elif isinstance(value, (list, tuple)) and depth < 3:
                for v in value:
                    walk(v, depth + 1)
        for obj in _transports(self.sim):
            for value in vars(obj).values():
                walk(value, 0)
        return len(found)


class RecordingEngine:
    """the driver's engine, every call of it written to the trace; what the engine lacks, the proxy lacks too"""

    def __init__(self, inner, trace):
        self.__dict__["_inner"], self.__dict__["_trace"] = inner, trace

    def __getattr__(self, name):
        value = getattr(self._inner, name)
        if not callable(value):
            return value
        if name in _EVENT:
            event = _EVENT[name]
        else:
            event = ("launch:" if name.startswith(_LAUNCHES) else "engine:") + name
        return self._trace.wrap(event, value)

    def __setattr__(self, name, value):
        setattr(self._inner, name, value)


def _flow(lt, ctx, slab, masked):
    if not masked:
        return lt.TaylorGreenVortex(ctx, slab.extended_resolution, 400, 0.1, lt.D3Q19(), slab=slab)
    block = torch.zeros(slab.extended_resolution, dtype=torch.bool)
    block[20:24, 2:5, :] = True                                   # crosses the cut of the periodic ring

    class WithBlock(lt.TaylorGreenVortex):
        @property
        def boundaries(self):
            return [lt.BounceBackBoundary(block)]
    return WithBlock(ctx, slab.extended_resolution, 400, 0.1, lt.D3Q19(), slab=slab)


def run_case(name):
    """the trace of one case, as a list of lines"""
    import lettuce_amd as lt
    gpu = name in GPU_CASES
    driver, kwargs, masked = (GPU_CASES if gpu else CPU_CASES)[name]
    switches = {k: os.environ.pop(k) for k in list(os.environ) if k.startswith("LT_SLAB_")}
    try:
        kwargs = dict(kwargs)
        if gpu:
            ctx = lt.Context("cuda:0", torch.float32, use_native=True)
        else:
            from slab_cpu_engine import OracleSlabEngine
            ctx = lt.Context("cpu", torch.float64, use_native=False)
            kwargs["engine"] = OracleSlabEngine("D3Q19", torch.float64, "bgk")
        slab = lt.ZSlab(RESOLUTION, rank=0, world_size=1)
        flow = _flow(lt, ctx, slab, masked)
        sim = getattr(lt, driver)(flow, lt.BGKCollision(flow.units.relaxation_parameter_lu), slab, **kwargs)
        trace = Trace(sim)
        sim.engine = RecordingEngine(sim.engine, trace)
        for window in (sim._cw, sim._window):
            if window is not None:
                trace.hook_transport(window)
        if driver == "TwoStepSlabSimulation":
            trace.lines.append(f"schedule direct={sim._direct_ok()} signalled={sim._signalled_ok()} "
                               f"masked={sim._masked} overlap={sim.overlap}")
        with trace.patched():
            for n in BATCHES:
                trace.lines.append(f"batch {n}")
                sim(n)
            trace.lines.append("read f")
            _ = sim.f                                             # the streaming pass that presents f runs here
        if gpu:
            torch.cuda.synchronize()
        # the rank's own planes: the ghost planes hold only the populations an exchange wrote, the rest was never set
        assert bool(torch.isfinite(sim.local_f()).all())
        trace.lines.append(f"tensors held: {trace.held_tensors()}")
        return trace.lines
    finally:
        os.environ.update(switches)


def recorded(name):
    with open(os.path.join(FIXTURES, name + ".txt")) as fh:
        return fh.read().splitlines()


def assert_same_trace(name):
    got, want = run_case(name), recorded(name)
    for k, (g, w) in enumerate(zip(got, want), start=1):
        assert g == w, f"{name}, line {k}: issued '{g}', recorded '{w}'"
    assert len(got) == len(want), f"{name}: {len(got)} lines issued, {len(want)} recorded"


if __name__ == "__main__":
    cases = {"cpu": CPU_CASES, "gpu": GPU_CASES}[sys.argv[1]]
    out_dir = sys.argv[2] if len(sys.argv) > 2 else FIXTURES
    os.makedirs(out_dir, exist_ok=True)
    for case in cases:
        with open(os.path.join(out_dir, case + ".txt"), "w") as out:
            out.write("\n".join(run_case(case)) + "\n")
        print("recorded", case)
