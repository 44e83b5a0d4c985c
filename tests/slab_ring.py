"""N slab ranks in one process: a periodic ``[nx, ny, nz_local * world]`` domain cut into ``world`` slabs, one engine
per rank, the schedules of ``lettuce_amd/_slab.py`` issued by hand and the halo messages moved between the ranks by
plain tensor copies -- no process group, no ``mp.spawn``.  Test infrastructure.

An engine is anything with the slab entry points of ``lettuce_amd._native.Plan`` (layout ``LAYOUT_SLAB``):
``slab_cpu_engine.OracleSlabEngine`` on the CPU, the HIP plans on the GPU.  Rank r's message from below is rank
r - 1's upper message, its message from above rank r + 1's lower one.

A run is ``collide_planes`` on every plane of every slab (the ghost planes were filled by periodic indexing, for this
first launch only), ``fused`` stream-collide steps by the named schedule and ``stream_planes``: what
``OracleSimulation.step(fused + 1)`` gives on the global state.

Two-step schedules (two ghost planes; double steps + one single step when ``fused`` is odd):
  planes        stream_collide_twice_planes over all interior planes, pack_two_step, unpack_two_step
  packed-edges  two stream_collide_twice_planes_packed launches that write the messages, the planes in between, unpack
  merged-edges  stream_collide_twice_edges with both message buffers, the planes in between, unpack
  direct        stream_collide_twice_edges_direct fed from the messages of the double step before (the ghost planes
                of the field are NaN from the second double step on), the planes in between; no pack, no unpack --
                the messages are scattered only before a launch that reads the field's ghost planes
  signalled     stream_collide_twice_slab (+ wait_edges), pack, unpack
One-step schedule (one ghost plane):
  pair          stream_collide_plane_pair_packed on the two outer planes, stream_collide_planes between them, unpack
"""
import torch

from oracle import lettuce_oracle as orc

TWO_STEP_SCHEDULES = ("planes", "packed-edges", "merged-edges", "direct", "signalled")
SCHEDULES = TWO_STEP_SCHEDULES + ("pair",)


def decompose(f_global, world, ghosts):
    """[q, nx, ny, nz] -> ``world`` tensors [q, nz_local + 2 ghosts, ny, nx], ghost planes by periodic indexing"""
    nz = f_global.shape[3]
    assert nz % world == 0
    nzl = nz // world
    slabs = []
    for r in range(world):
        z = (torch.arange(-ghosts, nzl + ghosts) + r * nzl) % nz
        slabs.append(f_global[..., z].permute(0, 3, 2, 1).contiguous())
    return slabs


def gather(slabs, ghosts):
    """the interior planes of the slabs as one [q, nx, ny, nz] tensor on the CPU"""
    parts = [s[:, ghosts:s.shape[1] - ghosts].cpu() for s in slabs]
    return torch.cat(parts, dim=1).permute(0, 3, 2, 1).contiguous()


class SlabRing:
    """``engines``: one per rank.  ``fault`` (negative controls): "wrong-neighbour" takes every message from the
    neighbour on the other side, "swapped-crossing-blocks" exchanges the near-plane and the far-plane crossing
    blocks of every two-step message on delivery.  ``sync``: called before the polling wave of the signalled
    schedule is enqueued (``torch.cuda.synchronize`` on the GPU)."""

    def __init__(self, engines, lattice, schedule, device="cpu", edge_planes=2, fault=None, sync=None):
        assert schedule in SCHEDULES, schedule
        self.engines, self.world = list(engines), len(engines)
        self.lat = orc.LATTICES[lattice]
        self.schedule, self.device, self.edge, self.fault = schedule, device, edge_planes, fault
        self.sync = sync if sync is not None else (lambda: None)
        self.ghosts = 1 if schedule == "pair" else 2
        ez = [v[2] for v in self.lat.e]
        self.n_in_plane, self.n_crossing = ez.count(0), ez.count(1)

    # ---- tensors --------------------------------------------------------------------------------
    def _populations(self, engine, t):
        t = t.to(self.device)
        if getattr(engine, "pop_stride", 0):
            return engine.populations_like(t)           # a plan with padded populations takes only its own tensors
        return t.contiguous()

    def _message(self, like):
        blocks = self.n_crossing if self.ghosts == 1 else self.n_in_plane + 2 * self.n_crossing
        return torch.zeros([blocks, like.shape[2], like.shape[3]], dtype=like.dtype, device=like.device)

    # ---- the exchange ---------------------------------------------------------------------------
    def _deliver(self):
        """every rank's (message from below, message from above): copies of the neighbours' send buffers"""
        w, step = self.world, (-1 if self.fault == "wrong-neighbour" else 1)
        for r in range(w):
            self.from_below[r].copy_(self.send_up[(r - step) % w])
            self.from_above[r].copy_(self.send_down[(r + step) % w])
            if self.fault == "swapped-crossing-blocks" and self.ghosts == 2:
                a, b = self.n_in_plane, self.n_crossing
                for msg in (self.from_below[r], self.from_above[r]):
                    near = msg[a:a + b].clone()
                    msg[a:a + b] = msg[a + b:a + 2 * b]
                    msg[a + b:a + 2 * b] = near

    def _pack(self, bufs):
        for r, eng in enumerate(self.engines):
            eng.pack_two_step(bufs[r], -1, self.send_down[r])
            eng.pack_two_step(bufs[r], +1, self.send_up[r])

    def _unpack(self, bufs):
        for r, eng in enumerate(self.engines):
            eng.unpack_two_step(bufs[r], -1, self.from_below[r])
            eng.unpack_two_step(bufs[r], +1, self.from_above[r])

    def _field_ghosts(self, bufs):
        """direct schedule: the last messages are still in the receive buffers; a launch that reads the ghost planes
        of the field comes next (TwoStepSlabSimulation._field_ghosts)"""
        if self.in_messages:
            self._unpack(bufs)
            self.in_messages = False

    # ---- the schedules --------------------------------------------------------------------------
    def _double_step(self, cur, nxt, tau, first):
        lo, hi, edge, how = self.lo, self.hi, self.edge, self.schedule
        for r, eng in enumerate(self.engines):
            f, out, down, up = cur[r], nxt[r], self.send_down[r], self.send_up[r]
            if how == "planes":
                eng.stream_collide_twice_planes(f, out, tau, lo, hi)
                continue
            if how == "signalled":
                eng.stream_collide_twice_slab(f, out, tau)
                self.sync()                               # the polling wave is enqueued behind a finished launch
                eng.wait_edges()
                continue
            if how == "packed-edges":
                eng.stream_collide_twice_planes_packed(f, out, tau, lo, lo + edge, pack_lower=down)
                eng.stream_collide_twice_planes_packed(f, out, tau, hi - edge, hi, pack_upper=up)
            elif how == "merged-edges":
                eng.stream_collide_twice_edges(f, out, tau, edge, pack_lower=down, pack_upper=up)
            else:
                if first:                                 # the ghost planes of the field hold the neighbours' planes
                    eng.stream_collide_twice_edges_direct(f, out, tau, edge, None, None, down, up)
                else:
                    f[:, :lo] = float("nan")
                    f[:, hi:] = float("nan")
                    eng.stream_collide_twice_edges_direct(f, out, tau, edge, self.from_below[r], self.from_above[r],
                                                          down, up)
            if hi - lo > 2 * edge:
                eng.stream_collide_twice_planes(f, out, tau, lo + edge, hi - edge)
        if how in ("planes", "signalled"):
            self._pack(nxt)
        self._deliver()
        if how == "direct":
            self.in_messages = True
        else:
            self._unpack(nxt)

    def _single_step_two_ghosts(self, cur, nxt, tau):
        self._field_ghosts(cur)
        for r, eng in enumerate(self.engines):
            eng.stream_collide_planes(cur[r], nxt[r], tau, self.lo, self.hi)
        self._pack(nxt)
        self._deliver()
        self._unpack(nxt)

    def _pair_step(self, cur, nxt, tau):
        lo, hi = self.lo, self.hi
        for r, eng in enumerate(self.engines):
            eng.stream_collide_plane_pair_packed(cur[r], nxt[r], tau, lo, hi - 1, self.send_down[r], self.send_up[r])
            if hi - lo > 2:
                eng.stream_collide_planes(cur[r], nxt[r], tau, lo + 1, hi - 1)
        self._deliver()
        for r, eng in enumerate(self.engines):
            eng.unpack(nxt[r], hi, -1, self.from_above[r])
            eng.unpack(nxt[r], 0, +1, self.from_below[r])

    # ---- a run ----------------------------------------------------------------------------------
    def run(self, f_global, tau, fused):
        """post-streaming populations [q, nx, ny, nz] (CPU) after collide + ``fused`` stream-collide steps + stream"""
        g = self.ghosts
        cur = [self._populations(e, s) for e, s in zip(self.engines, decompose(f_global, self.world, g))]
        nxt = [self._populations(e, torch.zeros_like(s)) for e, s in zip(self.engines, cur)]
        n2 = cur[0].shape[1]
        self.lo, self.hi = g, n2 - g
        assert self.ghosts == 1 or self.hi - self.lo >= 2 * self.edge
        new = lambda: [self._message(c) for c in cur]                                    # noqa: E731
        self.send_down, self.send_up, self.from_below, self.from_above = new(), new(), new(), new()
        self.in_messages = False
        for r, eng in enumerate(self.engines):
            eng.collide_planes(cur[r], nxt[r], tau, 0, n2)
        cur, nxt = nxt, cur
        left, first = fused, True
        while left:
            if self.ghosts == 1:
                self._pair_step(cur, nxt, tau)
                left -= 1
            elif left >= 2:
                self._double_step(cur, nxt, tau, first)
                left -= 2
            else:
                self._single_step_two_ghosts(cur, nxt, tau)
                left -= 1
            cur, nxt, first = nxt, cur, False
        self._field_ghosts(cur)
        for r, eng in enumerate(self.engines):
            eng.stream_planes(cur[r], nxt[r], self.lo, self.hi)
        return gather(nxt, g)
