"""The special two-step launches of the slab layout, on every lattice they are built for, against the float64 oracle.

``lt_stream_collide_twice_planes_packed``, ``_edges``, ``_edges_direct`` and ``_slab`` -- lbm2_kernel in MODE 1 and
MODE 2 and the straight-line schedule of a two-plane edge -- are instantiated for D3Q15 fp32 / fp64, D3Q19 fp32 / fp64
and D3Q27 fp32, with BGK and as streaming-only plans.  The message slots (in-plane | near crossing | far crossing
blocks: 5 + 5 + 5, 9 + 5 + 5, 9 + 9 + 9), the tile a workgroup owns and the plane a segment starts at are per-lattice
and per-launch arithmetic, so every one of these instantiations is launched here.

Per launch: (b) the output planes and both messages within the project's tolerance of the oracle, which pulls twice
from the same extended field in float64 (``OracleSlabEngine.stream_collide_twice_planes`` on the promoted input) --
this is the net; (a) in addition, bit for bit what two ``stream_collide_planes`` launches and ``pack_two_step`` give;
(c) the planes the launch does not own keep the value they were filled with.

Axes.  Crossed: lattice and dtype (5) x collision (bgk, none) x five geometries
    tile widths x tiles along y, nz_local, edge_planes, segment length of set_two_step(1, seg):
    1 x 2, 4, 2, 0     the smallest slab: the two-plane edges (straight-line schedule) cover it
    1 x 3, 5, 2, 2     three tiles, an odd plane count, one plane between the edges
    1 x 2, 9, 3, 2     three-plane edges (the sweep), segments of 2 + 1 planes in the packed launches
    1 x 8, 9, 3, 3     a tile count divisible by 8 (both XCD renumberings), three layers in the signalling launch
    1 x 8, 4, 2, 0     the same tile count with the straight-line schedule
Sampled (bgk): two tile widths (2 x 3 tiles, 5 planes, seg 3) on every lattice and dtype, and padded populations
(``set_population_stride`` / ``populations_like``) on D3Q19 fp32, D3Q15 fp64 and D3Q27 fp32.  Every case runs the
four entry points as four tests, each with its variants (lower / upper message, with / without messages, received
messages with NaN ghost planes / the field's ghost planes, two signalling launches on one plan).

The ring cases run whole schedules of lettuce_amd/_slab.py between 2 and 3 plans in one process (slab_ring.py, checked
on the CPU by test_slab_ring.py) from a state without symmetries, against the oracle of the global domain.

Tolerances: ATOL and assert_close of test_gpu_paths_vs_oracle.py -- fp64 1e-12 max(1, |f|max), fp32 1e-5 max(1, |f|max)
max(1, n / 10).  The oracle's own fp32 path is within 5.0e-7 max|f| of float64 on these states after five collides;
the faults test_slab_ring.py injects move the result by 3.9e-3 max|f| and more.
"""
import functools

import numpy as np
import pytest
import torch

from conftest import TORCH_DT
from oracle import lettuce_oracle as orc
from slab_cpu_engine import OracleSlabEngine
from slab_ring import TWO_STEP_SCHEDULES, SlabRing
from test_gpu_engine import ATOL, dev
from test_gpu_paths_vs_oracle import TAU, assert_close, oracle, perturbed_state

pytestmark = pytest.mark.gpu

UNTOUCHED = -7.0
LATTICES = [("D3Q15", "f32"), ("D3Q15", "f64"), ("D3Q19", "f32"), ("D3Q19", "f64"), ("D3Q27", "f32")]
# (tile widths, tiles along y, nz_local, edge_planes, seg)
GEOMETRIES = [(1, 2, 4, 2, 0), (1, 3, 5, 2, 2), (1, 2, 9, 3, 2), (1, 8, 9, 3, 3), (1, 8, 4, 2, 0)]
TWO_WIDTHS = (2, 3, 5, 2, 3)
PADDED = (1, 3, 9, 3, 0)


def _tile(lat, dt):
    """(width, rows) of a two-step tile: rows of 256 bytes, 8 of them (D3Q27: 4)"""
    return (64 if dt == "f32" else 32), (4 if lat == "D3Q27" else 8)


def _cases():
    out = []
    for lat, dt in LATTICES:
        for coll in ("bgk", "none"):
            out += [(lat, dt, coll, g, False) for g in GEOMETRIES]
        out.append((lat, dt, "bgk", TWO_WIDTHS, False))
    out += [(lat, dt, "bgk", PADDED, True) for lat, dt in (("D3Q19", "f32"), ("D3Q15", "f64"), ("D3Q27", "f32"))]
    return out


def _case_id(c):
    lat, dt, coll, (tw, ty, nz, edge, seg), padded = c
    return f"{lat}-{dt}-{coll}-{tw}x{ty}tiles-nz{nz}-edge{edge}-seg{seg}" + ("-padded" if padded else "")


CASES = _cases()
case_params = pytest.mark.parametrize("case", CASES, ids=[_case_id(c) for c in CASES])


def _resolution(case):
    lat, dt, _, (tw, ty, nz, _, _), _ = case
    width, rows = _tile(lat, dt)
    return [tw * width, ty * rows, nz]


def _plan(case):
    from lettuce_amd._native import Plan, LAYOUT_SLAB
    lat, dt, coll, (_, _, nz, _, seg), padded = case
    res = _resolution(case)
    plan = Plan(lat, TORCH_DT[dt], coll, res, [], layout=LAYOUT_SLAB, ghost_planes=2)
    plan.set_two_step(1, seg)
    if padded:
        nodes = (nz + 4) * res[1] * res[0]
        plan.set_population_stride(nodes + (64 * 3 if dt == "f32" else 32 * 5))
    return plan


def _populations(plan, t):
    return plan.populations_like(t) if plan.pop_stride else t.clone()


def _untouched(plan):
    out = plan.empty_populations()
    out.fill_(UNTOUCHED)
    return out


def _message_sets(lat):
    ez = [v[2] for v in orc.LATTICES[lat].e]
    return tuple([q for q in range(len(ez)) if ez[q] == v] for v in (0, 1, -1))


@functools.lru_cache(maxsize=None)
def _reference(case):
    """the input (every plane random, the ghost planes included), what the one-step launches and the pack kernel
    make of it, what the oracle makes of it in float64, and the ghost planes as the messages a neighbour would send"""
    lat, dt, coll, (_, _, nz, _, _), _ = case
    nx, ny, _ = _resolution(case)
    n2 = nz + 4
    f_cpu = perturbed_state(lat, [nx, ny, n2], TORCH_DT[dt], 5).permute(0, 3, 2, 1).contiguous()
    plan = _plan(case)
    f = _populations(plan, dev(f_cpu))
    a, b = _untouched(plan), _untouched(plan)
    plan.stream_collide_planes(f, a, TAU, 1, n2 - 1)
    plan.stream_collide_planes(a, b, TAU, 2, n2 - 2)
    blocks = plan.two_step_message_blocks()
    in_plane, up, down = _message_sets(lat)
    assert blocks == len(in_plane) + len(up) + len(down)
    want_down, want_up = (torch.zeros([blocks, ny, nx], dtype=f.dtype, device="cuda") for _ in range(2))
    plan.pack_two_step(b, -1, want_down)
    plan.pack_two_step(b, +1, want_up)
    engine = OracleSlabEngine(lat, torch.float64, coll)
    engine.ghosts = 2
    f64 = f_cpu.double()
    o = torch.full_like(f64, UNTOUCHED)
    engine.stream_collide_twice_planes(f64, o, TAU, 2, n2 - 2)
    o_down, o_up = (torch.zeros([blocks, ny, nx], dtype=torch.float64) for _ in range(2))
    engine.pack_two_step(o, -1, o_down)
    engine.pack_two_step(o, +1, o_up)
    from_below = torch.cat([f_cpu[in_plane, 1], f_cpu[up, 1], f_cpu[up, 0]])
    from_above = torch.cat([f_cpu[in_plane, n2 - 2], f_cpu[down, n2 - 2], f_cpu[down, n2 - 1]])
    torch.cuda.synchronize()
    return {"f": f_cpu, "ref": b.clone().contiguous(), "down": want_down, "up": want_up, "oracle": o.numpy(),
            "oracle_down": o_down.numpy(), "oracle_up": o_up.numpy(), "from_below": dev(from_below),
            "from_above": dev(from_above), "n2": n2, "blocks": blocks}


def _check(case, ref, out, ranges, down=None, up=None, what=""):
    """`out` after a launch that owns the planes of `ranges`; `down` / `up`: the messages it wrote"""
    dt, n2 = case[1], ref["n2"]
    owned = torch.zeros(n2, dtype=torch.bool)
    for b, e in ranges:
        owned[b:e] = True
    got = out.clone().contiguous()
    got_np, where = got.cpu().numpy(), owned.numpy()
    diff = float(np.abs(got_np[:, where] - ref["oracle"][:, where]).max())
    print(f"{_case_id(case)} {what}: max |launch - oracle| {diff:.3e} on planes {ranges}")
    assert_close(got_np[:, where], ref["oracle"][:, where], dt, 2, False)                 # (b) the net
    for name, msg in (("down", down), ("up", up)):
        if msg is not None:
            assert_close(msg.cpu().numpy(), ref["oracle_" + name], dt, 2, False)
    owned = owned.cuda()
    same = got[:, owned] == ref["ref"][:, owned]
    assert bool(same.all()), (what, "planes (of the owned ones), populations that differ from two one-step launches",
                              torch.nonzero(~same.flatten(2).all(2).T).tolist()[:20])       # (a)
    for name, msg in (("down", down), ("up", up)):
        if msg is not None:
            blocks = torch.nonzero(~(msg == ref[name]).flatten(1).all(1)).flatten().tolist()
            assert not blocks, (what, f"blocks of the {name}ward message that differ from the pack kernel's", blocks)
    assert bool((got[:, ~owned] == UNTOUCHED).all()), (what, "wrote planes it does not own")  # (c)


def _messages(ref):
    return (torch.full_like(ref["down"], UNTOUCHED) for _ in range(2))


def _setup(case):
    ref = _reference(case)
    plan = _plan(case)
    return ref, plan, _populations(plan, dev(ref["f"])), ref["n2"], case[3][3]


# --------------------------------------------------------------------------- the launches
@case_params
def test_packed_launches_of_the_lower_and_the_upper_edge(case):
    ref, plan, f, n2, edge = _setup(case)
    out, (down, up) = _untouched(plan), _messages(ref)
    plan.stream_collide_twice_planes_packed(f, out, TAU, 2, 2 + edge, pack_lower=down)
    _check(case, ref, out, [(2, 2 + edge)], down=down, what="packed, lower")
    assert bool((up == UNTOUCHED).all())
    out = _untouched(plan)
    plan.stream_collide_twice_planes_packed(f, out, TAU, n2 - 2 - edge, n2 - 2, pack_upper=up)
    _check(case, ref, out, [(n2 - 2 - edge, n2 - 2)], up=up, what="packed, upper")
    # one launch over the whole slab writes both messages
    out, (down, up) = _untouched(plan), _messages(ref)
    plan.stream_collide_twice_planes_packed(f, out, TAU, 2, n2 - 2, pack_lower=down, pack_upper=up)
    _check(case, ref, out, [(2, n2 - 2)], down=down, up=up, what="packed, whole slab")


@case_params
def test_both_edges_in_one_launch_with_and_without_messages(case):
    ref, plan, f, n2, edge = _setup(case)
    ranges = [(2, 2 + edge), (n2 - 2 - edge, n2 - 2)]
    out, (down, up) = _untouched(plan), _messages(ref)
    plan.stream_collide_twice_edges(f, out, TAU, edge, pack_lower=down, pack_upper=up)
    _check(case, ref, out, ranges, down=down, up=up, what="edges with messages")
    out = _untouched(plan)
    plan.stream_collide_twice_edges(f, out, TAU, edge)
    _check(case, ref, out, ranges, what="edges without messages")


@case_params
def test_direct_edge_launch_fed_from_the_received_messages(case):
    ref, plan, f, n2, edge = _setup(case)
    ranges = [(2, 2 + edge), (n2 - 2 - edge, n2 - 2)]
    # the ghost planes of the field as the messages the neighbours would have sent; the field's own are NaN
    poisoned = _populations(plan, f)
    poisoned[:, :2] = float("nan")
    poisoned[:, n2 - 2:] = float("nan")
    out, (down, up) = _untouched(plan), _messages(ref)
    plan.stream_collide_twice_edges_direct(poisoned, out, TAU, edge, ref["from_below"], ref["from_above"], down, up)
    _check(case, ref, out, ranges, down=down, up=up, what="direct, received messages")
    # without received messages the launch reads the ghost planes of the field
    out, (down, up) = _untouched(plan), _messages(ref)
    plan.stream_collide_twice_edges_direct(f, out, TAU, edge, None, None, down, up)
    _check(case, ref, out, ranges, down=down, up=up, what="direct, ghost planes of the field")


@case_params
def test_signalling_launch_over_the_whole_slab_and_its_counter(case):
    """lt_stream_collide_twice_slab, twice on one plan: the target of the counter accumulates with the launches.
    The polling wave is enqueued on a second stream only after the launch has been synchronised, so it finds the
    counter at its target or never will: a wrong target shows as wait_timed_out(), after one wait of a second."""
    ref, plan, f, n2, _ = _setup(case)
    side = torch.cuda.Stream()
    for launch in (1, 2):
        out = _untouched(plan)
        plan.stream_collide_twice_slab(f, out, TAU)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            plan.wait_edges()
            assert not plan.wait_timed_out(), f"launch {launch}: the counter never reached the plan's target"
        _check(case, ref, out, [(2, n2 - 2)], what=f"signalling launch {launch}")


# --------------------------------------------------------------------------- whole schedules on a ring of plans
RING_SHAPE = {2: (6, 3), 3: (5, 2)}       # world: (nz_local, edge_planes) -- the edges cover the slab / leave a plane


def _ring_state(lat, dt, world, seed=9):
    width, rows = _tile(lat, dt)
    return perturbed_state(lat, [width, 2 * rows, RING_SHAPE[world][0] * world], TORCH_DT[dt], seed)


def _run_ring(lat, dt, coll, world, schedule, fused, tau=TAU):
    from lettuce_amd._native import Plan, LAYOUT_SLAB
    f0 = _ring_state(lat, dt, world)
    nzl, edge = RING_SHAPE[world]
    ghosts = 1 if schedule == "pair" else 2
    plans = [Plan(lat, TORCH_DT[dt], coll, list(f0.shape[1:3]) + [nzl], [], layout=LAYOUT_SLAB, ghost_planes=ghosts)
             for _ in range(world)]
    ring = SlabRing(plans, lat, schedule, device="cuda", edge_planes=edge, sync=torch.cuda.synchronize)
    got = ring.run(f0, tau, fused)
    if schedule == "signalled":
        assert not any(p.wait_timed_out() for p in plans)
    return got


def _against_oracle(got, want, dt, fused, what):
    print(f"{what}: max |ring - oracle| {float((got.double() - want).abs().max()):.3e}")
    assert_close(got.numpy(), want.numpy(), dt, fused + 1, False)


@pytest.mark.parametrize("fused", [4, 5])
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("lat,dt", LATTICES, ids=[f"{a}-{b}" for a, b in LATTICES])
def test_two_step_schedules_between_ranks_against_the_global_oracle(lat, dt, world, fused):
    """2 ranks: both neighbours are the same peer; 3: distinct.  Even: double steps only; odd: a single step after a
    double step that left its messages in the receive buffers.  All schedules, and the one-step pair schedule, give
    the same bits."""
    sim = oracle(lat, _ring_state(lat, dt, world), "bgk")
    want = sim.step(fused + 1)
    results = {}
    for schedule in TWO_STEP_SCHEDULES + ("pair",):
        results[schedule] = _run_ring(lat, dt, "bgk", world, schedule, fused)
        _against_oracle(results[schedule], want, dt, fused, f"{lat} {dt} {world} ranks {schedule} {fused}")
    for schedule, got in results.items():
        assert torch.equal(got, results["planes"]), f"{schedule} differs from the plain two-step launches"


PAIR_ONLY = [("D3Q27", "f64", "bgk"), ("D3Q27", "f32", "kbc"), ("D3Q19", "f32", "smagorinsky")]


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("lat,dt,coll", PAIR_ONLY, ids=["-".join(c) for c in PAIR_ONLY])
def test_one_step_pair_schedule_between_ranks_against_the_global_oracle(lat, dt, coll, world):
    fused = 5
    f0 = _ring_state(lat, dt, world)
    if coll == "smagorinsky":
        from test_gpu_smagorinsky import TAU as tau, reference
        sim = reference(lat, f0, 0.17, tau)                 # the plan's default constant
    else:
        tau, sim = TAU, oracle(lat, f0, coll)
    want = sim.step(fused + 1)
    got = _run_ring(lat, dt, coll, world, "pair", fused, tau)
    _against_oracle(got, want, dt, fused, f"{lat} {dt} {coll} {world} ranks pair")
