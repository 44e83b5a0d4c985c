"""The constant-pressure equilibrium outlet of the HIP engine (LT_BOUNDARY_PRESSURE_OUTLET = 4, the kernels' ABBD =
kOutletsP + chain).

References: the reference's own vectors (tests/golden/outlet_p_*.npz, boundaries in the stored order) and the mirror's
torch path on the CPU, which test_outlet_p_host.py pins to those vectors.  Bounds are those of test_gpu_engine.py with an
outlet: fp64 1e-12 max(1, |f|max) x 10, fp32 1e-5 max(1, |f|max) x 10.  One engine path against
another is bit for bit.  Every comparison prints its largest difference before it asserts."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import lettuce_amd as lt
from conftest import golden, unpack_nsm, TORCH_DT, ROOT
from outlet_p_cases import (FIXTURES, LATTICES, collision_kind, dtype_tag, lattice_of, make_collision, mirror_flow,
                            plan_entries)
from test_gpu_engine import ATOL, dev
from test_gpu_paths_vs_oracle import expected_launches, perturbed_state

pytestmark = pytest.mark.gpu

NAMED = "constant-pressure outlet"


def assert_close(got, want, dt, what=""):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    bound = ATOL[dt] * max(1.0, float(np.abs(want).max())) * 10
    err = float(np.abs(got - want).max())
    print(f"{what}: max |difference| {err:.3e} (bound {bound:.1e})")
    assert err <= bound, what


def chain_of(lat, layout=0):
    d = LATTICES[lat.lower()]().d
    return 2 if d == 3 and layout == 0 else 1


def fixture_plan(g, name, entries=None, **kwargs):
    from lettuce_amd._native import Plan
    plan = Plan(lattice_of(name).upper(), TORCH_DT[dtype_tag(name)], collision_kind(g), [int(r) for r in g["resolution"]],
                plan_entries(g, name) if entries is None else entries, **kwargs)
    if not kwargs:
        plan.set_masks(dev(g["no_collision_mask"]), dev(unpack_nsm(g)))
    return plan


def run(plan, f0, n, tau):
    a = dev(f0)
    out, _ = plan.run(a, torch.empty_like(a), tau, n)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def synthetic(lat, res, outlets, block=True, with_inlet=True):
    """a fixture-like description of a flow the generator did not write: inlet on the face opposite the first outlet,
    a block in the middle, `outlets` = [(class name, direction, rho_outlet)] in that order"""
    d = len(res)
    first = outlets[0][1]
    axis = [i for i, c in enumerate(first) if c][0]
    inlet = np.zeros(res, dtype=bool)
    index = [slice(None)] * d
    index[axis] = 0 if first[axis] > 0 else res[axis] - 1
    inlet[tuple(index)] = True
    solid = np.zeros(res, dtype=bool)
    if block:
        solid[tuple(slice(n // 2 - 1, n // 2 + 1) for n in res)] = True
    others = ["BounceBackBoundary"] + (["EquilibriumBoundaryPU"] if with_inlet else [])
    kinds = [o[0] for o in outlets] + others
    order = np.argsort(kinds, kind="stable")                      # classes as Simulation sorts them, outlets as listed
    directions = [list(o[1]) for o in outlets] + [[0] * d] * len(others)
    rhos = [o[2] for o in outlets] + [0.0] * len(others)
    return {"resolution": np.array(res), "boundary_order": np.array([kinds[i] for i in order]),
            "boundary_direction": np.array([directions[i] for i in order]), "rho_outlet": np.array([rhos[i] for i in order]),
            "inlet_mask": inlet, "inlet_velocity_pu": np.array([float(c) for c in first]), "block_mask": solid,
            "reynolds": 100.0, "mach": 0.05, "domain_length_x": 2.0, "collision": np.array("bgk"), "tau": 0.7}


def masks_and_entries(g, name):
    """no_collision_mask, no_streaming_mask (uint8, CPU) and the plan entries of a description, from the mirror"""
    flow = mirror_flow(g, name, lt.Context("cpu", TORCH_DT[dtype_tag(name)], use_native=False), set_f0=False)
    sim = lt.Simulation(flow, lt.BGKCollision(0.7), [])
    entries = [b.native_generator(i).plan_entry(flow) for i, b in enumerate(sim.boundaries[1:], start=1)]
    return sim.no_collision_mask.to(torch.uint8), sim.no_streaming_mask.to(torch.uint8), entries


# --------------------------------------------------------------------------- the reference's vectors
@pytest.mark.parametrize("name", FIXTURES)
def test_plan_against_the_reference_vectors(name):
    """lt_collide alone and lt_run for 1, 2 and 6 steps, boundaries in the stored order; the kernel is the
    pressure-outlet instantiation of the lattice's deepest chain"""
    g = golden(name)
    dt = dtype_tag(name)
    tau = float(g["tau"])
    plan = fixture_plan(g, name)
    lat = lattice_of(name)
    kernel = plan.kernel_name()
    assert kernel.startswith(f"lbm_kernel<{'float' if dt == 'f32' else 'double'}, lt::{lat}, 0, ") \
        and kernel.endswith(f", {4 + chain_of(lat)}>"), kernel
    f0 = dev(g["f0"])
    got = plan.collide(f0, torch.empty_like(f0), tau).cpu().numpy()
    assert_close(got, g["collided"], dt, f"{name} collided")
    for n in (1, 2, 6):
        got = run(plan, g["f0"], n, tau)
        assert plan.last_run_info() == expected_launches("one", n - 1, True), plan.last_run_info()
        assert_close(got, g[f"f{n}"], dt, f"{name} f{n}")


# --------------------------------------------------------------------------- one engine path against another
PATHS = ["outlet_p_d1q3_xm_r102_f64", "outlet_p_d2q9_ym_r102_f32", "outlet_p_three_d2q9_f64", "outlet_p_mixed_d3q19_f32",
         "outlet_p_three_d3q19_f32", "outlet_p_axes_d3q27_f32", "outlet_p_row_d3q19_f32", "outlet_p_kbc_d3q27_f64",
         "outlet_p_d3q15_zp_r102_f64", "outlet_p_block_d2q9_f64"]


@pytest.mark.parametrize("name", PATHS)
def test_fused_stream_then_collide_resident_and_cache_policies_agree_bit_for_bit(name):
    g = golden(name)
    tau = float(g["tau"])
    plan = fixture_plan(g, name)
    f = dev(g["f0"])
    a, b, c, d = (torch.empty_like(f) for _ in range(4))
    plan.set_tuning(0)
    plan.stream(f, a)
    plan.collide(a, b, tau)
    plan.stream_collide(f, c, tau)
    plan.set_tuning(3)
    assert plan.kernel_name().endswith(f", 3, false, {4 + chain_of(lattice_of(name))}>"), plan.kernel_name()
    plan.stream_collide(f, d, tau)
    e = plan.collide(a, torch.empty_like(f), tau)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(c.cpu().numpy(), b.cpu().numpy())
    np.testing.assert_array_equal(d.cpu().numpy(), c.cpu().numpy())
    np.testing.assert_array_equal(e.cpu().numpy(), b.cpu().numpy())
    assert float((c - f).abs().max()) > 1e-4
    if len(g["resolution"]) == 1:
        return                                           # (resident populations exist for 2-D and 3-D plans)
    # resident (padded, engine-owned buffers) against dense
    dense, resident = fixture_plan(g, name), fixture_plan(g, name)
    dense.set_resident(0)
    resident.set_resident(1)
    want = run(dense, g["f0"], 6, tau)
    resident.resident_load(f, tau)
    resident.resident_advance(tau, 5)
    assert resident.last_run_info() == expected_launches("one", 5, True)
    got = resident.resident_store(torch.empty_like(f))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(got.cpu().numpy(), want)


SLAB = ["outlet_p_d3q19_xp_r102_f32", "outlet_p_d3q19_ym_r100_f64", "outlet_p_d3q27_zp_r102_f32", "outlet_p_d3q15_zm_r102_f64",
        "outlet_p_three_d3q19_f32", "outlet_p_mixed_d3q19_f64", "outlet_p_row_d3q19_f32", "outlet_p_smagorinsky_d3q19_f32"]


def slab_tensors(g, ghosts=1):
    """populations and masks of a fixture in the slab layout [.., z, y, x] with periodic ghost planes"""
    def extend(t):
        t = t.permute(*range(t.dim() - 3), t.dim() - 1, t.dim() - 2, t.dim() - 3)          # x, y, z -> z, y, x
        z = t.dim() - 3
        lo, hi = t.narrow(z, t.shape[z] - ghosts, ghosts), t.narrow(z, 0, ghosts)
        return torch.cat([lo, t, hi], dim=z).contiguous()
    return (extend(torch.tensor(g["f0"])), extend(torch.tensor(g["no_collision_mask"])),
            extend(torch.tensor(unpack_nsm(g))))


@pytest.mark.parametrize("name", SLAB)
def test_slab_layout_with_one_ghost_plane_reproduces_the_reference_layout_bit_for_bit(name):
    """lt_stream_collide_planes and the packed plane pair of a slab plan against lt_stream_collide in the reference
    layout; an outlet along z sits on the last / first interior plane (no LT_BOUNDARY_ABSENT)"""
    from lettuce_amd._native import LAYOUT_SLAB
    g = golden(name)
    tau = float(g["tau"])
    res = [int(r) for r in g["resolution"]]
    nz = res[2]
    ref = fixture_plan(g, name)
    want = ref.stream_collide(dev(g["f0"]), torch.empty_like(dev(g["f0"])), tau).permute(0, 3, 2, 1).contiguous()
    slab = fixture_plan(g, name, layout=LAYOUT_SLAB, ghost_planes=1)
    f, ncm, nsm = slab_tensors(g)
    assert list(f.shape) == slab.f_shape
    slab.set_masks(dev(ncm), dev(nsm))
    f = dev(f)
    out = torch.full_like(f, float("nan"))
    slab.stream_collide_planes(f, out, tau, 1, nz + 1)
    torch.cuda.synchronize()
    assert slab.kernel_name().endswith(", 5>") and ", lt::d3q" in slab.kernel_name(), slab.kernel_name()
    assert torch.equal(out[:, 1:nz + 1], want)
    up, down = slab.crossing(1), slab.crossing(-1)
    out2 = torch.full_like(f, float("nan"))
    pack_first = torch.empty([len(down), res[1], res[0]], device="cuda", dtype=f.dtype)
    pack_second = torch.empty([len(up), res[1], res[0]], device="cuda", dtype=f.dtype)
    slab.stream_collide_plane_pair_packed(f, out2, tau, 1, nz, pack_first, pack_second)
    torch.cuda.synchronize()
    assert torch.equal(out2[:, 1], want[:, 0]) and torch.equal(out2[:, nz], want[:, nz - 1])
    assert torch.equal(pack_first, want[down, 0]) and torch.equal(pack_second, want[up, nz - 1])


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_an_absent_outlet_along_z_does_nothing(dt):
    """LT_BOUNDARY_ABSENT: another rank holds the plane.  The rank's masks carry no trace of the outlet, and its plan
    computes what the periodic plan without the outlet computes, bit for bit, through the pressure-outlet kernel"""
    from lettuce_amd._native import LAYOUT_SLAB, Plan
    name = f"outlet_p_d3q19_zp_r102_{dt}"
    g = golden(name)
    res = [int(r) for r in g["resolution"]]
    inlet_and_block = synthetic("d3q19", res, [("EquilibriumOutletP", [0, 0, 1], 1.02)])
    ncm, nsm, entries = masks_and_entries(inlet_and_block, name)
    slot = [e["kind"] for e in entries].index("pressure_outlet")
    assert slot == len(entries) - 1
    ncm = torch.where(ncm == slot + 1, torch.zeros_like(ncm), ncm)          # the masks of a rank without the plane
    keep = torch.tensor(inlet_and_block["inlet_mask"] | inlet_and_block["block_mask"])
    nsm = nsm * keep.to(torch.uint8)
    without = [e for e in entries if e["kind"] != "pressure_outlet"]
    tau = 0.7
    ref = Plan("D3Q19", TORCH_DT[dt], "bgk", res, without)
    ref.set_masks(dev(ncm), dev(nsm))
    want = ref.stream_collide(dev(g["f0"]), torch.empty_like(dev(g["f0"])), tau).permute(0, 3, 2, 1).contiguous()
    absent = [dict(e, present=False) if e["kind"] == "pressure_outlet" else e for e in entries]
    slab = Plan("D3Q19", TORCH_DT[dt], "bgk", res, absent, layout=LAYOUT_SLAB, ghost_planes=1)
    fake = dict(g, no_collision_mask=ncm.numpy(), no_streaming_mask=np.packbits(nsm.numpy().astype(bool), axis=None),
                no_streaming_mask_shape=np.array(nsm.shape))
    f, ncm_s, nsm_s = slab_tensors(fake)
    slab.set_masks(dev(ncm_s), dev(nsm_s))
    out = torch.full_like(dev(f), float("nan"))
    slab.stream_collide_planes(dev(f), out, tau, 1, res[2] + 1)
    torch.cuda.synchronize()
    assert slab.kernel_name().endswith(", 5>"), slab.kernel_name()
    assert "lbm_kernel<" in ref.kernel_name() and not ref.kernel_name().endswith(", 5>")
    assert torch.equal(out[:, 1:res[2] + 1], want)
    # ... and present, it does something on that plane
    present = Plan("D3Q19", TORCH_DT[dt], "bgk", res, entries, layout=LAYOUT_SLAB, ghost_planes=1)
    present.set_masks(dev(ncm_s), dev(nsm_s))
    out2 = torch.full_like(dev(f), float("nan"))
    present.stream_collide_planes(dev(f), out2, tau, 1, res[2] + 1)
    torch.cuda.synchronize()
    assert torch.equal(out2[:, 1:res[2]], out[:, 1:res[2]]) and not torch.equal(out2[:, res[2]], out[:, res[2]])


def test_outlets_on_three_axes_are_refused_on_slabs_with_the_reason_the_other_outlet_has():
    from lettuce_amd._native import LAYOUT_SLAB, Plan
    name = "outlet_p_axes_d3q27_f32"
    g = golden(name)
    with pytest.raises(Exception, match="all three axes"):
        Plan("D3Q27", torch.float32, "bgk", [int(r) for r in g["resolution"]], plan_entries(g, name), layout=LAYOUT_SLAB,
             ghost_planes=1)
    mixed = [{"kind": "abb_outlet", "axis": 0, "side": 1}, {"kind": "pressure_outlet", "axis": 1, "side": 1},
             {"kind": "pressure_outlet", "axis": 2, "side": -1}]
    with pytest.raises(Exception, match="all three axes"):
        Plan("D3Q19", torch.float32, "bgk", [8, 6, 4], mixed, layout=LAYOUT_SLAB)


# --------------------------------------------------------------------------- every collision, through lt.Simulation
def _collisions(flow, lat):
    tau = 0.7
    acceleration = [2e-4, -1e-4, 1.5e-4][:flow.stencil.d]
    made = {"none": lt.NoCollision(), "bgk": lt.BGKCollision(tau), "smagorinsky": lt.SmagorinskyCollision(tau, 0.3),
            "trt": lt.TRTCollision(tau, 1.4375), "regularized": lt.RegularizedCollision(),
            "bgk-guo": lt.BGKCollision(tau, force=lt.Guo(flow, tau, acceleration)),
            "smagorinsky-shanchen": lt.SmagorinskyCollision(tau, 0.3, force=lt.ShanChen(flow, tau, acceleration))}
    if lat in ("d2q9", "d3q27"):
        made["kbc"] = lt.KBCCollision(tau)
    return made


COLLISIONS = [("none", "outlet_p_three_d2q9_f64", 0), ("bgk", "outlet_p_mixed_d3q19_f64", 1), ("kbc", "outlet_p_axes_d3q27_f64", 2),
              ("kbc", "outlet_p_three_d2q9_f32", 2), ("smagorinsky", "outlet_p_three_d3q19_f32", 3),
              ("trt", "outlet_p_d3q15_ym_r102_f64", 8), ("regularized", "outlet_p_axes_d3q27_f32", 9),
              ("bgk-guo", "outlet_p_three_d3q19_f64", 5), ("smagorinsky-shanchen", "outlet_p_mixed_d2q9_f64", 7),
              ("bgk", "outlet_p_d1q3_xp_r102_f64", 1)]


@pytest.mark.parametrize("collision,name,coll", COLLISIONS, ids=[f"{c[0]}-{c[1]}" for c in COLLISIONS])
def test_simulation_with_every_collision_against_the_torch_path(collision, name, coll):
    """lt.Simulation on a native context against the mirror's CPU path from the same state, 4 steps: every collision the
    one-step kernels have, forced BGK and forced Smagorinsky included, on a fixture's boundaries in the stored order"""
    g = golden(name)
    dt, lat = dtype_tag(name), lattice_of(name)
    flows = {}
    for where, context in (("cpu", lt.Context("cpu", TORCH_DT[dt], use_native=False)),
                           ("gpu", lt.Context("cuda:0", TORCH_DT[dt], use_native=True))):
        flow = mirror_flow(g, name, context)
        sim = lt.Simulation(flow, _collisions(flow, lat)[collision], [])
        sim(4)
        flows[where] = (flow, sim)
    kernel = flows["gpu"][1]._native.plan.kernel_name()
    assert f"lt::{lat}, 0, {coll}, true, true, true," in kernel and kernel.endswith(f", {4 + chain_of(lat)}>"), kernel
    assert_close(flows["gpu"][0].f.cpu().numpy(), flows["cpu"][0].f.numpy(), dt, f"{collision} on {name}")


def test_obstacle_with_two_pressure_outlets_native_equals_the_torch_path():
    """an Obstacle whose boundaries hold two EquilibriumOutletP (+x and +y, planes meeting in an edge) on a native
    context == the mirror's CPU path, for both orders of the two (str() decides, as in the reference); the native
    simulation reports a pressure-outlet one-step kernel; and the order matters: the two runs are not the same flow"""
    res = [10, 8, 6]
    name = "outlet_p_obstacle_d3q19_f64"
    f0 = perturbed_state("D3Q19", res, torch.float64, 31)
    on_cpu = {}
    for order in (("x", "y"), ("y", "x")):
        outlets = [("EquilibriumOutletP", [1, 0, 0] if a == "x" else [0, 1, 0], 1.02 if a == "x" else 0.99) for a in order]
        g = synthetic("d3q19", res, outlets)
        result = {}
        for where, context in (("cpu", lt.Context("cpu", torch.float64, use_native=False)),
                               ("gpu", lt.Context("cuda:0", torch.float64, use_native=True))):
            flow = mirror_flow(g, name, context, set_f0=False)
            assert isinstance(flow, lt.Obstacle)
            flow.f = context.convert_to_tensor(f0.clone())          # (the torch path steps its tensor in place)
            sim = lt.Simulation(flow, lt.BGKCollision(0.6), [])
            listed = [b.direction for b in sim.boundaries[1:] if isinstance(b, lt.EquilibriumOutletP)]
            assert listed == [o[1] for o in outlets]
            sim(6)
            result[where] = flow.f.cpu().numpy()
            if where == "gpu":
                kernel = sim._native.plan.kernel_name()
                assert kernel.startswith("lbm_kernel<double, lt::d3q19, 0, 1, true, true, true,") and kernel.endswith(", 6>")
        assert_close(result["gpu"], result["cpu"], "f64", f"order {order}")
        on_cpu[order] = result["cpu"]
    gap = float(np.abs(on_cpu[("x", "y")] - on_cpu[("y", "x")]).max())
    print(f"one order against the other: {gap:.2e}")
    assert gap > 1e-6


TUBES = [([16], [("EquilibriumOutletP", [-1], 1.02), ("EquilibriumOutletP", [1], 0.98)], False),
         ([16], [("EquilibriumOutletP", [1], 0.98), ("EquilibriumOutletP", [-1], 1.02)], False),
         ([16], [("AntiBounceBackOutlet", [1], 0.0), ("EquilibriumOutletP", [-1], 1.02)], True),
         ([3], [("EquilibriumOutletP", [-1], 1.02), ("EquilibriumOutletP", [1], 0.98)], False),
         ([2], [("EquilibriumOutletP", [-1], 1.02), ("EquilibriumOutletP", [1], 0.98)], False),
         ([2], [("EquilibriumOutletP", [1], 0.98), ("EquilibriumOutletP", [-1], 1.02)], False),
         ([2], [("AntiBounceBackOutlet", [1], 0.0), ("EquilibriumOutletP", [-1], 1.02)], False)]


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("res,outlets,inlet", TUBES, ids=[f"{t[0][0]}-{'-'.join(o[0][:1] + 'mp'[o[1][0] > 0] for o in t[1])}" for t in TUBES])
def test_a_tube_with_an_outlet_at_each_end_of_d1q3_against_the_torch_path(res, outlets, inlet, dt):
    """D1Q3 with outlets on -x and +x, two constant-pressure ones in both orders and one beside an anti-bounce-back
    outlet (with an inlet in the pressure outlet's plane, which that outlet overwrites): lt.Simulation on a native context
    == the mirror's CPU path.  On three nodes both outlets read the middle node; on two nodes each outlet's neighbour
    lies in the other's plane and is rebuilt (chain depth 1)"""
    g = synthetic("d1q3", res, outlets, block=False, with_inlet=inlet)
    name = f"outlet_p_tube_d1q3_{dt}"
    f0 = perturbed_state("D1Q3", res, TORCH_DT[dt], 17)
    result = {}
    for where, context in (("cpu", lt.Context("cpu", TORCH_DT[dt], use_native=False)),
                           ("gpu", lt.Context("cuda:0", TORCH_DT[dt], use_native=True))):
        flow = mirror_flow(g, name, context, set_f0=False)
        flow.f = context.convert_to_tensor(f0.clone())
        sim = lt.Simulation(flow, lt.BGKCollision(0.7), [])
        listed = [(type(b).__mro__[1].__name__, b.direction) for b in sim.boundaries[1:] if isinstance(b, lt.AntiBounceBackOutlet)]
        assert listed == [(o[0], o[1]) for o in outlets]
        sim(4)
        result[where] = flow.f.cpu().numpy()
        if where == "gpu":
            kernel = sim._native.plan.kernel_name()
            assert f"lt::d1q3, 0, 1, true, true, true," in kernel and kernel.endswith(", 5>"), kernel
    assert np.isfinite(result["cpu"]).all() and float(np.abs(result["cpu"] - f0.numpy()).max()) > 1e-4
    assert_close(result["gpu"], result["cpu"], dt, f"{res} {[o[0] for o in outlets]}")


# --------------------------------------------------------------------------- lt_plan_update_boundary
def test_a_new_rho_outlet_changes_the_next_step_and_a_moved_outlet_the_plane():
    from lettuce_amd._native import NativeEngineError
    name = "outlet_p_d3q19_yp_r100_f32"
    g = golden(name)
    tau = float(g["tau"])
    entries = plan_entries(g, name)
    slot = [e["kind"] for e in entries].index("pressure_outlet")
    plan = fixture_plan(g, name)
    first = run(plan, g["f0"], 3, tau)
    plan.update_boundary(slot, dict(entries[slot], rho_outlet=1.02))
    second = run(plan, g["f0"], 3, tau)
    fresh = fixture_plan(g, name, entries=[dict(e, rho_outlet=1.02) if e["kind"] == "pressure_outlet" else e for e in entries])
    fresh.set_masks(dev(g["no_collision_mask"]), dev(unpack_nsm(g)))
    np.testing.assert_array_equal(second, run(fresh, g["f0"], 3, tau))
    gap = float(np.abs(second - first).max())
    print(f"rho_outlet 1.0 -> 1.02 after 3 steps: {gap:.2e}")
    assert gap > 100 * ATOL["f32"]
    # moved to the other side of its axis, with the masks of the new place: what a fresh plan computes
    moved = golden("outlet_p_d3q19_ym_r100_f32")
    plan.update_boundary(slot, dict(entries[slot], side=-1, rho_outlet=1.0))
    plan.set_masks(dev(moved["no_collision_mask"]), dev(unpack_nsm(moved)))
    # (the inlet of that fixture is on the other face: only the outlet's entry is compared, on the same masks)
    other = fixture_plan(g, name, entries=[dict(e, side=-1) if e["kind"] == "pressure_outlet" else e for e in entries])
    other.set_masks(dev(moved["no_collision_mask"]), dev(unpack_nsm(moved)))
    np.testing.assert_array_equal(run(plan, g["f0"], 3, tau), run(other, g["f0"], 3, tau))
    # what lt_plan_create refuses is refused here too, and the kind cannot change
    with pytest.raises(NativeEngineError, match=NAMED):
        plan.update_boundary(slot, dict(entries[slot], axis=3))
    with pytest.raises(NativeEngineError, match="kind cannot change"):
        plan.update_boundary(slot, {"kind": "abb_outlet", "axis": 1, "side": 1})


def test_a_replayed_graph_follows_rho_outlet():
    """a batch that replays the captured 32-step graph after lt_plan_update_boundary gives what eager launches give, bit
    for bit, and not what the graph captured for the old density would"""
    name = "outlet_p_d2q9_xp_r100_f64"
    g = golden(name)
    tau = float(g["tau"])
    entries = plan_entries(g, name)
    slot = [e["kind"] for e in entries].index("pressure_outlet")
    graph, eager = fixture_plan(g, name), fixture_plan(g, name)
    graph.set_graph_mode(1)
    eager.set_graph_mode(0)
    first = run(graph, g["f0"], 70, tau)
    assert graph.last_run_info() == expected_launches("one", 5, True)         # 64 of 69 fused steps in the graph
    np.testing.assert_array_equal(first, run(eager, g["f0"], 70, tau))
    for plan in (graph, eager):
        plan.update_boundary(slot, dict(entries[slot], rho_outlet=1.03))
    second = run(graph, g["f0"], 70, tau)
    assert graph.last_run_info() == expected_launches("one", 5, True)
    np.testing.assert_array_equal(second, run(eager, g["f0"], 70, tau))
    gap = float(np.abs(second - first).max())
    print(f"rho_outlet 1.0 against 1.03 after 70 steps: {gap:.2e}")
    assert np.isfinite(second).all() and gap > 1000 * ATOL["f64"]


# --------------------------------------------------------------------------- several steps per launch: refused by name
def test_multi_step_entry_points_refuse_the_boundary_and_lt_run_keeps_the_one_step_kernel():
    from lettuce_amd._native import LAYOUT_SLAB, NativeEngineError, Plan
    cases = [("d3q19", "D3Q19", "f32", [6, 16, 64], [1, 0, 0]),        # the masked two-step kernel's own shape (outlet at
             ("d3q19", "D3Q19", "f32", [6, 16, 64], [0, 0, 1]),        # the last plane of the sweep; then along the rows)
             ("d2q9", "D2Q9", "f64", [16, 128], [1, 0])]               # the 2-D two-step and the many-step kernels' shape
    with_the_other_outlet = {}
    for tag, lat, dt, res, direction in cases:
        name = f"outlet_p_refusal_{tag}_{dt}"
        g = synthetic(tag, res, [("EquilibriumOutletP", direction, 1.02)])
        ncm, nsm, entries = masks_and_entries(g, name)
        plan = Plan(lat, TORCH_DT[dt], "bgk", res, entries)
        plan.set_masks(dev(ncm), dev(nsm))
        plan.set_two_step(1)
        plan.set_many_step(1)
        why = plan.two_step_admitted()
        assert why is not None and NAMED in why and "EquilibriumOutletP" in why, why
        f = dev(perturbed_state(lat, res, TORCH_DT[dt], 3))
        with pytest.raises(NativeEngineError, match=NAMED):
            plan.stream_collide_twice(f, torch.empty_like(f), 0.7)
        if lat == "D2Q9":
            with pytest.raises(NativeEngineError, match=NAMED):
                plan.stream_collide_many(f, torch.empty_like(f), 0.7, 4)
        assert plan.kernel_name().startswith("lbm_kernel<") and plan.kernel_name().endswith(f", {4 + chain_of(tag)}>")
        run(plan, f.cpu(), 5, 0.7)
        assert plan.last_run_info() == expected_launches("one", 4, True), plan.last_run_info()
        # the same flow with the other outlet in that place is one the multi-step kernels take: the refusal is this
        # boundary's
        ncm, nsm, entries = masks_and_entries(synthetic(tag, res, [("AntiBounceBackOutlet", direction, 0.0)]), name)
        assert [e["kind"] for e in entries].count("abb_outlet") == 1
        other = Plan(lat, TORCH_DT[dt], "bgk", res, entries)
        other.set_masks(dev(ncm), dev(nsm))
        other.set_two_step(1)
        other.set_many_step(1)
        with_the_other_outlet[f"{lat} {res} {direction}"] = other.two_step_admitted()
    assert all(why is None for why in with_the_other_outlet.values()), with_the_other_outlet
    slab = Plan("D3Q19", torch.float32, "bgk", [64, 16, 12], [{"kind": "pressure_outlet", "axis": 0, "side": 1}],
                layout=LAYOUT_SLAB, ghost_planes=2)
    assert NAMED in slab.two_step_admitted()
    f = torch.rand(slab.f_shape, device="cuda") * 0.01 + 0.04
    with pytest.raises(NativeEngineError, match=NAMED):
        slab.stream_collide_twice_planes(f, torch.empty_like(f), 0.7, 2, 14)
    with pytest.raises(NativeEngineError, match=NAMED):
        slab.stream_collide_twice_edges(f, torch.empty_like(f), 0.7, 2)


def _slab_carrier(context, slab, res, block):
    """Obstacle on a z-slab with an inlet at x = 0, pressure outlets on +x (first) and +z, and a bounce-back block"""
    class OutX(lt.EquilibriumOutletP):
        def __str__(self):
            return "outlet-a"

    class OutZ(lt.EquilibriumOutletP):
        def __str__(self):
            return "outlet-b"

    class Carrier(lt.Obstacle):
        made = None

        @property
        def boundaries(self):
            if self.made is None:
                x = self.grid[0]
                self.made = [lt.EquilibriumBoundaryPU(self.context, torch.abs(x) < 1e-6, [1.0, 0.0, 0.0]),
                             OutX([1, 0, 0], self, 1.02), OutZ([0, 0, 1], self, 0.99), lt.BounceBackBoundary(self.mask)]
            return self.made

    resolution = slab.extended_resolution if slab is not None else res
    flow = Carrier(context, resolution, 100, 0.05, 2, stencil=lt.D3Q19(), slab=slab)
    flow.mask = block if slab is None else block[:, :, slab.z_indices()]
    return flow


def _slab_state(res):
    block = torch.zeros(res, dtype=torch.bool)
    block[3:5, 2:4, 3:5] = True
    return block, perturbed_state("D3Q19", res, torch.float64, 41)


def _slab_worker(rank, world, port, res, steps, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    context = lt.Context("cuda:0", torch.float64, use_native=True)
    block, f0 = _slab_state(res)
    slab = lt.ZSlab(res)
    flow = _slab_carrier(context, slab, res, block)
    flow.f = context.convert_to_tensor(f0[..., slab.z_indices()])
    sim = lt.SlabSimulation(flow, lt.BGKCollision(0.6), slab)
    kernel = sim.engine.kernel_name()
    sim(steps)
    f = sim.gather_f()
    if rank == 0:
        np.savez(os.path.join(out_dir, "out.npz"), f=f.cpu().numpy(), kernel=np.array(kernel))
    dist.barrier()
    dist.destroy_process_group()


def test_slab_driver_with_two_ranks_against_the_single_domain():
    """SlabSimulation, two ranks sharing the GPU, pressure outlets along x and along z (the decomposed axis: present on
    the upper rank, LT_BOUNDARY_ABSENT on the lower), against the mirror's CPU path on the whole domain; and the
    two-step slab driver refuses the flow with the reason"""
    import tempfile
    res, steps = [10, 6, 8], 5
    block, f0 = _slab_state(res)
    whole = _slab_carrier(lt.Context("cpu", torch.float64, use_native=False), None, res, block)
    whole.f = f0.clone()
    lt.Simulation(whole, lt.BGKCollision(0.6), [])(steps)
    with tempfile.TemporaryDirectory() as tmp:
        mp.spawn(_slab_worker, args=(2, 29300 + os.getpid() % 1000, res, steps, tmp), nprocs=2, join=True)
        got = np.load(os.path.join(tmp, "out.npz"))
        kernel, f = str(got["kernel"]), got["f"]
    assert "lbm_kernel<double, lt::d3q19, 1, 1, true, true," in kernel and kernel.endswith(", 5>"), kernel
    assert_close(f, whole.f.numpy(), "f64", "two ranks against the whole domain")
    context = lt.Context("cuda:0", torch.float32, use_native=True)
    res2 = [64, 8, 12]
    slab = lt.ZSlab(res2, 0, 1)
    flow = _slab_carrier(context, slab, res2, torch.zeros(res2, dtype=torch.bool))
    with pytest.raises(lt.LettuceException, match=NAMED):
        lt.TwoStepSlabSimulation(flow, lt.BGKCollision(0.6), slab)
