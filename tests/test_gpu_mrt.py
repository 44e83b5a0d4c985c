"""The MRT collision of the HIP engine (LT_COLLISION_MRT = 10; the kernels' COLL 10: Dellar on D2Q9, Hermite on D3Q27,
11: Lallemand), in the manner of test_gpu_relaxations.py, whose helpers and shapes are reused.

The CPU reference is the mirror's torch path (lettuce_amd.MRTCollision on a CPU context, pinned to the reference's own
vectors by test_mrt_host.py) in float64, stepping the same (fp32: the same fp32) initial state -- with the plan's
boundaries through the oracle's boundary operators -- plus the vectors of tests/golden.

Tolerances are the project's own: ATOL 1e-12 / 1e-5 times max(1, |f|max), times max(1, n / 10) in fp32, times 10 with
an anti-bounce-back or pressure outlet.  The engine sums the two matrix products in ascending index where the reference
runs a GEMM, so both agree at rounding level, not bit for bit; one engine kernel against another is bit for bit.  Every
comparison prints its largest difference before it asserts.
"""
import ctypes

import numpy as np
import pytest
import torch

import lettuce_amd as lt
from conftest import golden, TORCH_DT
from oracle import lettuce_oracle as orc
from outlet_p_cases import mirror_flow
from test_gpu_engine import ATOL, _masked_case, dev
from test_gpu_outlet_p import synthetic
from test_gpu_paths_vs_oracle import _Oracle, _oracle_boundary, expected_launches, perturbed_state
from test_gpu_smagorinsky import MASKED_LAYOUTS, SMALL, STENCILS, _two_outlets, assert_close, run as _run
from test_host_api import UniformFlow
from test_mrt_host import FIXTURES, TRANSFORMS, check_plan_refusals, make_collision, quiet, rates_of

pytestmark = pytest.mark.gpu

TAU = 0.7
STEPS = (1, 2, 3, 8)
LATTICE = {"dellar": "D2Q9", "lallemand": "D2Q9", "hermite": "D3Q27"}
COLL = {"dellar": 10, "lallemand": 11, "hermite": 10}
CASES = [pytest.param(t, dt, id=f"{t}-{dt}") for t in TRANSFORMS for dt in ("f64", "f32")]


def run(plan, f0, n):
    return _run(plan, f0, n, 1.0)                   # (tau is not read by an MRT plan)


def mrt_plan(transform, dt, res, rates=None, entries=(), **kwargs):
    from lettuce_amd._native import Plan
    plan = Plan(LATTICE[transform], TORCH_DT[dt], "mrt", res, entries, **kwargs)
    plan.set_mrt(TRANSFORMS[transform][0].__name__, rates_of(transform, TAU) if rates is None else rates)
    return plan


# --------------------------------------------------------------------------- the CPU reference
class _Reference(_Oracle):
    """the oracle's stepping and boundaries around the mirror's torch path of MRT"""
    transform, rates = "dellar", None

    def _collision(self, f):
        flow = self.__dict__.get("_flow")
        if flow is None:
            context = lt.Context("cpu", f.dtype, use_native=False)
            flow = self._flow = UniformFlow(context, list(f.shape[1:]), 1, 0.01, STENCILS[self.lat.name]())
            self._op = make_collision(self.transform, context, self.rates, flow.stencil)
        flow.f = f
        return quiet(self._op, flow)


def reference(transform, f0, rates=None, entries=(), ncm=None, nsm=None, dtype=torch.float64):
    L = orc.LATTICES[LATTICE[transform]]
    sim = _Reference(L, f0.to(dtype).clone(), "mrt", 1.0)
    sim.transform, sim.rates = transform, rates_of(transform, TAU) if rates is None else rates
    if ncm is not None:
        sim.boundaries = [_oracle_boundary(L, e, f0.dtype) for e in entries]
        sim.no_collision_mask, sim.no_streaming_mask = ncm.cpu(), nsm.cpu()
    return sim


def kernel_prefix(transform, dt, layout=0):
    return f"lbm_kernel<{'float' if dt == 'f32' else 'double'}, lt::{LATTICE[transform].lower()}, {layout}, {COLL[transform]},"


# --------------------------------------------------------------------------- lt_collide
@pytest.mark.parametrize("transform,dt", CASES)
def test_collide_against_the_cpu_path(transform, dt):
    lat = LATTICE[transform]
    res = SMALL[lat]
    f0 = perturbed_state(lat, res, TORCH_DT[dt], 11)
    plan = mrt_plan(transform, dt, res)
    got = plan.collide(dev(f0), torch.empty_like(dev(f0)), 1.0).cpu().numpy()
    sim = reference(transform, f0)
    want = sim._collision(sim.f).numpy()
    gap = float(np.abs(want - lt.BGKCollision(TAU)(sim._flow).numpy()).max())
    print(f"distance from BGK: {gap:.2e}")
    assert gap > 10 * ATOL["f32"]
    assert_close(got, want, dt, what=f"collide {transform} {dt}")
    assert plan.kernel_name().startswith(kernel_prefix(transform, dt)), plan.kernel_name()


# --------------------------------------------------------------------------- the reference's vectors, through Simulation
def _native_simulation(transform, dt, res, f0, rates):
    context = lt.Context("cuda:0", TORCH_DT[dt], use_native=True)
    flow = lt.TaylorGreenVortex(context, res, 1600, 0.1, TRANSFORMS[transform][2]())
    flow.f = dev(torch.as_tensor(f0))
    collision = make_collision(transform, context, list(rates), flow.stencil)
    return flow, collision, lt.Simulation(flow, collision, [])


@pytest.mark.parametrize("name", FIXTURES)
def test_simulation_against_the_reference_vectors(name):
    """collision(flow) on a native context is one launch of the collide kernel; f after 1, 2, 3 and 10 steps through
    lt.Simulation, which counts one-step launches only in automatic mode"""
    g = golden(name)
    _, transform, lat, dt = name.split("_")
    res = [int(r) for r in g["resolution"]]
    flow, collision, sim = _native_simulation(transform, dt, res, g["f0"], g["rates"])
    assert sim._native is not None and collision.native_available()
    assert_close(collision(flow).cpu().numpy(), g["collided"], dt, what=f"{name} collided")
    assert set(flow._collision_plans) == {"mrt"}
    assert flow._collision_plans["mrt"].kernel_name().startswith(kernel_prefix(transform, dt))
    done = 0
    for n in (1, 2, 3, 10):
        sim(n - done)
        done = n
        got = flow.f.cpu().numpy()
        info = sim._native.plan.last_run_info()
        assert info["two_step_launches"] == 0 and info["many_step_launches"] == 0, info
        assert_close(got, g[f"f{n}"], dt, n, what=f"{name} f{n}")
    assert sim._native.plan.kernel_name().startswith(kernel_prefix(transform, dt)), sim._native.plan.kernel_name()


@pytest.mark.parametrize("transform", list(TRANSFORMS))
def test_simulation_on_the_asymmetric_states(transform):
    """densities 0.5 - 1.5 at tau 0.501 (collided, 1 and 5 steps) and 1 / 20 - 20 at 0.7 and 1.7 (collided, 1 step)"""
    lat = TRANSFORMS[transform][1]
    g, states = golden(f"asymmetric_mrt_{transform}_{lat}_f64"), golden(f"asymmetric_states_{lat}_f64")
    res = [int(r) for r in states["resolution"]]
    for kind, tau, steps in (("moderate", 0.501, (1, 5)), ("wide", 0.7, (1,)), ("wide", 1.7, (1,))):
        key = f"{kind}_tau{tau}"
        flow, collision, sim = _native_simulation(transform, "f64", res, states[f"f0_{kind}"], g[f"{key}_rates"])
        assert_close(collision(flow).cpu().numpy(), g[f"{key}_collided"], "f64", what=f"{transform} {key} collided")
        done = 0
        for n in steps:
            sim(n - done)
            done = n
            assert_close(flow.f.cpu().numpy(), g[f"{key}_f{n}"], "f64", n, what=f"{transform} {key} f{n}")


# --------------------------------------------------------------------------- lt_run: kernel, launches, result
RUNS = [pytest.param(t, dt, res, switches, id=f"{t}-{dt}-{'x'.join(map(str, res))}{'-switched' if switches else ''}")
        for t, dt, res, switches in [
            ("dellar", "f64", [12, 10], False), ("dellar", "f32", [12, 10], False),
            ("lallemand", "f64", [12, 10], False), ("lallemand", "f32", [12, 10], False),
            # grids the many-step and the two-step kernels take with BGK: MRT has neither
            ("lallemand", "f64", [16, 128], True), ("dellar", "f32", [16, 64], False),
            ("hermite", "f64", [4, 6, 5], False), ("hermite", "f32", [4, 6, 5], False),
            ("hermite", "f32", [6, 12, 128], True)]]


@pytest.mark.parametrize("transform,dt,res,switches", RUNS)
def test_lt_run_against_the_cpu_path(transform, dt, res, switches):
    from lettuce_amd._native import NativeEngineError
    lat = LATTICE[transform]
    f0 = perturbed_state(lat, res, TORCH_DT[dt], 3)
    plan = mrt_plan(transform, dt, res)
    if switches:
        with pytest.raises(NativeEngineError, match="MRT collision has the one-step kernels only"):
            plan.set_two_step(1)
        plan.set_many_step(1)
        assert "MRT" in plan.two_step_admitted()
        f = dev(f0)
        with pytest.raises(NativeEngineError, match="MRT"):
            plan.stream_collide_twice(f, torch.empty_like(f), 1.0)
        if lat == "D2Q9":
            with pytest.raises(NativeEngineError, match="MRT"):
                plan.stream_collide_many(f, torch.empty_like(f), 1.0, 4)
    assert plan.kernel_name().startswith(kernel_prefix(transform, dt) + " true, true, false,"), plan.kernel_name()
    sim, want, done = reference(transform, f0), {}, 0
    for n in STEPS:
        sim.step(n - done)
        done = n
        want[n] = sim.f.numpy().copy()
    for n in STEPS:
        got = run(plan, f0, n)
        assert plan.last_run_info() == expected_launches("one", n - 1, False), (n, plan.last_run_info())
        assert_close(got, want[n], dt, n, what=f"{transform} {dt} {res} n = {n}")
    # 3 + 5 through lt_continue from the post-collision populations lt_run leaves in its other buffer
    a = dev(f0)
    result, fstar = plan.run(a, torch.empty_like(a), 1.0, 3)
    out, _ = plan.run(fstar, result, 1.0, 5, from_fstar=True)
    torch.cuda.synchronize()
    assert plan.last_run_info() == expected_launches("one", 5, False), plan.last_run_info()
    assert_close(out.cpu().numpy(), want[8], dt, 8, what=f"{transform} {dt} {res} 3 + 5")


# --------------------------------------------------------------------------- one kernel against another, bit for bit
@pytest.mark.parametrize("transform,dt", CASES)
def test_fused_is_bit_identical_to_stream_then_collide(transform, dt):
    lat = LATTICE[transform]
    res = SMALL[lat]
    plan = mrt_plan(transform, dt, res)
    f = dev(perturbed_state(lat, res, TORCH_DT[dt], 7))
    a, b, c = torch.empty_like(f), torch.empty_like(f), torch.empty_like(f)
    plan.stream(f, a)
    plan.collide(a, b, 1.0)
    plan.stream_collide(f, c, 1.0)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(c.cpu().numpy(), b.cpu().numpy())
    assert float((b - f).abs().max()) > 1e-4


@pytest.mark.parametrize("transform,res", [("lallemand", [12, 10]), ("hermite", [5, 6, 7])])
def test_fused_is_bit_identical_to_stream_then_collide_with_boundaries(transform, res):
    lat = LATTICE[transform]
    f0, ncm, nsm, entries = _masked_case(lat, res, torch.float32, (0, 1), 21, with_field=True)
    plan = mrt_plan(transform, "f32", res, entries=entries)
    plan.set_masks(dev(ncm), dev(nsm))
    f = dev(f0)
    a, b, c = torch.empty_like(f), torch.empty_like(f), torch.empty_like(f)
    plan.stream(f, a)
    plan.collide(a, b, 1.0)
    plan.stream_collide(f, c, 1.0)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(c.cpu().numpy(), b.cpu().numpy())


def test_resident_and_cache_policies_are_bit_identical():
    res = [4, 6, 5]
    f0 = perturbed_state("D3Q27", res, torch.float32, 9)
    dense, resident, streaming = (mrt_plan("hermite", "f32", res) for _ in range(3))
    dense.set_resident(0)
    resident.set_resident(1)
    streaming.set_resident(0)
    streaming.set_tuning(3)
    assert ", 1, 0, 3, false>" in streaming.kernel_name(), streaming.kernel_name()
    want = run(dense, f0, 8)
    np.testing.assert_array_equal(run(streaming, f0, 8), want)
    f = dev(f0)
    resident.resident_load(f, 1.0)
    resident.resident_advance(1.0, 7)
    assert resident.last_run_info() == expected_launches("one", 7, False)
    got = resident.resident_store(torch.empty_like(f))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(got.cpu().numpy(), want)


# --------------------------------------------------------------------------- plans with boundaries
MRT_MASKED = [m for m in MASKED_LAYOUTS if m[0] in ("D2Q9", "D3Q27")]
MRT_MASKED = [(t,) + m for m in MRT_MASKED for t in TRANSFORMS if LATTICE[t] == m[0]]


@pytest.mark.parametrize("transform,lat,res,dt,outlets,with_field,layout", MRT_MASKED,
                         ids=[f"{m[0]}-{'x'.join(map(str, m[2]))}-{m[3]}-{m[4]}-outlets-{m[6]}" for m in MRT_MASKED])
def test_masked_plans_against_the_cpu_path(transform, lat, res, dt, outlets, with_field, layout):
    """bounce-back, equilibrium (table / per-node field) and one or two anti-bounce-back outlets through lt_run against
    the CPU path; in the slab layout (periodic, no ghost planes) the same plan in the other memory order"""
    from lettuce_amd._native import LAYOUT_SLAB
    dtype = TORCH_DT[dt]
    make = _masked_case if outlets == 1 else _two_outlets
    args = (lat, res, dtype, (0, 1), 40) if outlets == 1 else (lat, res, dtype, 40)
    f0, ncm, nsm, entries = make(*args, with_field=with_field)
    if layout == "reference":
        plan = mrt_plan(transform, dt, res, entries=entries)
        plan.set_masks(dev(ncm), dev(nsm))
        state = f0
    else:
        slab_entries = [dict(e, field=e["field"].permute(0, 3, 2, 1).contiguous()) if "field" in e else e for e in entries]
        plan = mrt_plan(transform, dt, res, entries=slab_entries, layout=LAYOUT_SLAB)
        plan.set_masks(dev(ncm.permute(2, 1, 0)), dev(nsm.permute(0, 3, 2, 1)))
        state = f0.permute(0, 3, 2, 1)
    assert plan.kernel_name().startswith(kernel_prefix(transform, dt, 0 if layout == "reference" else 1) + " true, true, true,"), \
        plan.kernel_name()
    sim, done = reference(transform, f0, entries=entries, ncm=ncm, nsm=nsm), 0
    for n in (1, 2, 3, 8):
        sim.step(n - done)
        done = n
        got = run(plan, state, n)
        assert plan.last_run_info() == expected_launches("one", n - 1, True), plan.last_run_info()
        if layout == "slab":
            got = got.transpose(0, 3, 2, 1)
        assert_close(got, sim.f.numpy(), dt, n, outlet=True, what=f"{transform} {dt} {layout} {outlets} outlet(s) n = {n}")


PRESSURE = [("dellar", "f32", [12, 10], [("EquilibriumOutletP", [1, 0], 1.02)]),
            ("lallemand", "f64", [12, 10], [("EquilibriumOutletP", [1, 0], 1.02), ("AntiBounceBackOutlet", [0, 1], 0.0)]),
            ("hermite", "f64", [10, 8, 6], [("EquilibriumOutletP", [1, 0, 0], 1.02), ("EquilibriumOutletP", [0, 1, 0], 0.99)]),
            ("hermite", "f32", [10, 8, 6], [("EquilibriumOutletP", [0, 0, 1], 0.99)])]


@pytest.mark.parametrize("transform,dt,res,outlets", PRESSURE, ids=[f"{p[0]}-{p[1]}-{len(p[3])}" for p in PRESSURE])
def test_pressure_outlet_plan_native_equals_the_torch_path(transform, dt, res, outlets):
    """an Obstacle with an inlet, a block and constant-pressure outlets: lt.Simulation on a native context against the
    mirror's CPU path in float64 from the same state; the kernel is the pressure-outlet instantiation"""
    lat = LATTICE[transform]
    g = synthetic(lat.lower(), res, outlets)
    name = f"outlet_p_mrt_{lat.lower()}_{dt}"
    f0 = perturbed_state(lat, res, TORCH_DT[dt], 31)
    rates = rates_of(transform, TAU)
    result = {}
    for where, context in (("cpu", lt.Context("cpu", torch.float64, use_native=False)),
                           ("gpu", lt.Context("cuda:0", TORCH_DT[dt], use_native=True))):
        flow = mirror_flow(g, name, context, set_f0=False)
        flow.f = context.convert_to_tensor(f0.clone())
        sim = lt.Simulation(flow, make_collision(transform, context, rates, flow.stencil), [])
        for n, more in ((1, 1), (2, 1), (3, 1), (8, 5)):
            quiet(sim, more)
            result[where, n] = flow.f.cpu().numpy().copy()          # (the torch path steps its tensor in place)
        if where == "gpu":
            kernel = sim._native.plan.kernel_name()
            chain = 2 if len(res) == 3 else 1
            assert kernel.startswith(kernel_prefix(transform, dt) + " true, true, true,") and kernel.endswith(f", {4 + chain}>"), kernel
            info = sim._native.plan.last_run_info()
            assert info["two_step_launches"] == 0 and info["many_step_launches"] == 0, info
    for n in (1, 2, 3, 8):
        assert_close(result["gpu", n], result["cpu", n], dt, n, outlet=True, what=f"{transform} {dt} pressure outlet n = {n}")


# --------------------------------------------------------------------------- the slab layout
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_slab_plane_launches_reproduce_the_reference_layout_bit_for_bit(dt):
    """lt_stream_collide_planes and the packed plane pair of a slab plan (one ghost plane per side, filled as the
    periodic neighbours would) against lt_stream_collide of the same state in the reference layout"""
    from lettuce_amd._native import LAYOUT_SLAB
    res = [10, 6, 8]                                                 # x, y, z
    f0 = perturbed_state("D3Q27", res, TORCH_DT[dt], 13)
    ref = mrt_plan("hermite", dt, res)
    want = ref.stream_collide(dev(f0), torch.empty_like(dev(f0)), 1.0).permute(0, 3, 2, 1).contiguous()   # [q, z, y, x]
    slab = mrt_plan("hermite", dt, res, layout=LAYOUT_SLAB, ghost_planes=1)
    core = dev(f0.permute(0, 3, 2, 1))
    f = torch.cat([core[:, -1:], core, core[:, :1]], dim=1).contiguous()
    assert list(f.shape) == slab.f_shape
    nz = res[2]
    out = torch.full_like(f, float("nan"))
    slab.stream_collide_planes(f, out, 1.0, 1, nz + 1)
    torch.cuda.synchronize()
    assert torch.equal(out[:, 1:nz + 1], want)
    assert ", 1, 10, true, true, false," in slab.kernel_name()
    up, down = slab.crossing(1), slab.crossing(-1)
    out2 = torch.full_like(f, float("nan"))
    pack_first = torch.empty([len(down), res[1], res[0]], device="cuda", dtype=TORCH_DT[dt])
    pack_second = torch.empty([len(up), res[1], res[0]], device="cuda", dtype=TORCH_DT[dt])
    slab.stream_collide_plane_pair_packed(f, out2, 1.0, 1, nz, pack_first, pack_second)
    torch.cuda.synchronize()
    assert torch.equal(out2[:, 1], want[:, 0]) and torch.equal(out2[:, nz], want[:, nz - 1])
    assert torch.equal(pack_first, want[down, 0]) and torch.equal(pack_second, want[up, nz - 1])


def test_slab_simulation_on_one_gpu_and_the_two_step_driver_refuses():
    from lettuce_amd._slab import ZSlab, SlabSimulation, TwoStepSlabSimulation
    context = lt.Context("cuda:0", torch.float32, use_native=True)
    res = [64, 8, 12]
    rates = rates_of("hermite", TAU)

    def slab_flow():
        slab = ZSlab(res, 0, 1)
        flow = lt.TaylorGreenVortex(context, slab.extended_resolution, 400, 0.1, lt.D3Q27(), slab=slab)
        return slab, flow

    slab, flow = slab_flow()
    with pytest.raises(lt.LettuceException, match="MRT"):
        TwoStepSlabSimulation(flow, make_collision("hermite", context, rates, flow.stencil), slab)
    slab, flow = slab_flow()
    whole = lt.TaylorGreenVortex(lt.Context("cpu", torch.float64, use_native=False), res, 400, 0.1, lt.D3Q27())
    g = torch.Generator().manual_seed(6)
    noise = 1 + 0.1 * (2 * torch.rand(whole.f.shape, generator=g, dtype=torch.float64) - 1)
    f0 = (whole.f * noise).float()
    h = slab.halo
    flow.f = dev(torch.cat([f0[..., -h:], f0, f0[..., :h]], dim=-1))
    sim = SlabSimulation(flow, make_collision("hermite", context, rates, flow.stencil), slab)
    assert ", 1, 10, true, true, false," in sim.engine.kernel_name(), sim.engine.kernel_name()
    sim(5)
    ref = reference("hermite", f0, rates)
    ref.step(5)
    assert_close(sim.gather_f().cpu().numpy(), ref.f.numpy(), "f32", 5, what="hermite: slab driver, 5 steps")


# --------------------------------------------------------------------------- new rates between batches
def _noisy_simulation(context, transform, rates, f=None):
    res = [16, 16] if LATTICE[transform] == "D2Q9" else [8, 8, 8]
    flow = lt.TaylorGreenVortex(context, res, 1600, 0.1, TRANSFORMS[transform][2]())
    g = torch.Generator().manual_seed(2)
    noise = 1 + 0.1 * (2 * torch.rand(flow.f.shape, generator=g) - 1)
    flow.f = flow.f * noise.to(flow.f.device) if f is None else f.clone()
    collision = make_collision(transform, context, rates, flow.stencil)
    return flow, collision, lt.Simulation(flow, collision, [])


@pytest.mark.parametrize("transform", list(TRANSFORMS))
def test_changing_the_rates_between_batches_needs_no_new_plan(transform):
    context = lt.Context("cuda:0", torch.float32, use_native=True)
    old, new = rates_of(transform, TAU), rates_of(transform, 0.9)[::-1]
    flow, collision, sim = _noisy_simulation(context, transform, old)
    plan = sim._native.plan
    sim(3)
    after3 = flow.f.clone()
    collision.relaxation_parameters = context.convert_to_tensor(new)
    sim(3)
    assert sim._native.plan is plan
    fresh_flow, _, fresh = _noisy_simulation(context, transform, new, after3)
    fresh(3)
    assert torch.equal(flow.f, fresh_flow.f)
    same_flow, _, same = _noisy_simulation(context, transform, old, after3)
    same(3)
    gap = float((flow.f - same_flow.f).abs().max())
    print(f"old against new rates after 3 steps: {gap:.2e}")
    assert gap > 50 * ATOL["f32"]
    # ... and without looking at flow.f in between: the second batch starts from what the first one left
    flow2, collision2, sim2 = _noisy_simulation(context, transform, old)
    sim2(3)
    collision2.relaxation_parameters = context.convert_to_tensor(new)
    sim2(3)
    assert torch.equal(flow2.f, flow.f)


def test_a_replayed_graph_follows_the_rates():
    """transform and rates are part of the captured graph's key: a batch that replays the 32-step graph after
    lt_plan_set_mrt gives what eager launches give, bit for bit, and not what the stale graph would"""
    res = [12, 10]
    f0 = perturbed_state("D2Q9", res, torch.float64, 23)
    graph, eager = mrt_plan("lallemand", "f64", res), mrt_plan("lallemand", "f64", res)
    graph.set_graph_mode(1)
    eager.set_graph_mode(0)
    first = run(graph, f0, 70)
    assert graph.last_run_info() == expected_launches("one", 5, False)        # 64 of 69 fused steps in the graph
    np.testing.assert_array_equal(first, run(eager, f0, 70))
    new = rates_of("lallemand", 1.3)[::-1]
    for plan in (graph, eager):
        plan.set_mrt("D2Q9Lallemand", new)
    second = run(graph, f0, 70)
    assert graph.last_run_info() == expected_launches("one", 5, False)
    np.testing.assert_array_equal(second, run(eager, f0, 70))
    gap = float(np.abs(second - first).max())
    print(f"old against new rates after 70 steps: {gap:.2e}")
    assert gap > 1000 * ATOL["f64"]
    # the same rates with the other transform of the lattice: the key holds the transform as well
    for plan in (graph, eager):
        plan.set_mrt("D2Q9Dellar", new)
    third = run(graph, f0, 70)
    np.testing.assert_array_equal(third, run(eager, f0, 70))
    assert float(np.abs(third - second).max()) > 1000 * ATOL["f64"]


# --------------------------------------------------------------------------- the C ABI's refusals
def test_refusals_return_their_status_and_message():
    from lettuce_amd import _native
    lib = ctypes.CDLL(_native.library_path())
    for fn in ("lt_plan_create", "lt_plan_set_mrt", "lt_collide", "lt_run", "lt_plan_set_two_step", "lt_plan_two_step_admitted"):
        getattr(lib, fn).restype = ctypes.c_int
    lib.lt_plan_create.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    lib.lt_plan_set_mrt.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.c_int]
    lib.lt_plan_set_two_step.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32]
    lib.lt_plan_two_step_admitted.argtypes = [ctypes.c_void_p]
    lib.lt_plan_destroy.argtypes = [ctypes.c_void_p]
    check_plan_refusals(lib, _native)


def test_set_mrt_validates_and_leaves_the_plan_unchanged():
    from lettuce_amd._native import NativeEngineError, Plan
    res = [12, 10]
    f0 = perturbed_state("D2Q9", res, torch.float32, 3)
    plan = mrt_plan("lallemand", "f32", res)
    before = run(plan, f0, 3)
    good = rates_of("lallemand", TAU)
    for bad in (0.0, -0.1, float("nan"), float("inf")):
        with pytest.raises(NativeEngineError, match="finite and > 0"):
            plan.set_mrt("D2Q9Lallemand", good[:-1] + [bad])
        np.testing.assert_array_equal(run(plan, f0, 3), before)
    with pytest.raises(NativeEngineError, match="8 relaxation rates"):
        plan.set_mrt("D2Q9Lallemand", good[:-1])
    with pytest.raises(NativeEngineError, match="belongs to D3Q27"):
        plan.set_mrt("D3Q27Hermite", rates_of("hermite", TAU))
    with pytest.raises(NativeEngineError, match="has no HIP kernels"):
        plan.set_mrt("D1Q3Transform", [1.0] * 3)
    np.testing.assert_array_equal(run(plan, f0, 3), before)
    with pytest.raises(NativeEngineError, match="not MRT"):
        Plan("D2Q9", torch.float32, "bgk", res).set_mrt("D2Q9Lallemand", good)
    with pytest.raises(NativeEngineError, match="lt_plan_set_mrt must give"):
        run(Plan("D2Q9", torch.float32, "mrt", res), f0, 3)
    with pytest.raises(NativeEngineError, match="MRT collision exists for D2Q9"):
        Plan("D3Q19", torch.float32, "mrt", [4, 4, 4])
    with pytest.raises(NativeEngineError, match="body force"):
        plan.set_force([1e-3, 0], 0.5, 0.3)
    # the rates of the conserved moments are not used, and tau is not read
    other = mrt_plan("lallemand", "f32", res, rates=[0.6, 1.9, 7.0] + good[3:])
    a = dev(f0)
    out, _ = other.run(a, torch.empty_like(a), 0.55, 3)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), before)
    # Dellar with one rate is BGK at that rate, up to rounding
    dellar = mrt_plan("dellar", "f32", res, rates=[TAU] * 9)
    bgk = Plan("D2Q9", torch.float32, "bgk", res)
    assert_close(run(dellar, f0, 3), _run(bgk, f0, 3, TAU), "f32", 3, what="Dellar with one rate against BGK")
