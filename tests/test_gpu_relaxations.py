"""The TRT and the regularised collision of the HIP engine (LT_COLLISION_TRT = 8, LT_COLLISION_REGULARIZED = 9), in the
manner of test_gpu_smagorinsky.py, whose helpers and shapes are reused.

The CPU reference is the mirror's torch path (lettuce_amd.TRTCollision / RegularizedCollision on a CPU context, pinned
to the reference's own vectors by test_relaxations_host.py) in float64, stepping the same (fp32: the same fp32) initial
state -- with the plan's boundaries through the oracle's boundary operators -- plus the vectors of tests/golden.

Tolerances are the project's own: ATOL 1e-12 / 1e-5 times max(1, |f|max), times max(1, n / 10) in fp32, times 10 with
an anti-bounce-back outlet.  The engine multiplies by 1 / (2 tau) and 1 - 1 / tau formed on the host in double and sums
Pi over opposite pairs where the reference divides and runs a GEMM, so both agree with it at rounding level, not bit
for bit; one engine kernel against another is bit for bit.  Every comparison prints its largest difference before it
asserts.
"""
import numpy as np
import pytest
import torch

import lettuce_amd as lt
from conftest import golden, TORCH_DT
from oracle import lettuce_oracle as orc
from test_gpu_engine import ATOL, _masked_case, dev, plan_for
from test_gpu_paths_vs_oracle import _Oracle, _oracle_boundary, expected_launches, perturbed_state
from test_gpu_smagorinsky import MASKED_LAYOUTS, SMALL, STENCILS, _two_outlets, assert_close, run as _run
from test_host_api import UniformFlow
from test_relaxations_host import FIXTURES

pytestmark = pytest.mark.gpu

TAU = 0.7                    # tau_plus of TRT, tau of the regularised collision
TAU_MINUS = 2.5
STEPS = (1, 2, 3, 8)
COLL = {"trt": 8, "regularized": 9}
OPERATORS = list(COLL)


def run(plan, f0, n, tau=TAU):
    return _run(plan, f0, n, tau)


# --------------------------------------------------------------------------- the CPU reference
def cpu_collision(operator, flow, tau=TAU, tau_minus=TAU_MINUS):
    if operator == "trt":
        return lt.TRTCollision(tau, tau_minus)
    collision = lt.RegularizedCollision()
    collision.native_generator().tau(flow)         # the first use takes the flow's tau ...
    collision.tau = tau                            # ... which an assignment replaces
    return collision


class _Reference(_Oracle):
    """the oracle's stepping and boundaries around the mirror's torch path of the operator"""
    operator, tau_minus = "trt", TAU_MINUS

    def _collision(self, f):
        flow = self.__dict__.get("_flow")
        if flow is None:
            context = lt.Context("cpu", f.dtype, use_native=False)
            flow = self._flow = UniformFlow(context, list(f.shape[1:]), 1, 0.01, STENCILS[self.lat.name]())
        flow.f = f
        return cpu_collision(self.operator, flow, self.tau, self.tau_minus)(flow)


def reference(operator, lat, f0, tau=TAU, tau_minus=TAU_MINUS, entries=(), ncm=None, nsm=None):
    L = orc.LATTICES[lat]
    sim = _Reference(L, f0.double().clone(), operator, tau)
    sim.operator, sim.tau_minus = operator, tau_minus
    if ncm is not None:
        sim.boundaries = [_oracle_boundary(L, e, f0.dtype) for e in entries]
        sim.no_collision_mask, sim.no_streaming_mask = ncm.cpu(), nsm.cpu()
    return sim


def make_plan(operator, lat, dt, res, entries=(), tau_minus=TAU_MINUS, **kwargs):
    from lettuce_amd._native import Plan
    plan = Plan(lat, TORCH_DT[dt], operator, res, entries, **kwargs)
    if operator == "trt":
        plan.set_trt(tau_minus)
    return plan


# --------------------------------------------------------------------------- lt_collide
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("lat", list(SMALL))
@pytest.mark.parametrize("operator", OPERATORS)
def test_collide_against_the_cpu_path(operator, lat, dt):
    res = SMALL[lat]
    f0 = perturbed_state(lat, res, TORCH_DT[dt], 11)
    plan = make_plan(operator, lat, dt, res)
    got = plan.collide(dev(f0), torch.empty_like(dev(f0)), TAU).cpu().numpy()
    sim = reference(operator, lat, f0)
    want = sim._collision(sim.f).numpy()
    # the state tells the operator from BGK: the CPU path itself is more than ten fp32 tolerances away from BGK's
    # result, so a kernel that relaxed everything with tau could not pass below
    bgk = lt.BGKCollision(TAU)(sim._flow).numpy()
    gap = float(np.abs(want - bgk).max())
    print(f"distance from BGK: {gap:.2e}")
    if lat == "D1Q3":
        # ... except on D1Q3, where both operators ARE BGK at tau on every state: with three populations sum x = 0 and
        # sum e x = 0 leave x = f - feq one degree of freedom, c (-2, 1, 1) -- no antisymmetric part for tau_minus to
        # relax, and exactly what w_q / (2 cs^4) (e_q^2 - cs^2) Pi_xx rebuilds from Pi_xx = 2 c.  What a wrong kernel
        # can still do there is use the wrong scalar: the state must tell TRT from the swapped relaxation times and
        # the regularised collision from the one without its correction (tau = 1: feq)
        assert gap <= 8 * 2.0 ** -52 * float(np.abs(want).max())        # (the CPU path runs in float64)
        other = lt.TRTCollision(TAU_MINUS, TAU) if operator == "trt" else cpu_collision(operator, sim._flow, 1.0)
        gap = float(np.abs(want - other(sim._flow).numpy()).max())
        print(f"distance from the operator with the wrong scalar: {gap:.2e}")
    assert gap > 10 * ATOL["f32"]
    assert_close(got, want, dt, what=f"collide {operator} {lat} {dt}")
    assert f"lt::{lat.lower()}, 0, {COLL[operator]}," in plan.kernel_name(), plan.kernel_name()


@pytest.mark.parametrize("name", FIXTURES)
def test_collide_and_steps_against_the_reference_vectors(name):
    """the reference's collided field, and its populations after 1, 2, 3 and 10 steps through lt_run"""
    g = golden(name)
    operator, lat, dt = name.split("_")
    lat = lat.upper()
    res = [int(r) for r in g["resolution"]]
    tau = float(g["tau"])
    plan = make_plan(operator, lat, dt, res, tau_minus=float(g["tau_minus"]) or 1.0)
    f0 = torch.tensor(g["f0"])
    got = plan.collide(dev(f0), torch.empty_like(dev(f0)), tau).cpu().numpy()
    assert_close(got, g["collided"], dt, what=f"{name} collided")
    for n in (1, 2, 3, 10):
        assert_close(run(plan, f0, n, tau), g[f"f{n}"], dt, n, what=f"{name} f{n}")


# --------------------------------------------------------------------------- lt_run: kernel, launches, result
def _case(cid, lat, dt, res, switches, kernel, launches):
    return pytest.param(lat, dt, res, switches, kernel, launches, id=cid)


TWO = {"two_step": 1}
RUNS = [
    _case("one-d1q3-f64", "D1Q3", "f64", [40], {}, "lbm_kernel<double, lt::d1q3, 0, {c},", "one"),
    _case("one-d2q9-f32", "D2Q9", "f32", [12, 10], {}, "lbm_kernel<float, lt::d2q9, 0, {c},", "one"),
    # a grid the many-step and the 2-D two-step kernels take with BGK: neither has these collisions
    _case("one-d2q9-f64-tileable", "D2Q9", "f64", [16, 128], {"two_step": 1, "many_step": 1},
          "lbm_kernel<double, lt::d2q9, 0, {c},", "one"),
    _case("one-d3q15-f64", "D3Q15", "f64", [5, 6, 7], {}, "lbm_kernel<double, lt::d3q15, 0, {c},", "one"),
    _case("one-d3q15-f32-tileable", "D3Q15", "f32", [6, 16, 128], TWO, "lbm_kernel<float, lt::d3q15, 0, {c},", "one"),
    _case("one-d3q19-f32", "D3Q19", "f32", [6, 5, 8], {}, "lbm_kernel<float, lt::d3q19, 0, {c},", "one"),
    _case("one-d3q19-f64-tileable", "D3Q19", "f64", [5, 24, 96], TWO, "lbm_kernel<double, lt::d3q19, 0, {c},", "one"),
    _case("one-d3q27-f32-tileable", "D3Q27", "f32", [6, 12, 128], TWO, "lbm_kernel<float, lt::d3q27, 0, {c},", "one"),
    _case("one-d3q27-f64", "D3Q27", "f64", [4, 6, 5], {}, "lbm_kernel<double, lt::d3q27, 0, {c},", "one"),
    # automatic mode never pairs the steps of these plans (the sweeps have not been measured: DESIGN.md section 7)
    _case("one-d3q19-f32-tileable-automatic", "D3Q19", "f32", [6, 24, 192], {},
          "lbm_kernel<float, lt::d3q19, 0, {c},", "one"),
    _case("lbm2-d3q19-f32-3x3-tiles", "D3Q19", "f32", [6, 24, 192], TWO, "lbm2_kernel<float, lt::d3q19, 0, {c}, 64, 8,", "two"),
]


@pytest.mark.parametrize("lat,dt,res,switches,kernel,launches", RUNS)
@pytest.mark.parametrize("operator", OPERATORS)
def test_lt_run_path_against_the_cpu_path(operator, lat, dt, res, switches, kernel, launches):
    f0 = perturbed_state(lat, res, TORCH_DT[dt], 3)
    plan = make_plan(operator, lat, dt, res)
    setters = {"two_step": plan.set_two_step, "many_step": plan.set_many_step}
    for key, value in switches.items():
        setters[key](value)
    assert plan.kernel_name().startswith(kernel.format(c=COLL[operator])), plan.kernel_name()
    if launches == "two":
        assert plan.two_step_admitted() is None
    sim, want, done = reference(operator, lat, f0), {}, 0
    for n in STEPS:
        sim.step(n - done)
        done = n
        want[n] = sim.f.numpy().copy()
    for n in STEPS:
        got = run(plan, f0, n)
        assert plan.last_run_info() == expected_launches(launches, n - 1, False), (n, plan.last_run_info())
        assert_close(got, want[n], dt, n, what=f"{operator} {lat} {dt} {res} n = {n}")
    # 3 + 5 through lt_continue from the post-collision populations lt_run leaves in its other buffer
    a = dev(f0)
    result, fstar = plan.run(a, torch.empty_like(a), TAU, 3)
    out, _ = plan.run(fstar, result, TAU, 5, from_fstar=True)
    torch.cuda.synchronize()
    assert plan.last_run_info() == expected_launches(launches, 5, False), plan.last_run_info()
    assert_close(out.cpu().numpy(), want[8], dt, 8, what=f"{operator} {lat} {dt} {res} 3 + 5")


# --------------------------------------------------------------------------- one kernel against another, bit for bit
@pytest.mark.parametrize("seg", [1, 2, 7, 0])
@pytest.mark.parametrize("layout", ["reference", "slab"])
@pytest.mark.parametrize("operator", OPERATORS)
def test_two_step_launch_is_bit_identical_to_two_single_steps(operator, layout, seg):
    from lettuce_amd._native import LAYOUT_SLAB
    if layout == "reference":
        plan = make_plan(operator, "D3Q19", "f32", [14, 16, 128])
    else:
        plan = make_plan(operator, "D3Q19", "f32", [128, 16, 14], layout=LAYOUT_SLAB)
    assert plan.f_shape == [19, 14, 16, 128]
    f = dev(perturbed_state("D3Q19", [14, 16, 128], torch.float32, 5))
    a, b, c = torch.empty_like(f), torch.empty_like(f), torch.full_like(f, float("nan"))
    plan.stream_collide(f, a, TAU)
    plan.stream_collide(a, b, TAU)
    plan.set_two_step(1, seg)
    assert plan.kernel_name().startswith(
        f"lbm2_kernel<float, lt::d3q19, {0 if layout == 'reference' else 1}, {COLL[operator]}, 64, 8,")
    plan.stream_collide_twice(f, c, TAU)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(c.cpu().numpy(), b.cpu().numpy())
    assert float((b - f).abs().max()) > 1e-4                       # the steps did something


@pytest.mark.parametrize("layout", ["reference", "slab"])
@pytest.mark.parametrize("operator", OPERATORS)
def test_two_step_launch_on_three_by_three_tiles(operator, layout):
    """[6, 24, 192]: 3 x 3 tiles of 64 x 8, every tile with all eight neighbours"""
    from lettuce_amd._native import LAYOUT_SLAB
    if layout == "reference":
        plan = make_plan(operator, "D3Q19", "f32", [6, 24, 192])
    else:
        plan = make_plan(operator, "D3Q19", "f32", [192, 24, 6], layout=LAYOUT_SLAB)
    f = dev(perturbed_state("D3Q19", [6, 24, 192], torch.float32, 15))
    a, b, c = torch.empty_like(f), torch.empty_like(f), torch.full_like(f, float("nan"))
    plan.stream_collide(f, a, TAU)
    plan.stream_collide(a, b, TAU)
    plan.set_two_step(1)
    assert plan.two_step_admitted() is None
    plan.stream_collide_twice(f, c, TAU)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(c.cpu().numpy(), b.cpu().numpy())


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("lat", list(SMALL))
@pytest.mark.parametrize("operator", OPERATORS)
def test_fused_is_bit_identical_to_stream_then_collide(operator, lat, dt):
    res = SMALL[lat]
    plan = make_plan(operator, lat, dt, res)
    f = dev(perturbed_state(lat, res, TORCH_DT[dt], 7))
    a, b, c = torch.empty_like(f), torch.empty_like(f), torch.empty_like(f)
    plan.stream(f, a)
    plan.collide(a, b, TAU)
    plan.stream_collide(f, c, TAU)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(c.cpu().numpy(), b.cpu().numpy())


@pytest.mark.parametrize("operator", OPERATORS)
def test_fused_is_bit_identical_to_stream_then_collide_with_boundaries(operator):
    lat, res, dtype = "D3Q19", [6, 7, 8], torch.float32
    f0, ncm, nsm, entries = _masked_case(lat, res, dtype, (0, 1), 21, with_field=True)
    plan = make_plan(operator, lat, "f32", res, entries)
    plan.set_masks(dev(ncm), dev(nsm))
    f = dev(f0)
    a, b, c = torch.empty_like(f), torch.empty_like(f), torch.empty_like(f)
    plan.stream(f, a)
    plan.collide(a, b, TAU)
    plan.stream_collide(f, c, TAU)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(c.cpu().numpy(), b.cpu().numpy())


@pytest.mark.parametrize("lat,res,switches,launches", [("D3Q19", [6, 24, 192], TWO, "two"), ("D3Q19", [6, 24, 192], {}, "one"),
                                                       ("D3Q27", [4, 6, 5], {}, "one")])
@pytest.mark.parametrize("operator", OPERATORS)
def test_resident_is_bit_identical_to_dense(operator, lat, res, switches, launches):
    f0 = perturbed_state(lat, res, torch.float32, 9)
    dense = make_plan(operator, lat, "f32", res)
    resident = make_plan(operator, lat, "f32", res)
    for plan in (dense, resident):
        if switches:
            plan.set_two_step(switches["two_step"])
    dense.set_resident(0)
    resident.set_resident(1)
    assert resident.resident_enabled()[0] and not dense.resident_enabled()[0]
    want = run(dense, f0, 8)
    f = dev(f0)
    resident.resident_load(f, TAU)
    resident.resident_advance(TAU, 7)
    assert resident.last_run_info() == expected_launches(launches, 7, False)
    got = resident.resident_store(torch.empty_like(f))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(got.cpu().numpy(), want)


# --------------------------------------------------------------------------- plans with boundaries
@pytest.mark.parametrize("lat,res,dt,outlets,with_field,layout", MASKED_LAYOUTS,
                         ids=[f"{m[0]}-{'x'.join(map(str, m[1]))}-{m[2]}-{m[3]}-outlets-{m[5]}" for m in MASKED_LAYOUTS])
@pytest.mark.parametrize("operator", OPERATORS)
def test_masked_plans_against_the_cpu_path(operator, lat, res, dt, outlets, with_field, layout):
    """bounce-back, equilibrium (table / per-node field) and one or two anti-bounce-back outlets: lt_run, which
    must stay on the one-step kernel (the masked two-step kernels do not have these collisions), against the CPU path;
    in the slab layout (periodic, no ghost planes) the same plan in the other memory order"""
    from lettuce_amd._native import LAYOUT_SLAB
    dtype = TORCH_DT[dt]
    make = _masked_case if outlets == 1 else _two_outlets
    args = (lat, res, dtype, (0, 1), 40) if outlets == 1 else (lat, res, dtype, 40)
    f0, ncm, nsm, entries = make(*args, with_field=with_field)
    if layout == "reference":
        plan = make_plan(operator, lat, dt, res, entries)
        plan.set_masks(dev(ncm), dev(nsm))
        state = f0
    else:
        slab_entries = [dict(e, field=e["field"].permute(0, 3, 2, 1).contiguous()) if "field" in e else e for e in entries]
        plan = make_plan(operator, lat, dt, res, slab_entries, layout=LAYOUT_SLAB)
        plan.set_masks(dev(ncm.permute(2, 1, 0)), dev(nsm.permute(0, 3, 2, 1)))
        state = f0.permute(0, 3, 2, 1)
    plan.set_two_step(1)
    why = plan.two_step_admitted()
    assert why is not None and ("TRT" if operator == "trt" else "regularised") in why, why
    assert plan.kernel_name().startswith(f"lbm_kernel<{'float' if dt == 'f32' else 'double'}, lt::{lat.lower()}, "
                                         f"{0 if layout == 'reference' else 1}, {COLL[operator]}, true, true, true,"), \
        plan.kernel_name()
    sim, done = reference(operator, lat, f0, entries=entries, ncm=ncm, nsm=nsm), 0
    for n in (1, 2, 5):
        sim.step(n - done)
        done = n
        got = run(plan, state, n)
        assert plan.last_run_info() == expected_launches("one", n - 1, True), plan.last_run_info()
        if layout == "slab":
            got = got.transpose(0, 3, 2, 1)
        assert_close(got, sim.f.numpy(), dt, n, outlet=True,
                     what=f"{operator} {lat} {dt} {layout} {outlets} outlet(s) n = {n}")


# --------------------------------------------------------------------------- the slab layout
@pytest.mark.parametrize("operator", OPERATORS)
def test_slab_plane_launches_reproduce_the_reference_layout_bit_for_bit(operator):
    """lt_stream_collide_planes and the packed plane pair of a slab plan (one ghost plane per side, filled as the
    periodic neighbours would) against lt_stream_collide of the same state in the reference layout"""
    from lettuce_amd._native import LAYOUT_SLAB
    res = [10, 6, 8]                                                 # x, y, z
    f0 = perturbed_state("D3Q19", res, torch.float32, 13)
    ref = make_plan(operator, "D3Q19", "f32", res)
    want = ref.stream_collide(dev(f0), torch.empty_like(dev(f0)), TAU).permute(0, 3, 2, 1).contiguous()   # [q, z, y, x]
    slab = make_plan(operator, "D3Q19", "f32", res, layout=LAYOUT_SLAB, ghost_planes=1)
    core = dev(f0.permute(0, 3, 2, 1))
    f = torch.cat([core[:, -1:], core, core[:, :1]], dim=1).contiguous()
    assert list(f.shape) == slab.f_shape
    nz = res[2]
    out = torch.full_like(f, float("nan"))
    slab.stream_collide_planes(f, out, TAU, 1, nz + 1)
    torch.cuda.synchronize()
    assert torch.equal(out[:, 1:nz + 1], want)
    assert f", 1, {COLL[operator]}, true, true, false," in slab.kernel_name()
    # the two boundary planes with the halo messages packed by the same launch
    up, down = slab.crossing(1), slab.crossing(-1)
    out2 = torch.full_like(f, float("nan"))
    pack_first = torch.empty([len(down), res[1], res[0]], device="cuda")
    pack_second = torch.empty([len(up), res[1], res[0]], device="cuda")
    slab.stream_collide_plane_pair_packed(f, out2, TAU, 1, nz, pack_first, pack_second)
    torch.cuda.synchronize()
    assert torch.equal(out2[:, 1], want[:, 0]) and torch.equal(out2[:, nz], want[:, nz - 1])
    assert torch.equal(pack_first, want[down, 0]) and torch.equal(pack_second, want[up, nz - 1])


# --------------------------------------------------------------------------- lt.Simulation
def _noisy_simulation(context, collision, f=None):
    flow = lt.TaylorGreenVortex(context, [16, 16, 16], 1600, 0.1, lt.D3Q19())
    g = torch.Generator().manual_seed(2)
    noise = 1 + 0.1 * (2 * torch.rand(flow.f.shape, generator=g) - 1)
    flow.f = flow.f * noise.to(flow.f.device) if f is None else f.clone()
    return flow, lt.Simulation(flow, collision, [])


def test_changing_tau_minus_between_calls_needs_no_new_plan():
    context = lt.Context("cuda:0", torch.float32, use_native=True)
    collision = lt.TRTCollision(TAU, 1.0)
    flow, sim = _noisy_simulation(context, collision)
    plan = sim._native.plan
    sim(3)
    after3 = flow.f.clone()
    collision.tau_minus = TAU_MINUS
    sim(3)
    assert sim._native.plan is plan
    fresh_flow, fresh = _noisy_simulation(context, lt.TRTCollision(TAU, TAU_MINUS), after3)
    fresh(3)
    assert torch.equal(flow.f, fresh_flow.f)
    same_flow, same = _noisy_simulation(context, lt.TRTCollision(TAU, 1.0), after3)
    same(3)
    assert float((flow.f - same_flow.f).abs().max()) > 50 * ATOL["f32"]
    # ... and without looking at flow.f in between: the second batch carries on from what the first one left
    collision2 = lt.TRTCollision(TAU, 1.0)
    flow2, sim2 = _noisy_simulation(context, collision2)
    sim2(3)
    collision2.tau_minus = TAU_MINUS
    sim2(3)
    assert torch.equal(flow2.f, flow.f)


def test_a_replayed_graph_follows_tau_minus():
    """tau_minus is part of the captured graph's key: a batch that replays the 32-step graph after lt_plan_set_trt
    gives what eager launches give, bit for bit, and not what the stale graph would"""
    res = [12, 10]
    f0 = perturbed_state("D2Q9", res, torch.float64, 23)
    graph, eager = make_plan("trt", "D2Q9", "f64", res, tau_minus=1.0), make_plan("trt", "D2Q9", "f64", res, tau_minus=1.0)
    graph.set_graph_mode(1)
    eager.set_graph_mode(0)
    first = run(graph, f0, 70)
    assert graph.last_run_info() == expected_launches("one", 5, False)        # 64 of 69 fused steps in the graph
    np.testing.assert_array_equal(first, run(eager, f0, 70))
    graph.set_trt(TAU_MINUS)
    eager.set_trt(TAU_MINUS)
    second = run(graph, f0, 70)
    assert graph.last_run_info() == expected_launches("one", 5, False)
    np.testing.assert_array_equal(second, run(eager, f0, 70))
    # the comparisons above are bit for bit in fp64: that the setting reached the kernels at all shows in a difference
    # a thousand times the fp64 engine bound (after 70 steps most of what tau_minus relaxes has decayed: 1.1e-4)
    gap = float(np.abs(second - first).max())
    print(f"tau_minus 1.0 against {TAU_MINUS} after 70 steps: {gap:.2e}")
    assert gap > 1000 * ATOL["f64"]


@pytest.mark.parametrize("operator", OPERATORS)
def test_engine_collide_of_the_operator(operator):
    """collision(flow) on a native context is the engine's collide kernel: one plan for the kind, tau (and tau_minus)
    handed to it before every launch"""
    context = lt.Context("cuda:0", torch.float64, use_native=True)
    flow = lt.TaylorGreenVortex(context, [12, 10], 100, 0.05, lt.D2Q9())
    f0 = perturbed_state("D2Q9", [12, 10], torch.float64, 17)
    flow.f = dev(f0)
    collision = cpu_collision(operator, flow)
    for tau, tau_minus in ((TAU, TAU_MINUS), (0.9, 1.0), (TAU, TAU_MINUS)):
        if operator == "trt":
            collision.tau_plus, collision.tau_minus = tau, tau_minus
        else:
            collision.tau = tau
        got = collision(flow).cpu().numpy()
        sim = reference(operator, "D2Q9", f0, tau, tau_minus)
        assert_close(got, sim._collision(sim.f).numpy(), "f64", what=f"{operator}, tau = {tau}, tau_minus = {tau_minus}")
    assert set(flow._collision_plans) == {operator}


def test_regularized_simulation_takes_the_flows_tau_and_follows_assignments():
    context = lt.Context("cuda:0", torch.float32, use_native=True)
    collision = lt.RegularizedCollision(0.9)                        # the constructor's value is not used
    flow, sim = _noisy_simulation(context, collision)
    f0 = flow.f.cpu()
    sim(2)
    own = flow.units.relaxation_parameter_lu
    assert collision.tau == own
    ref = reference("regularized", "D3Q19", f0, own)
    ref.step(2)
    assert_close(flow.f.cpu().numpy(), ref.f.numpy(), "f32", 2, what="two steps at the flow's tau")
    collision.tau = TAU
    sim(2)
    ref.tau = TAU
    ref.step(2)
    assert_close(flow.f.cpu().numpy(), ref.f.numpy(), "f32", 4, what="two more at the assigned tau")


# --------------------------------------------------------------------------- the C ABI's refusals
def test_set_trt_validates_and_leaves_the_plan_unchanged():
    from lettuce_amd._native import NativeEngineError, Plan
    res = [6, 5, 8]
    f0 = perturbed_state("D3Q19", res, torch.float32, 3)
    plan = make_plan("trt", "D3Q19", "f32", res, tau_minus=1.7)
    before = run(plan, f0, 3)
    for bad in (0.0, -0.1, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(NativeEngineError, match="tau_minus"):
            plan.set_trt(bad)
        np.testing.assert_array_equal(run(plan, f0, 3), before)
    for other in ("bgk", "smagorinsky", "regularized"):
        with pytest.raises(NativeEngineError, match="not TRT"):
            Plan("D3Q19", torch.float32, other, res).set_trt(1.1)
    default = run(make_plan("trt", "D3Q19", "f32", res, tau_minus=1.0), f0, 3)
    np.testing.assert_array_equal(run(Plan("D3Q19", torch.float32, "trt", res), f0, 3), default)      # 1.0 until set
    plan.set_trt(TAU)                                                # equal relaxation times: BGK's relaxation
    assert_close(run(plan, f0, 3), run(plan_for("D3Q19", torch.float32, "bgk", res), f0, 3), "f32", 3, what="tau_minus = tau")
    # no body force on either collision, as on KBC
    for operator in OPERATORS:
        with pytest.raises(NativeEngineError, match="body force"):
            make_plan(operator, "D3Q19", "f32", res).set_force([1e-3, 0, 0], 0.5, 0.3)


@pytest.mark.parametrize("operator", OPERATORS)
def test_two_step_admission(operator):
    """D3Q19 fp64, the other lattices, masked plans and slabs report LT_ERR_UNSUPPORTED with a reason that names the
    collision, and lt_run on them counts one-step launches only"""
    from lettuce_amd._native import LAYOUT_SLAB, NativeEngineError
    named = "TRT" if operator == "trt" else "regularised"
    cases = [("D3Q19", "f64", [5, 24, 96]), ("D3Q27", "f32", [6, 12, 128]), ("D3Q15", "f32", [6, 16, 128]),
             ("D2Q9", "f32", [16, 128])]
    for lat, dt, res in cases:
        plan = make_plan(operator, lat, dt, res)
        plan.set_two_step(1)
        plan.set_many_step(1)
        why = plan.two_step_admitted()
        assert named in why and "plain two-step sweep of periodic D3Q19 fp32 plans" in why, why
        f = dev(perturbed_state(lat, res, TORCH_DT[dt], 3))
        with pytest.raises(NativeEngineError, match=named):
            plan.stream_collide_twice(f, torch.empty_like(f), TAU)
        if lat == "D2Q9":
            with pytest.raises(NativeEngineError, match=named):
                plan.stream_collide_many(f, torch.empty_like(f), TAU, 4)
        run(plan, f.cpu(), 5)
        assert plan.last_run_info() == expected_launches("one", 4, False)
    res = [6, 16, 64]
    f0, ncm, nsm, entries = _masked_case("D3Q19", res, torch.float32, (0, 1), 21)
    masked = make_plan(operator, "D3Q19", "f32", res, entries)
    masked.set_masks(dev(ncm), dev(nsm))
    masked.set_two_step(1)
    assert named in masked.two_step_admitted()
    run(masked, f0, 5)
    assert masked.last_run_info() == expected_launches("one", 4, True)
    slab = make_plan(operator, "D3Q19", "f32", [64, 16, 12], layout=LAYOUT_SLAB, ghost_planes=2)
    assert named in slab.two_step_admitted()
    f = torch.rand(slab.f_shape, device="cuda") * 0.01 + 0.04
    with pytest.raises(NativeEngineError, match=named):
        slab.stream_collide_twice_planes(f, torch.empty_like(f), TAU, 2, 14)
    # the periodic D3Q19 fp32 plan has the sweep; automatic mode leaves it alone
    plan = make_plan(operator, "D3Q19", "f32", [16, 256, 256])
    assert plan.kernel_name().startswith(f"lbm_kernel<float, lt::d3q19, 0, {COLL[operator]},"), plan.kernel_name()
    plan.set_two_step(1)
    assert plan.two_step_admitted() is None
    assert plan.kernel_name().startswith(f"lbm2_kernel<float, lt::d3q19, 0, {COLL[operator]}, 64, 8,"), plan.kernel_name()


@pytest.mark.parametrize("operator", OPERATORS)
def test_two_step_slab_driver_refuses_the_collision_and_the_one_step_driver_takes_it(operator):
    from lettuce_amd._slab import ZSlab, SlabSimulation, TwoStepSlabSimulation
    context = lt.Context("cuda:0", torch.float32, use_native=True)
    res = [64, 8, 12]
    named = "TRT" if operator == "trt" else "regularised"

    def slab_flow():
        slab = ZSlab(res, 0, 1)
        flow = lt.TaylorGreenVortex(context, slab.extended_resolution, 400, 0.1, lt.D3Q19(), slab=slab)
        return slab, flow

    slab, flow = slab_flow()
    with pytest.raises(lt.LettuceException, match=named):
        TwoStepSlabSimulation(flow, cpu_collision(operator, flow), slab)
    slab, flow = slab_flow()
    whole = lt.TaylorGreenVortex(lt.Context("cpu", torch.float64, use_native=False), res, 400, 0.1, lt.D3Q19())
    g = torch.Generator().manual_seed(6)
    noise = 1 + 0.1 * (2 * torch.rand(whole.f.shape, generator=g, dtype=torch.float64) - 1)
    f0 = (whole.f * noise).float()
    h = slab.halo
    flow.f = dev(torch.cat([f0[..., -h:], f0, f0[..., :h]], dim=-1))
    sim = SlabSimulation(flow, cpu_collision(operator, flow), slab)
    assert f", 1, {COLL[operator]}, true, true, false," in sim.engine.kernel_name()
    sim(5)
    ref = reference(operator, "D3Q19", f0)
    ref.step(5)
    assert_close(sim.gather_f().cpu().numpy(), ref.f.numpy(), "f32", 5, what=f"{operator}: slab driver, 5 steps")
