"""The Smagorinsky collision of the HIP engine (LT_COLLISION_SMAGORINSKY), in the manner of test_gpu_paths_vs_oracle.py.

The CPU reference is the mirror's torch path (lettuce_amd.SmagorinskyCollision on a CPU context, pinned to the
reference's own vectors by test_smagorinsky_host.py) in float64, stepping the same (fp32: the same fp32) initial state
-- with the plan's boundaries through the oracle's boundary operators -- plus the vectors of tests/golden.

Tolerances are the project's own: ATOL 1e-12 / 1e-5 times max(1, |f|max), times max(1, n / 10) in fp32, times 10 with
an anti-bounce-back outlet.  The engine forms S:S with one division by 2 rho cs^2 and a reciprocal per iteration
where the reference divides the d x d components, so it agrees at rounding level (as KBC does), not bit for bit.
Every comparison prints its largest difference before it asserts.
"""
import numpy as np
import pytest
import torch

import lettuce_amd as lt
from conftest import golden, TORCH_DT
from oracle import lettuce_oracle as orc
from test_gpu_engine import ATOL, _masked_case, dev, plan_for
from test_gpu_paths_vs_oracle import _Oracle, _oracle_boundary, expected_launches, perturbed_state
from test_host_api import UniformFlow
from test_smagorinsky_host import LATTICES as FIXTURE_LATTICES, OBSTACLES, obstacle_from

pytestmark = pytest.mark.gpu

TAU = 0.51
STEPS = (1, 2, 3, 8)
STENCILS = {"D1Q3": lt.D1Q3, "D2Q9": lt.D2Q9, "D3Q15": lt.D3Q15, "D3Q19": lt.D3Q19, "D3Q27": lt.D3Q27}


# --------------------------------------------------------------------------- the CPU reference
class _Reference(_Oracle):
    """the oracle's stepping and boundaries around the mirror's Smagorinsky torch path"""
    constant = 0.17

    def _collision(self, f):
        flow = self.__dict__.get("_flow")
        if flow is None:
            context = lt.Context("cpu", f.dtype, use_native=False)
            flow = self._flow = UniformFlow(context, list(f.shape[1:]), 1, 0.01, STENCILS[self.lat.name]())
        flow.f = f
        return lt.SmagorinskyCollision(self.tau, self.constant)(flow)


def reference(lat, f0, constant, tau=TAU, entries=(), ncm=None, nsm=None):
    L = orc.LATTICES[lat]
    sim = _Reference(L, f0.double().clone(), "smagorinsky", tau)
    sim.constant = constant
    if ncm is not None:
        sim.boundaries = [_oracle_boundary(L, e, f0.dtype) for e in entries]
        sim.no_collision_mask, sim.no_streaming_mask = ncm.cpu(), nsm.cpu()
    return sim


def assert_close(got, want, dt, n=1, outlet=False, what=""):
    got, want = np.asarray(got), np.asarray(want)
    scale = (max(1.0, n / 10) if dt == "f32" else 1.0) * (10 if outlet else 1)
    tol = ATOL[dt] * max(1.0, float(np.abs(want).max())) * scale
    print(f"{what}: max |difference| {float(np.abs(got - want).max()):.3e} (bound {tol:.1e})")
    np.testing.assert_allclose(got, want, rtol=0, atol=tol)


def smagorinsky_plan(lat, dt, res, constant, entries=(), **kwargs):
    from lettuce_amd._native import Plan
    plan = Plan(lat, TORCH_DT[dt], "smagorinsky", res, entries, **kwargs)
    plan.set_smagorinsky(constant)
    return plan


def run(plan, f0, n, tau=TAU):
    a = dev(f0)
    out, _ = plan.run(a, torch.empty_like(a), tau, n)
    torch.cuda.synchronize()
    return out.cpu().numpy()


SMALL = {"D1Q3": [40], "D2Q9": [12, 10], "D3Q15": [5, 6, 7], "D3Q19": [6, 5, 8], "D3Q27": [4, 6, 5]}


# --------------------------------------------------------------------------- lt_collide
@pytest.mark.parametrize("constant", [0.17, 1.0])
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("lat", list(SMALL))
def test_collide_against_the_cpu_path(lat, dt, constant):
    res = SMALL[lat]
    f0 = perturbed_state(lat, res, TORCH_DT[dt], 11)
    plan = smagorinsky_plan(lat, dt, res, constant)
    got = plan.collide(dev(f0), torch.empty_like(dev(f0)), TAU).cpu().numpy()
    sim = reference(lat, f0, constant)
    want = sim._collision(sim.f).numpy()
    if constant == 1.0:
        # the state tells the operator from BGK: the CPU path itself is ten tolerances and more away from BGK's result
        # (1.9e-4 .. 3.7e-4 on these states), so a kernel that relaxed with tau alone could not pass below
        bgk = lt.BGKCollision(TAU)(sim._flow).numpy()
        assert np.abs(want - bgk).max() > 10 * ATOL["f32"]
    assert_close(got, want, dt, what=f"collide {lat} {dt} C = {constant}")
    assert f"lt::{lat.lower()}, 0, 3," in plan.kernel_name(), plan.kernel_name()


GOLDEN = [f"smagorinsky_{lat}_{kind}_{dt}" for lat in FIXTURE_LATTICES for kind in ("default", "strong")
          for dt in ("f64", "f32")]


@pytest.mark.parametrize("name", GOLDEN)
def test_collide_and_steps_against_the_reference_vectors(name):
    """the reference's collided field, and its populations after 1, 2, 3 and 10 steps through lt_run"""
    g = golden(name)
    _, lat, _, dt = name.split("_")
    lat = lat.upper()
    res = [int(r) for r in g["resolution"]]
    tau, constant = float(g["tau"]), float(g["constant"])
    plan = smagorinsky_plan(lat, dt, res, constant)
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
    _case("one-d1q3-f64", "D1Q3", "f64", [40], {}, "lbm_kernel<double, lt::d1q3, 0, 3,", "one"),
    _case("one-d2q9-f32", "D2Q9", "f32", [12, 10], {}, "lbm_kernel<float, lt::d2q9, 0, 3,", "one"),
    # a grid the many-step and the 2-D two-step kernels take with BGK: neither has this collision
    _case("one-d2q9-f64-tileable", "D2Q9", "f64", [16, 128], {"two_step": 1, "many_step": 1},
          "lbm_kernel<double, lt::d2q9, 0, 3,", "one"),
    _case("one-d3q15-f64", "D3Q15", "f64", [5, 6, 7], {}, "lbm_kernel<double, lt::d3q15, 0, 3,", "one"),
    _case("one-d3q15-f32-tileable", "D3Q15", "f32", [6, 16, 128], TWO, "lbm_kernel<float, lt::d3q15, 0, 3,", "one"),
    _case("one-d3q19-f32", "D3Q19", "f32", [6, 5, 8], {}, "lbm_kernel<float, lt::d3q19, 0, 3,", "one"),
    _case("one-d3q19-f64-tileable", "D3Q19", "f64", [5, 24, 96], TWO, "lbm_kernel<double, lt::d3q19, 0, 3,", "one"),
    _case("one-d3q27-f32-tileable", "D3Q27", "f32", [6, 12, 128], TWO, "lbm_kernel<float, lt::d3q27, 0, 3,", "one"),
    _case("one-d3q27-f64", "D3Q27", "f64", [4, 6, 5], {}, "lbm_kernel<double, lt::d3q27, 0, 3,", "one"),
    # automatic mode pairs steps only in the streaming regime (populations beyond the caches), as for BGK
    _case("one-d3q19-f32-tileable-automatic", "D3Q19", "f32", [6, 24, 192], {},
          "lbm_kernel<float, lt::d3q19, 0, 3,", "one"),
    _case("lbm2-d3q19-f32-3x3-tiles", "D3Q19", "f32", [6, 24, 192], TWO, "lbm2_kernel<float, lt::d3q19, 0, 3, 64, 8,", "two"),
    _case("lbm2-d3q19-f32-48x64x256", "D3Q19", "f32", [48, 64, 256], TWO, "lbm2_kernel<float, lt::d3q19, 0, 3, 64, 8,", "two"),
]


@pytest.mark.parametrize("lat,dt,res,switches,kernel,launches", RUNS)
def test_lt_run_path_against_the_cpu_path(lat, dt, res, switches, kernel, launches):
    constant = 1.0
    f0 = perturbed_state(lat, res, TORCH_DT[dt], 3)
    plan = smagorinsky_plan(lat, dt, res, constant)
    setters = {"two_step": plan.set_two_step, "many_step": plan.set_many_step}
    for key, value in switches.items():
        setters[key](value)
    assert plan.kernel_name().startswith(kernel), plan.kernel_name()
    if launches == "two":
        assert plan.two_step_admitted() is None
    sim, want, done = reference(lat, f0, constant), {}, 0
    for n in STEPS:
        sim.step(n - done)
        done = n
        want[n] = sim.f.numpy().copy()
    for n in STEPS:
        got = run(plan, f0, n)
        assert plan.last_run_info() == expected_launches(launches, n - 1, False), (n, plan.last_run_info())
        assert_close(got, want[n], dt, n, what=f"{lat} {dt} {res} n = {n}")
    # 3 + 5 through lt_continue from the post-collision populations lt_run leaves in its other buffer
    a = dev(f0)
    result, fstar = plan.run(a, torch.empty_like(a), TAU, 3)
    out, _ = plan.run(fstar, result, TAU, 5, from_fstar=True)
    torch.cuda.synchronize()
    assert plan.last_run_info() == expected_launches(launches, 5, False), plan.last_run_info()
    assert_close(out.cpu().numpy(), want[8], dt, 8, what=f"{lat} {dt} {res} 3 + 5")


# --------------------------------------------------------------------------- one kernel against another, bit for bit
@pytest.mark.parametrize("seg", [1, 2, 7, 0])
@pytest.mark.parametrize("layout", ["reference", "slab"])
def test_two_step_launch_is_bit_identical_to_two_single_steps(layout, seg):
    from lettuce_amd._native import LAYOUT_SLAB
    if layout == "reference":
        plan = smagorinsky_plan("D3Q19", "f32", [14, 16, 128], 1.0)
    else:
        plan = smagorinsky_plan("D3Q19", "f32", [128, 16, 14], 1.0, layout=LAYOUT_SLAB)
    assert plan.f_shape == [19, 14, 16, 128]
    f = dev(perturbed_state("D3Q19", [14, 16, 128], torch.float32, 5))
    a, b, c = torch.empty_like(f), torch.empty_like(f), torch.full_like(f, float("nan"))
    plan.stream_collide(f, a, TAU)
    plan.stream_collide(a, b, TAU)
    plan.set_two_step(1, seg)
    assert plan.kernel_name().startswith(f"lbm2_kernel<float, lt::d3q19, {0 if layout == 'reference' else 1}, 3, 64, 8,")
    plan.stream_collide_twice(f, c, TAU)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(c.cpu().numpy(), b.cpu().numpy())
    assert float((b - f).abs().max()) > 1e-4                       # the steps did something


def test_automatic_mode_pairs_the_steps_of_a_large_grid():
    """populations beyond the caches (2 x 19 x 4 B x 1 M nodes = 160 MB): lt_run takes the two-step kernel on the
    engine's padded buffers by itself, and the result is what one-step launches give, bit for
    bit -- it does not depend on how a caller splits the steps into batches"""
    res = [16, 256, 256]
    f0 = perturbed_state("D3Q19", res, torch.float32, 19)
    plan = smagorinsky_plan("D3Q19", "f32", res, 1.0)
    assert plan.kernel_name().startswith("lbm2_kernel<float, lt::d3q19, 0, 3, 64, 8,"), plan.kernel_name()
    assert plan.resident_enabled()[0]
    got = run(plan, f0, 6)
    assert plan.last_run_info() == expected_launches("two", 5, False)
    single = smagorinsky_plan("D3Q19", "f32", res, 1.0)
    single.set_two_step(0)
    want = run(single, f0, 6)
    assert single.last_run_info() == expected_launches("one", 5, False)
    np.testing.assert_array_equal(got, want)
    for other in ("D3Q27", "D3Q15"):                               # no such kernel: one step per launch, dense buffers
        plan = smagorinsky_plan(other, "f32", res, 1.0)
        assert plan.kernel_name().startswith(f"lbm_kernel<float, lt::{other.lower()}, 0, 3,") and not plan.resident_enabled()[0]


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("lat", list(SMALL))
def test_fused_is_bit_identical_to_stream_then_collide(lat, dt):
    res = SMALL[lat]
    plan = smagorinsky_plan(lat, dt, res, 1.0)
    f = dev(perturbed_state(lat, res, TORCH_DT[dt], 7))
    a, b, c = torch.empty_like(f), torch.empty_like(f), torch.empty_like(f)
    plan.stream(f, a)
    plan.collide(a, b, TAU)
    plan.stream_collide(f, c, TAU)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(c.cpu().numpy(), b.cpu().numpy())


def test_fused_is_bit_identical_to_stream_then_collide_with_boundaries():
    lat, res, dtype = "D3Q19", [6, 7, 8], torch.float32
    f0, ncm, nsm, entries = _masked_case(lat, res, dtype, (0, 1), 21, with_field=True)
    plan = smagorinsky_plan(lat, "f32", res, 1.0, entries)
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
def test_resident_is_bit_identical_to_dense(lat, res, switches, launches):
    f0 = perturbed_state(lat, res, torch.float32, 9)
    dense = smagorinsky_plan(lat, "f32", res, 1.0)
    resident = smagorinsky_plan(lat, "f32", res, 1.0)
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
def _two_outlets(lat, res, dtype, seed, with_field):
    """_masked_case with an outlet on +x, and a second one on -y (their planes meet in an edge)"""
    L = orc.LATTICES[lat]
    f0, ncm, nsm, entries = _masked_case(lat, res, dtype, (0, 1), seed, with_field=with_field)
    direction = [0] * L.d
    direction[1] = -1
    m, sm = orc.abb_masks(f0.shape, orc.OracleBoundary("abb_outlet", direction=direction), L)
    nsm |= sm.to(torch.uint8)
    entries = entries + [{"kind": "abb_outlet", "axis": 1, "side": -1}]
    ncm[m] = len(entries)
    return f0, ncm, nsm, entries


MASKED = [("D2Q9", [12, 10], "f64", 1, False), ("D2Q9", [16, 64], "f32", 1, True), ("D2Q9", [12, 10], "f64", 2, True),
          ("D3Q15", [5, 6, 7], "f64", 1, True), ("D3Q19", [6, 8, 64], "f32", 1, False), ("D3Q19", [6, 7, 8], "f64", 2, False),
          ("D3Q19", [6, 16, 64], "f32", 2, True), ("D3Q27", [5, 6, 7], "f32", 1, True), ("D3Q27", [4, 6, 5], "f64", 2, False)]


MASKED_LAYOUTS = [m + (layout,) for m in MASKED for layout in ("reference", "slab") if layout == "reference" or len(m[1]) == 3]


@pytest.mark.parametrize("lat,res,dt,outlets,with_field,layout", MASKED_LAYOUTS,
                         ids=[f"{m[0]}-{'x'.join(map(str, m[1]))}-{m[2]}-{m[3]}-outlets-{m[5]}" for m in MASKED_LAYOUTS])
def test_masked_plans_against_the_cpu_path(lat, res, dt, outlets, with_field, layout):
    """bounce-back, equilibrium (table / per-node field) and one or two anti-bounce-back outlets: lt_run, which
    must stay on the one-step kernel (the masked two-step kernels do not have this collision), against the CPU path;
    in the slab layout (periodic, no ghost planes) the same plan in the other memory order"""
    from lettuce_amd._native import LAYOUT_SLAB
    dtype, constant = TORCH_DT[dt], 1.0
    make = _masked_case if outlets == 1 else _two_outlets
    args = (lat, res, dtype, (0, 1), 40) if outlets == 1 else (lat, res, dtype, 40)
    f0, ncm, nsm, entries = make(*args, with_field=with_field)
    if layout == "reference":
        plan = smagorinsky_plan(lat, dt, res, constant, entries)
        plan.set_masks(dev(ncm), dev(nsm))
        state = f0
    else:
        slab_entries = [dict(e, field=e["field"].permute(0, 3, 2, 1).contiguous()) if "field" in e else e for e in entries]
        plan = smagorinsky_plan(lat, dt, res, constant, slab_entries, layout=LAYOUT_SLAB)
        plan.set_masks(dev(ncm.permute(2, 1, 0)), dev(nsm.permute(0, 3, 2, 1)))
        state = f0.permute(0, 3, 2, 1)
    plan.set_two_step(1)
    assert plan.two_step_admitted() is not None
    assert plan.kernel_name().startswith(f"lbm_kernel<{'float' if dt == 'f32' else 'double'}, lt::{lat.lower()}, "
                                         f"{0 if layout == 'reference' else 1}, 3, true, true, true,"), plan.kernel_name()
    sim, done = reference(lat, f0, constant, entries=entries, ncm=ncm, nsm=nsm), 0
    for n in (1, 2, 5):
        sim.step(n - done)
        done = n
        got = run(plan, state, n)
        assert plan.last_run_info() == expected_launches("one", n - 1, True), plan.last_run_info()
        if layout == "slab":
            got = got.transpose(0, 3, 2, 1)
        assert_close(got, sim.f.numpy(), dt, n, outlet=True, what=f"{lat} {dt} {layout} {outlets} outlet(s) n = {n}")


@pytest.mark.parametrize("name,stencil,dt", OBSTACLES, ids=[o[0] for o in OBSTACLES])
def test_obstacle_through_the_simulation_matches_the_reference_vectors(name, stencil, dt):
    g = golden(name)
    flow, sim = obstacle_from(g, stencil, lt.Context("cuda:0", TORCH_DT[dt], use_native=True))
    assert sim._native is not None
    done = 0
    for n in (1, 2, 10):
        sim(n - done)
        done = n
        assert_close(flow.f.cpu().numpy(), g[f"f{n}"], dt, n, outlet=True, what=f"{name} f{n}")
    assert ", 3, true, true, true," in sim._native.plan.kernel_name(), sim._native.plan.kernel_name()   # fused, masked
    assert sim._native.plan.last_run_info()["two_step_launches"] == 0


# --------------------------------------------------------------------------- the slab layout
def test_slab_plane_launches_reproduce_the_reference_layout_bit_for_bit():
    """lt_stream_collide_planes and the packed plane pair of a slab plan (one ghost plane per side, filled as the
    periodic neighbours would) against lt_stream_collide of the same state in the reference layout"""
    from lettuce_amd._native import LAYOUT_SLAB
    res = [10, 6, 8]                                                 # x, y, z
    f0 = perturbed_state("D3Q19", res, torch.float32, 13)
    ref = smagorinsky_plan("D3Q19", "f32", res, 1.0)
    want = ref.stream_collide(dev(f0), torch.empty_like(dev(f0)), TAU).permute(0, 3, 2, 1).contiguous()   # [q, z, y, x]
    slab = smagorinsky_plan("D3Q19", "f32", res, 1.0, layout=LAYOUT_SLAB, ghost_planes=1)
    core = dev(f0.permute(0, 3, 2, 1))
    f = torch.cat([core[:, -1:], core, core[:, :1]], dim=1).contiguous()
    assert list(f.shape) == slab.f_shape
    nz = res[2]
    out = torch.full_like(f, float("nan"))
    slab.stream_collide_planes(f, out, TAU, 1, nz + 1)
    torch.cuda.synchronize()
    assert torch.equal(out[:, 1:nz + 1], want)
    assert ", 1, 3, true, true, false," in slab.kernel_name()
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
def test_changing_the_constant_between_calls_needs_no_new_plan():
    context = lt.Context("cuda:0", torch.float32, use_native=True)

    def simulation(constant, f=None):
        flow = lt.TaylorGreenVortex(context, [16, 16, 16], 1600, 0.1, lt.D3Q19())
        g = torch.Generator().manual_seed(2)
        noise = 1 + 0.1 * (2 * torch.rand(flow.f.shape, generator=g) - 1)
        flow.f = flow.f * noise.to(flow.f.device) if f is None else f.clone()
        collision = lt.SmagorinskyCollision(TAU, constant)
        return flow, collision, lt.Simulation(flow, collision, [])

    flow, collision, sim = simulation(0.17)
    plan = sim._native.plan
    sim(3)
    after3 = flow.f.clone()
    collision.constant = 1.0
    sim(3)
    assert sim._native.plan is plan
    fresh_flow, _, fresh = simulation(1.0, after3)
    fresh(3)
    assert torch.equal(flow.f, fresh_flow.f)
    same_flow, _, same = simulation(0.17, after3)
    same(3)
    assert float((flow.f - same_flow.f).abs().max()) > 50 * ATOL["f32"]
    # ... and without looking at flow.f in between: the second batch carries on from what the first one left
    flow2, collision2, sim2 = simulation(0.17)
    sim2(3)
    collision2.constant = 1.0
    sim2(3)
    assert torch.equal(flow2.f, flow.f)


def test_engine_collide_of_the_operator_follows_its_constant():
    """collision(flow) on a native context is the engine's collide kernel: one plan for the kind, the constant handed
    to it before every launch"""
    context = lt.Context("cuda:0", torch.float64, use_native=True)
    flow = lt.TaylorGreenVortex(context, [12, 10], 100, 0.05, lt.D2Q9())
    f0 = perturbed_state("D2Q9", [12, 10], torch.float64, 17)
    flow.f = dev(f0)
    for constant in (0.17, 1.0, 0.17):
        got = lt.SmagorinskyCollision(TAU, constant)(flow).cpu().numpy()
        sim = reference("D2Q9", f0, constant)
        assert_close(got, sim._collision(sim.f).numpy(), "f64", what=f"operator, C = {constant}")
    assert set(flow._collision_plans) == {"smagorinsky"}


# --------------------------------------------------------------------------- the C ABI's refusals
def test_set_smagorinsky_validates_and_leaves_the_plan_unchanged():
    from lettuce_amd._native import NativeEngineError
    res = [6, 5, 8]
    f0 = perturbed_state("D3Q19", res, torch.float32, 3)
    plan = smagorinsky_plan("D3Q19", "f32", res, 0.4)
    before = run(plan, f0, 3)
    for bad in (-0.1, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(NativeEngineError, match="Smagorinsky constant"):
            plan.set_smagorinsky(bad)
        np.testing.assert_array_equal(run(plan, f0, 3), before)
    with pytest.raises(NativeEngineError, match="not Smagorinsky"):
        plan_for("D3Q19", torch.float32, "bgk", res).set_smagorinsky(0.2)
    default = run(smagorinsky_plan("D3Q19", "f32", res, 0.17), f0, 3)
    from lettuce_amd._native import Plan
    np.testing.assert_array_equal(run(Plan("D3Q19", torch.float32, "smagorinsky", res), f0, 3), default)   # 0.17 until set
    plan.set_smagorinsky(0.0)                                        # no eddy viscosity: BGK's relaxation
    assert_close(run(plan, f0, 3), run(plan_for("D3Q19", torch.float32, "bgk", res), f0, 3), "f32", 3, what="C = 0")


def test_two_step_admission():
    """D3Q19 fp64, D3Q27, masked plans and slabs report LT_ERR_UNSUPPORTED with a reason, and lt_run on them counts
    one-step launches only"""
    from lettuce_amd._native import LAYOUT_SLAB, NativeEngineError
    cases = [("D3Q19", "f64", [5, 24, 96]), ("D3Q27", "f32", [6, 12, 128]), ("D3Q15", "f32", [6, 16, 128])]
    for lat, dt, res in cases:
        plan = smagorinsky_plan(lat, dt, res, 1.0)
        plan.set_two_step(1)
        assert "no two-step kernel for this lattice / dtype / collision" in plan.two_step_admitted()
        f = dev(perturbed_state(lat, res, TORCH_DT[dt], 3))
        with pytest.raises(NativeEngineError, match="no kernel for layout 0 collision 3 mode 3"):
            plan.stream_collide_twice(f, torch.empty_like(f), TAU)
        run(plan, f.cpu(), 5)
        assert plan.last_run_info() == expected_launches("one", 4, False)
    res = [6, 16, 64]
    f0, ncm, nsm, entries = _masked_case("D3Q19", res, torch.float32, (0, 1), 21)
    masked = smagorinsky_plan("D3Q19", "f32", res, 1.0, entries)
    masked.set_masks(dev(ncm), dev(nsm))
    masked.set_two_step(1)
    assert "no two-step kernel" in masked.two_step_admitted()
    run(masked, f0, 5)
    assert masked.last_run_info() == expected_launches("one", 4, True)
    slab = smagorinsky_plan("D3Q19", "f32", [64, 16, 12], 1.0, layout=LAYOUT_SLAB, ghost_planes=2)
    assert "plain two-step sweep of periodic plans only" in slab.two_step_admitted()
    f = torch.rand(slab.f_shape, device="cuda") * 0.01 + 0.04
    with pytest.raises(NativeEngineError, match="periodic plans only"):
        slab.stream_collide_twice_planes(f, torch.empty_like(f), TAU, 2, 14)
    # the same plan with BGK has the launch: the refusal is this collision's
    bgk = plan_for("D3Q19", torch.float32, "bgk", [6, 24, 192])
    bgk.set_two_step(1)
    assert bgk.two_step_admitted() is None


def test_two_step_slab_driver_refuses_the_collision_and_the_one_step_driver_takes_it():
    from lettuce_amd._slab import ZSlab, SlabSimulation, TwoStepSlabSimulation
    context = lt.Context("cuda:0", torch.float32, use_native=True)
    res, tau, constant = [64, 8, 12], TAU, 1.0

    def slab_flow():
        slab = ZSlab(res, 0, 1)
        flow = lt.TaylorGreenVortex(context, slab.extended_resolution, 400, 0.1, lt.D3Q19(), slab=slab)
        return slab, flow

    slab, flow = slab_flow()
    with pytest.raises(lt.LettuceException, match="plain two-step sweep of periodic plans only"):
        TwoStepSlabSimulation(flow, lt.SmagorinskyCollision(tau, constant), slab)
    slab, flow = slab_flow()
    whole = lt.TaylorGreenVortex(lt.Context("cpu", torch.float64, use_native=False), res, 400, 0.1, lt.D3Q19())
    g = torch.Generator().manual_seed(6)
    noise = 1 + 0.1 * (2 * torch.rand(whole.f.shape, generator=g, dtype=torch.float64) - 1)
    f0 = (whole.f * noise).float()
    h = slab.halo
    flow.f = dev(torch.cat([f0[..., -h:], f0, f0[..., :h]], dim=-1))
    sim = SlabSimulation(flow, lt.SmagorinskyCollision(tau, constant), slab)
    assert ", 1, 3, true, true, false," in sim.engine.kernel_name()
    sim(5)
    ref = reference("D3Q19", f0, constant, tau)
    ref.step(5)
    assert_close(sim.gather_f().cpu().numpy(), ref.f.numpy(), "f32", 5, what="slab driver, 5 steps")
