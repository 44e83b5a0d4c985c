"""Body forces of the HIP engine (lt_plan_set_force): Guo and Shan-Chen inside the BGK and Smagorinsky kernels, in the
manner of test_gpu_smagorinsky.py.

The CPU reference is the mirror's torch path (lettuce_amd.Guo / ShanChen in BGKCollision / SmagorinskyCollision on a CPU
context, pinned to the reference's own vectors by test_force_host.py) in float64, stepping the same (fp32: the same
fp32) initial state -- with the plan's boundaries through the oracle's boundary operators -- plus the vectors of
tests/golden.  The acceleration has three different components: a wrong axis permutation shows.

Tolerances are the project's own: ATOL 1e-12 / 1e-5 times max(1, |f|max), times max(1, n / 10) in fp32, times 10 with
an anti-bounce-back outlet.  The engine sums the source term in another order than the reference, so it agrees at
rounding level, not bit for bit; one engine kernel against another is bit for bit.  Every comparison prints its
largest difference before it asserts.
"""
import numpy as np
import pytest
import torch

import lettuce_amd as lt
from conftest import golden, TORCH_DT
from oracle import lettuce_oracle as orc
from test_gpu_engine import ATOL, _masked_case, dev, plan_for
from test_gpu_paths_vs_oracle import _Oracle, _oracle_boundary, expected_launches, perturbed_state
from test_gpu_smagorinsky import MASKED_LAYOUTS, SMALL, STENCILS, _two_outlets, assert_close
from test_host_api import UniformFlow
from test_force_host import PERIODIC as GOLDEN, channel, parabola_error

pytestmark = pytest.mark.gpu

ACCELERATION = (2e-3, -3e-3, 1e-3)
STEPS = (1, 2, 3, 8)
# (scheme, operator): tau, Smagorinsky constant, the kernels' COLL
SCHEMES = {("guo", "bgk"): (0.8, None, 5), ("guo", "smagorinsky"): (0.51, 1.0, 7), ("shanchen", "bgk"): (0.8, None, 5)}
SCHEME_IDS = ["-".join(k) for k in SCHEMES]
FLOAT = {"f32": "float", "f64": "double"}


def scales(scheme, tau):
    """(ueq_scale, source_scale) of lt_plan_set_force"""
    return (0.5, 1 - 1 / (2 * tau)) if scheme == "guo" else (tau, 0.0)


# --------------------------------------------------------------------------- the CPU reference
class _Reference(_Oracle):
    """the oracle's stepping and boundaries around the mirror's torch path of a collision with a force"""
    scheme, operator, constant, acceleration = "guo", "bgk", None, None

    def _collision(self, f, forced=True):
        flow = self.__dict__.get("_flow")
        if flow is None:
            context = lt.Context("cpu", f.dtype, use_native=False)
            flow = self._flow = UniformFlow(context, list(f.shape[1:]), 1, 0.01, STENCILS[self.lat.name]())
        flow.f = f
        force = None
        if forced:
            force = {"guo": lt.Guo, "shanchen": lt.ShanChen}[self.scheme](flow, self.tau, list(self.acceleration))
        if self.operator == "bgk":
            return lt.BGKCollision(self.tau, force=force)(flow)
        return lt.SmagorinskyCollision(self.tau, self.constant, force=force)(flow)


def reference(lat, f0, scheme, operator, acceleration=None, entries=(), ncm=None, nsm=None):
    L = orc.LATTICES[lat]
    tau, constant, _ = SCHEMES[(scheme, operator)]
    sim = _Reference(L, f0.double().clone(), operator, tau)
    sim.scheme, sim.operator, sim.constant = scheme, operator, constant
    sim.acceleration = ACCELERATION[:L.d] if acceleration is None else acceleration
    if ncm is not None:
        sim.boundaries = [_oracle_boundary(L, e, f0.dtype) for e in entries]
        sim.no_collision_mask, sim.no_streaming_mask = ncm.cpu(), nsm.cpu()
    return sim


def forced_plan(lat, dt, res, scheme, operator, entries=(), acceleration=None, **kwargs):
    from lettuce_amd._native import Plan
    tau, constant, _ = SCHEMES[(scheme, operator)]
    plan = Plan(lat, TORCH_DT[dt], operator, res, entries, **kwargs)
    if constant is not None:
        plan.set_smagorinsky(constant)
    plan.set_force(ACCELERATION[:len(res)] if acceleration is None else acceleration, *scales(scheme, tau))
    return plan


def run(plan, f0, n, tau):
    a = dev(f0)
    out, _ = plan.run(a, torch.empty_like(a), tau, n)
    torch.cuda.synchronize()
    return out.cpu().numpy()


# --------------------------------------------------------------------------- lt_collide
@pytest.mark.parametrize("scheme,operator", list(SCHEMES), ids=SCHEME_IDS)
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("lat", list(SMALL))
def test_collide_against_the_cpu_path(lat, dt, scheme, operator):
    res = SMALL[lat]
    tau, _, coll = SCHEMES[(scheme, operator)]
    f0 = perturbed_state(lat, res, TORCH_DT[dt], 11)
    plan = forced_plan(lat, dt, res, scheme, operator)
    got = plan.collide(dev(f0), torch.empty_like(dev(f0)), tau).cpu().numpy()
    sim = reference(lat, f0, scheme, operator)
    want = sim._collision(sim.f).numpy()
    # the state and the acceleration tell the operator from the unforced one: a kernel that ignored the force could
    # not pass below
    unforced = sim._collision(sim.f, forced=False).numpy()
    gap = float(np.abs(want - unforced).max())
    print(f"the CPU path's distance from the unforced operator: {gap:.2e}")
    assert gap > 10 * ATOL["f32"]
    assert_close(got, want, dt, what=f"collide {lat} {dt} {scheme} {operator}")
    assert f"lt::{lat.lower()}, 0, {coll}," in plan.kernel_name(), plan.kernel_name()


@pytest.mark.parametrize("name", GOLDEN)
def test_collide_and_steps_against_the_reference_vectors(name):
    """the reference's collided field, and its populations after 1, 2, 3 and 10 steps through lt_run"""
    g = golden(name)
    _, scheme, operator, lat, dt = name.split("_")
    lat = lat.upper()
    res = [int(r) for r in g["resolution"]]
    tau = float(g["tau"])
    assert (tau, scales(scheme, tau)) == (SCHEMES[(scheme, operator)][0], (float(g["ueq_scale"]), float(g["source_scale"])))
    plan = forced_plan(lat, dt, res, scheme, operator, acceleration=[float(a) for a in g["acceleration"]])
    f0 = torch.tensor(g["f0"])
    got = plan.collide(dev(f0), torch.empty_like(dev(f0)), tau).cpu().numpy()
    assert_close(got, g["collided"], dt, what=f"{name} collided")
    for n in (1, 2, 3, 10):
        assert_close(run(plan, f0, n, tau), g[f"f{n}"], dt, n, what=f"{name} f{n}")


# --------------------------------------------------------------------------- lt_run: kernel, launches, result
def _case(cid, lat, dt, res, scheme, operator, switches, launches):
    return pytest.param(lat, dt, res, scheme, operator, switches, launches, id=cid)


TWO = {"two_step": 1}
ONE_STEP = [_case(f"one-{lat.lower()}-{dt}-{scheme}-{operator}", lat, dt, SMALL[lat], scheme, operator, {}, "one")
            for lat in SMALL for dt in ("f64", "f32") for scheme, operator in SCHEMES]
RUNS = ONE_STEP + [
    # grids the many-step, the 2-D two-step and (with BGK) the 3-D two-step kernels of other lattices take: a forced
    # plan has none of them
    _case("one-d2q9-f64-tileable", "D2Q9", "f64", [16, 128], "guo", "bgk", {"two_step": 1, "many_step": 1}, "one"),
    _case("one-d2q9-f32-tileable", "D2Q9", "f32", [16, 128], "shanchen", "bgk", {"two_step": 1, "many_step": 1}, "one"),
    _case("one-d3q15-f32-tileable", "D3Q15", "f32", [6, 16, 128], "guo", "bgk", TWO, "one"),
    _case("one-d3q27-f32-tileable", "D3Q27", "f32", [6, 12, 128], "guo", "bgk", TWO, "one"),
    _case("one-d3q19-f64-tileable", "D3Q19", "f64", [5, 24, 96], "guo", "bgk", TWO, "one"),
    # Smagorinsky with a force does not fit the sweep's registers: one step per launch
    _case("one-d3q19-f32-tileable-smagorinsky", "D3Q19", "f32", [6, 24, 192], "guo", "smagorinsky", TWO, "one"),
    # never automatic
    _case("one-d3q19-f32-tileable-automatic", "D3Q19", "f32", [6, 24, 192], "guo", "bgk", {}, "one"),
    _case("lbm2-d3q19-f32-3x3-tiles-guo", "D3Q19", "f32", [6, 24, 192], "guo", "bgk", TWO, "two"),
    _case("lbm2-d3q19-f32-3x3-tiles-shanchen", "D3Q19", "f32", [6, 24, 192], "shanchen", "bgk", TWO, "two"),
    _case("lbm2-d3q19-f32-48x64x256", "D3Q19", "f32", [48, 64, 256], "guo", "bgk", TWO, "two"),
]


@pytest.mark.parametrize("lat,dt,res,scheme,operator,switches,launches", RUNS)
def test_lt_run_path_against_the_cpu_path(lat, dt, res, scheme, operator, switches, launches):
    tau, _, coll = SCHEMES[(scheme, operator)]
    f0 = perturbed_state(lat, res, TORCH_DT[dt], 3)
    plan = forced_plan(lat, dt, res, scheme, operator)
    setters = {"two_step": plan.set_two_step, "many_step": plan.set_many_step}
    for key, value in switches.items():
        setters[key](value)
    if launches == "two":
        kernel = f"lbm2_kernel<float, lt::d3q19, 0, {coll}, 64, 8,"
        assert plan.two_step_admitted() is None
    else:
        kernel = f"lbm_kernel<{FLOAT[dt]}, lt::{lat.lower()}, 0, {coll},"
        if switches:
            assert "body force" in plan.two_step_admitted()
    assert plan.kernel_name().startswith(kernel), plan.kernel_name()
    sim, want, done = reference(lat, f0, scheme, operator), {}, 0
    for n in STEPS:
        sim.step(n - done)
        done = n
        want[n] = sim.f.numpy().copy()
    for n in STEPS:
        got = run(plan, f0, n, tau)
        assert plan.last_run_info() == expected_launches(launches, n - 1, False), (n, plan.last_run_info())
        assert_close(got, want[n], dt, n, what=f"{lat} {dt} {res} n = {n}")
    # 3 + 5 through lt_continue from the post-collision populations lt_run leaves in its other buffer
    a = dev(f0)
    result, fstar = plan.run(a, torch.empty_like(a), tau, 3)
    out, _ = plan.run(fstar, result, tau, 5, from_fstar=True)
    torch.cuda.synchronize()
    assert plan.last_run_info() == expected_launches(launches, 5, False), plan.last_run_info()
    assert_close(out.cpu().numpy(), want[8], dt, 8, what=f"{lat} {dt} {res} 3 + 5")


# --------------------------------------------------------------------------- one kernel against another, bit for bit
@pytest.mark.parametrize("seg", [1, 2, 7, 0])
@pytest.mark.parametrize("layout", ["reference", "slab"])
def test_two_step_launch_is_bit_identical_to_two_single_steps(layout, seg):
    from lettuce_amd._native import LAYOUT_SLAB
    tau = 0.8
    if layout == "reference":
        plan = forced_plan("D3Q19", "f32", [14, 16, 128], "guo", "bgk")
    else:
        plan = forced_plan("D3Q19", "f32", [128, 16, 14], "guo", "bgk", layout=LAYOUT_SLAB)
    assert plan.f_shape == [19, 14, 16, 128]
    f = dev(perturbed_state("D3Q19", [14, 16, 128], torch.float32, 5))
    a, b, c = torch.empty_like(f), torch.empty_like(f), torch.full_like(f, float("nan"))
    plan.stream_collide(f, a, tau)
    plan.stream_collide(a, b, tau)
    plan.set_two_step(1, seg)
    assert plan.kernel_name().startswith(f"lbm2_kernel<float, lt::d3q19, {0 if layout == 'reference' else 1}, 5, 64, 8,")
    plan.stream_collide_twice(f, c, tau)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(c.cpu().numpy(), b.cpu().numpy())
    assert float((b - f).abs().max()) > 1e-4                       # the steps did something


@pytest.mark.parametrize("scheme,operator", list(SCHEMES), ids=SCHEME_IDS)
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("lat", list(SMALL))
def test_fused_is_bit_identical_to_stream_then_collide(lat, dt, scheme, operator):
    res = SMALL[lat]
    tau = SCHEMES[(scheme, operator)][0]
    plan = forced_plan(lat, dt, res, scheme, operator)
    f = dev(perturbed_state(lat, res, TORCH_DT[dt], 7))
    a, b, c = torch.empty_like(f), torch.empty_like(f), torch.empty_like(f)
    plan.stream(f, a)
    plan.collide(a, b, tau)
    plan.stream_collide(f, c, tau)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(c.cpu().numpy(), b.cpu().numpy())


@pytest.mark.parametrize("scheme,operator", list(SCHEMES), ids=SCHEME_IDS)
@pytest.mark.parametrize("lat,res,dt", [("D3Q19", [6, 7, 8], "f32"), ("D2Q9", [12, 10], "f64"), ("D3Q27", [4, 6, 5], "f64")])
def test_fused_is_bit_identical_to_stream_then_collide_with_boundaries(lat, res, dt, scheme, operator):
    tau = SCHEMES[(scheme, operator)][0]
    f0, ncm, nsm, entries = _masked_case(lat, res, TORCH_DT[dt], (0, 1), 21, with_field=True)
    plan = forced_plan(lat, dt, res, scheme, operator, entries)
    plan.set_masks(dev(ncm), dev(nsm))
    f = dev(f0)
    a, b, c = torch.empty_like(f), torch.empty_like(f), torch.empty_like(f)
    plan.stream(f, a)
    plan.collide(a, b, tau)
    plan.stream_collide(f, c, tau)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(c.cpu().numpy(), b.cpu().numpy())


@pytest.mark.parametrize("lat,res,operator,switches,launches",
                         [("D3Q19", [6, 24, 192], "bgk", TWO, "two"), ("D3Q19", [6, 24, 192], "bgk", {}, "one"),
                          ("D3Q19", [6, 24, 192], "smagorinsky", TWO, "one"), ("D3Q27", [4, 6, 5], "bgk", {}, "one")])
def test_resident_is_bit_identical_to_dense(lat, res, operator, switches, launches):
    tau = SCHEMES[("guo", operator)][0]
    f0 = perturbed_state(lat, res, torch.float32, 9)
    dense = forced_plan(lat, "f32", res, "guo", operator)
    resident = forced_plan(lat, "f32", res, "guo", operator)
    for plan in (dense, resident):
        if switches:
            plan.set_two_step(switches["two_step"])
    dense.set_resident(0)
    resident.set_resident(1)
    assert resident.resident_enabled()[0] and not dense.resident_enabled()[0]
    want = run(dense, f0, 8, tau)
    f = dev(f0)
    resident.resident_load(f, tau)
    resident.resident_advance(tau, 7)
    assert resident.last_run_info() == expected_launches(launches, 7, False)
    got = resident.resident_store(torch.empty_like(f))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("scheme,operator", list(SCHEMES), ids=SCHEME_IDS)
def test_slab_plane_launches_reproduce_the_reference_layout_bit_for_bit(scheme, operator):
    """lt_stream_collide_planes and the packed plane pair of a slab plan (one ghost plane per side, filled as the
    periodic neighbours would) against lt_stream_collide of the same state in the reference layout: the acceleration
    reaches the kernel in the memory order of either layout"""
    from lettuce_amd._native import LAYOUT_SLAB
    tau, _, coll = SCHEMES[(scheme, operator)]
    res = [10, 6, 8]                                                 # x, y, z
    f0 = perturbed_state("D3Q19", res, torch.float32, 13)
    ref = forced_plan("D3Q19", "f32", res, scheme, operator)
    want = ref.stream_collide(dev(f0), torch.empty_like(dev(f0)), tau).permute(0, 3, 2, 1).contiguous()   # [q, z, y, x]
    slab = forced_plan("D3Q19", "f32", res, scheme, operator, layout=LAYOUT_SLAB, ghost_planes=1)
    core = dev(f0.permute(0, 3, 2, 1))
    f = torch.cat([core[:, -1:], core, core[:, :1]], dim=1).contiguous()
    assert list(f.shape) == slab.f_shape
    nz = res[2]
    out = torch.full_like(f, float("nan"))
    slab.stream_collide_planes(f, out, tau, 1, nz + 1)
    torch.cuda.synchronize()
    assert torch.equal(out[:, 1:nz + 1], want)
    assert f", 1, {coll}, true, true, false," in slab.kernel_name()
    # the plane pair, and the two boundary planes with the halo messages packed by the same launch
    out1 = torch.full_like(f, float("nan"))
    slab.stream_collide_plane_pair(f, out1, tau, 1, nz)
    up, down = slab.crossing(1), slab.crossing(-1)
    out2 = torch.full_like(f, float("nan"))
    pack_first = torch.empty([len(down), res[1], res[0]], device="cuda")
    pack_second = torch.empty([len(up), res[1], res[0]], device="cuda")
    slab.stream_collide_plane_pair_packed(f, out2, tau, 1, nz, pack_first, pack_second)
    torch.cuda.synchronize()
    assert torch.equal(out1[:, 1], want[:, 0]) and torch.equal(out1[:, nz], want[:, nz - 1])
    assert torch.equal(out2[:, 1], want[:, 0]) and torch.equal(out2[:, nz], want[:, nz - 1])
    assert torch.equal(pack_first, want[down, 0]) and torch.equal(pack_second, want[up, nz - 1])
    # a slab with two ghost planes has no forced two-step launch
    from lettuce_amd._native import NativeEngineError
    two = forced_plan("D3Q19", "f32", [64, 16, 12], scheme, operator, layout=LAYOUT_SLAB, ghost_planes=2)
    assert "body force" in two.two_step_admitted()
    g = torch.rand(two.f_shape, device="cuda") * 0.01 + 0.04
    with pytest.raises(NativeEngineError, match="body force"):
        two.stream_collide_twice_planes(g, torch.empty_like(g), tau, 2, 14)


@pytest.mark.parametrize("operator", ["bgk", "smagorinsky"])
@pytest.mark.parametrize("lat,dt,res,switches", [("D3Q19", "f32", [6, 24, 192], TWO), ("D3Q19", "f32", [6, 5, 8], {}),
                                                 ("D2Q9", "f64", [16, 128], {"many_step": 1}), ("D1Q3", "f64", [40], {})])
def test_removing_the_force_gives_the_plan_that_never_had_one(lat, dt, res, switches, operator):
    tau, constant, _ = SCHEMES[("guo", operator)]
    f0 = perturbed_state(lat, res, TORCH_DT[dt], 23)
    never = plan_for(lat, TORCH_DT[dt], operator, res)
    plan = forced_plan(lat, dt, res, "guo", operator)
    for p in (never, plan):
        if constant is not None:
            p.set_smagorinsky(constant)
        if "two_step" in switches:
            p.set_two_step(1)
        if "many_step" in switches:
            p.set_many_step(1)
    forced = run(plan, f0, 5, tau)
    forced_name = plan.kernel_name()
    plan.set_force(None)
    assert plan.kernel_name() == never.kernel_name() and forced_name != never.kernel_name()
    want = run(never, f0, 5, tau)
    np.testing.assert_array_equal(run(plan, f0, 5, tau), want)
    assert plan.last_run_info() == never.last_run_info()
    assert float(np.abs(forced - want).max()) > 10 * ATOL["f32"]
    a = dev(f0)
    np.testing.assert_array_equal(plan.collide(a, torch.empty_like(a), tau).cpu().numpy(),
                                  never.collide(a, torch.empty_like(a), tau).cpu().numpy())


@pytest.mark.parametrize("scheme,operator", list(SCHEMES), ids=SCHEME_IDS)
@pytest.mark.parametrize("lat,dt", [("D2Q9", "f64"), ("D3Q19", "f32"), ("D3Q27", "f64")])
def test_the_zero_vector_is_a_forced_plan_that_agrees_with_the_unforced_one(lat, dt, scheme, operator):
    res = SMALL[lat]
    tau, constant, coll = SCHEMES[(scheme, operator)]
    f0 = perturbed_state(lat, res, TORCH_DT[dt], 29)
    plan = forced_plan(lat, dt, res, scheme, operator, acceleration=[0.0] * len(res))
    assert f", 0, {coll}," in plan.kernel_name()
    unforced = plan_for(lat, TORCH_DT[dt], operator, res)
    if constant is not None:
        unforced.set_smagorinsky(constant)
    assert_close(run(plan, f0, 5, tau), run(unforced, f0, 5, tau), dt, 5, what=f"zero force {lat} {dt}")


# --------------------------------------------------------------------------- plans with boundaries
@pytest.mark.parametrize("scheme,operator", [("guo", "bgk"), ("guo", "smagorinsky")], ids=["guo-bgk", "guo-smagorinsky"])
@pytest.mark.parametrize("lat,res,dt,outlets,with_field,layout", MASKED_LAYOUTS,
                         ids=[f"{m[0]}-{'x'.join(map(str, m[1]))}-{m[2]}-{m[3]}-outlets-{m[5]}" for m in MASKED_LAYOUTS])
def test_masked_plans_against_the_cpu_path(lat, res, dt, outlets, with_field, layout, scheme, operator):
    """bounce-back, equilibrium (table / per-node field) and one or two anti-bounce-back outlets: lt_run, which
    must stay on the one-step kernel (no masked multi-step kernel takes a force), against the CPU path; in the slab
    layout (periodic, no ghost planes) the same plan in the other memory order"""
    from lettuce_amd._native import LAYOUT_SLAB
    dtype = TORCH_DT[dt]
    tau, _, coll = SCHEMES[(scheme, operator)]
    make = _masked_case if outlets == 1 else _two_outlets
    args = (lat, res, dtype, (0, 1), 40) if outlets == 1 else (lat, res, dtype, 40)
    f0, ncm, nsm, entries = make(*args, with_field=with_field)
    if layout == "reference":
        plan = forced_plan(lat, dt, res, scheme, operator, entries)
        plan.set_masks(dev(ncm), dev(nsm))
        state = f0
    else:
        slab_entries = [dict(e, field=e["field"].permute(0, 3, 2, 1).contiguous()) if "field" in e else e for e in entries]
        plan = forced_plan(lat, dt, res, scheme, operator, slab_entries, layout=LAYOUT_SLAB)
        plan.set_masks(dev(ncm.permute(2, 1, 0)), dev(nsm.permute(0, 3, 2, 1)))
        state = f0.permute(0, 3, 2, 1)
    plan.set_two_step(1)
    if len(res) == 2:
        plan.set_many_step(1)
    assert "body force" in plan.two_step_admitted()
    assert plan.kernel_name().startswith(f"lbm_kernel<{FLOAT[dt]}, lt::{lat.lower()}, "
                                         f"{0 if layout == 'reference' else 1}, {coll}, true, true, true,"), plan.kernel_name()
    sim, done = reference(lat, f0, scheme, operator, entries=entries, ncm=ncm, nsm=nsm), 0
    for n in (1, 2, 5):
        sim.step(n - done)
        done = n
        got = run(plan, state, n, tau)
        assert plan.last_run_info() == expected_launches("one", n - 1, True), plan.last_run_info()
        if layout == "slab":
            got = got.transpose(0, 3, 2, 1)
        assert_close(got, sim.f.numpy(), dt, n, outlet=True, what=f"{lat} {dt} {layout} {outlets} outlet(s) n = {n}")


@pytest.mark.parametrize("lat,res,dt", [("D2Q9", [12, 10], "f64"), ("D3Q19", [6, 7, 8], "f32")])
def test_a_forced_collide_leaves_boundary_nodes_alone(lat, res, dt):
    """bounce-back and equilibrium nodes away from the outlet plane come out of a forced collide exactly as out of the
    unforced plan's; the colliding nodes do not"""
    tau = 0.8
    f0, ncm, nsm, entries = _masked_case(lat, res, TORCH_DT[dt], (0, 1), 31)
    forced = forced_plan(lat, dt, res, "guo", "bgk", entries)
    unforced = plan_for(lat, TORCH_DT[dt], "bgk", res, entries)
    out = []
    for plan in (forced, unforced):
        plan.set_masks(dev(ncm), dev(nsm))
        out.append(plan.collide(dev(f0), torch.empty_like(dev(f0)), tau).cpu().numpy())
    kinds = np.array([0] + [{"bounce_back": 1, "equilibrium": 2, "abb_outlet": 3}[e["kind"]] for e in entries])[ncm.numpy()]
    boundary = (kinds == 1) | (kinds == 2)
    boundary[-1] = False                                            # the outlet plane (+x): its nodes see their neighbour
    assert boundary.sum() > 5
    np.testing.assert_array_equal(out[0][:, boundary], out[1][:, boundary])
    fluid = kinds == 0
    assert float(np.abs(out[0][:, fluid] - out[1][:, fluid]).max()) > 10 * ATOL["f32"]


# --------------------------------------------------------------------------- lt.Simulation
def test_poiseuille_through_the_simulation_matches_the_reference_vectors():
    g = golden("force_poiseuille2d_d2q9_f64")
    context = lt.Context("cuda:0", torch.float64, use_native=True)
    flow = lt.PoiseuilleFlow2D(context, [int(r) for r in g["resolution"]], float(g["reynolds"]), float(g["mach"]), lt.D2Q9())
    tau = flow.units.relaxation_parameter_lu
    force = lt.Guo(flow, tau, flow.acceleration)
    sim = lt.Simulation(flow, lt.BGKCollision(tau, force=force), [])
    assert sim._native is not None
    done = 0
    for n in (1, 2, 10):
        sim(n - done)
        done = n
        assert_close(flow.f.cpu().numpy(), g[f"f{n}"], "f64", n, what=f"poiseuille f{n}")
    assert_close(flow.u(acceleration=force.acceleration).cpu().numpy(), g["u10"], "f64", what="poiseuille u")
    assert ", 0, 5, true, true, true," in sim._native.plan.kernel_name(), sim._native.plan.kernel_name()   # fused, masked
    info = sim._native.plan.last_run_info()
    assert info["two_step_launches"] == 0 and info["many_step_launches"] == 0


def test_a_body_force_drives_the_parabolic_channel_profile_on_the_engine():
    """the channel of test_force_host.py in fp64: 4000 one-step launches on 64 nodes, the same 5e-3 of the peak
    velocity, and the populations of the CPU run"""
    context = lt.Context("cuda:0", torch.float64, use_native=True)
    flow, _ = channel(context)
    err = parabola_error(flow)
    print(f"distance from the parabola: {err:.3e} of the peak (bound 5e-3)")
    assert err < 5e-3
    cpu, _ = channel(lt.Context("cpu", torch.float64, use_native=False))
    assert_close(flow.f.cpu().numpy(), cpu.f.numpy(), "f64", 4000, what="channel, 4000 steps, engine against the CPU path")


def test_changing_the_acceleration_between_calls_needs_no_new_plan():
    context = lt.Context("cuda:0", torch.float32, use_native=True)
    first, second = [2e-3, -3e-3, 1e-3], [-1e-3, 2e-3, 3e-3]

    def simulation(acceleration, f=None):
        flow = lt.TaylorGreenVortex(context, [16, 16, 16], 1600, 0.1, lt.D3Q19())
        g = torch.Generator().manual_seed(2)
        noise = 1 + 0.1 * (2 * torch.rand(flow.f.shape, generator=g) - 1)
        flow.f = flow.f * noise.to(flow.f.device) if f is None else f.clone()
        force = lt.Guo(flow, 0.8, acceleration)
        return flow, force, lt.Simulation(flow, lt.BGKCollision(0.8, force=force), [])

    flow, force, sim = simulation(first)
    plan = sim._native.plan
    sim(3)
    after3 = flow.f.clone()
    force.acceleration = context.convert_to_tensor(second)
    sim(3)
    assert sim._native.plan is plan
    fresh_flow, _, fresh = simulation(second, after3)
    fresh(3)
    assert torch.equal(flow.f, fresh_flow.f)
    same_flow, _, same = simulation(first, after3)
    same(3)
    assert float((flow.f - same_flow.f).abs().max()) > 50 * ATOL["f32"]
    # ... and without looking at flow.f in between: the second batch does not carry on from a stale state
    flow2, force2, sim2 = simulation(first)
    sim2(3)
    force2.acceleration = context.convert_to_tensor(second)
    sim2(3)
    assert torch.equal(flow2.f, flow.f)


def test_engine_collide_of_the_operators_follows_the_force():
    """collision(flow) on a native context is the engine's collide kernel: one plan per kind, the force handed to it
    before every launch -- and taken away again for an operator without one"""
    context = lt.Context("cuda:0", torch.float64, use_native=True)
    flow = lt.TaylorGreenVortex(context, [12, 10], 100, 0.05, lt.D2Q9())
    f0 = perturbed_state("D2Q9", [12, 10], torch.float64, 17)
    flow.f = dev(f0)
    for acceleration in ((2e-3, -3e-3), (-1e-3, 4e-3), None):
        for scheme, operator in SCHEMES:
            tau, constant, _ = SCHEMES[(scheme, operator)]
            force = None
            if acceleration is not None:
                force = {"guo": lt.Guo, "shanchen": lt.ShanChen}[scheme](flow, tau, list(acceleration))
            collision = (lt.BGKCollision(tau, force=force) if operator == "bgk"
                         else lt.SmagorinskyCollision(tau, constant, force=force))
            got = collision(flow).cpu().numpy()
            sim = reference("D2Q9", f0, scheme, operator, acceleration=acceleration)
            want = sim._collision(sim.f, forced=acceleration is not None).numpy()
            assert_close(got, want, "f64", what=f"operator {scheme} {operator} a = {acceleration}")
    assert set(flow._collision_plans) == {"bgk", "smagorinsky"}


# --------------------------------------------------------------------------- the slab drivers
def test_slab_driver_takes_the_force_and_the_two_step_driver_refuses_it():
    from lettuce_amd._slab import ZSlab, SlabSimulation, TwoStepSlabSimulation
    context = lt.Context("cuda:0", torch.float32, use_native=True)
    res, tau = [64, 8, 12], 0.8

    def slab_flow():
        slab = ZSlab(res, 0, 1)
        flow = lt.TaylorGreenVortex(context, slab.extended_resolution, 400, 0.1, lt.D3Q19(), slab=slab)
        return slab, flow

    slab, flow = slab_flow()
    with pytest.raises(lt.LettuceException, match="body force"):
        TwoStepSlabSimulation(flow, lt.BGKCollision(tau, force=lt.Guo(flow, tau, list(ACCELERATION))), slab)
    slab, flow = slab_flow()
    whole = lt.TaylorGreenVortex(lt.Context("cpu", torch.float64, use_native=False), res, 400, 0.1, lt.D3Q19())
    g = torch.Generator().manual_seed(6)
    noise = 1 + 0.1 * (2 * torch.rand(whole.f.shape, generator=g, dtype=torch.float64) - 1)
    f0 = (whole.f * noise).float()
    h = slab.halo
    flow.f = dev(torch.cat([f0[..., -h:], f0, f0[..., :h]], dim=-1))
    sim = SlabSimulation(flow, lt.BGKCollision(tau, force=lt.Guo(flow, tau, list(ACCELERATION))), slab)
    assert ", 1, 5, true, true, false," in sim.engine.kernel_name()
    sim(5)
    ref = reference("D3Q19", f0, "guo", "bgk")
    ref.step(5)
    assert_close(sim.gather_f().cpu().numpy(), ref.f.numpy(), "f32", 5, what="slab driver, 5 steps")
    unforced = reference("D3Q19", f0, "guo", "bgk", acceleration=(0.0, 0.0, 0.0))
    unforced.step(5)
    assert float(np.abs(ref.f.numpy() - unforced.f.numpy()).max()) > 100 * ATOL["f32"]


# --------------------------------------------------------------------------- the C ABI's refusals
def test_set_force_validates_and_leaves_the_plan_unchanged():
    from lettuce_amd._native import NativeEngineError
    res, tau = [6, 5, 8], 0.8
    f0 = perturbed_state("D3Q19", res, torch.float32, 3)
    plan = forced_plan("D3Q19", "f32", res, "guo", "bgk")
    before = run(plan, f0, 3, tau)
    nan, inf = float("nan"), float("inf")
    for bad in ([nan, 0, 0], [0, inf, 0], [0, 0, -inf]):
        with pytest.raises(NativeEngineError, match="must be finite"):
            plan.set_force(bad, 0.5, 0.375)
        np.testing.assert_array_equal(run(plan, f0, 3, tau), before)
    for scale in ((nan, 0.375), (0.5, inf)):
        with pytest.raises(NativeEngineError, match="must be finite"):
            plan.set_force([1e-3, 0, 0], *scale)
        np.testing.assert_array_equal(run(plan, f0, 3, tau), before)
    with pytest.raises(NativeEngineError, match="components"):
        plan.set_force([1e-3, 0], 0.5, 0.375)
    # an unforced plan that refuses stays unforced
    unforced = plan_for("D3Q19", torch.float32, "bgk", res)
    name, want = unforced.kernel_name(), run(unforced, f0, 3, tau)
    with pytest.raises(NativeEngineError, match="must be finite"):
        unforced.set_force([nan, 0, 0], 0.5, 0.375)
    assert unforced.kernel_name() == name
    np.testing.assert_array_equal(run(unforced, f0, 3, tau), want)
    for lat, coll, r in (("D3Q27", "kbc", [4, 6, 5]), ("D3Q19", "none", res), ("D2Q9", "kbc", [12, 10])):
        other = plan_for(lat, torch.float32, coll, r)
        state = perturbed_state(lat, r, torch.float32, 3)
        name, want = other.kernel_name(), run(other, state, 3, tau)
        for acceleration in ([1e-3] * len(r), None):
            with pytest.raises(NativeEngineError, match="BGK and Smagorinsky") as refusal:
                other.set_force(acceleration, 0.5, 0.375)
            assert refusal.value.code == 2                           # LT_ERR_UNSUPPORTED
        assert other.kernel_name() == name
        np.testing.assert_array_equal(run(other, state, 3, tau), want)


def test_multi_step_entry_points_name_the_force():
    """the explicit entry points of the kernels that have no forced variant return LT_ERR_UNSUPPORTED with a reason
    that names the force; lt_run on those plans counts one-step launches only"""
    from lettuce_amd._native import NativeEngineError
    tau = 0.8
    two_d = forced_plan("D2Q9", "f64", [16, 128], "guo", "bgk")
    two_d.set_two_step(1)
    two_d.set_many_step(1)
    f = dev(perturbed_state("D2Q9", [16, 128], torch.float64, 3))
    reason = ("a body force (lt_plan_set_force) has the one-step kernels and the plain two-step sweep of periodic D3Q19 fp32 "
              "plans without masks only: no many-step, 2-D, masked, role-wave or slab two-step kernel takes it")
    for call, steps in ((lambda: two_d.stream_collide_many(f, torch.empty_like(f), tau, 4), "several steps"),
                        (lambda: two_d.stream_collide_twice(f, torch.empty_like(f), tau), "two steps")):
        with pytest.raises(NativeEngineError, match="body force") as refusal:
            call()
        assert refusal.value.code == 2                               # LT_ERR_UNSUPPORTED
        assert f"{steps} per launch: {reason}" in str(refusal.value), str(refusal.value)
    assert "body force" in two_d.two_step_admitted()
    for lat, dt, res in (("D3Q19", "f64", [5, 24, 96]), ("D3Q27", "f32", [6, 12, 128]), ("D3Q15", "f32", [6, 16, 128])):
        plan = forced_plan(lat, dt, res, "guo", "bgk")
        plan.set_two_step(1)
        assert "body force" in plan.two_step_admitted()
        g = dev(perturbed_state(lat, res, TORCH_DT[dt], 3))
        with pytest.raises(NativeEngineError, match="body force"):
            plan.stream_collide_twice(g, torch.empty_like(g), tau)
    smagorinsky = forced_plan("D3Q19", "f32", [6, 24, 192], "guo", "smagorinsky")
    smagorinsky.set_two_step(1)
    assert "Smagorinsky with a body force" in smagorinsky.two_step_admitted()
    # the same plans without the force have their launches: the refusal is the force's
    bgk = plan_for("D3Q19", torch.float32, "bgk", [6, 24, 192])
    bgk.set_two_step(1)
    assert bgk.two_step_admitted() is None
    forced = forced_plan("D3Q19", "f32", [6, 24, 192], "guo", "bgk")
    forced.set_two_step(1)
    assert forced.two_step_admitted() is None
