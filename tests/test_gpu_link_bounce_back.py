"""Interpolated and half-way bounce-back on the HIP path: the link pass (``lt_apply_links``) alone and behind the
one-step launches of ``lt_run`` against the CPU torch path of ``lt.InterpolatedBounceBackBoundary``, the same under a
``Simulation`` on a native context, the refusals, and ``lt_link_force`` against an exact host sum.

Bounds: bit identity wherever the arithmetic is the pass alone (no collision); with a collision the bound
test_gpu_engine.py uses with boundaries, ATOL[dt] * max(1, |f|max) * 10; the force within the summation bound of
test_boundary_force_host.py, (n - 1) * 2^-53 * sum |terms| for n terms.  Every comparison prints its largest difference
before it asserts.

Measured on an MI355X: the pass alone and the runs without a collision differ from the torch path by 0 on every slot; with
a collision the largest difference after 4 steps is 1.5e-7 (fp32, KBC) and 2.2e-16 (fp64); the force kernel stays within
0.05 of its bound (largest error 1.1e-16); with the two D3Q15 grids 290 tests in 4 s."""
import functools
import math

import numpy as np
import pytest
import torch

import lettuce_amd as lt
from conftest import TORCH_DT
from test_boundary_force_host import U, assert_within_bound
from test_gpu_engine import ATOL
from test_host_api import ctx, UniformFlow
from test_link_bounce_back_host import STENCIL, body_mask, dense_definition, random_fractions, random_state

pytestmark = pytest.mark.gpu

# small extents make x_ff wrap onto the far side (and onto the body itself); 67 makes the last workgroup ragged
GRIDS = [("D2Q9", [5, 67]), ("D2Q9", [3, 4]), ("D3Q19", [6, 5, 67]), ("D3Q27", [4, 4, 4]), ("D3Q27", [3, 3, 5]),
         ("D3Q15", [6, 5, 7]), ("D3Q15", [3, 3, 5])]
MASKS = ["isolated", "plate", "block", "seam", "sphere", "none"]
CASES = [(lat, res, mask) for lat, res in GRIDS for mask in MASKS]


def case_id(case):
    return f"{case[0].lower()}-{'x'.join(map(str, case[1]))}-{case[2]}"


def native(dt):
    return lt.Context(device="cuda:0", dtype=TORCH_DT[dt], use_native=True)


def body_of(lat, res, kind):
    """(mask, fractions): the host masks with random fractions on both sides of 1/2; a circle / sphere with the
    analytic ones"""
    if kind != "sphere":
        return body_mask(kind, res), random_fractions(lat, tuple(res))
    stencil = STENCIL[lat]()
    grid = torch.meshgrid(*[torch.arange(n, dtype=torch.float64) for n in res], indexing="ij")
    center = [0.5 * (n - 1) + 0.1 * (a + 1) for a, n in enumerate(res)]
    radius = max(0.9, 0.3 * min(res))
    mask = sum((g - c) ** 2 for g, c in zip(grid, center)) < radius ** 2
    return mask, lt.sphere_link_fractions(stencil, grid, center, radius)


def signed_state(lat, res, dt):
    """random populations, about a tenth of them negative"""
    f = random_state(lat, tuple(res), dt)
    flip = random_state(lat, tuple(res), dt, seed=5)
    return torch.where(flip < 0.6 * f.abs().mean(), -f, f)


def smooth_state(lat, res, dt):
    """w_q (1 + 0.1 noise): near an equilibrium at rest, without symmetries -- a state every collision takes"""
    stencil = STENCIL[lat]()
    w = torch.as_tensor(np.array(stencil.w), dtype=torch.float64).reshape([-1] + [1] * len(res))
    noise = random_state(lat, tuple(res), "f64", seed=11) / w - 1.0
    return (w * (1.0 + 0.2 * noise)).to(TORCH_DT[dt])


def link_plan(lat, res, dt, collision, boundary, masks=True):
    """a plan whose only boundary is the body, with its links (and, for stepping, its masks)"""
    from lettuce_amd import _native
    plan = _native.Plan(lat, TORCH_DT[dt], collision, list(res), [{"kind": "link_bounce_back"}])
    ncm = boundary.mask.to(torch.uint8)
    links = lt.native_link_list(boundary, 1, ncm, STENCIL[lat](), TORCH_DT[dt])
    count = plan.set_links(0, *links)
    assert count == len(links[0])
    if masks:
        plan.set_masks(ncm.cuda(), None)
    return plan


def cpu_flow(lat, res, dt, boundary, f, reynolds=100):
    flow = UniformFlow(ctx(dt), list(res), reynolds, 0.05, STENCIL[lat]())
    flow.boundaries = [boundary]
    flow.f = f.clone()
    return flow


def assert_same_bits(got, want, what):
    difference = float((got.double() - want.double()).abs().max()) if got.numel() else 0.0
    print(f"{what}: largest difference {difference:.3e}")
    assert torch.equal(got, want), what


# ------------------------------------------------------------------------------------------------ 1. the pass alone
@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_link_pass_alone_is_bit_identical_to_the_torch_call(case, dt):
    lat, res, kind = case
    mask, fractions = body_of(lat, res, kind)
    boundary = lt.InterpolatedBounceBackBoundary(mask, fractions)
    f = signed_state(lat, res, dt)
    want = boundary(cpu_flow(lat, res, dt, boundary, f))
    plan = link_plan(lat, res, dt, "none", boundary, masks=False)
    g = f.cuda()
    out = plan.apply_links(g)
    assert out is g
    assert_same_bits(g.cpu(), want, f"{case_id(case)} {dt} dense")
    if kind == "none":
        assert torch.equal(g.cpu(), f)                               # the empty list launches nothing, changes nothing
    else:
        assert not torch.equal(want, f)
    # ... with a population stride: 256 bytes of padding and more behind every population
    nodes = int(np.prod(res))
    esize = 4 if dt == "f32" else 8
    stride = ((nodes * esize + 255) // 256 + 1) * 256 // esize
    plan.set_population_stride(stride)
    padded = plan.populations_like(f.cuda())
    plan.apply_links(padded)
    assert_same_bits(padded.cpu(), want, f"{case_id(case)} {dt} stride {stride}")


# ------------------------------------------------------------------------------------------- 2. runs, no collision
@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_runs_without_a_collision_are_bit_identical_to_the_torch_path(case, dt):
    lat, res, kind = case
    mask, fractions = body_of(lat, res, kind)
    f = signed_state(lat, res, dt)
    plan = link_plan(lat, res, dt, "none", lt.InterpolatedBounceBackBoundary(mask, fractions))
    for n in (1, 2, 5):
        flow = cpu_flow(lat, res, dt, lt.InterpolatedBounceBackBoundary(mask, fractions), f)
        lt.Simulation(flow, lt.NoCollision(), [])(n)
        a = f.cuda()
        out, _ = plan.run(a, torch.empty_like(a), 1.0, n)
        assert_same_bits(out.cpu(), flow.f, f"{case_id(case)} {dt} n = {n}")
        info = plan.last_run_info()
        assert info["two_step_launches"] == 0 and info["many_step_launches"] == 0, info


# ----------------------------------------------------------------------------------------- 3. runs with a collision
COLLIDING = ([(lat, res, "bgk") for lat, res in GRIDS] + [("D2Q9", [5, 67], "kbc"), ("D3Q27", [4, 4, 4], "kbc"),
                                                          ("D3Q27", [3, 3, 5], "kbc"), ("D3Q19", [6, 5, 67], "smagorinsky")])
OPERATOR = {"bgk": lambda tau: lt.BGKCollision(tau), "kbc": lambda tau: lt.KBCCollision(tau),
            "smagorinsky": lambda tau: lt.SmagorinskyCollision(tau)}


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("kind", ["block", "sphere"])
@pytest.mark.parametrize("lat,res,collision", COLLIDING, ids=[f"{c[0].lower()}-{'x'.join(map(str, c[1]))}-{c[2]}" for c in COLLIDING])
def test_runs_with_a_collision_against_the_torch_path(lat, res, collision, kind, dt):
    mask, fractions = body_of(lat, res, kind)
    f = smooth_state(lat, res, dt)
    n = 4
    flow = cpu_flow(lat, res, dt, lt.InterpolatedBounceBackBoundary(mask, fractions), f, reynolds=1)
    tau = flow.units.relaxation_parameter_lu             # KBCCollision takes the flow's, whatever it is given: 0.76 .. 1.0
    assert 0.7 < tau < 1.1
    lt.Simulation(flow, OPERATOR[collision](tau), [])(n)
    plan = link_plan(lat, res, dt, collision, lt.InterpolatedBounceBackBoundary(mask, fractions))
    a = f.cuda()
    out, _ = plan.run(a, torch.empty_like(a), tau, n)
    want = flow.f
    tol = ATOL[dt] * max(1.0, float(want.abs().max())) * 10
    difference = float((out.cpu() - want).abs().max())
    print(f"{lat} {res} {collision} {kind} {dt}: largest difference {difference:.3e}, bound {tol:.3e}")
    assert bool(torch.isfinite(want).all()) and not torch.equal(want, f)
    assert difference <= tol


# ------------------------------------------------------------------------------------------------ 4. under Simulation
def native_simulation(lat, res, dt, boundary, f, collision):
    flow = UniformFlow(native(dt), list(res), 100, 0.05, STENCIL[lat]())
    flow.boundaries = [boundary]
    flow.f = f.cuda()
    simulation = lt.Simulation(flow, collision, [])
    assert simulation._native is not None, "HIP engine not in use"
    return flow, simulation


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("lat,res", [("D2Q9", [16, 8]), ("D3Q27", [4, 4, 4]), ("D3Q19", [6, 5, 67])],
                         ids=["d2q9-16x8", "d3q27-4x4x4", "d3q19-6x5x67"])
def test_simulation_batches_carry_on_bit_for_bit(lat, res, dt):
    """sim(3); sim(2) equals sim(5): the carry from the post-collision buffer and the deferred streaming pass"""
    mask, fractions = body_of(lat, res, "block")
    f = smooth_state(lat, res, dt)
    flow_a, sim_a = native_simulation(lat, res, dt, lt.InterpolatedBounceBackBoundary(mask, fractions), f, lt.BGKCollision(0.8))
    sim_a(3)
    sim_a(2)
    flow_b, sim_b = native_simulation(lat, res, dt, lt.InterpolatedBounceBackBoundary(mask, fractions), f, lt.BGKCollision(0.8))
    sim_b(5)
    assert_same_bits(flow_a.f.cpu(), flow_b.f.cpu(), f"{lat} {res} {dt} 3 + 2 against 5")
    for simulation in (sim_a, sim_b):
        info = simulation._native.plan.last_run_info()
        print(f"  {info}")
        assert info["two_step_launches"] == 0 and info["many_step_launches"] == 0 and info["single_step_launches"] > 0
    cpu = cpu_flow(lat, res, dt, lt.InterpolatedBounceBackBoundary(mask, fractions), f)
    lt.Simulation(cpu, lt.BGKCollision(0.8), [])(5)
    tol = ATOL[dt] * max(1.0, float(cpu.f.abs().max())) * 10
    difference = float((flow_b.f.cpu() - cpu.f).abs().max())
    print(f"  against the torch path: largest difference {difference:.3e}, bound {tol:.3e}")
    assert difference <= tol


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_assigning_fractions_or_mask_between_batches_takes_effect(dt):
    lat, res = "D2Q9", [16, 8]
    mask, fractions = body_of(lat, res, "block")
    other_fractions = random_fractions(lat, tuple(res), seed=21)
    other_mask = body_mask("plate", res)
    f = signed_state(lat, res, dt)

    def play(flow, simulation, boundary, change):
        simulation(2)
        if change >= 1:
            boundary.fractions = other_fractions
        simulation(2)
        if change >= 2:
            boundary.mask = other_mask
            simulation.no_collision_mask = flow.context.convert_to_tensor(other_mask.to(torch.uint8), dtype=torch.uint8)
        simulation(3)
        return flow.f.cpu()

    results = []
    for change in (0, 1, 2):
        body = lt.InterpolatedBounceBackBoundary(mask, fractions)
        flow, simulation = native_simulation(lat, res, dt, body, f, lt.NoCollision())
        got = play(flow, simulation, body, change)
        body = lt.InterpolatedBounceBackBoundary(mask, fractions)
        cpu = cpu_flow(lat, res, dt, body, f)
        want = play(cpu, lt.Simulation(cpu, lt.NoCollision(), []), body, change)
        assert_same_bits(got, want, f"{dt} change {change}")
        results.append(got)
    assert not torch.equal(results[0], results[1]) and not torch.equal(results[1], results[2])


# ----------------------------------------------------------------------------------------------------- 5. refusals
def test_refusals_by_name():
    from lettuce_amd import _native
    lat, res, dt = "D3Q19", [8, 16, 64], "f32"                       # a grid the two-step kernels tile
    boundary = lt.HalfwayBounceBackBoundary(body_mask("block", res))
    plan = link_plan(lat, res, dt, "bgk", boundary)
    f = smooth_state(lat, res, dt).cuda()
    out = torch.empty_like(f)
    with pytest.raises(_native.NativeEngineError, match="two steps per launch with link bounce-back") as e:
        plan.set_two_step(1)
    assert e.value.code == 2                                         # LT_ERR_UNSUPPORTED
    with pytest.raises(_native.NativeEngineError, match="two steps per launch with link bounce-back"):
        plan.stream_collide_twice(f, out, 0.8)
    assert "link bounce-back" in plan.two_step_admitted()
    with pytest.raises(_native.NativeEngineError, match="a range of planes per launch with link bounce-back"):
        plan.collide_planes(f, out, 0.8, 0, 4)
    with pytest.raises(_native.NativeEngineError, match="a range of planes per launch with link bounce-back"):
        plan.stream_collide_planes(f, out, 0.8, 2, 8)
    plan.run(f, out, 0.8, 3)                                         # and the plan still steps, one update per launch
    assert plan.last_run_info() == {"single_step_launches": 2, "two_step_launches": 0, "many_step_launches": 0}
    flat = link_plan("D2Q9", [16, 8], "f64", "bgk", lt.HalfwayBounceBackBoundary(body_mask("block", [16, 8])))
    g = smooth_state("D2Q9", [16, 8], "f64").cuda()
    with pytest.raises(_native.NativeEngineError, match="several steps per launch with link bounce-back"):
        flat.set_many_step(1)
    with pytest.raises(_native.NativeEngineError, match="several steps per launch with link bounce-back"):
        flat.stream_collide_many(g, torch.empty_like(g), 0.8, 4)
    # at plan creation: the slab layout, ghost planes, 1-D
    link = [{"kind": "link_bounce_back"}]
    with pytest.raises(_native.NativeEngineError, match="link bounce-back: 2-D / 3-D plans in the reference layout") as e:
        _native.Plan("D3Q19", torch.float32, "bgk", [8, 8, 6], link, layout=_native.LAYOUT_SLAB, ghost_planes=1)
    assert e.value.code == 2
    with pytest.raises(_native.NativeEngineError, match="link bounce-back: 2-D / 3-D plans in the reference layout"):
        _native.Plan("D3Q19", torch.float32, "bgk", [8, 8, 6], link, layout=_native.LAYOUT_SLAB)
    with pytest.raises(_native.NativeEngineError, match="link bounce-back: 2-D / 3-D plans"):
        _native.Plan("D1Q3", torch.float32, "bgk", [16], link)
    # stepped before its links were given
    bare = _native.Plan(lat, torch.float32, "bgk", res, link)
    bare.set_masks(boundary.mask.to(torch.uint8).cuda(), None)
    for call in (lambda: bare.collide(f, out, 0.8), lambda: bare.stream_collide(f, out, 0.8),
                 lambda: bare.run(f, out, 0.8, 2), lambda: bare.apply_links(f)):
        with pytest.raises(_native.NativeEngineError, match="lt_plan_set_links must give its links first") as e:
            call()
        assert e.value.code == 1                                     # LT_ERR_INVALID
    bare.stream(f, out)                                              # streaming alone needs none
    # lists the kernels could not index safely
    ok = lt.native_link_list(boundary, 1, boundary.mask.to(torch.uint8), STENCIL[lat](), torch.float32)
    nodes, directions, c1, c2, second = ok
    with pytest.raises(_native.NativeEngineError, match="outside"):
        bare.set_links(0, nodes + int(np.prod(res)), directions, c1, c2, second)
    with pytest.raises(_native.NativeEngineError, match="outside"):
        bare.set_links(0, nodes, directions + 19, c1, c2, second)
    with pytest.raises(_native.NativeEngineError, match="sorted by node, then by direction"):
        bare.set_links(0, nodes.flip(0), directions.flip(0), c1, c2, second)
    with pytest.raises(_native.NativeEngineError, match="not link bounce-back"):
        _native.Plan(lat, torch.float32, "bgk", res, [{"kind": "bounce_back"}]).set_links(0, *ok)
    with pytest.raises(_native.NativeEngineError, match="lt_plan_set_links must give its links first"):
        bare.collide(f, out, 0.8)                                    # none of them left a list behind


def test_a_body_touching_an_inlet_is_refused_by_the_stepper():
    res = [16, 12]
    solid = torch.zeros(res, dtype=torch.bool)
    solid[1:3, 5:8] = True                                           # its links reach the inlet's row x = 0
    flow = lt.Obstacle(native("f64"), res, 50, 0.05, domain_length_x=4.0, stencil=lt.D2Q9(),
                       solid_boundary=lt.HalfwayBounceBackBoundary)
    flow.mask = solid
    flow.initialize()
    simulation = lt.Simulation(flow, lt.BGKCollision(0.8), [])
    with pytest.raises(lt.NativeEngineError, match="reads a node of another boundary"):
        simulation(1)
    solid = torch.zeros(res, dtype=torch.bool)
    solid[6:9, 5:8] = True                                           # clear of the inlet and the outlet: it runs
    clear = lt.Obstacle(native("f64"), res, 50, 0.05, domain_length_x=4.0, stencil=lt.D2Q9(),
                        solid_boundary=lt.HalfwayBounceBackBoundary)
    clear.mask = solid
    clear.initialize()
    host = lt.Obstacle(ctx("f64"), res, 50, 0.05, domain_length_x=4.0, stencil=lt.D2Q9(),
                       solid_boundary=lt.HalfwayBounceBackBoundary)
    host.mask = solid
    host.initialize()
    lt.Simulation(clear, lt.BGKCollision(0.8), [])(6)
    lt.Simulation(host, lt.BGKCollision(0.8), [])(6)
    tol = ATOL["f64"] * max(1.0, float(host.f.abs().max())) * 10
    difference = float((clear.f.cpu() - host.f).abs().max())
    print(f"Obstacle with a half-way body, 6 steps: largest difference {difference:.3e}, bound {tol:.3e}")
    assert difference <= tol


class _PressureStream(lt.Obstacle):
    """the Obstacle with the constant-pressure outlet in place of the anti-bounce-back one (kernels of their own)"""

    @property
    def boundaries(self):
        inlet, _, body = super().boundaries
        return [inlet, lt.EquilibriumOutletP(self._unit_vector().tolist(), self), body]


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("lat,res", [("D2Q9", [16, 12]), ("D3Q19", [12, 6, 7])], ids=["d2q9", "d3q19"])
def test_an_interpolated_body_beside_a_constant_pressure_outlet(lat, res, dt):
    stencil = STENCIL[lat]()
    solid = torch.zeros(res, dtype=torch.bool)
    solid[tuple(slice(n // 2 - 1, n // 2 + 1) for n in res)] = True
    fractions = random_fractions(lat, tuple(res), seed=41)
    flows = []
    for context in (native(dt), ctx(dt)):
        flow = _PressureStream(context, list(res), 50, 0.05, domain_length_x=4.0, stencil=stencil,
                               solid_boundary=lambda mask: lt.InterpolatedBounceBackBoundary(mask, fractions))
        flow.mask = solid
        flow.initialize()
        simulation = lt.Simulation(flow, lt.BGKCollision(0.8), [])
        simulation(6)
        flows.append(flow)
    want = flows[1].f
    tol = ATOL[dt] * max(1.0, float(want.abs().max())) * 10
    difference = float((flows[0].f.cpu() - want).abs().max())
    print(f"{lat} {res} {dt} pressure outlet and interpolated body, 6 steps: largest difference {difference:.3e}, bound {tol:.3e}")
    assert bool(torch.isfinite(want).all()) and difference <= tol


# ------------------------------------------------------------------------------------------------------- 6. the force
def exact_link_force(stencil, f, mask, fractions):
    """the definition on post-streaming populations: per component (fsum(terms), fsum(|terms|), number of terms), the
    terms e_{q,c} f_q(x_s) and e_{q,c} f_r(x_f) of every link"""
    res = list(mask.shape)
    f = f.detach().cpu().double()
    _, links = dense_definition(stencil, f, mask, fractions)
    terms = [[] for _ in range(stencil.d)]
    for node, r, _, _, _ in links:
        x_s = tuple(int(i) for i in np.unravel_index(node, res))
        e_r = [int(c) for c in stencil.e[r]]
        x_f = tuple((x_s[a] + e_r[a]) % res[a] for a in range(stencil.d))
        q = int(stencil.opposite[r])
        for c in range(stencil.d):
            e = int(stencil.e[q][c])
            if e:
                terms[c] += [e * float(f[(q,) + x_s]), e * float(f[(r,) + x_f])]
    return [(math.fsum(t), math.fsum(abs(v) for v in t), len(t)) for t in terms]


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("case", [c for c in CASES if c[2] in ("block", "sphere", "seam", "none")], ids=case_id)
def test_link_force_against_an_exact_host_sum(case, dt):
    lat, res, kind = case
    stencil = STENCIL[lat]()
    mask, fractions = body_of(lat, res, kind)
    boundary = lt.InterpolatedBounceBackBoundary(mask, fractions)
    plan = link_plan(lat, res, dt, "none", boundary, masks=False)
    f = signed_state(lat, res, dt)
    if kind == "none":
        other = link_plan(lat, res, dt, "none", lt.HalfwayBounceBackBoundary(body_mask("block", res)), masks=False)
        assert bool((other.link_force(0, f.cuda()) != 0).any())
    first = plan.link_force(0, f.cuda()).clone()
    second = plan.link_force(0, f.cuda())
    assert first.dtype == torch.float64 and list(first.shape) == [stencil.d]
    assert torch.equal(first, second)                                # two calls, the same bits
    exact = exact_link_force(stencil, f, mask, fractions)
    assert_within_bound(first.cpu().tolist(), exact, torch.float64, f"{case_id(case)} {dt}")
    if kind == "none":
        assert first.cpu().tolist() == [0.0] * stencil.d
    from lettuce_amd.ext._reporter import link_momentum_exchange
    host = link_momentum_exchange(stencil, f, boundary.links(stencil, TORCH_DT[dt]))
    assert_within_bound(host.tolist(), exact, torch.float64, f"{case_id(case)} {dt} torch expression")


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("n_links", [5, 320000], ids=["5-links", "every-node-8-directions"])
def test_link_force_has_the_bits_of_the_documented_summation_order(n_links, dt):
    """A synthetic sorted list on D2Q9 [200, 200], every node x the directions 1 .. 8: 320 000 links > 1024 * 256, so a
    thread of the first workgroups adds two links; and its first 5 links alone.  The order of link_bounce.hpp and
    reduce.hpp, emulated on the host (fixed_order_sum.py), predicts the bytes.  Terms as link_force_kernel adds them:
    +- out, +- back per link, out = f_q(x_s), back = f_r(x_f), the sign that of e_{q,c}.
    What pins the ORDER are the fp64 plans: fp32 terms widened to fp64 add exactly whatever the order, so the fp32 cases
    show only that every item is taken exactly once."""
    import fixed_order_sum as fos
    from lettuce_amd import _native
    lat, res = "D2Q9", [200, 200]
    stencil = STENCIL[lat]()
    nodes = np.repeat(np.arange(res[0] * res[1]), 8)[:n_links]
    directions = np.tile(np.arange(1, 9), res[0] * res[1])[:n_links]
    f = signed_state(lat, res, dt)
    e = np.array(stencil.e, dtype=np.int64)
    opposite = np.array([int(o) for o in stencil.opposite])
    x_s = np.stack(np.unravel_index(nodes, res), axis=1)
    x_f = (x_s + e[directions]) % np.array(res)
    q = opposite[directions]
    values = f.double().numpy()
    out, back = values[q, x_s[:, 0], x_s[:, 1]], values[directions, x_f[:, 0], x_f[:, 1]]
    items = np.zeros((stencil.d, n_links, 2))
    for c in range(stencil.d):
        sign = np.sign(e[q, c]).astype(np.float64)
        items[c, :, 0], items[c, :, 1] = np.where(sign != 0, sign * out, 0.0), np.where(sign != 0, sign * back, 0.0)
    want = np.asarray(fos.link_force(items), dtype=np.float64)
    plan = _native.Plan(lat, TORCH_DT[dt], "none", res, [{"kind": "link_bounce_back"}])
    coefficient = torch.zeros(n_links, dtype=TORCH_DT[dt])
    assert plan.set_links(0, nodes, directions, coefficient, coefficient, np.zeros(n_links, dtype=np.uint8)) == n_links
    got = plan.link_force(0, f.cuda()).cpu().numpy()
    print(f"{n_links} links {dt}: got {got.tolist()!r}, emulation {want.tolist()!r}")
    # (over every node and direction the terms cancel -- each population leaves one node and comes back to another: what
    # is left in fp64 is the rounding of this very order, 5e-15 and 2e-14 on an MI355X; the fp32 terms add exactly, to 0.0)
    assert got.dtype == np.float64 and (n_links > 5 or bool((got != 0).all())) and got.tobytes() == want.tobytes()


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("lat,res", [("D2Q9", [16, 12]), ("D3Q27", [8, 8, 8])], ids=["d2q9", "d3q27"])
def test_drag_coefficient_on_native_and_cpu_contexts(lat, res, dt):
    """the same populations on both contexts: lt_link_force there, the torch expression here, both within the summation
    bound of the exact sum over the scale (one rounding of the division, half an ulp of the cast)"""
    stencil = STENCIL[lat]()
    solid = torch.zeros(res, dtype=torch.bool)
    solid[tuple(slice(n // 2 - 1, n // 2 + 1) for n in res)] = True
    fractions = random_fractions(lat, tuple(res), seed=31)
    area = 0.75
    values = {}
    f = signed_state(lat, res, dt)
    for name, context in (("native", native(dt)), ("cpu", ctx(dt))):
        flow = lt.Obstacle(context, list(res), 50, 0.05, domain_length_x=4.0, stencil=stencil,
                           solid_boundary=lambda mask: lt.InterpolatedBounceBackBoundary(mask, fractions))
        flow.mask = solid
        flow.f = f.to(context.device)
        body = flow.boundaries[2]
        drag = lt.DragCoefficient(flow, body, area)
        lift = lt.LiftCoefficient(flow, body, area)
        assert (drag._link_plan is None) and isinstance(body, lt.InterpolatedBounceBackBoundary)
        values[name] = (float(drag()), float(lift()))
        assert (drag._link_plan is not None) == (name == "native")   # the engine's sum there, the torch expression here
        units = flow.units
        scale = (0.5 * units.characteristic_density_lu * units.characteristic_velocity_lu ** 2
                 * area * units.convert_length_to_lu(1.0) ** (stencil.d - 1))
    exact = exact_link_force(stencil, f, solid, fractions)
    for name, (c_d, c_l) in values.items():
        for c, value in ((0, c_d), (1, c_l)):
            want = exact[c][0] / scale
            bound = max(exact[c][2] - 1, 0) * U * exact[c][1] / scale + 2 * U * abs(want)
            if dt == "f32":
                bound += 0.5 * float(np.spacing(np.float32(abs(value))))
            print(f"{lat} {dt} {name} C[{c}] = {value!r}, F / scale = {want!r}, error {abs(value - want):.3e}, bound {bound:.3e}")
            assert abs(value - want) <= bound
    assert values["native"][0] != 0.0
