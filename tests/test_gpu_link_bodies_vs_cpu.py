"""Link bounce-back bodies (``lt.InterpolatedBounceBackBoundary`` / ``lt.HalfwayBounceBackBoundary``, plan boundary kind
6) on every one-step kernel family and every launch path of the HIP engine, against the mirror's own torch path on a CPU
context in float64 -- the definition of the boundary (tests/test_link_bounce_back_host.py ties it to a dense statement).
The cases, the collision table and the references are in tests/link_body_cases.py; tests/test_link_bodies_host.py checks
without a GPU that every list is two-sided, no case is refused and every reference is finite with E_ref > 0.

A. every collision number of tests/test_tune3_census.py in every 2-D / 3-D unit that has it (Guo and Shan-Chen for 5
   and 7), both dtypes, the ``block`` and ``sphere`` bodies alone in the plan: ``collide`` and ``run`` for 1 and 4 steps
   against the reference, the plan's kernel named; and directly, on a plan whose body has an empty list, every slot of a
   solid node equal to the input (collide) or to the engine's own ``stream`` of it (fused), bit for bit.
B. the body among other boundaries, its index chosen: a wall and an inlet, one anti-bounce-back outlet on each axis and
   side (the contiguous axis with 64 nodes too), two and three outlets with one of constant pressure, two bodies, MRT
   with a pressure outlet -- ``run`` and ``lt.Simulation`` on a native context against the mirror on the CPU.
C. launch paths, engine against engine, ``torch.equal``: cache policy 3, replayed graphs (and ``set_links`` /
   ``set_masks`` on the plan that holds one), resident padded buffers, a population stride, and ``lt.Simulation`` with a
   ``BoundaryForce`` reporter reading ``flow.f`` while the streaming pass is pending.
D. D3Q15: the bit pin of the force kernel's summation order (the pass alone, the runs without a collision and the force
   against an exact host sum take D3Q15 through the case lists of tests/test_gpu_link_bounce_back.py).

Gates: fp64 |gpu - cpu64| <= 1e-12 max(1, |f|max) (test_gpu_engine.ATOL); fp32 the rounding-level gate of
tests/test_gpu_fp32_error_budget.py, E_gpu <= 4 E_ref with E = max |. - cpu64| / w_q and E_ref the mirror's own fp32
run from the same fp32 state; bit identity wherever the arithmetic is the pass alone (no collision) and between two
engine paths.  Every comparison prints its figures before it asserts.

In C.5 each reported force is held to the exact host sum over the populations the reporter was handed on that context
(the summation bound of tests/test_boundary_force_host.py), and those populations to the CPU's by the gates at every
report.  The native force is also held to the exact sum over the CPU populations of that step wherever that bound can
hold: in fp64 (the two contexts differ by a few 1e-16 per population, the bound is 2e-15 .. 2e-14) and without a
collision (the same bits).  In fp32 with a collision two correct runs differ by 1e-7 per population and the bound is
half an ulp of the force, 2e-9 .. 4e-9: that difference is printed (up to 1.0e-7 on an MI355X), not asserted.

Measured on an MI355X: the largest fp64 difference is 4.4e-16 (forced Smagorinsky, D2Q9 [5, 67], 4 steps; bound 1e-12);
the largest E_gpu / E_ref is 1.42 (the regularised collision, D2Q9 [12, 10], sphere, 4 steps; E_ref 4.6e-7), 1.40 in
part B (D3Q27 beside an outlet at x+, one step); no case needs a factor of its own; every no-collision run and every
engine-against-engine comparison differs by 0; 130 tests (1898 comparisons: one test per kernel family, kind of scene,
lattice and dtype, the cases looped over inside and printed one by one) in 10 s."""
import warnings

import numpy as np
import pytest
import torch

import lettuce_amd as lt
import link_body_cases as cases
from conftest import TORCH_DT
from link_body_cases import COLLISION, FACTOR, SCENES
from test_boundary_force_host import assert_within_bound
from test_gpu_engine import ATOL
from test_gpu_link_bounce_back import exact_link_force, signed_state
from test_link_bounce_back_host import STENCIL, random_fractions

pytestmark = pytest.mark.gpu

UNTOUCHED = -7.0
PAD = 96                       # elements between the populations of the resident buffers, beyond the field
# case id (as the comparisons print it) -> the next power of two above a measured E_gpu / E_ref that honestly exceeds 4, the arithmetic that explains it
# in DESIGN.md section 2; beyond 16 it is a bug
FACTORS = {}


@pytest.fixture(autouse=True)
def _nothing_runs_after_a_device_fault():
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as exc:
        pytest.exit(f"the device reported a fault; no further launches: {exc}", returncode=3)


def native(dt):
    return lt.Context(device="cuda:0", dtype=TORCH_DT[dt], use_native=True)


class _Gates:
    """collects the comparisons of one test: each prints its figures at once, `check` asserts them all"""

    def __init__(self, key, lat, dt):
        self.lat, self.dt, self.failures = lat, dt, []
        self.factor = FACTORS.get(key, FACTOR)

    def hold(self, got, want64, want32, what):
        got = got.detach().cpu().double().numpy()
        assert np.isfinite(got).all(), what
        if self.dt == "f64":
            difference = float(np.abs(got - want64).max())
            bound = ATOL["f64"] * max(1.0, float(np.abs(want64).max()))
            print(f"{what}: largest difference {difference:.3e}, bound {bound:.3e}")
            if not difference <= bound:
                self.failures.append((what, difference, bound))
            return
        e_ref = cases.weighted_error(self.lat, want32, want64)
        e_gpu = cases.weighted_error(self.lat, got, want64)
        print(f"{what}: E_ref {e_ref:.3e}  E_gpu {e_gpu:.3e}  ratio {e_gpu / e_ref:.2f}  (gate {self.factor:g})")
        # (0 < E_ref < 1e-4 is what the host companion holds every reference to: a yardstick, neither zero nor a blunder)
        if not (0 < e_ref < 1e-4 and e_gpu <= self.factor * e_ref):
            self.failures.append((what, e_ref, e_gpu, e_gpu / e_ref))

    def same_bits(self, got, want, what):
        got = got.detach().cpu().double().numpy()
        difference = float(np.abs(got - want).max())
        print(f"{what}: largest difference to the torch path of the same dtype {difference:.3e}")
        if not np.array_equal(got, want):
            self.failures.append((what, "bits", difference))

    def check(self):
        assert not self.failures, self.failures


def assert_equal_bits(got, want, what):
    difference = float((got.double() - want.double()).abs().max())
    print(f"{what}: largest difference {difference:.3e}")
    assert torch.equal(got, want), what


def link_plan(case, dt, boundary=None, empty=False):
    """the plan of a part A / C case, the body its only boundary, with its list (or an empty one) and its masks"""
    coll, scheme, lat, res, kind = case[:5]
    boundary = cases.body(lat, res, kind) if boundary is None else boundary
    plan = COLLISION[(coll, scheme)][1](lat, dt, res, [{"kind": "link_bounce_back"}])
    ncm = boundary.mask.to(torch.uint8)
    links = lt.native_link_list(boundary, 1, ncm, STENCIL[lat](), TORCH_DT[dt])
    if empty:
        links = tuple(t[:0] for t in links)
    else:
        assert len(links[0]) > 0
    assert plan.set_links(0, *links) == len(links[0])
    plan.set_masks(ncm.cuda(), None)
    return plan


def assert_kernel(plan, case, dt, policy=0):
    """the plan names the family's own kernel: scalar, lattice, reference layout, the collision number, masks, policy"""
    coll, _, lat = case[:3]
    kernel = "lbm_kernel_occ4" if (lat, dt, coll) == ("D3Q27", "f32", 2) else "lbm_kernel"
    name = plan.kernel_name()
    fields = name.split(", ")
    assert name.startswith(f"{kernel}<{'float' if dt == 'f32' else 'double'}, lt::{lat.lower()}, 0, {coll}, "), name
    assert fields[6] == "true" and fields[9] == str(policy), name


def one_step_launches_only(plan, fused):
    info = plan.last_run_info()
    assert info == {"single_step_launches": fused, "two_step_launches": 0, "many_step_launches": 0}, info


def steps(plan, f0, tau, n):
    a = f0.clone()
    out, _ = plan.run(a, torch.empty_like(a), tau, n)
    return out


# ------------------------------------------------------------------------------- A. every family around a body
# One test per kernel family (collision number and force scheme) and dtype; inside it every unit that has the family,
# every shape and both bodies, each comparison printed under its own case id and all of them asserted at the end.
PART_A = cases.part_a_cases()
FAMILIES = cases.variants()


def family_id(variant):
    return f"coll{variant[0]}{'-' + variant[1] if variant[1] else ''}"


def cases_of(variant):
    members = [case for case in PART_A if case[:2] == variant]
    assert {case[2] for case in members} == cases.units_of(variant[0]) and len(members) >= 4
    return members


def _steps_around_a_body(case, dt):
    """collide and lt_run for 1 and 4 steps of one case against the reference: the comparisons that failed"""
    coll, scheme, lat, res, kind = case
    tau = COLLISION[(coll, scheme)][2]
    plan = link_plan(case, dt)
    assert_kernel(plan, case, dt)
    f0 = cases.state(lat, res, dt).cuda()
    want64 = cases.reference(lat, res, dt, coll, scheme, kind, "f64")
    want32 = cases.reference(lat, res, dt, coll, scheme, kind, "f32") if dt == "f32" else want64
    same = cases.reference(lat, res, dt, coll, scheme, kind, dt)
    what = f"{cases.part_a_id(case)} {dt}"
    gates = _Gates(what, lat, dt)
    got = {"collide": plan.collide(f0, torch.full_like(f0, UNTOUCHED), tau)}
    for n in cases.RUNS:
        got[n] = steps(plan, f0, tau, n)
        one_step_launches_only(plan, n - 1)
    for key, value in got.items():
        gates.hold(value, want64[key], want32[key], f"{what} {key}")
        if coll == 0:                                   # the arithmetic is the pass alone
            gates.same_bits(value, same[key], f"{what} {key}")
    assert not np.array_equal(want64["collide"], f0.cpu().double().numpy())
    return gates.failures


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("variant", FAMILIES, ids=family_id)
def test_every_collision_family_steps_around_a_body(variant, dt):
    failures = [failure for case in cases_of(variant) for failure in _steps_around_a_body(case, dt)]
    assert not failures, failures


def _solid_nodes_of(case, dt):
    """the state before the pass: the same plan entries, the body's list empty, so that the pass launches nothing"""
    coll, scheme, lat, res, kind = case
    tau = COLLISION[(coll, scheme)][2]
    boundary = cases.body(lat, res, kind)
    plan = link_plan(case, dt, boundary, empty=True)
    assert_kernel(plan, case, dt)
    solid = boundary.mask.cuda()
    f0 = cases.state(lat, res, dt).cuda()
    collided = plan.collide(f0, torch.full_like(f0, UNTOUCHED), tau)
    fused = plan.stream_collide(f0, torch.full_like(f0, UNTOUCHED), tau)
    streamed = plan.stream(f0, torch.full_like(f0, UNTOUCHED))
    stencil = STENCIL[lat]()
    rolled = torch.stack([torch.roll(f0[q], shifts=tuple(int(c) for c in stencil.e[q]), dims=tuple(range(stencil.d)))
                          for q in range(stencil.q)])
    what = f"{cases.part_a_id(case)} {dt}"
    assert int(solid.sum()) >= 2
    assert_equal_bits(streamed, rolled, f"{what}: the engine's stream against torch.roll")
    assert_equal_bits(collided[:, solid], f0[:, solid], f"{what}: solid nodes after collide against the input")
    assert_equal_bits(fused[:, solid], streamed[:, solid], f"{what}: solid nodes after the fused step against the streamed input")
    if coll != 0:                                       # ... while every fluid node was collided
        assert bool(((collided != f0).any(dim=0) | solid).all())
        assert bool(((fused != streamed).any(dim=0) | solid).all())


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("variant", FAMILIES, ids=family_id)
def test_solid_nodes_are_neither_collided_nor_touched(variant, dt):
    for case in cases_of(variant):
        _solid_nodes_of(case, dt)


# ------------------------------------------------------------------------------- B. the body among other boundaries
# One test per kind of scene (a .. e), lattice and dtype; inside it every scene of that kind on that lattice.
SCENE_GROUPS = sorted({(cid[0], SCENES[cid][1]) for cid in SCENES})


def scenes_of(group):
    members = [cid for cid in SCENES if (cid[0], SCENES[cid][1]) == group]
    assert members
    return members


def _body_among_other_boundaries(cid, dt):
    _, lat, res, _, boundaries = SCENES[cid]
    want64 = cases.scene_reference(cid, dt, "f64")
    want32 = cases.scene_reference(cid, dt, "f32") if dt == "f32" else want64
    gates = _Gates(f"{cid} {dt}", lat, dt)
    f0 = cases.state(lat, res, dt).cuda()
    plan, tau = cases.scene_plan(cid, dt)
    assert plan.kernel_name().split(", ")[6] == "true", plan.kernel_name()
    print(f"{cid} {dt}: {plan.kernel_name()}")
    for n in cases.SCENE_STEPS:
        gates.hold(steps(plan, f0, tau, n), want64[n], want32[n], f"{cid} {dt} run n = {n}")
        one_step_launches_only(plan, n - 1)
    # the same through lt.Simulation on a native context: its masks and the upload of the lists
    flow, simulation = cases.scene_simulation(cid, native(dt))
    assert simulation._native is not None, "HIP engine not in use"
    done = 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for n in cases.SCENE_STEPS:
            simulation(n - done)
            done = n
            gates.hold(flow.f, want64[n], want32[n], f"{cid} {dt} Simulation n = {n}")
    info = simulation._native.plan.last_run_info()
    assert info["two_step_launches"] == 0 and info["many_step_launches"] == 0, info
    return gates.failures


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("group", SCENE_GROUPS, ids=[f"{g[0]}-{g[1].lower()}" for g in SCENE_GROUPS])
def test_a_body_among_other_boundaries(group, dt):
    failures = [failure for cid in scenes_of(group) for failure in _body_among_other_boundaries(cid, dt)]
    assert not failures, failures


# ------------------------------------------------------------------------------- C. launch paths, engine against engine
PART_C = cases.PART_C


def _eager(case, dt, f0, n, boundary=None):
    plan = link_plan(case, dt, boundary)
    plan.set_tuning(0)
    plan.set_graph_mode(0)
    plan.set_resident(0)
    out = steps(plan, f0, COLLISION[(case[0], case[1])][2], n)
    one_step_launches_only(plan, n - 1)
    return out


def _cache_policy_3_is_bit_identical_to_policy_0(case):
    coll, scheme, lat, res, kind, dt = case
    tau = COLLISION[(coll, scheme)][2]
    plan = link_plan(case, dt)
    f0 = cases.state(lat, res, dt).cuda()
    got = {}
    for policy in (3, 0):
        plan.set_tuning(policy)
        assert_kernel(plan, case, dt, policy)
        got[policy] = (plan.collide(f0, torch.full_like(f0, UNTOUCHED), tau), steps(plan, f0, tau, 4))
    what = cases.part_c_id(case)
    assert_equal_bits(got[3][0], got[0][0], f"{what} collide, policy 3 against 0")
    assert_equal_bits(got[3][1], got[0][1], f"{what} 4 steps, policy 3 against 0")
    assert not torch.equal(got[0][1], f0)


@pytest.mark.parametrize("case", PART_C, ids=cases.part_c_id)
def test_replayed_graphs_and_a_new_list_or_mask_on_the_plan_that_holds_one(case):
    """1 + 70 steps: two replayed chunks of 32 fused steps, each with the pass behind it, and an eager remainder; then
    other fractions (``set_links``) and another body (``set_masks`` and its list) on the same plan and buffers"""
    coll, scheme, lat, res, kind, dt = case
    tau = COLLISION[(coll, scheme)][2]
    n = cases.GRAPH_STEPS
    f0 = cases.state(lat, res, dt).cuda()
    first = cases.body(lat, res, kind)
    other_fractions = lt.InterpolatedBounceBackBoundary(first.mask, random_fractions(lat, tuple(res), seed=21))
    other_body = cases.body(lat, res, "sphere" if kind == "block" else "block")
    plan = link_plan(case, dt, first)
    plan.set_graph_mode(1)
    a, b = f0.clone(), torch.empty_like(f0)
    what = cases.part_c_id(case)

    def replay():
        a.copy_(f0)
        out, _ = plan.run(a, b, tau, n)
        assert bool(torch.isfinite(out).all())
        return out.clone()

    got = replay()
    want = _eager(case, dt, f0, n, first)
    assert_equal_bits(got, want, f"{what}: {n} steps, replayed graphs against eager launches")
    plan.set_links(0, *lt.native_link_list(other_fractions, 1, first.mask.to(torch.uint8), STENCIL[lat](), TORCH_DT[dt]))
    changed = replay()
    assert_equal_bits(changed, _eager(case, dt, f0, n, other_fractions), f"{what}: after set_links with other fractions")
    assert not torch.equal(changed, got)
    ncm = other_body.mask.to(torch.uint8)
    plan.set_masks(ncm.cuda(), None)
    plan.set_links(0, *lt.native_link_list(other_body, 1, ncm, STENCIL[lat](), TORCH_DT[dt]))
    moved = replay()
    assert_equal_bits(moved, _eager(case, dt, f0, n, other_body), f"{what}: after set_masks with another body and its list")
    assert not torch.equal(moved, changed)


def _resident_padded_buffers_are_bit_identical_to_the_dense_run(case):
    coll, scheme, lat, res, kind, dt = case
    tau = COLLISION[(coll, scheme)][2]
    f0 = cases.state(lat, res, dt).cuda()
    want = _eager(case, dt, f0, 4)
    plan = link_plan(case, dt)
    plan.set_resident(1, PAD)
    enabled, stride = plan.resident_enabled()
    nodes = int(np.prod(res))
    assert enabled and stride > nodes and stride % nodes != 0, (stride, nodes)
    what = cases.part_c_id(case)
    for advances in ((3,), (2, 1)):
        plan.resident_load(f0, tau)
        for k in advances:
            plan.resident_advance(tau, k)
            one_step_launches_only(plan, k)
        got = plan.resident_store(torch.full_like(f0, UNTOUCHED))
        assert_equal_bits(got, want, f"{what}: resident load, advance {advances}, store (stride {stride}) against 4 dense steps")


def _a_population_stride_is_bit_identical_to_the_dense_run(case):
    coll, scheme, lat, res, kind, dt = case
    tau = COLLISION[(coll, scheme)][2]
    f0 = cases.state(lat, res, dt).cuda()
    want = _eager(case, dt, f0, 4)
    plan = link_plan(case, dt)
    nodes, esize = int(np.prod(res)), 4 if dt == "f32" else 8
    stride = ((nodes * esize + 255) // 256 + 1) * 256 // esize       # 256 bytes of padding and more behind every population
    plan.set_population_stride(stride)
    a, b = plan.populations_like(f0), plan.empty_populations()
    b.fill_(UNTOUCHED)
    out, _ = plan.run(a, b, tau, 4)
    one_step_launches_only(plan, 3)
    assert out.stride(0) == stride
    assert_equal_bits(out.contiguous(), want, f"{cases.part_c_id(case)}: 4 steps with population stride {stride} against dense")


@pytest.mark.parametrize("case", PART_C, ids=cases.part_c_id)
def test_cache_policy_resident_buffers_and_population_stride_against_the_dense_run(case):
    """C.1, C.3 and C.4, each torch.equal to the eager dense policy-0 run of the same case"""
    _cache_policy_3_is_bit_identical_to_policy_0(case)
    _resident_padded_buffers_are_bit_identical_to_the_dense_run(case)
    _a_population_stride_is_bit_identical_to_the_dense_run(case)


class _Recording:
    """an observable that keeps the populations it was handed, on the host"""

    def __init__(self, observable):
        self.observable, self.context, self.seen = observable, observable.context, []

    def __call__(self, f):
        self.seen.append(f.detach().cpu().clone())
        return self.observable(f)


def _reported(case, context, f0, steps_, interval):
    coll, scheme, lat, res, kind = case[:5]
    equilibrium = lt.IncompressibleQuadraticEquilibrium(cases.equilibria.RHO0) if coll in cases.INCOMPRESSIBLE else None
    flow = cases.UniformFlow(context, list(res), 1, 0.01, STENCIL[lat](), equilibrium)
    boundary = cases.body(lat, res, kind)
    flow.boundaries = [boundary]
    flow.f = context.convert_to_tensor(f0.clone(), dtype=context.dtype)     # (the torch path steps in place)
    recording = _Recording(lt.BoundaryForce(flow, boundary))
    reporter = lt.ObservableReporter(recording, interval=interval, out=[])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        simulation = lt.Simulation(flow, cases.mirror_operator(coll, scheme, lat, flow), [reporter])
        simulation(steps_)
    return flow, simulation, recording.seen, [entry[2:] for entry in reporter.out], boundary


REPORTED = [c for c in PART_C if c[0] == 1] + [(0, None, "D3Q15", (6, 5, 7), "sphere", dt) for dt in ("f32", "f64")]


@pytest.mark.parametrize("case", REPORTED, ids=cases.part_c_id)
def test_a_force_reporter_under_simulation_reads_the_pending_pass(case):
    """12 steps, a BoundaryForce on the body every 3: the reporter reads flow.f while the deferred streaming pass of a
    link plan is pending"""
    coll, scheme, lat, res, kind, dt = case
    stencil = STENCIL[lat]()
    f0 = cases.state(lat, res, dt)
    flow, simulation, seen, forces, boundary = _reported(case, native(dt), f0, 12, 3)
    assert simulation._native is not None, "HIP engine not in use"
    cpu = {run: _reported(case, lt.Context("cpu", TORCH_DT[run], use_native=False), f0.to(TORCH_DT[run]), 12, 3)
           for run in {dt, "f64"}}
    what = cases.part_c_id(case)
    gates = _Gates(what, lat, dt)
    assert len(seen) == len(forces) == 5 and len(cpu["f64"][2]) == 5                  # i = 0, 3, 6, 9, 12
    for k in range(5):
        if k == 0 or coll == 0:                         # the state itself; the pass alone
            gates.same_bits(seen[k], cpu[dt][2][k].double().numpy(), f"{what} populations at report {k}")
        if k > 0:
            gates.hold(seen[k], cpu["f64"][2][k].numpy(), cpu[dt][2][k].double().numpy(), f"{what} populations at report {k}")
        exact = exact_link_force(stencil, seen[k], boundary.mask, boundary.fractions)
        assert_within_bound(forces[k], exact, TORCH_DT[dt], f"{what} report {k}, native context")
        host = exact_link_force(stencil, cpu[dt][2][k], boundary.mask, boundary.fractions)
        assert_within_bound(cpu[dt][3][k], host, TORCH_DT[dt], f"{what} report {k}, CPU context")
        if coll == 0 or dt == "f64" or k == 0:
            # the exact sum over the CPU populations of that step: the same bits without a collision; in fp64 the two
            # contexts' populations differ by a few 1e-16, the bound is (n - 1) 2^-53 sum |terms| = 2e-15 .. 2e-14
            assert_within_bound(forces[k], host, TORCH_DT[dt], f"{what} report {k}, native force over the CPU populations")
        else:
            # fp32 with a collision: two correct runs differ by 1e-7 per population, the bound is half an ulp of the
            # force (3e-9): the native force is tied to the CPU's through its own populations above
            errors = [abs(float(v) - e[0]) for v, e in zip(forces[k], host)]
            print(f"{what} report {k}: |native force - exact sum over the CPU populations| {errors}")
        assert any(float(v) != 0.0 for v in forces[k])
    gates.hold(flow.f, cpu["f64"][0].f.numpy(), cpu[dt][0].f.double().numpy(), f"{what} populations at the end")
    info = simulation._native.plan.last_run_info()
    assert info["two_step_launches"] == 0 and info["many_step_launches"] == 0, info
    gates.check()


# ------------------------------------------------------------------------------- D. D3Q15: the summation order
@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("res", [[6, 5, 7], [3, 3, 5]], ids=["6x5x7", "3x3x5"])
def test_d3q15_link_force_has_the_bits_of_the_documented_summation_order(res, dt):
    """every node x the directions 1 .. 14 as a synthetic sorted list: the order of link_bounce.hpp and reduce.hpp,
    emulated on the host (fixed_order_sum.py), predicts the bytes (the fp64 plans pin the order; fp32 terms widened to
    fp64 add exactly, so those cases show that every item is taken exactly once)"""
    import fixed_order_sum as fos
    from lettuce_amd import _native
    lat = "D3Q15"
    stencil = STENCIL[lat]()
    nodes_total = int(np.prod(res))
    nodes = np.repeat(np.arange(nodes_total), stencil.q - 1)
    directions = np.tile(np.arange(1, stencil.q), nodes_total)
    n_links = len(nodes)
    f = signed_state(lat, res, dt)
    e = np.array(stencil.e, dtype=np.int64)
    opposite = np.array([int(o) for o in stencil.opposite])
    x_s = np.stack(np.unravel_index(nodes, res), axis=1)
    x_f = (x_s + e[directions]) % np.array(res)
    q = opposite[directions]
    values = f.double().numpy()
    out = values[q, x_s[:, 0], x_s[:, 1], x_s[:, 2]]
    back = values[directions, x_f[:, 0], x_f[:, 1], x_f[:, 2]]
    items = np.zeros((stencil.d, n_links, 2))
    for c in range(stencil.d):
        sign = np.sign(e[q, c]).astype(np.float64)
        items[c, :, 0], items[c, :, 1] = np.where(sign != 0, sign * out, 0.0), np.where(sign != 0, sign * back, 0.0)
    want = np.asarray(fos.link_force(items), dtype=np.float64)
    plan = _native.Plan(lat, TORCH_DT[dt], "none", res, [{"kind": "link_bounce_back"}])
    coefficient = torch.zeros(n_links, dtype=TORCH_DT[dt])
    assert plan.set_links(0, nodes, directions, coefficient, coefficient, np.zeros(n_links, dtype=np.uint8)) == n_links
    got = plan.link_force(0, f.cuda()).cpu().numpy()
    few = plan.link_force(0, f.cuda()).cpu().numpy()
    print(f"D3Q15 {res} {n_links} links {dt}: got {got.tolist()!r}, emulation {want.tolist()!r}")
    assert got.dtype == np.float64 and got.tobytes() == want.tobytes() and few.tobytes() == got.tobytes()
    # its first 5 links alone: a sum that does not cancel
    head = _native.Plan(lat, TORCH_DT[dt], "none", res, [{"kind": "link_bounce_back"}])
    assert head.set_links(0, nodes[:5], directions[:5], coefficient[:5], coefficient[:5], np.zeros(5, dtype=np.uint8)) == 5
    got = head.link_force(0, f.cuda()).cpu().numpy()
    want = np.asarray(fos.link_force(items[:, :5]), dtype=np.float64)
    print(f"D3Q15 {res} 5 links {dt}: got {got.tolist()!r}, emulation {want.tolist()!r}")
    assert bool((got != 0).all()) and got.tobytes() == want.tobytes()
