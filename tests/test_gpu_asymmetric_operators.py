"""Every operator that agrees with the reference "at rounding level" -- KBC, Smagorinsky, TRT, the regularised collision,
Guo and Shan-Chen forcing (BGK and Smagorinsky), the anti-bounce-back outlet and EquilibriumOutletP -- on states away
from rho = 1: the fp64 parity test and the fp32 error-budget test of test_gpu_smagorinsky.py, test_gpu_relaxations.py,
test_gpu_force.py, test_gpu_fp32_error_budget.py and test_gpu_outlet_p_fp32_error_budget.py with the state swapped
for asymmetric_states.asymmetric_state (their CPU paths, plans and error measure reused by import).

    moderate  rho in 0.5 .. 1.5            tau = 0.501, 0.7, 1.7    1 and 5 steps
    wide      rho in 1 / 20 .. 20          tau = 0.7, 1.7           1 step (five steps diverge on the CPU at tau <= 0.7)

fp64: |gpu - cpu_fp64| <= ATOL["f64"] max(1, max|f|), times 10 with an outlet (the bound of the files named above).
fp32: E_gpu <= 4 E_ref with E = max |. - cpu_fp64| / w_q and E_ref the CPU path's own fp32 error from the same fp32
state.  That E_ref is a yardstick (finite runs, an error in every weight class, 1e-7 < E_ref < 1e-4) is checked without
a GPU in test_asymmetric_operators_host.py; the measured ratios are in DESIGN.md section 2.

KBC's branch is a discontinuity: the nodes whose gamma lies within the CPU path's own fp32 uncertainty of the threshold
(asymmetric_states.MARGIN) are left out, at every step a case runs; the populations such a node sends out are left out
with it.  A case with such a node after its first step runs that one step only.  Both stabiliser lines themselves are
pinned by test_gpu_kbc_branch.py.

Launcher identity: where an operator has a kernel of two or of many steps per launch, that launch returns the bits of
one-step launches on the wide state too.
"""
import functools

import numpy as np
import pytest
import torch

import asymmetric_states as st
import lettuce_amd as lt
from conftest import TORCH_DT
from oracle import lettuce_oracle as orc
from outlet_p_cases import mirror_flow
from test_gpu_engine import ATOL, _masked_case, dev
from test_gpu_fp32_error_budget import FACTOR, GRID
from test_gpu_paths_vs_oracle import _Feq, _Oracle, _oracle_boundary
import test_gpu_force as forces
import test_gpu_outlet_p_fp32_error_budget as outlet_p
import test_gpu_relaxations as relaxations
import test_gpu_relaxations_fp32_error_budget as relaxations_budget
import test_gpu_smagorinsky as smagorinsky

pytestmark = pytest.mark.gpu

SEED = 7
SETTINGS = [(kind, tau, steps) for kind, taus, steps in (("moderate", (0.501, 0.7, 1.7), (1, 5)), ("wide", (0.7, 1.7), (1,)))
            for tau in taus]
SETTING_IDS = [f"{kind}-tau{tau}" for kind, tau, _ in SETTINGS]
# a case whose ratio honestly exceeds 4: the rule of FACTORS in test_gpu_fp32_error_budget.py
FACTORS = {}


def _directions(lat):
    return [(axis, side) for axis in range(orc.LATTICES[lat].d) for side in (1, -1)]


def _op(oid, family, lat, **what):
    return (oid, family, lat, tuple(sorted(what.items())))


OPERATORS = (
    [_op(f"kbc-periodic-{lat.lower()}", "oracle", lat, coll="kbc", abb=None, masked=False) for lat in ("D2Q9", "D3Q27")]
    + [_op("kbc-masked-d2q9", "oracle", "D2Q9", coll="kbc", abb=(0, -1), masked=True),
       _op("kbc-masked-d3q27", "oracle", "D3Q27", coll="kbc", abb=(0, 1), masked=True)]
    + [_op(f"bgk-outlet-{lat.lower()}-{'xyz'[axis]}{'+' if side > 0 else '-'}", "oracle", lat, coll="bgk", abb=(axis, side),
           masked=True) for lat in ("D2Q9", "D3Q19", "D3Q27") for axis, side in _directions(lat)]
    + [_op(f"smagorinsky-{name}-{lat.lower()}", "smagorinsky", lat, constant=constant)
       for lat in ("D2Q9", "D3Q19", "D3Q27") for name, constant in (("default", 0.17), ("strong", 1.0))]
    + [_op(f"{scheme}-{operator}-{lat.lower()}", "force", lat, scheme=scheme, operator=operator)
       for lat in ("D2Q9", "D3Q19") for scheme, operator in (("guo", "bgk"), ("shanchen", "bgk"), ("guo", "smagorinsky"))]
    + [_op(f"{operator}-{lat.lower()}", "relaxation", lat, operator=operator)
       for operator in relaxations.OPERATORS for lat in ("D2Q9", "D3Q19", "D3Q27")]
    + [_op(f"outlet-p-{lat.lower()}", "outlet_p", lat) for lat in ("D2Q9", "D3Q19", "D3Q27")]
)
OPERATOR_IDS = [op[0] for op in OPERATORS]
FORCED_SMAGORINSKY_CONSTANT = 1.0


def state(lat, kind, dt):
    """the state of a case: float64 for f64, rounded to fp32 for f32"""
    f = st.asymmetric_state(lat, GRID[lat], kind, SEED)
    return f.float() if dt == "f32" else f


def has_outlet(op):
    _, family, _, what = op
    return family == "outlet_p" or dict(what).get("abb") is not None


def _masks(lat, abb, dtype):
    _, ncm, nsm, entries = _masked_case(lat, GRID[lat], dtype, abb, 43)
    return ncm, nsm, entries


# --------------------------------------------------------------------------- the CPU paths
class _Stepper:
    """lt.Simulation behind the oracle's interface"""

    def __init__(self, flow, sim):
        self.flow, self.sim = flow, sim

    @property
    def f(self):
        return self.flow.f

    def step(self, n):
        self.sim(n)


def cpu_simulation(op, tau, f0, table_dtype):
    """the CPU path of an operator in f0's dtype; table_dtype: the dtype of the plan (its feq table is rounded to it)"""
    _, family, lat, what = op
    what = dict(what)
    L = orc.LATTICES[lat]
    if family == "oracle":
        sim = _Oracle(L, f0.clone(), what["coll"], tau)
        if what["masked"]:
            ncm, nsm, entries = _masks(lat, what["abb"], table_dtype)
            sim.boundaries = [_oracle_boundary(L, e, table_dtype) for e in entries]
            for b in sim.boundaries:
                if isinstance(b, _Feq):
                    b.feq = b.feq.to(f0.dtype)
            sim.no_collision_mask, sim.no_streaming_mask = ncm, nsm
        return sim
    if family == "smagorinsky":
        sim = smagorinsky._Reference(L, f0.clone(), "smagorinsky", tau)
        sim.constant = what["constant"]
        return sim
    if family == "force":
        sim = forces._Reference(L, f0.clone(), what["operator"], tau)
        sim.scheme, sim.operator = what["scheme"], what["operator"]
        sim.constant = FORCED_SMAGORINSKY_CONSTANT if what["operator"] == "smagorinsky" else None
        sim.acceleration = forces.ACCELERATION[:L.d]
        return sim
    if family == "relaxation":
        sim = relaxations._Reference(L, f0.clone(), what["operator"], tau)
        sim.operator, sim.tau_minus = what["operator"], relaxations_budget.tau_minus_of(tau)
        return sim
    flow = mirror_flow(outlet_p.description(lat), f"outlet_p_asymmetric_{lat.lower()}_f32",
                       lt.Context("cpu", f0.dtype, use_native=False), set_f0=False)
    flow.f = f0.clone()
    return _Stepper(flow, lt.Simulation(flow, lt.BGKCollision(tau), []))


def _fluid(sim):
    ncm = getattr(sim, "no_collision_mask", None)
    return None if ncm is None else (ncm == 0)


@functools.lru_cache(maxsize=None)
def cpu_pair(op, kind, tau, dt, steps):
    """({n: (cpu in dt, cpu in fp64)}, {n: populations [q, *res] to leave out}, the number of excluded nodes) for n in
    steps, from the state in dt.  Nothing is left out except for KBC."""
    _, family, lat, what = op
    L = orc.LATTICES[lat]
    f0 = state(lat, kind, dt)
    kbc = dict(what).get("coll") == "kbc"
    sims = [cpu_simulation(op, tau, f0.to(dtype), TORCH_DT[dt]) for dtype in (f0.dtype, torch.float64)]
    out, drop, done, nodes = {}, {}, 0, 0
    dropped = torch.zeros([L.q] + GRID[lat], dtype=torch.bool)
    for n in steps:
        for _ in range(n - done):
            if kbc:
                # (fp64 cases: the set of the fp32 state's own CPU runs would need that state; the state's fp32
                # rounding stands in for it, which moves gamma by as much as the fp32 arithmetic does)
                g_own = st.kbc_gamma(sims[0].f.float(), tau)[0].double()
                g_64 = st.kbc_gamma(sims[1].f, tau)[0]
                excluded = g_64.abs() <= st.MARGIN * (g_own - g_64).abs()
                fluid = _fluid(sims[1])
                if fluid is not None:
                    excluded &= fluid
                # what an excluded node holds after the step, and what it sends to its neighbours -- and every
                # population that has met a left-out one in a later collision (none: see `steps_of`)
                sent = torch.stack([torch.roll(excluded, shifts=tuple(L.e[q]), dims=tuple(range(L.d))) for q in range(L.q)])
                new = sent | excluded[None]
                if dropped.any() or (done > 0 and new.any()):
                    raise AssertionError("an excluded node after the first step: run this case for one step only")
                dropped |= new
                nodes += int(excluded.sum())
            for sim in sims:
                sim.step(1)
            done += 1
        assert sims[0].f.dtype == f0.dtype and sims[1].f.dtype == torch.float64
        out[n] = tuple(sim.f.double().numpy().copy() for sim in sims)
        drop[n] = dropped.numpy().copy()
    return out, drop, nodes


def steps_of(op, kind, tau, dt, steps):
    """the steps a case runs: KBC with a node within the margin of the threshold after its first step runs one step"""
    if dict(op[3]).get("coll") != "kbc" or steps == (1,):
        return steps
    try:
        cpu_pair(op, kind, tau, dt, steps)
        return steps
    except AssertionError:
        return (1,)


def weighted_error(lat, got, want, drop):
    """max over q and the nodes kept of |got - want| / w_q, per population"""
    L = orc.LATTICES[lat]
    err = np.where(drop, 0.0, np.abs(np.asarray(got, dtype=np.float64) - want))
    return err.reshape(L.q, -1).max(axis=1) / np.asarray(L.w)


def reference_error(op, kind, tau, n, steps):
    """E_ref of the fp32 case after checking what the gate assumes: finite runs, an error in every weight class"""
    lat = op[2]
    pairs, drop, _ = cpu_pair(op, kind, tau, "f32", steps)
    own, want = pairs[n]
    assert np.isfinite(own).all() and np.isfinite(want).all()
    per_q = weighted_error(lat, own, want, drop[n])
    for w in sorted(set(orc.LATTICES[lat].w)):
        members = [q for q, wq in enumerate(orc.LATTICES[lat].w) if wq == w]
        assert per_q[members].max() > 0, f"no fp32 error in the weight class {w}"
    return float(per_q.max())


# --------------------------------------------------------------------------- the plans
def gpu_plan(op, dt, tau):
    from lettuce_amd._native import Plan
    _, family, lat, what = op
    what, dtype, res = dict(what), TORCH_DT[dt], GRID[lat]
    if family == "oracle":
        if not what["masked"]:
            return Plan(lat, dtype, what["coll"], res, [])
        ncm, nsm, entries = _masks(lat, what["abb"], dtype)
        plan = Plan(lat, dtype, what["coll"], res, entries)
        plan.set_masks(dev(ncm), dev(nsm))
        return plan
    if family == "smagorinsky":
        plan = Plan(lat, dtype, "smagorinsky", res, [])
        plan.set_smagorinsky(what["constant"])
        return plan
    if family == "force":
        plan = Plan(lat, dtype, what["operator"], res, [])
        if what["operator"] == "smagorinsky":
            plan.set_smagorinsky(FORCED_SMAGORINSKY_CONSTANT)
        plan.set_force(forces.ACCELERATION[:len(res)], *forces.scales(what["scheme"], tau))
        return plan
    if family == "relaxation":
        return relaxations.make_plan(what["operator"], lat, dt, res, tau_minus=relaxations_budget.tau_minus_of(tau))
    stepper = cpu_simulation(op, tau, state(lat, "moderate", dt), dtype)
    flow, sim = stepper.flow, stepper.sim
    entries = [b.native_generator(i).plan_entry(flow) for i, b in enumerate(sim.boundaries[1:], start=1)]
    assert [e["kind"] for e in entries] == ["bounce_back", "equilibrium", "pressure_outlet"]
    plan = Plan(lat, dtype, "bgk", res, entries)
    plan.set_masks(dev(sim.no_collision_mask.to(torch.uint8)), dev(sim.no_streaming_mask.to(torch.uint8)))
    return plan


# --------------------------------------------------------------------------- the tests
@pytest.mark.parametrize("kind,tau,steps", SETTINGS, ids=SETTING_IDS)
@pytest.mark.parametrize("op", OPERATORS, ids=OPERATOR_IDS)
def test_fp64_parity_with_the_cpu_path(op, kind, tau, steps):
    lat = op[2]
    steps = steps_of(op, kind, tau, "f64", steps)
    plan = gpu_plan(op, "f64", tau)
    f0 = state(lat, kind, "f64")
    pairs, drop, _ = cpu_pair(op, kind, tau, "f64", steps)
    for n in steps:
        want = pairs[n][1]
        a = dev(f0)
        out, _ = plan.run(a, torch.empty_like(a), tau, n)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert got.dtype == np.float64 and np.isfinite(got).all()
        tol = ATOL["f64"] * max(1.0, float(np.abs(want).max())) * (10 if has_outlet(op) else 1)
        diff = float(np.where(drop[n], 0.0, np.abs(got - want)).max())
        print(f"{op[0]} {kind} tau {tau} n = {n}: max |gpu - cpu| {diff:.3e} (bound {tol:.1e}, {int(drop[n].sum())} populations "
              f"left out, kernel {plan.kernel_name().split('<')[0]})")
        assert diff <= tol


@pytest.mark.parametrize("kind,tau,steps", SETTINGS, ids=SETTING_IDS)
@pytest.mark.parametrize("op", OPERATORS, ids=OPERATOR_IDS)
def test_fp32_error_within_the_reference_arithmetics_own(request, op, kind, tau, steps):
    lat = op[2]
    steps = steps_of(op, kind, tau, "f32", steps)
    plan = gpu_plan(op, "f32", tau)
    f0 = state(lat, kind, "f32")
    factor = FACTORS.get(request.node.callspec.id, FACTOR)
    pairs, drop, _ = cpu_pair(op, kind, tau, "f32", steps)
    failures = []
    for n in steps:
        e_ref = reference_error(op, kind, tau, n, steps)
        a = dev(f0)
        out, _ = plan.run(a, torch.empty_like(a), tau, n)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert got.dtype == np.float32 and np.isfinite(got).all()
        e_gpu = float(weighted_error(lat, got, pairs[n][1], drop[n]).max())
        print(f"{op[0]} {kind} tau {tau} n = {n}: E_ref {e_ref:.3e}  E_gpu {e_gpu:.3e}  ratio {e_gpu / e_ref:.2f}  "
              f"(gate {factor:g}, {int(drop[n].sum())} populations left out, kernel {plan.kernel_name().split('<')[0]})")
        if not e_gpu <= factor * e_ref:
            failures.append((n, e_ref, e_gpu, e_gpu / e_ref))
    assert not failures, f"(n, E_ref, E_gpu, ratio) beyond {factor:g} x E_ref: {failures}"


# --------------------------------------------------------------------------- launcher identity on the wide state
TWO_STEP_GRID = [2, 8, 64]                     # one 64 x 8 tile that is its own neighbour
WIDE_TAU = 0.7


def _plan_of(operator, lat, dt, res):
    from lettuce_amd._native import Plan
    if operator == "smagorinsky":
        return smagorinsky.smagorinsky_plan(lat, dt, res, 1.0)
    if operator == "forced-bgk":
        plan = Plan(lat, TORCH_DT[dt], "bgk", res, [])
        plan.set_force(forces.ACCELERATION[:len(res)], *forces.scales("guo", WIDE_TAU))
        return plan
    return relaxations.make_plan(operator, lat, dt, res, tau_minus=relaxations_budget.tau_minus_of(WIDE_TAU))


@pytest.mark.parametrize("operator,coll", [("smagorinsky", 3), ("forced-bgk", 5), ("trt", 8), ("regularized", 9)])
def test_two_step_launch_equals_two_single_steps_on_the_wide_state(operator, coll):
    plan = _plan_of(operator, "D3Q19", "f32", TWO_STEP_GRID)
    f = dev(st.asymmetric_state("D3Q19", TWO_STEP_GRID, "wide", SEED).float())
    a, b, c = torch.empty_like(f), torch.empty_like(f), torch.full_like(f, float("nan"))
    plan.stream_collide(f, a, WIDE_TAU)
    plan.stream_collide(a, b, WIDE_TAU)
    plan.set_two_step(1)
    assert plan.two_step_admitted() is None
    assert plan.kernel_name().startswith(f"lbm2_kernel<float, lt::d3q19, 0, {coll}, 64, 8,"), plan.kernel_name()
    plan.stream_collide_twice(f, c, WIDE_TAU)
    torch.cuda.synchronize()
    assert torch.isfinite(b).all() and float((b - f).abs().max()) > 1e-4
    assert torch.equal(c, b)


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_many_step_kbc_launch_equals_single_steps_on_the_wide_state(dt):
    from lettuce_amd._native import Plan
    res, tau = [8, 64], 1.7
    plan = Plan("D2Q9", TORCH_DT[dt], "kbc", res, [])
    plan.set_many_step(1)
    assert plan.kernel_name().startswith("lbm_many_kernel"), plan.kernel_name()
    f = dev(st.asymmetric_state("D2Q9", res, "wide", SEED).to(TORCH_DT[dt]))
    a, b = f.clone(), torch.empty_like(f)
    for k in (1, 2, 3):
        plan.stream_collide(a, b, tau)
        a, b = b, a
        got = torch.full_like(f, float("nan"))
        plan.stream_collide_many(f, got, tau, k)
        torch.cuda.synchronize()
        assert torch.isfinite(a).all() and torch.equal(got, a), k


# --------------------------------------------------------------------------- the reference's own vectors (host tests)
FIXTURE_CASES = (("moderate", 0.501, (1, 5)), ("wide", 0.7, (1,)), ("wide", 1.7, (1,)))


def fixture_runs(op, fixture):
    """(what, the CPU path's float64 result, the reference's) for every case of tests/golden/asymmetric_<fixture>_<lattice>_f64
    (oracle/gen_golden.py, asymmetric_cases): the collided field and the populations after 1 (and 5) steps, from the
    states asymmetric_states.py regenerates bit for bit"""
    from conftest import golden
    lat = op[2]
    g, s = golden(f"asymmetric_{fixture}_{lat.lower()}_f64"), golden(f"asymmetric_states_{lat.lower()}_f64")
    res = [int(r) for r in s["resolution"]]
    assert g["acceleration"].tolist() == list(forces.ACCELERATION[:len(res)])
    for kind, tau, steps in FIXTURE_CASES:
        f0 = st.asymmetric_state(lat, res, kind, int(s[f"seed_{kind}"]))
        assert f0.numpy().tobytes() == s[f"f0_{kind}"].tobytes()
        key = f"{kind}_tau{tau}"
        sim = cpu_simulation(op, float(g[key + "_tau_used"]), f0, torch.float64)
        yield f"{key} collided", sim._collision(sim.f).numpy(), g[key + "_collided"]
        done = 0
        for n in steps:
            sim.step(n - done)
            done = n
            yield f"{key} f{n}", sim.f.numpy(), g[f"{key}_f{n}"]
