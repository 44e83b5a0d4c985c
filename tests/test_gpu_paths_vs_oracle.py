"""Each kernel lt_run can choose, pinned against the CPU oracle in float64.

The rest of the GPU suite mostly holds one kernel against another (two-step against two one-step launches, fused
against collide + stream, resident against dense), so an error both paths share, or one in lt_run's bookkeeping
(the first collide-only step, the deferred last stream, lt_continue from f*, the odd remainder step, resident load /
store, graph chunks), would pass there.  Here every case names the kernel lt_run must land on and the launches it
must count -- a quiet fall-back to the one-step kernel fails -- and compares n in {1, 2, 3, 8} steps and a batch
split 3 + 5 with the oracle stepping the same (fp32: the same fp32) initial state in float64.

Tolerances as in test_gpu_engine.py: fp64 1e-12 max|f|, fp32 1e-5 max|f| max(1, n / 10), ten times that with an
anti-bounce-back outlet.  Not bit identity: the oracle's einsum order depends on the CPU's BLAS.
"""
import functools
import math

import numpy as np
import pytest
import torch

from conftest import TORCH_DT
from oracle import lettuce_oracle as orc
from test_gpu_engine import ATOL, _masked_case, dev, plan_for

pytestmark = pytest.mark.gpu

TAU = 0.7
STEPS = (1, 2, 3, 8)


# --------------------------------------------------------------------------- the oracle, with the engine's boundaries
class _Feq:
    """an equilibrium boundary as a plan holds it: one feq per population (the table) or per node (a field)"""
    kind = "feq"

    def __init__(self, feq):
        self.feq = feq


class _Oracle(orc.OracleSimulation):
    def _boundary(self, b, f):
        if b.kind == "feq":
            return b.feq.expand_as(f).clone()
        return super()._boundary(b, f)


def _oracle_boundary(L, entry, dtype):
    if entry["kind"] == "bounce_back":
        return orc.OracleBoundary("bounce_back")
    if entry["kind"] == "abb_outlet":
        direction = [0] * L.d
        direction[entry["axis"]] = entry["side"]
        return orc.OracleBoundary("abb_outlet", direction=direction)
    if "field" in entry:
        return _Feq(entry["field"].detach().cpu().double())
    # the plan keeps its table in its own dtype
    feq = torch.tensor(entry["feq"], dtype=torch.float64).to(dtype).double()
    return _Feq(feq.reshape([-1] + [1] * L.d))


def oracle(lat, f0, coll, entries=(), ncm=None, nsm=None):
    """OracleSimulation in float64 from f0 (promoted), with the plan's boundaries in the plan's index order"""
    L = orc.LATTICES[lat]
    sim = _Oracle(L, f0.double().clone(), coll, TAU)
    if ncm is not None:
        sim.boundaries = [_oracle_boundary(L, e, f0.dtype) for e in entries]
        sim.no_collision_mask, sim.no_streaming_mask = ncm.cpu(), nsm.cpu()
    return sim


def assert_close(got, want, dt, n, outlet):
    scale = (max(1.0, n / 10) if dt == "f32" else 1.0) * (10 if outlet else 1)
    tol = ATOL[dt] * max(1.0, float(np.abs(want).max())) * scale
    np.testing.assert_allclose(got, want, rtol=0, atol=tol)


def perturbed_state(lat, res, dtype, seed):
    """equilibria of a random density around 1 and a non-zero mean velocity, times 1 + 5 % noise per population: every
    moment, the higher-order ones included, is resolved (KBC's gamma is well conditioned on it)"""
    L = orc.LATTICES[lat]
    g = torch.Generator().manual_seed(seed)
    e, w = orc.lattice_tensors(L, torch.float64)
    rho = 1 + 0.05 * (torch.rand(res, generator=g, dtype=torch.float64) - 0.5)
    u0 = torch.tensor([0.05, -0.03, 0.02][:L.d], dtype=torch.float64).reshape([-1] + [1] * L.d)
    u = u0 + 0.02 * (torch.rand([L.d] + res, generator=g, dtype=torch.float64) - 0.5)
    feq = orc.quadratic_equilibrium(rho, u, e, w)
    return (feq * (1 + 0.05 * (2 * torch.rand([L.q] + res, generator=g, dtype=torch.float64) - 1))).to(dtype)


# --------------------------------------------------------------------------- the path matrix
# (id, lattice, dtype, collision, resolution, masks, switches, kernel, launches)
#   masks: None (periodic) or (outlet (axis, side) | None, per-node equilibrium field, inlet face opposite the outlet)
#   switches: what the plan is told before it runs (empty: lt_run's automatic choice)
#   launches: "two" = pairs + the odd remainder, "many" = launches of up to 8 steps (7 with an outlet), "one"
def _case(cid, lat, dt, coll, res, masks, switches, kernel, launches):
    return pytest.param(lat, dt, coll, res, masks, switches, kernel, launches, id=cid)


TWO = {"two_step": 1}
TWO_2D = {"two_step": 1, "many_step": 0}
LBM2 = [
    _case("lbm2-d3q19-f32-3x3-tiles", "D3Q19", "f32", "bgk", [6, 24, 192], None, TWO, "lbm2_kernel", "two"),
    _case("lbm2-d3q19-f64", "D3Q19", "f64", "bgk", [5, 24, 96], None, TWO, "lbm2_kernel", "two"),
    _case("lbm2-d3q15-f32", "D3Q15", "f32", "bgk", [6, 16, 128], None, TWO, "lbm2_kernel", "two"),
    _case("lbm2-d3q15-f64", "D3Q15", "f64", "bgk", [5, 8, 64], None, TWO, "lbm2_kernel", "two"),
    _case("lbm2-d3q27-f32", "D3Q27", "f32", "bgk", [6, 12, 128], None, TWO, "lbm2_kernel", "two"),
    _case("lbm2-d3q19-f32-48x64x256", "D3Q19", "f32", "bgk", [48, 64, 256], None, TWO, "lbm2_kernel", "two"),
]
LBM2M = [
    # the outlet on the last plane of the sweep (reference layout: x = last, AX = 2)
    _case("lbm2m-ax2-d3q19-f32", "D3Q19", "f32", "bgk", [6, 16, 128], ((0, 1), False, False), TWO, "lbm2m_kernel", "two"),
    _case("lbm2m-ax2-d3q19-f32-field", "D3Q19", "f32", "bgk", [5, 8, 64], ((0, 1), True, False), TWO, "lbm2m_kernel", "two"),
    _case("lbm2m-ax2-d3q15-f32", "D3Q15", "f32", "bgk", [5, 8, 64], ((0, 1), False, False), TWO, "lbm2m_kernel", "two"),
    _case("lbm2m-ax2-d3q15-f64-field", "D3Q15", "f64", "bgk", [6, 8, 64], ((0, 1), True, False), TWO, "lbm2m_kernel", "two"),
    _case("lbm2m-ax2-d3q27-f32", "D3Q27", "f32", "bgk", [6, 8, 64], ((0, 1), False, False), TWO, "lbm2m_kernel", "two"),
    _case("lbm2m-no-outlet-d3q19-f32", "D3Q19", "f32", "bgk", [5, 8, 64], (None, True, False), TWO, "lbm2m_kernel", "two"),
    # the outlet at an end of the rows (z = last or z = 0, AX = 0), an inlet face of equilibrium nodes opposite
    _case("lbm2m-ax0+-d3q19-f32", "D3Q19", "f32", "bgk", [5, 16, 128], ((2, 1), False, True), TWO, "lbm2m_kernel", "two"),
    _case("lbm2m-ax0--d3q19-f32-field", "D3Q19", "f32", "bgk", [6, 8, 64], ((2, -1), True, True), TWO, "lbm2m_kernel", "two"),
    _case("lbm2m-ax0+-d3q15-f32", "D3Q15", "f32", "bgk", [5, 8, 64], ((2, 1), False, True), TWO, "lbm2m_kernel", "two"),
    _case("lbm2m-ax0--d3q15-f64", "D3Q15", "f64", "bgk", [4, 16, 64], ((2, -1), False, True), TWO, "lbm2m_kernel", "two"),
    _case("lbm2m-ax0+-d3q27-f32-field", "D3Q27", "f32", "bgk", [5, 4, 64], ((2, 1), True, True), TWO, "lbm2m_kernel", "two"),
    _case("lbm2m-ax0--d3q27-f32", "D3Q27", "f32", "bgk", [4, 8, 128], ((2, -1), False, True), TWO, "lbm2m_kernel", "two"),
]
TWO_2D_CASES = [
    _case("lbm2d2-d2q9-f32", "D2Q9", "f32", "bgk", [12, 128], None, TWO_2D, "lbm2d2_kernel", "two"),
    _case("lbm2d2-d2q9-f64", "D2Q9", "f64", "bgk", [10, 192], None, TWO_2D, "lbm2d2_kernel", "two"),
    _case("lbm2d2m-d2q9-f32", "D2Q9", "f32", "bgk", [12, 64], ((0, 1), False, False), TWO_2D, "lbm2d2m_kernel", "two"),
    _case("lbm2d2m-d2q9-f64-field", "D2Q9", "f64", "bgk", [9, 128], ((0, 1), True, False), TWO_2D, "lbm2d2m_kernel", "two"),
    _case("lbm2d2m-no-outlet-d2q9-f32", "D2Q9", "f32", "bgk", [10, 192], (None, False, False), TWO_2D, "lbm2d2m_kernel", "two"),
]
MANY = [
    _case("many-d2q9-f32", "D2Q9", "f32", "bgk", [24, 32], None, {}, "lbm_many_kernel", "many"),
    _case("many-masked-d2q9-f64", "D2Q9", "f64", "bgk", [24, 16], ((0, 1), False, False), {}, "lbm_many_kernel", "many"),
    _case("many-masked-d2q9-f32-field", "D2Q9", "f32", "bgk", [16, 32], ((1, -1), True, False), {}, "lbm_many_kernel", "many"),
    _case("many-kbc-d2q9-f64", "D2Q9", "f64", "kbc", [16, 24], None, {"many_step": 1}, "lbm_many_kernel", "many"),
    _case("many-kbc-masked-d2q9-f32", "D2Q9", "f32", "kbc", [24, 16], ((0, 1), False, False), {"many_step": 1},
          "lbm_many_kernel", "many"),
]
ONE_STEP_KBC = [
    _case("one-kbc-masked-d3q27-f32", "D3Q27", "f32", "kbc", [6, 8, 10], ((0, 1), False, False), {}, "lbm_kernel", "one"),
    _case("one-kbc-masked-d3q27-f64", "D3Q27", "f64", "kbc", [5, 6, 8], ((2, -1), True, False), {}, "lbm_kernel", "one"),
    _case("one-kbc-masked-d2q9-f64", "D2Q9", "f64", "kbc", [12, 10], ((1, 1), False, False), {}, "lbm_kernel", "one"),
    _case("one-kbc-masked-d2q9-f32", "D2Q9", "f32", "kbc", [16, 24], ((0, -1), True, False), {}, "lbm_kernel", "one"),
]
PATHS = LBM2 + LBM2M + TWO_2D_CASES + MANY + ONE_STEP_KBC


def _build(lat, dt, coll, res, masks, switches, seed=3):
    """(plan, f0, oracle entries): the plan with its switches set; f0 a perturbed state in the plan's dtype"""
    dtype = TORCH_DT[dt]
    f0 = perturbed_state(lat, res, dtype, seed)
    if masks is None:
        plan, entries, ncm, nsm = plan_for(lat, dtype, coll, res), (), None, None
    else:
        abb, with_field, inlet_face = masks
        _, ncm, nsm, entries = _masked_case(lat, res, dtype, abb, seed + 40, with_field=with_field,
                                            inlet_face=inlet_face)
        plan = plan_for(lat, dtype, coll, res, entries)
        plan.set_masks(dev(ncm), dev(nsm))
    setters = {"two_step": plan.set_two_step, "many_step": plan.set_many_step, "graph": plan.set_graph_mode,
               "resident": plan.set_resident}
    for key, value in switches.items():
        setters[key](value)
    return plan, f0, (entries, ncm, nsm)


@functools.lru_cache(maxsize=None)
def _oracle_snapshots(lat, dt, coll, res, masks, seed=3):
    """the oracle's populations after each n of STEPS (one run, stepped on): shared by the dense and resident runs"""
    dtype = TORCH_DT[dt]
    f0 = perturbed_state(lat, list(res), dtype, seed)
    if masks is None:
        sim = oracle(lat, f0, coll)
    else:
        abb, with_field, inlet_face = masks
        _, ncm, nsm, entries = _masked_case(lat, list(res), dtype, abb, seed + 40, with_field=with_field,
                                            inlet_face=inlet_face)
        sim = oracle(lat, f0, coll, entries, ncm, nsm)
    out, done = {}, 0
    for n in STEPS:
        sim.step(n - done)
        done = n
        out[n] = sim.f.numpy().copy()
    return out


def expected_launches(launches, fused, outlet):
    """last_run_info after `fused` stream-collide steps of lt_run / lt_continue / lt_resident_advance"""
    if launches == "two":
        return {"single_step_launches": fused % 2, "two_step_launches": fused // 2, "many_step_launches": 0}
    if launches == "many" and fused >= 2:
        return {"single_step_launches": 0, "two_step_launches": 0,
                "many_step_launches": math.ceil(fused / (7 if outlet else 8))}
    return {"single_step_launches": fused, "two_step_launches": 0, "many_step_launches": 0}


def _kernel(plan):
    return plan.kernel_name().split("<")[0]


def _assert_kernel(plan, kernel):
    name = _kernel(plan)
    assert name == kernel or (kernel == "lbm_kernel" and name == "lbm_kernel_occ4"), plan.kernel_name()


@pytest.mark.parametrize("lat,dt,coll,res,masks,switches,kernel,launches", PATHS)
def test_lt_run_path_against_the_oracle(lat, dt, coll, res, masks, switches, kernel, launches):
    plan, f0, _ = _build(lat, dt, coll, res, masks, switches)
    _assert_kernel(plan, kernel)
    want = _oracle_snapshots(lat, dt, coll, tuple(res), masks)
    outlet = masks is not None and masks[0] is not None
    for n in STEPS:
        a = dev(f0)
        out, _ = plan.run(a, torch.empty_like(a), TAU, n)
        torch.cuda.synchronize()
        assert plan.last_run_info() == expected_launches(launches, n - 1, outlet), (n, plan.last_run_info())
        assert_close(out.cpu().numpy(), want[n], dt, n, outlet)
    # 3 + 5 through lt_continue from the post-collision populations lt_run leaves in its other buffer
    a = dev(f0)
    result, fstar = plan.run(a, torch.empty_like(a), TAU, 3)
    out, _ = plan.run(fstar, result, TAU, 5, from_fstar=True)
    torch.cuda.synchronize()
    assert plan.last_run_info() == expected_launches(launches, 5, outlet), plan.last_run_info()
    assert_close(out.cpu().numpy(), want[8], dt, 8, outlet)
    # ... and with the last stream deferred (what lt.Simulation runs): the caller streams f* itself
    plan.set_deferred_stream(True)
    try:
        a = dev(f0)
        fstar, scratch = plan.run(a, torch.empty_like(a), TAU, 3)
        fstar, scratch = plan.run(fstar, scratch, TAU, 5, from_fstar=True)
    finally:
        plan.set_deferred_stream(False)
    out = plan.stream(fstar, scratch)
    torch.cuda.synchronize()
    assert_close(out.cpu().numpy(), want[8], dt, 8, outlet)
    if masks is not None and launches == "two":
        assert plan.canary_status()["status"] == 1


@pytest.mark.parametrize("lat,dt,coll,res,masks,switches,kernel,launches", LBM2 + LBM2M)
def test_resident_path_against_the_oracle(lat, dt, coll, res, masks, switches, kernel, launches):
    """the same kernels on the engine's padded buffers: load (collide), advance (fused), store (stream)"""
    plan, f0, _ = _build(lat, dt, coll, res, masks, dict(switches, resident=1))
    assert plan.resident_enabled()[0]
    _assert_kernel(plan, kernel)
    want = _oracle_snapshots(lat, dt, coll, tuple(res), masks)
    outlet = masks is not None and masks[0] is not None
    f = dev(f0)
    for n in STEPS:
        plan.resident_load(f, TAU)
        plan.resident_advance(TAU, n - 1)
        assert plan.last_run_info() == expected_launches(launches, n - 1, outlet), (n, plan.last_run_info())
        out = plan.resident_store(torch.empty_like(f))
        torch.cuda.synchronize()
        assert_close(out.cpu().numpy(), want[n], dt, n, outlet)
    plan.resident_load(f, TAU)                                  # 3, look, 5 more from what the engine kept
    plan.resident_advance(TAU, 2)
    plan.resident_store(torch.empty_like(f))
    plan.resident_advance(TAU, 5)
    assert plan.last_run_info() == expected_launches(launches, 5, outlet)
    out = plan.resident_store(torch.empty_like(f))
    torch.cuda.synchronize()
    assert_close(out.cpu().numpy(), want[8], dt, 8, outlet)


def test_graph_replay_path_against_the_oracle():
    """set_graph_mode(1): the fused steps run as replays of a captured 32-step graph; 70 steps = collide, two
    chunks, five eager steps, stream; 66 more through lt_continue replay two chunks again"""
    lat, dt, res, masks = "D2Q9", "f64", [16, 24], ((0, 1), True, False)
    plan, f0, (entries, ncm, nsm) = _build(lat, dt, "bgk", res, masks, {"graph": 1, "many_step": 0})
    _assert_kernel(plan, "lbm_kernel")
    sim = oracle(lat, f0, "bgk", entries, ncm, nsm)
    a = dev(f0)
    result, fstar = plan.run(a, torch.empty_like(a), TAU, 70)
    torch.cuda.synchronize()
    assert plan.last_run_info() == expected_launches("one", 5, True)        # 64 of 69 fused steps in the graph
    sim.step(70)
    assert_close(result.cpu().numpy(), sim.f.numpy(), dt, 70, True)
    out, _ = plan.run(fstar, result, TAU, 66, from_fstar=True)
    torch.cuda.synchronize()
    assert plan.last_run_info() == expected_launches("one", 2, True)
    sim.step(66)
    assert_close(out.cpu().numpy(), sim.f.numpy(), dt, 136, True)


# --------------------------------------------------------------------------- lt_plan_update_boundary
def _ax0_case(side, seed=33):
    dtype = torch.float32
    res = [5, 8, 64]
    f0 = perturbed_state("D3Q19", res, dtype, seed)
    _, ncm, nsm, entries = _masked_case("D3Q19", res, dtype, (2, side), seed, inlet_face=True)
    return f0, ncm, nsm, entries


def _run(plan, f0, n):
    a = dev(f0)
    out, _ = plan.run(a, torch.empty_like(a), TAU, n)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_update_boundary_refuses_an_invalid_outlet_and_leaves_the_plan_unchanged():
    from lettuce_amd._native import NativeEngineError
    f0, ncm, nsm, entries = _ax0_case(1)
    plan = plan_for("D3Q19", torch.float32, "bgk", [5, 8, 64], entries)
    plan.set_masks(dev(ncm), dev(nsm))
    plan.set_two_step(1)
    before = _run(plan, f0, 5)
    name, status = plan.kernel_name(), plan.canary_status()
    assert status["status"] == 1 and plan.two_step_admitted() is None
    idx = [e["kind"] for e in entries].index("abb_outlet")
    for bad in ({"axis": 3, "side": 1}, {"axis": -1, "side": 1}, {"axis": 2, "side": 0}, {"axis": 2, "side": 2}):
        with pytest.raises(NativeEngineError, match="outlet"):
            plan.update_boundary(idx, dict(bad, kind="abb_outlet"))
        assert plan.kernel_name() == name and plan.two_step_admitted() is None
        assert plan.canary_status() == status
        np.testing.assert_array_equal(_run(plan, f0, 5), before)
        assert plan.last_run_info()["two_step_launches"] == 2
    # a 2-D plan has no axis 2
    f2, ncm2, nsm2, entries2 = _masked_case("D2Q9", [12, 64], torch.float64, (0, 1), 5)
    plan2 = plan_for("D2Q9", torch.float64, "bgk", [12, 64], entries2)
    plan2.set_masks(dev(ncm2), dev(nsm2))
    with pytest.raises(NativeEngineError, match="outlet"):
        plan2.update_boundary(2, {"kind": "abb_outlet", "axis": 2, "side": 1})


def test_flipping_an_ax0_outlet_decides_the_two_step_admission_again():
    """An outlet at z = last (AX = 0) flipped to z = 0 while the masks stay those of z = last: the masked two-step
    kernel's admission (no-streaming bits on the outlet column, equilibrium nodes on the face opposite) no longer
    holds, so lt_run must give what one-step launches give; with the masks of the new side it is admitted again,
    the first-use check runs again and lt_run matches the oracle.  And the order lt.Simulation updates a plan in
    (masks first, then the boundary) ends on the two-step kernel too."""
    fp, ncm_p, nsm_p, entries_p = _ax0_case(1)
    _, ncm_m, nsm_m, entries_m = _ax0_case(-1)
    idx = [e["kind"] for e in entries_p].index("abb_outlet")
    assert entries_m[idx] == {"kind": "abb_outlet", "axis": 2, "side": -1}
    plan = plan_for("D3Q19", torch.float32, "bgk", [5, 8, 64], entries_p)
    plan.set_masks(dev(ncm_p), dev(nsm_p))
    plan.set_two_step(1)
    assert _kernel(plan) == "lbm2m_kernel" and plan.canary_status()["status"] == 1
    plan.update_boundary(idx, entries_m[idx])                    # masks kept
    assert plan.canary_status()["status"] == 0
    assert plan.two_step_admitted() is not None and _kernel(plan) == "lbm_kernel"
    paired = _run(plan, fp, 8)
    assert plan.last_run_info()["two_step_launches"] == 0
    plan.set_two_step(0)
    np.testing.assert_array_equal(paired, _run(plan, fp, 8))
    plan.set_two_step(1)
    plan.set_masks(dev(ncm_m), dev(nsm_m))                       # the masks of the flipped outlet
    assert _kernel(plan) == "lbm2m_kernel"
    want = oracle("D3Q19", fp, "bgk", entries_m, ncm_m, nsm_m).step(8).numpy()
    got = _run(plan, fp, 8)
    assert plan.last_run_info()["two_step_launches"] == 3 and plan.canary_status()["status"] == 1
    assert_close(got, want, "f32", 8, True)
    plan.set_two_step(0)
    np.testing.assert_array_equal(_run(plan, fp, 8), got)

    # lt.Simulation's order: the new masks reach the plan before the new outlet does
    plan = plan_for("D3Q19", torch.float32, "bgk", [5, 8, 64], entries_p)
    plan.set_two_step(1)
    plan.set_masks(dev(ncm_m), dev(nsm_m))
    assert plan.two_step_admitted() is not None                  # masks of z = 0, outlet still at z = last
    plan.update_boundary(idx, entries_m[idx])
    assert plan.two_step_admitted() is None and _kernel(plan) == "lbm2m_kernel"
    got = _run(plan, fp, 8)
    assert plan.last_run_info()["two_step_launches"] == 3 and plan.canary_status()["status"] == 1
    assert_close(got, want, "f32", 8, True)


def test_geometry_update_resets_the_first_use_check():
    """moving an outlet (side, or present / absent) or switching an equilibrium boundary between its table and a
    per-node field runs the first-use check again; a new inlet value does not"""
    f0, ncm, nsm, entries = _masked_case("D3Q19", [6, 16, 64], torch.float32, (0, 1), 21)
    plan = plan_for("D3Q19", torch.float32, "bgk", [6, 16, 64], entries)
    plan.set_masks(dev(ncm), dev(nsm))
    plan.set_two_step(1)
    _run(plan, f0, 3)
    assert plan.canary_status()["status"] == 1
    eq = [e["kind"] for e in entries].index("equilibrium")
    plan.update_boundary(eq, {"kind": "equilibrium", "feq": [v * 1.01 for v in entries[eq]["feq"]]})
    assert plan.canary_status()["status"] == 1
    field = dev(torch.tensor(entries[eq]["feq"], dtype=torch.float32).reshape(-1, 1, 1, 1).expand(19, 6, 16, 64))
    plan.update_boundary(eq, {"kind": "equilibrium", "field": field})
    assert plan.canary_status()["status"] == 0
    _run(plan, f0, 3)
    assert plan.canary_status()["status"] == 1
    abb = [e["kind"] for e in entries].index("abb_outlet")
    plan.update_boundary(abb, {"kind": "abb_outlet", "axis": 0, "side": -1})
    assert plan.canary_status()["status"] == 0
    assert plan.two_step_admitted() is not None                  # the no-streaming bits are those of x = last
    plan.update_boundary(abb, {"kind": "abb_outlet", "axis": 0, "side": 1})
    assert plan.canary_status()["status"] == 0 and plan.two_step_admitted() is None
    _run(plan, f0, 3)
    assert plan.canary_status()["status"] == 1


# --------------------------------------------------------------------------- boundaries that change between batches
def _obstacle(lat, res, dt):
    import lettuce_amd as lt
    ctx = lt.Context("cuda:0", TORCH_DT[dt], use_native=True)
    flow = lt.Obstacle(ctx, res, 100, 0.1, domain_length_x=2, stencil=getattr(lt, lat)())
    grid = flow.grid
    near = (grid[0] - 0.7) ** 2 + (grid[1] - 0.5 * float(grid[1].max())) ** 2
    flow.mask = near < 0.2 ** 2
    flow.initialize()
    return flow, lt.Simulation(flow, lt.BGKCollision(flow.units.relaxation_parameter_lu), [])


def _mirror(sim, f):
    """the oracle of sim's present boundaries and masks, from f (float64): the inlet's feq recomputed from its
    velocity and pressure in float64"""
    import lettuce_amd as lt
    flow = sim.flow
    L = orc.LATTICES[type(flow.stencil).__name__]
    u = flow.units
    units = orc.Units(u.reynolds_number, u.mach_number, characteristic_length_lu=u.characteristic_length_lu,
                      characteristic_length_pu=u.characteristic_length_pu,
                      characteristic_velocity_pu=u.characteristic_velocity_pu,
                      characteristic_density_lu=u.characteristic_density_lu,
                      characteristic_density_pu=u.characteristic_density_pu)
    e, w = orc.lattice_tensors(L, torch.float64)
    o = _Oracle(L, f, "bgk", float(u.relaxation_parameter_lu))
    bnds = []
    for b in sim.boundaries[1:]:
        if isinstance(b, lt.AntiBounceBackOutlet):
            bnds.append(orc.OracleBoundary("abb_outlet", direction=list(b.direction)))
        elif isinstance(b, lt.BounceBackBoundary):
            bnds.append(orc.OracleBoundary("bounce_back"))
        else:
            feq = orc.quadratic_equilibrium(units.pressure_pu_to_density_lu(b.pressure.detach().cpu().double()),
                                            units.velocity_to_lu(b.velocity.detach().cpu().double()), e, w)
            bnds.append(_Feq(feq.reshape([L.q] + [1] * L.d) if feq.dim() == 1 else feq))
    o.boundaries = bnds
    o.no_collision_mask = sim.no_collision_mask.cpu()
    o.no_streaming_mask = sim.no_streaming_mask.cpu()
    return o


CHANGING = [("D2Q9", [24, 64], "f64", "dense"), ("D2Q9", [24, 64], "f64", "resident"),
            ("D2Q9", [24, 64], "f64", "many"), ("D2Q9", [24, 64], "f64", "two"),
            ("D3Q19", [16, 8, 64], "f32", "dense"), ("D3Q19", [16, 8, 64], "f32", "resident"),
            ("D3Q19", [16, 8, 64], "f32", "two")]
PATH_SWITCHES = {"dense": {"resident": 0, "many_step": 0, "two_step": 0},
                 "resident": {"resident": 1, "many_step": 0, "two_step": 0},
                 "many": {"resident": 0, "many_step": 1, "two_step": 0},
                 "two": {"resident": 0, "many_step": 0, "two_step": 1}}


@pytest.mark.parametrize("lat,res,dt,path", CHANGING, ids=[f"{t[0]}-{t[3]}" for t in CHANGING])
def test_boundaries_and_masks_changed_between_batches(lat, res, dt, path):
    """lt.Simulation on an Obstacle; between batches the inlet velocity is edited in place, replaced by a per-node
    field and back, the pressure changes, no_collision_mask is replaced and flow.f is edited in place.  The oracle
    takes the same changes at the same step."""
    import lettuce_amd as lt
    flow, sim = _obstacle(lat, res, dt)
    plan = sim._native.plan
    for key, value in PATH_SWITCHES[path].items():
        {"resident": plan.set_resident, "many_step": plan.set_many_step, "two_step": plan.set_two_step}[key](value)
    kernel = {"dense": "lbm_kernel", "resident": "lbm_kernel", "many": "lbm_many_kernel",
              "two": "lbm2d2m_kernel" if lat == "D2Q9" else "lbm2m_kernel"}[path]
    launches = {"dense": "single_step_launches", "resident": "single_step_launches", "many": "many_step_launches",
                "two": "two_step_launches"}[path]
    inlet = next(b for b in sim.boundaries[1:] if isinstance(b, lt.EquilibriumBoundaryPU))
    f = flow.f.detach().cpu().double()
    steps = 0

    def batch(k, look=True):
        nonlocal f, steps
        o = _mirror(sim, f)
        sim(k)
        o.step(k)
        f, steps = o.f, steps + k
        assert _kernel(plan) == kernel, plan.kernel_name()
        assert plan.last_run_info()[launches] > 0, plan.last_run_info()
        assert plan.resident_enabled()[0] == (path == "resident")
        if look:
            assert_close(flow.f.detach().cpu().numpy(), f.numpy(), dt, steps, True)

    batch(5)
    inlet.velocity.mul_(1.2)                                     # in place: a new _version
    batch(4, look=False)
    batch(5)
    vel = inlet.velocity.detach().clone()
    grid = flow.grid
    profile = (1 + 0.3 * torch.sin(torch.pi * grid[1] / float(grid[1].max()))).to(vel.device, vel.dtype)
    inlet.velocity = torch.stack([vel[a] * profile for a in range(flow.stencil.d)])   # a per-node field
    batch(5)
    inlet.velocity = vel                                         # and back to one velocity
    batch(4)
    inlet.pressure = flow.context.convert_to_tensor(0.02)
    batch(5)
    ncm = sim.no_collision_mask.clone()
    bb = [i for i, b in enumerate(sim.boundaries) if isinstance(b, lt.BounceBackBoundary)][0]
    block = [slice(res[0] // 2, res[0] // 2 + 2)] + [slice(2, 4)] * (len(res) - 1)
    ncm[tuple(block)] = bb
    sim.no_collision_mask = ncm
    batch(5)
    flow.f[:, 3:5] *= 1.01                                       # flow.f edited in place
    f[:, 3:5] *= 1.01
    batch(5)
    if path == "two":
        assert plan.canary_status()["status"] == 1
