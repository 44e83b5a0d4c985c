"""Both stabiliser lines of KBC -- `gamma < 1e-15 -> 2` and `gamma != gamma -> 2` -- in every KBC kernel, D2Q9 and D3Q27,
fp32 and fp64, on the branch state of asymmetric_states.py: gamma in about -80 .. 120, negative on 8 to 133 nodes of a
case, and eight nodes at rest on which both entropic sums are exactly 0 in the kernels' arithmetic.

Per kernel, on the nodes outside the excluded set of asymmetric_states.branch_reference (conditions and counts:
test_kbc_branch_host.py and DESIGN.md section 2; no node is excluded today):
  fp64  |gpu - cpu_fp64| <= ATOL["f64"] max(1, max|f|)                                  (ATOL of test_gpu_engine.py)
  fp32  E_gpu <= 4 E_ref, E = max |. - cpu_fp64| / w_q over the same nodes              (test_gpu_fp32_error_budget.py)
on every node the result is finite, and every kernel returns the bits of the collide-only kernel on ALL nodes: one
arithmetic, one branch (collide_kbc is compiled without contraction).  The fused kernels are fed the state streamed
backwards, so that what they collide is the constructed state.  One collision only: a node on the other side of the
threshold would spread.  Without either line the D3Q27 cases fail: a negative gamma kept moves a population by
beta |gamma - 2| |dh|, three orders of magnitude beyond either gate, and 0 / 0 is not finite.
"""
import functools

import numpy as np
import pytest
import torch

import asymmetric_states as st
import bgk_arithmetic
from conftest import TORCH_DT
from oracle import lettuce_oracle as orc
from test_gpu_engine import ATOL, dev
from test_gpu_fp32_error_budget import FACTOR, weighted_error
from test_gpu_paths_vs_oracle import _Oracle, _oracle_boundary, expected_launches

pytestmark = pytest.mark.gpu

TAUS = (0.51, 1.7)
GRID = {"D2Q9": (16, 24), "D3Q27": (6, 8, 10)}
MANY_GRID = (8, 64)                                  # the smallest grid lbm_many_kernel takes
SLAB_GRIDS = ((6, 8, 10), (8, 6, 10))                # x = 6 and x = 8: rows that are no multiple / a multiple of 4 nodes
KERNELS = {"D2Q9": ("fused", "run", "masked-collide", "masked-fused", "many"),
           "D3Q27": ("fused", "run", "masked-collide", "masked-fused", "slab-collide", "slab-fused")}
CASES = [pytest.param(lat, dt, kernel, id=f"{lat.lower()}-{dt}-{kernel}")
         for lat in KERNELS for dt in ("f32", "f64") for kernel in ("collide",) + KERNELS[lat]]


def grids_of(lat, kernel):
    if kernel == "many":
        return (MANY_GRID,)
    return SLAB_GRIDS if kernel.startswith("slab") else (GRID[lat],)


# --------------------------------------------------------------------------- the CPU path
@functools.lru_cache(maxsize=None)
def cpu_collided(lat, res, dt, tau):
    """(cpu in the state's dtype, cpu in fp64 from the same state), float64 arrays: one KBC collision of the oracle"""
    L = orc.LATTICES[lat]
    f = st.branch_case(lat, res, dt)
    out = []
    for dtype in (f.dtype, torch.float64):
        e, w = orc.lattice_tensors(L, dtype)
        out.append(orc.kbc(f.to(dtype), tau, e, w).double().numpy())
    return tuple(out)


def masks(lat, res, dtype):
    """a bounce-back block in the middle and an equilibrium face at x = last (one feq table), no outlet: the plan of
    lbm_kernel_occ4 on D3Q27 fp32"""
    L = orc.LATTICES[lat]
    ncm = torch.zeros(list(res), dtype=torch.uint8)
    ncm[tuple(slice(n // 2 - 1, n // 2 + 1) for n in res)] = 1
    ncm[-1] = 2
    nsm = torch.zeros([L.q] + list(res), dtype=torch.uint8)
    e, w = orc.lattice_tensors(L, dtype)
    feq = orc.quadratic_equilibrium(torch.tensor(1.1, dtype=dtype), torch.tensor([0.03, -0.02, 0.01][:L.d], dtype=dtype), e, w)
    return ncm, nsm, [{"kind": "bounce_back"}, {"kind": "equilibrium", "feq": feq.double().tolist()}]


def assert_within_the_gates(got, lat, res, dt, tau, nodes, what):
    """`got`: post-collision populations [q, *res]; `nodes`: the boolean grid of the nodes that collided"""
    ref = st.branch_reference(lat, res, tau)
    own, want = cpu_collided(lat, res, dt, tau)
    assert np.isfinite(got).all(), f"{what}: not finite on {int((~np.isfinite(got)).any(0).sum())} nodes"
    where = nodes & ~ref["excluded"].numpy()
    assert (where & ref["zero"].numpy()).sum() >= 4 and where.sum() >= 0.95 * nodes.sum()
    if dt == "f64":
        tol = ATOL["f64"] * max(1.0, float(np.abs(want).max()))
        diff = float(np.abs(got - want)[:, where].max())
        print(f"{what} tau {tau}: max |gpu - cpu| {diff:.3e} (bound {tol:.1e}) on {int(where.sum())} nodes")
        assert diff <= tol
    else:
        e_ref = float(weighted_error(lat, own[:, where], want[:, where]).max())
        e_gpu = float(weighted_error(lat, got[:, where], want[:, where]).max())
        print(f"{what} tau {tau}: E_ref {e_ref:.3e}  E_gpu {e_gpu:.3e}  ratio {e_gpu / e_ref:.2f} on {int(where.sum())} nodes")
        assert 1e-7 < e_ref < 1e-4 and e_gpu <= FACTOR * e_ref, (e_ref, e_gpu, e_gpu / e_ref)


# --------------------------------------------------------------------------- the kernels
def _name(plan):
    return plan.kernel_name().split("<")[0]


def collided_by(kernel, lat, res, dt, tau):
    """(post-collision populations [q, *res] as the kernel left them (numpy), the boolean grid of collided nodes,
    the boundary nodes' expected values or None)"""
    from lettuce_amd._native import LAYOUT_SLAB, Plan
    dtype = TORCH_DT[dt]
    f0 = st.branch_case(lat, res, dt)
    before = torch.tensor(bgk_arithmetic.unstream(f0.numpy(), lat))          # streams onto f0
    everywhere = np.ones(res, dtype=bool)
    if kernel in ("collide", "fused", "run", "many"):
        plan = Plan(lat, dtype, "kbc", list(res), [])
        plan.set_many_step(1 if kernel == "many" else 0)
        if kernel == "collide":
            out = plan.collide(dev(f0), torch.empty_like(dev(f0)), tau)
        elif kernel == "fused":
            out = plan.stream_collide(dev(before), torch.empty_like(dev(before)), tau)
        elif kernel == "many":
            assert _name(plan) == "lbm_many_kernel", plan.kernel_name()
            out = torch.full_like(dev(before), float("nan"))
            plan.stream_collide_many(dev(before), out, tau, 1)
        else:
            a = dev(f0)
            streamed, fstar = plan.run(a, torch.empty_like(a), tau, 1)
            torch.cuda.synchronize()
            assert plan.last_run_info() == expected_launches("one", 0, False), plan.last_run_info()
            assert torch.equal(plan.stream(fstar.clone(), torch.empty_like(fstar)), streamed)
            out = torch.tensor(bgk_arithmetic.unstream(streamed.cpu().numpy(), lat))
        if kernel != "many":
            assert _name(plan) == "lbm_kernel", plan.kernel_name()
        torch.cuda.synchronize()
        return out.cpu().numpy(), everywhere, None
    if kernel.startswith("masked"):
        ncm, nsm, entries = masks(lat, res, dtype)
        plan = Plan(lat, dtype, "kbc", list(res), entries)
        plan.set_masks(dev(ncm), dev(nsm))
        plan.set_many_step(0)
        assert _name(plan) == ("lbm_kernel_occ4" if (lat, dt) == ("D3Q27", "f32") else "lbm_kernel"), plan.kernel_name()
        src = dev(f0 if kernel == "masked-collide" else before)
        out = (plan.collide if kernel == "masked-collide" else plan.stream_collide)(src, torch.empty_like(src), tau)
        torch.cuda.synchronize()
        sim = _Oracle(orc.LATTICES[lat], f0.double().clone(), "kbc", tau)
        sim.boundaries = [_oracle_boundary(orc.LATTICES[lat], e, dtype) for e in entries]
        sim.no_collision_mask, sim.no_streaming_mask = ncm, nsm
        return out.cpu().numpy(), (ncm == 0).numpy(), sim.collide().numpy()
    plan = Plan(lat, dtype, "kbc", list(res), [], layout=LAYOUT_SLAB)       # x contiguous: [q, z, y, x]
    assert _name(plan) == "lbm_kernel" and f"lt::{lat.lower()}, 1, 2," in plan.kernel_name(), plan.kernel_name()
    src = dev((f0 if kernel == "slab-collide" else before).permute(0, 3, 2, 1))
    assert list(src.shape) == plan.f_shape
    out = (plan.collide if kernel == "slab-collide" else plan.stream_collide)(src, torch.empty_like(src), tau)
    torch.cuda.synchronize()
    return out.permute(0, 3, 2, 1).contiguous().cpu().numpy(), everywhere, None


@functools.lru_cache(maxsize=None)
def collide_only(lat, res, dt, tau):
    return collided_by("collide", lat, res, dt, tau)[0]


@pytest.mark.parametrize("tau", TAUS)
@pytest.mark.parametrize("lat,dt,kernel", CASES)
def test_kbc_kernel_on_the_branch_state(lat, dt, kernel, tau):
    for res in grids_of(lat, kernel):
        what = f"{lat} {dt} {kernel} {list(res)}"
        got, collided, boundary = collided_by(kernel, lat, res, dt, tau)
        assert_within_the_gates(got, lat, res, dt, tau, collided, what)
        # one arithmetic, one branch: the collide-only kernel's bits on every node that collided, none excluded
        same = (got == collide_only(lat, res, dt, tau)).all(0)
        assert same[collided].all(), f"{what}: {int((~same & collided).sum())} nodes differ from the collide-only kernel"
        if boundary is not None:
            tol = ATOL[dt] * max(1.0, float(np.abs(boundary).max()))
            np.testing.assert_allclose(got[:, ~collided], boundary[:, ~collided], rtol=0, atol=tol)
