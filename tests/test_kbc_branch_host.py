"""The conditions under which tests/test_gpu_kbc_branch.py may exclude or gate anything, checked without a GPU.  They
are conditions on the CPU path alone, not measurements of a kernel: both runs finite, E_ref a yardstick inside the
bounds of test_fp32_error_budget_host.py, the excluded set small, and enough nodes on either side of the threshold and
on 0 / 0 left among the compared ones."""
import numpy as np
import pytest
import torch

import asymmetric_states as st
import bgk_arithmetic
from oracle import lettuce_oracle as orc
from test_gpu_fp32_error_budget import weighted_error
from test_gpu_kbc_branch import GRID, MANY_GRID, SLAB_GRIDS, TAUS, cpu_collided

GRIDS = [("D2Q9", GRID["D2Q9"]), ("D2Q9", MANY_GRID)] + [("D3Q27", res) for res in SLAB_GRIDS]
assert GRID["D3Q27"] in SLAB_GRIDS
IDS = [f"{lat.lower()}-{'x'.join(map(str, res))}" for lat, res in GRIDS]


@pytest.mark.parametrize("tau", TAUS)
@pytest.mark.parametrize("lat,res", GRIDS, ids=IDS)
def test_the_cpu_path_is_a_yardstick_on_the_branch_state(lat, res, tau):
    ref = st.branch_reference(lat, res, tau)
    keep = ~ref["excluded"].numpy()
    for dt in ("f32", "f64"):
        own, want = cpu_collided(lat, res, dt, tau)
        assert np.isfinite(own).all() and np.isfinite(want).all()
    own, want = cpu_collided(lat, res, "f32", tau)
    per_q = weighted_error(lat, own[:, keep], want[:, keep])
    for w in sorted(set(orc.LATTICES[lat].w)):
        members = [q for q, wq in enumerate(orc.LATTICES[lat].w) if wq == w]
        assert per_q[members].max() > 0, f"no fp32 error in the weight class {w}"
    print(f"E_ref {per_q.max():.3e}")
    assert 1e-7 < per_q.max() < 1e-4


@pytest.mark.parametrize("tau", TAUS)
@pytest.mark.parametrize("lat,res", GRIDS, ids=IDS)
def test_excluded_nodes_and_census_of_the_branch_state(lat, res, tau):
    ref = st.branch_reference(lat, res, tau)
    excluded, zero = ref["excluded"], ref["zero"]
    nodes = excluded.numel()
    assert not (excluded & zero).any()                               # a node with sum_h == 0 is never excluded
    assert int(excluded.sum()) <= st.EXCLUDED_CAP * nodes
    compared = ~excluded
    s32, s64 = st.stabilised(ref["gamma32"]), st.stabilised(ref["gamma64"])
    negative = int((compared & ~zero & (ref["gamma64"] < st.THRESHOLD)).sum())
    positive = int((compared & ~zero & (ref["gamma64"] > st.THRESHOLD)).sum())
    print(f"excluded {int(excluded.sum())} of {nodes}; compared: gamma < 1e-15 on {negative}, > 1e-15 on {positive}, "
          f"sum_h == 0 on {int(zero.sum())}; gamma in {float(ref['gamma64'][~zero].min()):.3g} .. "
          f"{float(ref['gamma64'][~zero].max()):.3g}")
    assert negative >= 8 and positive >= 8 and int(zero.sum()) >= 4
    # the CPU path's fp32 and fp64 runs take the same branch on every compared node (on the nodes at rest both return
    # f: x = f - feq is exactly 0 in fp32 and below 1e-8 f in fp64, whatever gamma is made of it)
    assert not ((s32 != s64) & compared & ~zero).any()
    assert s32[zero].all()


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("lat,res", GRIDS, ids=IDS)
def test_the_nodes_at_rest_are_equilibria_bit_for_bit_in_both_arithmetics(lat, res, dt):
    """f == feq exactly in torch's arithmetic at the place the nodes have in the grid (sum_h == 0, gamma = NaN) and in
    the kernels' rho, u and feq restated in numpy (the BGK collision returns f itself): there collide_kbc divides 0 by
    0, whichever kernel runs it"""
    f = st.branch_case(lat, res, dt)
    gamma, sum_h = st.kbc_gamma(f, TAUS[0])
    at = st.patch_index(lat)[1:]
    assert (sum_h[at] == 0).all() and torch.isnan(gamma[at]).all()
    assert int((sum_h == 0).sum()) == st.PATCH_NODES
    own = bgk_arithmetic.collide(f.numpy(), lat, 0.7)
    assert (own[st.patch_index(lat)] == f.numpy()[st.patch_index(lat)]).all()
    # the rest of the fp64 state is the fp32 state
    other = st.branch_case(lat, res, "f32").double()
    mask = torch.ones(res, dtype=torch.bool)
    mask[at] = False
    assert torch.equal(f.double()[:, mask], other[:, mask])


@pytest.mark.parametrize("tau", TAUS)
@pytest.mark.parametrize("lat", list(GRID))
def test_a_kernel_without_the_first_stabiliser_line_is_far_beyond_the_gate(lat, tau):
    res = GRID[lat]
    L = orc.LATTICES[lat]
    ref = st.branch_reference(lat, res, tau)
    f = st.branch_case(lat, res, "f32").double()
    e, w = orc.lattice_tensors(L, torch.float64)
    feq = orc.quadratic_equilibrium(orc.density(f), orc.velocity(f, e), e, w)
    ds = orc._kbc_shear_part(f, e) - orc._kbc_shear_part(feq, e)
    raw = (f - 1. / (2 * tau) * (2 * ds + ref["gamma64"] * (f - feq - ds))).numpy()
    nodes = (st.stabilised(ref["gamma64"]) & ~ref["excluded"] & ~ref["zero"]).numpy()
    own, want = cpu_collided(lat, res, "f32", tau)
    e_ref = float(weighted_error(lat, own, want).max())
    per_node = (np.abs(raw - want) / np.asarray(L.w).reshape([-1] + [1] * L.d)).max(0)[nodes]
    print(f"{int(nodes.sum())} stabilised nodes; the unstabilised collision is {per_node.min():.2e} .. {per_node.max():.2e} "
          f"away, E_ref {e_ref:.2e}")
    assert per_node.max() > 100 * 4 * e_ref
