"""States away from rho = 1 for every operator, and a state that reaches both stabiliser lines of KBC.

`asymmetric_state` is the generator of the BGK bit fixtures (oracle/gen_golden.py, `asymmetric_state`) restated with
the oracle's tables: the fixtures store their f0, and test_asymmetric_states_host.py holds this restatement to it bit
for bit.

`kbc_branch_state` spreads KBC's gamma over both signs.  With x = f - feq split into its shear part ds and the rest dh,

    gamma = 1 / beta - (2 - 1 / beta) <ds, dh> / <dh, dh>,        <a, b> = sum_q a_q b_q / feq_q.

On D3Q27 +-5 % noise per population never makes gamma negative: dh has 20 degrees of freedom against the 6 of ds, so
<dh, dh> swamps <ds, dh>.  Scaling dh by c < 1 at fixed ds leaves rho, u, feq and ds as they are and multiplies the
ratio by 1 / c, so `gamma < 1e-15 -> 2` is taken on a good share of the nodes (the counts: DESIGN.md section 2).

`rest_patch` gives nodes at rest, f_q = w_q rho0, with rho0 chosen so that sum_q f_q == rho0 exactly both in torch's
summation order and in the kernels' (bgk_arithmetic.py): there f == feq bit for bit, ds = dh = 0, both sums are 0 and
gamma = 0 / 0 -- the second stabiliser line, `gamma != gamma -> 2`.

`branch_case` puts the two together (the fp64 state is the fp32 state promoted, except for the rest nodes, which are
exact in each precision) and computes the one set of nodes a comparison with the CPU path may leave out: those whose
gamma lies within the CPU path's own fp32 uncertainty of the threshold, on either side of which a correct kernel may
land.
"""
import functools

import numpy as np
import torch

import bgk_arithmetic
from oracle import lettuce_oracle as orc

THRESHOLD = 1e-15                    # kbc_collision.py: gamma[gamma < 1e-15] = 2
MARGIN = 4.0                         # the project's factor on the reference's own fp32 error (FACTOR of the budget tests)
EXCLUDED_CAP = 0.05                  # at most this share of the nodes may be left out
BRANCH_EPS, BRANCH_SEED = 0.3, 5
PATCH_NODES = 8


def _rho_u(lat, res, kind, g):
    L = orc.LATTICES[lat]
    r = torch.rand(res, generator=g, dtype=torch.float64)
    rho = 1 + (r - 0.5) if kind == "moderate" else 20.0 ** (2 * r - 1)
    u = 0.1 * (torch.rand([L.d] + list(res), generator=g, dtype=torch.float64) - 0.5)
    return rho, u


def asymmetric_state(lat, res, kind, seed):
    """float64 populations: equilibria of a random density (moderate: 1 + (rand - 0.5); wide: 20^(2 rand - 1)) and
    a random velocity (0.1 (rand - 0.5) per component), times 1 +- 5 % per population"""
    L = orc.LATTICES[lat]
    g = torch.Generator().manual_seed(seed)
    rho, u = _rho_u(lat, res, kind, g)
    noise = 1 + 0.05 * (2 * torch.rand([L.q] + list(res), generator=g, dtype=torch.float64) - 1)
    e, _ = orc.lattice_tensors(L, torch.float64)
    w = torch.tensor(L.w, dtype=torch.float64).reshape([-1] + [1] * L.d)
    eu = torch.tensordot(e, u, dims=1)
    uu = (u * u).sum(0)
    return w * rho * (1 + 3 * eu + 4.5 * eu * eu - 1.5 * uu) * noise


def kbc_branch_state(lat, res, seed=BRANCH_SEED, eps=BRANCH_EPS):
    """float64 populations on a moderate density whose KBC gamma has both signs: feq + ds + c dh with c = eps^(2 rand)
    per node, ds and dh the shear part and the rest of +-5 % feq noise without its mass and momentum"""
    L = orc.LATTICES[lat]
    g = torch.Generator().manual_seed(seed)
    rho, u = _rho_u(lat, res, "moderate", g)
    e, w = orc.lattice_tensors(L, torch.float64)
    feq = orc.quadratic_equilibrium(rho, u, e, w)
    x = feq * 0.05 * (2 * torch.rand([L.q] + list(res), generator=g, dtype=torch.float64) - 1)
    wq = w.reshape([-1] + [1] * L.d)
    m0, m1 = x.sum(0), torch.einsum("qa,q...->a...", e, x)
    x = x - wq * m0 - 3 * wq * torch.einsum("qa,a...->q...", e, m1)
    ds = orc._kbc_shear_part(feq + x, e) - orc._kbc_shear_part(feq, e)
    dh = x - ds
    c = eps ** (2 * torch.rand(res, generator=g, dtype=torch.float64))
    return feq + ds + c * dh


def kbc_gamma(f, tau):
    """(gamma before the stabiliser, sum_h) per node, with the oracle's operators in f's dtype"""
    L = next(v for v in orc.LATTICES.values() if v.q == f.shape[0] and v.d == f.dim() - 1)
    e, w = orc.lattice_tensors(L, f.dtype)
    beta = 1. / (2 * tau)
    feq = orc.quadratic_equilibrium(orc.density(f), orc.velocity(f, e), e, w)
    ds = orc._kbc_shear_part(f, e) - orc._kbc_shear_part(feq, e)
    dh = f - feq - ds
    sum_s, sum_h = orc.density(ds * dh / feq)[0], orc.density(dh * dh / feq)[0]
    return 1. / beta - (2 - 1. / beta) * sum_s / sum_h, sum_h


def stabilised(gamma):
    """the nodes on which either stabiliser line sets gamma = 2"""
    return (gamma < THRESHOLD) | torch.isnan(gamma)


@functools.lru_cache(maxsize=None)
def rest_patch(lat, dt, count=PATCH_NODES, seed=77):
    """[q, count] populations at rest on which f == feq bit for bit in torch's arithmetic and in the kernels': the
    first `count` of 4096 random densities in 0.5 .. 1.5 that the sum over q reproduces exactly in both orders"""
    L = orc.LATTICES[lat]
    dtype = {"f32": torch.float32, "f64": torch.float64}[dt]
    g = torch.Generator().manual_seed(seed)
    rho0 = (0.5 + torch.rand(4096, generator=g, dtype=torch.float64)).to(dtype)
    _, w = orc.lattice_tensors(L, dtype)
    f = w[:, None] * rho0[None, :]
    shaped = f.reshape([L.q, -1] + [1] * (L.d - 1))
    own = torch.tensor(bgk_arithmetic.collide(shaped.numpy(), lat, 0.7)).reshape(L.q, -1)
    _, sum_h = kbc_gamma(shaped, 0.7)
    # torch sums the nodes after the last whole vector block in another order (bgk_arithmetic.py): exact there too
    rows = torch.tensor(bgk_arithmetic.density_row_sum_order(f.numpy()))
    keep = (own == f).all(0) & (sum_h.reshape(-1) == 0) & (rows == rho0)
    chosen = torch.nonzero(keep).flatten()[:count]
    assert len(chosen) == count, f"{lat} {dt}: only {len(chosen)} of 4096 rest nodes are exact"
    return f[:, chosen].contiguous()


def patch_index(lat, count=PATCH_NODES):
    """where the rest nodes go: `count` nodes of the row [1, (1,) 1 : 1 + count] -- clear of the solid block and of the
    faces the masked cases occupy"""
    d = orc.LATTICES[lat].d
    return tuple([slice(None)] + [1] * (d - 1) + [slice(1, 1 + count)])


@functools.lru_cache(maxsize=None)
def branch_case(lat, res, dt, count=PATCH_NODES):
    """the branch state of `lat` on `res` (a tuple) in dtype dt: the fp32 state, promoted for f64, with the rest nodes
    of that precision written over the nodes of patch_index"""
    assert res[-1] >= count + 2
    f = kbc_branch_state(lat, list(res)).float()
    if dt == "f64":
        f = f.double()
    f[patch_index(lat, count)] = rest_patch(lat, dt, count)
    return f


@functools.lru_cache(maxsize=None)
def branch_reference(lat, res, tau, count=PATCH_NODES):
    """What the GPU tests of the branch state stand on, from the fp32 state alone (so one set serves both dtypes):
    gamma of the CPU path in fp32 and in fp64, the nodes with sum_h == 0 in fp32, and the excluded nodes
    |gamma_64| <= MARGIN |gamma_32 - gamma_64| (never one with sum_h == 0: the comparison with NaN is false)"""
    f32 = branch_case(lat, res, "f32", count)
    g32, h32 = kbc_gamma(f32, tau)
    g64, _ = kbc_gamma(f32.double(), tau)
    zero = h32 == 0
    excluded = (g64.abs() <= MARGIN * (g32.double() - g64).abs()) & ~zero
    return {"gamma32": g32, "gamma64": g64, "zero": zero, "excluded": excluded}
