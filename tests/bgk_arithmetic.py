"""The BGK step of the HIP kernels restated operation for operation in numpy (every + - * / rounds once, in the
array's dtype, in the order the kernel uses: csrc/kernels.hpp `moments`, `square_norm`, `feq_q`, `collide_bgk`), and
the one place where the reference's CPU path deviates from it.

The kernel sums rho over q as ATen's `cascade_sum` does in its main loop: the first 16 populations from zero, the rest
from zero, the two partial sums added.  ATen takes that loop only for whole blocks of four SIMD vectors of the
flattened node index (AVX2: 32 fp32 / 16 fp64 nodes, AVX-512: 64 / 32).  The nodes after the last whole block -- the
tail of a grid whose node count is no multiple of the block -- go through `row_sum`, which keeps four interleaved
partial sums p_k = sum_i f[4 i + k], adds the populations beyond the last multiple of four to p_0 and returns
((p_0 + p_1) + p_2) + p_3.  So on a ragged grid the reference's own rho depends on where a node lies and on the vector
width of the CPU that ran it; `tail_block` below is the block of the machine that made the fixtures (stored in them).
With tail_block = None every node is summed as the kernel sums it.
"""
import numpy as np

from oracle import lettuce_oracle as orc


def density_kernel_order(f):
    q, T = f.shape[0], f.dtype.type
    head, tail = np.zeros(f.shape[1:], T), np.zeros(f.shape[1:], T)
    for i in range(q):
        if i < 16:
            head = head + f[i]
        else:
            tail = tail + f[i]
    return tail + head if q > 16 else head


def density_row_sum_order(f):
    """ATen's row_sum (SumKernel.cpp): four interleaved partial sums"""
    q, T = f.shape[0], f.dtype.type
    p = [np.zeros(f.shape[1:], T) for _ in range(4)]
    for i in range(q // 4):
        for k in range(4):
            p[k] = p[k] + f[4 * i + k]
    for i in range(4 * (q // 4), q):
        p[0] = p[0] + f[i]
    return ((p[0] + p[1]) + p[2]) + p[3]


def tail_nodes(shape, tail_block):
    """boolean grid: the nodes after the last whole block of `tail_block` nodes of the flattened index"""
    n = int(np.prod(shape))
    flat = np.arange(n) >= (n // tail_block) * tail_block if tail_block else np.zeros(n, dtype=bool)
    return flat.reshape(shape)


def collide(f, lat, tau, tail_block=None):
    L = orc.LATTICES[lat]
    T = f.dtype.type
    e = np.array(L.e)
    grid = f.shape[1:]
    rho = density_kernel_order(f)
    if tail_block:
        rho = np.where(tail_nodes(grid, tail_block), density_row_sum_order(f), rho)
    zero = np.zeros(grid, T)

    def signed_sum(terms, signs):
        acc = zero
        for t, s in zip(terms, signs):
            if s > 0:
                acc = acc + t
            elif s < 0:
                acc = acc - t
        return acc
    u = [signed_sum(f, e[:, a]) / rho for a in range(L.d)]
    uxu = u[0] * u[0]
    for a in range(1, L.d):
        uxu = uxu + u[a] * u[a]
    d0, d1, tau_inv = T(2.0 * orc.CS2), T(orc.CS2), T(1.0 / tau)
    out = np.empty_like(f)
    for q in range(L.q):
        exu = signed_sum(u, e[q])
        a = (T(2) * exu - uxu) / d0
        b = exu / d1
        feq = T(L.w[q]) * (rho * (a + T(0.5) * (b * b) + T(1)))
        out[q] = f[q] - tau_inv * (f[q] - feq)
    return out


def stream(f, lat):
    L = orc.LATTICES[lat]
    out = f.copy()
    for q in range(1, L.q):
        out[q] = np.roll(f[q], tuple(L.e[q]), axis=tuple(range(L.d)))
    return out


def unstream(f, lat):
    """the post-collision populations a post-streaming field came from (periodic, no no-streaming bits)"""
    L = orc.LATTICES[lat]
    out = f.copy()
    for q in range(1, L.q):
        out[q] = np.roll(f[q], tuple(-c for c in L.e[q]), axis=tuple(range(L.d)))
    return out


def steps(f, lat, tau, n, tail_block=None, solid=None):
    """n steps collide -> bounce-back on `solid` -> stream"""
    L = orc.LATTICES[lat]
    for _ in range(n):
        collided = collide(f, lat, tau, tail_block)
        if solid is not None:
            collided = np.where(solid, f[list(L.opposite)], collided)
        f = stream(collided, lat)
    return f
