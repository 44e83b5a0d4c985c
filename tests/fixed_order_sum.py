"""Host emulation of the engine's fixed-order fp64 reduction (lettuce_amd/csrc/reduce.hpp), plain numpy: given the
terms of every item and the launch geometry it predicts the BITS of an observable, not a bound around it.

The order, as reduce.hpp documents it:
  thread     adds its terms one after the other, from +0.0
  wave       six steps v += v(lane + off), off = 32, 16, ..., 1; lane 0 holds the tree's sum
  workgroup  the four waves in wave order
  grid       one workgroup over the workgroups' partials: a scalar -- thread t adds the partials t, t + 256, ..., then
             the tree and the waves once more; three components -- one thread adds a component's partials in index order

Every add below is one numpy fp64 add (IEEE round-to-nearest, as the GPU's); nothing calls numpy's own ``sum``, whose
order is its own.  A slot without a term holds +0.0: no accumulator here is ever -0.0 (each starts at +0.0, and a sum is
-0.0 only if both operands are), so adding +0.0 changes no bit -- which is also why `acc -= v` may be written
``acc + (-v)``."""
import numpy as np

THREADS = 256                 # threads of a workgroup: four waves of 64 lanes
REDUCE_BLOCKS = 1024          # workgroups of the scalar observables (api.hip, kReduceBlocks)
FORCE_BLOCKS = 1024           # the most workgroups of the two force observables (LT_BOUNDARY_FORCE_BLOCKS, LT_LINK_FORCE_BLOCKS)
FORCE_SKEW = 61               # boundary force: slots a workgroup moves on from one pass to the next (kForceSkew)


def in_order(terms):
    """[..., k] -> [...]: the terms of the last axis added one after the other, from +0.0"""
    terms = np.asarray(terms, dtype=np.float64)
    acc = np.zeros(terms.shape[:-1], dtype=np.float64)
    for k in range(terms.shape[-1]):
        acc = acc + terms[..., k]
    return acc


def wave_tree(v):
    """[..., 64] -> [...]: the shuffle tree; a lane whose partner lies beyond the wave reads its own value"""
    v = np.array(v, dtype=np.float64)
    assert v.shape[-1] == 64
    for off in (32, 16, 8, 4, 2, 1):
        v = v + np.concatenate([v[..., off:], v[..., 64 - off:]], axis=-1)
    return v[..., 0]


def workgroup_sum(acc):
    """[..., 256] per-thread accumulators -> [...]: the tree of every wave, then the waves in wave order"""
    acc = np.asarray(acc, dtype=np.float64)
    waves = wave_tree(acc.reshape(acc.shape[:-1] + (THREADS // 64, 64)))
    total = waves[..., 0]
    for w in range(1, THREADS // 64):
        total = total + waves[..., w]
    return total


def finish_scalar(partials):
    """[blocks] -> scalar: finish_sum_kernel"""
    partials = np.asarray(partials, dtype=np.float64)
    padded = np.zeros((len(partials) + THREADS - 1) // THREADS * THREADS, dtype=np.float64)
    padded[:len(partials)] = partials
    return workgroup_sum(in_order(padded.reshape(-1, THREADS).T))


def finish_components(partials):
    """[c, blocks] -> [c]: finish_components_kernel, a component's partials in index order from +0.0"""
    return in_order(np.asarray(partials, dtype=np.float64))


def grid_stride(items, blocks):
    """Thread order of a grid-stride loop.  items [n, m]: the m terms of item i in the order the thread adds them.
    Returns [blocks, 256, passes * m]: workgroup b, thread t takes the items b 256 + t + k blocks 256, k = 0, 1, ..."""
    items = np.asarray(items, dtype=np.float64)
    n, m = items.shape
    per_pass = blocks * THREADS
    passes = max(1, (n + per_pass - 1) // per_pass)
    slots = np.zeros((passes * per_pass, m), dtype=np.float64)
    slots[:n] = items
    return slots.reshape(passes, blocks, THREADS, m).transpose(1, 2, 0, 3).reshape(blocks, THREADS, passes * m)


def rotated(items, blocks, skew=FORCE_SKEW):
    """Thread order of boundary_force_kernel: pass k covers the items [k P, (k + 1) P), P = blocks * 256, and workgroup b
    takes the 256 items of slot (b + skew k) mod blocks of it.  Same shapes as grid_stride."""
    items = np.asarray(items, dtype=np.float64)
    n, m = items.shape
    per_pass = blocks * THREADS
    passes = max(1, (n + per_pass - 1) // per_pass)
    slots = np.zeros((passes * per_pass, m), dtype=np.float64)
    slots[:n] = items
    slots = slots.reshape(passes, blocks, THREADS, m)
    by_block = np.empty_like(slots)
    for k in range(passes):
        by_block[k] = slots[k, (np.arange(blocks) + skew * k) % blocks]
    return by_block.transpose(1, 2, 0, 3).reshape(blocks, THREADS, passes * m)


def force_blocks(n):
    """workgroups of the first launch of a force observable over n nodes / links"""
    return min((n + THREADS - 1) // THREADS, FORCE_BLOCKS)


def scalar_observable(items, blocks=REDUCE_BLOCKS):
    """a scalar observable over items [n] (one term each) or [n, m], on the plan's fixed grid"""
    items = np.asarray(items, dtype=np.float64)
    items = items.reshape(len(items), -1)
    return finish_scalar(workgroup_sum(in_order(grid_stride(items, blocks))))


def boundary_force(items):
    """items [c, n nodes, m]: component c's terms of node i in q order (+0.0 where a link carries nothing)"""
    blocks = force_blocks(np.asarray(items).shape[1])
    return finish_components([workgroup_sum(in_order(rotated(component, blocks))) for component in items])


def link_force(items):
    """items [c, n links, 2]: component c's terms (out, back) of link i, signed (+0.0 where e_{q,c} = 0); n = 0 -> zeros"""
    items = np.asarray(items, dtype=np.float64)
    blocks = force_blocks(items.shape[1])
    if blocks == 0:
        return np.zeros(items.shape[0], dtype=np.float64)
    return finish_components([workgroup_sum(in_order(grid_stride(component, blocks))) for component in items])
