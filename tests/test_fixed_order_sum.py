"""The host emulation of the fixed-order reduction (fixed_order_sum.py) takes every item exactly once: on
integer-valued terms every order is exact, so under each launch geometry the GPU tests use the emulation must equal the
plain integer sum -- of random integers (an item dropped, or taken twice, moves the sum) and of ones (the count)."""
import numpy as np
import pytest

import fixed_order_sum as fos

# items of the geometries of the GPU tests: D2Q9 [5, 7] and [520, 510] nodes, D3Q19 [6, 5, 67] nodes, 5 and
# 200 * 200 * 8 links; and the edges of a pass: one workgroup exactly, one item into the second pass
SIZES = [35, 2010, 265200, 5, 320000, 256, 257, 262144, 262145]


def integers(n, m, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(-2 ** 20, 2 ** 20, size=(n, m)).astype(np.float64)


@pytest.mark.parametrize("n", SIZES)
def test_scalar_observable_takes_every_item_once(n):
    items = integers(n, 1, n)
    assert fos.scalar_observable(items[:, 0]) == items.sum(dtype=np.int64) == int(sum(items[:, 0].tolist()))
    assert fos.scalar_observable(np.ones(n)) == n


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("order", ["rotated", "grid_stride"])
def test_force_observables_take_every_term_once(n, order):
    observable = fos.boundary_force if order == "rotated" else fos.link_force
    m = 8 if order == "rotated" else 2
    items = np.stack([integers(n, m, 3 * n + c) for c in range(3)])
    got = observable(items)
    assert got.tolist() == [float(int(sum(component.ravel().tolist()))) for component in items]
    assert observable(np.ones((3, n, m))).tolist() == [float(n * m)] * 3


def test_the_rotation_moves_a_workgroup_61_slots_per_pass():
    """two passes over 1024 workgroups: item i of pass 1 lies in slot (i - P) // 256 and goes to workgroup slot - 61"""
    blocks, per_pass = 1024, 1024 * fos.THREADS
    ids = np.arange(265200, dtype=np.float64).reshape(-1, 1)
    by_thread = fos.rotated(ids, blocks)
    assert by_thread.shape == (blocks, fos.THREADS, 2)
    assert by_thread[965, 7].tolist() == [965 * 256 + 7, per_pass + 2 * 256 + 7]          # (965 + 61) mod 1024 = 2
    assert by_thread[1023, 0].tolist() == [1023 * 256, 0.0]                                # slot 60 of pass 1: past the end
    plain = fos.grid_stride(ids, blocks)
    assert plain[2, 7].tolist() == [2 * 256 + 7, per_pass + 2 * 256 + 7]


def test_the_order_shows_in_the_bits():
    """the emulation is not just a sum: on terms of mixed magnitude it differs from the exact sum as the tree does"""
    terms = np.array([1.0, 2.0 ** -53, 0.0, 2.0 ** -53] + [0.0] * 252)
    # thread 0 holds 1.0; lanes 1 and 3 meet first (off = 2: 2^-52 in lane 1), then lane 0 takes lane 1: 1 + 2^-52
    assert fos.scalar_observable(terms) == 1.0 + 2.0 ** -52
    # added one after the other, each 2^-53 is lost to the 1.0
    assert fos.in_order(terms) == 1.0
