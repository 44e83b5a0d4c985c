"""Periodic BGK, bit for bit against the reference's CPU path on states WITHOUT symmetries.

The other bit-identity vectors (test_gpu_engine.py: BIT_IDENTICAL, TWO_STEP_GOLDEN, the cfg1 vectors) are Taylor-Green
and shear-layer flows: smooth, rho within a few 1e-3 of 1, one tau each, opposite populations nearly equal.  On those a
summation order exchanged between a population and its opposite cancels, dividends near 0 and quotients far from
+-1/3 do not occur, and no population is negative.  The vectors here (tests/golden/bgk_bits_*, oracle/gen_golden.py
bgk_bits) are random densities (moderate: 0.5 .. 1.5, wide: 1/20 .. 20), random velocities and +-5 % per population,
stepped by the reference at tau = 0.501 (populations go negative), 0.7 and 1.7 -- with 1 and with 8 threads, same bits.

Every comparison is np.testing.assert_array_equal; every case names the kernel and counts the launches, so a quiet
fall-back to one-step launches cannot pass.

What these vectors found: the reference's own rho is not summed in one order.  torch.sum over q
takes the cascade order the kernels reproduce only for whole blocks of four SIMD vectors of the flattened node index
(32 fp32 / 16 fp64 nodes); the nodes after the last whole block -- the tail of a grid whose node count is no multiple
of the block -- are summed in four interleaved partial sums, one ulp of rho apart on 5 % of such nodes.  The kernels
keep ONE order for every node.  So on the ragged grids ([7, 5], [6, 5, 7]: tails of 3 and 18 / 2 nodes) the engine is
held, bit for bit, to
  * the reference's vectors after one step at every node outside the tail, and
  * the kernels' arithmetic restated in numpy (tests/bgk_arithmetic.py) at every node, after 1 and 5 steps;
test_oracle_golden.py shows without a GPU that the same restatement with rho of the tail nodes in the interleaved order
IS the reference, bit for bit, on every vector here.  Where the node count is a multiple of 64 (the tile grids) and for
D1Q3 (three terms: both orders coincide) the vectors themselves are the target.
"""
import math

import numpy as np
import pytest
import torch

import bgk_arithmetic
from conftest import golden, unpack_nsm, TORCH_DT
from test_gpu_engine import dev, plan_for

pytestmark = pytest.mark.gpu

BITS_TAUS = {"moderate": (0.501, 0.7, 1.7), "wide": (0.7, 1.7)}
BITS = [(lat, dt) for lat in ("D1Q3", "D2Q9", "D3Q15", "D3Q19", "D3Q27") for dt in ("f32", "f64")]
TILES = [(lat, dt) for lat, dt in BITS if lat != "D1Q3" and (lat, dt) != ("D3Q27", "f64")]
BOUNCE_BACK = [(lat, dt) for lat in ("D2Q9", "D3Q19") for dt in ("f32", "f64")]
NO_LAUNCHES = {"single_step_launches": 0, "two_step_launches": 0, "many_step_launches": 0}


def _ids(cases):
    return [f"{lat.lower()}-{dt}" for lat, dt in cases]


def launches(**counts):
    return dict(NO_LAUNCHES, **counts)


def run(plan, f0, tau, n):
    a = dev(f0)
    out, _ = plan.run(a, torch.empty_like(a), tau, n)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def run_resident(plan, f0, tau, n):
    f = dev(f0)
    plan.resident_load(f, tau)
    plan.resident_advance(tau, n - 1)
    info = plan.last_run_info()
    out = plan.resident_store(torch.empty_like(f))
    torch.cuda.synchronize()
    return out.cpu().numpy(), info


def collide_then_stream(plan, f0, tau, n):
    """n whole steps through the operator entry points"""
    a = dev(f0)
    b = torch.empty_like(a)
    for _ in range(n):
        plan.collide(a, b, tau)
        plan.stream(b, a)
    torch.cuda.synchronize()
    return a.cpu().numpy()


# --------------------------------------------------------------------------- the one-step kernel, ragged grids
def expected_on_a_ragged_grid(g, lat, f0, tau, n, want, solid=None):
    """(the populations the kernels' one summation order gives after n steps, the nodes outside the reference's tail);
    with whole blocks only, or three terms, that is the reference's vector itself"""
    grid = f0.shape[1:]
    in_blocks = ~bgk_arithmetic.tail_nodes(grid, int(g["sum_block"]))
    if lat == "D1Q3" or in_blocks.all():
        return want, np.ones(grid, dtype=bool)
    return bgk_arithmetic.steps(f0, lat, tau, n, None, solid), in_blocks


def assert_bits_on_a_ragged_grid(got, g, lat, f0, tau, n, want, what, solid=None):
    restated, in_blocks = expected_on_a_ragged_grid(g, lat, f0, tau, n, want, solid)
    np.testing.assert_array_equal(got, restated, err_msg=f"{what}: the kernels' arithmetic")
    if n == 1:                  # one step: a node's post-collision populations depend on that node alone
        np.testing.assert_array_equal(bgk_arithmetic.unstream(got, lat)[:, in_blocks],
                                      bgk_arithmetic.unstream(want, lat)[:, in_blocks],
                                      err_msg=f"{what}: the reference outside its tail")
        assert in_blocks.sum() >= 0.9 * in_blocks.size


@pytest.mark.parametrize("lat,dt", BITS, ids=_ids(BITS))
def test_one_step_kernel_on_states_without_symmetries(lat, dt):
    g = golden(f"bgk_bits_{lat.lower()}_{dt}")
    res = [int(r) for r in g["resolution"]]
    plan = plan_for(lat, TORCH_DT[dt], "bgk", res, [])
    assert plan.kernel_name().startswith("lbm_kernel"), plan.kernel_name()
    for kind, taus in BITS_TAUS.items():
        f0 = g[f"f0_{kind}"]
        for tau in taus:
            for n in (1, 5):
                want = g[f"{kind}_tau{tau}_f{n}"]
                assert_bits_on_a_ragged_grid(run(plan, f0, tau, n), g, lat, f0, tau, n, want, f"{kind} tau {tau} n {n}")
                assert plan.last_run_info() == launches(single_step_launches=n - 1), (n, plan.last_run_info())
            assert_bits_on_a_ragged_grid(collide_then_stream(plan, f0, tau, 5), g, lat, f0, tau, 5,
                                         g[f"{kind}_tau{tau}_f5"], f"{kind} tau {tau} collide, stream")
            assert_bits_on_a_ragged_grid(collide_then_stream(plan, f0, tau, 1), g, lat, f0, tau, 1,
                                         g[f"{kind}_tau{tau}_f1"], f"{kind} tau {tau} collide, stream once")
    assert plan.kernel_name().startswith("lbm_kernel"), plan.kernel_name()


# --------------------------------------------------------------------------- every multi-step launcher, smallest tiles
def _two_step_plan(lat, dt, res, policy=None, resident=False):
    plan = plan_for(lat, TORCH_DT[dt], "bgk", res, [])
    plan.set_two_step(1)
    if lat == "D2Q9":
        plan.set_many_step(0)
    if policy is not None:
        plan.set_shift_policy(policy)
    if resident:
        plan.set_resident(1)
        assert plan.resident_enabled()[0]
    assert plan.two_step_admitted() is None, plan.two_step_admitted()
    return plan


@pytest.mark.parametrize("lat,dt", TILES, ids=_ids(TILES))
def test_every_launcher_on_the_smallest_tiles(lat, dt):
    """[2, 8, 64] (one 64 x 8 tile in fp32, two tiles in fp64 and for D3Q27: every tile its own neighbour) and
    D2Q9 [5, 64]: f4 = 3 fused steps (a pair and the odd remainder), f5 = 4 fused steps (two pairs)."""
    g = golden(f"bgk_bits_tiles_{lat.lower()}_{dt}")
    res = [int(r) for r in g["resolution"]]
    f0, tau = g["f0"], float(g["tau"])
    two_step_kernel = "lbm2d2_kernel" if lat == "D2Q9" else "lbm2_kernel"

    def pairs(n):
        return launches(two_step_launches=(n - 1) // 2, single_step_launches=(n - 1) % 2)

    # one step per launch
    one = plan_for(lat, TORCH_DT[dt], "bgk", res, [])
    one.set_two_step(0)
    one.set_many_step(0)
    assert one.kernel_name().split("<")[0] == "lbm_kernel", one.kernel_name()
    for n in (4, 5):
        np.testing.assert_array_equal(run(one, f0, tau, n), g[f"f{n}"], err_msg=f"one-step n {n}")
        assert one.last_run_info() == launches(single_step_launches=n - 1), (n, one.last_run_info())

    # two steps per launch on the caller's buffers
    two = _two_step_plan(lat, dt, res)
    name = two.kernel_name()
    assert name.split("<")[0] == two_step_kernel, name
    for n in (4, 5):
        np.testing.assert_array_equal(run(two, f0, tau, n), g[f"f{n}"], err_msg=f"two-step n {n}")
        assert two.last_run_info() == pairs(n), (n, two.last_run_info())

    # ... with the one-role schedule (D3Q19 fp32 has two schedules; elsewhere the policy names the same kernel)
    old = _two_step_plan(lat, dt, res, policy=6)
    if (lat, dt) == ("D3Q19", "f32"):
        assert name.endswith(", 1, 0, 1, 1>") and old.kernel_name().endswith(", 1, 0, 1>"), (name, old.kernel_name())
    else:
        assert old.kernel_name() == name, (name, old.kernel_name())
    for n in (4, 5):
        np.testing.assert_array_equal(run(old, f0, tau, n), g[f"f{n}"], err_msg=f"one-role two-step n {n}")
        assert old.last_run_info() == pairs(n), (n, old.last_run_info())

    # ... and on the engine's padded resident buffers, both schedules
    for policy in (None, 6):
        res_plan = _two_step_plan(lat, dt, res, policy=policy, resident=True)
        assert res_plan.kernel_name() == (name if policy is None else old.kernel_name())
        for n in (4, 5):
            got, info = run_resident(res_plan, f0, tau, n)
            np.testing.assert_array_equal(got, g[f"f{n}"], err_msg=f"resident two-step policy {policy} n {n}")
            assert info == pairs(n), (n, policy, info)


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_many_step_kernel_on_its_smallest_grid(dt):
    """lbm_many_kernel takes grids whose extents are both multiples of 8 ([5, 64] is not one): [8, 64], lt_run's
    automatic choice.  f4 / f5: one launch of 3 / 4 steps; f10: 9 fused steps, a launch of 8 and one of 1.  The
    two-step kernel and the one-step kernel on the same vectors."""
    g = golden(f"bgk_bits_many_d2q9_{dt}")
    res = [int(r) for r in g["resolution"]]
    f0, tau = g["f0"], float(g["tau"])
    many = plan_for("D2Q9", TORCH_DT[dt], "bgk", res, [])
    assert many.kernel_name().split("<")[0] == "lbm_many_kernel", many.kernel_name()
    two = _two_step_plan("D2Q9", dt, res)
    assert two.kernel_name().split("<")[0] == "lbm2d2_kernel", two.kernel_name()
    one = plan_for("D2Q9", TORCH_DT[dt], "bgk", res, [])
    one.set_many_step(0)
    one.set_two_step(0)
    assert one.kernel_name().split("<")[0] == "lbm_kernel", one.kernel_name()
    for n in (4, 5, 10):
        np.testing.assert_array_equal(run(many, f0, tau, n), g[f"f{n}"], err_msg=f"many-step n {n}")
        assert many.last_run_info() == launches(many_step_launches=math.ceil((n - 1) / 8)), (n, many.last_run_info())
        np.testing.assert_array_equal(run(two, f0, tau, n), g[f"f{n}"], err_msg=f"two-step n {n}")
        assert two.last_run_info() == launches(two_step_launches=(n - 1) // 2, single_step_launches=(n - 1) % 2)
        np.testing.assert_array_equal(run(one, f0, tau, n), g[f"f{n}"], err_msg=f"one-step n {n}")
        assert one.last_run_info() == launches(single_step_launches=n - 1)


# --------------------------------------------------------------------------- a bounce-back block
@pytest.mark.parametrize("lat,dt", BOUNCE_BACK, ids=_ids(BOUNCE_BACK))
def test_bounce_back_block_on_states_without_symmetries(lat, dt):
    """Bounce-back only copies populations, so the fluid nodes around a solid block keep the reference's bits too.
    The ragged grids ([7, 5], [6, 5, 7]) do not tile: lt_run has only the one-step kernel for them, also when it is
    asked to pair the steps."""
    g = golden(f"bgk_bits_bb_{lat.lower()}_{dt}")
    res = [int(r) for r in g["resolution"]]
    f0, tau = g["f0"], float(g["tau"])
    assert not unpack_nsm(g).any()
    for two_step in (0, 1):
        plan = plan_for(lat, TORCH_DT[dt], "bgk", res, [{"kind": "bounce_back"}])
        plan.set_masks(dev(g["no_collision_mask"]), dev(unpack_nsm(g)))
        plan.set_two_step(two_step)
        if two_step:
            assert "does not tile" in plan.two_step_admitted()
        assert plan.kernel_name().split("<")[0] == "lbm_kernel", plan.kernel_name()
        solid = g["block_mask"].astype(bool)
        for n in (1, 5):
            assert_bits_on_a_ragged_grid(run(plan, f0, tau, n), g, lat, f0, tau, n, g[f"f{n}"], f"n {n}", solid)
            assert plan.last_run_info() == launches(single_step_launches=n - 1), (n, plan.last_run_info())
        assert_bits_on_a_ragged_grid(collide_then_stream(plan, f0, tau, 5), g, lat, f0, tau, 5, g["f5"],
                                     "collide, stream", solid)
