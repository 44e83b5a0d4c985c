"""Admission and launcher, held to each other at the smallest grids where they can disagree.

api.hip admits a plan to the two-step and many-step launches and the launchers of unit.inc refuse what they cannot run;
both read csrc/launch_limits.hpp.  Were the admission looser than a launcher, lt_run would commit a plan to a launch that
returns "no kernel"; were it tighter, a plan would quietly lose its two-step launch.  So on exactly one tile of every
3-D unit the plan is admitted, the launch runs and lt_run takes it; one row or half a tile further it is not admitted,
the explicit launch is refused as unsupported (never a HIP error) and lt_run gives the bits of one-step launches.  The
2-D strips and the many-step limits likewise.  (Larger tiles, segment lengths, masks with outlets, resident buffers and
the reference's vectors: test_gpu_engine.py, test_gpu_bgk_bits_vs_reference.py, test_gpu_paths_vs_oracle.py.)"""
import numpy as np
import pytest
import torch

from conftest import TORCH_DT
from oracle import lettuce_oracle as orc
from test_gpu_engine import dev, plan_for, _random_state

pytestmark = pytest.mark.gpu

TAU = 0.7
# unit -> (tile width, rows without masks, rows with masks): the table of DESIGN.md section 4, "Launch limits"
TILE = {("D3Q15", "f32"): (64, 8, 8), ("D3Q15", "f64"): (32, 8, 8), ("D3Q19", "f32"): (64, 8, 8),
        ("D3Q19", "f64"): (32, 8, 0), ("D3Q27", "f32"): (64, 4, 4), ("D3Q27", "f64"): (32, 0, 0)}
WITH_KERNEL = [unit for unit, tile in TILE.items() if tile[1] > 0]
NO_LAUNCHES = {"single_step_launches": 0, "two_step_launches": 0, "many_step_launches": 0}


def _ids(units):
    return [f"{lat.lower()}-{dt}" for lat, dt in units]


def _state(lat, res, dt, seed=5):
    return dev(_random_state(orc.LATTICES[lat], list(res), TORCH_DT[dt], seed))


def _plan(lat, dt, res, two_step, block=False):
    plan = plan_for(lat, TORCH_DT[dt], "bgk", res, [{"kind": "bounce_back"}] if block else [])
    if block:                                   # one solid node in the middle
        ncm = torch.zeros(res, dtype=torch.uint8)
        ncm[tuple(n // 2 for n in res)] = 1
        plan.set_masks(dev(ncm), dev(torch.zeros([orc.LATTICES[lat].q] + list(res), dtype=torch.uint8)))
    plan.set_two_step(two_step)
    if lat == "D2Q9":
        plan.set_many_step(0)
    return plan


def _run(plan, f, n):
    out, _ = plan.run(f.clone(), torch.empty_like(f), TAU, n)
    torch.cuda.synchronize()
    return out.cpu().numpy(), plan.last_run_info()


def _two_single_steps(lat, dt, res, f, block=False):
    one = _plan(lat, dt, res, 0, block)
    a, b = torch.empty_like(f), torch.empty_like(f)
    one.stream_collide(f, a, TAU)
    one.stream_collide(a, b, TAU)
    return b.cpu().numpy()


def _assert_not_admitted(lat, dt, res, block=False):
    """no two-step launch: the admission says that the grid does not tile, the explicit launch is refused as
    unsupported, lt_run launches single steps and returns what a plan that never pairs its steps returns"""
    from lettuce_amd._native import NativeEngineError
    f = _state(lat, res, dt)
    plan = _plan(lat, dt, res, 1, block)
    why = plan.two_step_admitted()
    assert why is not None and "the grid does not tile" in why, why
    with pytest.raises(NativeEngineError) as err:
        plan.stream_collide_twice(f, torch.empty_like(f), TAU)
    assert err.value.code == 2, (err.value.code, str(err.value))           # LT_ERR_UNSUPPORTED
    assert plan.kernel_name().split("<")[0] == "lbm_kernel", plan.kernel_name()
    got, info = _run(plan, f, 3)
    assert info == dict(NO_LAUNCHES, single_step_launches=2), info
    want, _ = _run(_plan(lat, dt, res, 0, block), f, 3)
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("lat,dt", WITH_KERNEL, ids=_ids(WITH_KERNEL))
def test_exactly_one_tile_is_admitted_launched_and_taken_by_run(lat, dt):
    width, rows, _ = TILE[lat, dt]
    res = [2, rows, width]
    f = _state(lat, res, dt)
    plan = _plan(lat, dt, res, 1)
    assert plan.two_step_admitted() is None, plan.two_step_admitted()
    assert plan.kernel_name().startswith("lbm2_kernel<") and f", {width}, {rows}, " in plan.kernel_name(), plan.kernel_name()
    got = plan.stream_collide_twice(f, torch.full_like(f, float("nan")), TAU)
    np.testing.assert_array_equal(got.cpu().numpy(), _two_single_steps(lat, dt, res, f))
    got, info = _run(plan, f, 3)
    assert info == dict(NO_LAUNCHES, two_step_launches=1), info
    want, info = _run(_plan(lat, dt, res, 0), f, 3)
    assert info == dict(NO_LAUNCHES, single_step_launches=2), info
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("grown", ["a-row-more", "half-a-tile-more"])
@pytest.mark.parametrize("lat,dt", WITH_KERNEL, ids=_ids(WITH_KERNEL))
def test_a_grid_that_does_not_tile_is_refused_by_both(lat, dt, grown):
    width, rows, _ = TILE[lat, dt]
    _assert_not_admitted(lat, dt, [2, rows + 1, width] if grown == "a-row-more" else [2, rows, width + width // 2])


def test_units_without_a_kernel_are_refused_by_both():
    """D3Q27 fp64 has no two-step tile at all; D3Q19 fp64 has none with masks (8 rows need 168 944 B of LDS) -- while its
    periodic plan on the same grid has one"""
    _assert_not_admitted("D3Q27", "f64", [2, 8, 32])
    _assert_not_admitted("D3Q19", "f64", [3, 8, 32], block=True)
    assert _plan("D3Q19", "f64", [3, 8, 32], 1).two_step_admitted() is None


def test_masked_tile_of_every_unit_with_one():
    """the masked launch on one tile, three planes and a bounce-back node: admitted (first-use check included), equal to
    two masked single steps, taken by lt_run"""
    for (lat, dt), (width, _, rows) in TILE.items():
        if rows == 0:
            continue
        res = [3, rows, width]
        f = _state(lat, res, dt)
        plan = _plan(lat, dt, res, 1, block=True)
        assert plan.two_step_admitted() is None, (lat, dt, plan.two_step_admitted())
        assert plan.kernel_name().startswith("lbm2m_kernel<") and f", {width}, {rows}, " in plan.kernel_name(), plan.kernel_name()
        got = plan.stream_collide_twice(f, torch.full_like(f, float("nan")), TAU)
        np.testing.assert_array_equal(got.cpu().numpy(), _two_single_steps(lat, dt, res, f, block=True), err_msg=f"{lat} {dt}")
        assert _run(plan, f, 3)[1] == dict(NO_LAUNCHES, two_step_launches=1), (lat, dt)


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("extent,strip", [(64, 64), (128, 128), (192, 64), (96, 0)])
def test_2d_strip_is_the_widest_that_divides_the_contiguous_extent(extent, strip, dt):
    res = [5, extent]
    if not strip:                 # no strip divides the extent: no two-step kernel, and the explicit launch says so
        _assert_not_admitted("D2Q9", dt, res)
        return
    f = _state("D2Q9", res, dt)
    plan = _plan("D2Q9", dt, res, 1)
    assert plan.two_step_admitted() is None, plan.two_step_admitted()
    scalar = "float" if dt == "f32" else "double"
    assert plan.kernel_name() == f"lbm2d2_kernel<{scalar}, lt::d2q9, 1, {strip}>", plan.kernel_name()
    want, info = _run(_plan("D2Q9", dt, res, 0), f, 4)
    assert info == dict(NO_LAUNCHES, single_step_launches=3), info
    got, info = _run(plan, f, 4)
    assert info == dict(NO_LAUNCHES, two_step_launches=1, single_step_launches=1), info
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_many_step_limits(dt):
    """[8, 64]: 8 steps per launch, 9 refused with the range; with an anti-bounce-back outlet 7 and 8; [8, 60] is no
    multiple of the 8 x 8 tile: lt_run launches single steps, same bits"""
    from lettuce_amd._native import NativeEngineError
    res = [8, 64]
    f = _state("D2Q9", res, dt)
    one = _plan("D2Q9", dt, res, 0)
    want, _ = _run(one, f, 9)
    plan = plan_for("D2Q9", TORCH_DT[dt], "bgk", res)
    plan.set_many_step(1)
    assert plan.kernel_name().startswith("lbm_many_kernel<") and plan.kernel_name().endswith(", 1, 8, 8, 8>"), plan.kernel_name()
    got, info = _run(plan, f, 9)                             # 8 fused steps: one launch
    assert info == dict(NO_LAUNCHES, many_step_launches=1), info
    np.testing.assert_array_equal(got, want)
    with pytest.raises(NativeEngineError, match=r"n_steps = 9 \(1\.\.8 per launch for this plan\)") as err:
        plan.stream_collide_many(f, torch.empty_like(f), TAU, 9)
    assert err.value.code == 1, err.value.code               # LT_ERR_INVALID

    # one outlet (at the last row of axis 0, with the reference's no-streaming bits): one step fewer
    L = orc.LATTICES["D2Q9"]
    m, sm = orc.abb_masks(f.shape, orc.OracleBoundary("abb_outlet", direction=[1, 0]), L)
    ncm = torch.zeros(res, dtype=torch.uint8)
    ncm[m] = 1
    outlet = plan_for("D2Q9", TORCH_DT[dt], "bgk", res, [{"kind": "abb_outlet", "axis": 0, "side": 1}])
    outlet.set_masks(dev(ncm), dev(sm.to(torch.uint8)))
    outlet.set_many_step(1)
    a, b = f.clone(), torch.empty_like(f)
    for _ in range(7):
        outlet.stream_collide(a, b, TAU)
        a, b = b, a
    got = outlet.stream_collide_many(f, torch.full_like(f, float("nan")), TAU, 7)
    np.testing.assert_array_equal(got.cpu().numpy(), a.cpu().numpy())
    with pytest.raises(NativeEngineError, match=r"n_steps = 8 \(1\.\.7 per launch for this plan\)"):
        outlet.stream_collide_many(f, torch.empty_like(f), TAU, 8)
    _, info = _run(outlet, f, 9)                             # 8 fused steps: a launch of 7 and one of 1
    assert info == dict(NO_LAUNCHES, many_step_launches=2), info

    res = [8, 60]
    f = _state("D2Q9", res, dt)
    plan = plan_for("D2Q9", TORCH_DT[dt], "bgk", res)
    plan.set_many_step(1)
    assert plan.kernel_name().split("<")[0] == "lbm_kernel", plan.kernel_name()
    got, info = _run(plan, f, 9)
    assert info == dict(NO_LAUNCHES, single_step_launches=8), info
    np.testing.assert_array_equal(got, _run(_plan("D2Q9", dt, res, 0), f, 9)[0])
