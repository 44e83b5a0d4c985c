"""The two-step sweep with separate producer and consumer waves (lbm2_kernel, SCHED = 1; csrc/twostep_roles.hpp)
against the one-step kernel and against the one-role schedule of the same instantiation (shift policy 6), bit for
bit: every segment length 1 .. 9 and 128 (short last segments included), odd and even step counts, tiles that wrap
in both tiled axes ([n, 8, 64]: one 64 x 8 tile that is its own neighbour; [n, 24, 192]: 3 x 3 tiles), caller's dense
buffers and the engine's padded resident ones.  The launch counts are asserted, so a fall-back to single steps
cannot pass."""
import pytest
import torch

from conftest import TORCH_DT

pytestmark = pytest.mark.gpu

# the dtypes whose D3Q19 BGK sweep is instantiated with separate roles (csrc/dispatch.hpp, the last column of the units)
ROLE_DTYPES = ["f32"]
TAU = 0.6


def plans_for(dt, res, seg):
    from lettuce_amd._native import Plan
    new, old, one = (Plan("D3Q19", TORCH_DT[dt], "bgk", res, []) for _ in range(3))
    new.set_two_step(1, seg)
    old.set_two_step(1, seg)
    old.set_shift_policy(6)
    one.set_two_step(0)
    return new, old, one


def populations(plan, dt):
    torch.manual_seed(11)
    w = torch.rand(19, 1, 1, 1, device="cuda", dtype=TORCH_DT[dt]) * 0.05 + 0.02
    return (w * (1 + 0.1 * torch.rand(plan.f_shape, device="cuda", dtype=TORCH_DT[dt]))).contiguous()


@pytest.mark.parametrize("dt", ROLE_DTYPES)
def test_the_new_schedule_is_what_the_plan_reports_and_policy_6_the_old_one(dt):
    new, old, _ = plans_for(dt, [16, 8, 64], 0)
    name_new, name_old = new.kernel_name(), old.kernel_name()
    assert name_new.startswith("lbm2_kernel<") and name_new.endswith(", 1, 0, 1, 1>"), name_new
    assert name_old.startswith("lbm2_kernel<") and name_old.endswith(", 1, 0, 1>"), name_old
    assert name_new.startswith(name_old[:-1])              # the nine parameters of the old name, one appended


SEGS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 128]
GRIDS = [[6, 8, 64], [48, 8, 64], [256, 8, 64], [6, 24, 192], [48, 24, 192], [256, 24, 192]]


@pytest.mark.parametrize("buffers", ["dense", "resident"])
@pytest.mark.parametrize("seg", SEGS)
@pytest.mark.parametrize("res", GRIDS, ids=lambda r: "x".join(map(str, r)))
@pytest.mark.parametrize("dt", ROLE_DTYPES)
def test_role_waves_equal_single_steps_and_the_one_role_schedule(dt, res, seg, buffers):
    """lt_run and the resident path on a whole periodic grid.  A whole-grid plan takes only segment lengths that
    divide the sweep axis (lt_plan_set_two_step refuses the others, asserted here -- no launch of either schedule
    exists for them); the slab test below runs EVERY segment length on the same grids, short last segments included."""
    from lettuce_amd._native import NativeEngineError, Plan
    if res[0] % seg:
        with pytest.raises(NativeEngineError, match="does not divide"):
            Plan("D3Q19", TORCH_DT[dt], "bgk", res, []).set_two_step(1, seg)
        return
    new, old, one = plans_for(dt, res, seg)
    f0 = populations(new, dt)
    # n steps = one collide, n - 1 fused steps, one stream -> n = 5 has an even number of fused steps (two launches
    # of the two-step kernel), n = 4 an odd one (one launch and a single step)
    for n in (5, 4):
        got = {}
        for key, plan in (("new", new), ("old", old), ("one", one)):
            fused = n - 1
            if buffers == "dense":
                out, _ = plan.run(f0.clone(), torch.empty_like(f0), TAU, n)
            else:
                plan.set_resident(1, -1)
                assert plan.resident_enabled()[0]
                plan.resident_load(f0, TAU)
                plan.resident_advance(TAU, fused)
                out = plan.resident_store(torch.empty_like(f0))
            torch.cuda.synchronize()
            info = plan.last_run_info()
            if key == "one":
                assert info["two_step_launches"] == 0 and info["single_step_launches"] == fused, (key, info)
            else:
                assert info["two_step_launches"] == fused // 2 and info["single_step_launches"] == fused % 2, (key, info)
            got[key] = out
        assert torch.isfinite(got["one"]).all()
        assert torch.equal(got["new"], got["one"]), (n, float((got["new"] - got["one"]).abs().max()))
        assert torch.equal(got["new"], got["old"]), (n, float((got["new"] - got["old"]).abs().max()))


@pytest.mark.parametrize("seg", SEGS)
@pytest.mark.parametrize("res", GRIDS, ids=lambda r: "x".join(map(str, r)))
@pytest.mark.parametrize("dt", ROLE_DTYPES)
def test_role_waves_on_a_slab_with_every_segment_length(dt, res, seg):
    """the same grids as a slab with ghost planes (slab layout, the sweep of the multi-GPU driver), where any segment
    length is taken and the last segment may be short: the launch over all owned planes against two single-step
    launches and against the one-role schedule"""
    from lettuce_amd._native import Plan, LAYOUT_SLAB
    n2, n1, n0 = res
    new, old = (Plan("D3Q19", TORCH_DT[dt], "bgk", [n0, n1, n2], [], layout=LAYOUT_SLAB, ghost_planes=2) for _ in range(2))
    new.set_two_step(1, seg)
    old.set_two_step(1, seg)
    old.set_shift_policy(6)
    assert new.kernel_name().endswith(", 1, 0, 1, 1>") and old.kernel_name().endswith(", 1, 0, 1>")
    f0 = populations(new, dt)
    m = f0.shape[1]
    assert m == n2 + 4
    a, b, c, d = (torch.zeros_like(f0) for _ in range(4))
    new.stream_collide_planes(f0, a, TAU, 1, m - 1)
    new.stream_collide_planes(a, b, TAU, 2, m - 2)
    new.stream_collide_twice_planes(f0, c, TAU, 2, m - 2)
    old.stream_collide_twice_planes(f0, d, TAU, 2, m - 2)
    torch.cuda.synchronize()
    assert torch.isfinite(b[:, 2:m - 2]).all()
    assert torch.equal(b[:, 2:m - 2], c[:, 2:m - 2])
    assert torch.equal(c, d)


@pytest.mark.parametrize("seg", [1, 2, 5, 10])
@pytest.mark.parametrize("dt", ROLE_DTYPES)
def test_one_role_wave_launch_equals_two_single_launches(dt, seg):
    """the launch by itself (lt_stream_collide_twice), wrap in all three axes"""
    new, old, one = plans_for(dt, [10, 16, 128], seg)
    f0 = populations(new, dt)
    a, b, c, d = (torch.empty_like(f0) for _ in range(4))
    one.stream_collide(f0, a, TAU)
    one.stream_collide(a, b, TAU)
    new.stream_collide_twice(f0, c, TAU)
    old.stream_collide_twice(f0, d, TAU)
    torch.cuda.synchronize()
    assert torch.equal(b, c) and torch.equal(c, d)
