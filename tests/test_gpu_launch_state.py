"""No entry point of the engine leaves a trace in the plan.

What belongs to one launch -- the second plane range and the segment length of the edge launches, the counter of the
signalling launch, the received halo messages of the direct edge launch, the strides of the resident buffers, the steps
of a many-step launch -- is handed to the launch and kept nowhere.  So a plan that has been through every slab driver,
through a refused call, through the first-use check with resident buffers in flight or through a many-step launch
computes, in its next call, exactly what a fresh plan computes in that call.  Every comparison is bit for bit.
"""
import pytest
import torch

from conftest import TORCH_DT
from oracle import lettuce_oracle as orc
from test_gpu_engine import dev, plan_for
from test_gpu_paths_vs_oracle import TAU, perturbed_state
from test_gpu_slab_launches_vs_oracle import UNTOUCHED, _message_sets

pytestmark = pytest.mark.gpu


def _untouched(plan):
    out = plan.empty_populations()
    out.fill_(UNTOUCHED)
    return out


# --------------------------------------------------------------------------- slab: every two-step driver, then one more
def _slab_plan(lat, dt, res):
    from lettuce_amd._native import Plan, LAYOUT_SLAB
    plan = Plan(lat, TORCH_DT[dt], "bgk", res, [], layout=LAYOUT_SLAB, ghost_planes=2)
    plan.set_two_step(1, 3)
    return plan


@pytest.mark.parametrize("lat,dt,res", [("D3Q19", "f32", [64, 16, 5]), ("D3Q15", "f64", [32, 16, 5])],
                         ids=["D3Q19-f32", "D3Q15-f64"])
def test_slab_drivers_leave_nothing_behind_for_the_next_launch(lat, dt, res):
    """one tile wide, two tiles high, 9 memory planes, edges of 2, segments of 3"""
    from lettuce_amd._native import NativeEngineError
    nx, ny, n2 = res[0], res[1], res[2] + 4
    edge = 2
    f_cpu = perturbed_state(lat, [nx, ny, n2], TORCH_DT[dt], 5).permute(0, 3, 2, 1).contiguous()
    f = dev(f_cpu)
    # the ghost planes as the messages the neighbours would have sent; the field's own are NaN
    in_plane, up, down = _message_sets(lat)
    from_below = dev(torch.cat([f_cpu[in_plane, 1], f_cpu[up, 1], f_cpu[up, 0]]))
    from_above = dev(torch.cat([f_cpu[in_plane, n2 - 2], f_cpu[down, n2 - 2], f_cpu[down, n2 - 1]]))
    poisoned = f.clone()
    poisoned[:, :2] = float("nan")
    poisoned[:, n2 - 2:] = float("nan")

    fresh = _slab_plan(lat, dt, res)
    want = _untouched(fresh)
    fresh.stream_collide_twice_planes(f, want, TAU, 2, n2 - 2)

    plan = _slab_plan(lat, dt, res)
    blocks = plan.two_step_message_blocks()

    def messages():
        return (torch.full([blocks, ny, nx], UNTOUCHED, dtype=f.dtype, device="cuda") for _ in range(2))

    def same_as_fresh(out, ranges, what):
        owned = torch.zeros(n2, dtype=torch.bool, device="cuda")
        for b, e in ranges:
            owned[b:e] = True
        assert torch.equal(out[:, owned], want[:, owned]), what
        assert bool((out[:, ~owned] == UNTOUCHED).all()), (what, "wrote planes it does not own")

    edges = [(2, 2 + edge), (n2 - 2 - edge, n2 - 2)]
    out, (lower, upper) = _untouched(plan), messages()
    plan.stream_collide_twice_edges(f, out, TAU, edge, pack_lower=lower, pack_upper=upper)              # 1
    same_as_fresh(out, edges, "edges with messages")
    out, (lower, upper) = _untouched(plan), messages()
    plan.stream_collide_twice_edges_direct(poisoned, out, TAU, edge, from_below, from_above, lower, upper)   # 2
    same_as_fresh(out, edges, "direct edges from the received messages")
    out = _untouched(plan)
    plan.stream_collide_twice_slab(f, out, TAU)                                                         # 3
    same_as_fresh(out, [(2, n2 - 2)], "signalling launch")
    out, (lower, upper) = _untouched(plan), messages()
    plan.stream_collide_twice_planes_packed(f, out, TAU, 2, n2 - 2, pack_lower=lower, pack_upper=upper)   # 4
    same_as_fresh(out, [(2, n2 - 2)], "packed launch over the whole slab")
    with pytest.raises(NativeEngineError, match=r"in-place operation is not supported \(in == out\)") as refused:   # 5
        plan.stream_collide_twice_edges_direct(f, f, TAU, edge, from_below, from_above, lower, upper)
    assert refused.value.code == 1                                                                      # LT_ERR_INVALID
    # 6: no second range, no segment of `edge` planes, no counter, no received messages, no NaN from (2) are left
    out = _untouched(plan)
    plan.stream_collide_twice_planes(f, out, TAU, 2, n2 - 2)
    torch.cuda.synchronize()
    same_as_fresh(out, [(2, n2 - 2)], "the launch after all of them")


# --------------------------------------------------------------------------- periodic, masks: the first-use check
RES_MASKED = [8, 8, 64]                  # contiguous extent 64: one tile of the masked two-step kernel


def _masked_plan(canary=1):
    """one bounce-back block, one face of equilibrium nodes; two steps per launch on resident buffers"""
    L = orc.LATTICES["D3Q19"]
    e, w = orc.lattice_tensors(L, torch.float32)
    feq = orc.quadratic_equilibrium(torch.tensor(1.02, dtype=torch.float32),
                                    torch.tensor([0.04, 0.01, -0.02], dtype=torch.float32), e, w)
    entries = [{"kind": "bounce_back"}, {"kind": "equilibrium", "feq": feq.double().tolist()}]
    ncm = torch.zeros(RES_MASKED, dtype=torch.uint8)
    ncm[3:5, 2:5, 20:30] = 1
    ncm[0] = 2
    plan = plan_for("D3Q19", torch.float32, "bgk", RES_MASKED, entries)
    plan.set_masks(dev(ncm), dev(torch.zeros([L.q] + RES_MASKED, dtype=torch.uint8)))
    plan.set_two_step(1)
    plan.set_resident(1)
    plan.set_canary(canary)
    return plan


def _resident_four_steps(plan, f):
    plan.resident_load(f, TAU)
    plan.resident_advance(TAU, 4)
    info = plan.last_run_info()
    out = plan.resident_store(torch.empty_like(f))
    torch.cuda.synchronize()
    return out, info


def test_first_use_check_inside_a_resident_advance_leaves_nothing_behind():
    f = dev(perturbed_state("D3Q19", RES_MASKED, torch.float32, 7))
    checked, trusted = _masked_plan(canary=1), _masked_plan(canary=0)
    out_checked, info_checked = _resident_four_steps(checked, f)      # the check fires in here, resident strides in flight
    out_trusted, info_trusted = _resident_four_steps(trusted, f)
    assert checked.canary_status()["status"] == 1, checked.canary_status()
    assert trusted.canary_status()["status"] == 2, trusted.canary_status()
    assert info_checked == info_trusted == {"single_step_launches": 0, "two_step_launches": 2, "many_step_launches": 0}
    assert torch.equal(out_checked, out_trusted)
    # ... and the plan's own buffers are the caller's again
    got, _ = checked.run(f.clone(), torch.empty_like(f), TAU, 3)
    want, _ = _masked_plan().run(f.clone(), torch.empty_like(f), TAU, 3)
    torch.cuda.synchronize()
    assert torch.equal(got, want)


# --------------------------------------------------------------------------- 2-D: a many-step launch, then lt_run
def test_many_step_launch_leaves_nothing_behind_for_lt_run():
    res = [64, 16]
    f = dev(perturbed_state("D2Q9", res, torch.float64, 11))

    def plan_with_many_steps():
        plan = plan_for("D2Q9", torch.float64, "bgk", res)
        plan.set_many_step(1)
        return plan

    plan = plan_for("D2Q9", torch.float64, "bgk", res)
    plan.stream_collide_many(f, torch.empty_like(f), TAU, 3)
    plan.set_many_step(1)
    got, _ = plan.run(f.clone(), torch.empty_like(f), TAU, 5)
    fresh = plan_with_many_steps()
    want, _ = fresh.run(f.clone(), torch.empty_like(f), TAU, 5)
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    assert plan.last_run_info() == fresh.last_run_info() == {"single_step_launches": 0, "two_step_launches": 0,
                                                             "many_step_launches": 1}
