"""A/B of the kernels with a body force IN ONE PROCESS ON THE SAME BUFFERS, alternating samples, five per side and set
of buffers (the method of tools/same_buffer_ab.py).  D3Q19, 256^3, fp32, BGK with Guo's force,
one JSON line per comparison and set of buffers; every comparison carries the unforced side TWICE, so that the
run-to-run spread is measured by the same samples:
  (a) one-step   lt_stream_collide unforced (twice) against forced, dense buffers
  (b) two-step   the unforced one-role sweep (shift policy 6; twice) against the forced sweep
  (c) forced     one forced two-step launch against two forced one-step launches
(b) and (c) on dense buffers and on buffers with the engine's pad between populations (what lt_run's resident mode
streams from).  ms_per_update = time of one lattice update of the whole grid.
usage: force_ab.py [--size N]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import lettuce_amd._native as nat

dev = torch.device("cuda:0")
TAU, ACCELERATION = 0.8, (2e-3, -3e-3, 1e-3)
SIZE = int(sys.argv[sys.argv.index("--size") + 1]) if "--size" in sys.argv else 256


def plan_for(forced, padded=False, two_step=False):
    plan = nat.Plan("D3Q19", torch.float32, "bgk", [SIZE] * 3, [], device=dev)
    if forced:
        plan.set_force(ACCELERATION, 0.5, 1 - 1 / (2 * TAU))
    if padded:
        plan.set_population_stride(-(-(SIZE ** 3 + 32832) // 64) * 64)
    plan.set_two_step(1 if two_step else 0, 0)
    if two_step and not forced:
        plan.set_shift_policy(6)            # the one-role schedule, which the forced sweep runs
    return plan


def sample(launch, f, g, updates_per_call):
    """ms per lattice update over 10 ping-pong pairs of `launch`"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    launch(f, g)
    e0.record()
    for _ in range(10):
        launch(f, g)
        launch(g, f)
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) / (20 * updates_per_call), 4)


def compare(tag, sides, buffers_of, kernels):
    """sides: name -> (launch(f, g), lattice updates per call); two sets of buffers, five alternating samples each"""
    for trial in range(2):
        f = buffers_of.empty_populations(); f.uniform_(0.04, 0.06)
        g = buffers_of.empty_populations(); g.zero_()
        times = {name: [] for name in sides}
        for _ in range(5):
            for name, (launch, updates) in sides.items():
                times[name].append(sample(launch, f, g, updates))
        print(json.dumps({"what": tag, "size": SIZE, "buffers": trial, "ms_per_update": times, "kernels": kernels}),
              flush=True)
        del f, g
        torch.cuda.empty_cache()
        junk = torch.empty(3 * 1024 ** 3 // 4, device=dev)      # shift where the next buffers land
        del junk


def one(plan):
    return (lambda f, g, p=plan: p.stream_collide(f, g, TAU), 1)


def two(plan):
    return (lambda f, g, p=plan: p.stream_collide_twice(f, g, TAU), 2)


unforced, forced = plan_for(False), plan_for(True)
compare("(a) one-step D3Q19 fp32 dense", {"unforced": one(unforced), "unforced again": one(unforced), "forced": one(forced)},
        unforced, {"unforced": unforced.kernel_name(), "forced": forced.kernel_name()})
for padded in (False, True):
    where = "padded" if padded else "dense"
    single = plan_for(True, padded)
    twice = plan_for(True, padded, two_step=True)
    plain = plan_for(False, padded, two_step=True)
    f = twice.empty_populations(); f.uniform_(0.04, 0.06)
    a, b, c = twice.empty_populations(), twice.empty_populations(), twice.empty_populations()
    single.stream_collide(f, a, TAU)
    single.stream_collide(a, b, TAU)
    twice.stream_collide_twice(f, c, TAU)
    torch.cuda.synchronize()
    print(json.dumps({"what": "forced two-step launch bit-identical to two forced one-step launches", "padded": padded,
                      "bit_identical": bool(torch.equal(b, c))}), flush=True)
    del f, a, b, c
    torch.cuda.empty_cache()
    compare(f"(b) two-step D3Q19 fp32 {where}",
            {"unforced one-role": two(plain), "unforced one-role again": two(plain), "forced": two(twice)}, twice,
            {"unforced one-role": plain.kernel_name(), "forced": twice.kernel_name()})
    compare(f"(c) forced D3Q19 fp32 {where}",
            {"two-step": two(twice), "one-step pair": one(single), "one-step pair again": one(single)}, twice,
            {"two-step": twice.kernel_name(), "one-step pair": single.kernel_name()})
