"""A/B of the fused one-step MRT kernel beside the one-step BGK and KBC kernels of the same unit IN ONE PROCESS ON THE
SAME BUFFERS, alternating samples, five per side and two sets of buffers (the method of tools/same_buffer_ab.py and
tools/relaxations_ab.py).  One JSON line per case and set of buffers:
  d3q27   D3Q27 256^3 fp32, Hermite
  small   D2Q9 128^2 fp64, Lallemand
  large   D2Q9 4096^2 fp32, Lallemand
ms_per_update = time of one lattice update of the whole grid; glups = nodes / that time.
usage: mrt_ab.py [d3q27] [small] [large]        (profiles/mrt_ab.jsonl is this output)"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import lettuce_amd._native as nat

dev = torch.device("cuda:0")
TAU = 0.51
CASES = {"d3q27": ("D3Q27", torch.float32, [256] * 3, "D3Q27Hermite", tuple(range(4, 10))),
         "small": ("D2Q9", torch.float64, [128] * 2, "D2Q9Lallemand", (3, 4)),
         "large": ("D2Q9", torch.float32, [4096] * 2, "D2Q9Lallemand", (3, 4))}
WHAT = [a for a in sys.argv[1:] if a in CASES] or list(CASES)


def rates_of(q, d, second):
    """tau on the second-order moments, distinct rates 1.05 + 0.05 k on the higher ones (tools/gen_golden_mrt.py)"""
    rates, k = [], 0
    for i in range(q):
        if i <= d:
            rates.append(1.0)
        elif i in second:
            rates.append(TAU)
        else:
            rates.append(1.05 + 0.05 * k)
            k += 1
    return rates


def sample(launch, f, g):
    """ms per lattice update over 10 ping-pong pairs of `launch`"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    launch(f, g)
    e0.record()
    for _ in range(10):
        launch(f, g)
        launch(g, f)
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) / 20, 5)


for case in WHAT:
    lattice, dtype, res, transform, second = CASES[case]
    plans = {}
    for collision in ("bgk", "kbc", "mrt"):
        plan = nat.Plan(lattice, dtype, collision, res, [], device=dev)
        if collision == "mrt":
            plan.set_mrt(transform, rates_of(plan.q, plan.d, second))
        plan.set_two_step(0, 0)
        plans[collision] = plan
    nodes = 1
    for r in res:
        nodes *= r
    for trial in range(2):
        f = plans["bgk"].empty_populations(); f.uniform_(0.9 / plans["bgk"].q, 1.1 / plans["bgk"].q)
        g = plans["bgk"].empty_populations(); g.zero_()
        times = {name: [] for name in plans}
        for _ in range(5):
            for name, plan in plans.items():
                times[name].append(sample(lambda a, b, p=plan: p.stream_collide(a, b, TAU), f, g))
        best = {name: min(v) for name, v in times.items()}
        print(json.dumps({"what": f"one-step {lattice} {'x'.join(map(str, res))} {str(dtype).split('.')[1]} {transform}",
                          "buffers": trial, "ms_per_update": times,
                          "glups_best": {name: round(nodes / (t * 1e6), 3) for name, t in best.items()},
                          "mrt_over_bgk_best": round(best["mrt"] / best["bgk"], 3),
                          "finite": bool(torch.isfinite(f).all()),
                          "kernels": {name: plan.kernel_name() for name, plan in plans.items()}}), flush=True)
        del f, g
        torch.cuda.empty_cache()
        junk = torch.empty(3 * 1024 ** 3 // 4, device=dev)      # shift where the next buffers land
        del junk
