"""A/B of the one-step BGK kernel with the incompressible equilibrium against the one-step quadratic BGK kernel of the
same build, IN ONE PROCESS ON THE SAME BUFFERS, alternating samples, five per side and two sets of buffers (the method of
tools/relaxations_ab.py).  The quadratic kernel is sampled twice per round ("quadratic" and
"quadratic again"): the spread of one kernel against itself is what a ratio between two kernels is read against.
  D3Q19 256^3 fp32 and D2Q9 4096^2 fp64, lt_stream_collide on dense buffers, one JSON line per grid and set of buffers
ms_per_update = time of one lattice update of the whole grid.
usage: incompressible_ab.py [--size3d N] [--size2d N]        (profiles/incompressible_ab.jsonl is this output)"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import lettuce_amd._native as nat

dev = torch.device("cuda:0")
TAU, RHO0 = 0.51, 1.1


def option(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


GRIDS = (("D3Q19", torch.float32, [option("--size3d", 256)] * 3), ("D2Q9", torch.float64, [option("--size2d", 4096)] * 2))


def plan_for(lattice, dtype, res, incompressible):
    plan = nat.Plan(lattice, dtype, "bgk", res, [], device=dev)
    if incompressible:
        plan.set_equilibrium("incompressible", RHO0)
    plan.set_two_step(0, 0)
    return plan


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
    return round(e0.elapsed_time(e1) / 20, 4)


for lattice, dtype, res in GRIDS:
    quadratic, incompressible = plan_for(lattice, dtype, res, False), plan_for(lattice, dtype, res, True)
    sides = {"quadratic": quadratic, "incompressible": incompressible, "quadratic again": quadratic}
    kernels = {name: plan.kernel_name() for name, plan in sides.items()}
    for trial in range(2):
        f = quadratic.empty_populations(); f.uniform_(0.04, 0.06)
        g = quadratic.empty_populations(); g.zero_()
        times = {name: [] for name in sides}
        for _ in range(5):
            for name, plan in sides.items():
                times[name].append(sample(lambda a, b, p=plan: p.stream_collide(a, b, TAU), f, g))
        median = {name: statistics.median(v) for name, v in times.items()}
        print(json.dumps({"what": f"one-step BGK {lattice} {str(dtype).split('.')[-1]} dense", "resolution": res,
                          "buffers": trial, "ms_per_update": times,
                          "incompressible_over_quadratic": round(median["incompressible"] / median["quadratic"], 4),
                          "quadratic_again_over_quadratic": round(median["quadratic again"] / median["quadratic"], 4),
                          "kernels": kernels}), flush=True)
        del f, g
        torch.cuda.empty_cache()
        junk = torch.empty(3 * 1024 ** 3 // 4, device=dev)      # shift where the next buffers land
        del junk
