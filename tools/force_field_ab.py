"""A/B of the one-step kernel with a per-node force field against the one with the uniform force IN ONE PROCESS ON THE
SAME BUFFERS, alternating samples, five per side and set of buffers (the method of tools/force_ab.py; DESIGN.md section
7).  D3Q19, 256^3, fp32, periodic, BGK with Guo's force; the field is constant in space with the uniform side's values,
so that both sides compute the same populations (checked bit for bit before anything is timed).  The uniform side is
carried TWICE, so that the run-to-run spread is measured by the same samples.  One JSON line per set of buffers with every
sample, then one line with the medians and their ratio.  ms_per_update = time of one lattice update of the whole grid.
usage: force_field_ab.py [--size N]"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import lettuce_amd._native as nat

dev = torch.device("cuda:0")
TAU, ACCELERATION = 0.8, (2e-3, -3e-3, 1e-3)
SIZE = int(sys.argv[sys.argv.index("--size") + 1]) if "--size" in sys.argv else 256
SCALES = (0.5, 1 - 1 / (2 * TAU))


def sample(plan, f, g):
    """ms per lattice update over 10 ping-pong pairs of lt_stream_collide, one warm-up launch before them"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    plan.stream_collide(f, g, TAU)
    e0.record()
    for _ in range(10):
        plan.stream_collide(f, g, TAU)
        plan.stream_collide(g, f, TAU)
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) / 20, 4)


uniform = nat.Plan("D3Q19", torch.float32, "bgk", [SIZE] * 3, [], device=dev)
uniform.set_force(ACCELERATION, *SCALES)
field_plan = nat.Plan("D3Q19", torch.float32, "bgk", [SIZE] * 3, [], device=dev)
field = torch.tensor(ACCELERATION, dtype=torch.float32, device=dev).reshape(3, 1, 1, 1).expand(3, SIZE, SIZE, SIZE).contiguous()
field_plan.set_force_field(field, *SCALES)
for plan in (uniform, field_plan):
    plan.set_two_step(0, 0)
kernels = {"uniform": uniform.kernel_name(), "field": field_plan.kernel_name()}

f = uniform.empty_populations(); f.uniform_(0.04, 0.06)
a, b = uniform.empty_populations(), uniform.empty_populations()
uniform.stream_collide(f, a, TAU)
field_plan.stream_collide(f, b, TAU)
torch.cuda.synchronize()
print(json.dumps({"what": "constant field bit-identical to the uniform force", "size": SIZE,
                  "bit_identical": bool(torch.equal(a, b))}), flush=True)
del f, a, b
torch.cuda.empty_cache()

sides = {"uniform": uniform, "uniform again": uniform, "field": field_plan}
every = {name: [] for name in sides}
for trial in range(2):
    f = uniform.empty_populations(); f.uniform_(0.04, 0.06)
    g = uniform.empty_populations(); g.zero_()
    times = {name: [] for name in sides}
    for _ in range(5):
        for name, plan in sides.items():
            times[name].append(sample(plan, f, g))
    print(json.dumps({"what": "one-step D3Q19 fp32 BGK + Guo, uniform force against force field", "size": SIZE,
                      "buffers": trial, "ms_per_update": times, "kernels": kernels}), flush=True)
    for name in sides:
        every[name] += times[name]
    del f, g
    torch.cuda.empty_cache()
    junk = torch.empty(3 * 1024 ** 3 // 4, device=dev)      # shift where the next buffers land
    del junk
median = {name: statistics.median(v) for name, v in every.items()}
print(json.dumps({"what": "medians", "size": SIZE, "ms_per_update": median,
                  "field_over_uniform": round(median["field"] / median["uniform"], 4),
                  "uniform_again_over_uniform": round(median["uniform again"] / median["uniform"], 4),
                  "bytes_ratio_expected": round((2 * 19 + 3) / (2 * 19), 4)}), flush=True)
