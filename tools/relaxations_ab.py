"""A/B of the TRT and the regularised kernels IN ONE PROCESS ON THE SAME BUFFERS, alternating samples, five per side and
two sets of buffers (the method of tools/smagorinsky_ab.py and tools/same_buffer_ab.py).  256^3,
D3Q19, fp32, one JSON line per comparison and set of buffers:
  one-step   lt_stream_collide with TRT and with the regularised collision against BGK, dense buffers
  two-step   per operator: one two-step launch against two of its own one-step launches, on dense buffers and on
             buffers with the engine's pad between populations (what lt_run's resident mode streams from)
ms_per_update = time of one lattice update of the whole grid.
usage: relaxations_ab.py [one-step] [two-step] [--size N]        (profiles/relaxations_ab.jsonl is this output)"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import lettuce_amd._native as nat

dev = torch.device("cuda:0")
TAU, TAU_MINUS = 0.51, 19.25          # tau_minus = 1/2 + (3/16) / (tau - 1/2)
SIZE = int(sys.argv[sys.argv.index("--size") + 1]) if "--size" in sys.argv else 256
WHAT = [a for a in sys.argv[1:] if a in ("one-step", "two-step")] or ["one-step", "two-step"]
OPERATORS = ("trt", "regularized")


def plan_for(collision, padded=False, two_step=False):
    plan = nat.Plan("D3Q19", torch.float32, collision, [SIZE] * 3, [], device=dev)
    if collision == "trt":
        plan.set_trt(TAU_MINUS)
    if padded:
        plan.set_population_stride(-(-(SIZE ** 3 + 32832) // 64) * 64)
    plan.set_two_step(1 if two_step else 0, 0)
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


def compare(tag, sides, kernels, buffers_of):
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


if "one-step" in WHAT:
    sides, kernels, first = {}, {}, None
    for collision in ("bgk",) + OPERATORS:
        plan = plan_for(collision)
        first = first or plan
        sides[collision] = (lambda f, g, p=plan: p.stream_collide(f, g, TAU), 1)
        kernels[collision] = plan.kernel_name()
    compare("one-step D3Q19 fp32 dense", sides, kernels, first)

if "two-step" in WHAT:
    for operator in OPERATORS:
        for padded in (False, True):
            single = plan_for(operator, padded)
            twice = plan_for(operator, padded, two_step=True)
            kernels = {"one-step pair": single.kernel_name(), "two-step": twice.kernel_name()}
            f = twice.empty_populations(); f.uniform_(0.04, 0.06)
            a, b, c = twice.empty_populations(), twice.empty_populations(), twice.empty_populations()
            single.stream_collide(f, a, TAU)
            single.stream_collide(a, b, TAU)
            twice.stream_collide_twice(f, c, TAU)
            torch.cuda.synchronize()
            same = bool(torch.equal(b, c))
            del f, a, b, c
            torch.cuda.empty_cache()
            sides = {"one-step pair": (lambda f, g, p=single: p.stream_collide(f, g, TAU), 1),
                     "two-step": (lambda f, g, p=twice: p.stream_collide_twice(f, g, TAU), 2)}
            print(json.dumps({"what": f"two-step {operator} D3Q19 fp32 bit-identical to two one-step launches",
                              "padded": padded, "bit_identical": same}), flush=True)
            compare(f"two-step {operator} D3Q19 fp32 {'padded' if padded else 'dense'}", sides, kernels, twice)
