"""A/B of the Smagorinsky kernels IN ONE PROCESS ON THE SAME BUFFERS, alternating samples, five per side (the method of
tools/same_buffer_ab.py).  256^3, fp32, one JSON line per comparison and set of buffers:
  one-step   lt_stream_collide with Smagorinsky against BGK (D3Q19) and against BGK and KBC (D3Q27), dense buffers
  two-step   D3Q19: one two-step Smagorinsky launch against two one-step Smagorinsky launches, on dense buffers and on
             buffers with the engine's pad between populations (what lt_run's resident mode streams from)
  residency  D3Q19 one-step Smagorinsky by workgroups per CU (lt_plan_set_residency; 3 = what BGK gets, 0 = no cap)
ms_per_update = time of one lattice update of the whole grid.
usage: smagorinsky_ab.py [one-step] [two-step] [residency] [--size N]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import lettuce_amd._native as nat

dev = torch.device("cuda:0")
TAU, CONSTANT = 0.51, 0.17
SIZE = int(sys.argv[sys.argv.index("--size") + 1]) if "--size" in sys.argv else 256
WHAT = [a for a in sys.argv[1:] if a in ("one-step", "two-step", "residency")] or ["one-step", "two-step"]


def plan_for(lattice, collision, padded=False, two_step=False):
    plan = nat.Plan(lattice, torch.float32, collision, [SIZE] * 3, [], device=dev)
    if collision == "smagorinsky":
        plan.set_smagorinsky(CONSTANT)
    if padded:
        plan.set_population_stride(-(-(SIZE ** 3 + 32832) // 64) * 64)
    if two_step:
        plan.set_two_step(1, 0)
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


def compare(tag, sides, buffers_of):
    """sides: name -> (launch(f, g), lattice updates per call); two sets of buffers, five alternating samples each"""
    for trial in range(2):
        f = buffers_of.empty_populations(); f.uniform_(0.04, 0.06)
        g = buffers_of.empty_populations(); g.zero_()
        times = {name: [] for name in sides}
        for _ in range(5):
            for name, (launch, updates) in sides.items():
                times[name].append(sample(launch, f, g, updates))
        print(json.dumps({"what": tag, "size": SIZE, "buffers": trial, "ms_per_update": times,
                          "kernels": {name: kernel for name, kernel in KERNELS.items() if name in sides}}), flush=True)
        del f, g
        torch.cuda.empty_cache()
        junk = torch.empty(3 * 1024 ** 3 // 4, device=dev)      # shift where the next buffers land
        del junk


KERNELS = {}


if "one-step" in WHAT:
    for lattice, collisions in (("D3Q19", ("bgk", "smagorinsky")), ("D3Q27", ("bgk", "kbc", "smagorinsky"))):
        sides, first = {}, None
        for collision in collisions:
            plan = plan_for(lattice, collision)
            plan.set_two_step(0)
            first = first or plan
            sides[collision] = (lambda f, g, p=plan: p.stream_collide(f, g, TAU), 1)
            KERNELS[collision] = plan.kernel_name()
        compare(f"one-step {lattice} fp32 dense", sides, first)

if "residency" in WHAT:
    sides, first = {}, None
    for collision, caps in (("bgk", (3,)), ("smagorinsky", (3, 4, 5, 0))):
        for cap in caps:
            plan = plan_for("D3Q19", collision)
            plan.set_two_step(0)
            plan.set_residency(cap)
            first = first or plan
            sides[f"{collision} {cap} per CU"] = (lambda f, g, p=plan: p.stream_collide(f, g, TAU), 1)
            KERNELS[f"{collision} {cap} per CU"] = plan.kernel_name()
    compare("one-step D3Q19 fp32 dense by workgroups per CU", sides, first)

if "two-step" in WHAT:
    for padded in (False, True):
        single = plan_for("D3Q19", "smagorinsky", padded)
        single.set_two_step(0)
        twice = plan_for("D3Q19", "smagorinsky", padded, two_step=True)
        KERNELS["one-step pair"], KERNELS["two-step"] = single.kernel_name(), twice.kernel_name()
        f = twice.empty_populations(); f.uniform_(0.04, 0.06)
        a, b, c = twice.empty_populations(), twice.empty_populations(), twice.empty_populations()
        single.stream_collide(f, a, TAU)
        single.stream_collide(a, b, TAU)
        twice.stream_collide_twice(f, c, TAU)
        torch.cuda.synchronize()
        same = bool(torch.equal(b, c))
        del f, a, b, c
        torch.cuda.empty_cache()
        bgk = plan_for("D3Q19", "bgk", padded, two_step=True)      # for scale: BGK's two-step launch on the same buffers
        KERNELS["two-step bgk"] = bgk.kernel_name()
        sides = {"one-step pair": (lambda f, g, p=single: p.stream_collide(f, g, TAU), 1),
                 "two-step": (lambda f, g, p=twice: p.stream_collide_twice(f, g, TAU), 2),
                 "two-step bgk": (lambda f, g, p=bgk: p.stream_collide_twice(f, g, TAU), 2)}
        print(json.dumps({"what": "two-step D3Q19 fp32 bit-identical to two one-step launches", "padded": padded,
                          "bit_identical": same}), flush=True)
        compare(f"two-step D3Q19 fp32 {'padded' if padded else 'dense'}", sides, twice)
