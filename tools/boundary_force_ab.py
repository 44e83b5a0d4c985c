"""lt.BoundaryForce on the HIP path against its torch expression, IN ONE PROCESS ON THE SAME STATE, alternating, the
median of 20 timed calls per side after 5 warm-up calls, device events around each call.
  "hip"    lt.BoundaryForce(flow, body)() on a native context: lt_boundary_force, two launches
  "torch"  the torch expression of the definition on the same device and the same flow.f
           (lettuce_amd.ext._reporter.momentum_exchange: one torch.roll of the mask per q, masked gathers, fp64 sums)
cfg4 of bench.py: Obstacle D3Q27 256^3 fp32 with the sphere mask, after 20 KBC steps.  Also recorded: the surface of the
body, the bytes the kernel reads by construction (one byte per node; per solid node the bytes of its q - 1 neighbours;
per link from a solid to a fluid node one population) and the peak memory of each side.  If the torch side cannot
allocate, the record holds its error message instead of its times: that is the finding.  No pass/fail number.
usage: boundary_force_ab.py [--size 256] [--steps 20] [--out profiles/boundary_force_ab.jsonl]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import lettuce_amd as lt
from lettuce_amd.ext._reporter import momentum_exchange

WARMUP, CALLS = 5, 20


def option(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


SIZE = int(option("--size", "256"))
STEPS = int(option("--steps", "20"))
OUT = option("--out", os.path.join(ROOT, "profiles", "boundary_force_ab.jsonl"))


def timed(call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    call()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1), 4)


def peak_mib(call):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    call()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - before) / 2 ** 20, 1)


def main():
    assert torch.cuda.is_available(), "boundary_force_ab.py measures on the GPU"
    ctx = lt.Context(device="cuda:0", dtype=torch.float32, use_native=True)
    flow = lt.Obstacle(ctx, [SIZE] * 3, 100, 0.1, domain_length_x=4, stencil=lt.D3Q27())
    x, y, z = flow.grid
    flow.mask = ((x - 1) ** 2 + (y - 2) ** 2 + (z - 2) ** 2) < 0.5 ** 2
    flow.initialize()
    simulation = lt.Simulation(flow, lt.KBCCollision(), [])
    simulation(STEPS)
    f = flow.f                                         # completes the pending streaming pass
    body = next(b for b in flow.boundaries if isinstance(b, lt.BounceBackBoundary))
    observable = lt.BoundaryForce(flow, body)
    solid = observable.mask != 0
    stencil = flow.stencil
    links = 0
    for q in range(1, stencil.q):
        e = [int(v) for v in stencil.e[q]]
        links += int((solid & ~torch.roll(solid, shifts=tuple(e), dims=(0, 1, 2))).sum())
    nodes, solid_nodes = solid.numel(), int(solid.sum())
    record = {"what": f"BoundaryForce, Obstacle D3Q27 {SIZE}^3 fp32 (cfg4's sphere) after {STEPS} KBC steps",
              "resolution": [SIZE] * 3, "solid_nodes": solid_nodes, "solid_to_fluid_links": links,
              "kernel_bytes_by_construction": nodes + solid_nodes * (stencil.q - 1) + links * 4,
              "torch_bytes_of_f": f.numel() * 4, "warmup": WARMUP, "calls": CALLS}
    sides = {"hip": lambda: observable(f), "torch": lambda: momentum_exchange(stencil, f, solid)}
    try:
        a, b = observable.force(f).double().cpu(), sides["torch"]().double().cpu()
        record["force_hip"], record["force_torch"] = a.tolist(), b.tolist()
    except torch.OutOfMemoryError as error:
        record["torch_error"] = str(error).splitlines()[0]
        del sides["torch"]
        record["force_hip"] = observable.force(f).double().cpu().tolist()
    times = {name: [] for name in sides}
    for n in range(WARMUP + CALLS):
        for name, call in sides.items():             # alternating
            t = timed(call)
            if n >= WARMUP:
                times[name].append(t)
    record["ms_per_call"] = times
    record["median_ms"] = {name: statistics.median(v) for name, v in times.items()}
    record["min_ms"] = {name: min(v) for name, v in times.items()}
    record["peak_mib"] = {name: peak_mib(call) for name, call in sides.items()}
    if "torch" in sides:
        record["torch_over_hip"] = round(record["median_ms"]["torch"] / record["median_ms"]["hip"], 2)
    line = json.dumps(record)
    print(line, flush=True)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as out:
        out.write(line + "\n")


if __name__ == "__main__":
    main()
