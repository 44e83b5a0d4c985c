"""ms per call (device events around each call; 5 warm-up calls, then [median, min, max] of 20) of four auxiliary launches
at the sizes DESIGN.md section 7 records -- lt_boundary_force and lt_link_force on cfg4's sphere (D3Q27 256^3 fp32),
lt_kinetic_energy on the same field, lt_jacobi with 64 sweeps at 256^3 fp32 -- with the library LT_ENGINE_LIBRARY names
(default: the in-tree one).  For an A/B of two builds of the library: one fresh process per build, alternating; every
call appends one JSON line that carries LABEL (which build) and RUN (its place in the alternation).  No pass/fail number.
usage: [LT_ENGINE_LIBRARY=path/to/liblettuce_hip.so] aux_launch_ab.py OUT.jsonl LABEL [RUN]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import lettuce_amd as lt
from lettuce_amd import _native

OUT, LABEL = sys.argv[1], sys.argv[2]
RUN = int(sys.argv[3]) if len(sys.argv) > 3 else 1
SIZE = 256
CENTER, RADIUS = (64.0, 128.0, 128.0), 32.0          # cfg4's sphere in lattice units (domain length 4 over 256 nodes)


def median_ms(call, warmup=5, calls=20):
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    times = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return round(statistics.median(times), 5), round(min(times), 5), round(max(times), 5)


stencil = lt.D3Q27()
res = [SIZE] * 3
g = torch.Generator().manual_seed(3)
f = ((0.5 + torch.rand([27, *res], generator=g, dtype=torch.float32)) / 27).cuda()
grid = torch.meshgrid(*[torch.arange(n, dtype=torch.float64, device="cuda") for n in res], indexing="ij")
mask = sum((x - c) ** 2 for x, c in zip(grid, CENTER)) < RADIUS ** 2
boundary = lt.InterpolatedBounceBackBoundary(mask, lt.sphere_link_fractions(stencil, grid, CENTER, RADIUS, mask=mask))
plan = _native.Plan("D3Q27", torch.float32, "none", res, [{"kind": "link_bounce_back"}])
links = lt.native_link_list(boundary, 1, mask.to(torch.uint8), stencil, torch.float32)
n_links = plan.set_links(0, *links)
solid = mask.to(torch.uint8).contiguous()
record = {"library": LABEL, "run": RUN, "resolution": res,
          "solid_nodes": int(mask.sum()), "links": n_links, "warmup": 5, "calls": 20}
record["boundary_force_ms"] = median_ms(lambda: plan.boundary_force(f, solid))
record["link_force_ms"] = median_ms(lambda: plan.link_force(0, f))
record["kinetic_energy_lu_ms"] = median_ms(lambda: plan.kinetic_energy_lu(f))
record["values"] = {"boundary_force": plan.boundary_force(f, solid).tolist(), "link_force": plan.link_force(0, f).tolist(),
                    "kinetic_energy_lu": float(plan.kinetic_energy_lu(f))}
del f, plan
rhs = torch.rand(res, generator=g, dtype=torch.float32)
rhs = (rhs - rhs.mean()).cuda()
p0 = torch.zeros_like(rhs)
record["jacobi_64_sweeps_ms"] = median_ms(lambda: _native.jacobi(rhs, p0, 0.1, 0.0, 64))
record["format"] = "[median, min, max] ms per call"
line = json.dumps(record)
print(line, flush=True)
with open(OUT, "a") as out:
    out.write(line + "\n")
