"""cfg4 of bench.py (Obstacle D3Q27 256^3 fp32 KBC, the sphere) with the full-way BounceBackBoundary against the
InterpolatedBounceBackBoundary with sphere_link_fractions, IN ONE PROCESS, alternating, device events around batches of
steps after warm-up batches.
  "full_way"      lt.Obstacle as it is: the solid nodes bounce back inside the stepping kernel
  "interpolated"  lt.Obstacle(solid_boundary=...): the stepping kernel leaves the solid nodes alone and one launch over
                  the link list follows every step (link_bounce_kernel)
Also recorded: solid nodes and links, the link pass's own time (Plan.apply_links on the stepper's plan, device events
around batches of calls), the drag coefficient of both bodies after the timed steps.  No pass/fail number.
usage: link_bounce_ab.py [--size 256] [--batch 50] [--rounds 8] [--out profiles/link_bounce_ab.jsonl]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import lettuce_amd as lt

WARMUP = 2


def option(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


SIZE = int(option("--size", "256"))
BATCH = int(option("--batch", "50"))
ROUNDS = int(option("--rounds", "8"))
OUT = option("--out", os.path.join(ROOT, "profiles", "link_bounce_ab.jsonl"))
CENTER, RADIUS = (1.0, 2.0, 2.0), 0.5


def timed(call, count):
    """ms per call of `count` calls between two device events"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(count):
        call()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) / count, 5)


def build(ctx, interpolated):
    made = []

    def solid_boundary(mask):
        # once per flow (flow.boundaries builds its list anew on every access); the fractions on the device: [q, *res]
        # in fp64 is 3.6 GB at 256^3, the link list that is kept a few MB
        if not made:
            grid = tuple(g.to(ctx.device) for g in flow.grid)
            made.append(lt.InterpolatedBounceBackBoundary(mask, lt.sphere_link_fractions(flow.stencil, grid, CENTER, RADIUS,
                                                                                         mask=mask)))
        return made[0]
    flow = lt.Obstacle(ctx, [SIZE] * 3, 100, 0.1, domain_length_x=4, stencil=lt.D3Q27(),
                       solid_boundary=solid_boundary if interpolated else None)
    x, y, z = flow.grid
    flow.mask = ((x - CENTER[0]) ** 2 + (y - CENTER[1]) ** 2 + (z - CENTER[2]) ** 2) < RADIUS ** 2
    flow.initialize()
    simulation = lt.Simulation(flow, lt.KBCCollision(), [])
    return flow, simulation


def main():
    assert torch.cuda.is_available(), "link_bounce_ab.py measures on the GPU"
    ctx = lt.Context(device="cuda:0", dtype=torch.float32, use_native=True)
    sides = {"full_way": build(ctx, False), "interpolated": build(ctx, True)}
    body = sides["interpolated"][1].boundaries[-1]
    assert isinstance(body, lt.InterpolatedBounceBackBoundary)
    links = body.links(sides["interpolated"][0].stencil, torch.float32)
    record = {"what": f"Obstacle D3Q27 {SIZE}^3 fp32 KBC (cfg4's sphere): full-way against interpolated bounce-back",
              "resolution": [SIZE] * 3, "solid_nodes": int(body.mask.sum()), "links": len(links),
              "links_below_one_half": int((~links.second).sum()), "batch": BATCH, "rounds": ROUNDS, "warmup_batches": WARMUP}
    times = {name: [] for name in sides}
    for n in range(WARMUP + ROUNDS):
        for name, (flow, simulation) in sides.items():               # alternating
            t = timed(lambda: simulation(BATCH), 1) / BATCH
            if n >= WARMUP:
                times[name].append(round(t, 5))
    record["ms_per_step"] = times
    record["median_ms_per_step"] = {name: statistics.median(v) for name, v in times.items()}
    record["min_ms_per_step"] = {name: min(v) for name, v in times.items()}
    record["interpolated_over_full_way"] = round(record["median_ms_per_step"]["interpolated"]
                                                 / record["median_ms_per_step"]["full_way"], 4)
    record["launches"] = {name: simulation._native.plan.last_run_info() for name, (_, simulation) in sides.items()}
    record["kernel"] = {name: simulation._native.plan.kernel_name() for name, (_, simulation) in sides.items()}
    # the pass alone: on a copy of the populations (it is in place), the stepper's plan and list
    flow, simulation = sides["interpolated"]
    scratch = flow.f.clone()
    plan = simulation._native.plan
    alone = [timed(lambda: plan.apply_links(scratch), 200) for _ in range(WARMUP + ROUNDS)][WARMUP:]
    record["link_pass_ms"] = alone
    record["link_pass_median_ms"] = statistics.median(alone)
    del scratch
    for name, (flow, simulation) in sides.items():
        solid = simulation.boundaries[-1] if name == "interpolated" else flow.mask
        record.setdefault("drag_coefficient", {})[name] = float(lt.DragCoefficient(flow, solid, area=3.14159265 * RADIUS ** 2)())
    record["steps_done"] = {name: flow.i for name, (flow, _) in sides.items()}
    line = json.dumps(record)
    print(line, flush=True)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as out:
        out.write(line + "\n")


if __name__ == "__main__":
    main()
