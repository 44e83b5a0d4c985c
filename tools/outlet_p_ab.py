"""A/B of the constant-pressure outlet against the anti-bounce-back outlet IN ONE PROCESS ON THE SAME BUFFERS,
alternating samples, five per side and two sets of buffers (the method of tools/relaxations_ab.py).
The reference's Obstacle (inlet at x = 0, a bounce-back sphere, the outlet on +x), D3Q19, fp32, 256^3, BGK, both plans
held to one step per launch (lt_stream_collide): the masked one-step kernel with the anti-bounce-back outlet (ABBD 0,
lane hand-over where the rows allow it) against the pressure-outlet kernel (ABBD 6).  One JSON line per set of buffers;
ms_per_update = time of one lattice update of the whole grid.
usage: outlet_p_ab.py [--size N]        (profiles/outlet_p_ab.jsonl holds the lines of one run at 256^3)"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import lettuce_amd as lt

dev = torch.device("cuda:0")
SIZE = int(sys.argv[sys.argv.index("--size") + 1]) if "--size" in sys.argv else 256
TAU = 0.51


class PressureObstacle(lt.Obstacle):
    @property
    def boundaries(self):
        inlet, _, solid = super().boundaries
        return [inlet, lt.EquilibriumOutletP(self._unit_vector().tolist(), self, rho_outlet=1.0), solid]


def plan_of(cls):
    context = lt.Context(device="cuda:0", dtype=torch.float32, use_native=True)
    flow = cls(context, [SIZE] * 3, 100, 0.05, domain_length_x=10, stencil=lt.D3Q19())
    x, y, z = flow.grid
    flow.mask = ((x - 3.0) ** 2 + (y - 5.0) ** 2 + (z - 5.0) ** 2) < 1.0
    sim = lt.Simulation(flow, lt.BGKCollision(TAU), [])
    sim._native._sync_masks()
    sim._native.plan.set_two_step(0)
    sim._native.plan.set_many_step(0)
    return sim, sim._native.plan, flow.f.clone()


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


sims = {"abb outlet": plan_of(lt.Obstacle), "pressure outlet": plan_of(PressureObstacle)}
sides = {name: (lambda f, g, p=plan: p.stream_collide(f, g, TAU)) for name, (_, plan, _) in sims.items()}
kernels = {name: plan.kernel_name() for name, (_, plan, _) in sims.items()}
start = sims["abb outlet"][2]
for trial in range(2):
    f, g = start.clone(), torch.zeros_like(start)
    times = {name: [] for name in sides}
    for _ in range(5):
        for name, launch in sides.items():
            f.copy_(start)                                   # every sample from the same state
            times[name].append(sample(launch, f, g))
    print(json.dumps({"what": "Obstacle D3Q19 fp32 one step per launch", "size": SIZE, "buffers": trial,
                      "ms_per_update": times, "kernels": kernels}), flush=True)
    del f, g
    torch.cuda.empty_cache()
    junk = torch.empty(3 * 1024 ** 3 // 4, device=dev)      # shift where the next buffers land
    del junk
