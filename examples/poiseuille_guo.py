"""Plane Poiseuille flow driven by a body force: the channel of the reference's `PoiseuilleFlow2D` (D2Q9, bounce-back
rows at y = 0 and y = -1, periodic along x) with Guo's forcing scheme inside the BGK collision, written against
`lettuce_amd`.  On an MI355X the default context runs the HIP engine, whose collide kernels take the force
(`lt_plan_set_force`); `--cpu` uses the torch path.  Prints the distance of the velocity profile from the parabola.

    python examples/poiseuille_guo.py [--cpu] [--resolution 32] [--steps 20000]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lettuce_amd as lt  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--resolution", type=int, default=32)
    ap.add_argument("--steps", type=int, default=20000)
    args = ap.parse_args()
    context = (lt.Context("cpu", torch.float64, use_native=False) if args.cpu
               else lt.Context(dtype=torch.float64))
    flow = lt.PoiseuilleFlow2D(context, resolution=args.resolution, reynolds_number=10, mach_number=0.05,
                               stencil=lt.D2Q9)
    tau = flow.units.relaxation_parameter_lu
    force = lt.Guo(flow, tau, [1e-6, 0.0])             # acceleration in lattice units
    simulation = lt.Simulation(flow, lt.BGKCollision(tau, force=force), [])
    mlups = simulation(args.steps)
    # lattice units: walls half a spacing inside the bounce-back rows, u_x = a / (2 nu) (y - 1/2) (ny - 3/2 - y)
    ny = flow.resolution[1]
    y = torch.arange(1, ny - 1, dtype=torch.float64)
    a = float(force.acceleration[0])
    parabola = a / (2 * flow.units.viscosity_lu) * (y - 0.5) * (ny - 1.5 - y)
    u = flow.u(acceleration=force.acceleration)[0][:, 1:-1].double().cpu()
    distance = float((u - parabola[None, :]).abs().max() / parabola.max())
    print(f"tau = {tau:.4f}, a = {a:.3e} (lattice units), {args.steps} steps")
    print(f"peak velocity {float(u.max()):.6e}, parabola {float(parabola.max()):.6e}")
    print(f"distance from the parabola: {distance:.3e} of the peak velocity")
    print(f"{mlups:.1f} MLUPS on {context.device} "
          f"({'HIP engine' if context.use_native else 'torch ops'})")


if __name__ == "__main__":
    main()
