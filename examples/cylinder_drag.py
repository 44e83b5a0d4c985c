"""Drag and lift of a cylinder in a channel stream: the reference's `Obstacle` flow (D2Q9, equilibrium inlet,
anti-bounce-back outlet, full-way bounce-back on the cylinder) with the momentum-exchange observables
`lt.DragCoefficient` and `lt.LiftCoefficient` reported every N steps, written against `lettuce_amd`.  On an MI355X the
default context runs the HIP engine, where the force is one masked reduction over the cylinder's surface links
(`lt_boundary_force`); `--cpu` uses the torch path.  Prints the two series; from the lift's period follows the
Strouhal number.

    python examples/cylinder_drag.py [--cpu] [--ny 64] [--reynolds 100] [--steps 20000] [--interval 500]
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
    ap.add_argument("--ny", type=int, default=64, help="nodes across the stream; the domain is 3 x as long")
    ap.add_argument("--reynolds", type=float, default=100.0)
    ap.add_argument("--steps", type=int, default=20000)
    ap.add_argument("--interval", type=int, default=500)
    args = ap.parse_args()
    context = (lt.Context("cpu", torch.float64, use_native=False) if args.cpu
               else lt.Context(dtype=torch.float64))
    # physical units: a cylinder of diameter 1 in a domain 12 x 4, slightly off the centre line so that shedding starts
    ny, diameter = args.ny, 1.0
    flow = lt.Obstacle(context, [3 * ny, ny], reynolds_number=args.reynolds, mach_number=0.05, domain_length_x=12.0,
                       char_length=diameter, stencil=lt.D2Q9())
    x, y = flow.grid
    flow.mask = (x - 3.0) ** 2 + (y - 2.05) ** 2 < (diameter / 2) ** 2
    flow.initialize()                                  # fluid at rest inside the body
    body = next(b for b in flow.boundaries if isinstance(b, lt.BounceBackBoundary))
    drag = lt.ObservableReporter(lt.DragCoefficient(flow, body, area=diameter), interval=args.interval, out=None)
    lift = lt.ObservableReporter(lt.LiftCoefficient(flow, body, area=diameter), interval=args.interval, out=None)
    simulation = lt.Simulation(flow, lt.BGKCollision(flow.units.relaxation_parameter_lu), [drag, lift])
    mlups = simulation(args.steps)
    print(f"{int(flow.mask.sum())} solid nodes, tau = {flow.units.relaxation_parameter_lu:.4f}")
    print("step      t_pu        C_d         C_l")
    for (i, t, cd), (_, _, cl) in zip(drag.out, lift.out):
        print(f"{i:<9d} {t:<11.4f} {cd:<11.6f} {cl:<11.6f}")
    print(f"{mlups:.1f} MLUPS on {context.device} "
          f"({'HIP engine' if context.use_native else 'torch ops'})")


if __name__ == "__main__":
    main()
