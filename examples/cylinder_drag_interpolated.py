"""Drag of a cylinder with the wall where the circle is: the cylinder of `cylinder_drag.py` (the reference's `Obstacle`,
D2Q9, equilibrium inlet; here with the constant-pressure outlet) run twice -- with the full-way `BounceBackBoundary`, which puts the wall half
a link from the nearest node whatever the shape (a staircase), and with `lt.InterpolatedBounceBackBoundary`, whose link
fractions `lt.sphere_link_fractions` takes from the circle itself (linear interpolated bounce-back after Bouzidi,
Firdaouss and Lallemand).  `lt.DragCoefficient` reports the momentum-exchange force on either body every N steps.  On an
MI355X the default context runs the HIP engine: one sparse launch over the cylinder's links follows every step
(`lt_plan_set_links`), and the force is a sum over the same list (`lt_link_force`); `--cpu` uses the torch path.

    python examples/cylinder_drag_interpolated.py [--cpu] [--ny 64] [--reynolds 100] [--steps 20000] [--interval 500]
                                                  [--collision bgk|kbc]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lettuce_amd as lt  # noqa: E402

CENTER, DIAMETER = (3.0, 2.05), 1.0


class Stream(lt.Obstacle):
    """the Obstacle with the constant-pressure outlet it names as the alternative to its anti-bounce-back outlet (which
    at these parameters goes unstable near step 3700, whatever the body's boundary)"""

    @property
    def boundaries(self):
        inlet, _, body = super().boundaries
        return [inlet, lt.EquilibriumOutletP(self._unit_vector().tolist(), self), body]


def run(context, args, interpolated):
    def on_the_circle(mask):
        return lt.InterpolatedBounceBackBoundary(mask, lt.sphere_link_fractions(flow.stencil, flow.grid, CENTER,
                                                                                DIAMETER / 2, mask=mask))
    ny = args.ny
    flow = Stream(context, [3 * ny, ny], reynolds_number=args.reynolds, mach_number=0.05, domain_length_x=12.0,
                       char_length=DIAMETER, stencil=lt.D2Q9(), solid_boundary=on_the_circle if interpolated else None)
    x, y = flow.grid
    flow.mask = (x - CENTER[0]) ** 2 + (y - CENTER[1]) ** 2 < (DIAMETER / 2) ** 2
    flow.initialize()                                  # fluid at rest inside the body
    body = flow.boundaries[-1]                         # the same mask and fractions as the simulation's own
    drag = lt.ObservableReporter(lt.DragCoefficient(flow, body, area=DIAMETER), interval=args.interval, out=None)
    tau = flow.units.relaxation_parameter_lu
    collision = lt.KBCCollision(tau) if args.collision == "kbc" else lt.BGKCollision(tau)
    simulation = lt.Simulation(flow, collision, [drag])
    mlups = simulation(args.steps)
    return drag.out, mlups, int(flow.mask.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--ny", type=int, default=64, help="nodes across the stream; the domain is 3 x as long")
    ap.add_argument("--reynolds", type=float, default=100.0)
    ap.add_argument("--steps", type=int, default=20000)
    ap.add_argument("--interval", type=int, default=500)
    ap.add_argument("--collision", choices=["bgk", "kbc"], default="bgk")
    args = ap.parse_args()
    context = (lt.Context("cpu", torch.float64, use_native=False) if args.cpu
               else lt.Context(dtype=torch.float64))
    full, mlups_full, solid = run(context, args, False)
    new, mlups_new, _ = run(context, args, True)
    print(f"{solid} solid nodes")
    print("step      t_pu        C_d full-way   C_d interpolated")
    for (i, t, a), (_, _, b) in zip(full, new):
        print(f"{i:<9d} {t:<11.4f} {a:<14.6f} {b:<14.6f}")
    print(f"{mlups_full:.1f} / {mlups_new:.1f} MLUPS (full-way / interpolated) on {context.device} "
          f"({'HIP engine' if context.use_native else 'torch ops'})")


if __name__ == "__main__":
    main()
