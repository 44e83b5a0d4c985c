"""Kolmogorov flow: a doubly periodic box driven by the body force a_x = A sin(k y), spun up from rest towards the
laminar steady state u_x = A / (nu k^2) sin(k y) -- `lt.KolmogorovFlow2D` with `lt.GuoField`, Guo's forcing scheme with an
acceleration per node inside the BGK collision.  On an MI355X the default context runs the HIP engine, whose collide
kernels read the field (`lt_plan_set_force_field`); `--cpu` uses the torch path.  Prints the series of the kinetic energy
and the distance of the velocity profile from the analytic one.

    python examples/kolmogorov_flow.py [--cpu] [--resolution 64] [--wavenumber 1] [--viscous-times 12]
"""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lettuce_amd as lt  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--resolution", type=int, default=64)
    ap.add_argument("--wavenumber", type=int, default=1)
    ap.add_argument("--viscous-times", type=float, default=12.0, help="run for this many 1 / (nu k^2)")
    args = ap.parse_args()
    context = (lt.Context("cpu", torch.float64, use_native=False) if args.cpu
               else lt.Context(dtype=torch.float64))
    flow = lt.KolmogorovFlow2D(context, [args.resolution] * 2, reynolds_number=1.0, mach_number=0.01,
                               wavenumber=args.wavenumber)
    tau = flow.units.relaxation_parameter_lu
    force = lt.GuoField(flow, tau, flow.acceleration_lu())           # [2, nx, ny], lattice units
    k = 2 * math.pi * args.wavenumber / args.resolution
    steps = int(args.viscous_times / (flow.units.viscosity_lu * k * k))
    energy = lt.ObservableReporter(lt.IncompressibleKineticEnergy(flow), interval=max(1, steps // 12), out=None)
    simulation = lt.Simulation(flow, lt.BGKCollision(tau, force=force), [energy])
    mlups = simulation(steps)
    print(f"tau = {tau:.4f}, A = {flow.amplitude_lu:.3e} (lattice units), k = {k:.4f}, {steps} steps")
    print("step, time, kinetic energy (physical units)")
    for row in energy.out:
        print("  " + ", ".join(f"{float(v):.6e}" for v in row))
    # the velocity with the half-force correction of the scheme, against the laminar profile
    u = flow.units.convert_velocity_to_pu(flow.u(acceleration=force.acceleration)).double().cpu()
    want = flow.analytic_solution(steps)[1].double().cpu()
    error = float(((u - want) ** 2).sum().sqrt() / (want ** 2).sum().sqrt())
    print(f"relative L2 distance from u_x = sin({args.wavenumber} y): {error:.3e}")
    print(f"max |u_y| {float(u[1].abs().max()):.2e}")
    print(f"{mlups:.1f} MLUPS on {context.device} "
          f"({'HIP engine' if context.use_native else 'torch ops'})")


if __name__ == "__main__":
    main()
