"""Generate tests/golden/jacobi_*.npz and pressure_decay_16x16.npz by running the REFERENCE's own PyTorch CPU path.

Build-container only, like tools/gen_golden_spectrum.py (whose way of importing the read-only reference checkout it
shares): only the arrays written here are committed.  Run:  python tools/gen_golden_jacobi.py [substring ...]

(a) jacobi_<shape>.npz -- fixed sweep counts.  Seeded random rhs and p0 without symmetries (uniform in +-0.05, drawn in
    fp64, rounded to fp32 so that both dtypes start from the same numbers), dx = 0.37.  For dt in (f32, f64): p1_<dt>, p2_<dt>,
    p3_<dt>, p8_<dt> (the reference's torch_jacobi with tol_abs = 0.0 and max_num_steps = 1, 2, 3, 8), r8_<dt> (the residuum of
    the 8th iterate, by the reference's expression) and err_<dt> (float64 [8]: mean(r^2) of the iterates 1 ... 8 with
    r widened to fp64 and the squares summed by math.fsum -- the exact-order-free value the engine's error is held to).
    2-D: [1, 7], [2, 3], [5, 7], [12, 20], [33, 17], [64, 66]; 3-D: [2, 3, 1], [6, 10, 7], [17, 5, 33].
(b) in jacobi_12x20.npz and jacobi_6x10x7.npz also a tolerance stop: tol_<dt> = sqrt(err5 * err6) of the reference's own
    errors (the tensors of its `error > tol_abs`), stop_<dt> = its result for that tolerance and stop_it_<dt> = the
    iteration count, identified by matching the result against the sequence of iterates.  ASSERTS err6 / err5 < 0.99: the
    verdict then sits at least 0.5 % from both neighbours.  (The reference starts from error = 1: a tolerance of 1 or
    more ends it before the first sweep, hence the amplitude.)
(c) pressure_decay_16x16.npz -- lt.DecayingTurbulence(resolution [16, 16], Re 1000, Ma 0.05, D2Q9, k0 = 2, randseed = 1), ALL
    defaults (initialize_pressure and initialize_fneq on): rho_<dt> (pressure_poisson of the flow's initial state, what
    initialize() uses) and f_<dt> (the constructed flow.f), fp64 and fp32.
"""
import math

import numpy as np
import torch

from gen_golden_relaxations import lt, DT, wanted, quiet, npy, save  # noqa: F401
from lettuce._flow import pressure_poisson
from lettuce.util import torch_jacobi

DX = 0.37
AMPLITUDE = 0.05         # of rhs and p0: the errors of the first iterates are then below 1, the reference's starting value
COUNTS = (1, 2, 3, 8)
SHAPES = [[1, 7], [2, 3], [5, 7], [12, 20], [33, 17], [64, 66], [2, 3, 1], [6, 10, 7], [17, 5, 33]]
STOPS = [[12, 20], [6, 10, 7]]


def residuum(f, p, dim):
    """the reference's residuum of p: its expression, restated with a loop over the axes in its order"""
    total = None
    for shift in (1, -1):
        for axis in range(dim):
            term = p.roll(shifts=shift, dims=axis)
            total = term if total is None else total + term
    return f - (total - 2 * dim * p) / (DX ** 2)


def mean_square(r):
    v = r.double().numpy().ravel()
    return math.fsum(v * v) / v.size


def case(shape, seed):
    name = "jacobi_" + "x".join(str(n) for n in shape)
    if not wanted(name):
        return
    dim = len(shape)
    g = torch.Generator().manual_seed(seed)
    rhs = (AMPLITUDE * (2 * torch.rand(shape, generator=g, dtype=torch.float64) - 1)).to(torch.float32)
    p0 = (AMPLITUDE * (2 * torch.rand(shape, generator=g, dtype=torch.float64) - 1)).to(torch.float32)
    out = dict(rhs=npy(rhs), p0=npy(p0), dx=np.float64(DX))
    for dt in ("f32", "f64"):
        f, p = rhs.to(DT[dt]), p0.to(DT[dt])
        iterates = [torch_jacobi(f, p, DX, dim, tol_abs=0.0, max_num_steps=n) for n in range(1, 13)]
        for n in COUNTS:
            out[f"p{n}_{dt}"] = npy(iterates[n - 1])
        out[f"r8_{dt}"] = npy(residuum(f, iterates[7], dim))
        out[f"err_{dt}"] = np.array([mean_square(residuum(f, q, dim)) for q in iterates[:8]])
        if shape in STOPS:
            # the reference's own errors: tensors of the context dtype
            e5, e6 = (float(torch.mean(residuum(f, iterates[k], dim) ** 2)) for k in (4, 5))
            assert e6 / e5 < 0.99, (name, dt, e6 / e5)
            tol = math.sqrt(e5 * e6)
            stop = torch_jacobi(f, p, DX, dim, tol_abs=tol, max_num_steps=100)
            hits = [k + 1 for k, q in enumerate(iterates) if torch.equal(q, stop)]
            assert hits == [6], (name, dt, hits)
            out[f"tol_{dt}"], out[f"stop_{dt}"], out[f"stop_it_{dt}"] = np.float64(tol), npy(stop), np.int64(hits[0])
            print(f"  {name} {dt}: err5 {e5:.6e}, err6 {e6:.6e} (ratio {e6 / e5:.3f}), tol {tol:.6e}")
    save(name, **out)


def decay():
    name = "pressure_decay_16x16"
    if not wanted(name):
        return
    out = {}
    for dt in ("f64", "f32"):
        ctx = lt.Context(device="cpu", dtype=DT[dt], use_native=False)
        flow = quiet(lt.DecayingTurbulence, ctx, [16, 16], 1000, 0.05, k0=2, randseed=1)
        assert flow.initialize_pressure and flow.initialize_fneq and type(flow.stencil).__name__ == "D2Q9"
        out[f"f_{dt}"] = npy(flow.f)
        p0, u0 = flow.initial_pu()
        rho0 = ctx.convert_to_tensor(flow.units.convert_pressure_pu_to_density_lu(p0))
        u0 = ctx.convert_to_tensor(flow.units.convert_velocity_to_lu(u0))
        out[f"rho_{dt}"] = npy(pressure_poisson(flow.units, u0, rho0))
    out.update(resolution=np.array([16, 16]), reynolds=np.float64(1000), mach=np.float64(0.05), k0=np.float64(2),
               randseed=np.int64(1))
    print(f"  {name}: max |rho - 1| {np.abs(out['rho_f64'] - 1).max():.3e}, fp32 against fp64: "
          f"rho {np.abs(out['rho_f32'] - out['rho_f64']).max():.3e}, f {np.abs(out['f_f32'] - out['f_f64']).max():.3e}")
    save(name, **out)


if __name__ == "__main__":
    for i, shape in enumerate(SHAPES):
        case(shape, 8100 + i)
    decay()
