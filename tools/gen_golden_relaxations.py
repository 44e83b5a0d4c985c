"""Generate tests/golden/trt_*.npz and tests/golden/regularized_*.npz by running the REFERENCE's own PyTorch CPU path.

Build-container only, like tools/gen_golden_force.py (whose way of importing the read-only reference checkout it
shares): only the arrays written here are committed.  Run:  python tools/gen_golden_relaxations.py [substring ...]

Every file holds f0, the collided field collision(flow), f after 1, 2, 3 and 10 steps and the scalar parameters.  The
initial state is a Taylor-Green vortex (Re 1600, Ma 0.1) with 5 % multiplicative noise per population (seeded), on
D2Q9 [12, 10], D3Q15 and D3Q19 [10, 8, 6], D3Q27 [6, 8, 6], each in fp32 and fp64.
  trt_<lat>_<dt>               TRTCollision(tau_plus = 0.8, tau_minus = 3.0) -- with tau_minus = 1.1, 1.5 and 2.0 the
                               result is within 4.1e-4, 8.0e-4 and 1.1e-3 of BGK's after 10 steps (D2Q9): below or at
                               the 1e-3 asked below
  regularized_<lat>_<dt>       RegularizedCollision() at the flow's own tau (relaxation_parameter_lu, 0.5006-0.5013:
                               the reference takes it on the first call whatever the constructor got)
  regularized_tau07_<lat>_<dt> the same object with .tau = 0.7 assigned after its first call.  NOT WRITTEN: at 0.7 the
                               result is 2.2e-3 ... 3.9e-3 from BGK's after the collision but only 5.5e-4 ... 6.6e-4
                               after 10 steps (0.75: 3.5e-4 ... 4.6e-4, 0.8: 2.0e-4), below the 1e-3 asked below, and
                               towards tau = 1 both operators return feq.  The tests reach an assigned tau through the
                               mirror's torch path instead, which the files at the flow's own tau pin
Before a file is written the generator ASSERTS that the reference's result differs from the wrong operators -- BGK at
the same tau for both, for TRT also the two relaxation times swapped -- by at least 10 times the engine tests' fp32
bound (1e-5) after the collision and 100 times after 10 steps.  A fixture that does not separate is not written (the
generator says so and goes on).
"""
import contextlib
import io
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")


def import_reference():
    for name in ("h5py", "pyevtk", "pyevtk.hl", "mmh3"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["pyevtk"].hl = sys.modules["pyevtk.hl"]
    sys.path.insert(0, REF)
    with contextlib.redirect_stdout(io.StringIO()):
        import lettuce as lt
    return lt


lt = import_reference()
torch.set_num_threads(8)
DT = {"f64": torch.float64, "f32": torch.float32}
SNAPSHOTS = (1, 2, 3, 10)
TAU_PLUS, TAU_MINUS, TAU_RELAXED, NOISE = 0.8, 3.0, 0.7, 0.05
ENGINE_F32 = 1e-5       # the engine tests' fp32 bound
ONLY = sys.argv[1:]


def wanted(name):
    return not ONLY or any(k in name for k in ONLY)


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def npy(t):
    return t.detach().cpu().numpy().copy()


def save(name, **arrays):
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    assert size < 600 * 1024, f"{name}: {size} bytes"
    print(f"{name:44s} {size / 1024:9.1f} KiB")


def noisy_tgv(ctx, res, stencil, seed):
    flow = quiet(lt.TaylorGreenVortex, ctx, res, 1600, 0.1, stencil)
    g = torch.Generator().manual_seed(seed)
    factor = 1 + NOISE * (2 * torch.rand(flow.f.shape, generator=g, dtype=torch.float64) - 1)
    flow.f = (flow.f.double() * factor).to(ctx.dtype)
    return flow


def collided_and_steps(flow, collision, steps):
    collided = npy(collision(flow))
    sim = quiet(lt.Simulation, flow, collision, [])
    out = {}
    for i in range(1, max(steps) + 1):
        quiet(sim, 1)
        if i in steps:
            out[i] = npy(flow.f)
    return collided, out


def regularized(flow, tau):
    """the reference's object as a user gets it to `tau`: the first call takes the flow's tau, then .tau is assigned"""
    collision = lt.RegularizedCollision()
    collision(flow)
    if tau is not None:
        collision.tau = tau
    return collision


def case(name, res, stencil_name, dt, operator, tau, seed):
    if not wanted(name):
        return
    ctx = lt.Context(device="cpu", dtype=DT[dt], use_native=False)

    def fresh():
        return noisy_tgv(ctx, res, getattr(lt, stencil_name)(), seed)

    flow = fresh()
    f0 = npy(flow.f)
    own = float(flow.units.relaxation_parameter_lu)
    if operator == "trt":
        collision = lt.TRTCollision(TAU_PLUS, TAU_MINUS)
        tau_now = TAU_PLUS
        wrong = {"BGK at tau_plus": lambda fl: lt.BGKCollision(TAU_PLUS),
                 "relaxation times swapped": lambda fl: lt.TRTCollision(TAU_MINUS, TAU_PLUS)}
    else:
        collision = regularized(flow, tau)
        tau_now = float(collision.tau)
        assert tau_now == (own if tau is None else tau)
        wrong = {"BGK at the same tau": lambda fl: lt.BGKCollision(tau_now)}
    collided, snaps = collided_and_steps(flow, collision, SNAPSHOTS)
    assert np.isfinite(collided).all() and all(np.isfinite(v).all() for v in snaps.values())
    report = []
    for what, make in wrong.items():
        other = fresh()
        c, s = collided_and_steps(other, make(other), (10,))
        c, s = float(np.abs(c - collided).max()), float(np.abs(s[10] - snaps[10]).max())
        report.append(f"{what} {c:.2e} / {s:.2e}")
        if not (c >= 10 * ENGINE_F32 and s >= 100 * ENGINE_F32):
            print(f"  {name}: NOT WRITTEN, '{what}' separates by {c:.2e} / {s:.2e} only")
            return
    print(f"  {name}: " + "; ".join(report))
    save(name, seed=np.int64(seed), f0=f0, collided=collided, tau=np.float64(tau_now),
         tau_minus=np.float64(TAU_MINUS if operator == "trt" else 0.0), flow_tau=np.float64(own),
         noise=np.float64(NOISE), reynolds=np.float64(1600), mach=np.float64(0.1),
         resolution=np.array(flow.resolution), **{f"f{i}": v for i, v in snaps.items()})


CASES = (("d2q9", "D2Q9", [12, 10]), ("d3q15", "D3Q15", [10, 8, 6]), ("d3q19", "D3Q19", [10, 8, 6]),
         ("d3q27", "D3Q27", [6, 8, 6]))

if __name__ == "__main__":
    for seed, (tag, stencil_name, res) in enumerate(CASES):
        for dt in ("f64", "f32"):
            case(f"trt_{tag}_{dt}", res, stencil_name, dt, "trt", None, 4000 + seed)
            case(f"regularized_{tag}_{dt}", res, stencil_name, dt, "regularized", None, 4100 + seed)
            case(f"regularized_tau07_{tag}_{dt}", res, stencil_name, dt, "regularized", TAU_RELAXED, 4200 + seed)
