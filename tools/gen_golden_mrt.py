"""Generate tests/golden/mrt_*.npz and tests/golden/asymmetric_mrt_*.npz by running the REFERENCE's own PyTorch CPU path
(MRTCollision with D2Q9Dellar, D2Q9Lallemand and D3Q27Hermite).

Build-container only, like tools/gen_golden_relaxations.py (whose way of importing the read-only reference checkout it
shares): only the arrays written here are committed.  Run:  python tools/gen_golden_mrt.py [substring ...]

  mrt_{dellar,lallemand}_d2q9_{f64,f32}, mrt_hermite_d3q27_{f64,f32}
      Taylor-Green vortex (Re 1600, Ma 0.1; D2Q9 16 x 16, D3Q27 8^3) times 1 +- 5 % noise per population (seeded).
      f0, rates, collided = collision(flow), f after 1, 2, 3 and 10 steps.  The f32 files also hold collided_f64 and
      f<i>_f64: the reference run in fp64 from the same fp32 state -- what the fp32 run's own error is measured against.
  asymmetric_mrt_{dellar,lallemand}_d2q9_f64, asymmetric_mrt_hermite_d3q27_f64
      the states of tests/golden/asymmetric_states_{d2q9,d3q27}_f64.npz (densities 0.5 - 1.5 and 1/20 - 20) with the
      keys of the other asymmetric_* files: moderate at tau 0.501 (collided, 1 and 5 steps), wide at 0.7 and 1.7
      (collided, 1 step).

Rates: 1.0 for the conserved moments, tau for the second-order ones (Dellar 3-5, Lallemand 3-4, Hermite 4-9; 0.7 in the
mrt_* files) and 1.05 + 0.05 k for the k-th remaining moment -- all distinct, so a permuted rate shows up.  Before a
file is written the generator asserts that the result is finite and at least 1e-4 from BGK at the same tau.
"""
import os
import sys
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden_relaxations import lt, quiet, npy, noisy_tgv, collided_and_steps, DT, SNAPSHOTS, OUT  # noqa: E402
from lettuce.util import moments as ref_moments  # noqa: E402

warnings.filterwarnings("ignore")
TAU = 0.7
ONLY = [a for a in sys.argv[1:]]
# transform -> (class, lattice tag, stencil, resolution, indices of the second-order moments)
TRANSFORMS = {"dellar": ("D2Q9Dellar", "d2q9", "D2Q9", [16, 16], (3, 4, 5)),
              "lallemand": ("D2Q9Lallemand", "d2q9", "D2Q9", [16, 16], (3, 4)),
              "hermite": ("D3Q27Hermite", "d3q27", "D3Q27", [8, 8, 8], tuple(range(4, 10)))}


def save(name, **arrays):
    """(the fp32 Hermite file holds its fp64 twin as well: 0.75 MiB, below the 1 MiB a committed file may have)"""
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    assert size < 1000 * 1024, f"{name}: {size} bytes"
    print(f"{name:44s} {size / 1024:9.1f} KiB")


def wanted(name):
    return not ONLY or any(k in name for k in ONLY)


def rates_of(transform, tau):
    _, _, stencil, _, second = TRANSFORMS[transform]
    q, d = int(stencil.split("Q")[1]), int(stencil[1])
    rates, k = [], 0
    for i in range(q):
        if i <= d:
            rates.append(1.0)
        elif i in second:
            rates.append(tau)
        else:
            rates.append(1.05 + 0.05 * k)
            k += 1
    assert len(set(rates[i] for i in range(d + 1, q) if i not in second)) == q - d - 1 - len(second)
    return rates


def mrt(ctx, transform, stencil, rates):
    return lt.MRTCollision(getattr(ref_moments, TRANSFORMS[transform][0])(stencil, ctx), rates, ctx)


def tgv_case(transform, dt, seed):
    cls, tag, stencil_name, res, _ = TRANSFORMS[transform]
    name = f"mrt_{transform}_{tag}_{dt}"
    if not wanted(name):
        return
    ctx = lt.Context(device="cpu", dtype=DT[dt], use_native=False)
    rates = rates_of(transform, TAU)
    flow = noisy_tgv(ctx, res, getattr(lt, stencil_name)(), seed)
    f0 = npy(flow.f)
    collided, snaps = collided_and_steps(flow, mrt(ctx, transform, flow.stencil, rates), SNAPSHOTS)
    assert np.isfinite(collided).all() and all(np.isfinite(v).all() for v in snaps.values())
    other = noisy_tgv(ctx, res, getattr(lt, stencil_name)(), seed)
    gap = float(np.abs(npy(lt.BGKCollision(TAU)(other)) - collided).max())
    assert gap >= 1e-4, gap
    extra = {}
    if dt == "f32":
        ctx64 = lt.Context(device="cpu", dtype=torch.float64, use_native=False)
        flow64 = quiet(lt.TaylorGreenVortex, ctx64, res, 1600, 0.1, getattr(lt, stencil_name)())
        flow64.f = torch.tensor(f0).double()
        c64, s64 = collided_and_steps(flow64, mrt(ctx64, transform, flow64.stencil, rates), SNAPSHOTS)
        extra = {"collided_f64": c64, **{f"f{i}_f64": v for i, v in s64.items()}}
        w = np.array(flow.stencil.w).reshape([-1] + [1] * len(res))
        print(f"  {name}: E_ref collided {(np.abs(collided - c64) / w).max():.2e}, "
              f"10 steps {(np.abs(snaps[10] - s64[10]) / w).max():.2e}")
    print(f"  {name}: |MRT - BGK({TAU})| = {gap:.2e}")
    save(name, seed=np.int64(seed), f0=f0, rates=np.array(rates), collided=collided, tau=np.float64(TAU),
         noise=np.float64(0.05), reynolds=np.float64(1600), mach=np.float64(0.1), resolution=np.array(res),
         **{f"f{i}": v for i, v in snaps.items()}, **extra)


def asymmetric_case(transform):
    cls, tag, stencil_name, _, _ = TRANSFORMS[transform]
    name = f"asymmetric_mrt_{transform}_{tag}_f64"
    if not wanted(name):
        return
    states = np.load(os.path.join(OUT, f"asymmetric_states_{tag}_f64.npz"))
    res = [int(r) for r in states["resolution"]]
    ctx = lt.Context(device="cpu", dtype=torch.float64, use_native=False)
    out = {}
    for kind, tau, steps in (("moderate", 0.501, (1, 5)), ("wide", 0.7, (1,)), ("wide", 1.7, (1,))):
        flow = quiet(lt.TaylorGreenVortex, ctx, res, 1600, 0.1, getattr(lt, stencil_name)())
        flow.f = torch.tensor(states[f"f0_{kind}"])
        rates = rates_of(transform, tau)
        collided, snaps = collided_and_steps(flow, mrt(ctx, transform, flow.stencil, rates), steps)
        assert np.isfinite(collided).all() and all(np.isfinite(v).all() for v in snaps.values())
        key = f"{kind}_tau{tau}"
        out[f"{key}_tau_used"] = np.float64(tau)
        out[f"{key}_rates"] = np.array(rates)
        out[f"{key}_collided"] = collided
        for i, v in snaps.items():
            out[f"{key}_f{i}"] = v
    save(name, **out)


if __name__ == "__main__":
    for n, transform in enumerate(TRANSFORMS):
        for dt in ("f64", "f32"):
            tgv_case(transform, dt, 5000 + n)
        asymmetric_case(transform)
    # how far the two D2Q9 transforms are apart on the same state and rates' recipe
    a, b = (np.load(os.path.join(OUT, f"mrt_{t}_d2q9_f64.npz")) for t in ("dellar", "lallemand"))
    print(f"|Dellar - Lallemand| on their fixtures' collided fields: {np.abs(a['collided'] - b['collided']).max():.2e}")
