"""Generate tests/golden/spectrum_<flow>_<shape>.npz by running the REFERENCE's own PyTorch CPU path.

Build-container only, like tools/gen_golden_equilibria.py (whose way of importing the read-only reference checkout
it shares): only the arrays written here are committed.  Run:  python tools/gen_golden_spectrum.py [substring ...]

Cases: Taylor-Green vortex (Re 1600, Ma 0.1) on D2Q9 [16, 16], [6, 8], [7, 9], [33, 32] and D3Q19 [8, 12, 10],
[5, 6, 7], [16, 16, 16]; DecayingTurbulence (Re 1000, Ma 0.05, ic_energy 0.5, initialize_pressure=False) on D2Q9
[16, 16] (k0 4) and [9, 9] (k0 2) and D3Q19 [12, 12, 12] (k0 3), each with its own randseed.

Every file holds
  f0                      the flow's initial populations with 5 % seeded multiplicative noise, rounded to fp32: every
                          bin of its spectrum then holds real energy
  f10_f32, f10_f64        the reference's states after 10 BGK steps (tau = 0.6) from f0, run in fp32 and in fp64
                          (f10_f64 goes to spectrum_<...>_f64state.npz where one file would pass 900 KiB)
  spec0_f32, spec0_f64    the reference's EnergySpectrum of f0 in an fp32 and an fp64 context
  spec10_f32, spec10_f64  ... of f10_f32 in the fp32 and of f10_f64 in the fp64 context
  resolution, stencil, reynolds, mach, tau, noise, seed
and for DecayingTurbulence also randseed, k0, ic_energy, u_init (initial_pu's velocity, float64), spectrum and
wavenumbers (flow.energy_spectrum), char_velocity_pu and spec_init_f64: the reference's EnergySpectrum of its own
initial state (no noise) in fp64.

Before a file is written the generator ASSERTS that on each of the four states the smallest bin holds at least 6e-7 of
the largest, so that per-bin relative errors mean something.
"""
import numpy as np
import torch

from gen_golden_relaxations import lt, DT, NOISE, wanted, quiet, npy, save, OUT  # noqa: F401

TAU, STEPS, FLOOR = 0.6, 10, 6e-7
SPLIT = 900 * 1024
TGV = [("D2Q9", [16, 16]), ("D2Q9", [6, 8]), ("D2Q9", [7, 9]), ("D2Q9", [33, 32]),
       ("D3Q19", [8, 12, 10]), ("D3Q19", [5, 6, 7]), ("D3Q19", [16, 16, 16])]
DECAY = [("D2Q9", [16, 16], 4, 11), ("D2Q9", [9, 9], 2, 12), ("D3Q19", [12, 12, 12], 3, 13)]


def make_flow(kind, dt, stencil_name, res, k0=None, randseed=None):
    ctx = lt.Context(device="cpu", dtype=DT[dt], use_native=False)
    stencil = getattr(lt, stencil_name)()
    if kind == "tgv":
        return quiet(lt.TaylorGreenVortex, ctx, list(res), 1600, 0.1, stencil)
    return quiet(lt.DecayingTurbulence, ctx, list(res), 1000, 0.05, k0=k0, ic_energy=0.5, stencil=stencil,
                 initialize_pressure=False, randseed=randseed)


def spectrum(flow):
    return npy(quiet(lt.EnergySpectrum, flow)()).astype(np.float64 if flow.context.dtype == torch.float64 else np.float32)


def case(kind, stencil_name, res, seed, k0=None, randseed=None):
    name = f"spectrum_{kind}_" + "x".join(str(n) for n in res)
    if not wanted(name):
        return
    out, extra = {}, {}
    f0 = None
    for dt in ("f32", "f64"):
        flow = make_flow(kind, dt, stencil_name, res, k0, randseed)
        if kind == "decay" and dt == "f64":
            extra = dict(randseed=np.int64(randseed), k0=np.float64(k0), ic_energy=np.float64(0.5),
                         u_init=np.asarray(flow.initial_pu()[1], dtype=np.float64),
                         spectrum=np.asarray(flow.energy_spectrum[0], dtype=np.float64),
                         wavenumbers=np.asarray(flow.energy_spectrum[1]),
                         char_velocity_pu=np.float64(flow.units.characteristic_velocity_pu),
                         spec_init_f64=spectrum(flow))
        if f0 is None:
            g = torch.Generator().manual_seed(seed)
            factor = 1 + NOISE * (2 * torch.rand(flow.f.shape, generator=g, dtype=torch.float64) - 1)
            f0 = (flow.f.double() * factor).to(torch.float32)
        flow.f = f0.to(DT[dt])
        out[f"spec0_{dt}"] = spectrum(flow)
        sim = quiet(lt.Simulation, flow, lt.BGKCollision(TAU), [])
        quiet(sim, STEPS)
        out[f"f10_{dt}"] = npy(flow.f)
        out[f"spec10_{dt}"] = spectrum(flow)
    for key in ("spec0_f32", "spec0_f64", "spec10_f32", "spec10_f64"):
        s = out[key].astype(np.float64)
        assert np.isfinite(s).all() and s.min() >= FLOOR * s.max(), (name, key, s.min() / s.max())
    e_ref = np.abs(out["spec10_f32"].astype(np.float64) - out["spec10_f64"]).max() / out["spec10_f64"].max()
    print(f"  {name}: K = {len(out['spec0_f64'])}, min / max bin {min(out[k].min() / out[k].max() for k in out if k.startswith('spec')):.2e}, "
          f"E_ref (10 steps) {e_ref:.2e}")
    out.update(extra)
    out.update(f0=npy(f0), resolution=np.array(res), stencil=np.array(stencil_name), reynolds=np.float64(
        1600 if kind == "tgv" else 1000), mach=np.float64(0.1 if kind == "tgv" else 0.05), tau=np.float64(TAU),
        noise=np.float64(NOISE), seed=np.int64(seed))
    if sum(v.nbytes for v in out.values()) > SPLIT:
        save(name + "_f64state", f10_f64=out.pop("f10_f64"))
    save(name, **out)


if __name__ == "__main__":
    for i, (stencil_name, res) in enumerate(TGV):
        case("tgv", stencil_name, res, 7000 + i)
    for i, (stencil_name, res, k0, randseed) in enumerate(DECAY):
        case("decay", stencil_name, res, 7100 + i, k0, randseed)
