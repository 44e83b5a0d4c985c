"""Generate tests/golden/smagorinsky_*.npz by running the REFERENCE's own PyTorch CPU path.

Build-container only, like oracle/gen_golden.py (whose way of importing the read-only reference checkout it
shares): only the arrays written here are committed.  Run:  python tools/gen_golden_smagorinsky.py [substring ...]

Periodic files (D2Q9, D3Q15, D3Q19, D3Q27 x fp32, fp64 x two parameter sets) hold f0, the collided field
collision(flow), the tau_eff field of that call, f after 1, 2, 3 and 10 steps, the kinetic-energy series and
the scalar parameters.  The initial state is a Taylor-Green vortex with multiplicative noise per population: on a
smooth state the operator is BGK to within the test tolerances.  Two sets per lattice and dtype:
  default   tau = 0.6,  constant 0.17 (the reference's default), 5 % noise
  strong    tau = 0.51, constant 1.0, 10 % noise -- here the eddy viscosity matters, and the generator ASSERTS that
            the reference's result differs from plain BGK at the same tau and from a run with iterations = 1 by at
            least 50 times the tolerance the tests use for that dtype, after the collision and after 10 steps.
            A fixture that does not separate them is not written.
Two obstacle runs (equilibrium inlet, anti-bounce-back outlet, bounce-back body; masks stored as the other obstacle
fixtures store them): Obstacle2D D2Q9 fp64 and Obstacle3D D3Q19 fp32, 10 steps each.
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
# the tolerances the separation is measured against: fp64 the 1e-12 of the engine tests; fp32 3.5e-6, i.e. the engine
# tests' 1e-5 relative to the largest population of these states (|f|max = 0.35 .. 0.49) -- the figure the inputs of
# the "strong" set (tau = 0.51, constant 1.0, 10 % noise) were chosen against.  The host tests (2e-14 / 8e-7) are
# tighter; the engine tests' absolute 1e-5 is separated from the one-iteration variant by a factor of 20 to 44.
TEST_TOL = {"f64": 1e-12, "f32": 3.5e-6}
SNAPSHOTS = (1, 2, 3, 10)
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
    print(f"{name:44s} {os.path.getsize(path) / 1024:9.1f} KiB")


def ke(flow):
    return float(lt.IncompressibleKineticEnergy(flow)())


def noisy_tgv(ctx, res, stencil, noise, seed):
    flow = quiet(lt.TaylorGreenVortex, ctx, res, 1600, 0.1, stencil)
    g = torch.Generator().manual_seed(seed)
    factor = 1 + noise * (2 * torch.rand(flow.f.shape, generator=g, dtype=torch.float64) - 1)
    flow.f = (flow.f.double() * factor).to(ctx.dtype)
    return flow


def run(flow, collision, steps):
    """f after each of `steps` and the kinetic-energy series of every step"""
    sim = quiet(lt.Simulation, flow, collision, [])
    out, energy = {}, [ke(flow)]
    for i in range(1, max(steps) + 1):
        quiet(sim, 1)
        energy.append(ke(flow))
        if i in steps:
            out[i] = npy(flow.f)
    return out, np.array(energy, dtype=np.float64), sim


def periodic_case(name, res, stencil_name, dt, tau, constant, noise, seed, separate):
    if not wanted(name):
        return
    ctx = lt.Context(device="cpu", dtype=DT[dt], use_native=False)

    def fresh():
        return noisy_tgv(ctx, res, getattr(lt, stencil_name)(), noise, seed)

    flow = fresh()
    f0 = npy(flow.f)
    collision = lt.SmagorinskyCollision(tau, constant)
    collided = npy(collision(flow))
    tau_eff = npy(collision.tau_eff)
    assert np.array_equal(npy(flow.f), f0), "collision(flow) must not change flow.f"
    snaps, energy, _ = run(flow, collision, SNAPSHOTS)
    assert all(np.isfinite(v).all() for v in snaps.values()) and np.isfinite(tau_eff).all()
    if separate:
        need = 50 * TEST_TOL[dt]
        bgk_flow = fresh()
        bgk_collided = npy(lt.BGKCollision(tau)(bgk_flow))
        bgk_snaps, _, _ = run(bgk_flow, lt.BGKCollision(tau), (10,))
        one_flow = fresh()
        one = lt.SmagorinskyCollision(tau, constant)
        one.iterations = 1
        one_collided = npy(one(one_flow))
        one_snaps, _, _ = run(one_flow, one, (10,))
        gaps = {"bgk, collide": np.abs(collided - bgk_collided).max(),
                "bgk, 10 steps": np.abs(snaps[10] - bgk_snaps[10]).max(),
                "one iteration, collide": np.abs(collided - one_collided).max(),
                "one iteration, 10 steps": np.abs(snaps[10] - one_snaps[10]).max()}
        print(f"  {name}: tau_eff in [{tau_eff.min():.4f}, {tau_eff.max():.4f}]; "
              + ", ".join(f"{k} {v:.2e}" for k, v in gaps.items()) + f" (needed {need:.1e})")
        short = {what: gap for what, gap in gaps.items() if gap < need}
        if short:
            # not accepted: other inputs (the next seed of the noise), the same parameters
            assert seed < 2500, f"{name}: no seed separates the reference from {short} by {need:.1e}"
            print(f"  {name}: seed {seed} rejected ({short})")
            return periodic_case(name, res, stencil_name, dt, tau, constant, noise, seed + 100, separate)
    save(name, seed=np.int64(seed), f0=f0, collided=collided, tau_eff=tau_eff, energy_pu=energy, tau=np.float64(tau),
         constant=np.float64(constant), noise=np.float64(noise), reynolds=np.float64(1600), mach=np.float64(0.1),
         resolution=np.array(flow.resolution), **{f"f{i}": v for i, v in snaps.items()})


def obstacle_case(name, res, stencil, dt, constant, domain_length_x, center, radius):
    if not wanted(name):
        return
    ctx = lt.Context(device="cpu", dtype=DT[dt], use_native=False)
    flow = quiet(lt.Obstacle, ctx, list(res), 100, 0.1, domain_length_x, stencil=stencil)
    r2 = sum((g - c) ** 2 for g, c in zip(flow.grid, center))
    flow.mask = (r2 < radius ** 2)
    quiet(flow.initialize)   # initial_pu depends on the mask (obstacle.py:94-99)
    tau = flow.units.relaxation_parameter_lu
    f0 = npy(flow.f)
    snaps, energy, sim = run(flow, lt.SmagorinskyCollision(tau, constant), (1, 2, 10))
    assert all(np.isfinite(v).all() for v in snaps.values())
    order = [type(b).__name__ for b in sorted(flow.boundaries, key=lambda b: str(b))]
    save(name, f0=f0, energy_pu=energy, tau=np.float64(tau), constant=np.float64(constant),
         obstacle_mask=npy(flow.mask), boundary_order=np.array(order),
         u_char_lu=np.float64(flow.units.characteristic_velocity_lu), char_length_lu=np.float64(flow.char_length_lu),
         domain_length_x=np.float64(domain_length_x), resolution=np.array(flow.resolution),
         no_collision_mask=npy(sim.no_collision_mask),
         no_streaming_mask=np.packbits(npy(sim.no_streaming_mask).astype(bool), axis=None),
         no_streaming_mask_shape=np.array(sim.no_streaming_mask.shape),
         **{f"f{i}": v for i, v in snaps.items()})


PERIODIC = (("d2q9", "D2Q9", [24, 20]), ("d3q15", "D3Q15", [10, 8, 6]), ("d3q19", "D3Q19", [10, 8, 6]),
            ("d3q27", "D3Q27", [10, 8, 6]))

if __name__ == "__main__":
    for seed, (tag, stencil_name, res) in enumerate(PERIODIC):
        for dt in ("f64", "f32"):
            periodic_case(f"smagorinsky_{tag}_default_{dt}", res, stencil_name, dt, 0.6, 0.17, 0.05, 1000 + seed, False)
            periodic_case(f"smagorinsky_{tag}_strong_{dt}", res, stencil_name, dt, 0.51, 1.0, 0.10, 2000 + seed, True)
    obstacle_case("smagorinsky_obstacle2d_d2q9_f64", [32, 20], lt.D2Q9(), "f64", 1.0, 4.0, (1.0, 1.25), 0.4)
    obstacle_case("smagorinsky_obstacle3d_d3q19_f32", [16, 12, 8], lt.D3Q19(), "f32", 1.0, 4.0, (1.0, 1.5, 1.0), 0.5)
