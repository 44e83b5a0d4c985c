"""Generate tests/golden/force_*.npz by running the REFERENCE's own PyTorch CPU path.

Build-container only, like tools/gen_golden_smagorinsky.py (whose way of importing the read-only reference checkout
it shares): only the arrays written here are committed.  Run:  python tools/gen_golden_force.py [substring ...]

Periodic files hold f0, the collided field collision(flow), f after 1, 2, 3 and 10 steps, u(acceleration) of the
initial state and the scalar parameters.  The initial state is a Taylor-Green vortex with 5 % multiplicative noise per
population (seeded); tau = 0.8 (0.51 with Smagorinsky, constant 1.0), acceleration (2e-3, -3e-3, 1e-3)[:d] -- three
different components, so that a wrong axis permutation shows.
  guo_bgk         D2Q9 [12, 10], D3Q15 and D3Q19 [10, 8, 6], D3Q27 [6, 8, 6]
  guo_smagorinsky D2Q9, D3Q19
  shanchen_bgk    D2Q9, D3Q19
each in fp32 and fp64.  Before a Guo + BGK file is written the generator ASSERTS that the reference's result differs
from six wrong operators (no force, no velocity shift, a shift of 1, a source term without its 1 - 1 / (2 tau), the
acceleration's components reversed, force.tau = 0.6) by at least 10 times the engine tests' fp32 bound (1e-5) after
the collision and 100 times after 10 steps, and -- in fp64, against the 1e-12 of the fp64 engine tests -- from two
subtler ones (the source term evaluated at the unshifted velocity, Shan-Chen in place of Guo).  The other schemes are
held against "no force" and "components reversed".  A fixture that does not separate is not written.
One PoiseuilleFlow2D run (Guo + BGK, D2Q9 [16, 16], fp64, 10 steps): masks stored as the obstacle fixtures store
them, the analytic solution and the unit conversion's scalars.
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
ACCELERATION = (2e-3, -3e-3, 1e-3)
TAU, NOISE = 0.8, 0.05
ENGINE_F32, ENGINE_F64 = 1e-5, 1e-12       # the engine tests' bounds
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


class WrongGuo(lt.Guo):
    """Guo's scheme with one thing wrong: the velocity shift, or the factor of the source term"""

    def __init__(self, flow, tau, acceleration, shift=0.5, factor=True):
        super().__init__(flow, tau, acceleration)
        self._shift, self._factor = shift, factor

    @property
    def ueq_scaling_factor(self):
        return self._shift

    def source_term(self, u):
        s = super().source_term(u)
        return s if self._factor else s / (1 - 1 / (2 * self.tau))


class SourceAtUnshiftedVelocity(lt.BGKCollision):
    def __call__(self, flow):
        u = flow.u() + self.force.u_eq(flow)
        feq = flow.equilibrium(flow, u=u)
        return flow.f - 1.0 / self.tau * (flow.f - feq) + self.force.source_term(flow.u())


def collided_and_steps(flow, collision, steps):
    collided = npy(collision(flow))
    sim = quiet(lt.Simulation, flow, collision, [])
    out = {}
    for i in range(1, max(steps) + 1):
        quiet(sim, 1)
        if i in steps:
            out[i] = npy(flow.f)
    return collided, out


def make_collision(scheme, operator, flow, tau, force_tau, acceleration, constant):
    force = {"guo": lt.Guo, "shanchen": lt.ShanChen}[scheme](flow, force_tau, acceleration)
    if operator == "bgk":
        return lt.BGKCollision(tau, force=force), force
    return lt.SmagorinskyCollision(tau, constant, force=force), force


def periodic_case(name, res, stencil_name, dt, scheme, operator, seed):
    if not wanted(name):
        return
    ctx = lt.Context(device="cpu", dtype=DT[dt], use_native=False)
    tau, constant = (TAU, 0.0) if operator == "bgk" else (0.51, 1.0)

    def fresh():
        return noisy_tgv(ctx, res, getattr(lt, stencil_name)(), seed)

    flow = fresh()
    d = flow.stencil.d
    acceleration = list(ACCELERATION[:d])
    f0 = npy(flow.f)
    collision, force = make_collision(scheme, operator, flow, tau, tau, acceleration, constant)
    u0 = npy(flow.u(acceleration=force.acceleration))
    collided, snaps = collided_and_steps(flow, collision, SNAPSHOTS)
    assert np.isfinite(collided).all() and all(np.isfinite(v).all() for v in snaps.values())

    def gap(make):
        """(collided, f10) distance of the reference's result from that of a wrong operator"""
        other = fresh()
        c, s = collided_and_steps(other, make(other), (10,))
        return float(np.abs(c - collided).max()), float(np.abs(s[10] - snaps[10]).max())

    plain = {"bgk": lambda fl: lt.BGKCollision(tau),
             "smagorinsky": lambda fl: lt.SmagorinskyCollision(tau, constant)}[operator]
    wrong = {"no force": plain,
             "acceleration components reversed":
                 lambda fl: make_collision(scheme, operator, fl, tau, tau, acceleration[::-1], constant)[0]}
    subtle = {}
    if scheme == "guo" and operator == "bgk":
        wrong.update({
            "no velocity shift": lambda fl: lt.BGKCollision(tau, force=WrongGuo(fl, tau, acceleration, shift=0.0)),
            "shift of 1.0": lambda fl: lt.BGKCollision(tau, force=WrongGuo(fl, tau, acceleration, shift=1.0)),
            "source without its 1 - 1/(2 tau)":
                lambda fl: lt.BGKCollision(tau, force=WrongGuo(fl, tau, acceleration, factor=False)),
            "force.tau = 0.6": lambda fl: lt.BGKCollision(tau, force=lt.Guo(fl, 0.6, acceleration))})
        subtle = {"source at the unshifted velocity":
                      lambda fl: SourceAtUnshiftedVelocity(tau, force=lt.Guo(fl, tau, acceleration)),
                  "Shan-Chen for Guo": lambda fl: lt.BGKCollision(tau, force=lt.ShanChen(fl, tau, acceleration))}
    report = []
    for what, make in wrong.items():
        c, s = gap(make)
        report.append(f"{what} {c:.2e} / {s:.2e}")
        assert c >= 10 * ENGINE_F32 and s >= 100 * ENGINE_F32, f"{name}: '{what}' separates by {c:.2e} / {s:.2e} only"
    if dt == "f64":
        for what, make in subtle.items():
            c, s = gap(make)
            report.append(f"{what} {c:.2e} / {s:.2e}")
            assert c >= 10 * ENGINE_F64 and s >= 100 * ENGINE_F64, f"{name}: '{what}' separates by {c:.2e} / {s:.2e} only"
    print(f"  {name}: " + "; ".join(report))
    save(name, seed=np.int64(seed), f0=f0, collided=collided, u0=u0, tau=np.float64(tau), force_tau=np.float64(tau),
         constant=np.float64(constant), acceleration=np.array(acceleration, dtype=np.float64),
         ueq_scale=np.float64(force.ueq_scaling_factor),
         source_scale=np.float64(1 - 1 / (2 * tau) if scheme == "guo" else 0.0), noise=np.float64(NOISE),
         reynolds=np.float64(1600), mach=np.float64(0.1), resolution=np.array(flow.resolution),
         **{f"f{i}": v for i, v in snaps.items()})


def poiseuille_case(name, res, dt, reynolds, mach):
    if not wanted(name):
        return
    ctx = lt.Context(device="cpu", dtype=DT[dt], use_native=False)
    flow = quiet(lt.PoiseuilleFlow2D, ctx, list(res), reynolds, mach, lt.D2Q9())
    tau = flow.units.relaxation_parameter_lu
    f0 = npy(flow.f)
    force = lt.Guo(flow, tau, flow.acceleration)
    collision = lt.BGKCollision(tau, force=force)
    sim = quiet(lt.Simulation, flow, collision, [])
    snaps = {}
    for i in range(1, 11):
        quiet(sim, 1)
        if i in (1, 2, 10):
            snaps[i] = npy(flow.f)
    assert all(np.isfinite(v).all() for v in snaps.values())
    p, u = flow.analytic_solution()
    save(name, f0=f0, tau=np.float64(tau), acceleration=npy(flow.acceleration), resolution=np.array(flow.resolution),
         reynolds=np.float64(reynolds), mach=np.float64(mach),
         analytic_p=npy(p), analytic_u=npy(u), u10=npy(flow.u(acceleration=force.acceleration)),
         viscosity_pu=np.float64(flow.units.viscosity_pu), viscosity_lu=np.float64(flow.units.viscosity_lu),
         char_length_lu=np.float64(flow.units.characteristic_length_lu),
         u_char_lu=np.float64(flow.units.characteristic_velocity_lu),
         no_collision_mask=npy(sim.no_collision_mask),
         no_streaming_mask=np.packbits(npy(sim.no_streaming_mask).astype(bool), axis=None),
         no_streaming_mask_shape=np.array(sim.no_streaming_mask.shape),
         **{f"f{i}": v for i, v in snaps.items()})


CASES = (("guo", "bgk", "d2q9", "D2Q9", [12, 10]), ("guo", "bgk", "d3q15", "D3Q15", [10, 8, 6]),
         ("guo", "bgk", "d3q19", "D3Q19", [10, 8, 6]), ("guo", "bgk", "d3q27", "D3Q27", [6, 8, 6]),
         ("guo", "smagorinsky", "d2q9", "D2Q9", [12, 10]), ("guo", "smagorinsky", "d3q19", "D3Q19", [10, 8, 6]),
         ("shanchen", "bgk", "d2q9", "D2Q9", [12, 10]), ("shanchen", "bgk", "d3q19", "D3Q19", [10, 8, 6]))

if __name__ == "__main__":
    for seed, (scheme, operator, tag, stencil_name, res) in enumerate(CASES):
        for dt in ("f64", "f32"):
            periodic_case(f"force_{scheme}_{operator}_{tag}_{dt}", res, stencil_name, dt, scheme, operator, 3000 + seed)
    poiseuille_case("force_poiseuille2d_d2q9_f64", [16, 16], "f64", 10, 0.05)
