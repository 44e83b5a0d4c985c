"""Generate tests/golden/outlet_p_*.npz by running the REFERENCE's own PyTorch CPU path with its EquilibriumOutletP.

Build-container only, like tools/gen_golden_relaxations.py (whose way of importing the read-only reference checkout it
shares): only the arrays written here are committed.  Run:  python tools/gen_golden_outlet_p.py [substring ...]

The carrier is the reference's Obstacle (Re 100, Ma 0.05, domain_length_x 2; it exists in one, two and three
dimensions) with its `boundaries` replaced: an equilibrium inlet (1 pu towards the first outlet) on the face opposite
the first outlet, a bounce-back block of two nodes per axis in the middle of the grid, which touches no outlet plane,
and the outlets of the case.  The state is the Obstacle's own with 5 % multiplicative noise per population (seeded).
Every file holds
  f0, collided (Simulation._collide alone: collision, then the boundaries in index order), f1, f2, f6
  no_collision_mask, no_streaming_mask (packed bits) and no_streaming_mask_shape
  boundary_order (class names), boundary_direction and rho_outlet (0 where the class has none) per boundary, IN THE
      ORDER THE REFERENCE USED: among objects of one class Simulation sorts by the default repr, i.e. by address, and
      with several outlets the order changes the result
  inlet_mask, inlet_velocity_pu, block_mask, tau, resolution, collision and what the carrier was built from
Cases:
  outlet_p_<lat>_<axis><p|m>_r<100|102>_<dt>   one outlet on each axis and side, rho_outlet 1.0 and 1.02: D1Q3 [16],
                                               D2Q9 [12, 10], D3Q15 and D3Q19 [10, 8, 6], D3Q27 [6, 8, 6]
  outlet_p_three_<lat>_<dt>                    pressure outlets on +x, +y, -y (two axes): D2Q9, D3Q19
  outlet_p_mixed_<lat>_<dt>                    anti-bounce-back on +x, pressure outlets on +y and -y: D2Q9, D3Q19
  outlet_p_axes_d3q27_<dt>                     pressure outlets on +x, +y and +z (planes meeting in a corner)
  outlet_p_row_d3q19_f32, outlet_p_row_d2q9_*  the outlet's normal along the contiguous axis, rows of one whole wave:
                                               D3Q19 [4, 5, 64] outlet +z, D2Q9 [5, 64] outlet +y
  outlet_p_kbc_d3q27_f64, outlet_p_smagorinsky_d3q19_f32   one case each with another collision, outlet +x
  outlet_p_block_d2q9_f64                      THE EXCEPTION: the block reaches the outlet plane (+x), which pins that
                                               the outlet overwrites a bounce-back node
Before a file is written the generator ASSERTS that everything is finite and that f6 differs from the same run with an
anti-bounce-back outlet in place of every pressure outlet, and from the same run with every rho_outlet raised by 0.02,
by at least 100 times the engine tests' fp32 bound (1e-5).  A fixture that does not separate is not written (the
generator says so and goes on).
"""
import contextlib
import io
import os
import sys
import types
import warnings

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
warnings.filterwarnings("ignore", message="Using a non-tuple sequence")     # the reference's list indices
torch.set_num_threads(8)
DT = {"f64": torch.float64, "f32": torch.float32}
SNAPSHOTS = (1, 2, 6)
NOISE, REYNOLDS, MACH, LENGTH_X = 0.05, 100, 0.05, 2
ENGINE_F32 = 1e-5       # the engine tests' fp32 bound
SMAGORINSKY_TAU, KBC_TAU = 0.55, 0.55     # (KBC runs at the flow's own tau whatever it is given; the file says which)
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


def unit(d, axis, side):
    v = [0] * d
    v[axis] = side
    return v


def make_flow(ctx, res, stencil, seed, outlets, block_to_plane):
    """outlets: [(kind, direction, rho_outlet)], kind 'p' (EquilibriumOutletP) or 'a' (AntiBounceBackOutlet)"""
    d = len(res)
    first = outlets[0][1]
    axis = [i for i, c in enumerate(first) if c][0]
    inlet_mask = torch.zeros(res, dtype=torch.bool)
    index = [slice(None)] * d
    index[axis] = 0 if first[axis] > 0 else res[axis] - 1
    inlet_mask[tuple(index)] = True
    velocity = [float(c) for c in first]           # 1 pu = the characteristic velocity, towards the first outlet
    block = torch.zeros(res, dtype=torch.bool)
    where = [slice(n // 2 - 1, n // 2 + 1) for n in res]
    if block_to_plane:                             # the exception: up to and including the first outlet's plane
        where[axis] = slice(res[axis] // 2 - 1, res[axis]) if first[axis] > 0 else slice(0, res[axis] // 2 + 1)
    block[tuple(where)] = True

    class Carrier(lt.Obstacle):
        made = None

        @property
        def boundaries(self):
            if self.made is None:
                outs = [lt.EquilibriumOutletP(list(v), self, rho_outlet=rho) if kind == "p"
                        else lt.AntiBounceBackOutlet(list(v), self) for kind, v, rho in outlets]
                self.made = ([lt.EquilibriumBoundaryPU(self.context, inlet_mask, velocity)] + outs
                             + [lt.BounceBackBoundary(block)])
            return self.made

    flow = quiet(Carrier, ctx, list(res), REYNOLDS, MACH, LENGTH_X, stencil=stencil)
    g = torch.Generator().manual_seed(seed)
    factor = 1 + NOISE * (2 * torch.rand(flow.f.shape, generator=g, dtype=torch.float64) - 1)
    flow.f = (flow.f.double() * factor).to(ctx.dtype)
    return flow, inlet_mask, velocity, block


def make_collision(flow, collision):
    if collision == "kbc":
        return lt.KBCCollision(KBC_TAU), KBC_TAU
    if collision == "smagorinsky":
        return lt.SmagorinskyCollision(SMAGORINSKY_TAU), SMAGORINSKY_TAU
    tau = float(flow.units.relaxation_parameter_lu)
    return lt.BGKCollision(tau), tau


def run(ctx, res, stencil_name, seed, outlets, collision, block_to_plane):
    flow, inlet_mask, velocity, block = make_flow(ctx, res, getattr(lt, stencil_name)(), seed, outlets, block_to_plane)
    operator, _ = make_collision(flow, collision)
    sim = quiet(lt.Simulation, flow, operator, [])
    f0 = flow.f.clone()
    out = {"f0": npy(f0), "collided": npy(sim._collide())}
    flow.f = f0.clone()
    for i in range(1, max(SNAPSHOTS) + 1):
        quiet(sim, 1)
        if i in SNAPSHOTS:
            out[f"f{i}"] = npy(flow.f)
    tau = float(operator.tau)          # what ran: the reference's KBC takes the flow's tau on its first call
    return flow, sim, tau, inlet_mask, velocity, block, out


def case(name, res, stencil_name, dt, outlets, seed, collision="bgk", block_to_plane=False):
    if not wanted(name):
        return
    ctx = lt.Context(device="cpu", dtype=DT[dt], use_native=False)
    flow, sim, tau, inlet_mask, velocity, block, out = run(ctx, res, stencil_name, seed, outlets, collision,
                                                           block_to_plane)
    if not all(np.isfinite(v).all() for v in out.values()):
        print(f"  {name}: NOT WRITTEN, not finite")
        return
    wrong = {"anti-bounce-back outlets instead": [("a", v, rho) for kind, v, rho in outlets],
             "rho_outlet + 0.02": [(kind, v, rho + 0.02) for kind, v, rho in outlets]}
    report = []
    for what, others in wrong.items():
        other = run(ctx, res, stencil_name, seed, others, collision, block_to_plane)[-1]
        gap = float(np.abs(other["f6"] - out["f6"]).max())
        report.append(f"{what} {gap:.2e}")
        if not gap >= 100 * ENGINE_F32:
            print(f"  {name}: NOT WRITTEN, '{what}' separates by {gap:.2e} only")
            return
    print(f"  {name}: " + "; ".join(report))
    d = len(res)
    kinds, dirs, rhos = [], [], []
    for b in sim.boundaries[1:]:
        kinds.append(type(b).__name__)
        # the reference's outlets keep `index` (-1 / 0 on their axis, slices elsewhere), not the direction
        index = getattr(b, "index", None)
        dirs.append([0] * d if index is None else [0 if isinstance(i, slice) else (1 if i == -1 else -1) for i in index])
        rhos.append(float(b.rho_outlet) if hasattr(b, "rho_outlet") else 0.0)
    save(name, seed=np.int64(seed), tau=np.float64(tau), collision=np.array(collision),
         reynolds=np.float64(REYNOLDS), mach=np.float64(MACH), domain_length_x=np.float64(LENGTH_X),
         noise=np.float64(NOISE), resolution=np.array(flow.resolution),
         boundary_order=np.array(kinds), boundary_direction=np.array(dirs), rho_outlet=np.array(rhos, dtype=np.float64),
         inlet_mask=npy(inlet_mask), inlet_velocity_pu=np.array(velocity, dtype=np.float64), block_mask=npy(block),
         no_collision_mask=npy(sim.no_collision_mask),
         no_streaming_mask=np.packbits(npy(sim.no_streaming_mask).astype(bool), axis=None),
         no_streaming_mask_shape=np.array(sim.no_streaming_mask.shape), **out)


SINGLE = (("d1q3", "D1Q3", [16]), ("d2q9", "D2Q9", [12, 10]), ("d3q15", "D3Q15", [10, 8, 6]),
          ("d3q19", "D3Q19", [10, 8, 6]), ("d3q27", "D3Q27", [6, 8, 6]))
BOTH = ("f64", "f32")


def P(d, axis, side, rho):
    return ("p", unit(d, axis, side), rho)


if __name__ == "__main__":
    seed = 5000
    for tag, stencil_name, res in SINGLE:
        d = len(res)
        for axis in range(d):
            for side in (1, -1):
                for rho in (1.0, 1.02):
                    for dt in BOTH:
                        seed += 1
                        case(f"outlet_p_{tag}_{'xyz'[axis]}{'p' if side > 0 else 'm'}_r{round(100 * rho)}_{dt}", res,
                             stencil_name, dt, [P(d, axis, side, rho)], seed)
    for tag, stencil_name, res in (("d2q9", "D2Q9", [12, 10]), ("d3q19", "D3Q19", [10, 8, 6])):
        d = len(res)
        for dt in BOTH:
            seed += 1
            case(f"outlet_p_three_{tag}_{dt}", res, stencil_name, dt,
                 [P(d, 0, 1, 1.0), P(d, 1, 1, 1.02), P(d, 1, -1, 0.99)], seed)
            seed += 1
            case(f"outlet_p_mixed_{tag}_{dt}", res, stencil_name, dt,
                 [("a", unit(d, 0, 1), 0.0), P(d, 1, 1, 1.02), P(d, 1, -1, 1.0)], seed)
    for dt in BOTH:
        seed += 1
        case(f"outlet_p_axes_d3q27_{dt}", [6, 8, 6], "D3Q27", dt, [P(3, 0, 1, 1.0), P(3, 1, 1, 1.02), P(3, 2, 1, 0.99)],
             seed)
    case("outlet_p_row_d3q19_f32", [4, 5, 64], "D3Q19", "f32", [P(3, 2, 1, 1.02)], 5901)
    case("outlet_p_row_d2q9_f32", [5, 64], "D2Q9", "f32", [P(2, 1, 1, 1.02)], 5902)
    case("outlet_p_row_d2q9_f64", [5, 64], "D2Q9", "f64", [P(2, 1, 1, 1.02)], 5903)
    case("outlet_p_kbc_d3q27_f64", [6, 8, 6], "D3Q27", "f64", [P(3, 0, 1, 1.02)], 5904, collision="kbc")
    case("outlet_p_smagorinsky_d3q19_f32", [10, 8, 6], "D3Q19", "f32", [P(3, 0, 1, 1.02)], 5905, collision="smagorinsky")
    case("outlet_p_block_d2q9_f64", [12, 10], "D2Q9", "f64", [P(2, 0, 1, 1.02)], 5906, block_to_plane=True)
