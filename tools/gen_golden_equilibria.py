"""Generate tests/golden/incompressible_*.npz and lessmemory_*.npz by running the REFERENCE's own PyTorch CPU path.

Build-container only, like tools/gen_golden_relaxations.py (whose way of importing the read-only reference checkout, noisy
Taylor-Green state and size cap it shares): only the arrays written here are committed.
Run:  python tools/gen_golden_equilibria.py [substring ...]

The reference's IncompressibleQuadraticEquilibrium cannot be instantiated as shipped (it lacks native_available and
native_generator); the subclass below adds the two methods and nothing else, its __call__ is the reference's.

Periodic files, incompressible_<op>_<lat>_<dt> with rho0 = 1.1 on D2Q9 [12, 10], D3Q15 and D3Q19 [10, 8, 6], D3Q27
[6, 8, 6], fp32 and fp64, Taylor-Green vortex (Re 1600, Ma 0.1):
  bgk          BGKCollision(0.8)
  trt          TRTCollision(0.8, 3.0)
  regularized  RegularizedCollision() at the flow's own tau
  guo          BGKCollision(0.8, force=Guo(flow, 0.8, [1e-4, 0, ...]))
Each holds finit (the flow's own initial populations: Flow.initialize with initialize_f_neq), f0 (finit with 5 %
multiplicative noise per population, seeded), feq = equilibrium(flow) of the noisy state, the collided field, f after 1,
2, 3 and 10 steps, rho0 and the scalars.
Masked files, incompressible_obstacle_<lat>_<dt>: the reference's Obstacle with a solid block (inlet, bounce-back,
anti-bounce-back outlet), the same equilibrium, BGK at the flow's tau, D2Q9 [32, 20] and D3Q19 [16, 12, 8].
lessmemory_bgk_d2q9_f64: QuadraticEquilibriumLessMemory (as shipped) under BGK.

Before a file is written the generator ASSERTS that the result differs from the wrong models on the same f0 -- the same
operator with QuadraticEquilibrium, and with rho0 = 1.0 -- by at least 10 times the engine tests' fp32 bound (1e-5) after
the collision and 100 times after 10 steps.  A fixture that does not separate is reported and not written.  It also
asserts that LessMemory equals QuadraticEquilibrium bit for bit on every state it makes, and prints the result.
"""
import numpy as np
import torch

from gen_golden_relaxations import lt, DT, SNAPSHOTS, NOISE, ENGINE_F32, CASES, wanted, quiet, npy, save

RHO0 = 1.1
TAU, TAU_MINUS, ACCELERATION = 0.8, 3.0, 1e-4
OPERATORS = ("bgk", "trt", "regularized", "guo")


class Incompressible(lt.IncompressibleQuadraticEquilibrium):
    """the reference's class made instantiable: the two abstract methods it lacks"""

    def native_available(self):
        return False

    def native_generator(self):
        return None


def make_collision(operator, flow):
    if operator == "bgk":
        return lt.BGKCollision(TAU)
    if operator == "trt":
        return lt.TRTCollision(TAU, TAU_MINUS)
    if operator == "regularized":
        return lt.RegularizedCollision()           # takes the flow's tau on its first call
    acceleration = [ACCELERATION] + [0.0] * (flow.stencil.d - 1)
    return lt.BGKCollision(TAU, force=lt.Guo(flow, TAU, acceleration))


def run(flow, operator, steps=SNAPSHOTS):
    collision = make_collision(operator, flow)
    collided = npy(collision(flow))
    sim = quiet(lt.Simulation, flow, collision, [])
    out = {}
    for i in range(1, max(steps) + 1):
        quiet(sim, 1)
        if i in steps:
            out[i] = npy(flow.f)
    return collided, out, collision


def tgv(ctx, res, stencil_name, equilibrium):
    return quiet(lt.TaylorGreenVortex, ctx, res, 1600, 0.1, getattr(lt, stencil_name)(), equilibrium)


def noise_factor(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return 1 + NOISE * (2 * torch.rand(shape, generator=g, dtype=torch.float64) - 1)


def less_memory_equals_quadratic(ctx, res, stencil_name, f0, operator):
    """bit for bit: feq, the collided field and 10 steps"""
    results = []
    for equilibrium in (lt.QuadraticEquilibrium(), lt.QuadraticEquilibriumLessMemory()):
        flow = tgv(ctx, res, stencil_name, equilibrium)
        flow.f = torch.tensor(f0)
        feq = npy(flow.equilibrium(flow))
        collided, snaps, _ = run(flow, operator, (10,))
        results.append((feq, collided, snaps[10]))
    return all(np.array_equal(a, b) for a, b in zip(*results))


def periodic_case(name, res, stencil_name, dt, operator, seed):
    if not wanted(name):
        return
    ctx = lt.Context(device="cpu", dtype=DT[dt], use_native=False)
    flow = tgv(ctx, res, stencil_name, Incompressible(RHO0))
    finit = npy(flow.f)
    flow.f = (flow.f.double() * noise_factor(flow.f.shape, seed)).to(ctx.dtype)
    f0 = npy(flow.f)
    feq = npy(flow.equilibrium(flow))
    own = float(flow.units.relaxation_parameter_lu)
    collided, snaps, collision = run(flow, operator)
    assert np.isfinite(collided).all() and all(np.isfinite(v).all() and (v > 0).all() for v in snaps.values())
    same = less_memory_equals_quadratic(ctx, res, stencil_name, f0, operator)
    print(f"  {name}: QuadraticEquilibriumLessMemory == QuadraticEquilibrium bit for bit: {same}")
    assert same
    report = []
    for what, equilibrium in (("QuadraticEquilibrium", lt.QuadraticEquilibrium()), ("rho0 = 1.0", Incompressible(1.0))):
        other = tgv(ctx, res, stencil_name, equilibrium)
        other.f = torch.tensor(f0)
        c, s, _ = run(other, operator, (10,))
        c, s = float(np.abs(c - collided).max()), float(np.abs(s[10] - snaps[10]).max())
        report.append(f"{what} {c:.2e} / {s:.2e}")
        if not (c >= 10 * ENGINE_F32 and s >= 100 * ENGINE_F32):
            print(f"  {name}: NOT WRITTEN, '{what}' separates by {c:.2e} / {s:.2e} only")
            return
    print(f"  {name}: " + "; ".join(report))
    tau = own if operator == "regularized" else TAU
    save(name, seed=np.int64(seed), finit=finit, f0=f0, feq=feq, collided=collided, rho0=np.float64(RHO0),
         tau=np.float64(tau), tau_minus=np.float64(TAU_MINUS if operator == "trt" else 0.0), flow_tau=np.float64(own),
         acceleration=np.float64(ACCELERATION if operator == "guo" else 0.0), noise=np.float64(NOISE),
         reynolds=np.float64(1600), mach=np.float64(0.1), resolution=np.array(flow.resolution),
         **{f"f{i}": v for i, v in snaps.items()})


def less_memory_case(name, res, stencil_name, dt, seed):
    if not wanted(name):
        return
    ctx = lt.Context(device="cpu", dtype=DT[dt], use_native=False)
    flow = tgv(ctx, res, stencil_name, lt.QuadraticEquilibriumLessMemory())
    finit = npy(flow.f)
    flow.f = (flow.f.double() * noise_factor(flow.f.shape, seed)).to(ctx.dtype)
    f0 = npy(flow.f)
    feq = npy(flow.equilibrium(flow))
    collided, snaps, _ = run(flow, "bgk")
    same = less_memory_equals_quadratic(ctx, res, stencil_name, f0, "bgk")
    print(f"  {name}: QuadraticEquilibriumLessMemory == QuadraticEquilibrium bit for bit: {same}")
    assert same
    save(name, seed=np.int64(seed), finit=finit, f0=f0, feq=feq, collided=collided, tau=np.float64(TAU),
         flow_tau=np.float64(flow.units.relaxation_parameter_lu), noise=np.float64(NOISE), reynolds=np.float64(1600),
         mach=np.float64(0.1), resolution=np.array(flow.resolution), **{f"f{i}": v for i, v in snaps.items()})


def obstacle(ctx, res, stencil, equilibrium, block):
    flow = quiet(lt.Obstacle, ctx, list(res), 100, 0.1, 4.0, stencil=stencil, equilibrium=equilibrium)
    mask = np.zeros(res, dtype=bool)
    mask[tuple(slice(a, b) for a, b in block)] = True
    flow.mask = mask
    quiet(flow.initialize)          # initial_pu depends on the mask (obstacle.py:94-99)
    return flow


def obstacle_run(flow, steps):
    collision = lt.BGKCollision(flow.units.relaxation_parameter_lu)
    sim = quiet(lt.Simulation, flow, collision, [])
    out = {}
    for i in range(1, max(steps) + 1):
        quiet(sim, 1)
        if i in steps:
            out[i] = npy(flow.f)
    return out, sim


def obstacle_case(name, res, stencil_name, dt, block):
    if not wanted(name):
        return
    ctx = lt.Context(device="cpu", dtype=DT[dt], use_native=False)
    flow = obstacle(ctx, res, getattr(lt, stencil_name)(), Incompressible(RHO0), block)
    f0 = npy(flow.f)
    snaps, sim = obstacle_run(flow, SNAPSHOTS)
    assert all(np.isfinite(v).all() for v in snaps.values())
    report = []
    for what, equilibrium in (("QuadraticEquilibrium", lt.QuadraticEquilibrium()), ("rho0 = 1.0", Incompressible(1.0))):
        other = obstacle(ctx, res, getattr(lt, stencil_name)(), equilibrium, block)
        s, _ = obstacle_run(other, (10,))
        gap = float(np.abs(s[10] - snaps[10]).max())
        report.append(f"{what} {gap:.2e}")
        if not gap >= 100 * ENGINE_F32:
            print(f"  {name}: NOT WRITTEN, '{what}' separates by {gap:.2e} only after 10 steps")
            return
    print(f"  {name}: after 10 steps " + "; ".join(report))
    names = [type(b).__name__ for b in sorted(flow.boundaries, key=lambda b: str(b))]
    save(name, f0=f0, rho0=np.float64(RHO0), tau=np.float64(flow.units.relaxation_parameter_lu),
         obstacle_mask=npy(flow.mask), block=np.array(block), boundary_order=np.array(names),
         domain_length_x=np.float64(4.0), reynolds=np.float64(100), mach=np.float64(0.1),
         resolution=np.array(flow.resolution), no_collision_mask=npy(sim.no_collision_mask),
         no_streaming_mask=np.packbits(npy(sim.no_streaming_mask).astype(bool), axis=None),
         no_streaming_mask_shape=np.array(sim.no_streaming_mask.shape), **{f"f{i}": v for i, v in snaps.items()})


if __name__ == "__main__":
    for seed, (tag, stencil_name, res) in enumerate(CASES):
        for dt in ("f64", "f32"):
            for k, operator in enumerate(OPERATORS):
                periodic_case(f"incompressible_{operator}_{tag}_{dt}", res, stencil_name, dt, operator, 5000 + 100 * k + seed)
    for dt in ("f64", "f32"):
        obstacle_case(f"incompressible_obstacle_d2q9_{dt}", [32, 20], "D2Q9", dt, [(6, 10), (8, 13)])
        obstacle_case(f"incompressible_obstacle_d3q19_{dt}", [16, 12, 8], "D3Q19", dt, [(3, 6), (4, 8), (2, 6)])
    less_memory_case("lessmemory_bgk_d2q9_f64", [12, 10], "D2Q9", "f64", 5900)
