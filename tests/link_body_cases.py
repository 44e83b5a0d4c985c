"""What tests/test_gpu_link_bodies_vs_cpu.py and its host companion tests/test_link_bodies_host.py share: the table from
the kernels' collision number to the mirror's operator, the engine plan and the relaxation time; the cases (lattices,
shapes, bodies, scenes of a body among other boundaries); and the reference, the mirror's own torch path
(``lt.Simulation`` on a CPU context, ``use_native=False``) in fp64 and, for the fp32 gate, in fp32 from the same state.
Every reference is computed once, shared, and handed out as a read-only array."""
import functools
import warnings

import numpy as np
import torch

import lettuce_amd as lt
import test_gpu_equilibria as equilibria
import test_gpu_force as force
import test_gpu_mrt as mrt
import test_gpu_relaxations as relaxations
from conftest import TORCH_DT
from test_gpu_link_bounce_back import body_of
from test_gpu_paths_vs_oracle import perturbed_state
from test_gpu_tune3_vs_cpu import INCOMPRESSIBLE, SMAGORINSKY_CONSTANT, _transform, make_plan, tau_of
from test_host_api import UniformFlow
from test_link_bounce_back_host import STENCIL, random_fractions
from test_mrt_host import make_collision, rates_of
from test_tune3_census import COLLISIONS

SEED = 3
FACTOR = 4.0                   # fp32: E_gpu <= FACTOR * E_ref (tests/test_gpu_fp32_error_budget.py)
SHAPES = [("D2Q9", (5, 67)), ("D2Q9", (12, 10)), ("D3Q15", (6, 5, 7)), ("D3Q19", (6, 5, 67)), ("D3Q27", (4, 4, 4)),
          ("D3Q27", (6, 5, 7))]
BODIES = ("block", "sphere")
RUNS = (1, 4)
FORCED = {5: "bgk", 7: "smagorinsky"}


def shape_id(lat, res):
    return f"{lat.lower()}-{'x'.join(map(str, res))}"


# ------------------------------------------------------------------------------------------------- the collisions
def variants():
    """(collision number, force scheme or None) of every kernel family: Shan-Chen beside Guo for 5 and 7"""
    out = []
    for coll in sorted(COLLISIONS):
        out.append((coll, "guo" if coll in FORCED else None))
        if coll in FORCED:
            out.append((coll, "shanchen"))
    return out


def units_of(coll):
    return {lat.upper() for lat in COLLISIONS[coll] if lat != "d1q3"}


def acceleration_of(coll, d):
    if coll in FORCED:
        return list(force.ACCELERATION[:d])
    return [equilibria.ACCELERATION] + [0.0] * (d - 1)


def mirror_operator(coll, scheme, lat, flow):
    """the mirror's operator of the kernels' collision number on `flow` (which carries the incompressible equilibrium
    for 17 .. 25)"""
    tau = tau_of(coll)
    if coll == 0:
        return lt.NoCollision()
    if coll == 1:
        return lt.BGKCollision(tau)
    if coll == 2:
        collision = lt.KBCCollision()
        collision.native_generator().tau(flow)          # the first use takes the flow's tau and the beta of it ...
        collision.tau, collision.beta = tau, 1.0 / (2.0 * tau)      # ... which an assignment replaces
        return collision
    if coll == 3:
        return lt.SmagorinskyCollision(tau, SMAGORINSKY_CONSTANT)
    if coll in FORCED:
        term = {"guo": lt.Guo, "shanchen": lt.ShanChen}[scheme](flow, tau, acceleration_of(coll, flow.stencil.d))
        if coll == 5:
            return lt.BGKCollision(tau, force=term)
        return lt.SmagorinskyCollision(tau, force.SCHEMES[("guo", "smagorinsky")][1], force=term)
    if coll in (8, 9):
        return relaxations.cpu_collision({8: "trt", 9: "regularized"}[coll], flow)
    if coll in (10, 11):
        transform = _transform(coll, lat)
        return make_collision(transform, flow.context, rates_of(transform, mrt.TAU), flow.stencil)
    return equilibria.cpu_collision(INCOMPRESSIBLE[coll], flow)


def engine_plan(coll, scheme, lat, dt, res, entries):
    """the plan of the collision number through `make_plan`; Shan-Chen: the same plan with that scheme's scales"""
    plan = make_plan(coll, lat, dt, list(res), list(entries))
    if scheme == "shanchen":
        plan.set_force(acceleration_of(coll, len(res)), *force.scales("shanchen", tau_of(coll)))
    plan.set_two_step(0)
    if len(res) == 2:
        plan.set_many_step(0)
    return plan


COLLISION = {(coll, scheme): (functools.partial(mirror_operator, coll, scheme), functools.partial(engine_plan, coll, scheme),
                              tau_of(coll)) for coll, scheme in variants()}


# ------------------------------------------------------------------------------------------------- states and flows
def state(lat, res, dt):
    """perturbed_state(lat, res, dtype, 3): no symmetries, a non-zero mean velocity, every moment resolved"""
    return perturbed_state(lat, list(res), TORCH_DT[dt], SEED)


def weights(lat):
    return np.asarray(STENCIL[lat]().w, dtype=np.float64)


def weighted_error(lat, got, want):
    """max over q and nodes of |got - want| / w_q"""
    err = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64))
    return float((err.reshape(len(weights(lat)), -1).max(axis=1) / weights(lat)).max())


def cpu_flow(lat, res, dtype, coll=1, reynolds=1, mach=0.01):
    context = lt.Context("cpu", dtype, use_native=False)
    equilibrium = lt.IncompressibleQuadraticEquilibrium(equilibria.RHO0) if coll in INCOMPRESSIBLE else None
    return UniformFlow(context, list(res), reynolds, mach, STENCIL[lat](), equilibrium)


def frozen(array):
    array = np.ascontiguousarray(array)
    array.setflags(write=False)
    return array


def body(lat, res, kind):
    mask, fractions = body_of(lat, list(res), kind)
    return lt.InterpolatedBounceBackBoundary(mask, fractions)


def link_census(lat, res, boundary):
    """(links, links with d >= 1/2, distinct directions) of a body's list"""
    links = boundary.links(STENCIL[lat](), torch.float64)
    return len(links), int(links.second.sum()), len(set(links.direction.tolist()))


@functools.lru_cache(maxsize=None)
def reference(lat, res, dt, coll, scheme, kind, run):
    """part A: {"collide": after the collision and the body's rule, 1: after one step, 4: after four} of the mirror's
    torch path in the dtype `run` from the state of dtype `dt`, the body the only boundary; float64 arrays"""
    f0 = state(lat, res, dt)

    def fresh():
        flow = cpu_flow(lat, res, TORCH_DT[run], coll)
        flow.boundaries = [body(lat, res, kind)]
        flow.f = f0.to(TORCH_DT[run]).clone()
        return flow, lt.Simulation(flow, mirror_operator(coll, scheme, lat, flow), [])

    out = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        flow, sim = fresh()
        out["collide"] = frozen(sim._collide().double().numpy().copy())
        flow, sim = fresh()
        done = 0
        for n in RUNS:
            sim(n - done)
            done = n
            assert flow.f.dtype == TORCH_DT[run]
            out[n] = frozen(flow.f.double().numpy().copy())
    return out


def part_a_cases():
    """(collision number, scheme, lattice, resolution, body) of every family in every unit that has it"""
    return [(coll, scheme, lat, res, kind) for coll, scheme in variants() for lat, res in SHAPES if lat in units_of(coll)
            for kind in BODIES]


def part_a_id(case):
    coll, scheme, lat, res, kind = case
    return f"coll{coll}{'-' + scheme if scheme else ''}-{shape_id(lat, res)}-{kind}"


# part C: one body per 2-D / 3-D unit under BGK, KBC on D3Q27 (fp32: the _occ4 kernel) and one MRT plan
PART_C = ([(1, None, lat, res, "block", dt) for lat, res in (SHAPES[0], SHAPES[2], SHAPES[3], SHAPES[5]) for dt in ("f32", "f64")]
          + [(2, None, "D3Q27", (6, 5, 7), "sphere", "f32"), (10, None, "D2Q9", (12, 10), "sphere", "f64")])
GRAPH_STEPS = 1 + 70           # one collide, 70 fused steps (two replayed chunks of 32 and six eager ones), one stream


def part_c_id(case):
    return f"{part_a_id(case[:5])}-{case[5]}"


@functools.lru_cache(maxsize=None)
def long_reference(lat, res, dt, coll, scheme, kind, steps=GRAPH_STEPS):
    """the mirror's fp64 populations after `steps` steps (part C replays graphs over that many)"""
    flow = cpu_flow(lat, res, torch.float64, coll)
    flow.boundaries = [body(lat, res, kind)]
    flow.f = state(lat, res, dt).double().clone()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        lt.Simulation(flow, mirror_operator(coll, scheme, lat, flow), [])(steps)
    return frozen(flow.f.numpy().copy())


# ------------------------------------------------------------------------------------------------- part B: scenes
# A scene: (lattice, resolution, collision, boundaries in index order).  A boundary is ("body", seed of its fractions,
# first node), ("inlet",) -- the face x = 0 --, ("wall", nodes), ("abb", axis, side) or ("pout", axis, side, rho).
RHO_OUTLET = 1.02
TAU_MINUS = 2.5
SCENE_ACCELERATION = (2e-3, -3e-3, 1e-3)
SMALL = {"D2Q9": (12, 10), "D3Q15": (7, 6, 8), "D3Q19": (7, 6, 8), "D3Q27": (7, 6, 8)}
ROW = {"D2Q9": (5, 64), "D3Q15": (4, 6, 64), "D3Q19": (4, 6, 64), "D3Q27": (4, 6, 64)}


def _first_node(res, planes):
    """the first node of a block of two nodes along the last axis that stays two nodes clear of the boundary planes
    `planes` = [(axis, side)] (side -1: the plane 0, +1: the plane n - 1), else in the middle"""
    d = len(res)
    at = []
    for axis, n in enumerate(res):
        length = 2 if axis == d - 1 else 1
        if (axis, -1) in planes and (axis, 1) in planes:
            raise ValueError("a body between two planes of one axis")
        if (axis, -1) in planes:
            at.append(n - 2 - length)
        elif (axis, 1) in planes:
            at.append(2)
        else:
            at.append(n // 2 - (length - 1))
    return tuple(at)


def _scene(cid, lat, res, collision, *boundaries):
    planes = [(0, -1) if b[0] == "inlet" else (b[1], b[2]) for b in boundaries if b[0] in ("inlet", "abb", "pout")]
    first = _first_node(res, planes)
    seeds = iter((41, 43, 47))
    made = []
    for b in boundaries:
        if b[0] == "body":
            shift = b[1] if len(b) > 1 else tuple(0 for _ in res)
            made.append(("body", next(seeds), tuple(f + s for f, s in zip(first, shift))))
        else:
            made.append(b)
    return cid, lat, tuple(res), collision, tuple(made)


def _wall(res):
    return ("wall", tuple([1] + [0] * (len(res) - 1)))


def _scenes():
    out = []
    # (a) a full-way wall and an equilibrium inlet; the body's index lowest, in the middle, highest
    for lat in ("D2Q9", "D3Q15", "D3Q19", "D3Q27"):
        res = SMALL[lat]
        others = [("inlet",), _wall(res)]
        for name, at in (("lowest", 0), ("middle", 1), ("highest", 2)):
            boundaries = others[:at] + [("body",)] + others[at:]
            out.append(_scene(f"a-{lat.lower()}-bgk-body-{name}", lat, res, "bgk", *boundaries))
    for lat, collision in (("D3Q27", "kbc"), ("D3Q19", "trt"), ("D2Q9", "guo")):
        out.append(_scene(f"a-{lat.lower()}-{collision}-body-middle", lat, SMALL[lat], collision, ("inlet",), ("body",),
                          _wall(SMALL[lat])))
    # (b) one anti-bounce-back outlet on each axis and side; the body's index below and above the outlet's; the
    # contiguous axis with 64 nodes along it (the kernels' abb0_slot)
    for lat in ("D2Q9", "D3Q15", "D3Q19", "D3Q27"):
        d = len(SMALL[lat])
        faces = [(axis, side, SMALL[lat]) for axis in range(d) for side in (1, -1)] + [(d - 1, 1, ROW[lat]), (d - 1, -1, ROW[lat])]
        for axis, side, res in faces:
            face = f"{'xyz'[axis]}{'+' if side > 0 else '-'}{'-row' if res == ROW[lat] else ''}"
            for name, boundaries in (("below", [("body",), ("abb", axis, side)]), ("above", [("abb", axis, side), ("body",)])):
                out.append(_scene(f"b-{lat.lower()}-bgk-{face}-body-{name}", lat, res, "bgk", *boundaries))
    for lat, collision in (("D2Q9", "kbc"), ("D3Q27", "trt"), ("D3Q19", "guo")):
        d = len(SMALL[lat])
        out.append(_scene(f"b-{lat.lower()}-{collision}-row-body-below", lat, ROW[lat], collision, ("body",), ("abb", d - 1, 1)))
        out.append(_scene(f"b-{lat.lower()}-{collision}-x+-body-above", lat, SMALL[lat], collision, ("abb", 0, 1), ("body",)))
    # (c) two and three outlets on different axes, one of them of constant pressure
    out.append(_scene("c-d2q9-abb-pout", "D2Q9", SMALL["D2Q9"], "bgk", ("abb", 0, 1), ("body",), ("pout", 1, -1, RHO_OUTLET)))
    out.append(_scene("c-d2q9-two-abb", "D2Q9", SMALL["D2Q9"], "bgk", ("body",), ("abb", 0, 1), ("abb", 1, 1)))
    for lat in ("D3Q15", "D3Q19", "D3Q27"):
        res = SMALL[lat]
        out.append(_scene(f"c-{lat.lower()}-two-abb-pout", lat, res, "bgk", ("abb", 0, 1), ("abb", 1, -1), ("body",),
                          ("pout", 2, 1, RHO_OUTLET)))
        out.append(_scene(f"c-{lat.lower()}-three-abb", lat, res, "bgk", ("abb", 0, -1), ("body",), ("abb", 1, 1), ("abb", 2, -1)))
        out.append(_scene(f"c-{lat.lower()}-abb-pout", lat, res, "bgk", ("body",), ("pout", 0, 1, RHO_OUTLET), ("abb", 2, 1)))
    # (d) two bodies, different fractions
    for lat in ("D2Q9", "D3Q19"):
        res = SMALL[lat]
        away = tuple([-4 if lat == "D2Q9" else 0] + [0] * (len(res) - 2) + [0 if lat == "D2Q9" else -4])
        out.append(_scene(f"d-{lat.lower()}-two-bodies", lat, (16, 10) if lat == "D2Q9" else (7, 6, 12), "bgk", ("body",),
                          ("body", away)))
        out.append(_scene(f"d-{lat.lower()}-two-bodies-and-an-outlet", lat, (16, 10) if lat == "D2Q9" else (7, 6, 12), "bgk",
                          ("body",), ("abb", 1, 1), ("body", away)))
    # (e) MRT with a pressure outlet
    out.append(_scene("e-d2q9-dellar-pout", "D2Q9", SMALL["D2Q9"], "dellar", ("body",), ("pout", 0, 1, RHO_OUTLET)))
    out.append(_scene("e-d2q9-lallemand-pout", "D2Q9", SMALL["D2Q9"], "lallemand", ("pout", 1, -1, RHO_OUTLET), ("body",)))
    out.append(_scene("e-d3q27-hermite-pout", "D3Q27", SMALL["D3Q27"], "hermite", ("body",), ("pout", 2, 1, RHO_OUTLET)))
    return out


SCENES = {s[0]: s for s in _scenes()}
SCENE_STEPS = (1, 4)
SCENE_TAU = 0.8


def _ordered(cls, position):
    """among objects Simulation sorts by str(): the position is chosen, not left to class names"""
    class Ordered(cls):
        def __str__(self):
            return f"boundary-{position:03d}"
    Ordered.__name__ = cls.__name__
    return Ordered


def scene_body_mask(res, first):
    solid = torch.zeros(list(res), dtype=torch.bool)
    solid[first] = True
    solid[tuple(f + (1 if a == len(res) - 1 else 0) for a, f in enumerate(first))] = True
    return solid


def scene_flow(cid, context, f0=None):
    """the mirror's flow of a scene on `context` with its boundaries (listed in reverse: str() decides), populations
    `f0` (default: the state of the context's dtype); its relaxation time is SCENE_TAU"""
    _, lat, res, _, boundaries = SCENES[cid]
    stencil = STENCIL[lat]()
    mach = 0.05
    reynolds = res[0] * mach / np.sqrt(3.0) / ((SCENE_TAU - 0.5) / 3.0)
    flow = UniformFlow(context, list(res), reynolds, mach, stencil)
    made = []
    for position, b in enumerate(boundaries):
        if b[0] == "body":
            fractions = random_fractions(lat, tuple(res), seed=b[1])
            made.append(_ordered(lt.InterpolatedBounceBackBoundary, position)(scene_body_mask(res, b[2]), fractions))
        elif b[0] == "inlet":
            mask = torch.zeros(list(res), dtype=torch.bool)
            mask[0] = True
            velocity = [1.0] + [0.0] * (stencil.d - 1)
            made.append(_ordered(lt.EquilibriumBoundaryPU, position)(context, context.convert_to_tensor(mask, dtype=torch.bool),
                                                                    velocity))
        elif b[0] == "wall":
            mask = torch.zeros(list(res), dtype=torch.bool)
            mask[tuple(slice(c, c + 2) if a else slice(c, c + 1) for a, c in enumerate(b[1]))] = True
            made.append(_ordered(lt.BounceBackBoundary, position)(context.convert_to_tensor(mask, dtype=torch.bool)))
        else:
            direction = [0] * stencil.d
            direction[b[1]] = b[2]
            if b[0] == "abb":
                made.append(_ordered(lt.AntiBounceBackOutlet, position)(direction, flow))
            else:
                made.append(_ordered(lt.EquilibriumOutletP, position)(direction, flow, rho_outlet=b[3]))
    flow.boundaries = made[::-1]
    dt = "f32" if context.dtype == torch.float32 else "f64"
    flow.f = context.convert_to_tensor((state(lat, res, dt) if f0 is None else f0).clone(), dtype=context.dtype)
    return flow


def scene_collision(cid, flow):
    _, lat, _, collision, _ = SCENES[cid]
    tau = SCENE_TAU
    if collision == "bgk":
        return lt.BGKCollision(tau)
    if collision == "kbc":
        return lt.KBCCollision()                      # takes the flow's relaxation time, SCENE_TAU
    if collision == "trt":
        return lt.TRTCollision(tau, TAU_MINUS)
    if collision == "guo":
        return lt.BGKCollision(tau, force=lt.Guo(flow, tau, list(SCENE_ACCELERATION[:flow.stencil.d])))
    return make_collision(collision, flow.context, rates_of(collision, mrt.TAU), flow.stencil)


def scene_simulation(cid, context, f0=None, reporter=()):
    flow = scene_flow(cid, context, f0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        simulation = lt.Simulation(flow, scene_collision(cid, flow), list(reporter))
    kinds = [b[0] for b in SCENES[cid][4]]
    names = {"body": "InterpolatedBounceBackBoundary", "inlet": "EquilibriumBoundaryPU", "wall": "BounceBackBoundary",
             "abb": "AntiBounceBackOutlet", "pout": "EquilibriumOutletP"}
    assert [type(b).__name__ for b in simulation.boundaries[1:]] == [names[k] for k in kinds]
    return flow, simulation


def scene_plan(cid, dt):
    """(the engine plan of a scene with its masks and link lists, built from the mirror's boundaries on a CPU context,
    the relaxation time of its calls)"""
    from lettuce_amd._native import Plan
    _, lat, res, collision, _ = SCENES[cid]
    flow, simulation = scene_simulation(cid, lt.Context("cpu", TORCH_DT[dt], use_native=False))
    entries = [b.native_generator(i).plan_entry(flow) for i, b in enumerate(simulation.boundaries[1:], start=1)]
    if collision in mrt.LATTICE:
        plan = mrt.mrt_plan(collision, dt, list(res), entries=entries)
    else:
        plan = Plan(lat, TORCH_DT[dt], "bgk" if collision == "guo" else collision, list(res), entries)
        if collision == "trt":
            plan.set_trt(TAU_MINUS)
        if collision == "guo":
            plan.set_force(list(SCENE_ACCELERATION[:len(res)]), *force.scales("guo", SCENE_TAU))
    for index, b in enumerate(simulation.boundaries[1:], start=1):
        if isinstance(b, lt.InterpolatedBounceBackBoundary):
            links = lt.native_link_list(b, index, simulation.no_collision_mask, flow.stencil, TORCH_DT[dt])
            assert plan.set_links(index - 1, *links) == len(links[0]) > 0
    plan.set_masks(simulation.no_collision_mask.cuda(), simulation.no_streaming_mask.to(torch.uint8).cuda())
    plan.set_two_step(0)
    if len(res) == 2:
        plan.set_many_step(0)
    return plan, float(flow.units.relaxation_parameter_lu) if collision == "kbc" else SCENE_TAU


@functools.lru_cache(maxsize=None)
def scene_reference(cid, dt, run):
    """{n: populations after n steps} of the mirror's torch path in the dtype `run` from the state of dtype `dt`"""
    _, lat, res, _, _ = SCENES[cid]
    context = lt.Context("cpu", TORCH_DT[run], use_native=False)
    flow, simulation = scene_simulation(cid, context, state(lat, res, dt).to(TORCH_DT[run]))
    out, done = {}, 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for n in SCENE_STEPS:
            simulation(n - done)
            done = n
            out[n] = frozen(flow.f.double().numpy().copy())
    return out
