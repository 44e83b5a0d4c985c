"""The momentum-exchange force on a bounce-back body on the host (CPU, no GPU needed): the torch path of
``lt.BoundaryForce`` against a restatement of its definition, the momentum balance of a periodic box, the drag and lift
coefficients, the plumbing of ``lt_boundary_force`` and the refusals.

The comparator is never the code under test: ``exact_force`` below restates the definition (fp64, CPU) -- per q,
``up = torch.roll(solid, e_q)`` and ``link = solid & ~up``; the terms 2 e_{q,c} f_q[link] are collected as Python floats
(2 f_q and the sign are exact) and the exact value is ``math.fsum(terms)`` per component.

Bound for every comparison of a sum with n terms (the bound of tests/test_jacobi_kernel_host.py, here for signed terms):
|got - fsum(terms)| <= (n - 1) * 2^-53 * fsum(|terms|); the output is cast to the context dtype, so fp32 adds half an
ulp of the result.  Nothing here takes a measured tolerance."""
import ctypes
import functools
import math
import os
import re

import numpy as np
import pytest
import torch

import lettuce_amd as lt
from conftest import ROOT, TORCH_DT
from test_host_api import ctx, UniformFlow

U = 2.0 ** -53
STENCIL = {"D1Q3": lt.D1Q3, "D2Q9": lt.D2Q9, "D3Q15": lt.D3Q15, "D3Q19": lt.D3Q19, "D3Q27": lt.D3Q27}
# extents 1 and 2 (below the stencil's reach), odd extents, a ragged grid of several workgroups
GRIDS = ([("D2Q9", r) for r in ([1, 4], [2, 2], [5, 3], [70, 67])]
         + [(lat, r) for lat in ("D3Q19", "D3Q27") for r in ([2, 3, 1], [6, 5, 67])] + [("D3Q15", [6, 5, 67])])
MASKS = ["none", "all", "isolated", "block", "checkerboard", "plate"]
CASES = [(lat, res, mask) for lat, res in GRIDS + [("D1Q3", [5])] for mask in MASKS]


def case_id(case):
    return f"{case[0].lower()}-{'x'.join(map(str, case[1]))}-{case[2]}"


def solid_mask(kind, res):
    """bool [*res]"""
    res = list(res)
    solid = torch.zeros(res, dtype=torch.bool)
    if kind == "all":
        solid[...] = True
    elif kind == "isolated":          # the corner (0, ..., 0), the last node and one in between: every axis wraps
        solid[tuple(0 for _ in res)] = True
        solid[tuple(n - 1 for n in res)] = True
        solid[tuple(n // 2 for n in res)] = True
    elif kind == "block":             # touches the low face of axis 0 and the high face of axis 1
        index = [slice(0, max(1, res[0] // 2))]
        if len(res) > 1:
            index.append(slice(res[1] - max(1, res[1] // 2), res[1]))
        if len(res) > 2:
            index.append(slice(res[2] // 4, max(res[2] // 4 + 1, res[2] // 2)))
        solid[tuple(index)] = True
    elif kind == "checkerboard":      # axis neighbours fluid, diagonal neighbours solid
        total = sum(torch.meshgrid(*[torch.arange(n) for n in res], indexing="ij"))
        solid = total % 2 == 0
    elif kind == "plate":             # one node thick, normal to axis 0, spanning the periodic box
        solid[res[0] // 2] = True
    else:
        assert kind == "none"
    return solid


@functools.lru_cache(maxsize=None)
def populations(lat, res, dt):
    """f = w_q * U(0.5, 1.5), seeded, 1 % of the entries negated, in the working dtype on the host: no symmetry that
    would hide a wrong sign or a swapped axis.  Shared; never written to."""
    stencil = STENCIL[lat]()
    g = torch.Generator().manual_seed(1234 + sum(res) + 7 * len(res) + stencil.q)
    shape = [stencil.q, *res]
    f = torch.as_tensor(np.array(stencil.w), dtype=torch.float64).reshape([-1] + [1] * len(res))
    f = f * (0.5 + torch.rand(shape, generator=g, dtype=torch.float64))
    f = torch.where(torch.rand(shape, generator=g, dtype=torch.float64) < 0.01, -f, f)
    return f.to(TORCH_DT[dt])


def exact_force(stencil, f, solid):
    """the definition: per component (fsum(terms), fsum(|terms|), number of terms).  f [q, *res] and solid [*res] on
    the host; f in any float dtype (it promotes to fp64 exactly)."""
    d = stencil.d
    f = f.detach().cpu().double()
    solid = solid.detach().cpu() != 0
    terms = [[] for _ in range(d)]
    for q in range(1, stencil.q):
        e = [int(x) for x in stencil.e[q]]
        up = torch.roll(solid, shifts=tuple(e), dims=tuple(range(d)))
        link = solid & ~up
        values = f[q][link].tolist()
        for c in range(d):
            if e[c]:
                terms[c] += [2.0 * e[c] * v for v in values]
    return [(math.fsum(t), math.fsum(abs(v) for v in t), len(t)) for t in terms]


def assert_within_bound(got, exact, dtype, what=""):
    """got: [d] values; exact: exact_force's answer.  Prints each figure before it asserts."""
    got = [float(v) for v in got]
    assert len(got) == len(exact)
    for c, (value, (want, magnitude, n)) in enumerate(zip(got, exact)):
        bound = max(n - 1, 0) * U * magnitude
        if dtype == torch.float32:
            bound += 0.5 * float(np.spacing(np.float32(abs(value))))
        err = abs(value - want)
        print(f"{what} F_{c} = {value!r}: {n} terms, error {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (what, c, value, want, n, err, bound)


# ------------------------------------------------------------------------------- torch path against the definition
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_torch_path_against_the_definition(case, dt):
    lat, res, kind = case
    stencil = STENCIL[lat]()
    flow = UniformFlow(ctx(dt), list(res), 100, 0.05, stencil)
    solid = solid_mask(kind, res)
    f = populations(lat, tuple(res), dt)
    flow.f = f.clone()
    obs = lt.BoundaryForce(flow, solid)
    got = obs()
    assert got.dtype == TORCH_DT[dt] and list(got.shape) == [stencil.d]
    exact = exact_force(stencil, f, solid)
    assert_within_bound(got.tolist(), exact, TORCH_DT[dt], case_id(case))
    assert torch.equal(obs(f), got)                                  # an explicit f is the same thing
    if kind in ("none", "all"):
        assert got.tolist() == [0.0] * stencil.d
    if kind == "block" and min(res) > 2:
        values = [e[0] for e in exact]
        assert len(set(values)) == len(values) and all(v != 0.0 for v in values)     # F_0 != F_1 != F_2


def test_a_body_in_a_stream_is_pushed_downstream():
    """sign: uniform flow in +x, one solid node, equilibrium populations -> F_0 > 0 and F_1 = 0 up to rounding"""
    flow = UniformFlow(ctx("f64"), [8, 8], 100, 0.05, lt.D2Q9())
    solid = torch.zeros([8, 8], dtype=torch.bool)
    solid[3, 4] = True
    rho = torch.ones([1, 8, 8], dtype=torch.float64)
    u = torch.zeros([2, 8, 8], dtype=torch.float64)
    u[0] = 0.05
    flow.f = flow.equilibrium(flow, rho=rho, u=u)
    force = lt.BoundaryForce(flow, solid)().tolist()
    assert force[0] > 1e-3 and abs(force[1]) < 1e-15


# ---------------------------------------------------------------------------------------------- momentum balance
BALANCE = [("D2Q9", [16, 12]), ("D3Q19", [8, 6, 10]), ("D3Q27", [8, 6, 10])]


def balance_mask(kind, res):
    solid = torch.zeros(res, dtype=torch.bool)
    solid[tuple(0 for _ in res)] = True                              # the corner node, in both masks
    if kind == "isolated":
        solid[tuple(n // 2 for n in res)] = True
        solid[tuple(n - 2 for n in res)] = True
    else:                                                            # a 3^d block
        solid[tuple(slice(n // 2 - 1, n // 2 + 2) for n in res)] = True
    return solid


def momentum(stencil, f):
    """P_c = sum_x sum_q e_{q,c} f_q, solid nodes included, exactly rounded"""
    e = np.array(stencil.e)
    f = f.detach().cpu().double()
    return [math.fsum(v for q in range(stencil.q) if e[q][c] for v in (float(e[q][c]) * f[q].reshape(-1)).tolist())
            for c in range(stencil.d)]


@pytest.mark.parametrize("kind", ["isolated", "block"])
@pytest.mark.parametrize("lat,res", BALANCE, ids=[f"{lat.lower()}-{'x'.join(map(str, r))}" for lat, r in BALANCE])
def test_momentum_balance_of_a_periodic_box(lat, res, kind):
    """bounce-back as the only boundary of a periodic box: P(t + 1) - P(t) = -F(t), provided the populations on
    solid-solid links are symmetric (f[:, solid] = w once, which they then stay).  fp64, BGK tau = 0.8.
    Bound: 4 * 2^-52 * sum |f(t)| -- 20 x the largest residual of the CPU path (0.2), which allows for other
    summation orders."""
    stencil = STENCIL[lat]()
    flow = UniformFlow(ctx("f64"), list(res), 100, 0.05, stencil)
    solid = balance_mask(kind, res)
    flow.boundaries = [lt.BounceBackBoundary(solid)]
    g = torch.Generator().manual_seed(99 + stencil.q)
    w = torch.as_tensor(np.array(stencil.w), dtype=torch.float64)
    f = w.reshape([-1] + [1] * stencil.d) * (0.5 + torch.rand([stencil.q, *res], generator=g, dtype=torch.float64))
    f[:, solid] = w[:, None]
    flow.f = f
    simulation = lt.Simulation(flow, lt.BGKCollision(0.8), [])
    observable = lt.BoundaryForce(flow, flow.boundaries[0])
    assert torch.equal(observable.mask.bool(), solid)
    simulation(1)
    for step in range(3):
        before = momentum(stencil, flow.f)
        force = observable().tolist()
        total = float(flow.f.abs().sum())
        simulation(1)
        after = momentum(stencil, flow.f)
        residual = max(abs(a - b + F) for a, b, F in zip(after, before, force))
        print(f"{lat} {res} {kind} step {step}: F = {force}, residual {residual:.3e} = "
              f"{residual / (2.0 ** -52 * total):.3f} * 2^-52 * sum |f|")
        assert math.sqrt(sum(F * F for F in force)) > 1e-4
        assert residual <= 4 * 2.0 ** -52 * total


# ------------------------------------------------------------------------------------------------- coefficients
@pytest.mark.parametrize("lat,res", [("D2Q9", [16, 12]), ("D3Q19", [12, 8, 8])], ids=["2d", "3d"])
def test_drag_and_lift_coefficients_scale_the_force(lat, res):
    stencil = STENCIL[lat]()
    flow = lt.Obstacle(ctx("f64"), list(res), 50, 0.05, domain_length_x=4.0, stencil=stencil)
    solid = torch.zeros(res, dtype=torch.bool)
    solid[tuple(slice(n // 2 - 1, n // 2 + 1) for n in res)] = True
    solid[tuple(n // 2 + 1 for n in res)] = True                     # lopsided: a lift that is not zero
    flow.mask = solid
    flow.initialize()
    lt.Simulation(flow, lt.BGKCollision(0.8), [])(3)
    d = stencil.d
    area = 0.5 if d == 2 else 0.25
    units = flow.units
    area_lu = area * units.convert_length_to_lu(1.0) ** (d - 1)
    scale = 0.5 * units.characteristic_density_lu * units.characteristic_velocity_lu ** 2 * area_lu
    force = lt.BoundaryForce(flow, solid)().tolist()
    drag = lt.DragCoefficient(flow, solid, area)
    lift = lt.LiftCoefficient(flow, lt.BounceBackBoundary(flow.mask), area)
    assert (drag.direction, lift.direction) == (0, 1) and drag.area_lu == pytest.approx(area_lu, rel=1e-15)
    assert force[0] > 0 and force[1] != 0
    for observable, component in ((drag, 0), (lift, 1), (lt.DragCoefficient(flow, solid, area, direction=d - 1), d - 1)):
        got = observable()
        assert got.dtype == torch.float64 and got.dim() == 0
        want = force[component] / scale
        print(f"{lat} {type(observable).__name__}[{component}] = {float(got)!r}, F / scale = {want!r}")
        assert abs(float(got) - want) <= 2 * U * abs(want)           # one division against the test's own product
    with pytest.raises(lt.LettuceException, match="DragCoefficient: direction 3"):
        lt.DragCoefficient(flow, solid, area, direction=3)


def test_observable_reporter_prints_the_components():
    flow = lt.Obstacle(ctx("f64"), [16, 12], 50, 0.05, domain_length_x=4.0, stencil=lt.D2Q9())
    solid = torch.zeros([16, 12], dtype=torch.bool)
    solid[7:10, 5:8] = True
    flow.mask = solid
    force = lt.ObservableReporter(lt.BoundaryForce(flow, solid), interval=2, out=None)
    drag = lt.ObservableReporter(lt.DragCoefficient(flow, solid, 0.75), interval=2, out=None)
    lt.Simulation(flow, lt.BGKCollision(0.8), [force, drag])(4)
    assert [len(row) for row in force.out] == [4] * 3 and [len(row) for row in drag.out] == [3] * 3
    assert np.isfinite(force.out).all() and force.out[-1][2] > 0


# ----------------------------------------------------------------------------------------------------- refusals
def test_mask_of_the_wrong_shape_is_refused_and_the_property_converts():
    flow = UniformFlow(ctx("f32"), [6, 5], 100, 0.05, lt.D2Q9())
    with pytest.raises(lt.LettuceException, match=r"BoundaryForce: mask of shape \[5, 6\] on a grid \[6, 5\]"):
        lt.BoundaryForce(flow, torch.zeros([5, 6], dtype=torch.bool))
    with pytest.raises(lt.LettuceException, match=r"LiftCoefficient: mask of shape \[6\]"):
        lt.LiftCoefficient(flow, lt.BounceBackBoundary(torch.zeros([6], dtype=torch.bool)), 1.0)
    obs = lt.BoundaryForce(flow, np.zeros([6, 5], dtype=bool))
    assert obs.mask.dtype == torch.uint8 and obs.mask.is_contiguous() and obs.mask.device == flow.context.device
    assert not obs.mask.any() and obs().tolist() == [0.0, 0.0]
    transposed = torch.zeros([5, 6], dtype=torch.bool)
    transposed[2, 3] = True
    obs.mask = transposed.t()                                        # re-converted: contiguous uint8 again
    assert obs.mask.dtype == torch.uint8 and obs.mask.is_contiguous() and obs.mask[3, 2] == 1 and obs.mask.sum() == 1
    with pytest.raises(lt.LettuceException, match="mask of shape"):
        obs.mask = torch.zeros([6, 6], dtype=torch.bool)
    assert not getattr(obs, "slab_aware", False)


def test_slab_simulation_refuses_the_force_by_name():
    slab = lt.ZSlab([8, 8, 8], 0, 1)
    flow = lt.Obstacle(ctx("f32"), slab.extended_resolution, 100, 0.05, domain_length_x=4.0, stencil=lt.D3Q19(),
                       slab=slab)
    for observable in (lt.BoundaryForce(flow, flow.mask), lt.DragCoefficient(flow, flow.mask, 1.0),
                       lt.LiftCoefficient(flow, flow.mask, 1.0)):
        reporter = lt.ObservableReporter(observable, interval=1, out=None)
        with pytest.raises(lt.LettuceException, match="reporter ObservableReporter reads flow.f"):
            lt.SlabSimulation(flow, lt.BGKCollision(0.8), slab, reporter=[reporter])


# ----------------------------------------------------------------------------------------------------- plumbing
def test_binding_header_and_library(engine_library):
    from lettuce_amd import _native
    vp = ctypes.c_void_p
    assert _native.SYMBOLS["lt_boundary_force"] == (ctypes.c_int, [vp, vp, vp, vp, vp, vp])
    assert hasattr(_native.Plan, "boundary_force")
    header = open(os.path.join(ROOT, "include", "lettuce_hip.h")).read()
    assert re.search(r"int\s+lt_boundary_force\s*\(\s*lt_plan\s*\*\s*plan\s*,\s*const\s+void\s*\*\s*f_dev\s*,"
                     r"\s*const\s+uint8_t\s*\*\s*solid_dev\s*,\s*double\s*\*\s*partial_scratch_dev\s*,"
                     r"\s*double\s*\*\s*out_dev\s*,\s*void\s*\*\s*stream\s*\)\s*;", header)
    assert re.search(r"#define\s+LT_ABI_VERSION\s+2\b", header)      # one new entry point, no struct changes
    assert re.search(rf"#define\s+LT_BOUNDARY_FORCE_BLOCKS\s+{_native.BOUNDARY_FORCE_BLOCKS}\b", header)
    lib = ctypes.CDLL(engine_library)
    lib.lt_abi_version.restype = ctypes.c_int
    assert lib.lt_abi_version() == 2
    assert hasattr(lib, "lt_boundary_force")
    lib.lt_boundary_force.restype = ctypes.c_int
    lib.lt_boundary_force.argtypes = _native.SYMBOLS["lt_boundary_force"][1]
    assert lib.lt_boundary_force(None, None, None, None, None, None) == 1      # LT_ERR_INVALID, nothing dereferenced
    lib.lt_last_error.restype = ctypes.c_char_p
    assert b"null plan" in lib.lt_last_error()
