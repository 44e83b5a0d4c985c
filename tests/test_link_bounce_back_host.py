"""Interpolated and half-way bounce-back on the host (CPU, no GPU needed): the torch path of
``lt.InterpolatedBounceBackBoundary`` / ``lt.HalfwayBounceBackBoundary`` against an independent statement of the half-way
rule, the force-driven channel with walls on and off the half-way position, the gap fallback, ``sphere_link_fractions``
against a bisection, the compact link list against the dense definition, the force and ``Obstacle(solid_boundary=...)``.

Bounds: bit identity where the arithmetic is the same; the channel gates are those of the formulation's prototype (the
interpolated error at most 100 x the full-way one at d = 1/2, below half of it off the half-way position); the sums use
the bound of test_boundary_force_host.py.  Every comparison prints its figures before it asserts.

Measured (CPU, fp64, 6000 steps, max |u - parabola| / max parabola; full-way / interpolated):
  tau = 1/2 + sqrt(3)/4, d = 1/2:  4.0e-12 / 7.1e-12        tau = 0.8, d = 1/4:  0.1309 / 0.0150 (8.7 x)
                                                             tau = 0.8, d = 3/4:  0.1231 / 0.0164 (7.5 x)"""
import functools
import math

import numpy as np
import pytest
import torch

import lettuce_amd as lt
from conftest import TORCH_DT
from test_boundary_force_host import U, assert_within_bound, exact_force
from test_host_api import ctx, UniformFlow

STENCIL = {"D2Q9": lt.D2Q9, "D3Q15": lt.D3Q15, "D3Q19": lt.D3Q19, "D3Q27": lt.D3Q27}
GRIDS = [("D2Q9", [5, 7]), ("D3Q19", [4, 5, 6]), ("D3Q27", [4, 4, 4]), ("D3Q15", [5, 4, 6])]
MASKS = ["isolated", "plate", "block", "seam"]


def body_mask(kind, res):
    """bool [*res]: an isolated node, a plate one node thick (normal to axis 0, across the box), a block of two nodes,
    a body of two nodes across the periodic seam of axis 0; "none": empty"""
    res = list(res)
    solid = torch.zeros(res, dtype=torch.bool)
    mid = tuple(n // 2 for n in res)
    if kind == "isolated":
        solid[mid] = True
    elif kind == "plate":
        solid[res[0] // 2] = True
    elif kind == "block":
        solid[mid] = True
        solid[tuple(m + (1 if a == len(res) - 1 else 0) for a, m in enumerate(mid))] = True
    elif kind == "seam":
        solid[(0,) + mid[1:]] = True
        solid[(res[0] - 1,) + mid[1:]] = True
    else:
        assert kind == "none"
    return solid


@functools.lru_cache(maxsize=None)
def random_state(lat, res, dt, seed=0):
    """f = w_q * U(0.5, 1.5), seeded: no symmetry.  Shared; never written to."""
    stencil = STENCIL[lat]()
    g = torch.Generator().manual_seed(4321 + seed + sum(res) + stencil.q)
    w = torch.as_tensor(np.array(stencil.w), dtype=torch.float64).reshape([-1] + [1] * len(res))
    return (w * (0.5 + torch.rand([stencil.q, *res], generator=g, dtype=torch.float64))).to(TORCH_DT[dt])


def random_fractions(lat, res, seed=0):
    """[q, *res] in (0, 1], on both sides of 1/2, some exactly 1/2 and 1"""
    stencil = STENCIL[lat]()
    g = torch.Generator().manual_seed(77 + seed + sum(res) + stencil.q)
    d = 0.02 + 0.98 * torch.rand([stencil.q, *res], generator=g, dtype=torch.float64)
    pick = torch.rand([stencil.q, *res], generator=g, dtype=torch.float64)
    d = torch.where(pick < 0.1, torch.full_like(d, 0.5), d)
    return torch.where(pick > 0.9, torch.ones_like(d), d)


def dense_definition(stencil, f, solid, fractions):
    """the issue's definition, slot by slot in Python loops: (g [q, *res], links [(node, r, c1, c2, second)]) with node
    the C-order index of x_s, in the order node, then direction; c1 / c2 torch scalars of f's dtype"""
    res = list(solid.shape)
    e = [[int(c) for c in v] for v in stencil.e]
    opposite = [int(o) for o in stencil.opposite]
    g = f.clone()
    links = []
    for node, x_s in enumerate(np.ndindex(*res)):
        if not solid[x_s]:
            continue
        for r in range(1, stencil.q):
            x_f = tuple((x_s[a] + e[r][a]) % res[a] for a in range(len(res)))
            if solid[x_f]:
                continue
            x_ff = tuple((x_f[a] + e[r][a]) % res[a] for a in range(len(res)))
            q = opposite[r]
            d = torch.tensor(0.5 if fractions is None else float(fractions[(r,) + x_s]), dtype=f.dtype)
            if solid[x_ff]:
                d = torch.tensor(0.5, dtype=f.dtype)
            if float(d) < 0.5:
                c1, c2, b, second = 2 * d, 1 - 2 * d, f[(q,) + x_ff], 0
            else:
                c1, c2, b, second = 1 / (2 * d), (2 * d - 1) / (2 * d), f[(r,) + x_f], 1
            g[(r,) + x_s] = c1 * f[(q,) + x_f] + c2 * b
            links.append((node, r, c1, c2, second))
    return g, links


# ------------------------------------------------------------------------ 1. half-way against an independent statement
@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("lat,res", GRIDS, ids=[g[0].lower() for g in GRIDS])
def test_halfway_rule_against_a_fluid_side_statement(lat, res, kind, dt):
    """after streaming, f_r(x_f) = f*_q(x_f) wherever x_f - e_r is solid: five steps, bit for bit on the fluid nodes"""
    stencil = STENCIL[lat]()
    solid = body_mask(kind, res)
    axes = tuple(range(stencil.d))
    flow = UniformFlow(ctx(dt), list(res), 100, 0.05, stencil)
    flow.boundaries = [lt.HalfwayBounceBackBoundary(solid)]
    flow.f = random_state(lat, tuple(res), dt).clone()
    simulation = lt.Simulation(flow, lt.BGKCollision(0.8), [])
    # the statement: its own flow without boundaries serves the collision; solid nodes are never collided and what
    # they hold never reaches a fluid node
    other = UniformFlow(ctx(dt), list(res), 100, 0.05, stencil)
    collision = lt.BGKCollision(0.8)
    f = random_state(lat, tuple(res), dt).clone()
    for step in range(5):
        simulation(1)
        other.f = f
        star = torch.where(solid, f, collision(other))
        f = torch.stack([torch.roll(star[r], shifts=tuple(int(c) for c in stencil.e[r]), dims=axes)
                         for r in range(stencil.q)])
        for r in range(1, stencil.q):
            behind = torch.roll(solid, shifts=tuple(int(c) for c in stencil.e[r]), dims=axes)      # x_f - e_r is solid
            f[r] = torch.where(behind & ~solid, star[int(stencil.opposite[r])], f[r])
        difference = float((flow.f - f)[:, ~solid].abs().max())
        print(f"{lat} {res} {kind} {dt} step {step}: largest difference on fluid nodes {difference:.3e}")
        assert torch.equal(flow.f[:, ~solid], f[:, ~solid])
    assert not torch.equal(flow.f[:, ~solid], random_state(lat, tuple(res), dt)[:, ~solid])


# -------------------------------------------------------------------------------------------------- 2., 3. the channel
@functools.lru_cache(maxsize=None)
def channel(tau, d, kind, steps=6000, nx=4, ny=10, a=1e-6):
    """D2Q9, nx x ny with wall rows at y = 0 and y = ny - 1 (8 fluid rows), BGK + Guo, fp64, from rest: the velocity
    profile u_x [nx, ny - 2] of the fluid rows.  kind "full": BounceBackBoundary; else the interpolated boundary with
    every fraction d."""
    flow = UniformFlow(ctx("f64"), [nx, ny], 100, 0.05, lt.D2Q9())
    solid = torch.zeros([nx, ny], dtype=torch.bool)
    solid[:, 0] = True
    solid[:, -1] = True
    if kind == "full":
        flow.boundaries = [lt.BounceBackBoundary(solid)]
    else:
        flow.boundaries = [lt.InterpolatedBounceBackBoundary(solid, torch.full([9, nx, ny], d, dtype=torch.float64))]
    flow.f = flow.equilibrium(flow, rho=torch.ones([1, nx, ny], dtype=torch.float64),
                              u=torch.zeros([2, nx, ny], dtype=torch.float64))
    force = lt.Guo(flow, tau, [a, 0.0])
    lt.Simulation(flow, lt.BGKCollision(tau, force=force), [])(steps)
    return flow.u(acceleration=force.acceleration)[0][:, 1:-1].clone()


def channel_error(u, tau, d, ny=10, a=1e-6):
    """max |u - parabola| / max parabola for walls at distance d from the first and the last fluid row"""
    y = torch.arange(1, ny - 1, dtype=torch.float64)
    parabola = a / (2 * (tau - 0.5) / 3) * (y - (1 - d)) * ((ny - 2 + d) - y)
    return float((u - parabola[None]).abs().max() / parabola.max())


def test_channel_at_the_halfway_position_keeps_the_exact_profile():
    """tau = 1/2 + sqrt(3)/4 (Lambda = 3/16), d = 1/2: the half-way rule gives the parabola exactly; the interpolated
    pass adds a few roundings per step, not orders of magnitude: gate 100 x the full-way error of the same run"""
    tau = 0.5 + math.sqrt(3) / 4
    full = channel_error(channel(tau, 0.5, "full"), tau, 0.5)
    new = channel_error(channel(tau, 0.5, "interpolated"), tau, 0.5)
    print(f"channel tau = {tau:.6f}, d = 1/2: full-way error {full:.3e}, interpolated {new:.3e}, ratio {new / full:.2f}")
    assert full < 1e-9                                               # the full-way run is the exact profile itself
    assert new <= 100 * full


@pytest.mark.parametrize("d", [0.25, 0.75])
def test_channel_off_the_halfway_position(d):
    """tau = 0.8: against the parabola whose walls stand at the true positions the interpolated error is below half the
    full-way error"""
    full = channel_error(channel(0.8, 0.5, "full"), 0.8, d)          # the full-way rule does not know d: one run
    new = channel_error(channel(0.8, d, "interpolated"), 0.8, d)
    print(f"channel tau = 0.8, d = {d}: full-way error {full:.4e}, interpolated {new:.4e}, ratio {full / new:.2f}")
    assert new < 0.5 * full


# ---------------------------------------------------------------------------------------------------- 4. gap fallback
@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_a_gap_one_node_wide_falls_back_to_the_halfway_rule(dt):
    res = [7, 5]
    stencil = lt.D2Q9()
    solid = torch.zeros(res, dtype=torch.bool)
    solid[2] = True
    solid[4] = True                                                  # row 3 is a gap one node wide
    fractions = torch.full([9] + res, 0.3, dtype=torch.float64)
    boundary = lt.InterpolatedBounceBackBoundary(solid, fractions)
    links = boundary.links(stencil, TORCH_DT[dt])
    into_gap = (links.xf // res[1]) == 3
    assert int(into_gap.sum()) == 2 * 3 * res[1] and int((~into_gap).sum()) == 2 * 3 * res[1]
    print(f"gap {dt}: c1 {links.c1[into_gap].unique().tolist()}, c2 {links.c2[into_gap].unique().tolist()}; "
          f"elsewhere c1 {links.c1[~into_gap].unique().tolist()}, c2 {links.c2[~into_gap].unique().tolist()}")
    assert bool((links.c1[into_gap] == 1).all()) and bool((links.c2[into_gap] == 0).all())
    assert bool(links.second[into_gap].all()) and not bool(links.second[~into_gap].any())
    c = torch.tensor(0.3, dtype=torch.float64).to(TORCH_DT[dt])
    assert bool((links.c1[~into_gap] == 2 * c).all()) and bool((links.c2[~into_gap] == 1 - 2 * c).all())
    flow = UniformFlow(ctx(dt), res, 100, 0.05, stencil)
    flow.f = random_state("D2Q9", tuple(res), dt).clone()
    got = boundary(flow)
    want, _ = dense_definition(stencil, flow.f, solid, fractions)
    assert torch.equal(got, want)
    flat, out = flow.f.reshape(9, -1), got.reshape(9, -1)
    assert torch.equal(out[links.direction[into_gap], links.node[into_gap]],
                       flat[links.opposite[into_gap], links.xf[into_gap]])


# ------------------------------------------------------------------------------------------- 5. sphere_link_fractions
@pytest.mark.parametrize("lat,res,center,spacing", [("D2Q9", [9, 9], [4.2, 3.9], 1.0), ("D3Q27", [8, 8, 8], [3.6, 3.9, 4.1], 1.0),
                                                    ("D3Q19", [8, 8, 8], [1.8, 1.95, 2.05], 0.5)],
                         ids=["circle", "sphere", "sphere-dx"])
def test_sphere_link_fractions_against_a_bisection(lat, res, center, spacing):
    stencil = STENCIL[lat]()
    radius = 2.3 * spacing
    grid = torch.meshgrid(*[spacing * torch.arange(n, dtype=torch.float64) for n in res], indexing="ij")
    fractions = lt.sphere_link_fractions(stencil, grid, center, radius)
    assert list(fractions.shape) == [stencil.q] + res and fractions.dtype == torch.float64
    inside = sum((g - c) ** 2 for g, c in zip(grid, center)) < radius ** 2
    assert bool(((fractions > 0) & (fractions <= 1)).all())
    worst, count = 0.0, 0
    for x_s in np.ndindex(*res):
        if not inside[x_s]:
            continue
        for r in range(1, stencil.q):
            e = [int(c) for c in stencil.e[r]]
            x_f = tuple(x_s[a] + e[a] for a in range(stencil.d))
            if all(0 <= x_f[a] < res[a] for a in range(stencil.d)) and inside[x_f]:
                continue                                             # (the sphere stays clear of the box's faces)
            outside = lambda t: math.sqrt(sum((spacing * (x_f[a] - t * e[a]) - center[a]) ** 2     # noqa: E731
                                              for a in range(stencil.d))) >= radius
            assert outside(0.0) and not outside(1.0)
            lo, hi = 0.0, 1.0
            for _ in range(60):
                mid = 0.5 * (lo + hi)
                lo, hi = (mid, hi) if outside(mid) else (lo, mid)
            worst = max(worst, abs(float(fractions[(r,) + x_s]) - 0.5 * (lo + hi)))
            count += 1
    print(f"{lat} {res}: {count} links, largest |fraction - bisection| = {worst:.3e}")
    assert count > 20 and worst <= 1e-12
    slots = torch.zeros_like(fractions, dtype=torch.bool)
    for r in range(1, stencil.q):
        e = tuple(-int(c) for c in stencil.e[r])
        slots[r] = inside & ~torch.roll(inside, shifts=e, dims=tuple(range(stencil.d)))
    assert bool((fractions[~slots] == 0.5).all())                    # what is no link slot holds 1/2
    assert len(fractions[slots].unique()) > count // 4               # and the links are not all alike
    boundary = lt.InterpolatedBounceBackBoundary(inside, fractions)
    assert len(boundary.links(stencil, torch.float64)) == count


# ----------------------------------------------------------------------------------------------------- 6. the link list
@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("kind", MASKS + ["none"])
@pytest.mark.parametrize("lat,res", GRIDS, ids=[g[0].lower() for g in GRIDS])
def test_compact_link_list_and_call_equal_the_dense_definition(lat, res, kind, dt):
    stencil = STENCIL[lat]()
    solid = body_mask(kind, res)
    fractions = random_fractions(lat, tuple(res))
    f = random_state(lat, tuple(res), dt)
    f = torch.where(random_state(lat, tuple(res), dt, seed=5) < 0.6 * f.abs().mean(), -f, f)       # negative ones too
    boundary = lt.InterpolatedBounceBackBoundary(solid, fractions)
    want, dense = dense_definition(stencil, f, solid, fractions)
    links = boundary.links(stencil, TORCH_DT[dt])
    got = list(zip(links.node.tolist(), links.direction.tolist(), links.c1.tolist(), links.c2.tolist(),
                   [int(s) for s in links.second.tolist()]))
    expected = [(n, r, float(c1), float(c2), s) for n, r, c1, c2, s in dense]
    print(f"{lat} {res} {kind} {dt}: {len(got)} links")
    assert got == expected                                           # the same links, coefficients and order
    assert got == sorted(got, key=lambda link: (link[0], link[1]))   # by node, then by direction
    assert links.c1.dtype == links.c2.dtype == TORCH_DT[dt]
    flow = UniformFlow(ctx(dt), list(res), 100, 0.05, stencil)
    flow.f = f.clone()
    out = boundary(flow)
    difference = float((out - want).abs().max())
    print(f"  largest |call - definition| = {difference:.3e}")
    assert torch.equal(out, want) and torch.equal(flow.f, f)         # and nothing is mutated in place
    assert (kind == "none") == (len(got) == 0)
    # what the engine takes: the same list, no refusal while the body is alone
    ncm = solid.to(torch.uint8) * 3
    nodes, directions, c1, c2, second = lt.native_link_list(boundary, 3, ncm, stencil, TORCH_DT[dt])
    assert nodes.dtype == torch.int32 and directions.dtype == second.dtype == torch.uint8
    assert list(zip(nodes.tolist(), directions.tolist(), c1.tolist(), c2.tolist(), second.tolist())) == got
    assert boundary.make_no_streaming_mask([stencil.q] + list(res), ctx(dt)) is None
    assert torch.equal(boundary.make_no_collision_mask(list(res), ctx(dt)), solid)


def test_assigning_mask_or_fractions_rebuilds_the_list_and_bad_fractions_are_refused():
    stencil, res = lt.D2Q9(), [5, 7]
    boundary = lt.InterpolatedBounceBackBoundary(body_mask("isolated", res))
    first = boundary.links(stencil, torch.float64)
    assert boundary.links(stencil, torch.float64) is first and bool((first.c1 == 1).all()) and bool((first.c2 == 0).all())
    boundary.fractions = torch.full([9] + res, 0.25, dtype=torch.float64)
    second = boundary.links(stencil, torch.float64)
    assert second is not first and bool((second.c1 == 0.5).all()) and bool((second.c2 == 0.5).all())
    boundary.mask = body_mask("block", res)
    assert len(boundary.links(stencil, torch.float64)) > len(second)
    boundary.fractions = torch.zeros([9] + res, dtype=torch.float64)
    with pytest.raises(lt.LettuceException, match=r"a fraction lies in \(0, 1\]"):
        boundary.links(stencil, torch.float64)
    boundary.fractions = torch.full([9, 5, 6], 0.5)
    with pytest.raises(lt.LettuceException, match="fractions of shape"):
        boundary.links(stencil, torch.float64)
    assert isinstance(lt.HalfwayBounceBackBoundary(body_mask("plate", res)), lt.InterpolatedBounceBackBoundary)


def test_the_engine_refuses_by_name_from_masks_alone():
    """a link whose x_f or x_ff belongs to another boundary; nodes of the body's mask under a higher index"""
    stencil, res = lt.D2Q9(), [8, 6]
    solid = torch.zeros(res, dtype=torch.bool)
    solid[3:5, 2:4] = True
    boundary = lt.HalfwayBounceBackBoundary(solid)
    ncm = solid.to(torch.uint8) * 2
    assert len(lt.native_link_list(boundary, 2, ncm, stencil, torch.float64)[0]) == 4 * 5     # 2 x 2 nodes, 5 fluid neighbours each
    touching = ncm.clone()
    touching[2, :] = 1                                               # an inlet row next to the body: x_f
    with pytest.raises(lt.NativeEngineError, match="reads a node of another boundary"):
        lt.native_link_list(boundary, 2, touching, stencil, torch.float64)
    two_away = ncm.clone()
    two_away[1, :] = 1                                               # ... two rows away: x_ff
    with pytest.raises(lt.NativeEngineError, match="reads a node of another boundary"):
        lt.native_link_list(boundary, 2, two_away, stencil, torch.float64)
    three_away = ncm.clone()
    three_away[0, :] = 1
    lt.native_link_list(boundary, 2, three_away, stencil, torch.float64)
    taken = ncm.clone()
    taken[3, 2] = 3                                                  # a higher index took a node of the body over
    with pytest.raises(lt.NativeEngineError, match="belong to a boundary of a higher index"):
        lt.native_link_list(boundary, 2, taken, stencil, torch.float64)
    wider = ncm.clone()
    wider[6, 4] = 2
    with pytest.raises(lt.NativeEngineError, match="outside its mask"):
        lt.native_link_list(boundary, 2, wider, stencil, torch.float64)
    assert boundary.native_available() and boundary.native_generator(2).plan_entry(None) == {"kind": "link_bounce_back"}
    from lettuce_amd import _native
    assert _native.LINK_BOUNDARY_KINDS == {"link_bounce_back": 6}


# ---------------------------------------------------------------------------------------------------------- 7. force
BALANCE = [("D2Q9", [16, 12]), ("D3Q19", [8, 6, 10]), ("D3Q27", [8, 6, 10])]


def fluid_momentum(stencil, f, solid):
    e = np.array(stencil.e)
    f = f.detach().cpu().double()[:, ~solid]
    return [math.fsum(v for q in range(stencil.q) if e[q][c] for v in (float(e[q][c]) * f[q]).tolist())
            for c in range(stencil.d)]


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("lat,res", BALANCE, ids=[g[0].lower() for g in BALANCE])
def test_link_force_on_a_halfway_body_equals_the_full_way_expression(lat, res, dt):
    """after a step with d = 1/2 what came back is what left, f_r(x_f) = f_q(x_s): the two-term sum is 2 e_q f_q(x_s).
    Both against the exact sum of those terms, bound of test_boundary_force_host.py"""
    from lettuce_amd.ext._reporter import link_momentum_exchange, momentum_exchange
    stencil = STENCIL[lat]()
    solid = torch.zeros(res, dtype=torch.bool)
    solid[tuple(slice(n // 2 - 1, n // 2 + 1) for n in res)] = True
    solid[tuple(0 for _ in res)] = True
    flow = UniformFlow(ctx(dt), list(res), 100, 0.05, stencil)
    body = lt.HalfwayBounceBackBoundary(solid)
    flow.boundaries = [body]
    flow.f = random_state(lat, tuple(res), dt, seed=3).clone()
    lt.Simulation(flow, lt.BGKCollision(0.8), [])(2)
    links = body.links(stencil, TORCH_DT[dt])
    got = link_momentum_exchange(stencil, flow.f, links)
    old = momentum_exchange(stencil, flow.f, solid)
    exact = exact_force(stencil, flow.f, solid)
    assert_within_bound(got.tolist(), exact, torch.float64, f"{lat} {dt} link_momentum_exchange")
    assert_within_bound(old.tolist(), exact, torch.float64, f"{lat} {dt} momentum_exchange")
    observable = lt.BoundaryForce(flow, body)
    assert torch.equal(observable.force(), got) and observable().dtype == TORCH_DT[dt]
    drag = lt.DragCoefficient(flow, body, 1.0)
    lift = lt.LiftCoefficient(flow, body, 1.0)
    assert float(drag()) != 0.0 and float(lift()) != 0.0 and float(drag()) != float(lift())
    # a full-way body and a bare mask do what they did
    assert torch.equal(lt.BoundaryForce(flow, lt.BounceBackBoundary(solid)).force(), old)
    assert torch.equal(lt.BoundaryForce(flow, solid).force(), old)


@pytest.mark.parametrize("lat,res", BALANCE, ids=[g[0].lower() for g in BALANCE])
def test_momentum_balance_of_a_periodic_box_with_an_interpolated_body(lat, res):
    """one body, fractions on both sides of 1/2, BGK tau = 0.8, fp64: over a step the fluid's momentum changes by -F,
    F on the populations after that step's streaming.  Bound as for the full-way body: 4 * 2^-52 * sum |f|."""
    stencil = STENCIL[lat]()
    solid = torch.zeros(res, dtype=torch.bool)
    solid[tuple(slice(n // 2 - 1, n // 2 + 2) for n in res)] = True
    solid[tuple(0 for _ in res)] = True
    flow = UniformFlow(ctx("f64"), list(res), 100, 0.05, stencil)
    body = lt.InterpolatedBounceBackBoundary(solid, random_fractions(lat, tuple(res), seed=9))
    flow.boundaries = [body]
    flow.f = random_state(lat, tuple(res), "f64", seed=4).clone()
    simulation = lt.Simulation(flow, lt.BGKCollision(0.8), [])
    observable = lt.BoundaryForce(flow, body)
    simulation(1)
    for step in range(3):
        before = fluid_momentum(stencil, flow.f, solid)
        total = float(flow.f[:, ~solid].abs().sum())
        simulation(1)
        after = fluid_momentum(stencil, flow.f, solid)
        force = observable().tolist()
        residual = max(abs(a - b + F) for a, b, F in zip(after, before, force))
        print(f"{lat} {res} step {step}: F = {force}, residual {residual:.3e} = "
              f"{residual / (2.0 ** -52 * total):.3f} * 2^-52 * sum |f|")
        assert math.sqrt(sum(F * F for F in force)) > 1e-4
        assert residual <= 4 * 2.0 ** -52 * total


# ------------------------------------------------------------------------------------------------------- 8. Obstacle
def test_obstacle_builds_the_solid_boundary_it_is_given():
    res = [16, 12]
    solid = torch.zeros(res, dtype=torch.bool)
    solid[6:9, 5:8] = True
    plain = lt.Obstacle(ctx("f64"), res, 50, 0.05, domain_length_x=4.0, stencil=lt.D2Q9())
    plain.mask = solid
    assert [type(b).__name__ for b in plain.boundaries] == ["EquilibriumBoundaryPU", "AntiBounceBackOutlet",
                                                            "BounceBackBoundary"]
    assert torch.equal(plain.boundaries[2]._mask, solid)
    fractions = torch.full([9] + res, 0.3, dtype=torch.float64)
    flow = lt.Obstacle(ctx("f64"), res, 50, 0.05, domain_length_x=4.0, stencil=lt.D2Q9(),
                       solid_boundary=lambda mask: lt.InterpolatedBounceBackBoundary(mask, fractions))
    flow.mask = solid
    body = flow.boundaries[2]
    assert isinstance(body, lt.InterpolatedBounceBackBoundary) and torch.equal(body.mask, solid)
    assert body.fractions is fractions
    with pytest.raises(TypeError):
        lt.Obstacle(ctx("f64"), res, 50, 0.05, 4.0, 1, 1, lt.D2Q9(), None, None, lt.HalfwayBounceBackBoundary)
    halfway = lt.Obstacle(ctx("f64"), res, 50, 0.05, domain_length_x=4.0, stencil=lt.D2Q9(),
                          solid_boundary=lt.HalfwayBounceBackBoundary)
    halfway.mask = solid
    halfway.initialize()
    simulation = lt.Simulation(halfway, lt.BGKCollision(0.8), [])
    assert type(simulation.boundaries[-1]).__name__ == "HalfwayBounceBackBoundary"       # sorts behind the other three
    assert torch.equal(simulation.no_collision_mask == 3, solid)
    simulation(5)
    assert bool(torch.isfinite(halfway.f).all()) and float(lt.DragCoefficient(halfway, simulation.boundaries[-1], 0.75)()) > 0


def test_slab_simulations_refuse_the_boundary_when_they_are_constructed():
    slab = lt.ZSlab([8, 8, 8], 0, 1)
    flow = lt.Obstacle(ctx("f32"), slab.extended_resolution, 100, 0.05, domain_length_x=4.0, stencil=lt.D3Q19(), slab=slab,
                       solid_boundary=lt.HalfwayBounceBackBoundary)
    for driver in (lt.SlabSimulation, lt.TwoStepSlabSimulation):
        with pytest.raises(lt.LettuceException, match=r"HalfwayBounceBackBoundary' \(link bounce-back\) has no slab kernel"):
            driver(flow, lt.BGKCollision(0.8), slab)


def test_binding_header_and_library(engine_library):
    import ctypes
    import os
    import re
    from conftest import ROOT
    from lettuce_amd import _native
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    assert _native.SYMBOLS["lt_plan_set_links"] == (ctypes.c_int, [vp, i32, i64, vp, vp, vp, vp, vp, vp])
    assert _native.SYMBOLS["lt_apply_links"] == (ctypes.c_int, [vp, vp, vp])
    assert _native.SYMBOLS["lt_link_force"] == (ctypes.c_int, [vp, i32, vp, vp, vp, vp])
    header = open(os.path.join(ROOT, "include", "lettuce_hip.h")).read()
    assert re.search(r"LT_BOUNDARY_LINK_BOUNCE_BACK\s*=\s*6\b", header)       # 5 stays unknown to lt_plan_create
    assert re.search(r"#define\s+LT_ABI_VERSION\s+2\b", header)      # new entry points, no struct changes
    assert re.search(rf"#define\s+LT_LINK_FORCE_BLOCKS\s+{_native.LINK_FORCE_BLOCKS}\b", header)
    lib = ctypes.CDLL(engine_library)
    for name in ("lt_plan_set_links", "lt_apply_links", "lt_link_force"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _native.SYMBOLS[name]
    lib.lt_last_error.restype = ctypes.c_char_p
    assert lib.lt_plan_set_links(None, 0, 0, None, None, None, None, None, None) == 1       # LT_ERR_INVALID
    assert b"null plan" in lib.lt_last_error()
    assert lib.lt_apply_links(None, None, None) == 1 and lib.lt_link_force(None, 0, None, None, None, None) == 1
