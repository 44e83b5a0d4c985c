"""The momentum-exchange force on the HIP path: ``lt_boundary_force`` through ``Plan.boundary_force`` against the
restatement of the definition in test_boundary_force_host.py (CPU, fp64, ``math.fsum``), its determinism, the
``BoundaryForce`` and ``DragCoefficient`` observables under a ``Simulation`` on a native context, and the refusals.

Bound, as on the host: |got - fsum(terms)| <= (n - 1) * 2^-53 * fsum(|terms|) per component with n terms; values cast to
fp32 add half an ulp of the result.  The kernel's own output is fp64 in both dtypes.

Measured on an MI355X: the kernel stays within 0.09 of the bound on every grid and mask (largest error 1.2e-15, D3Q27
[6, 5, 67]); the reported fp32 values are within their half ulp; 116 tests in 2 s."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import lettuce_amd as lt
from test_boundary_force_host import (GRIDS, MASKS, STENCIL, U, assert_within_bound, case_id, exact_force, populations,
                                      solid_mask)

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "f64": torch.float64}
CASES = [(lat, res, mask) for lat, res in GRIDS for mask in MASKS]


def native(dt):
    return lt.Context(device="cuda:0", dtype=DT[dt], use_native=True)


def plan_of(lat, res, dt, **kwargs):
    from lettuce_amd import _native
    return _native.Plan(lat, DT[dt], "none", list(res), **kwargs)


@functools.lru_cache(maxsize=None)
def exact(lat, res, kind, dt):
    return exact_force(STENCIL[lat](), populations(lat, res, dt), solid_mask(kind, res))


def on_device(mask):
    return mask.to(torch.uint8).contiguous().cuda()


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_kernel_against_the_definition(case, dt):
    lat, res, kind = case
    res = tuple(res)
    d = len(res)
    plan = plan_of(lat, res, dt)
    f = populations(lat, res, dt).cuda()
    if kind == "none":
        # first a call that leaves nonzero partial sums in the plan's scratch
        assert bool((plan.boundary_force(f, on_device(solid_mask("isolated", res))) != 0).any())
    got = plan.boundary_force(f, on_device(solid_mask(kind, res)))
    assert got.dtype == torch.float64 and list(got.shape) == [d]
    got = got.cpu().tolist()
    want = exact(lat, res, kind, dt)
    assert_within_bound(got, want, torch.float64, f"{case_id(case)} {dt}")
    if kind in ("none", "all"):
        assert got == [0.0] * d and all(n == 0 for _, _, n in want)
    if kind in ("isolated", "block", "checkerboard") and min(res) > 2:
        assert len(set(got)) == d and all(v != 0.0 for v in got)         # no symmetry: F_0 != F_1 != F_2


@pytest.mark.parametrize("lat,dt", [("D3Q19", "f32"), ("D3Q27", "f64"), ("D3Q15", "f32")])
def test_two_calls_give_the_same_bits(lat, dt):
    res = (6, 5, 67)
    plan, f = plan_of(lat, res, dt), populations(lat, res, dt).cuda()
    solid = on_device(solid_mask("checkerboard", res))
    first = plan.boundary_force(f, solid).clone()
    second = plan.boundary_force(f, solid)
    assert torch.equal(first, second) and bool((first != 0).all())


def force_terms(stencil, f, solid):
    """[d, nodes, q - 1] float64: what boundary_force_kernel adds for node i (C order of the grid) and q = 1 .. Q - 1, per
    logical component -- +-2 (double)f_q where x_s is solid and x_s - e_q is not and e_{q,c} != 0, +0.0 elsewhere"""
    d = stencil.d
    f = f.double().numpy().reshape(stencil.q, -1)
    items = np.zeros((d, f.shape[1], stencil.q - 1))
    for q in range(1, stencil.q):
        e = [int(x) for x in stencil.e[q]]
        link = (solid & ~torch.roll(solid, shifts=tuple(e), dims=tuple(range(d)))).numpy().ravel()
        v = np.where(link, 2.0 * f[q], 0.0)
        for c in range(d):
            if e[c]:
                items[c, :, q - 1] = v if e[c] > 0 else -v
    return items


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("lat,res", [("D2Q9", (5, 7)), ("D3Q19", (6, 5, 67)), ("D2Q9", (520, 510))],
                         ids=["d2q9-5x7", "d3q19-6x5x67", "d2q9-520x510"])
def test_the_force_has_the_bits_of_the_documented_summation_order(lat, res, dt):
    """The order of boundary_force.hpp and reduce.hpp, emulated on the host (fixed_order_sum.py), predicts the bytes:
    one workgroup; 8 workgroups with the last one partial; 1024 workgroups and two passes, where the rotation of the
    slots by 61 per pass decides which thread takes a node of the second pass.
    What pins the ORDER are the fp64 plans: fp32 terms widened to fp64 add exactly whatever the order, so the fp32 cases
    show only that every item is taken exactly once."""
    import fixed_order_sum as fos
    stencil = STENCIL[lat]()
    f, solid = populations(lat, res, dt), solid_mask("checkerboard", res)
    want = np.asarray(fos.boundary_force(force_terms(stencil, f, solid)), dtype=np.float64)
    got = plan_of(lat, res, dt).boundary_force(f.cuda(), on_device(solid)).cpu().numpy()
    print(f"{lat} {res} {dt}: got {got.tolist()!r}, emulation {want.tolist()!r}")
    assert got.dtype == np.float64 and bool((got != 0).all()) and got.tobytes() == want.tobytes()


# ------------------------------------------------------------------------------------------ through Simulation
class _CopyState(lt.Reporter):
    """keeps a host copy of flow.f at the steps the observable reporter acts on; placed before it in the list, so both
    see the same step.  Batchable like the library's reporters: the steps in between stay fused."""
    batchable = True

    def __init__(self, interval):
        super().__init__(interval)
        self.states = []

    def __call__(self, simulation):
        if simulation.flow.i % self.interval == 0:
            self.states.append((simulation.flow.i, simulation.flow.f.detach().cpu().clone()))


def run_obstacle(lat, res, block, collision, interval, steps, dt):
    stencil = STENCIL[lat]()
    flow = lt.Obstacle(native(dt), list(res), 50, 0.05, domain_length_x=4.0, stencil=stencil)
    solid = torch.zeros(list(res), dtype=torch.bool)
    solid[block] = True
    flow.mask = solid
    flow.initialize()
    body = next(b for b in flow.boundaries if isinstance(b, lt.BounceBackBoundary))
    area = 0.75
    copies = _CopyState(interval)
    force = lt.ObservableReporter(lt.BoundaryForce(flow, body), interval=interval, out=None)
    drag = lt.ObservableReporter(lt.DragCoefficient(flow, solid, area), interval=interval, out=None)
    simulation = lt.Simulation(flow, collision(flow), [copies, force, drag])
    assert simulation._native is not None, "HIP engine not in use"
    assert flow._engine_plan(flow.f) is not None
    simulation(steps)
    rows = steps // interval + 1
    assert len(copies.states) == len(force.out) == len(drag.out) == rows
    units = flow.units
    scale = (0.5 * units.characteristic_density_lu * units.characteristic_velocity_lu ** 2
             * area * units.convert_length_to_lu(1.0) ** (stencil.d - 1))
    for (i, state), reported, coefficient in zip(copies.states, force.out, drag.out):
        assert reported[0] == coefficient[0] == i and len(reported) == 2 + stencil.d and len(coefficient) == 3
        want = exact_force(stencil, state, solid)
        assert_within_bound(reported[2:], want, DT[dt], f"{lat} {dt} step {i}")
        assert i == 0 or reported[2] != 0.0                          # at rest inside the body: F = 0 before the first step
        # the coefficient: the fp64 sum over the scale, cast to the context dtype -- against the exact sum, the sum's
        # bound over the scale, one rounding of the division and half an ulp of the cast
        exact_c = want[0][0] / scale
        bound = max(want[0][2] - 1, 0) * U * want[0][1] / scale + 2 * U * abs(exact_c)
        if dt == "f32":
            bound += 0.5 * float(np.spacing(np.float32(abs(coefficient[2]))))
        print(f"{lat} {dt} step {i}: C_d = {coefficient[2]!r}, F_0 / scale = {exact_c!r}, bound {bound:.3e}")
        assert abs(coefficient[2] - exact_c) <= bound
    return force.out


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_reported_force_d2q9_bgk(dt):
    """Obstacle D2Q9 [16, 12] with a 3 x 3 block, BGK, every 2 of 6 steps: covers the deferred streaming pass"""
    out = run_obstacle("D2Q9", [16, 12], (slice(6, 9), slice(5, 8)), lambda flow: lt.BGKCollision(0.8), 2, 6, dt)
    assert [row[0] for row in out] == [0, 2, 4, 6] and out[-1][2] > 0


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_reported_force_d3q27_kbc(dt):
    """Obstacle D3Q27 [8, 8, 8] with a 2^3 block, KBC, every step of 3"""
    out = run_obstacle("D3Q27", [8, 8, 8], (slice(3, 5), slice(3, 5), slice(3, 5)),
                       lambda flow: lt.KBCCollision(flow.units.relaxation_parameter_lu), 1, 3, dt)
    assert [row[0] for row in out] == [0, 1, 2, 3] and out[-1][2] > 0


# ----------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    from lettuce_amd import _native
    f3 = torch.full([19, 8, 8, 6], 1.0 / 19, dtype=torch.float32, device="cuda")
    solid3 = torch.zeros([8, 8, 6], dtype=torch.uint8, device="cuda")
    slab = plan_of("D3Q19", [8, 8, 6], "f32", layout=_native.LAYOUT_SLAB, ghost_planes=1)
    with pytest.raises(_native.NativeEngineError, match="boundary force: 2-D / 3-D grids in the reference layout") as e:
        slab.boundary_force(torch.zeros(slab.f_shape, dtype=torch.float32, device="cuda"),
                            torch.zeros(slab.f_shape[1:], dtype=torch.uint8, device="cuda"))
    assert e.value.code == 2                                       # LT_ERR_UNSUPPORTED
    line = plan_of("D1Q3", [16], "f32")
    with pytest.raises(_native.NativeEngineError, match="boundary force: 2-D / 3-D grids") as e:
        line.boundary_force(torch.zeros([3, 16], dtype=torch.float32, device="cuda"),
                            torch.zeros([16], dtype=torch.uint8, device="cuda"))
    assert e.value.code == 2
    plan = plan_of("D3Q19", [8, 8, 6], "f32")
    with pytest.raises(_native.NativeEngineError, match="solid mask: need a contiguous uint8 tensor"):
        plan.boundary_force(f3, solid3.bool())
    with pytest.raises(_native.NativeEngineError, match="solid mask: need a contiguous uint8 tensor"):
        plan.boundary_force(f3, solid3[:, :, :5])
    with pytest.raises(_native.NativeEngineError, match="tensor dtype"):
        plan.boundary_force(f3.double(), solid3)
    scratch = torch.zeros([3, _native.BOUNDARY_FORCE_BLOCKS], dtype=torch.float64, device="cuda")
    out = torch.zeros([3], dtype=torch.float64, device="cuda")
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())                  # noqa: E731
    full = (ptr(f3), ptr(solid3), ptr(scratch), ptr(out))
    for missing in range(4):
        args = [None if k == missing else a for k, a in enumerate(full)]
        assert plan.lib.lt_boundary_force(plan._handle, *args, None) == 1          # LT_ERR_INVALID
        assert b"null populations / solid mask / scratch / output" in plan.lib.lt_last_error()
    assert plan.lib.lt_boundary_force(None, *full, None) == 1
    assert plan.boundary_force(f3, solid3).tolist() == [0.0] * 3    # and the plan still works
