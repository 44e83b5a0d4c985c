"""Body forces on the host (CPU, no GPU needed): the mirror's Guo and Shan-Chen schemes against vectors produced by
the reference's own CPU path (tests/golden/force_*.npz, made by tools/gen_golden_force.py), the channel flow they
drive, and the plumbing that hands a uniform force to the HIP engine (descriptor, binding, header, exported symbol,
refusals).

Bounds: those of test_smagorinsky_host.py -- fp64 the project's 2e-14, fp32 8e-7 -- for the collided field, the
velocity and every stepped snapshot alike."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import lettuce_amd as lt
from conftest import golden, unpack_nsm, TORCH_DT, ROOT
from test_host_api import ctx

ATOL = {"f64": 2e-14, "f32": 8e-7}
LATTICES = {"d2q9": lt.D2Q9, "d3q15": lt.D3Q15, "d3q19": lt.D3Q19, "d3q27": lt.D3Q27}
CASES = ([("guo", "bgk", lat) for lat in LATTICES]
         + [("guo", "smagorinsky", lat) for lat in ("d2q9", "d3q19")]
         + [("shanchen", "bgk", lat) for lat in ("d2q9", "d3q19")])
PERIODIC = [f"force_{scheme}_{operator}_{lat}_{dt}" for scheme, operator, lat in CASES for dt in ("f64", "f32")]
ENGINE_F32, ENGINE_F64 = 1e-5, 1e-12       # the engine tests' bounds, which the fixtures must separate from


def close(got, want, dt):
    got, want = np.asarray(got), np.asarray(want)
    err = float(np.abs(got - want).max())
    print(f"max |difference| {err:.3e} (bound {ATOL[dt]:.1e})")
    np.testing.assert_allclose(got, want, rtol=0, atol=ATOL[dt])


def fixture_flow(g, name):
    _, scheme, operator, lat, dt = name.split("_")
    flow = lt.TaylorGreenVortex(ctx(dt), [int(r) for r in g["resolution"]], float(g["reynolds"]), float(g["mach"]),
                                LATTICES[lat]())
    flow.f = torch.tensor(g["f0"])
    return flow, scheme, operator, dt


def make_collision(flow, g, scheme, operator, acceleration=None, force_tau=None):
    acceleration = [float(a) for a in g["acceleration"]] if acceleration is None else acceleration
    force_tau = float(g["force_tau"]) if force_tau is None else force_tau
    force = {"guo": lt.Guo, "shanchen": lt.ShanChen}[scheme](flow, force_tau, acceleration)
    if operator == "bgk":
        return lt.BGKCollision(float(g["tau"]), force=force)
    return lt.SmagorinskyCollision(float(g["tau"]), float(g["constant"]), force=force)


@pytest.mark.parametrize("name", PERIODIC)
def test_torch_path_matches_the_reference(name):
    """collision(flow), flow.u(acceleration=...) and f after 1, 2, 3 and 10 steps"""
    g = golden(name)
    flow, scheme, operator, dt = fixture_flow(g, name)
    assert flow.f.dtype == TORCH_DT[dt]
    collision = make_collision(flow, g, scheme, operator)
    f0 = flow.f.clone()
    close(collision(flow).numpy(), g["collided"], dt)
    assert torch.equal(flow.f, f0)
    close(flow.u(acceleration=collision.force.acceleration).numpy(), g["u0"], dt)
    assert collision.force.ueq_scaling_factor == pytest.approx(float(g["ueq_scale"]), rel=1e-15)
    sim = lt.Simulation(flow, collision, [])
    for i in range(1, 11):
        sim(1)
        if i in (1, 2, 3, 10):
            close(flow.f.numpy(), g[f"f{i}"], dt)


class _WrongGuo(lt.Guo):
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


class _SourceAtUnshiftedVelocity(lt.BGKCollision):
    def __call__(self, flow):
        u = flow.u() + self.force.u_eq(flow)
        feq = flow.equilibrium(flow, u=u)
        return flow.f - 1.0 / self.tau * (flow.f - feq) + self.force.source_term(flow.u())


def _after(g, name, make, steps=10):
    """(collided, f after `steps`) of the operator make(flow) from the fixture's initial state"""
    flow = fixture_flow(g, name)[0]
    collision = make(flow)
    collided = collision(flow).numpy()
    lt.Simulation(flow, collision, [])(steps)
    return collided, flow.f.numpy()


@pytest.mark.parametrize("name", PERIODIC)
def test_fixtures_tell_the_operator_from_wrong_ones(name):
    """what the generator asserted when it wrote them, checked again on the mirror: these vectors would catch an
    operator without the force, with a wrong velocity shift or source factor, with the axes of the acceleration
    mixed up or with the wrong relaxation time in the force -- by 10 engine tolerances (fp32: 1e-5) at the collision
    and 100 after 10 steps -- and, in fp64 (1e-12), a source term at the unshifted velocity or Shan-Chen for Guo"""
    g = golden(name)
    _, scheme, operator, dt = fixture_flow(g, name)
    tau, a = float(g["tau"]), [float(v) for v in g["acceleration"]]
    plain = ((lambda fl: lt.BGKCollision(tau)) if operator == "bgk"
             else (lambda fl: lt.SmagorinskyCollision(tau, float(g["constant"]))))
    wrong = {"no force": plain,
             "components reversed": lambda fl: make_collision(fl, g, scheme, operator, acceleration=a[::-1])}
    subtle = {}
    if (scheme, operator) == ("guo", "bgk"):
        wrong.update({"no velocity shift": lambda fl: lt.BGKCollision(tau, force=_WrongGuo(fl, tau, a, shift=0.0)),
                      "shift of 1": lambda fl: lt.BGKCollision(tau, force=_WrongGuo(fl, tau, a, shift=1.0)),
                      "source without its factor": lambda fl: lt.BGKCollision(tau, force=_WrongGuo(fl, tau, a, factor=False)),
                      "force.tau = 0.6": lambda fl: make_collision(fl, g, scheme, operator, force_tau=0.6)})
        if dt == "f64":
            subtle = {"source at the unshifted velocity": lambda fl: _SourceAtUnshiftedVelocity(tau, force=lt.Guo(fl, tau, a)),
                      "Shan-Chen for Guo": lambda fl: lt.BGKCollision(tau, force=lt.ShanChen(fl, tau, a))}
    for bound, variants in ((ENGINE_F32, wrong), (ENGINE_F64, subtle)):
        for what, make in variants.items():
            collided, f10 = _after(g, name, make)
            gaps = np.abs(collided - g["collided"]).max(), np.abs(f10 - g["f10"]).max()
            print(f"{what}: {gaps[0]:.2e} / {gaps[1]:.2e}")
            assert gaps[0] >= 10 * bound and gaps[1] >= 100 * bound, what


def test_reference_attributes_and_exports():
    flow = lt.TaylorGreenVortex(ctx(), [8, 8], 100, 0.05, lt.D2Q9())
    guo, shan = lt.Guo(flow, 0.8, [1e-3, 0]), lt.ShanChen(flow, 0.7, [1e-3, 0])
    assert isinstance(guo, lt.Force) and isinstance(shan, lt.Force)
    assert lt.ext.Guo is lt.Guo and lt.ext.ShanChen is lt.ShanChen and lt.ext.Force is lt.Force
    assert (guo.ueq_scaling_factor, shan.ueq_scaling_factor, shan.source_term(None)) == (0.5, 0.7, 0)
    assert guo.acceleration.dtype == torch.float64 and guo.flow is flow and guo.tau == 0.8
    assert lt.BGKCollision(0.8, force=guo).name() == "BGKCollision_Guo"
    with pytest.raises(TypeError):
        lt.Force(flow, 0.8, [0, 0])                                  # abstract, as in the reference


def test_descriptor_reads_acceleration_and_scales_late():
    flow = lt.TaylorGreenVortex(ctx(), [8, 8, 8], 100, 0.05, lt.D3Q19())
    guo = lt.Guo(flow, 0.8, [2e-3, -3e-3, 1e-3])
    collision = lt.BGKCollision(0.8, force=guo)
    desc = collision.native_generator()
    assert desc.kind == "bgk" and isinstance(desc.force, lt.native_desc.NativeForce) and desc.force.kind == "guo"
    assert desc.force.plan_args() == ((2e-3, -3e-3, 1e-3), 0.5, 1 - 1 / 1.6)
    guo.acceleration = flow.context.convert_to_tensor([0.0, 1e-3, 0.0])
    guo.tau = 0.6                                                    # re-read per batch, like tau
    assert desc.force.plan_args() == ((0.0, 1e-3, 0.0), 0.5, 1 - 1 / 1.2)
    shan = lt.ShanChen(flow, 0.7, [1e-3, 0, 0])
    desc = lt.SmagorinskyCollision(0.6, 0.2, force=shan).native_generator()
    assert desc.kind == "smagorinsky" and desc.force.kind == "shan_chen"
    assert desc.force.plan_args() == ((1e-3, 0.0, 0.0), 0.7, 0.0)
    shan.tau = 0.9
    assert desc.force.ueq_scale() == 0.9
    assert lt.BGKCollision(0.6).native_generator().force is None
    assert lt.SmagorinskyCollision(0.6).native_generator().force is None
    assert lt.NoCollision().native_generator().force is None


def test_native_availability():
    flow = lt.TaylorGreenVortex(ctx(), [8, 8], 100, 0.05, lt.D2Q9())
    for scheme in (lt.Guo, lt.ShanChen):
        uniform = scheme(flow, 0.8, [1e-3, 0])
        assert uniform.native_available()
        assert lt.BGKCollision(0.8, force=uniform).native_available()
        assert lt.SmagorinskyCollision(0.8, force=uniform).native_available()
        per_node = scheme(flow, 0.8, torch.zeros(2, 8, 8))
        assert not per_node.native_available()
        assert not lt.BGKCollision(0.8, force=per_node).native_available()
        assert not lt.SmagorinskyCollision(0.8, force=per_node).native_available()
        assert not scheme(flow, 0.8, [1e-3, 0, 0]).native_available()       # three components on a 2-D lattice
    assert not lt.BGKCollision(0.8, force=object()).native_available()
    assert not lt.SmagorinskyCollision(0.8, force=object()).native_available()
    once = lt.SmagorinskyCollision(0.8, force=lt.Guo(flow, 0.8, [1e-3, 0]))
    once.iterations = 1
    assert not once.native_available()


def test_native_context_refuses_what_the_engine_has_no_kernel_for():
    """Context(use_native=True) with a force the engine cannot take raises the usual NativeEngineError (a CPU context
    told it is native: the refusal comes before anything touches a device)"""
    from lettuce_amd._native import NativeEngineError
    context = ctx("f32")
    context.use_native = True
    flow = lt.TaylorGreenVortex(context, [8, 8], 100, 0.05, lt.D2Q9())
    with pytest.raises(NativeEngineError, match="no kernel for: collision 'BGKCollision'"):
        lt.Simulation(flow, lt.BGKCollision(0.6, force=object()), [])
    per_node = lt.Guo(flow, 0.6, torch.zeros(2, 8, 8))
    with pytest.raises(NativeEngineError, match="no kernel for: collision 'BGKCollision'"):
        lt.Simulation(flow, lt.BGKCollision(0.6, force=per_node), [])
    with pytest.raises(NativeEngineError, match="no kernel for: collision 'SmagorinskyCollision'"):
        lt.Simulation(flow, lt.SmagorinskyCollision(0.6, force=per_node), [])


def test_binding_header_and_library(engine_library):
    from lettuce_amd import _native
    assert _native.SYMBOLS["lt_plan_set_force"] == (
        ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.c_double, ctypes.c_double])
    assert hasattr(_native.Plan, "set_force")
    assert _native.COLLISION_IDS == {"none": 0, "bgk": 1, "kbc": 2, "smagorinsky": 3}     # the enum is unchanged
    header = open(os.path.join(ROOT, "include", "lettuce_hip.h")).read()
    assert re.search(r"int\s+lt_plan_set_force\s*\(\s*lt_plan\s*\*\s*plan\s*,\s*const\s+double\s*\*\s*acceleration\b[^;]*"
                     r"double\s+ueq_scale\s*,\s*double\s+source_scale\s*\)\s*;", header)
    assert re.search(r"#define\s+LT_ABI_VERSION\s+2\b", header)      # one new function only
    lib = ctypes.CDLL(engine_library)
    assert hasattr(lib, "lt_plan_set_force")
    lib.lt_plan_set_force.restype = ctypes.c_int
    lib.lt_plan_set_force.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.c_double, ctypes.c_double]
    lib.lt_abi_version.restype = ctypes.c_int
    assert lib.lt_abi_version() == 2
    a = (ctypes.c_double * 3)(1e-3, 0.0, 0.0)
    assert lib.lt_plan_set_force(None, a, 0.5, 0.375) != 0           # a null plan is refused, not dereferenced
    assert lib.lt_plan_set_force(None, None, 0.5, 0.0) != 0


def test_poiseuille_flow_matches_the_reference():
    """masks, units, analytic solution and ten forced steps between the bounce-back rows"""
    g = golden("force_poiseuille2d_d2q9_f64")
    flow = lt.PoiseuilleFlow2D(ctx(), [int(r) for r in g["resolution"]], float(g["reynolds"]), float(g["mach"]), lt.D2Q9)
    assert flow.initialize_with_zeros and isinstance(flow.stencil, lt.D2Q9)
    close(flow.f.numpy(), g["f0"], "f64")
    np.testing.assert_array_equal(flow.acceleration.numpy(), g["acceleration"])
    for name, value in (("viscosity_pu", flow.units.viscosity_pu), ("viscosity_lu", flow.units.viscosity_lu),
                        ("char_length_lu", flow.units.characteristic_length_lu),
                        ("u_char_lu", flow.units.characteristic_velocity_lu),
                        ("tau", flow.units.relaxation_parameter_lu)):
        assert float(value) == pytest.approx(float(g[name]), rel=1e-15), name
    p, u = flow.analytic_solution()
    close(p.numpy(), g["analytic_p"], "f64")
    close(u.numpy(), g["analytic_u"], "f64")
    mask = flow.boundaries[0].make_no_collision_mask(flow.resolution, flow.context).numpy()
    assert mask[:, 0].all() and mask[:, -1].all() and not mask[:, 1:-1].any()
    force = lt.Guo(flow, flow.units.relaxation_parameter_lu, flow.acceleration)
    sim = lt.Simulation(flow, lt.BGKCollision(flow.units.relaxation_parameter_lu, force=force), [])
    np.testing.assert_array_equal(sim.no_collision_mask.numpy(), g["no_collision_mask"])
    np.testing.assert_array_equal(sim.no_streaming_mask.numpy(), unpack_nsm(g))
    done = 0
    for n in (1, 2, 10):
        sim(n - done)
        done = n
        close(flow.f.numpy(), g[f"f{n}"], "f64")
    close(flow.u(acceleration=force.acceleration).numpy(), g["u10"], "f64")
    analytic = lt.PoiseuilleFlow2D(ctx(), [16, 16], 10, 0.05, lt.D2Q9(), initialize_with_zeros=False)
    assert float(analytic.u().abs().max()) > 0
    assert lt.flow_by_name["poiseuille2d"][0] is lt.PoiseuilleFlow2D


def channel(context, force_class=lt.Guo, a=(1e-5, 0.0), tau=0.8, steps=4000):
    """the forced channel of the physics test: D2Q9 [4, 16], zero initial state; returns (flow, force)"""
    flow = lt.PoiseuilleFlow2D(context, [4, 16], 1, 0.05, lt.D2Q9())
    force = force_class(flow, tau, list(a)) if force_class is not None else None
    lt.Simulation(flow, lt.BGKCollision(tau, force=force), [])(steps)
    return flow, force


def parabola_error(flow, a=1e-5, tau=0.8, applied=True):
    """distance of u_x on the fluid rows from a / (2 nu) (y - 1/2) (ny - 3/2 - y), relative to the peak"""
    ny = flow.resolution[1]
    nu = (tau - 0.5) / 3
    y = torch.arange(1, ny - 1, dtype=torch.float64)
    want = a / (2 * nu) * (y - 0.5) * (ny - 1.5 - y)
    acceleration = flow.context.convert_to_tensor([a, 0.0]) if applied else None
    got = flow.u(acceleration=acceleration)[0][:, 1:-1].double().cpu()
    return float((got - want[None, :]).abs().max() / want.max())


def test_a_body_force_drives_the_parabolic_channel_profile():
    """Physics, lattice units: 4000 steps from rest with a = (1e-5, 0), tau 0.8.  The reference itself ends 2.67e-3 of
    the peak velocity from the parabola (its discretisation error at 14 fluid rows, steady from 2000 steps on); the
    bound is twice that.  Without the force the flow stays at rest: an error of 1."""
    flow, _ = channel(ctx())
    err = parabola_error(flow)
    print(f"distance from the parabola: {err:.3e} of the peak (bound 5e-3)")
    assert err < 5e-3
    at_rest, _ = channel(ctx(), force_class=None, steps=50)
    assert parabola_error(at_rest, applied=False) == pytest.approx(1.0, abs=1e-12)


# --------------------------------------------------------------------------- densities far from 1
@pytest.mark.parametrize("lat", ["D2Q9", "D3Q19", "D3Q27"])
@pytest.mark.parametrize("scheme", ["guo", "shanchen"])
def test_mirror_on_the_asymmetric_states_against_the_reference(scheme, lat):
    """rho in 0.5 .. 1.5 at tau = 0.501 (1 and 5 steps) and in 1 / 20 .. 20 at tau = 0.7 and 1.7 (tests/golden/asymmetric_*,
    oracle/gen_golden.py): the CPU path the engine tests of these states compare with"""
    from test_gpu_asymmetric_operators import _op, fixture_runs
    for what, got, want in fixture_runs(_op(f"{scheme}-bgk", "force", lat, scheme=scheme, operator="bgk"), scheme):
        print(what, end=": ")
        close(got, want, "f64")
