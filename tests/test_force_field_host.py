"""Per-node body forces on the host (CPU, no GPU needed): ``GuoField`` / ``ShanChenField`` -- the two schemes with an
acceleration ``[d, *resolution]`` -- against the uniform classes, against the momentum they must add per node, and in
the Kolmogorov flow they drive; and the plumbing that hands a field to the HIP engine (descriptor, per-batch settings,
binding, header, exported symbol, refusals by name).

Bounds: 1e-14 in fp64 where two evaluations of the same formula differ in the order of a sum of at most three terms
(scaled by max(1, |f|max)) and for the momentum of a node, whose populations are O(1) and whose change is O(1e-3); the
Kolmogorov flow's bounds are the discretisation error of the scheme at 16 and 32 nodes per wave (1.64e-2 and 4.11e-3,
second order), measured on this CPU path."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import lettuce_amd as lt
from conftest import ROOT
from test_gpu_paths_vs_oracle import perturbed_state
from test_host_api import UniformFlow, ctx

UNIFORM = (2e-3, -3e-3, 1e-3)
GRIDS = [("D2Q9", [12, 10]), ("D3Q19", [6, 5, 8])]
STENCILS = {"D2Q9": lt.D2Q9, "D3Q19": lt.D3Q19}
SCHEMES = {"guo": (lt.Guo, lt.GuoField), "shanchen": (lt.ShanChen, lt.ShanChenField)}


def state(lat, res, seed=11):
    flow = UniformFlow(ctx("f64"), list(res), 1, 0.01, STENCILS[lat]())
    flow.f = perturbed_state(lat, list(res), torch.float64, seed)
    return flow


def random_field(res, seed=5, amplitude=3e-3, dtype=torch.float64):
    """a field without symmetries: uniform noise in [-1, 1) times `amplitude` and three different component scales"""
    g = torch.Generator().manual_seed(seed)
    d = len(res)
    scale = torch.tensor([1.0, -0.6, 0.35][:d], dtype=torch.float64).reshape([d] + [1] * d)
    return (amplitude * scale * (2 * torch.rand([d] + list(res), generator=g, dtype=torch.float64) - 1)).to(dtype)


def operator(name, tau, force):
    return lt.BGKCollision(tau, force=force) if name == "bgk" else lt.SmagorinskyCollision(tau, 1.0, force=force)


# --------------------------------------------------------------------------- 1: a constant field is the uniform class
@pytest.mark.parametrize("name", ["bgk", "smagorinsky"])
@pytest.mark.parametrize("scheme", list(SCHEMES))
@pytest.mark.parametrize("lat,res", GRIDS)
def test_constant_field_agrees_with_the_uniform_class(lat, res, scheme, name):
    flow = state(lat, res)
    uniform, field = SCHEMES[scheme]
    tau = 0.8 if name == "bgk" else 0.51
    a = torch.tensor(UNIFORM[:len(res)], dtype=torch.float64)
    expanded = a.reshape([-1] + [1] * len(res)).expand([len(res)] + res)
    want = operator(name, tau, uniform(flow, tau, a))(flow)
    got = operator(name, tau, field(flow, tau, expanded))(flow)
    unforced = operator(name, tau, None)(flow)
    bound = 1e-14 * max(1.0, float(want.abs().max()))
    print(f"max |difference| {float((got - want).abs().max()):.3e} (bound {bound:.1e}); distance from the unforced "
          f"operator {float((want - unforced).abs().max()):.2e}")
    assert float((want - unforced).abs().max()) > 1e-4
    assert float((got - want).abs().max()) <= bound


# --------------------------------------------------------------------------- 2: the momentum a node receives
@pytest.mark.parametrize("scheme", list(SCHEMES))
@pytest.mark.parametrize("lat,res", GRIDS)
def test_one_collision_adds_the_nodes_own_acceleration(lat, res, scheme):
    """BGK conserves mass and, with either scheme, adds exactly a(x) to the momentum of node x: Guo a / (2 tau) through
    the shifted equilibrium and a (1 - 1 / (2 tau)) through the source term, Shan-Chen (1 / tau) tau a through the
    equilibrium alone"""
    flow = state(lat, res, seed=13)
    tau = 0.8
    a = random_field(res)
    assert len({round(float(a[c].abs().max()), 6) for c in range(len(res))}) == len(res)
    f0 = flow.f.clone()
    df = lt.BGKCollision(tau, force=SCHEMES[scheme][1](flow, tau, a))(flow) - f0
    e = flow.torch_stencil.e.to(torch.float64)
    momentum = torch.stack([(e[:, c].reshape([-1] + [1] * len(res)) * df).sum(dim=0) for c in range(len(res))])
    mass = df.sum(dim=0)
    print(f"max |sum_q e_q df - a(x)| {float((momentum - a).abs().max()):.3e}, max |sum_q df| "
          f"{float(mass.abs().max()):.3e} (bounds 1e-14)")
    assert float((momentum - a).abs().max()) <= 1e-14
    assert float(mass.abs().max()) <= 1e-14


# --------------------------------------------------------------------------- 3: Kolmogorov flow
KOLMOGOROV_TAU, KOLMOGOROV_A = 0.8, 1e-6


def kolmogorov(context, n, force_class=None):
    """(flow, force, simulation, steps, laminar profile u_x [n, n] in lattice units) of the forced box at tau = 0.8 with
    A = 1e-6: int(12 / (nu k^2)) steps from rest, twelve viscous times of the forced wave"""
    force_class = lt.GuoField if force_class is None else force_class
    flow = lt.KolmogorovFlow2D(context, [n, n], 1.0, 0.05)
    nu, k = (KOLMOGOROV_TAU - 0.5) / 3, 2 * math.pi / n
    sine = torch.sin(k * torch.arange(n, dtype=torch.float64))[None, :].expand(n, n)
    a = torch.zeros(2, n, n, dtype=torch.float64)
    a[0] = KOLMOGOROV_A * sine
    force = force_class(flow, KOLMOGOROV_TAU, a)
    sim = lt.Simulation(flow, lt.BGKCollision(KOLMOGOROV_TAU, force=force), [])
    return flow, force, sim, int(12 / (nu * k * k)), KOLMOGOROV_A / (nu * k * k) * sine


def kolmogorov_error(flow, force, profile):
    """(relative L2 distance of u_x = j_x / rho + a_x / (2 rho) from the laminar profile, max |u_y|)"""
    rho = flow.rho()[0].double().cpu()
    u = (flow.j() / flow.rho()).double().cpu() + force.acceleration.double().cpu() / (2 * rho)
    return float(((u[0] - profile) ** 2).sum().sqrt() / (profile ** 2).sum().sqrt()), float(u[1].abs().max())


def test_kolmogorov_flow_reaches_the_laminar_profile_at_second_order():
    errors = {}
    for n, steps_want in ((16, 778), (32, 3112)):
        flow, force, sim, steps, profile = kolmogorov(ctx("f64"), n)
        assert steps == steps_want
        sim(steps)
        errors[n], uy = kolmogorov_error(flow, force, profile)
        print(f"[{n}, {n}], {steps} steps: relative L2 error {errors[n]:.3e}, max |u_y| {uy:.2e}")
        assert uy < 1e-12
    ratio = errors[16] / errors[32]
    print(f"ratio {ratio:.3f}")
    assert errors[16] < 2e-2
    assert 3.5 < ratio < 4.5


def test_kolmogorov_flow_units_force_and_analytic_solution():
    flow = lt.KolmogorovFlow2D(ctx("f64"), [12, 16], 10.0, 0.05, wavenumber=2)
    assert isinstance(flow.stencil, lt.D2Q9) and flow.resolution == [12, 16] and flow.boundaries == []
    p, u = flow.initial_pu()
    assert list(p.shape) == [1, 12, 16] and list(u.shape) == [2, 12, 16] and not p.any() and not u.any()
    np.testing.assert_allclose(flow.rho().numpy(), 1.0, rtol=0, atol=1e-15)
    k = 2 * math.pi * 2 / 16
    amplitude = float(flow.units.characteristic_velocity_lu * flow.units.viscosity_lu * k ** 2)
    a = flow.acceleration_lu()
    assert list(a.shape) == [2, 12, 16] and a.is_contiguous() and a.dtype == torch.float64
    want = amplitude * torch.sin(k * torch.arange(16, dtype=torch.float64))
    np.testing.assert_allclose(a[0].numpy(), want[None, :].expand(12, 16).numpy(), rtol=0, atol=1e-18)
    assert not a[1].any()
    # the laminar steady state peaks at the characteristic velocity, in physical units
    p, u = flow.analytic_solution(3.0)
    assert not p.any() and not u[1].any()
    np.testing.assert_allclose(u[0].numpy(), (want / amplitude)[None, :].expand(12, 16).numpy(), rtol=0, atol=1e-15)
    np.testing.assert_allclose(flow.units.convert_velocity_to_lu(u[0]).numpy(),
                               (want / (flow.units.viscosity_lu * k ** 2))[None, :].expand(12, 16).numpy(), rtol=1e-13)
    assert lt.ext.KolmogorovFlow2D is lt.KolmogorovFlow2D
    with pytest.raises(lt.LettuceException, match="wavenumber"):
        lt.KolmogorovFlow2D(ctx("f64"), [8, 8], 10.0, 0.05, wavenumber=0)


# --------------------------------------------------------------------------- 4: availability, descriptor, refusals
def test_native_availability_and_the_setter():
    flow = lt.TaylorGreenVortex(ctx(), [8, 6], 100, 0.05, lt.D2Q9())
    for uniform, field in SCHEMES.values():
        force = field(flow, 0.8, torch.zeros(2, 8, 6))
        assert isinstance(force, uniform) and isinstance(force, lt.Force)
        assert force.native_available() and force.acceleration.dtype == torch.float64
        assert lt.BGKCollision(0.8, force=force).native_available()
        assert lt.SmagorinskyCollision(0.8, force=force).native_available()
        once = lt.SmagorinskyCollision(0.8, force=force)
        once.iterations = 1
        assert not once.native_available()
        kept = force.acceleration
        kept[0, 1, 2] = 1e-3                                          # edited in place: the same tensor
        assert force.acceleration is kept
        force.acceleration = np.zeros((2, 8, 6), dtype=np.float32)    # converted once
        assert force.acceleration.dtype == torch.float64 and force.acceleration is not kept
        wrong = field(flow, 0.8, torch.zeros(2, 8, 7))                # a wrong extent constructs and is not available
        assert not wrong.native_available()
        assert not lt.BGKCollision(0.8, force=wrong).native_available()
        for bad in ([1e-3, 0.0], torch.zeros(3, 8, 6), torch.zeros(2, 8, 6, 1)):
            with pytest.raises(lt.LettuceException, match=r"\[d, \*resolution\]"):
                field(flow, 0.8, bad)
            with pytest.raises(lt.LettuceException, match=r"\[d, \*resolution\]"):
                force.acceleration = bad
    assert lt.BGKCollision(0.8, force=lt.GuoField(flow, 0.8, torch.zeros(2, 8, 6))).name() == "BGKCollision_GuoField"
    assert lt.ext.GuoField is lt.GuoField and lt.ext.ShanChenField is lt.ShanChenField


def test_descriptor_and_its_per_batch_calls():
    from lettuce_amd.native_desc import CollisionSettings, FieldRef, NativeForce
    flow = lt.TaylorGreenVortex(ctx(), [8, 6], 100, 0.05, lt.D2Q9())
    a = torch.zeros(2, 8, 6, dtype=torch.float64)
    guo = lt.GuoField(flow, 0.8, a)
    desc = lt.SmagorinskyCollision(0.6, 0.2, force=guo).native_generator()
    assert desc.kind == "smagorinsky" and isinstance(desc.force, NativeForce) and desc.force.kind == "guo"
    assert desc.force.field() is a and desc.force.acceleration is None
    settings = desc.settings(flow)
    assert settings.force is None and settings == CollisionSettings(smagorinsky=0.2, force_field=(FieldRef(a), 0.5, 1 - 1 / 1.6))
    calls = settings.calls()
    assert [name for name, _ in calls] == ["set_smagorinsky", "set_force_field"] == list(settings.setters)
    assert calls[1][1][0] is a and calls[1][1][1:] == (0.5, 1 - 1 / 1.6)
    assert hash(settings) == hash(desc.settings(flow)) and settings == desc.settings(flow)
    # read late: an edit in place, a new tensor and a new tau each give another record
    a[0, 0, 0] = 1e-3
    edited = desc.settings(flow)
    assert edited != settings and edited.calls()[1][1][0] is a
    b = torch.zeros(2, 8, 6, dtype=torch.float64)
    guo.acceleration = b
    replaced = desc.settings(flow)
    assert replaced != edited and replaced.calls()[1][1][0] is b
    guo.tau = 0.6
    assert desc.settings(flow).force_field[1:] == (0.5, 1 - 1 / 1.2)
    shan = lt.ShanChenField(flow, 0.7, a)
    desc = lt.BGKCollision(0.8, force=shan).native_generator()
    assert desc.force.kind == "shan_chen" and desc.settings(flow).force_field[1:] == (0.7, 0.0)
    shan.tau = 0.9
    assert desc.settings(flow).force_field[1] == 0.9
    # the uniform classes hand over what they handed over before
    uniform = lt.BGKCollision(0.8, force=lt.Guo(flow, 0.8, [1e-3, 0.0])).native_generator().settings(flow)
    assert uniform.force_field is None and uniform.setters == ("set_force",)
    # the arguments are those of Plan.set_force_field, by position
    import inspect
    from lettuce_amd._native import Plan
    bound = inspect.signature(Plan.set_force_field).bind(None, *calls[1][1])
    assert list(bound.arguments)[1:] == ["field", "ueq_scale", "source_scale"]


def test_slab_simulations_refuse_a_force_field_by_name():
    from slab_cpu_engine import OracleSlabEngine
    slab = lt.ZSlab([8, 4, 6], 0, 1)
    flow = lt.TaylorGreenVortex(ctx("f64"), slab.extended_resolution, 400, 0.1, lt.D3Q19(), slab=slab)
    for field in (lt.GuoField, lt.ShanChenField):
        collision = lt.BGKCollision(0.6, force=field(flow, 0.6, torch.zeros([3] + list(flow.resolution))))
        for driver in (lt.SlabSimulation, lt.TwoStepSlabSimulation):
            with pytest.raises(lt.LettuceException, match=f"force field '{field.__name__}' has no slab kernel"):
                driver(flow, collision, slab, engine=OracleSlabEngine("D3Q19", torch.float64, "bgk"))


def test_native_context_refuses_outlets_and_the_incompressible_equilibrium_by_name():
    """a CPU context told it is native: the refusal comes before anything touches a device"""
    from lettuce_amd._native import NativeEngineError
    context = ctx("f32")
    context.use_native = True
    flow = lt.Obstacle(context, [16, 8], 100, 0.1, domain_length_x=2)
    force = lt.GuoField(flow, 0.6, torch.zeros(2, 16, 8))
    with pytest.raises(NativeEngineError, match="no kernel for: force field 'GuoField' with the outlet "
                                                "'AntiBounceBackOutlet'"):
        lt.Simulation(flow, lt.BGKCollision(0.6, force=force), [])
    flow = lt.TaylorGreenVortex(context, [8, 8], 100, 0.05, lt.D2Q9(), equilibrium=lt.IncompressibleQuadraticEquilibrium())
    force = lt.ShanChenField(flow, 0.6, torch.zeros(2, 8, 8))
    with pytest.raises(NativeEngineError, match="no kernel for: force field 'ShanChenField' with equilibrium "
                                                "'IncompressibleQuadraticEquilibrium'"):
        lt.Simulation(flow, lt.BGKCollision(0.6, force=force), [])
    wrong = lt.GuoField(flow, 0.6, torch.zeros(2, 8, 7))
    with pytest.raises(NativeEngineError, match="no kernel for: collision 'BGKCollision'"):
        lt.Simulation(flow, lt.BGKCollision(0.6, force=wrong), [])


# --------------------------------------------------------------------------- 5: header, binding, library
def test_binding_header_and_library(engine_library):
    from lettuce_amd import _native
    assert _native.SYMBOLS["lt_plan_set_force_field"] == (
        ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.c_double])
    assert hasattr(_native.Plan, "set_force_field")
    assert _native.COLLISION_IDS == {"none": 0, "bgk": 1, "kbc": 2, "smagorinsky": 3}     # the enum is unchanged
    header = open(os.path.join(ROOT, "include", "lettuce_hip.h")).read()
    assert re.search(r"int\s+lt_plan_set_force_field\s*\(\s*lt_plan\s*\*\s*plan\s*,\s*const\s+void\s*\*\s*acceleration\b[^;]*"
                     r"double\s+ueq_scale\s*,\s*double\s+source_scale\s*\)\s*;", header)
    assert "NOT VALIDATED" in header
    assert re.search(r"#define\s+LT_ABI_VERSION\s+2\b", header)      # one new function only
    lib = ctypes.CDLL(engine_library)
    assert hasattr(lib, "lt_plan_set_force_field")
    lib.lt_plan_set_force_field.restype = ctypes.c_int
    lib.lt_plan_set_force_field.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.c_double]
    lib.lt_abi_version.restype = ctypes.c_int
    assert lib.lt_abi_version() == 2
    assert lib.lt_plan_set_force_field(None, None, 0.5, 0.375) != 0  # a null plan is refused, not dereferenced
    assert lib.lt_plan_set_force_field(None, ctypes.c_void_p(4096), 0.5, 0.375) != 0
