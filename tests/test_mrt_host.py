"""The MRT collision and the moment transforms on the host (CPU, no GPU needed): the mirror's torch path against vectors
produced by the reference's own CPU path (tests/golden/mrt_*.npz, made by tools/gen_golden_mrt.py), the reference's own
checks of its transforms, the properties that define the operator, and the plumbing that hands it to the HIP engine
(descriptor, binding, header, exported symbol, refusals).

Bounds: those of test_relaxations_host.py -- fp64 the project's 2e-14, fp32 8e-7 -- for the collided field and every
stepped snapshot alike.  Every comparison prints its largest difference before it asserts."""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest
import torch

import lettuce_amd as lt
from lettuce_amd import moments
from conftest import golden, TORCH_DT, ROOT
from test_host_api import ctx, UniformFlow
from test_relaxations_host import close, noisy

# transform -> (class, lattice tag, stencil, indices of the second-order moments)
TRANSFORMS = {"dellar": (moments.D2Q9Dellar, "d2q9", lt.D2Q9, (3, 4, 5)),
              "lallemand": (moments.D2Q9Lallemand, "d2q9", lt.D2Q9, (3, 4)),
              "hermite": (moments.D3Q27Hermite, "d3q27", lt.D3Q27, tuple(range(4, 10)))}
FIXTURES = [f"mrt_{t}_{TRANSFORMS[t][1]}_{dt}" for t in TRANSFORMS for dt in ("f64", "f32")]
SMALL = {"dellar": [8, 6], "lallemand": [8, 6], "hermite": [4, 6, 5]}


def rates_of(transform, tau):
    """the recipe of tools/gen_golden_mrt.py: 1 for the conserved moments, tau for the second-order ones, 1.05 + 0.05 k
    for the k-th remaining one"""
    cls, _, stencil, second = TRANSFORMS[transform]
    q, d = stencil().q, stencil().d
    rates, k = [], 0
    for i in range(q):
        if i <= d:
            rates.append(1.0)
        elif i in second:
            rates.append(tau)
        else:
            rates.append(1.05 + 0.05 * k)
            k += 1
    return rates


def make_collision(transform, context, rates, stencil=None):
    cls, _, stencil_cls, _ = TRANSFORMS[transform]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return lt.MRTCollision(cls(stencil or stencil_cls(), context), rates, context)


def quiet(fn, *args):
    """the two D2Q9 equilibria warn that they are experimental on every call"""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", lt.ExperimentalWarning)
        return fn(*args)


def noisy_d1q3(seed=7):
    """a D1Q3 flow (the Taylor-Green vortex has none) with 5 % noise per population"""
    flow = UniformFlow(ctx("f64"), [16], 1, 0.01, lt.D1Q3())
    g = torch.Generator().manual_seed(seed)
    flow.f = flow.f * (1 + 0.05 * (2 * torch.rand(flow.f.shape, generator=g, dtype=torch.float64) - 1))
    return flow


def fixture_flow(g, name):
    _, transform, lat, dt = name.split("_")
    flow = lt.TaylorGreenVortex(ctx(dt), [int(r) for r in g["resolution"]], float(g["reynolds"]), float(g["mach"]),
                                TRANSFORMS[transform][2]())
    flow.f = torch.tensor(g["f0"])
    return flow, transform, dt


# --------------------------------------------------------------------------- the reference's vectors
@pytest.mark.parametrize("name", FIXTURES)
def test_torch_path_matches_the_reference(name):
    """collision(flow) and f after 1, 2, 3 and 10 steps; the input is untouched"""
    g = golden(name)
    flow, transform, dt = fixture_flow(g, name)
    assert flow.f.dtype == TORCH_DT[dt]
    assert list(g["rates"]) == rates_of(transform, float(g["tau"]))
    collision = make_collision(transform, flow.context, list(g["rates"]), flow.stencil)
    assert collision.relaxation_parameters.dtype == TORCH_DT[dt]
    f0 = flow.f.clone()
    close(quiet(collision, flow).numpy(), g["collided"], dt)
    assert torch.equal(flow.f, f0)
    sim = lt.Simulation(flow, collision, [])
    for i in range(1, 11):
        quiet(sim, 1)
        if i in (1, 2, 3, 10):
            close(flow.f.numpy(), g[f"f{i}"], dt)


@pytest.mark.parametrize("transform", list(TRANSFORMS))
def test_torch_path_on_the_asymmetric_states(transform):
    """densities 0.5 - 1.5 at tau 0.501 and 1 / 20 - 20 at 0.7 and 1.7"""
    lat = TRANSFORMS[transform][1]
    g, states = golden(f"asymmetric_mrt_{transform}_{lat}_f64"), golden(f"asymmetric_states_{lat}_f64")
    res = [int(r) for r in states["resolution"]]
    for kind, tau, steps in (("moderate", 0.501, (1, 5)), ("wide", 0.7, (1,)), ("wide", 1.7, (1,))):
        key = f"{kind}_tau{tau}"
        flow = lt.TaylorGreenVortex(ctx("f64"), res, 1600, 0.1, TRANSFORMS[transform][2]())
        flow.f = torch.tensor(states[f"f0_{kind}"])
        collision = make_collision(transform, flow.context, list(g[f"{key}_rates"]), flow.stencil)
        scale = max(1.0, float(np.abs(g[f"{key}_collided"]).max()))
        print(key, end=": ")
        close(quiet(collision, flow).numpy() / scale, g[f"{key}_collided"] / scale, "f64")
        sim, done = lt.Simulation(flow, collision, []), 0
        for n in steps:
            quiet(sim, n - done)
            done = n
            print(f"{key} f{n}", end=": ")
            close(flow.f.numpy() / scale, g[f"{key}_f{n}"] / scale, "f64")


# --------------------------------------------------------------------------- the transforms
ALL_TRANSFORMS = [(moments.D1Q3Transform, lt.D1Q3), (moments.D2Q9Dellar, lt.D2Q9), (moments.D2Q9Lallemand, lt.D2Q9),
                  (moments.D3Q27Hermite, lt.D3Q27)]


@pytest.mark.parametrize("cls,stencil", ALL_TRANSFORMS, ids=[c.__name__ for c, _ in ALL_TRANSFORMS])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_matrix_times_inverse_is_the_identity(cls, stencil, dt):
    transform = cls(stencil(), ctx(dt))
    assert transform.matrix.dtype == TORCH_DT[dt] and list(transform.matrix.shape) == [stencil().q] * 2
    assert stencil in cls.supported_stencils and len(transform.names) == stencil().q
    product = (transform.matrix.double() @ transform.inverse.double()).numpy()
    err = float(np.abs(product - np.eye(stencil().q)).max())
    print(f"max |M M^-1 - I| {err:.2e}")
    assert err <= (1e-14 if dt == "f64" else 2e-6)
    f = torch.rand([stencil().q] + [3] * stencil().d, dtype=TORCH_DT[dt])
    back = transform.inverse_transform(transform.transform(f))
    assert float((back - f).abs().max()) <= (1e-14 if dt == "f64" else 1e-5)


def test_getitem_by_names():
    m = moments.D2Q9Lallemand(lt.D2Q9(), ctx())
    assert m["jx", "jy"] == [1, 2]
    assert m["rho"] == [0]
    assert moments.Transform(lt.D2Q9(), ctx()).names == [f"m{i}" for i in range(9)]


@pytest.mark.parametrize("cls", [moments.D2Q9Dellar, moments.D2Q9Lallemand])
def test_conserved_moments_d2q9(cls):
    m = moments.moment_tensor(np.array(lt.D2Q9().e), np.array([[0, 0], [1, 0], [0, 1]]))
    assert m == pytest.approx(cls.matrix[:3, :])
    t = moments.moment_tensor(torch.tensor(lt.D2Q9().e), torch.tensor([[0, 0], [1, 0], [0, 1]]))
    assert np.array_equal(t.numpy(), m)


@pytest.mark.parametrize("cls,stencil,names", [
    (moments.D2Q9Dellar, lt.D2Q9, None),
    (moments.D2Q9Lallemand, lt.D2Q9, ("rho", "jx", "jy", "qx", "qy")),
    (moments.D3Q27Hermite, lt.D3Q27, ("rho", "jx", "jy", "jz", "Pi_xx", "Pi_xy", "PI_xz", "PI_yy", "PI_yz", "PI_zz"))],
    ids=["dellar", "lallemand", "hermite"])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_moment_equilibrium_as_the_reference_checks_it(cls, stencil, names, dt):
    """transform(feq) against equilibrium(transform(f)) on the moments the reference's tests name, abs 1e-5"""
    context = ctx(dt)
    transform = cls(stencil(), context)
    flow = UniformFlow(context, 10, 1, 0.1, stencil=stencil())
    meq1 = transform.transform(flow.equilibrium(flow)).numpy()
    expect = lt.ExperimentalWarning if stencil is lt.D2Q9 else None
    if expect is None:
        meq2 = transform.equilibrium(transform.transform(flow.f), flow).numpy()
    else:
        with pytest.warns(expect):
            meq2 = transform.equilibrium(transform.transform(flow.f), flow).numpy()
    same = slice(None) if names is None else transform[names]
    err = float(np.abs(meq1[same] - meq2[same]).max())
    print(f"max |difference| {err:.2e}")
    assert meq1[same] == pytest.approx(meq2[same], abs=1e-5)


def test_base_class_equilibrium_warns_and_goes_through_the_flow():
    flow = noisy("f64", [8, 6], lt.D2Q9)
    base = moments.Transform(lt.D2Q9(), flow.context)
    with pytest.warns(lt.InefficientCodeWarning):
        meq = base.equilibrium(flow.f, flow)
    assert torch.equal(meq, flow.equilibrium(flow))
    d1 = moments.D1Q3Transform(lt.D1Q3(), flow.context)
    flow1 = noisy_d1q3()
    with pytest.warns(lt.InefficientCodeWarning):
        meq = d1.equilibrium(d1.transform(flow1.f), flow1)
    assert float((meq - d1.transform(flow1.equilibrium(flow1))).abs().max()) < 1e-14


def test_default_moment_transform():
    context = ctx()
    assert type(moments.get_default_moment_transform(lt.D1Q3(), context)) is moments.D1Q3Transform
    assert type(moments.get_default_moment_transform(lt.D2Q9(), context)) is moments.D2Q9Lallemand
    assert type(moments.get_default_moment_transform(lt.D2Q9, context)) is moments.D2Q9Lallemand
    with pytest.raises(lt.LettuceException, match="No default moment transform"):
        moments.get_default_moment_transform(lt.D3Q27(), context)
    assert not hasattr(lt, "D2Q9Lallemand")                # not star-imported, as in the reference


# --------------------------------------------------------------------------- properties
@pytest.mark.parametrize("transform", list(TRANSFORMS))
def test_mass_and_momentum_are_conserved(transform):
    flow = noisy("f64", SMALL[transform], TRANSFORMS[transform][2])
    collision = make_collision(transform, flow.context, rates_of(transform, 0.6))
    rho, j = flow.rho().clone(), flow.j().clone()
    flow.f = quiet(collision, flow)
    # exact in real arithmetic; in fp64 each of the q moments and each of the q rebuilt populations is a sum of q
    # products, every one rounded to 2^-53 of a value that the entries of M (up to 9) and M^-1 keep within 9 max(rho):
    # 2 q^2 roundings of 9 * 2^-53 max(rho) bound the drift of the two sums over q
    q = flow.stencil.q
    bound = 2 * q * q * 9 * 2.0 ** -53 * float(rho.abs().max())
    errs = float((flow.rho() - rho).abs().max()), float((flow.j() - j).abs().max())
    print(f"mass {errs[0]:.2e}, momentum {errs[1]:.2e} (bound {bound:.2e})")
    assert errs[0] <= bound and errs[1] <= bound


@pytest.mark.parametrize("tau", [0.51, 0.8, 1.7])
def test_dellar_with_equal_rates_is_bgk(tau):
    """Dellar's equilibrium moments are those of the quadratic equilibrium: with one rate MRT is BGK up to rounding"""
    flow = noisy("f64", [8, 6], lt.D2Q9)
    collision = make_collision("dellar", flow.context, [tau] * 9)
    err = float((quiet(collision, flow) - lt.BGKCollision(tau)(flow)).abs().max())
    print(f"tau {tau}: {err:.2e}")
    assert err <= 2e-14


def test_rates_assigned_after_construction_are_read_on_the_next_call():
    flow = noisy("f64", [8, 6], lt.D2Q9)
    collision = make_collision("lallemand", flow.context, rates_of("lallemand", 0.7))
    first = quiet(collision, flow)
    desc = collision.native_generator()
    assert desc.rates(flow) == tuple(rates_of("lallemand", 0.7))
    new = rates_of("lallemand", 0.9)[::-1]
    collision.relaxation_parameters = flow.context.convert_to_tensor(new)
    second = quiet(collision, flow)
    assert float((first - second).abs().max()) > 1e-4
    fresh = make_collision("lallemand", flow.context, new)
    assert torch.equal(second, quiet(fresh, flow))
    assert desc.rates(flow) == tuple(new)                                     # the descriptor reads late as well
    # in fp32 the rates are the fp32 values, as the reference's tensor holds them
    c32 = make_collision("lallemand", ctx("f32"), [0.7] * 9)
    assert c32.native_generator().rates(flow) == (float(np.float32(0.7)),) * 9


# --------------------------------------------------------------------------- plumbing
def test_descriptor_and_native_availability():
    context = ctx()
    for transform, (cls, _, stencil, _) in TRANSFORMS.items():
        collision = make_collision(transform, context, rates_of(transform, 0.7))
        assert isinstance(collision, lt.Collision) and lt.ext.MRTCollision is lt.MRTCollision
        assert collision.native_available()
        desc = collision.native_generator()
        assert isinstance(desc, lt.native_desc.NativeCollision) and desc.kind == "mrt"
        assert desc.transform == cls.__name__
        rates = desc.rates(None)
        assert isinstance(rates, tuple) and all(isinstance(r, float) for r in rates) and len(rates) == stencil().q
        hash(rates)                                                            # part of the steppers' carry key
        assert desc.constant is None and desc.tau_minus is None and desc.force is None
    for other in (lt.BGKCollision(0.6), lt.TRTCollision(0.6), lt.SmagorinskyCollision(0.6)):
        desc = other.native_generator()
        assert desc.transform is None and desc.rates is None


def test_an_unknown_transform_is_not_native():
    context = ctx()

    class Mine(moments.D2Q9Dellar):                        # a subclass may override the equilibrium
        pass

    assert not lt.MRTCollision(Mine(lt.D2Q9(), context), [1.0] * 9, context).native_available()
    assert not lt.MRTCollision(moments.D1Q3Transform(lt.D1Q3(), context), [1.0] * 3, context).native_available()
    assert not lt.MRTCollision(moments.Transform(lt.D2Q9(), context), [1.0] * 9, context).native_available()
    # a transform on a lattice that is not its own
    assert not lt.MRTCollision(moments.D2Q9Dellar(lt.D3Q27(), context), [1.0] * 9, context).native_available()
    # ... and such an operator still runs on the torch path, D1Q3 through the base class's equilibrium
    flow = noisy_d1q3()
    collision = lt.MRTCollision(moments.D1Q3Transform(lt.D1Q3(), flow.context), [1.0, 1.0, 0.8], flow.context)
    with pytest.warns(lt.InefficientCodeWarning):
        out = collision(flow)
    assert float((out - lt.BGKCollision(0.8)(flow)).abs().max()) < 1e-14     # one free moment: BGK at its rate


def _plan_desc(_native, stencil, collision, shape):
    d = _native._PlanDesc()
    d.abi_version, d.stencil, d.dtype, d.collision = 2, _native.STENCIL_IDS[stencil], 1, collision
    d.layout, d.ghost_planes, d.dims, d.n_boundaries = 0, 0, len(shape), 0
    for a in range(3):
        d.shape[a] = shape[a] if a < len(shape) else 1
    return d


def check_plan_refusals(lib, _native):
    """the refusals of lt_plan_set_mrt and of an MRT plan, each with its status and message; needs a device (a plan).
    Shared with tests/test_gpu_mrt.py."""
    INVALID, UNSUPPORTED = 1, 2
    lib.lt_last_error.restype = ctypes.c_char_p
    dbl = ctypes.c_double

    def create(stencil, collision, shape):
        handle = ctypes.c_void_p()
        rc = lib.lt_plan_create(ctypes.byref(_plan_desc(_native, stencil, collision, shape)), ctypes.byref(handle))
        assert rc == 0, lib.lt_last_error()
        return handle

    def refused(rc, status, text):
        message = lib.lt_last_error().decode()
        print(f"{rc}: {message}")
        assert rc == status and text in message, (rc, message)

    nine, twenty_seven = (dbl * 9)(*([1.0] * 9)), (dbl * 27)(*([1.0] * 27))
    bgk = create("D2Q9", 1, [8, 8])
    refused(lib.lt_plan_set_mrt(bgk, 1, nine, 9), INVALID, "not MRT")
    plan = create("D2Q9", 10, [8, 8])
    refused(lib.lt_plan_set_mrt(plan, 3, twenty_seven, 27), INVALID, "belongs to D3Q27")
    refused(lib.lt_plan_set_mrt(plan, 0, nine, 9), INVALID, "MRT transform 0")
    refused(lib.lt_plan_set_mrt(plan, 1, nine, 8), INVALID, "8 relaxation rates")
    refused(lib.lt_plan_set_mrt(plan, 2, twenty_seven, 27), INVALID, "27 relaxation rates")
    refused(lib.lt_plan_set_mrt(plan, 1, None, 9), INVALID, "null relaxation rates")
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        rates = (dbl * 9)(*([1.0] * 8 + [bad]))
        refused(lib.lt_plan_set_mrt(plan, 1, rates, 9), INVALID, "finite and > 0")
    big = create("D3Q27", 10, [4, 4, 4])
    refused(lib.lt_plan_set_mrt(big, 1, nine, 9), INVALID, "belongs to D2Q9")
    refused(lib.lt_plan_set_mrt(big, 2, nine, 9), INVALID, "belongs to D2Q9")
    # before lt_plan_set_mrt: collide and run are refused (the buffers are never touched)
    f = ctypes.c_void_p(0x1000)
    g = ctypes.c_void_p(0x2000)
    lib.lt_collide.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, dbl, ctypes.c_void_p]
    refused(lib.lt_collide(plan, f, g, 1.0, None), INVALID, "lt_plan_set_mrt must give")
    which = ctypes.c_int32(0)
    lib.lt_run.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, dbl, ctypes.c_int64, ctypes.c_void_p,
                           ctypes.POINTER(ctypes.c_int32)]
    refused(lib.lt_run(plan, f, g, 1.0, 3, None, ctypes.byref(which)), INVALID, "lt_plan_set_mrt must give")
    assert lib.lt_plan_set_mrt(plan, 2, nine, 9) == 0
    refused(lib.lt_plan_set_two_step(plan, 1, 0), UNSUPPORTED, "MRT collision has the one-step kernels only")
    assert lib.lt_plan_set_two_step(plan, -1, 0) == 0 and lib.lt_plan_set_two_step(plan, 0, 0) == 0
    assert lib.lt_plan_two_step_admitted(plan) == UNSUPPORTED
    assert b"MRT collision has the one-step kernels only" in lib.lt_last_error()
    for p in (bgk, plan, big):
        lib.lt_plan_destroy(p)


def test_binding_header_and_library(engine_library):
    from lettuce_amd import _native
    assert _native.SYMBOLS["lt_plan_set_mrt"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32,
                                                                 ctypes.POINTER(ctypes.c_double), ctypes.c_int32])
    assert hasattr(_native.Plan, "set_mrt")
    assert _native.MRT_COLLISION_IDS == {"mrt": 10}
    assert _native.MRT_TRANSFORM_IDS == {"D2Q9Dellar": 1, "D2Q9Lallemand": 2, "D3Q27Hermite": 3}
    header = open(os.path.join(ROOT, "include", "lettuce_hip.h")).read()
    assert re.search(r"\bLT_COLLISION_MRT\s*=\s*10\b", header)
    assert re.search(r"\bLT_MRT_D2Q9_DELLAR\s*=\s*1\b", header)
    assert re.search(r"\bLT_MRT_D2Q9_LALLEMAND\s*=\s*2\b", header)
    assert re.search(r"\bLT_MRT_D3Q27_HERMITE\s*=\s*3\b", header)
    assert re.search(r"int\s+lt_plan_set_mrt\s*\(\s*lt_plan\s*\*\s*plan\s*,\s*int\s+transform\s*,\s*const\s+double\s*\*\s*"
                     r"relaxation\s*,\s*int\s+count\s*\)\s*;", header)
    assert re.search(r"#define\s+LT_ABI_VERSION\s+2\b", header)
    assert "NOT read by an MRT plan" in header
    lib = ctypes.CDLL(engine_library)
    lib.lt_plan_set_mrt.restype = ctypes.c_int
    lib.lt_plan_set_mrt.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.c_int]
    lib.lt_abi_version.restype = ctypes.c_int
    assert lib.lt_abi_version() == 2
    lib.lt_last_error.restype = ctypes.c_char_p
    rates = (ctypes.c_double * 9)(*([1.0] * 9))
    assert lib.lt_plan_set_mrt(None, 1, rates, 9) == 1                        # LT_ERR_INVALID: refused, not dereferenced
    assert b"null plan" in lib.lt_last_error()
    # plan creation on a lattice without a transform: LT_ERR_UNSUPPORTED before any device is touched
    for stencil, shape in (("D3Q19", [4, 4, 4]), ("D3Q15", [4, 4, 4]), ("D1Q3", [8])):
        handle = ctypes.c_void_p()
        rc = lib.lt_plan_create(ctypes.byref(_plan_desc(_native, stencil, 10, shape)), ctypes.byref(handle))
        assert rc == 2 and b"MRT collision exists for D2Q9" in lib.lt_last_error(), (rc, lib.lt_last_error())
        assert handle.value is None
    # the refusals that need a plan need a device (LT_ERR_ALLOC without one); tests/test_gpu_mrt.py runs them there
    handle = ctypes.c_void_p()
    rc = lib.lt_plan_create(ctypes.byref(_plan_desc(_native, "D2Q9", 10, [8, 8])), ctypes.byref(handle))
    if rc == 0:
        lib.lt_plan_destroy(handle)
        check_plan_refusals(lib, _native)
    else:
        assert rc == 4 and not torch.cuda.is_available(), (rc, lib.lt_last_error())


def test_slab_driver_refuses_an_engine_without_set_mrt():
    class Engine:                                                    # no set_mrt
        pass

    context = ctx("f32")
    slab = lt.ZSlab([8, 8, 8], 0, 1)
    flow = lt.TaylorGreenVortex(context, slab.extended_resolution, 100, 0.05, lt.D3Q27(), slab=slab)
    with pytest.raises(lt.LettuceException, match="has no mrt collision"):
        lt.SlabSimulation(flow, make_collision("hermite", context, rates_of("hermite", 0.7)), slab, engine=Engine())


def test_native_simulation_refuses_an_unknown_transform(engine_library):
    """what Simulation does for any component whose native_available() is false: the torch path takes it, a native
    context names it and raises"""
    flow = noisy_d1q3()
    collision = lt.MRTCollision(moments.D1Q3Transform(lt.D1Q3(), flow.context), [1.0, 1.0, 0.8], flow.context)
    sim = lt.Simulation(flow, collision, [])
    with pytest.warns(lt.InefficientCodeWarning):
        sim(1)
    flow2 = noisy_d1q3()
    flow2.context.use_native = True                   # as if a GPU context had been requested
    with pytest.raises(lt.LettuceException, match="collision 'MRTCollision'"):
        lt.Simulation(flow2, collision, [])
