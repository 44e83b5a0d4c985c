"""Per-node body forces of the HIP engine (lt_plan_set_force_field; the kernels' COLL 37 and 39), in the manner of
test_gpu_force.py.

Two references.  A field that is constant in space against the kernels of the uniform force (lt_plan_set_force), bit for
bit: the field kernels form the node's velocity shift with the product the host forms for the uniform force.  And a
random field without symmetries -- three different component scales, asymmetric grids -- against the mirror's torch
path of ``GuoField`` / ``ShanChenField`` on a CPU context in float64 (pinned by test_force_field_host.py), stepping the
same initial state, with the plan's boundaries through the oracle's boundary operators.

Tolerances are test_gpu_force.py's: ATOL 1e-12 / 1e-5 times max(1, |f|max), times max(1, n / 10) in fp32; the fp32
error budget is test_gpu_fp32_error_budget.py's gate, E_gpu <= 4 E_ref.  Every comparison prints its largest difference
before it asserts.

The cases of a lattice run inside one test function (both dtypes, the three (scheme, operator) pairs), each named in
what it prints and in the message of its assertion: the suite runs again for every later change, and a test function
per combination would be some ninety of them here.
"""
import functools

import numpy as np
import pytest
import torch

import lettuce_amd as lt
from conftest import TORCH_DT
from oracle import lettuce_oracle as orc
from test_gpu_engine import ATOL, _masked_case, dev, plan_for
from test_gpu_paths_vs_oracle import _oracle_boundary, expected_launches, perturbed_state
from test_gpu_smagorinsky import SMALL, STENCILS, assert_close
from test_gpu_force import ACCELERATION, FLOAT, SCHEMES, STEPS, _Reference, forced_plan, run, scales
from test_gpu_fp32_error_budget import FACTOR, GRID, weighted_error
from test_host_api import UniformFlow
from test_force_field_host import kolmogorov, kolmogorov_error, random_field

pytestmark = pytest.mark.gpu

FIELD_CLASS = {"guo": lt.GuoField, "shanchen": lt.ShanChenField}
UNIFORM_CLASS = {"guo": lt.Guo, "shanchen": lt.ShanChen}


def field_coll(scheme, operator):
    """the kernels' COLL of a plan with a field: the uniform force's number with the field's bit (32)"""
    return SCHEMES[(scheme, operator)][2] | 32


# --------------------------------------------------------------------------- the CPU reference
class _FieldReference(_Reference):
    """test_gpu_force's reference with the field classes: `field` is the acceleration [d, *res]; `uniform` (a vector)
    instead evaluates the uniform class, forced=False the operator without a force"""
    field = None

    def _collision(self, f, forced=True, uniform=None):
        flow = self.__dict__.get("_flow")
        if flow is None:
            context = lt.Context("cpu", f.dtype, use_native=False)
            flow = self._flow = UniformFlow(context, list(f.shape[1:]), 1, 0.01, STENCILS[self.lat.name]())
        flow.f = f
        force = None
        if uniform is not None:
            force = UNIFORM_CLASS[self.scheme](flow, self.tau, list(uniform))
        elif forced:
            force = FIELD_CLASS[self.scheme](flow, self.tau, self.field.to(f.dtype))
        if self.operator == "bgk":
            return lt.BGKCollision(self.tau, force=force)(flow)
        return lt.SmagorinskyCollision(self.tau, self.constant, force=force)(flow)


def reference(lat, f0, scheme, operator, field, entries=(), ncm=None, nsm=None, dtype=torch.float64, tau=None):
    L = orc.LATTICES[lat]
    default_tau, constant, _ = SCHEMES[(scheme, operator)]
    sim = _FieldReference(L, f0.to(dtype).clone(), operator, default_tau if tau is None else tau)
    sim.scheme, sim.operator, sim.constant, sim.field = scheme, operator, constant, field.cpu()
    if ncm is not None:
        sim.boundaries = [_oracle_boundary(L, e, f0.dtype) for e in entries]
        sim.no_collision_mask, sim.no_streaming_mask = ncm.cpu(), nsm.cpu()
    return sim


def field_plan(lat, dt, res, scheme, operator, field, entries=(), tau=None):
    """(plan, the field on the device): BGK / Smagorinsky with the scheme's scales and the field"""
    from lettuce_amd._native import Plan
    default_tau, constant, _ = SCHEMES[(scheme, operator)]
    plan = Plan(lat, TORCH_DT[dt], operator, res, entries)
    if constant is not None:
        plan.set_smagorinsky(constant)
    on_device = dev(field.to(TORCH_DT[dt]))
    plan.set_force_field(on_device, *scales(scheme, default_tau if tau is None else tau))
    return plan, on_device


def constant_field(res, dt):
    d = len(res)
    a = torch.tensor(ACCELERATION[:d], dtype=TORCH_DT[dt])
    return a.reshape([d] + [1] * d).expand([d] + list(res)).contiguous()


# --------------------------------------------------------------------------- 1: constant field == uniform kernel
CASES = [(dt, scheme, operator) for dt in ("f64", "f32") for scheme, operator in SCHEMES]


@pytest.mark.parametrize("lat", list(SMALL))
def test_constant_field_gives_the_uniform_kernels_bits(lat):
    for dt, scheme, operator in CASES:
        _constant_field_case(lat, dt, scheme, operator)


def _constant_field_case(lat, dt, scheme, operator):
    what = f"{lat} {dt} {scheme} {operator}"
    res = SMALL[lat]
    tau, _, coll = SCHEMES[(scheme, operator)]
    f0 = perturbed_state(lat, res, TORCH_DT[dt], 11)
    uniform = forced_plan(lat, dt, res, scheme, operator)
    plan, _ = field_plan(lat, dt, res, scheme, operator, constant_field(res, dt))
    assert f"lt::{lat.lower()}, 0, {coll}," in uniform.kernel_name(), uniform.kernel_name()
    assert f"lt::{lat.lower()}, 0, {coll | 32}," in plan.kernel_name(), plan.kernel_name()
    a = dev(f0)
    want = uniform.collide(a, torch.empty_like(a), tau).cpu().numpy()
    got = plan.collide(a, torch.empty_like(a), tau).cpu().numpy()
    assert float(np.abs(want - f0.numpy()).max()) > 10 * ATOL["f32"], what
    np.testing.assert_array_equal(got, want, err_msg=f"collide {what}")
    for n in (1, 3):
        np.testing.assert_array_equal(run(plan, f0, n, tau), run(uniform, f0, n, tau), err_msg=f"{what} n = {n}")
        assert plan.last_run_info() == expected_launches("one", n - 1, False), what


# --------------------------------------------------------------------------- 2: random field against the CPU path
@functools.lru_cache(maxsize=None)
def _snapshots(lat, dt, scheme, operator):
    """the CPU path from perturbed_state(seed 3) with the random field: (f0, field, {n: f}, collided, unforced,
    uniform-with-the-mean), computed once per case"""
    res = SMALL[lat]
    f0 = perturbed_state(lat, res, TORCH_DT[dt], 3)
    field = random_field(res, dtype=TORCH_DT[dt])
    sim = reference(lat, f0, scheme, operator, field)
    collided = sim._collision(sim.f).numpy().copy()
    unforced = sim._collision(sim.f, forced=False).numpy().copy()
    mean = field.double().reshape(len(res), -1).mean(dim=1).tolist()
    uniform = sim._collision(sim.f, uniform=mean).numpy().copy()
    want, done = {}, 0
    for n in STEPS:
        sim.step(n - done)
        done = n
        want[n] = sim.f.numpy().copy()
    return f0, field, want, collided, unforced, uniform


@pytest.mark.parametrize("lat", list(SMALL))
def test_random_field_against_the_cpu_path(lat):
    for dt, scheme, operator in CASES:
        _random_field_case(lat, dt, scheme, operator)


def _random_field_case(lat, dt, scheme, operator):
    res = SMALL[lat]
    tau = SCHEMES[(scheme, operator)][0]
    coll = field_coll(scheme, operator)
    f0, field, want, collided, unforced, uniform = _snapshots(lat, dt, scheme, operator)
    # the state and the field tell the operator from the unforced one and from the uniform force with the field's mean:
    # a kernel that ignored the field, or its variation, could not pass below
    gaps = float(np.abs(collided - unforced).max()), float(np.abs(collided - uniform).max())
    print(f"{lat} {dt} {scheme} {operator}: the CPU path's distance from the unforced operator {gaps[0]:.2e}, from the "
          f"uniform force with the mean {gaps[1]:.2e}")
    assert min(gaps) > 10 * ATOL["f32"], (lat, dt, scheme, operator)
    plan, _ = field_plan(lat, dt, res, scheme, operator, field)
    a = dev(f0)
    got = plan.collide(a, torch.empty_like(a), tau).cpu().numpy()
    assert_close(got, collided, dt, what=f"collide {lat} {dt} {scheme} {operator}")
    for n in STEPS:
        got = run(plan, f0, n, tau)
        assert plan.kernel_name().startswith(f"lbm_kernel<{FLOAT[dt]}, lt::{lat.lower()}, 0, {coll}, true, true, false,"), \
            plan.kernel_name()
        assert plan.last_run_info() == expected_launches("one", n - 1, False), (n, plan.last_run_info())
        assert_close(got, want[n], dt, n, what=f"{lat} {dt} {scheme} {operator} n = {n}")


# --------------------------------------------------------------------------- 3: indexing edges
EDGES = [("D1Q3", [37]), ("D2Q9", [7, 5]), ("D2Q9", [64, 4]), ("D2Q9", [130, 3]), ("D3Q19", [6, 5, 7])]


def test_indexing_edges_against_the_cpu_path():
    """odd and asymmetric extents, rows that are whole waves, more than one workgroup with a ragged row: a wrong axis
    permutation or a wrong c * N stride of the field shows (three different component scales)"""
    for lat, res in EDGES:
        _edge_case(lat, res)


def _edge_case(lat, res):
    tau = SCHEMES[("guo", "bgk")][0]
    f0 = perturbed_state(lat, res, torch.float64, 19)
    field = random_field(res, seed=23)
    sim = reference(lat, f0, "guo", "bgk", field)
    sim.step(2)
    plan, _ = field_plan(lat, "f64", res, "guo", "bgk", field)
    assert_close(run(plan, f0, 2, tau), sim.f.numpy(), "f64", 2, what=f"{lat} {res} n = 2")
    if len(res) > 1:
        # the components swapped are another field: the comparison above would see it
        swapped = reference(lat, f0, "guo", "bgk", field.flip(0))
        swapped.step(2)
        assert float(np.abs(swapped.f.numpy() - sim.f.numpy()).max()) > 10 * ATOL["f32"], (lat, res)


# --------------------------------------------------------------------------- 4: plans with boundaries
MASKED = [("D2Q9", [12, 10]), ("D3Q19", [6, 5, 8]), ("D3Q27", [4, 6, 5])]


@pytest.mark.parametrize("lat,res", MASKED, ids=[m[0].lower() for m in MASKED])
def test_masked_plans_against_the_cpu_path(lat, res):
    """a bounce-back block and equilibrium nodes, by table and by per-node field, no outlet; the force field is non-zero
    on the boundary nodes too, which do not read it"""
    for dt in ("f64", "f32"):
        for scheme, operator in (("guo", "bgk"), ("guo", "smagorinsky")):
            _masked_case_against_the_cpu_path(lat, res, dt, scheme, operator)


def _masked_case_against_the_cpu_path(lat, res, dt, scheme, operator):
    tau = SCHEMES[(scheme, operator)][0]
    coll = field_coll(scheme, operator)
    field = random_field(res, seed=29, dtype=TORCH_DT[dt])
    for with_field in (False, True):
        f0, ncm, nsm, entries = _masked_case(lat, res, TORCH_DT[dt], None, 40, with_field=with_field)
        assert int((ncm == 1).sum()) > 3 and int((ncm == 2).sum()) > 3
        assert float(field[:, ncm != 0].abs().min()) > 0
        plan, _ = field_plan(lat, dt, res, scheme, operator, field, entries)
        plan.set_masks(dev(ncm), dev(nsm))
        assert plan.kernel_name().startswith(f"lbm_kernel<{FLOAT[dt]}, lt::{lat.lower()}, 0, {coll}, true, true, true,"), \
            plan.kernel_name()
        sim, done = reference(lat, f0, scheme, operator, field, entries=entries, ncm=ncm, nsm=nsm), 0
        for n in (1, 3):
            sim.step(n - done)
            done = n
            got = run(plan, f0, n, tau)
            assert plan.last_run_info() == expected_launches("one", n - 1, True), plan.last_run_info()
            assert_close(got, sim.f.numpy(), dt, n,
                         what=f"{lat} {dt} {scheme} {operator} per-node equilibrium {with_field} n = {n}")


def test_a_halfway_link_body_with_a_force_field():
    """D2Q9 with a half-way link bounce-back body (the separate pass behind every launch), through lt.Simulation"""
    res, tau = [12, 10], 0.8
    f0 = perturbed_state("D2Q9", res, torch.float64, 31)
    field = random_field(res, seed=37)
    mask = torch.zeros(res, dtype=torch.bool)
    mask[4:7, 3:6] = True

    def simulation(context):
        flow = UniformFlow(context, list(res), 1, 0.01, lt.D2Q9())
        flow.boundaries = [lt.HalfwayBounceBackBoundary(context.convert_to_tensor(mask))]
        flow.f = context.convert_to_tensor(f0)
        force = lt.GuoField(flow, tau, context.convert_to_tensor(field))
        return flow, lt.Simulation(flow, lt.BGKCollision(tau, force=force), [])

    flow, sim = simulation(lt.Context("cuda:0", torch.float64, use_native=True))
    cpu_flow, cpu_sim = simulation(lt.Context("cpu", torch.float64, use_native=False))
    for n in (1, 3):
        sim(n)
        cpu_sim(n)
        assert_close(flow.f.cpu().numpy(), cpu_flow.f.numpy(), "f64", what=f"link body, {n} more step(s)")
    assert ", 0, 37, true, true, true," in sim._native.plan.kernel_name(), sim._native.plan.kernel_name()


# --------------------------------------------------------------------------- 5: the fp32 error budget
@functools.lru_cache(maxsize=None)
def _budget_pair(lat, scheme, tau):
    """{n: (cpu_fp32, cpu_fp64)} from the same fp32 state and the same fp32 field"""
    f0 = perturbed_state(lat, GRID[lat], torch.float32, 3)
    field = random_field(GRID[lat], dtype=torch.float32)
    out = {n: [] for n in (1, 8)}
    for dtype in (torch.float32, torch.float64):
        sim, done = reference(lat, f0, scheme, "bgk", field, dtype=dtype, tau=tau), 0
        for n in (1, 8):
            sim.step(n - done)
            done = n
            assert sim.f.dtype == dtype
            out[n].append(sim.f.double().numpy().copy())
    return f0, field, {n: tuple(v) for n, v in out.items()}


@pytest.mark.parametrize("lat", ["D2Q9", "D3Q19"])
def test_fp32_error_within_the_reference_arithmetics_own(lat):
    """E = max over q and nodes of |. - cpu_fp64| / w_q: E_gpu <= 4 E_ref, the project's gate, for Guo and Shan-Chen at
    tau = 0.51 and 0.7 after 1 and 8 steps.  Measured ratios: 1.00 in all sixteen cases"""
    failures = []
    for scheme in ("guo", "shanchen"):
        for tau in (0.51, 0.7):
            failures += _budget_case(lat, scheme, tau)
    assert not failures, f"(scheme, tau, n, E_ref, E_gpu, ratio) beyond {FACTOR:g} x E_ref: {failures}"


def _budget_case(lat, scheme, tau):
    f0, field, pair = _budget_pair(lat, scheme, tau)
    plan, _ = field_plan(lat, "f32", GRID[lat], scheme, "bgk", field, tau=tau)
    failures = []
    for n in (1, 8):
        f32, f64 = pair[n]
        assert np.isfinite(f32).all() and np.isfinite(f64).all()
        e_ref = float(weighted_error(lat, f32, f64).max())
        got = run(plan, f0, n, tau)
        assert got.dtype == np.float32 and np.isfinite(got).all()
        e_gpu = float(weighted_error(lat, got, f64).max())
        print(f"{scheme}-field-bgk-{lat.lower()} tau {tau} n = {n}: E_ref {e_ref:.3e}  E_gpu {e_gpu:.3e}  "
              f"ratio {e_gpu / e_ref:.2f}  (gate {FACTOR:g})")
        assert e_ref > 0
        if not e_gpu <= FACTOR * e_ref:
            failures.append((scheme, tau, n, e_ref, e_gpu, e_gpu / e_ref))
    return failures


# --------------------------------------------------------------------------- 6: settings
def test_the_field_is_read_at_every_launch_and_the_later_setter_wins():
    lat, dt, res, tau = "D3Q19", "f64", SMALL["D3Q19"], 0.8
    f0 = perturbed_state(lat, res, torch.float64, 41)
    first, second = random_field(res, seed=43), random_field(res, seed=47)

    def cpu(field, n=2):
        sim = reference(lat, f0, "guo", "bgk", field)
        sim.step(n)
        return sim.f.numpy()

    plan, on_device = field_plan(lat, dt, res, "guo", "bgk", first)
    assert_close(run(plan, f0, 2, tau), cpu(first), dt, 2, what="the first field")
    on_device.copy_(dev(second))                                     # edited in place: no call
    assert_close(run(plan, f0, 2, tau), cpu(second), dt, 2, what="edited in place")
    assert float(np.abs(cpu(first) - cpu(second)).max()) > 10 * ATOL["f32"]
    replaced = dev(first.clone())
    plan.set_force_field(replaced, *scales("guo", tau))              # another tensor
    assert_close(run(plan, f0, 2, tau), cpu(first), dt, 2, what="replaced")
    # set_force after set_force_field: the uniform kernel and its result
    uniform = forced_plan(lat, dt, res, "guo", "bgk")
    plan.set_force(ACCELERATION, *scales("guo", tau))
    assert plan.kernel_name() == uniform.kernel_name()
    np.testing.assert_array_equal(run(plan, f0, 2, tau), run(uniform, f0, 2, tau))
    # ... and back; then no field: the plan that never had a force
    plan.set_force_field(replaced, *scales("guo", tau))
    assert ", 0, 37," in plan.kernel_name()
    assert_close(run(plan, f0, 2, tau), cpu(first), dt, 2, what="the field after the uniform force")
    plan.set_force_field(None)
    never = plan_for(lat, torch.float64, "bgk", res)
    assert plan.kernel_name() == never.kernel_name()
    np.testing.assert_array_equal(run(plan, f0, 2, tau), run(never, f0, 2, tau))


def test_set_force_field_validates_and_leaves_the_plan_unchanged():
    from lettuce_amd._native import NativeEngineError
    lat, dt, res, tau = "D2Q9", "f64", [12, 10], 0.8
    f0 = perturbed_state(lat, res, torch.float64, 3)
    field = random_field(res)
    plan, on_device = field_plan(lat, dt, res, "guo", "bgk", field)
    before = run(plan, f0, 2, tau)
    bad = {"dtype": on_device.float(), "shape": dev(random_field([12, 11])), "components": on_device[:1].contiguous(),
           "device": field.clone(), "dense": dev(random_field([10, 12])).permute(0, 2, 1)}
    for what, tensor in bad.items():
        with pytest.raises(NativeEngineError):
            plan.set_force_field(tensor, *scales("guo", tau))
        np.testing.assert_array_equal(run(plan, f0, 2, tau), before, err_msg=what)
    for scale in ((float("nan"), 0.375), (0.5, float("inf"))):
        with pytest.raises(NativeEngineError, match="must be finite"):
            plan.set_force_field(on_device, *scale)
        np.testing.assert_array_equal(run(plan, f0, 2, tau), before)
    for coll in ("kbc", "none", "trt"):
        other = plan_for(lat, torch.float64, coll, res)
        name = other.kernel_name()
        with pytest.raises(NativeEngineError, match="BGK and Smagorinsky") as refusal:
            other.set_force_field(on_device, *scales("guo", tau))
        assert refusal.value.code == 2 and other.kernel_name() == name          # LT_ERR_UNSUPPORTED


def test_refusals_name_the_pair():
    from lettuce_amd._native import LAYOUT_SLAB, NativeEngineError, Plan
    tau = 0.8
    res = [16, 128]
    field = dev(random_field(res))
    f = dev(perturbed_state("D2Q9", res, torch.float64, 3))

    def refused(call, words):
        with pytest.raises(NativeEngineError, match=words) as refusal:
            call()
        assert refusal.value.code == 2, str(refusal.value)             # LT_ERR_UNSUPPORTED

    # two steps and several steps per launch, asked after the field and before it
    plan = plan_for("D2Q9", torch.float64, "bgk", res)
    plan.set_force_field(field, *scales("guo", tau))
    refused(lambda: plan.set_two_step(1), "force field")
    refused(lambda: plan.set_many_step(1), "force field")
    refused(lambda: plan.stream_collide_twice(f, torch.empty_like(f), tau), "force field")
    refused(lambda: plan.stream_collide_many(f, torch.empty_like(f), tau, 4), "force field")
    assert "force field" in plan.two_step_admitted()
    run(plan, f.cpu(), 4, tau)
    assert plan.last_run_info() == expected_launches("one", 3, False)
    for switch in ("set_two_step", "set_many_step"):
        asked = plan_for("D2Q9", torch.float64, "bgk", res)
        getattr(asked, switch)(1)
        name = asked.kernel_name()
        refused(lambda: asked.set_force_field(field, *scales("guo", tau)), "force field")
        assert asked.kernel_name() == name and "37" not in name
    # the incompressible equilibrium, either order
    plan = plan_for("D2Q9", torch.float64, "bgk", res)
    plan.set_equilibrium("incompressible", 1.0)
    refused(lambda: plan.set_force_field(field, *scales("guo", tau)), "incompressible equilibrium")
    plan = plan_for("D2Q9", torch.float64, "bgk", res)
    plan.set_force_field(field, *scales("guo", tau))
    refused(lambda: plan.set_equilibrium("incompressible", 1.0), "force field")
    assert ", 0, 37," in plan.kernel_name()
    # outlets of either kind
    for entry, words in (({"kind": "abb_outlet", "axis": 0, "side": 1}, "anti-bounce-back outlet"),
                         ({"kind": "pressure_outlet", "axis": 1, "side": -1, "rho_outlet": 1.01}, "constant-pressure outlet")):
        plan = Plan("D2Q9", torch.float64, "bgk", res, [entry])
        refused(lambda: plan.set_force_field(field, *scales("guo", tau)), words)
    # slab layout and ghost planes: the binding says so before the library is asked, the library when asked directly
    res3 = [8, 6, 4]
    field3 = dev(random_field(res3, dtype=torch.float32))
    for kwargs in ({"layout": LAYOUT_SLAB}, {"layout": LAYOUT_SLAB, "ghost_planes": 1}):
        plan = Plan("D3Q19", torch.float32, "bgk", res3, [], **kwargs)
        with pytest.raises(NativeEngineError, match="slab plan"):
            plan.set_force_field(field3, *scales("guo", tau))
        code = plan.lib.lt_plan_set_force_field(plan._handle, field3.data_ptr(), 0.5, 0.375)
        assert code == 2 and "slab plan" in plan.lib.lt_last_error().decode()
        assert ", 1, 1," in plan.kernel_name()


# --------------------------------------------------------------------------- 7: lt.Simulation on the Kolmogorov flow
def test_kolmogorov_flow_through_the_simulation():
    """[16, 16] fp64: 100 steps against the CPU path, with flow.f read between two batches; 778 steps against the laminar
    profile within the bound of the host test (the scheme's discretisation error there is 1.64e-2)"""
    native = lt.Context("cuda:0", torch.float64, use_native=True)
    flow, force, sim, steps, profile = kolmogorov(native, 16)
    assert sim._native is not None and steps == 778
    cpu_flow, _, cpu_sim, _, _ = kolmogorov(lt.Context("cpu", torch.float64, use_native=False), 16)
    sim(40)
    cpu_sim(40)
    assert_close(flow.f.cpu().numpy(), cpu_flow.f.numpy(), "f64", what="40 steps")      # read in between the batches
    sim(60)
    cpu_sim(60)
    bound = 1e-12
    err = float((flow.f.cpu() - cpu_flow.f).abs().max())
    print(f"100 steps: max |difference| {err:.3e} (bound {bound:.0e})")
    assert err <= bound
    assert ", 0, 37, true, true, false," in sim._native.plan.kernel_name(), sim._native.plan.kernel_name()
    info = sim._native.plan.last_run_info()
    assert info["two_step_launches"] == 0 and info["many_step_launches"] == 0
    sim(steps - 100)
    error, uy = kolmogorov_error(flow, force, profile)
    print(f"{steps} steps: relative L2 error {error:.3e} (bound 2e-2), max |u_y| {uy:.2e}")
    assert error < 2e-2
    # the field edited in place between two batches is what the next batch applies: doubled, the flow accelerates
    # towards twice the profile
    force.acceleration.mul_(2)
    sim(steps)
    error2, _ = kolmogorov_error(flow, force, 2 * profile)
    print(f"{steps} more steps with the field doubled in place: relative L2 error {error2:.3e}")
    assert error2 < 2e-2
