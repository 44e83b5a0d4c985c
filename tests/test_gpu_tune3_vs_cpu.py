"""The one-step kernels with nontemporal loads and stores (the kernels' TUNE = 3) against the CPU paths in float64.

Every one-step kernel exists twice, as separate instantiations with their own register allocation and schedule.
lt_run picks TUNE = 3 above 128 MiB of populations (api.hip, resolve_tune) -- every grid users run -- and the
reference comparisons of the rest of the suite run grids far below that, i.e. the TUNE = 0 instantiations.
tests/tune3_census.txt (tests/test_tune3_census.py) lists every TUNE = 3 instantiation of the library; here each of
its lines is launched on a small grid with ``set_tuning(3)``:

* the plan is built through the public Plan API from the line's selector (lattice, dtype, collision and its setters,
  layout, masks, a constant-pressure outlet) and must name the line's kernel -- and the same name with TUNE 0 after
  ``set_tuning(0)``, so a quiet run of the cached kernel cannot pass;
* the line's mode runs through ``stream_collide`` / ``collide`` / ``stream`` (slab layout: the ``*_planes`` entry points
  over the owned planes of a plan with one ghost plane per side, filled as the periodic neighbours would), and lt_run
  for 3 and 4 steps (one collide, n - 1 fused steps, one stream, all of policy 3; slab layout: the periodic plan without
  ghost planes);
* each result is held to that operator's CPU path in float64 from the same (fp32: the same fp32) state -- the oracle
  for none / BGK / KBC, the ``_Reference`` classes of the Smagorinsky, force, TRT / regularised and MRT tests, the
  mirror's operators on the incompressible equilibrium, the mirror's torch path for a constant-pressure outlet -- within
  fp64 1e-12 max(1, |f|max), fp32 1e-5 max(1, |f|max) max(1, n / 10), ten times that with an outlet;
* and must be ``torch.equal`` to what the TUNE = 0 kernel gives (ROUNDING: the named exceptions, none).

Shapes: D1Q3 [37]; D2Q9 [12, 10]; 3-D [6, 5, 7] -- node counts that are no multiple of the 256-thread workgroup, a
wrap on every axis.  Plans with masks run a second time with the outlet's normal along the contiguous axis and 64
nodes along it (D2Q9 [5, 64], 3-D [4, 6, 64], slabs [64, 6, 4]): the kernels' ``abb0_slot`` path.  One case per 3-D
unit runs on engine-owned padded buffers (``set_resident(1, pad)``, three fused steps): the launch with a population
stride.

Also here: ``set_residency`` (the dynamic-LDS cap that is automatic only above 128 MiB and 8192 workgroups, so that no
other test reaches it) and the threshold of the automatic cache policy itself.
"""
import functools
import warnings

import numpy as np
import pytest
import torch

import lettuce_amd as lt
import test_gpu_equilibria as equilibria
import test_gpu_force as force
import test_gpu_mrt as mrt
import test_gpu_relaxations as relaxations
import test_gpu_smagorinsky as smagorinsky
from conftest import TORCH_DT
from test_gpu_engine import _masked_case, dev
from test_gpu_outlet_p import masks_and_entries, synthetic
from test_gpu_paths_vs_oracle import TAU, _Oracle, _oracle_boundary, oracle, perturbed_state
from test_gpu_smagorinsky import assert_close
from test_host_api import UniformFlow
from test_mrt_host import make_collision, quiet, rates_of
from test_tune3_census import census_lines
from oracle import lettuce_oracle as orc
from outlet_p_cases import mirror_flow

pytestmark = pytest.mark.gpu

UNTOUCHED = -7.0
FUSED, COLLIDE, STREAM = 0, 1, 2
RUNS = (3, 4)
PAD = 96                       # elements between the populations of the padded case, beyond the field (a multiple of 32)
RHO_OUTLET = 1.02
# kernel name -> the largest distance in ulp between its populations and those of the TUNE = 0 instantiation, for
# instantiations that contract the same expression differently.  None: every TUNE = 3 kernel is bit-identical to its twin.
ROUNDING = {}


@pytest.fixture(autouse=True)
def _nothing_runs_after_a_device_fault():
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as exc:
        pytest.exit(f"the device reported a fault; no further launches: {exc}", returncode=3)


# --------------------------------------------------------------------------- the collisions: plan, tau, CPU paths
class _IncompressibleReference(_Oracle):
    """the oracle's stepping and boundaries around the mirror's operators on the incompressible equilibrium"""
    operator = "bgk"

    def _collision(self, f):
        flow = self.__dict__.get("_flow")
        if flow is None:
            context = lt.Context("cpu", f.dtype, use_native=False)
            flow = self._flow = UniformFlow(context, list(f.shape[1:]), 1, 0.01, equilibria.STENCILS[self.lat.name](),
                                            lt.IncompressibleQuadraticEquilibrium(equilibria.RHO0))
        flow.f = f
        return equilibria.cpu_collision(self.operator, flow, self.tau)(flow)


def _with_masks(sim, lat, dtype, entries, ncm, nsm):
    if ncm is not None:
        L = orc.LATTICES[lat]
        sim.boundaries = [_oracle_boundary(L, e, dtype) for e in entries]
        sim.no_collision_mask, sim.no_streaming_mask = ncm.cpu(), nsm.cpu()
    return sim


def _transform(coll, lat):
    return "lallemand" if coll == 11 else {"D2Q9": "dellar", "D3Q27": "hermite"}[lat]


INCOMPRESSIBLE = {17: "bgk", 21: "guo", 24: "trt", 25: "regularized"}
PLAIN = {0: "none", 1: "bgk", 2: "kbc"}
FORCED = {5: ("guo", "bgk"), 7: ("guo", "smagorinsky")}
RELAXATIONS = {8: "trt", 9: "regularized"}
SMAGORINSKY_CONSTANT = 1.0


def tau_of(coll):
    """the relaxation time of the calls, as the CPU path of the collision's own tests has it"""
    if coll in PLAIN or coll in RELAXATIONS:
        return TAU
    if coll == 3:
        return smagorinsky.TAU
    if coll in FORCED:
        return force.SCHEMES[FORCED[coll]][0]
    if coll in INCOMPRESSIBLE:
        return equilibria.TAU
    return 1.0                                    # (an MRT plan does not read it)


def make_plan(coll, lat, dt, res, entries=(), **kwargs):
    """the plan of the kernels' collision number `coll` through the helpers of that collision's tests"""
    from lettuce_amd._native import Plan
    if coll in PLAIN:
        return Plan(lat, TORCH_DT[dt], PLAIN[coll], res, entries, **kwargs)
    if coll == 3:
        return smagorinsky.smagorinsky_plan(lat, dt, res, SMAGORINSKY_CONSTANT, entries, **kwargs)
    if coll in FORCED:
        return force.forced_plan(lat, dt, res, *FORCED[coll], entries=entries, **kwargs)
    if coll in RELAXATIONS:
        return relaxations.make_plan(RELAXATIONS[coll], lat, dt, res, entries, **kwargs)
    if coll in INCOMPRESSIBLE:
        return equilibria.make_plan(INCOMPRESSIBLE[coll], lat, dt, res, entries, **kwargs)
    return mrt.mrt_plan(_transform(coll, lat), dt, res, entries=entries, **kwargs)


def cpu_path(coll, lat, f0, entries=(), ncm=None, nsm=None):
    """that collision's CPU path in float64 from f0 (promoted), with the plan's boundaries: collide(), stream(), step(n), f"""
    masks = dict(entries=entries, ncm=ncm, nsm=nsm)
    if coll in PLAIN:
        return oracle(lat, f0, PLAIN[coll], **masks)
    if coll == 3:
        return smagorinsky.reference(lat, f0, SMAGORINSKY_CONSTANT, **masks)
    if coll in FORCED:
        return force.reference(lat, f0, *FORCED[coll], **masks)
    if coll in RELAXATIONS:
        return relaxations.reference(RELAXATIONS[coll], lat, f0, **masks)
    if coll in INCOMPRESSIBLE:
        sim = _IncompressibleReference(orc.LATTICES[lat], f0.double().clone(), INCOMPRESSIBLE[coll], equilibria.TAU)
        sim.operator = INCOMPRESSIBLE[coll]
        return _with_masks(sim, lat, f0.dtype, entries, ncm, nsm)
    return mrt.reference(_transform(coll, lat), f0, **masks)


def mirror_collision(coll, lat, flow):
    """the mirror's operator of `coll` on a flow with a constant-pressure outlet (the torch path is the CPU path there)"""
    tau = tau_of(coll)
    acceleration = list(force.ACCELERATION[:flow.stencil.d])
    if coll == 2:
        collision = lt.KBCCollision()
        collision.native_generator().tau(flow)          # the first use takes the flow's tau and the beta of it ...
        collision.tau, collision.beta = tau, 1.0 / (2.0 * tau)      # ... which an assignment replaces
        return collision
    if coll in PLAIN:
        return lt.BGKCollision(tau) if coll else lt.NoCollision()
    if coll == 3:
        return lt.SmagorinskyCollision(tau, SMAGORINSKY_CONSTANT)
    if coll == 5:
        return lt.BGKCollision(tau, force=lt.Guo(flow, tau, acceleration))
    if coll == 7:
        return lt.SmagorinskyCollision(tau, force.SCHEMES[FORCED[coll]][1], force=lt.Guo(flow, tau, acceleration))
    if coll in RELAXATIONS:
        return relaxations.cpu_collision(RELAXATIONS[coll], flow)
    transform = _transform(coll, lat)
    return make_collision(transform, flow.context, rates_of(transform, mrt.TAU), flow.stencil)


class _Mirror:
    """lt.Simulation's whole-field torch path behind the oracle's interface"""

    def __init__(self, sim):
        self.sim = sim

    @property
    def f(self):
        return self.sim.flow.f

    def collide(self):
        return quiet(self.sim._collide)

    def stream(self):
        return self.sim._stream()

    def step(self, n=1):
        for _ in range(n):
            self.collide()
            self.stream()
        return self.f


# --------------------------------------------------------------------------- the cases: one per line and shape
SMALL = {1: [37], 2: [12, 10], 3: [6, 5, 7]}
ROW = {2: [5, 64], 3: [4, 6, 64]}                 # 64 nodes along the contiguous axis of the reference layout ...
ROW_SLAB = [64, 6, 4]                             # ... and of the slab layout (x)


def _cases():
    out, padded = [], set()
    for unit, name, s in census_lines():
        lat, dt = unit.split("_")
        d = int(lat[1])
        shapes = ["small"]
        if s["masked"] and s["mode"] != STREAM and d > 1:
            shapes.append("row")
        if d == 3 and unit not in padded and (s["layout"], s["coll"], s["mode"], s["masked"]) == (0, 1, FUSED, 0):
            padded.add(unit)
            shapes.append("padded")
        for shape in shapes:
            cid = (f"{unit}-{'slab' if s['layout'] else 'ref'}-coll{s['coll']}-{('fused', 'collide', 'stream')[s['mode']]}"
                   f"{'-masked' if s['masked'] else ''}{'-pout' if s['n_pout'] else ''}-{shape}")
            out.append(pytest.param(lat.upper(), dt, name, dict(s), shape, id=cid))
    return out


CASES = _cases()


def _geometry(lat, s, shape):
    """(logical resolution, outlet (axis, side) of a plan with masks, per-node equilibrium field?)"""
    d = int(lat[1])
    if shape == "row":
        res = ROW_SLAB if s["layout"] else ROW[d]
        return list(res), ((0, -1) if s["layout"] else (d - 1, -1)), True
    return list(SMALL[d]), (0, 1), False


def _problem(lat, dt, s, shape):
    """(res, f0 on the CPU in the plan's dtype, ncm, nsm, plan entries) in the reference layout's axis order"""
    res, outlet, with_field = _geometry(lat, s, shape)
    f0 = perturbed_state(lat, res, TORCH_DT[dt], 11)
    if not s["masked"]:
        return res, f0, None, None, []
    if s["n_pout"]:
        direction = [0] * len(res)
        direction[outlet[0]] = outlet[1]
        g = synthetic(lat.lower(), res, [("EquilibriumOutletP", direction, RHO_OUTLET)])
        ncm, nsm, entries = masks_and_entries(g, f"outlet_p_tune3_{lat.lower()}_{dt}")
        return res, f0, ncm, nsm, entries
    _, ncm, nsm, entries = _masked_case(lat, res, TORCH_DT[dt], outlet, 51, with_field=with_field, inlet_face=(shape == "row"))
    return res, f0, ncm, nsm, entries


@functools.lru_cache(maxsize=None)
def _expected(lat, dt, coll, mode, masked, n_pout, shape, slab_row):
    """{"op": the line's mode applied once, 3: after three steps, 4: after four}: float64 arrays of the CPU path.  One
    computation per problem: the two layouts of a line share it where they share the resolution."""
    s = {"coll": coll, "mode": mode, "masked": masked, "n_pout": n_pout, "layout": int(slab_row)}
    res, f0, ncm, nsm, entries = _problem(lat, dt, s, shape)

    def fresh():
        if n_pout:
            _, outlet, _ = _geometry(lat, s, shape)
            direction = [0] * len(res)
            direction[outlet[0]] = outlet[1]
            g = synthetic(lat.lower(), res, [("EquilibriumOutletP", direction, RHO_OUTLET)])
            context = lt.Context("cpu", torch.float64, use_native=False)
            flow = mirror_flow(g, f"outlet_p_tune3_{lat.lower()}_f64", context, set_f0=False)
            flow.f = f0.double().clone()
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                return _Mirror(lt.Simulation(flow, mirror_collision(coll, lat, flow), []))
        return cpu_path(coll, lat, f0, entries, ncm, nsm)

    out = {}
    sim = fresh()
    if mode != COLLIDE:
        sim.stream()
    if mode != STREAM:
        sim.collide()
    out["op"] = sim.f.detach().numpy().copy()
    sim, done = fresh(), 0
    for n in RUNS:
        sim.step(n - done)
        done = n
        out[n] = sim.f.detach().numpy().copy()
    return out


def _to_slab(t, ghosts):
    """[.., x, y, z] -> [.., z + 2 ghosts, y, x], the ghost planes those of the periodic neighbours"""
    n = t.dim()
    t = t.permute(*range(n - 3), n - 1, n - 2, n - 3)
    if ghosts:
        t = torch.cat([t.narrow(n - 3, t.shape[n - 3] - ghosts, ghosts), t, t.narrow(n - 3, 0, ghosts)], dim=n - 3)
    return t.contiguous()


def _built(lat, dt, s, res, f0, ncm, nsm, entries, ghosts=0):
    """(plan with its masks set and neither pairs nor batches of steps, its input on the device) in the plan's layout"""
    from lettuce_amd._native import LAYOUT_SLAB
    coll = 0 if s["mode"] == STREAM else s["coll"]
    if s["layout"]:
        entries = [dict(e, field=_to_slab(e["field"], ghosts)) if "field" in e else e for e in entries]
        plan = make_plan(coll, lat, dt, res, entries, layout=LAYOUT_SLAB, ghost_planes=ghosts)
        f = _to_slab(f0, ghosts)
        if ncm is not None:
            ncm, nsm = _to_slab(ncm, ghosts), _to_slab(nsm, ghosts)
    else:
        plan = make_plan(coll, lat, dt, res, entries)
        f = f0
    assert list(f.shape) == plan.f_shape
    if ncm is not None:
        plan.set_masks(dev(ncm), dev(nsm))
    plan.set_two_step(0)
    if len(res) == 2:
        plan.set_many_step(0)
    return plan, dev(f)


def with_fields(name, mode=None, tune=None):
    """a one-step kernel's name with its STREAM and COLLIDE arguments those of `mode` and / or its TUNE argument `tune`"""
    fields = name.split(", ")
    if mode is not None:
        fields[4], fields[5] = {FUSED: ("true", "true"), COLLIDE: ("false", "true"), STREAM: ("true", "false")}[mode]
    if tune is not None:
        fields[9] = str(tune)
    return ", ".join(fields)


def _once(plan, mode, f, tau, planes=None):
    """the line's mode once: (output with UNTOUCHED where the launch does not write, the view the launch owns)"""
    out = torch.full_like(f, UNTOUCHED)
    if planes is None:
        {FUSED: lambda: plan.stream_collide(f, out, tau), COLLIDE: lambda: plan.collide(f, out, tau),
         STREAM: lambda: plan.stream(f, out)}[mode]()
        return out
    begin, end = planes
    {FUSED: lambda: plan.stream_collide_planes(f, out, tau, begin, end),
     COLLIDE: lambda: plan.collide_planes(f, out, tau, begin, end),
     STREAM: lambda: plan.stream_planes(f, out, begin, end)}[mode]()
    return out


def _steps(plan, f, tau, n):
    a = f.clone()
    out, _ = plan.run(a, torch.empty_like(a), tau, n)
    info = plan.last_run_info()
    assert info == {"single_step_launches": n - 1, "two_step_launches": 0, "many_step_launches": 0}, info
    return out


def _ulp_distance(a, b):
    """the largest distance in units in the last place between two arrays of one float type, and how many values differ"""
    differ = a != b
    if not differ.any():
        return 0, 0
    as_int = np.int32 if a.dtype == np.float32 else np.int64

    def ordered(x):
        return [int(v) if v >= 0 else -int(v & np.iinfo(as_int).max) for v in x[differ].view(as_int)]
    return max(abs(p - q) for p, q in zip(ordered(a), ordered(b))), int(differ.sum())


def _assert_same_bits(got3, got0, name, what):
    if torch.equal(got3, got0):
        return
    ulp, count = _ulp_distance(got3.cpu().numpy(), got0.cpu().numpy())
    print(f"{what}: {count} of {got3.numel()} values differ from the TUNE = 0 kernel, by up to {ulp} ulp")
    assert name in ROUNDING and ulp <= ROUNDING[name], \
        f"{what}: {name} and its TUNE = 0 twin differ in {count} of {got3.numel()} values, by up to {ulp} ulp"


def _logical(t, layout, ghosts=0):
    """populations of a plan as a float64 array in the reference layout's axis order, without ghost planes"""
    a = t.detach().cpu().double().numpy()
    if not layout:
        return a
    if ghosts:
        a = a[:, ghosts:-ghosts]
    return a.transpose(0, 3, 2, 1)


@pytest.mark.parametrize("lat,dt,name,s,shape", CASES)
def test_policy_3_kernel_against_the_cpu_path_and_its_policy_0_twin(lat, dt, name, s, shape):
    mode, layout, outlet = s["mode"], s["layout"], bool(s["masked"])
    coll = 0 if mode == STREAM else s["coll"]
    tau = tau_of(coll)
    res, f0, ncm, nsm, entries = _problem(lat, dt, s, shape)
    want = _expected(lat, dt, coll, mode, s["masked"], s["n_pout"], "small" if shape == "padded" else shape,
                     bool(layout) and shape == "row")
    what = f"{name} {shape}"

    def both_policies(plan, launches):
        """{key: output} of `launches` with cache policy 3 and with 0, the plan's kernel name asserted for both"""
        got = {}
        for tune in (3, 0):
            plan.set_tuning(tune)
            assert with_fields(plan.kernel_name(), mode=mode) == with_fields(name, tune=tune), (plan.kernel_name(), name)
            got[tune] = {key: launch() for key, launch in launches.items()}
        torch.cuda.synchronize()
        return got

    if shape == "padded":
        plan, f = _built(lat, dt, s, res, f0, ncm, nsm, entries)
        plan.set_resident(1, PAD)
        enabled, stride = plan.resident_enabled()
        assert enabled and stride > f[0].numel()

        def resident():
            plan.resident_load(f, tau)
            plan.resident_advance(tau, RUNS[1] - 1)
            assert plan.last_run_info()["single_step_launches"] == RUNS[1] - 1
            return plan.resident_store(torch.full_like(f, UNTOUCHED))
        got = both_policies(plan, {RUNS[1]: resident})
        assert_close(_logical(got[3][RUNS[1]], 0), want[RUNS[1]], dt, RUNS[1], outlet, f"{what} resident n = {RUNS[1]}")
        _assert_same_bits(got[3][RUNS[1]], got[0][RUNS[1]], name, what)
        return

    # the line's mode, once
    ghosts = 1 if layout else 0
    plan, f = _built(lat, dt, s, res, f0, ncm, nsm, entries, ghosts)
    planes = (1, f.shape[1] - 1) if layout else None
    got = both_policies(plan, {"op": lambda: _once(plan, mode, f, tau, planes)})
    if layout:                      # the ghost planes are not the launch's
        for tune in (3, 0):
            assert bool((got[tune]["op"][:, 0] == UNTOUCHED).all()) and bool((got[tune]["op"][:, -1] == UNTOUCHED).all())
    assert_close(_logical(got[3]["op"], layout, ghosts), want["op"], dt, 1, outlet, f"{what} once")
    _assert_same_bits(got[3]["op"], got[0]["op"], name, f"{what} once")
    # lt_run: one collide, n - 1 fused steps, one stream (slab layout: the periodic plan without ghost planes)
    if layout:
        plan, f = _built(lat, dt, s, res, f0, ncm, nsm, entries, 0)
    got = both_policies(plan, {n: (lambda n=n: _steps(plan, f, tau, n)) for n in RUNS})
    for n in RUNS:
        assert_close(_logical(got[3][n], layout), want[n], dt, n, outlet, f"{what} lt_run n = {n}")
        _assert_same_bits(got[3][n], got[0][n], name, f"{what} lt_run n = {n}")


# --------------------------------------------------------------------------- lt_plan_set_residency
UNITS = [(lat, dt) for lat in ("D2Q9", "D3Q19", "D3Q27", "D1Q3", "D3Q15") for dt in ("f32", "f64")]


@pytest.mark.parametrize("masked", [False, True], ids=["periodic", "masked"])
@pytest.mark.parametrize("lat,dt", UNITS, ids=[f"{u[0].lower()}_{u[1]}" for u in UNITS])
def test_residency_cap_launches_and_changes_no_population(lat, dt, masked):
    """set_residency(k), k in {2, 3, 4, 8}: the unused dynamic LDS of resolve_lds (3 and 4 are its automatic values above
    128 MiB and 8192 workgroups; 2 is the largest allocation, 8 none) -- the launch returns LT_OK (a refused launch would
    raise NativeEngineError with LT_ERR_HIP) and the populations are those without a cap, for both cache policies"""
    s = {"layout": 0, "coll": 1, "mode": FUSED, "masked": int(masked), "n_pout": 0}
    res, f0, ncm, nsm, entries = _problem(lat, dt, s, "small")
    plan, f = _built(lat, dt, s, res, f0, ncm, nsm, entries)
    for tune in (3, 0):
        plan.set_tuning(tune)
        plan.set_residency(0)
        want = _once(plan, FUSED, f, TAU)
        assert float((want - f).abs().max()) > 1e-4
        for k in (2, 3, 4, 8):
            plan.set_residency(k)
            got = _once(plan, FUSED, f, TAU)
            steps = _steps(plan, f, TAU, 3)
            torch.cuda.synchronize()
            assert torch.equal(got, want), (tune, k)
            plan.set_residency(0)
            assert torch.equal(steps, _steps(plan, f, TAU, 3)), (tune, k)


# --------------------------------------------------------------------------- the automatic cache policy
@pytest.mark.parametrize("lat,dt", UNITS, ids=[f"{u[0].lower()}_{u[1]}" for u in UNITS])
def test_automatic_cache_policy_switches_just_above_128_mib(lat, dt):
    """resolve_tune: policy 0 while both population buffers, 2 q N esize bytes, fit 128 MiB, 3 from the next node on --
    read from kernel_name() of plans nothing is launched on (lt_plan_create allocates the boundary table and the
    reduction scratch only, nothing that grows with the grid)"""
    from lettuce_amd._native import Plan
    q, d = int(lat.split("Q")[1]), int(lat[1])
    nodes = (128 << 20) // (2 * q * (4 if dt == "f32" else 8))
    for n, tune in ((nodes, 0), (nodes + 1, 3)):
        plan = Plan(lat, TORCH_DT[dt], "bgk", [n] + [1] * (d - 1))
        plan.set_two_step(0)
        plan.set_many_step(0)
        fields = plan.kernel_name().split(", ")
        assert fields[0].startswith("lbm_kernel<") and fields[9] == str(tune), (n, plan.kernel_name())
        plan.set_tuning(3 - tune)
        assert plan.kernel_name().split(", ")[9] == str(3 - tune)
        plan.close()
