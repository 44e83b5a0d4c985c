"""fp32 only: the operations that agree with the reference "at rounding level" by design (KBC, the anti-bounce-back
outlet, Smagorinsky, the body forces), gated by the reference arithmetic's OWN fp32 error instead of a fixed 1e-5.

Per case the CPU path runs twice from the same fp32 state, once in fp32 and once in fp64, and with w_q the lattice
weight

    E_ref = max over q and nodes of |cpu_fp32 - cpu_fp64| / w_q
    E_gpu = max over q and nodes of |gpu_fp32 - cpu_fp64| / w_q

The gate is E_gpu <= FACTOR * E_ref with FACTOR = 4: the kernels differ from the reference by a handful of single
roundings per population (one reciprocal for two divisions, the rescaled ds, pre-collision neighbour moments at the
outlet) while E_ref is already the accumulation of dozens; the factor absorbs those and the maximum over a few thousand
nodes.  A coefficient wrong at 1e-3 exceeds the gate thirtyfold (E_ref is 4e-7 .. 1.3e-5 in these units).  The measured
ratios are in DESIGN.md section 2.  Every case prints E_ref, E_gpu and their ratio before it asserts.

The CPU paths: OracleSimulation with the plan's boundaries (as test_gpu_paths_vs_oracle.py builds it) for KBC and
the outlet, the mirror's torch operators for Smagorinsky (test_gpu_smagorinsky.py) and the forces (test_gpu_force.py).
That the reference alone stays inside the gate's assumptions (both runs finite, E_ref > 0 in every weight class) is
checked without a GPU in test_fp32_error_budget_host.py.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import lettuce_oracle as orc
from test_gpu_engine import _masked_case, dev
from test_gpu_paths_vs_oracle import _Feq, _Oracle, _oracle_boundary, perturbed_state
import test_gpu_force as forces
import test_gpu_smagorinsky as smagorinsky

pytestmark = pytest.mark.gpu

FACTOR = 4.0
# a case whose ratio honestly exceeds 4 gets the next power of two above the measured ratio, with the arithmetic that
# explains it in DESIGN.md section 2; beyond 16 it is a bug
FACTORS = {}
TAUS = (0.51, 0.7)
STEPS = (1, 8)
SEED = 3
GRID = {"D2Q9": [16, 24], "D3Q19": [6, 8, 10], "D3Q27": [6, 8, 10]}


# --------------------------------------------------------------------------- the cases
def _case(cid, kind, lat, **what):
    return pytest.param(kind, lat, tuple(sorted(what.items())), id=cid)


def _directions(lat):
    return [(axis, side) for axis in range(orc.LATTICES[lat].d) for side in (1, -1)]


CASES = (
    [_case(f"kbc-periodic-{lat.lower()}", "oracle", lat, coll="kbc", abb=None, masked=False) for lat in ("D2Q9", "D3Q27")]
    + [_case("kbc-masked-d2q9", "oracle", "D2Q9", coll="kbc", abb=(0, -1), masked=True),
       _case("kbc-masked-d3q27", "oracle", "D3Q27", coll="kbc", abb=(0, 1), masked=True)]
    + [_case(f"bgk-outlet-{lat.lower()}-{'xyz'[axis]}{'+' if side > 0 else '-'}", "oracle", lat, coll="bgk",
             abb=(axis, side), masked=True)
       for lat in ("D2Q9", "D3Q19", "D3Q27") for axis, side in _directions(lat)]
    + [_case(f"smagorinsky-{name}-{lat.lower()}", "smagorinsky", lat, constant=constant)
       for lat in ("D2Q9", "D3Q19", "D3Q27") for name, constant in (("default", 0.17), ("strong", 1.0))]
    + [_case(f"{scheme}-bgk-{lat.lower()}", "force", lat, scheme=scheme)
       for lat in ("D2Q9", "D3Q19") for scheme in ("guo", "shanchen")]
)


def _masks(lat, abb):
    """bounce-back and equilibrium nodes (one feq table) and the outlet of _masked_case, on the CPU"""
    _, ncm, nsm, entries = _masked_case(lat, GRID[lat], torch.float32, abb, SEED + 40)
    return ncm, nsm, entries


def cpu_simulation(kind, lat, what, tau, dtype):
    """the CPU path of a case in `dtype`, from the fp32 state"""
    what = dict(what)
    L = orc.LATTICES[lat]
    f0 = perturbed_state(lat, GRID[lat], torch.float32, SEED).to(dtype)
    if kind == "oracle":
        sim = _Oracle(L, f0, what["coll"], tau)
        if what["masked"]:
            ncm, nsm, entries = _masks(lat, what["abb"])
            sim.boundaries = [_oracle_boundary(L, e, torch.float32) for e in entries]
            for b in sim.boundaries:                            # the plan's fp32 table, in the run's dtype
                if isinstance(b, _Feq):
                    b.feq = b.feq.to(dtype)
            sim.no_collision_mask, sim.no_streaming_mask = ncm, nsm
    elif kind == "smagorinsky":
        sim = smagorinsky._Reference(L, f0, "smagorinsky", tau)
        sim.constant = what["constant"]
    else:
        sim = forces._Reference(L, f0, "bgk", tau)
        sim.scheme, sim.operator, sim.constant = what["scheme"], "bgk", None
        sim.acceleration = forces.ACCELERATION[:L.d]
    return sim


@functools.lru_cache(maxsize=None)
def cpu_pair(kind, lat, what, tau):
    """{n: (cpu_fp32, cpu_fp64)} for n in STEPS, float64 arrays"""
    out = {n: [] for n in STEPS}
    for dtype in (torch.float32, torch.float64):
        sim, done = cpu_simulation(kind, lat, what, tau, dtype), 0
        for n in STEPS:
            sim.step(n - done)
            done = n
            assert sim.f.dtype == dtype
            out[n].append(sim.f.double().numpy().copy())
    return {n: tuple(v) for n, v in out.items()}


def weighted_error(lat, got, want):
    """per population: max over the nodes of |got - want| / w_q"""
    L = orc.LATTICES[lat]
    err = np.abs(np.asarray(got, dtype=np.float64) - want).reshape(L.q, -1).max(axis=1)
    return err / np.asarray(L.w)


def reference_error(kind, lat, what, tau, n):
    """E_ref, after checking the gate's assumptions about the reference: finite, and an error in every weight class"""
    f32, f64 = cpu_pair(kind, lat, what, tau)[n]
    assert np.isfinite(f32).all() and np.isfinite(f64).all()
    per_q = weighted_error(lat, f32, f64)
    for w in sorted(set(orc.LATTICES[lat].w)):
        members = [q for q, wq in enumerate(orc.LATTICES[lat].w) if wq == w]
        assert per_q[members].max() > 0, f"no fp32 error in the weight class {w}"
    return float(per_q.max())


def gpu_plan(kind, lat, what, tau):
    from lettuce_amd._native import Plan
    what = dict(what)
    res = GRID[lat]
    if kind == "oracle":
        if not what["masked"]:
            return Plan(lat, torch.float32, what["coll"], res, [])
        ncm, nsm, entries = _masks(lat, what["abb"])
        plan = Plan(lat, torch.float32, what["coll"], res, entries)
        plan.set_masks(dev(ncm), dev(nsm))
        return plan
    if kind == "smagorinsky":
        plan = Plan(lat, torch.float32, "smagorinsky", res, [])
        plan.set_smagorinsky(what["constant"])
        return plan
    plan = Plan(lat, torch.float32, "bgk", res, [])
    plan.set_force(forces.ACCELERATION[:len(res)], *forces.scales(what["scheme"], tau))
    return plan


@pytest.mark.parametrize("tau", TAUS)
@pytest.mark.parametrize("kind,lat,what", CASES)
def test_gpu_fp32_error_within_the_reference_arithmetics_own(request, kind, lat, what, tau):
    plan = gpu_plan(kind, lat, what, tau)
    f0 = perturbed_state(lat, GRID[lat], torch.float32, SEED)
    factor = FACTORS.get(request.node.callspec.id, FACTOR)
    failures = []
    for n in STEPS:
        e_ref = reference_error(kind, lat, what, tau, n)
        a = dev(f0)
        out, _ = plan.run(a, torch.empty_like(a), tau, n)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert got.dtype == np.float32 and np.isfinite(got).all()
        e_gpu = float(weighted_error(lat, got, cpu_pair(kind, lat, what, tau)[n][1]).max())
        print(f"{request.node.callspec.id} n = {n}: E_ref {e_ref:.3e}  E_gpu {e_gpu:.3e}  ratio {e_gpu / e_ref:.2f}  "
              f"(gate {factor:g}, kernel {plan.kernel_name().split('<')[0]})")
        if not e_gpu <= factor * e_ref:
            failures.append((n, e_ref, e_gpu, e_gpu / e_ref))
    assert not failures, f"(n, E_ref, E_gpu, ratio) beyond {factor:g} x E_ref: {failures}"
