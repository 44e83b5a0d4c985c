"""fp32 only: the TRT and the regularised collision, which agree with the reference "at rounding level" by design,
gated by the reference arithmetic's OWN fp32 error -- the definitions of tests/test_gpu_fp32_error_budget.py, reused by
import: E = max |delta f_q| / w_q, the gate E_gpu <= 4 E_ref, the grids D2Q9 [16, 24], D3Q19 and D3Q27 [6, 8, 10],
tau = 0.51 and 0.7, 1 and 8 steps.

TRT's tau_minus is 0.5 + (3 / 16) / (tau_plus - 0.5), the "magic" combination that fixes the bounce-back wall half way:
19.25 and 1.4375.  The CPU path is the mirror's torch operator (test_gpu_relaxations.py); E_ref is 3.9e-7 .. 2.3e-6 for
both operators.  The kernels differ from it by a handful of single roundings per population: a product with
1 / (2 tau) for a division, 1 - 1 / tau rounded once, Pi summed over opposite pairs instead of in index order.  The
measured ratios are in DESIGN.md section 2.  Every case prints E_ref, E_gpu and their ratio before it asserts.  That the
reference alone stays inside the gate's assumptions is checked without a GPU in
test_relaxations_fp32_error_budget_host.py.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import lettuce_oracle as orc
from test_gpu_engine import dev
from test_gpu_fp32_error_budget import FACTOR, GRID, SEED, STEPS, TAUS, weighted_error
from test_gpu_paths_vs_oracle import perturbed_state
import test_gpu_relaxations as relaxations

pytestmark = pytest.mark.gpu

CASES = [pytest.param(operator, lat, id=f"{operator}-{lat.lower()}") for operator in relaxations.OPERATORS for lat in GRID]


def tau_minus_of(tau):
    return 0.5 + (3.0 / 16.0) / (tau - 0.5)


@functools.lru_cache(maxsize=None)
def cpu_pair(operator, lat, tau):
    """{n: (cpu_fp32, cpu_fp64)} for n in STEPS, float64 arrays: the CPU path in both precisions from the fp32 state"""
    out = {n: [] for n in STEPS}
    for dtype in (torch.float32, torch.float64):
        f0 = perturbed_state(lat, GRID[lat], torch.float32, SEED).to(dtype)
        sim = relaxations._Reference(orc.LATTICES[lat], f0, operator, tau)
        sim.operator, sim.tau_minus = operator, tau_minus_of(tau)
        done = 0
        for n in STEPS:
            sim.step(n - done)
            done = n
            assert sim.f.dtype == dtype
            out[n].append(sim.f.double().numpy().copy())
    return {n: tuple(v) for n, v in out.items()}


def reference_error(operator, lat, tau, n):
    """E_ref, after checking the gate's assumptions about the reference: finite, and an error in every weight class"""
    f32, f64 = cpu_pair(operator, lat, tau)[n]
    assert np.isfinite(f32).all() and np.isfinite(f64).all()
    per_q = weighted_error(lat, f32, f64)
    for w in sorted(set(orc.LATTICES[lat].w)):
        members = [q for q, wq in enumerate(orc.LATTICES[lat].w) if wq == w]
        assert per_q[members].max() > 0, f"no fp32 error in the weight class {w}"
    return float(per_q.max())


@pytest.mark.parametrize("tau", TAUS)
@pytest.mark.parametrize("operator,lat", CASES)
def test_gpu_fp32_error_within_the_reference_arithmetics_own(request, operator, lat, tau):
    plan = relaxations.make_plan(operator, lat, "f32", GRID[lat], tau_minus=tau_minus_of(tau))
    f0 = perturbed_state(lat, GRID[lat], torch.float32, SEED)
    failures = []
    for n in STEPS:
        e_ref = reference_error(operator, lat, tau, n)
        a = dev(f0)
        out, _ = plan.run(a, torch.empty_like(a), tau, n)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert got.dtype == np.float32 and np.isfinite(got).all()
        e_gpu = float(weighted_error(lat, got, cpu_pair(operator, lat, tau)[n][1]).max())
        print(f"{request.node.callspec.id} n = {n}: E_ref {e_ref:.3e}  E_gpu {e_gpu:.3e}  ratio {e_gpu / e_ref:.2f}  "
              f"(gate {FACTOR:g}, kernel {plan.kernel_name().split('<')[0]})")
        if not e_gpu <= FACTOR * e_ref:
            failures.append((n, e_ref, e_gpu, e_gpu / e_ref))
    assert not failures, f"(n, E_ref, E_gpu, ratio) beyond {FACTOR:g} x E_ref: {failures}"
