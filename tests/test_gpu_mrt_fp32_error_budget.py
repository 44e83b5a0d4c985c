"""fp32 only: the MRT collision, which agrees with the reference "at rounding level" by design, gated by the reference
arithmetic's OWN fp32 error -- the definitions of tests/test_gpu_fp32_error_budget.py, reused by import:
E = max |delta f_q| / w_q, the gate E_gpu <= 4 E_ref, the grids D2Q9 [16, 24] and D3Q27 [6, 8, 10], tau = 0.51 and 0.7
on the second-order moments (distinct rates 1.05 .. 1.85 on the higher ones), 1 and 8 steps.

The CPU path is the mirror's torch operator (test_gpu_mrt.py) in fp32 and in fp64 from the same fp32 state.  The kernels
differ from it by the order of the two sums over q (ascending index against a GEMM's) and nothing else: coefficients,
reciprocal rates and the equilibrium moments are formed as the reference forms them.  The measured ratios are in
DESIGN.md section 2.  Every case prints E_ref, E_gpu and their ratio before it asserts.  That the reference alone stays
inside the gate's assumptions is checked without a GPU in test_mrt_fp32_error_budget_host.py.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import lettuce_oracle as orc
from test_gpu_engine import dev
from test_gpu_fp32_error_budget import FACTOR, GRID, SEED, STEPS, TAUS, weighted_error
from test_gpu_paths_vs_oracle import perturbed_state
from test_mrt_host import TRANSFORMS, rates_of
import test_gpu_mrt as mrt

pytestmark = pytest.mark.gpu

CASES = [pytest.param(t, id=t) for t in TRANSFORMS]


@functools.lru_cache(maxsize=None)
def cpu_pair(transform, tau):
    """{n: (cpu_fp32, cpu_fp64)} for n in STEPS, float64 arrays: the CPU path in both precisions from the fp32 state"""
    lat = mrt.LATTICE[transform]
    out = {n: [] for n in STEPS}
    for dtype in (torch.float32, torch.float64):
        f0 = perturbed_state(lat, GRID[lat], torch.float32, SEED)
        sim = mrt.reference(transform, f0, rates_of(transform, tau), dtype=dtype)
        done = 0
        for n in STEPS:
            sim.step(n - done)
            done = n
            assert sim.f.dtype == dtype
            out[n].append(sim.f.double().numpy().copy())
    return {n: tuple(v) for n, v in out.items()}


def reference_error(transform, tau, n):
    """E_ref, after checking the gate's assumptions about the reference: finite, and an error in every weight class"""
    lat = mrt.LATTICE[transform]
    f32, f64 = cpu_pair(transform, tau)[n]
    assert np.isfinite(f32).all() and np.isfinite(f64).all()
    per_q = weighted_error(lat, f32, f64)
    for w in sorted(set(orc.LATTICES[lat].w)):
        members = [q for q, wq in enumerate(orc.LATTICES[lat].w) if wq == w]
        assert per_q[members].max() > 0, f"no fp32 error in the weight class {w}"
    return float(per_q.max())


@pytest.mark.parametrize("tau", TAUS)
@pytest.mark.parametrize("transform", CASES)
def test_gpu_fp32_error_within_the_reference_arithmetics_own(request, transform, tau):
    lat = mrt.LATTICE[transform]
    plan = mrt.mrt_plan(transform, "f32", GRID[lat], rates_of(transform, tau))
    f0 = perturbed_state(lat, GRID[lat], torch.float32, SEED)
    failures = []
    for n in STEPS:
        e_ref = reference_error(transform, tau, n)
        a = dev(f0)
        out, _ = plan.run(a, torch.empty_like(a), 1.0, n)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert got.dtype == np.float32 and np.isfinite(got).all()
        e_gpu = float(weighted_error(lat, got, cpu_pair(transform, tau)[n][1]).max())
        print(f"{request.node.callspec.id} n = {n}: E_ref {e_ref:.3e}  E_gpu {e_gpu:.3e}  ratio {e_gpu / e_ref:.2f}  "
              f"(gate {FACTOR:g}, kernel {plan.kernel_name().split('<')[0]})")
        if not e_gpu <= FACTOR * e_ref:
            failures.append((n, e_ref, e_gpu, e_gpu / e_ref))
    assert not failures, f"(n, E_ref, E_gpu, ratio) beyond {FACTOR:g} x E_ref: {failures}"
