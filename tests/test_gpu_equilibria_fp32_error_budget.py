"""fp32 only: the collisions with the incompressible equilibrium (rho0 = 1.1), gated by the reference arithmetic's OWN
fp32 error as test_gpu_fp32_error_budget.py gates the other operations, whose definitions are used unchanged
(weighted_error, FACTOR = 4, GRID, TAUS, STEPS, SEED):

    E_ref = max over q and nodes of |cpu_fp32 - cpu_fp64| / w_q
    E_gpu = max over q and nodes of |gpu_fp32 - cpu_fp64| / w_q,        gate: E_gpu <= FACTOR * E_ref

for BGK, TRT and the regularised collision.  The CPU path is the mirror's torch path (test_equilibria_host.py pins it to
the reference's vectors), run in fp32 and in fp64 from the same fp32 state.  That the reference alone stays inside the
gate's assumptions is checked without a GPU in test_equilibria_fp32_error_budget_host.py.  The measured ratios are in
DESIGN.md section 2.  Every case prints E_ref, E_gpu and their ratio before it asserts.
"""
import functools

import numpy as np
import pytest
import torch

import lettuce_amd as lt
from oracle import lettuce_oracle as orc
from test_gpu_engine import dev
from test_gpu_fp32_error_budget import FACTOR, GRID, SEED, STEPS, TAUS, weighted_error
from test_gpu_paths_vs_oracle import perturbed_state
from test_host_api import UniformFlow

pytestmark = pytest.mark.gpu

RHO0 = 1.1
TAU_MINUS = 2.5
OPERATORS = ("bgk", "trt", "regularized")
CASES = [pytest.param(operator, lat, id=f"{operator}-{lat.lower()}") for operator in OPERATORS for lat in GRID]
STENCILS = {"D2Q9": lt.D2Q9, "D3Q19": lt.D3Q19, "D3Q27": lt.D3Q27}


def cpu_collision(operator, flow, tau):
    if operator == "bgk":
        return lt.BGKCollision(tau)
    if operator == "trt":
        return lt.TRTCollision(tau, TAU_MINUS)
    collision = lt.RegularizedCollision()
    collision.native_generator().tau(flow)         # the first use takes the flow's tau ...
    collision.tau = tau                            # ... which an assignment replaces
    return collision


@functools.lru_cache(maxsize=None)
def cpu_pair(operator, lat, tau):
    """{n: (cpu_fp32, cpu_fp64)} for n in STEPS, float64 arrays"""
    out = {n: [] for n in STEPS}
    for dtype in (torch.float32, torch.float64):
        context = lt.Context("cpu", dtype, use_native=False)
        flow = UniformFlow(context, GRID[lat], 1, 0.01, STENCILS[lat](), lt.IncompressibleQuadraticEquilibrium(RHO0))
        flow.f = perturbed_state(lat, GRID[lat], torch.float32, SEED).to(dtype)
        sim, done = lt.Simulation(flow, cpu_collision(operator, flow, tau), []), 0
        for n in STEPS:
            sim(n - done)
            done = n
            assert flow.f.dtype == dtype
            out[n].append(flow.f.double().numpy().copy())
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
    from lettuce_amd._native import Plan
    plan = Plan(lat, torch.float32, operator, GRID[lat], [])
    if operator == "trt":
        plan.set_trt(TAU_MINUS)
    plan.set_equilibrium("incompressible", RHO0)
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
              f"(gate {FACTOR:g}, kernel {plan.kernel_name().split('>')[0]})")
        if not e_gpu <= FACTOR * e_ref:
            failures.append((n, e_ref, e_gpu, e_gpu / e_ref))
    assert not failures, f"(n, E_ref, E_gpu, ratio) beyond {FACTOR:g} x E_ref: {failures}"
