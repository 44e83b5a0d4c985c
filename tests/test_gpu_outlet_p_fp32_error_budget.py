"""fp32 only: the constant-pressure equilibrium outlet gated by the reference arithmetic's OWN fp32 error -- the
definitions of tests/test_gpu_fp32_error_budget.py, reused by import: E = max |delta f_q| / w_q, the gate
E_gpu <= 4 E_ref, the grids D2Q9 [16, 24], D3Q19 and D3Q27 [6, 8, 10], tau = 0.51 and 0.7, 1 and 8
steps.

The flow: an equilibrium inlet at x = 0, a bounce-back block in the middle, an EquilibriumOutletP on +x with rho_outlet
= fp32(1.02), BGK.  The CPU path is the mirror's torch path (pinned to the reference's vectors by test_outlet_p_host.py),
run in fp32 and in fp64 from the same fp32 state; the density is the fp32 value in both.  The kernel's feq on the outlet
plane is the reference's bit for bit; what differs is the neighbour's velocity, taken from the moments of the
pre-collision populations (collision conserves them) where the reference sums the collided ones.  The measured ratios
are in DESIGN.md section 2.  Every case prints E_ref, E_gpu and their ratio before it asserts.  That the reference alone
stays inside the gate's assumptions is checked without a GPU in test_outlet_p_fp32_error_budget_host.py."""
import functools

import numpy as np
import pytest
import torch

import lettuce_amd as lt
from oracle import lettuce_oracle as orc
from outlet_p_cases import mirror_flow
from test_gpu_engine import dev
from test_gpu_fp32_error_budget import FACTOR, GRID, SEED, STEPS, TAUS, weighted_error
from test_gpu_paths_vs_oracle import perturbed_state

pytestmark = pytest.mark.gpu

CASES = list(GRID)
RHO_OUTLET = float(np.float32(1.02))


def description(lat):
    res = GRID[lat]
    d = len(res)
    inlet = np.zeros(res, dtype=bool)
    inlet[0] = True
    block = np.zeros(res, dtype=bool)
    block[tuple(slice(n // 2 - 1, n // 2 + 1) for n in res)] = True
    return {"resolution": np.array(res),
            "boundary_order": np.array(["BounceBackBoundary", "EquilibriumBoundaryPU", "EquilibriumOutletP"]),
            "boundary_direction": np.array([[0] * d, [0] * d, [1] + [0] * (d - 1)]),
            "rho_outlet": np.array([0.0, 0.0, RHO_OUTLET]), "inlet_mask": inlet, "block_mask": block,
            "inlet_velocity_pu": np.array([1.0] + [0.0] * (d - 1)), "reynolds": 100.0, "mach": 0.05, "domain_length_x": 2.0}


def cpu_simulation(lat, tau, dtype):
    name = f"outlet_p_budget_{lat.lower()}_f32"
    flow = mirror_flow(description(lat), name, lt.Context("cpu", dtype, use_native=False), set_f0=False)
    flow.f = perturbed_state(lat, GRID[lat], torch.float32, SEED).to(dtype)
    return flow, lt.Simulation(flow, lt.BGKCollision(tau), [])


@functools.lru_cache(maxsize=None)
def cpu_pair(lat, tau):
    """{n: (cpu_fp32, cpu_fp64)} for n in STEPS, float64 arrays: the CPU path in both precisions from the fp32 state"""
    out = {n: [] for n in STEPS}
    for dtype in (torch.float32, torch.float64):
        flow, sim = cpu_simulation(lat, tau, dtype)
        done = 0
        for n in STEPS:
            sim(n - done)
            done = n
            assert flow.f.dtype == dtype
            out[n].append(flow.f.double().numpy().copy())
    return {n: tuple(v) for n, v in out.items()}


def reference_error(lat, tau, n):
    """E_ref, after checking the gate's assumptions about the reference: finite, and an error in every weight class"""
    f32, f64 = cpu_pair(lat, tau)[n]
    assert np.isfinite(f32).all() and np.isfinite(f64).all()
    per_q = weighted_error(lat, f32, f64)
    for w in sorted(set(orc.LATTICES[lat].w)):
        members = [q for q, wq in enumerate(orc.LATTICES[lat].w) if wq == w]
        assert per_q[members].max() > 0, f"no fp32 error in the weight class {w}"
    return float(per_q.max())


@pytest.mark.parametrize("tau", TAUS)
@pytest.mark.parametrize("lat", CASES)
def test_gpu_fp32_error_within_the_reference_arithmetics_own(request, lat, tau):
    from lettuce_amd._native import Plan
    flow, sim = cpu_simulation(lat, tau, torch.float32)
    entries = [b.native_generator(i).plan_entry(flow) for i, b in enumerate(sim.boundaries[1:], start=1)]
    assert [e["kind"] for e in entries] == ["bounce_back", "equilibrium", "pressure_outlet"]
    plan = Plan(lat, torch.float32, "bgk", GRID[lat], entries)
    plan.set_masks(dev(sim.no_collision_mask.to(torch.uint8)), dev(sim.no_streaming_mask.to(torch.uint8)))
    assert plan.kernel_name().endswith(f", {5 if len(GRID[lat]) == 2 else 6}>"), plan.kernel_name()
    f0 = perturbed_state(lat, GRID[lat], torch.float32, SEED)
    failures = []
    for n in STEPS:
        e_ref = reference_error(lat, tau, n)
        a = dev(f0)
        out, _ = plan.run(a, torch.empty_like(a), tau, n)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert got.dtype == np.float32 and np.isfinite(got).all()
        e_gpu = float(weighted_error(lat, got, cpu_pair(lat, tau)[n][1]).max())
        print(f"{request.node.callspec.id} n = {n}: E_ref {e_ref:.3e}  E_gpu {e_gpu:.3e}  ratio {e_gpu / e_ref:.2f}  "
              f"(gate {FACTOR:g}, kernel {plan.kernel_name().split('<')[0]})")
        if not e_gpu <= FACTOR * e_ref:
            failures.append((n, e_ref, e_gpu, e_gpu / e_ref))
    assert not failures, f"(n, E_ref, E_gpu, ratio) beyond {FACTOR:g} x E_ref: {failures}"
