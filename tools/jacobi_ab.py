"""The Jacobi pressure solver on the HIP path against the reference's torch expression ON THE SAME DEVICE, in one process
on the same fields, timed to convergence (tol_abs = 1e-10, at most 100 000 sweeps: the defaults of pressure_poisson).
  "torch"     util._jacobi_expression on device tensors: eight rolls, a mean and a host synchronisation per sweep --
              what pressure_poisson would run without the engine
  "hip_K"     _native.jacobi (lt_jacobi) with batch = K in {16, 64, 256}: K sweeps enqueued per look at the stop flag
The field is the pressure-Poisson problem of the Taylor-Green vortex (Re 100, Ma 0.05, rho0 = 1): 256^2 and 1024^2 in
fp64 (D2Q9), 64^3 in fp32 (D3Q27).  seconds = a host clock around one solve, which ends in a device synchronise on
either path; every side is warmed with a short solve of the same shape first, the sides alternate, SAMPLES samples each
(the torch side one where a solve takes more than LONG seconds).  Also recorded: the iterations of each side (they must
agree), the largest difference of the results, and the mean time per sweep.  No pass/fail number.
usage: jacobi_ab.py [--cases 256x256:f64,1024x1024:f64,64x64x64:f32] [--out profiles/jacobi_ab.jsonl]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import lettuce_amd as lt
from lettuce_amd import _native, util
from lettuce_amd._flow import _poisson_problem

SAMPLES, LONG = 3, 8.0
BATCHES = (16, 64, 256)
TOL, MAX_STEPS = 1e-10, 100000
DT = {"f32": torch.float32, "f64": torch.float64}


def option(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


CASES = [(list(map(int, c.split(":")[0].split("x"))), c.split(":")[1])
         for c in option("--cases", "256x256:f64,1024x1024:f64,64x64x64:f32").split(",")]
OUT = option("--out", os.path.join(ROOT, "profiles", "jacobi_ab.jsonl"))


def problem(res, dt):
    ctx = lt.Context(device="cuda:0", dtype=DT[dt], use_native=True)
    flow = lt.TaylorGreenVortex(ctx, res, 100, 0.05, lt.D2Q9() if len(res) == 2 else lt.D3Q27(), initialize_fneq=False)
    p0, u = flow.initial_pu()
    u = flow.units.convert_velocity_to_lu(u)
    rho0 = torch.ones_like(flow.units.convert_pressure_pu_to_density_lu(p0))
    return _poisson_problem(flow.units, u, rho0)


def timed(call):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = call()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    assert torch.cuda.is_available(), "jacobi_ab.py measures on the GPU"
    lines = []
    for res, dt in CASES:
        rhs, p, dx = problem(res, dt)
        dim = len(res)
        sides = {"torch": lambda steps=MAX_STEPS: (util._jacobi_expression(rhs, p, dx, dim, TOL, steps), None)}
        for k in BATCHES:
            sides[f"hip_{k}"] = lambda steps=MAX_STEPS, k=k: _native.jacobi(rhs, p, dx, TOL, steps, batch=k)[:2]
        for call in sides.values():
            call(300)                                   # warm-up: code objects, allocator, the shapes of the window
        seconds = {name: [] for name in sides}
        results, iterations = {}, {}
        for sample in range(SAMPLES):
            for name, call in sides.items():
                if name == "torch" and sample > 0 and seconds[name][0] > LONG:
                    continue
                t, (result, its) = timed(call)
                seconds[name].append(round(t, 4))
                results[name], iterations[name] = result, its
        its = iterations["hip_64"]
        assert all(iterations[f"hip_{k}"] == its for k in BATCHES), iterations
        assert all(torch.equal(results[f"hip_{k}"], results["hip_64"]) for k in BATCHES)
        median = {name: statistics.median(v) for name, v in seconds.items()}
        record = {"what": "Jacobi to tol_abs 1e-10, Taylor-Green pressure-Poisson problem", "resolution": res, "dtype": dt,
                  "iterations": its, "hit_max_num_steps": its == MAX_STEPS, "seconds": seconds, "median_seconds": median,
                  "us_per_sweep": {name: round(1e6 * m / max(its, 1), 3) for name, m in median.items()},
                  "torch_over_hip": {name: round(median["torch"] / m, 2) for name, m in median.items() if name != "torch"},
                  "max_difference_hip_torch": float((results["hip_64"] - results["torch"]).abs().max()),
                  "max_abs_result": float(results["torch"].abs().max())}
        lines.append(json.dumps(record))
        print(lines[-1], flush=True)
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        with open(OUT, "w") as out:
            out.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
