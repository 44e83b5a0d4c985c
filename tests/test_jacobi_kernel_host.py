"""The arithmetic of the Jacobi sweep without a GPU: lettuce_amd/csrc/jacobi.hpp compiles for the host as it stands (its
per-node function and launch geometry; the kernels are left out), around tests/aux/jacobi_host.cpp, with
-ffp-contract=off as the kernels have it by pragma.  Run over every fixture of tests/golden/jacobi_*.npz
(tools/gen_golden_jacobi.py: the reference's torch_jacobi on the CPU): p after 1, 2, 3 and 8 sweeps and the residuum of
the 8th iterate are the reference's bit for bit in fp32 and fp64, and the fp64 sum of r^2 in the order of the two
launches is within (N - 1) * 2^-53 relative of math.fsum over the same squares -- the worst case of any order of N
non-negative terms (N <= 4356 here)."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_pressure_poisson_host import SHAPES, IDS, COUNTS, jacobi_fixture, same_bits

CSRC = os.path.join(ROOT, "lettuce_amd", "csrc")
NP_DT = {"f32": np.float32, "f64": np.float64}


def _compiler():
    for candidate in ("/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if os.path.exists(candidate):
            return candidate
    return shutil.which("clang++") or shutil.which("g++")


@pytest.fixture(scope="module")
def jacobi_host(tmp_path_factory):
    compiler = _compiler()
    if compiler is None:
        pytest.skip("no C++ compiler")
    work = tmp_path_factory.mktemp("jacobi_host")
    exe = work / "jacobi_host"
    subprocess.run([compiler, "-O2", "-std=c++17", "-ffp-contract=off", "-w", "-I" + CSRC,
                    os.path.join(ROOT, "tests", "aux", "jacobi_host.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, timeout=300)
    return work, exe


def sum_bound(r):
    """(fsum of the fp64 squares of r, (N - 1) * 2^-53 of it)"""
    squares = r.astype(np.float64).ravel() ** 2
    exact = math.fsum(squares)
    return exact, (squares.size - 1) * 2.0 ** -53 * exact


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_sweeps_and_residuum_are_the_references_bits(jacobi_host, shape, dt):
    work, exe = jacobi_host
    g = jacobi_fixture(shape)
    n = int(np.prod(shape))
    np.concatenate([g["rhs"].astype(NP_DT[dt]).ravel(), g["p0"].astype(NP_DT[dt]).ravel()]).tofile(work / "in.bin")
    extents = [str(e) for e in shape] + ["1"] * (3 - len(shape))
    out = subprocess.run([str(exe), dt, str(len(shape))] + extents + [repr(float(g["dx"])), "8", str(work / "in.bin"),
                                                                      str(work / "out.bin")], timeout=60)
    assert out.returncode == 0
    raw = (work / "out.bin").read_bytes()
    item = np.dtype(NP_DT[dt]).itemsize
    assert len(raw) == 9 * n * item + 8
    fields = np.frombuffer(raw[:9 * n * item], dtype=NP_DT[dt]).reshape([9] + shape)
    for k in COUNTS:
        assert same_bits(fields[k - 1], g[f"p{k}_{dt}"]), f"{shape} {dt}: p after {k} sweeps"
    assert same_bits(fields[8], g[f"r8_{dt}"]), f"{shape} {dt}: residuum of the 8th iterate"
    total = float(np.frombuffer(raw[9 * n * item:], dtype=np.float64)[0])
    exact, bound = sum_bound(g[f"r8_{dt}"])
    print(f"{shape} {dt}: ordered sum {total:.17e}, fsum {exact:.17e}, |difference| {abs(total - exact):.3e} "
          f"(bound {bound:.3e})")
    assert abs(total - exact) <= bound
    assert exact / n == pytest.approx(float(g[f"err_{dt}"][7]), rel=1e-15)
