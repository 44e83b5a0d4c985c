"""The arithmetic of collide_mrt without a GPU: lettuce_amd/csrc/mrt.hpp compiled for the host around
tests/aux/mrt_host.cpp with -ffp-contract=off and run on the initial state of every fixture of tests/golden/mrt_*.npz
and asymmetric_mrt_*.npz, with r_i = T(1) / T(s_i) formed as unit.inc forms them.

The reference's transform is a GEMM whose summation order is not specified, so the comparison is at rounding level:
  fp64   within 2e-14 max(1, |f|max) of the reference's collided field (the asymmetric states reach |f| = 9);
  fp32   E_host <= 4 E_ref with E = max |delta f_q| / w_q against the reference's fp64 result from the same fp32 state,
         E_ref being the reference's own fp32 error (`collided` against `collided_f64` of the fixture).
BGK at the same tau and Dellar's kernel on Lallemand's fixture must be at least 1e-4 away: the harness tells the
operators and the transforms apart.  The tables of mrt.hpp are held against those of lettuce_amd/moments.py entry by
entry.  Every comparison prints its largest difference before it asserts."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import lettuce_amd as lt
from lettuce_amd import moments
from conftest import golden, ROOT
from test_mrt_host import FIXTURES, TRANSFORMS, fixture_flow

CSRC = os.path.join(ROOT, "lettuce_amd", "csrc")
FP64_BOUND, FACTOR = 2e-14, 4.0


def _compiler():
    for candidate in ("/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if os.path.exists(candidate):
            return candidate
    return shutil.which("clang++") or shutil.which("g++")


@pytest.fixture(scope="module")
def mrt_host(tmp_path_factory):
    compiler = _compiler()
    if compiler is None:
        pytest.skip("no C++ compiler")
    work = tmp_path_factory.mktemp("mrt_host")
    exe = work / "mrt_host"
    subprocess.run([compiler, "-O2", "-std=c++17", "-ffp-contract=off", "-w", "-I" + CSRC,
                    os.path.join(ROOT, "tests", "aux", "mrt_host.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, timeout=600)
    return work, exe


def collide(mrt_host, transform, f0, rates, tag="x"):
    work, exe = mrt_host
    f0 = np.ascontiguousarray(f0)
    dt = "f32" if f0.dtype == np.float32 else "f64"
    f0.tofile(work / f"in_{tag}.bin")
    out = subprocess.run([str(exe), transform, dt, str(work / f"in_{tag}.bin"), str(work / f"out_{tag}.bin"),
                          str(f0[0].size)] + [repr(float(s)) for s in rates], timeout=120)
    assert out.returncode == 0
    return np.fromfile(work / f"out_{tag}.bin", dtype=f0.dtype).reshape(f0.shape)


def weighted(transform, got, want):
    """E = max over q and nodes of |got - want| / w_q"""
    w = np.asarray(TRANSFORMS[transform][2]().w).reshape([-1] + [1] * (got.ndim - 1))
    return float((np.abs(got.astype(np.float64) - want) / w).max())


@pytest.mark.parametrize("transform", list(TRANSFORMS))
def test_tables_are_those_of_the_python_module(mrt_host, transform):
    _, exe = mrt_host
    out = subprocess.run([str(exe), "tables", transform], capture_output=True, text=True, check=True, timeout=60).stdout
    table = np.array([[float(v) for v in line.split()] for line in out.strip().splitlines()])
    cls = TRANSFORMS[transform][0]
    q = cls.matrix.shape[0]
    assert table.shape == (2 * q, q)
    assert np.array_equal(table[:q], cls.matrix) and np.array_equal(table[q:], cls.inverse)


@pytest.mark.parametrize("name", FIXTURES)
def test_kernel_arithmetic_matches_the_reference(mrt_host, name):
    g = golden(name)
    _, transform, lat, dt = name.split("_")
    got = collide(mrt_host, transform, g["f0"], g["rates"])
    assert got.dtype == g["f0"].dtype
    if dt == "f64":
        bound = FP64_BOUND * max(1.0, float(np.abs(g["collided"]).max()))
        err = float(np.abs(got - g["collided"]).max())
        print(f"max |difference| {err:.3e} (bound {bound:.1e})")
        assert err <= bound
    else:
        e_ref = weighted(transform, g["collided"], g["collided_f64"])
        e_host = weighted(transform, got, g["collided_f64"])
        print(f"E_ref {e_ref:.3e}  E_host {e_host:.3e}  ratio {e_host / e_ref:.2f} (gate {FACTOR:g})")
        assert e_ref > 0 and e_host <= FACTOR * e_ref
    # ... and BGK at the same tau is not what the fixture holds
    flow = fixture_flow(g, name)[0]
    bgk = lt.BGKCollision(float(g["tau"]))(flow).numpy()
    gap = float(np.abs(bgk.astype(np.float64) - g["collided"]).max())
    print(f"distance of BGK at the same tau: {gap:.2e}")
    assert gap >= 1e-4


@pytest.mark.parametrize("transform", list(TRANSFORMS))
def test_kernel_arithmetic_on_the_asymmetric_states(mrt_host, transform):
    lat = TRANSFORMS[transform][1]
    g, states = golden(f"asymmetric_mrt_{transform}_{lat}_f64"), golden(f"asymmetric_states_{lat}_f64")
    for kind, tau in (("moderate", 0.501), ("wide", 0.7), ("wide", 1.7)):
        key = f"{kind}_tau{tau}"
        want = g[f"{key}_collided"]
        got = collide(mrt_host, transform, states[f"f0_{kind}"], g[f"{key}_rates"])
        bound = FP64_BOUND * max(1.0, float(np.abs(want).max()))
        err = float(np.abs(got - want).max())
        print(f"{key}: max |difference| {err:.3e} (bound {bound:.1e}, |f|max {float(np.abs(want).max()):.2f})")
        assert err <= bound


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_dellars_kernel_is_not_lallemands(mrt_host, dt):
    g = golden(f"mrt_lallemand_d2q9_{dt}")
    wrong = collide(mrt_host, "dellar", g["f0"], g["rates"])
    gap = float(np.abs(wrong.astype(np.float64) - g["collided"]).max())
    print(f"Dellar's kernel on Lallemand's fixture: {gap:.2e}")
    assert gap >= 1e-4
    # a permuted rate shows up as well: the two highest rates swapped
    rates = list(g["rates"])
    rates[-1], rates[-2] = rates[-2], rates[-1]
    swapped = collide(mrt_host, "lallemand", g["f0"], rates)
    gap = float(np.abs(swapped.astype(np.float64) - g["collided"]).max())
    print(f"two rates swapped: {gap:.2e}")
    assert gap >= 10 * (2e-14 if dt == "f64" else 8e-7)
