"""The role-separated two-step sweep (lbm2_kernel, SCHED = 1) lets producer and consumer waves run their own loops
between shared workgroup barriers: a different barrier count in the two roles for some segment length would hang the
GPU.  Both roles therefore run ONE control skeleton (csrc/twostep_roles.hpp); this compiles it for the host with
counting operations (tests/aux/role_sweep_count.cpp) -- no GPU, no hipcc."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_both_roles_meet_the_same_barriers_and_lds_slots_in_order(tmp_path):
    """segments of 1 .. 130 planes: equal barrier counts per role (= planes), every intermediate plane loaded and filled
    once and in order with the next plane's loads in flight, every output plane drained from slots that hold its three
    planes, no fill into a slot the same interval's drain reads"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "role_sweep_count"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "lettuce_amd", "csrc"),
                    os.path.join(ROOT, "tests", "aux", "role_sweep_count.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok 260", (out.stdout, out.stderr)


def test_wave_layout_of_the_instantiations():
    """11 + 4 waves for 64 x 8 fp32 tiles (consumers take two nodes per thread), 6 + 4 for 32 x 8: checked where the
    header computes it, by a static_assert-only translation unit"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src = ('#include "twostep_roles.hpp"\n'
           "using A = lt::RoleWaves<66 * 10, 64 * 8>;\n"
           "static_assert(A::PW == 11 && A::CW == 4 && A::CPB == 2 && A::THREADS == 960, \"64 x 8\");\n"
           "using B = lt::RoleWaves<34 * 10, 32 * 8>;\n"
           "static_assert(B::PW == 6 && B::CW == 4 && B::CPB == 1 && B::THREADS == 640, \"32 x 8\");\n")
    subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-x", "c++", "-I", os.path.join(ROOT, "lettuce_amd", "csrc"), "-"],
                   input=src, text=True, check=True)
