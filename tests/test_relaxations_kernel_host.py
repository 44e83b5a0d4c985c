"""The arithmetic of collide_trt and collide_regularized without a GPU: the text of the collide functions is cut out of
lettuce_amd/csrc/kernels.hpp (between its section markers), compiled for the host around tests/aux/collide_host.cpp and
run on the initial state of every fixture of tests/golden/trt_*.npz and regularized_*.npz, with the scalars formed as
unit.inc forms them.  The result is held against the reference's collided field with the bounds of the host tests (fp64
2e-14, fp32 8e-7).  The two target-specific lines of that text are replaced: the value barrier `launder` (inline
assembly, used by no collision) is dropped and KBC's hardware reciprocal becomes a division."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import golden, ROOT
from test_relaxations_host import ATOL, FIXTURES

CSRC = os.path.join(ROOT, "lettuce_amd", "csrc")


def _compiler():
    for candidate in ("/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if os.path.exists(candidate):
            return candidate
    return shutil.which("clang++") or shutil.which("g++")


def _excerpt():
    text = open(os.path.join(CSRC, "kernels.hpp")).read()
    constants = text[text.index("// ---- constants the reference builds"):text.index("// ---- population access")]
    collide = text[text.index("// ---- moments"):text.index("// ---- boundaries")]
    assert "collide_trt" in collide and "collide_regularized" in collide and "collide_bgk" in collide
    lines = [line for line in (constants + collide).splitlines() if "launder" not in line]
    return "\n".join(lines).replace("__builtin_amdgcn_rcpf(y)", "(1.0f / (y))") + "\n"


@pytest.fixture(scope="module")
def collide_host(tmp_path_factory):
    compiler = _compiler()
    if compiler is None:
        pytest.skip("no C++ compiler")
    work = tmp_path_factory.mktemp("collide_host")
    (work / "collide_excerpt.inc").write_text(_excerpt())
    exe = work / "collide_host"
    subprocess.run([compiler, "-O2", "-std=c++17", "-ffp-contract=off", "-w", "-I" + CSRC, "-I" + str(work),
                    os.path.join(ROOT, "tests", "aux", "collide_host.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, timeout=300)
    return work, exe


@pytest.mark.parametrize("name", FIXTURES)
def test_kernel_arithmetic_matches_the_reference(collide_host, name):
    work, exe = collide_host
    g = golden(name)
    operator, lat, dt = name.split("_")
    f0 = np.ascontiguousarray(g["f0"])
    f0.tofile(work / "in.bin")
    out = subprocess.run([str(exe), operator, lat, dt, str(work / "in.bin"), str(work / "out.bin"), str(f0[0].size),
                          repr(float(g["tau"])), repr(float(g["tau_minus"]) or 1.0)], timeout=60)
    assert out.returncode == 0
    got = np.fromfile(work / "out.bin", dtype=f0.dtype).reshape(f0.shape)
    err = float(np.abs(got.astype(np.float64) - g["collided"]).max())
    print(f"max |difference| {err:.3e} (bound {ATOL[dt]:.1e})")
    assert err <= ATOL[dt]
    # ... and BGK at the same tau is not what the fixture holds: the harness tells the operators apart
    subprocess.run([str(exe), "bgk", lat, dt, str(work / "in.bin"), str(work / "bgk.bin"), str(f0[0].size),
                    repr(float(g["tau"])), "1.0"], check=True, timeout=60)
    bgk = np.fromfile(work / "bgk.bin", dtype=f0.dtype).reshape(f0.shape)
    assert float(np.abs(bgk.astype(np.float64) - g["collided"]).max()) >= 1e-4
