"""The arithmetic of pressure_outlet_apply without a GPU: the text of the function is cut out of
lettuce_amd/csrc/kernels.hpp together with the moments and the equilibrium it calls, compiled for the host around
tests/aux/outlet_p_host.cpp and run on the outlet planes of the fixtures with one outlet (tests/golden/outlet_p_*.npz):
in the reference's collided field the plane holds feq(rho_outlet, u) of the plane next to it, which no later boundary
has touched.  Bounds as in test_relaxations_kernel_host.py: fp64 2e-14, fp32 8e-7."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import golden, ROOT
from outlet_p_cases import SINGLE, ROWS, dtype_tag, lattice_of

CSRC = os.path.join(ROOT, "lettuce_amd", "csrc")
ATOL = {"f64": 2e-14, "f32": 8e-7}


def _compiler():
    for candidate in ("/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if os.path.exists(candidate):
            return candidate
    return shutil.which("clang++") or shutil.which("g++")


def _excerpt():
    text = open(os.path.join(CSRC, "kernels.hpp")).read()
    constants = text[text.index("// ---- constants the reference builds"):text.index("// ---- population access")]
    collide = text[text.index("// ---- moments"):text.index("// ---- boundaries")]
    outlet = text[text.index("// EquilibriumOutletP ("):text.index("// What the boundaries with an index below")]
    assert "pressure_outlet_apply" in outlet and "for_each_feq" in outlet and "pressure_outlet_apply" not in collide
    lines = [line for line in (constants + collide + outlet).splitlines() if "launder" not in line]
    return "\n".join(lines).replace("__builtin_amdgcn_rcpf(y)", "(1.0f / (y))") + "\n"


@pytest.fixture(scope="module")
def outlet_host(tmp_path_factory):
    compiler = _compiler()
    if compiler is None:
        pytest.skip("no C++ compiler")
    work = tmp_path_factory.mktemp("outlet_p_host")
    (work / "outlet_p_excerpt.inc").write_text(_excerpt())
    exe = work / "outlet_p_host"
    subprocess.run([compiler, "-O2", "-std=c++17", "-ffp-contract=off", "-w", "-I" + CSRC, "-I" + str(work),
                    os.path.join(ROOT, "tests", "aux", "outlet_p_host.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, timeout=300)
    return work, exe


@pytest.mark.parametrize("name", SINGLE + ROWS)
def test_device_function_text_matches_the_reference(outlet_host, name):
    work, exe = outlet_host
    g = golden(name)
    dt = dtype_tag(name)
    kinds = [str(k) for k in g["boundary_order"]]
    slot = kinds.index("EquilibriumOutletP")
    assert slot == len(kinds) - 1                        # the last boundary: nothing rewrites its plane or its neighbour
    direction = g["boundary_direction"][slot]
    axis = int(np.nonzero(direction)[0][0])
    here = [slice(None)] * (1 + len(direction))
    there = list(here)
    here[1 + axis], there[1 + axis] = (-1, -2) if direction[axis] > 0 else (0, 1)
    want = g["collided"][tuple(here)]
    neighbour = np.ascontiguousarray(g["collided"][tuple(there)])
    neighbour.tofile(work / "in.bin")
    nodes = neighbour[0].size
    out = subprocess.run([str(exe), lattice_of(name), dt, str(work / "in.bin"), str(work / "out.bin"), str(nodes),
                          repr(float(g["rho_outlet"][slot]))], timeout=60)
    assert out.returncode == 0
    got = np.fromfile(work / "out.bin", dtype=neighbour.dtype).reshape(neighbour.shape)
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(f"max |difference| {err:.3e} (bound {ATOL[dt]:.1e})")
    assert err <= ATOL[dt]
    # ... and another density is not what the fixture holds: the harness tells rho_outlet apart
    subprocess.run([str(exe), lattice_of(name), dt, str(work / "in.bin"), str(work / "off.bin"), str(nodes),
                    repr(float(g["rho_outlet"][slot]) + 0.02)], check=True, timeout=60)
    off = np.fromfile(work / "off.bin", dtype=neighbour.dtype).reshape(neighbour.shape)
    assert float(np.abs(off.astype(np.float64) - want).max()) >= 1e-4
