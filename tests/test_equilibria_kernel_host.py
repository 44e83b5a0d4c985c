"""The arithmetic of the collide functions with the incompressible equilibrium without a GPU: the text of the collide
functions is cut out of lettuce_amd/csrc/kernels.hpp (between its section markers, as test_relaxations_kernel_host.py cuts
it), compiled for the host around tests/aux/equilibria_host.cpp and run on f0 of every periodic fixture of
tests/golden/incompressible_*.npz, with the scalars formed as unit.inc forms them.  The result is held against the
reference's collided field with that test's bounds (fp64 2e-14, fp32 8e-7); the quadratic equilibrium and rho0 = 1.0 on
the same input must miss the fixture by at least 1e-4."""
import os
import subprocess

import numpy as np
import pytest

from conftest import golden, ROOT
from test_relaxations_host import ATOL
from test_relaxations_kernel_host import CSRC, _compiler, _excerpt
from test_equilibria_host import FIXTURES


@pytest.fixture(scope="module")
def equilibria_host(tmp_path_factory):
    compiler = _compiler()
    if compiler is None:
        pytest.skip("no C++ compiler")
    work = tmp_path_factory.mktemp("equilibria_host")
    excerpt = _excerpt()
    assert "feq_inc_q" in excerpt and "feq_inc_pair" in excerpt and "for_each_feq_inc" in excerpt
    (work / "collide_excerpt.inc").write_text(excerpt)
    exe = work / "equilibria_host"
    subprocess.run([compiler, "-O2", "-std=c++17", "-ffp-contract=off", "-w", "-I" + CSRC, "-I" + str(work),
                    os.path.join(ROOT, "tests", "aux", "equilibria_host.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, timeout=300)
    return work, exe


def collide(work, exe, g, name, equilibrium, rho0, out):
    _, operator, lat, dt = name.split("_")
    f0 = np.ascontiguousarray(g["f0"])
    f0.tofile(work / "in.bin")
    subprocess.run([str(exe), operator, lat, dt, str(work / "in.bin"), str(work / out), str(f0[0].size),
                    repr(float(g["tau"])), repr(float(g["tau_minus"]) or 1.0), repr(float(g["acceleration"])),
                    str(equilibrium), repr(rho0)], check=True, timeout=60)
    return np.fromfile(work / out, dtype=f0.dtype).reshape(f0.shape).astype(np.float64)


@pytest.mark.parametrize("name", FIXTURES)
def test_kernel_arithmetic_matches_the_reference(equilibria_host, name):
    work, exe = equilibria_host
    g = golden(name)
    dt = name.split("_")[-1]
    got = collide(work, exe, g, name, 1, float(g["rho0"]), "out.bin")
    err = float(np.abs(got - g["collided"]).max())
    print(f"max |difference| {err:.3e} (bound {ATOL[dt]:.1e})")
    assert err <= ATOL[dt]
    # ... and neither the quadratic equilibrium nor rho0 = 1.0 is what the fixture holds
    quadratic = collide(work, exe, g, name, 0, 1.0, "quadratic.bin")
    one = collide(work, exe, g, name, 1, 1.0, "one.bin")
    gaps = float(np.abs(quadratic - g["collided"]).max()), float(np.abs(one - g["collided"]).max())
    print(f"quadratic {gaps[0]:.2e}, rho0 = 1.0 {gaps[1]:.2e}")
    assert gaps[0] >= 1e-4 and gaps[1] >= 1e-4
