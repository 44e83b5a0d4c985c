"""Which kernel a unit picks for which arguments is behaviour: bench.py, the profiling tools and the tests match on
the names, and a refactoring of csrc/unit.inc must not move a plan to another kernel.  tests/aux/dispatch_table.cpp
asks every unit's name function (nothing launches) for every combination of the arguments that path reads -- 451 584
selectors per unit -- and prints, per unit, the distinct names, the number of selectors with a kernel and a hash over
the whole ordered table; tests/dispatch_table.txt is that output of the library as it was before the ladders of
unit.inc became one walk over a stated set (the program linked against a library built from that commit's csrc/)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _units(text):
    """{unit: its lines} in the order of the output"""
    units = {}
    for line in text.splitlines():
        if line.startswith("unit "):
            units[line[5:]] = lines = []
        else:
            lines.append(line)
    return units


def _hipcc():
    return "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")


def test_every_unit_names_the_same_kernel_for_every_selector(engine_library, tmp_path):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not available")
    libdir = os.path.dirname(engine_library)
    exe = tmp_path / "dispatch_table"
    subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-Wall", "-Werror",
                    "-I" + os.path.join(ROOT, "lettuce_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "aux", "dispatch_table.cpp"), "-L" + libdir, "-llettuce_hip",
                    "-Wl,-rpath," + libdir, "-o", str(exe)], check=True, capture_output=True, timeout=600)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stderr)
    want = _units(open(os.path.join(ROOT, "tests", "dispatch_table.txt")).read())
    got = _units(out.stdout)
    assert len(want) == 10 and list(got) == list(want), (list(got), list(want))
    for unit in want:
        for i, (g, w) in enumerate(zip(got[unit] + [None], want[unit] + [None])):
            assert g == w, f"{unit}: line {i + 1} of its table is {g!r}, the fixture has {w!r}"
        assert len(got[unit]) == len(want[unit]), (unit, len(got[unit]), len(want[unit]))
    assert out.stdout == open(os.path.join(ROOT, "tests", "dispatch_table.txt")).read()


def test_collision_numbers_and_their_predicates(tmp_path):
    """dispatch.hpp's names for the kernels' collision numbers: tests/aux/collision_numbers.cpp holds every number, and
    coll_forced / coll_mrt / coll_base of it, against the values written out (5 and 7 forced, on 1 and 3; 10 and 11 MRT;
    8 and 9 neither), and the names against the ABI's lt_collision where they coincide.  Host code only."""
    hipcc = _hipcc()
    assert hipcc is not None, "the engine is built with hipcc"
    exe = tmp_path / "collision_numbers"
    subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-Wall", "-Werror",
                    "-I" + os.path.join(ROOT, "lettuce_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "aux", "collision_numbers.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, timeout=600)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    print(out.stdout)
    assert out.returncode == 0, out.stdout
    assert len(out.stdout.splitlines()) == 10 and "wrong" not in out.stdout
