"""The one-step kernels exist twice: with cached loads and stores (the kernels' TUNE = 0) and with nontemporal ones
(TUNE = 3), as separate instantiations with their own register allocation and schedule.  lt_run picks 3 above 128 MiB
of populations, which is where users run and where no parity test is.  tests/aux/tune3_census.cpp asks every unit's
name function (nothing launches) for every one-step selector with cache policy 3 -- both layouts, the three modes,
with and without masks, with and without a constant-pressure outlet, the three outlet depths, the outlet slot of the
contiguous axis, all collision numbers of dispatch.hpp -- and prints, per unit, each distinct TUNE = 3 kernel with
one selector that reaches it.  tests/tune3_census.txt is that output; tests/test_gpu_tune3_vs_cpu.py has a GPU case for
each of its lines, so an instantiation added to csrc/unit.inc without one fails here."""
import os
import re
import subprocess

import pytest

from test_dispatch_table import ROOT, _hipcc, _units

FIXTURE = os.path.join(ROOT, "tests", "tune3_census.txt")
# every collision number of dispatch.hpp and the units that have kernels for it
ALL_UNITS = {"d2q9", "d3q19", "d3q27", "d1q3", "d3q15"}
COLLISIONS = {0: ALL_UNITS, 1: ALL_UNITS, 2: {"d2q9", "d3q27"}, 3: ALL_UNITS, 5: ALL_UNITS, 7: ALL_UNITS, 8: ALL_UNITS,
              9: ALL_UNITS, 10: {"d2q9", "d3q27"}, 11: {"d2q9"}, 17: ALL_UNITS, 21: ALL_UNITS, 24: ALL_UNITS, 25: ALL_UNITS}
LINE = re.compile(r"  (lbm_kernel(?:_occ4)?)<(float|double), lt::(\w+), (\d), (\d+), (true|false), (true|false), (true|false), "
                  r"1, 0, 3, false(?:, (\d+))?> \| layout=(\d) coll=(\d+) mode=(\d) masked=(\d) n_pout=(\d) abb_depth=(\d) "
                  r"abb0_slot=(\d)$")


def census_lines(text=None):
    """[(unit, kernel name, {selector field: value})] of the fixture (or of `text`), in its order"""
    out = []
    for unit, lines in _units(open(FIXTURE).read() if text is None else text).items():
        for line in lines[:-1]:
            name, selector = line.strip().split(" | ")
            out.append((unit, name, {k: int(v) for k, v in (pair.split("=") for pair in selector.split())}))
    return out


def test_every_policy_3_kernel_of_every_unit_is_in_the_census(engine_library, tmp_path):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not available")
    libdir = os.path.dirname(engine_library)
    exe = tmp_path / "tune3_census"
    subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-Wall", "-Werror",
                    "-I" + os.path.join(ROOT, "lettuce_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "aux", "tune3_census.cpp"), "-L" + libdir, "-llettuce_hip",
                    "-Wl,-rpath," + libdir, "-o", str(exe)], check=True, capture_output=True, timeout=600)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stderr)
    want_text = open(FIXTURE).read()
    want, got = _units(want_text), _units(out.stdout)
    assert len(want) == 10 and list(got) == list(want), (list(got), list(want))
    for unit in want:
        missing = [line for line in got[unit] if line not in want[unit]]
        gone = [line for line in want[unit] if line not in got[unit]]
        assert not missing and not gone, (f"{unit}: the library has kernels of cache policy 3 that tests/tune3_census.txt "
                                          f"(and so tests/test_gpu_tune3_vs_cpu.py) does not: {missing}; the fixture "
                                          f"has lines the library does not: {gone}")
    assert out.stdout == want_text


def test_the_census_names_every_collision_in_every_unit_that_has_it():
    """the fixture itself: every line is a TUNE = 3 one-step name whose fields are its selector's, no name twice, and
    each collision number of dispatch.hpp appears in exactly the units that have it -- fused and collide-only, with and
    without masks (host only: reads the text)"""
    seen = {}
    names = set()
    for unit, lines in _units(open(FIXTURE).read()).items():
        lattice, scalar = unit.split("_")
        assert re.fullmatch(r"  kernels of policy 3: (\d+); selectors with a kernel: \d+ of \d+, \d+ of them of policy 0",
                            lines[-1]), lines[-1]
        assert int(lines[-1].split(":")[1].split(";")[0]) == len(lines) - 1
        for line in lines[:-1]:
            m = LINE.match(line)
            assert m, line
            (kernel, t, lat, layout, coll, stream, collide, masked, abbd, s_layout, s_coll, s_mode, s_masked, s_pout, s_depth,
             s_slot) = m.groups()
            assert (t, lat) == ({"f32": "float", "f64": "double"}[scalar], lattice), line
            assert layout == s_layout and (masked == "true") == (s_masked == "1"), line
            assert (stream, collide) == {"0": ("true", "true"), "1": ("false", "true"), "2": ("true", "false")}[s_mode], line
            assert int(coll) == (0 if s_mode == "2" else int(s_coll)), line
            assert (abbd is not None and int(abbd) >= 4) == (s_pout == "1") and s_depth == "0" and s_slot == "0", line
            assert (kernel == "lbm_kernel_occ4") == (unit == "d3q27_f32" and coll == "2" and masked == "true" and abbd is None)
            assert line.split(" | ")[0] not in names, line
            names.add(line.split(" | ")[0])
            if s_mode != "2":
                seen.setdefault((int(coll), s_mode, s_masked), set()).add(unit)
    for coll, lattices in COLLISIONS.items():
        units = {f"{lat}_{t}" for lat in lattices for t in ("f32", "f64")}
        for mode in "01":
            for masked in "01":
                assert seen.get((coll, mode, masked)) == units, (coll, mode, masked, seen.get((coll, mode, masked)))
    assert set(c for c, _, _ in seen) == set(COLLISIONS)
