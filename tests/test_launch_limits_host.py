"""csrc/launch_limits.hpp is the one statement of what a two-step or many-step launch needs from a lattice, a scalar
type and a grid: api.hip admits plans by it and the launchers of unit.inc refuse by it.  tests/aux/launch_limits.cpp
includes that header alone and holds it against numbers written out: every unit's tile without and with masks, the LDS
footprints behind them (150 480 B for the unmasked D3Q19 fp32 sweep, 163 832 of 163 840 B with masks), the 2-D strips,
the many-step limits and the 32-bit addressing predicates at their edges.  Host code only."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lettuce_amd", "csrc")


def test_launch_limits_against_the_numbers_written_out(tmp_path):
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")
    assert hipcc is not None, "the engine is built with hipcc"
    exe = tmp_path / "launch_limits"
    subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-Wall", "-Werror",
                    "-I" + CSRC, "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "aux", "launch_limits.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, timeout=600)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    print(out.stdout)
    assert out.returncode == 0, out.stdout
    assert "wrong" not in out.stdout and out.stdout.splitlines()[-1] == "0 mismatches"
    assert len(out.stdout.splitlines()) > 100          # the program ran its checks


def test_the_limits_are_stated_once():
    """The arithmetic lives in launch_limits.hpp: api.hip and unit.inc name it and restate none of it."""
    text = {name: open(os.path.join(CSRC, name)).read() for name in ("api.hip", "unit.inc", "launch_limits.hpp")}
    for name in ("api.hip", "unit.inc"):
        for literal in ("160 * 1024", "1ll << 32", "q == 15 ? 5 : 9"):
            assert literal not in text[name], (name, literal)
        assert '#include "launch_limits.hpp"' in text[name], name
    for constant in ("kManyMax", "kManyTile"):
        defined = [name for name in os.listdir(CSRC) if name.endswith((".hip", ".hpp", ".inc"))
                   for _ in re.findall(r"\b%s\s*=" % constant, open(os.path.join(CSRC, name)).read())]
        assert defined == ["launch_limits.hpp"], (constant, defined)
    # host / constexpr code only
    for word in ("__global__", "__device__", "asm"):
        assert word not in text["launch_limits.hpp"], word
