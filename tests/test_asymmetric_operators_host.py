"""The assumptions of tests/test_gpu_asymmetric_operators.py about the CPU paths, checked without a GPU: for every case
both runs (fp32 and fp64 from the same fp32 state) are finite and differ in every weight class, E_ref lies inside the
bounds of test_fp32_error_budget_host.py -- a case outside them would be dropped, not given a
wider gate -- and KBC leaves out at most 5 % of the nodes."""
import numpy as np
import pytest

import asymmetric_states as st
from conftest import golden
from test_gpu_asymmetric_operators import (GRID, OPERATOR_IDS, OPERATORS, SETTING_IDS, SETTINGS, cpu_pair, reference_error,
                                           steps_of)


@pytest.mark.parametrize("kind,tau,steps", SETTINGS, ids=SETTING_IDS)
@pytest.mark.parametrize("op", OPERATORS, ids=OPERATOR_IDS)
def test_the_cpu_path_is_a_yardstick_on_the_asymmetric_states(op, kind, tau, steps):
    steps = steps_of(op, kind, tau, "f32", steps)
    for n in steps:
        e_ref = reference_error(op, kind, tau, n, steps)
        print(f"n = {n}: E_ref {e_ref:.3e}")
        assert 1e-7 < e_ref < 1e-4, e_ref
    for dt in ("f32", "f64"):
        run = steps_of(op, kind, tau, dt, steps)
        pairs, drop, excluded = cpu_pair(op, kind, tau, dt, run)
        assert all(np.isfinite(a).all() and np.isfinite(b).all() for a, b in pairs.values())
        assert excluded <= st.EXCLUDED_CAP * int(np.prod(GRID[op[2]])), excluded
        if excluded:
            print(f"{dt}: {excluded} nodes within the margin of KBC's threshold, steps {run}")


BITS = [(lat, dt) for lat in ("D2Q9", "D3Q15", "D3Q19", "D3Q27") for dt in ("f64", "f32")]


@pytest.mark.parametrize("lat,dt", BITS, ids=[f"{a.lower()}-{b}" for a, b in BITS])
def test_the_state_generator_is_the_one_that_made_the_bgk_bit_fixtures(lat, dt):
    """asymmetric_state restates oracle/gen_golden.py's generator with the oracle's tables: the f0 the fixtures store,
    bit for bit (seeds and grids as bgk_bits_cases sets them)"""
    g = golden(f"bgk_bits_{lat.lower()}_{dt}")
    li = ("D1Q3", "D2Q9", "D3Q15", "D3Q19", "D3Q27").index(lat)
    res = [int(r) for r in g["resolution"]]
    for ki, kind in enumerate(("moderate", "wide")):
        f0 = st.asymmetric_state(lat, res, kind, 9100 + 10 * li + ki)
        f0 = f0.float() if dt == "f32" else f0
        assert f0.numpy().tobytes() == g[f"f0_{kind}"].tobytes()
