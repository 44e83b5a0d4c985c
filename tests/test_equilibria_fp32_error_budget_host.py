"""The assumptions of tests/test_gpu_equilibria_fp32_error_budget.py about the reference arithmetic, checked without a
GPU: for every case of that file both CPU runs (fp32 and fp64 from the same fp32 state) are finite and differ in every
weight class of the lattice, so E_ref > 0 is a yardstick and not a zero the gate would divide by."""
import pytest

from test_gpu_equilibria_fp32_error_budget import CASES, STEPS, TAUS, reference_error


@pytest.mark.parametrize("tau", TAUS)
@pytest.mark.parametrize("operator,lat", CASES)
def test_the_reference_has_an_fp32_error_in_every_weight_class(operator, lat, tau):
    for n in STEPS:
        e_ref = reference_error(operator, lat, tau, n)
        print(f"n = {n}: E_ref {e_ref:.3e}")
        # fp32 has 2^-24 = 6e-8 per rounding; a step is dozens of roundings on populations of the order of w_q
        assert 1e-7 < e_ref < 1e-4, e_ref
