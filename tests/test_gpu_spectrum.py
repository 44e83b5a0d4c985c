"""The energy spectrum on the HIP path: ``lt_energy_spectrum`` alone against an exact host sum, the ``EnergySpectrum``
observable on a native context against the reference's fixtures (tests/golden/spectrum_*.npz), and the decaying
turbulence flow end to end under an ``ObservableReporter``.

Kernel alone.  Reference: the exact sum of the squares of the same inputs per bin -- every square split into a product
and its rounding error (Dekker; an fp32 input's square is exact in fp64), summed with ``math.fsum`` and its remainder,
scaled in rational arithmetic.  Bound per bin: relative error <= (modes in the bin + 4) * 2^-53 -- every mode's energy
is formed with at most 4 roundings (a square, re^2 + im^2, two sums over the components; the halving is exact), a sum of
N non-negative terms adds at most N - 1 in any order (the kernel's other additions are of an exact 0), the scale one.

Observable.  The two gates of test_spectrum_host.py: fp64 2e-14 per bin; fp32 on the states after 10 steps
E <= FACTOR * E_ref.  Measured on an MI355X: see DESIGN.md section 2."""
import ctypes
import functools
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

import lettuce_amd as lt
from lettuce_amd.ext._reporter import spectrum_bins
from test_spectrum_host import (FIXTURES, IDS, FP64, TGV, DECAY, fixture, fixture_flow, gate_fp32, gate_fp64, per_bin)

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
SCALE = 1.0 / 37.5 ** 2
# the fixture shapes; K = 90 > 64 lanes; a ragged last wave; more modes than 1024 workgroups x 256; the other 3-D units
KERNEL_CASES = ([("D2Q9" if len(r) == 2 else "D3Q19", r) for r in TGV + [r for r in DECAY if r not in TGV]]
                + [("D2Q9", [128, 128]), ("D3Q19", [64, 64, 72]), ("D3Q15", [5, 6, 7]), ("D3Q27", [8, 12, 10])])
KERNEL_IDS = [f"{lat.lower()}-{'x'.join(map(str, res))}" for lat, res in KERNEL_CASES]


def native(dt):
    return lt.Context(device="cuda:0", dtype={"f32": torch.float32, "f64": torch.float64}[dt], use_native=True)


def plan_of(lat, res, dt, **kwargs):
    from lettuce_amd import _native
    return _native.Plan(lat, {"f32": torch.float32, "f64": torch.float64}[dt], "none", res, **kwargs)


@functools.lru_cache(maxsize=None)
def transformed_field(res, dt):
    """a seeded random complex field [d, *res, 2] in the working dtype (amplitudes over four decades, so that the bins
    differ), on the host.  Shared; never written to."""
    g = torch.Generator().manual_seed(4711 + sum(res) + len(res))
    x = torch.randn([len(res), *res, 2], generator=g, dtype=torch.float64)
    x = x * 10 ** (4 * torch.rand([len(res), *res, 1], generator=g, dtype=torch.float64) - 2)
    return x.to({"f32": torch.float32, "f64": torch.float64}[dt])


@functools.lru_cache(maxsize=None)
def exact_spectrum(res, dt, n_bins):
    """per bin: (the exact sum of 0.5 * SCALE * x^2 over the bin's inputs as a Fraction to 2^-106, modes in the bin)"""
    x = transformed_field(res, dt).double().numpy()
    d = len(res)
    x = np.moveaxis(x, 0, -2).reshape(-1, 2 * d)                 # [modes, 2 d]
    p = x * x
    hi = x * 134217729.0
    hi = hi - (hi - x)
    lo = x - hi
    err = ((hi * hi - p) + 2.0 * hi * lo) + lo * lo               # p + err == x^2 exactly
    bins = spectrum_bins(list(res))[0].numpy().reshape(-1)
    order = np.argsort(bins, kind="stable")
    counts = np.bincount(bins, minlength=n_bins)
    out, start = [], 0
    for n in range(n_bins):
        rows = order[start:start + counts[n]]
        start += counts[n]
        terms = np.concatenate([p[rows].ravel(), err[rows].ravel()]).tolist()
        s = math.fsum(terms)
        r = math.fsum(terms + [-s])
        out.append(((Fraction(s) + Fraction(r)) * Fraction(SCALE) / 2, int(counts[n])))
    return out


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("lat,res", KERNEL_CASES, ids=KERNEL_IDS)
def test_kernel_against_the_exact_sum(lat, res, dt):
    n_bins = spectrum_bins(res)[1]
    plan = plan_of(lat, res, dt)
    got = plan.energy_spectrum(transformed_field(tuple(res), dt).cuda(), SCALE, n_bins)
    assert got.dtype == torch.float64 and list(got.shape) == [n_bins]
    got = got.cpu().numpy()
    worst = 0.0
    for n, (want, modes) in enumerate(exact_spectrum(tuple(res), dt, n_bins)):
        assert want > 0 and modes > 0
        rel = float(abs(Fraction(float(got[n])) - want) / want)
        worst = max(worst, rel / ((modes + 4) * U))
        assert rel <= (modes + 4) * U, (n, modes, rel)
    print(f"{lat} {res} {dt}: K = {n_bins}, worst error {worst:.3f} of the bound (modes + 4) * 2^-53")


def test_fewer_bins_drop_the_modes_beyond_them():
    res, dt = (16, 16), "f64"
    K = spectrum_bins(list(res))[1]
    plan, x = plan_of("D2Q9", list(res), dt), transformed_field(res, dt).cuda()
    assert torch.equal(plan.energy_spectrum(x, SCALE, K - 3), plan.energy_spectrum(x, SCALE, K)[:K - 3])
    complex_input = torch.view_as_complex(x)
    assert torch.equal(plan.energy_spectrum(complex_input, SCALE, K), plan.energy_spectrum(x, SCALE, K))


@pytest.mark.parametrize("lat,res,dt", [("D3Q19", (64, 64, 72), "f32"), ("D2Q9", (128, 128), "f64")])
def test_two_calls_give_the_same_bits(lat, res, dt):
    plan, x = plan_of(lat, list(res), dt), transformed_field(res, dt).cuda()
    K = spectrum_bins(list(res))[1]
    first = plan.energy_spectrum(x, SCALE, K)
    second = plan.energy_spectrum(x, SCALE, K)
    assert torch.equal(first, second) and bool((first > 0).all())


def test_refusals():
    from lettuce_amd import _native
    x3 = torch.zeros([3, 8, 8, 8, 2], dtype=torch.float32, device="cuda")
    slab = plan_of("D3Q19", [8, 8, 6], "f32", layout=_native.LAYOUT_SLAB, ghost_planes=1)
    with pytest.raises(_native.NativeEngineError, match="energy spectrum: 2-D / 3-D grids in the reference layout") as e:
        slab.energy_spectrum(x3, 1.0, 4)
    assert e.value.code == 2                                       # LT_ERR_UNSUPPORTED
    line = plan_of("D1Q3", [16], "f32")
    with pytest.raises(_native.NativeEngineError, match="energy spectrum: 2-D / 3-D grids") as e:
        line.energy_spectrum(torch.zeros([1, 16, 2], dtype=torch.float32, device="cuda"), 1.0, 4)
    assert e.value.code == 2
    plan = plan_of("D3Q19", [8, 8, 8], "f32")
    with pytest.raises(_native.NativeEngineError, match="LT_SPECTRUM_MAX_BINS = 2048") as e:
        plan.energy_spectrum(x3, 1.0, _native.SPECTRUM_MAX_BINS + 1)
    assert e.value.code == 2
    with pytest.raises(_native.NativeEngineError, match="energy spectrum: 0 bins") as e:
        plan.energy_spectrum(x3, 1.0, 0)
    assert e.value.code == 1                                       # LT_ERR_INVALID
    with pytest.raises(_native.NativeEngineError, match="tensor dtype"):
        plan.energy_spectrum(x3.double(), 1.0, 4)
    scratch = torch.zeros([_native.SPECTRUM_BLOCKS, 4], dtype=torch.float64, device="cuda")
    out = torch.zeros([4], dtype=torch.float64, device="cuda")
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())                  # noqa: E731
    for args in ((None, ptr(scratch), ptr(out)), (ptr(x3), None, ptr(out)), (ptr(x3), ptr(scratch), None)):
        assert plan.lib.lt_energy_spectrum(plan._handle, args[0], 1.0, 4, args[1], args[2], None) == 1
        assert b"null transformed field / scratch / output" in plan.lib.lt_last_error()
    assert plan.lib.lt_energy_spectrum(None, ptr(x3), 1.0, 4, ptr(scratch), ptr(out), None) == 1
    assert plan.energy_spectrum(x3, 1.0, 4).tolist() == [0.0] * 4   # and the plan still works


# ------------------------------------------------------------------------- the observable on a native context
@pytest.mark.parametrize("kind,res", FIXTURES, ids=IDS)
def test_observable_fp64_against_the_reference(kind, res):
    g = fixture(kind, res)
    flow = fixture_flow(g, kind, native("f64"))
    assert flow._engine_plan(flow.f) is not None
    gate_fp64(flow, g, f"HIP {kind} {res}")


@pytest.mark.parametrize("kind,res", FIXTURES, ids=IDS)
def test_observable_fp32_within_the_reference_error_budget(kind, res):
    g = fixture(kind, res)
    flow = fixture_flow(g, kind, native("f32"))
    assert flow._engine_plan(flow.f) is not None
    gate_fp32(flow, g, f"HIP {kind} {res}")


# ------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("res", [[16, 16], [12, 12, 12]], ids=["d2q9-16x16", "d3q19-12x12x12"])
def test_decaying_turbulence_with_a_spectrum_reporter(res, dt):
    """10 BGK steps on the native path with a reporter every 5: three rows of K finite values.  fp64: the first row
    against the reference's spectrum of its own initial state at 2e-14 per bin (bin 0 holds the zeroed mean mode, i.e.
    rounding noise: bins below 6e-7 of the peak, the floor of the noisy fixtures, are held to 2e-14 of the peak).
    fp32: finite, and the total energy of the first row within 5 % of the reference's."""
    g = fixture("decay", res)
    flow = fixture_flow(g, "decay", native(dt))
    want = g["spec_init_f64"]
    K = len(want)
    reporter = lt.ObservableReporter(lt.EnergySpectrum(flow), interval=5, out=None)
    sim = lt.Simulation(flow, lt.BGKCollision(float(g["tau"])), [reporter])
    assert sim._native is not None, "HIP engine not in use"
    sim(10)
    rows = np.array(reporter.out)
    assert rows.shape == (3, 2 + K) and rows[:, 0].tolist() == [0, 5, 10] and np.isfinite(rows).all()
    first = rows[0, 2:]
    total, total_ref = float(first.sum()), float(want.sum())
    print(f"decay {res} {dt}: total energy {total:.9f}, the reference's {total_ref:.9f}; rows 5 and 10: "
          f"{rows[1, 2:].sum():.9f}, {rows[2, 2:].sum():.9f}")
    assert abs(total - total_ref) <= 0.05 * total_ref
    assert (rows[:, 2:] >= 0).all()
    if dt == "f64":
        strong = want >= 6e-7 * want.max()
        err = per_bin(first[strong], want[strong])
        print(f"decay {res} f64: first row, per-bin relative error {err:.3e} (bound {FP64:.0e})")
        assert err <= FP64
        assert np.abs(first - want)[~strong].max(initial=0.0) <= FP64 * want.max()
