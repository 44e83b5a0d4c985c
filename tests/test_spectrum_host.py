"""The energy spectrum and the decaying-turbulence flow on the host (CPU, no GPU needed): the integer bin rule against
the reference's mask formula, the mirror's torch path and ``DecayingTurbulence`` against vectors produced by the
reference's own CPU path (tests/golden/spectrum_*.npz, made by tools/gen_golden_spectrum.py), and the plumbing of
``lt_energy_spectrum``.

Bounds.  fp64: per-bin relative error <= 2e-14, the project's fp64 bound (two independent CPU fp64 evaluations of these
fixtures differ by 3.4e-15 at most).  fp32, on the states after 10 steps only: with E(s) = max_n |s_n - ref64_n| / max_n
ref64_n, E(mirror) <= FACTOR * E(reference's own fp32 spectrum), FACTOR = 4 as in test_gpu_fp32_error_budget.py; the
step-0 state is fp32-exact and its E_ref (2e-8 ... 2e-7) is too small to carry a budget."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import lettuce_amd as lt
from lettuce_amd.ext._reporter import spectrum_bins
from conftest import golden, ROOT
from test_host_api import ctx
from test_gpu_fp32_error_budget import FACTOR

FP64 = 2e-14
TGV = [[16, 16], [6, 8], [7, 9], [33, 32], [8, 12, 10], [5, 6, 7], [16, 16, 16]]
DECAY = [[16, 16], [9, 9], [12, 12, 12]]
FIXTURES = ([("tgv", r) for r in TGV] + [("decay", r) for r in DECAY])
IDS = [f"{kind}-{'x'.join(map(str, res))}" for kind, res in FIXTURES]
SHAPES = TGV + [[9, 9], [12, 12, 12], [64, 64, 64], [96, 96, 96]]


def fixture(kind, res):
    """the case's arrays; the fp64 10-step state of the largest case lives in a file of its own"""
    name = f"spectrum_{kind}_" + "x".join(str(n) for n in res)
    g = golden(name)
    if "f10_f64" not in g:
        g.update(golden(name + "_f64state"))
    return g


def fixture_flow(g, kind, context):
    res, stencil = [int(n) for n in g["resolution"]], getattr(lt, str(g["stencil"]))()
    if kind == "tgv":
        return lt.TaylorGreenVortex(context, res, float(g["reynolds"]), float(g["mach"]), stencil)
    return lt.DecayingTurbulence(context, res, float(g["reynolds"]), float(g["mach"]), k0=float(g["k0"]),
                                 ic_energy=float(g["ic_energy"]), stencil=stencil, initialize_pressure=False,
                                 randseed=int(g["randseed"]))


def spectrum_of(flow, state):
    flow.f = flow.context.convert_to_tensor(torch.as_tensor(state).to(flow.context.dtype))
    return lt.EnergySpectrum(flow)().detach().cpu().double().numpy()


def per_bin(got, want):
    return float(np.max(np.abs(got - want) / np.abs(want)))


def of_peak(got, ref64):
    return float(np.max(np.abs(np.asarray(got, dtype=np.float64) - ref64)) / np.max(ref64))


def gate_fp64(flow, g, what):
    for state, want in (("f0", "spec0_f64"), ("f10_f64", "spec10_f64")):
        got = spectrum_of(flow, g[state])
        assert got.shape == g[want].shape
        err = per_bin(got, g[want])
        print(f"{what} fp64 {state}: per-bin relative error {err:.3e} (bound {FP64:.0e})")
        assert err <= FP64


def gate_fp32(flow, g, what):
    ref64 = g["spec10_f64"]
    e_ref = of_peak(g["spec10_f32"], ref64)
    assert e_ref > 0
    got = spectrum_of(flow, g["f10_f32"])
    assert got.shape == ref64.shape
    e = of_peak(got, ref64)
    print(f"{what} fp32 after 10 steps: E_ref {e_ref:.3e}, E {e:.3e}, ratio {e / e_ref:.3f} (bound {FACTOR})")
    assert e <= FACTOR * e_ref
    return e / e_ref


# ---------------------------------------------------------------------------------------- the bin rule
def reference_bins(shape, dtype):
    """(bin of every mode, K) by the reference's mask formula (observable_reporter.py:78-97), norms in `dtype`; K for
    the modes no mask holds.  Asserts that no mode is in two masks."""
    freq = [np.fft.fftfreq(n, d=1 / n).astype(dtype) for n in shape]
    wavenumbers = np.stack(np.meshgrid(*freq, indexing="ij"))
    wavenorms = np.sqrt((wavenumbers * wavenumbers).sum(axis=0, dtype=dtype)).astype(dtype)
    K = int(wavenorms.max())
    out = np.full(shape, K, dtype=np.int64)
    hits = np.zeros(shape, dtype=np.int64)
    for n in np.arange(K).astype(dtype):
        mask = (wavenorms > n - dtype(0.5)) & (wavenorms <= n + dtype(0.5))
        out[mask] = int(n)
        hits += mask
    assert hits.max() <= 1
    return out, K


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_integer_bins_equal_the_reference_mask(shape, dtype):
    """bin for bin, the dropped modes included: zero mismatches"""
    want, K = reference_bins(shape, dtype)
    bins, n_bins = spectrum_bins(shape)
    assert n_bins == K
    got = np.minimum(bins.numpy(), K)
    assert got.shape == want.shape
    mismatches = int((got != want).sum())
    print(f"{shape} {np.dtype(dtype).name}: K = {K}, {int((want == K).sum())} dropped modes, {mismatches} mismatches")
    assert mismatches == 0


def test_observable_interface():
    flow = lt.TaylorGreenVortex(ctx("f64"), [6, 8], 100, 0.05, lt.D2Q9())
    obs = lt.EnergySpectrum(flow)
    assert "_wavemask" in vars(obs) and obs._wavemask is None            # nothing materialised ...
    want, K = reference_bins([6, 8], np.float64)
    assert obs.wavenumbers.tolist() == list(range(K)) and obs.dimensions == [6, 8]
    assert obs.dx == flow.units.convert_length_to_pu(1.0) and obs.norm == 6 / obs.dx
    mask = obs.wavemask                                                   # ... until somebody asks
    assert mask.dtype == torch.bool and list(mask.shape) == [6, 8, K]
    assert np.array_equal(mask.numpy(), want[..., None] == np.arange(K))
    flow3 = lt.TaylorGreenVortex(ctx("f64"), [5, 6, 7], 100, 0.05, lt.D3Q19())
    obs3 = lt.EnergySpectrum(flow3)
    assert obs3.norm == 5 * np.sqrt(2 * np.pi) / obs3.dx ** 2
    assert torch.equal(obs3.spectrum_from_u(flow3.u()), obs3())
    assert not getattr(obs3, "slab_aware", False)
    with pytest.raises(lt.LettuceException, match="EnergySpectrum: 2-D and 3-D"):
        lt.EnergySpectrum(_OneD(ctx("f64"), [8], 100, 0.05, lt.D1Q3()))


class _OneD(lt.ExtFlow):
    """a 1-D flow at rest, for the refusal"""

    def make_resolution(self, resolution, stencil=None):
        return resolution

    def make_units(self, reynolds_number, mach_number, resolution):
        return lt.UnitConversion(reynolds_number, mach_number, characteristic_length_lu=resolution[0])

    def initial_pu(self):
        zeros = self.context.zero_tensor(self.resolution)
        return zeros[None, ...], zeros[None, ...]

    @property
    def boundaries(self):
        return []


# ------------------------------------------------------------------- the torch path against the fixtures
@pytest.mark.parametrize("kind,res", FIXTURES, ids=IDS)
def test_torch_path_fp64_against_the_reference(kind, res):
    g = fixture(kind, res)
    gate_fp64(fixture_flow(g, kind, ctx("f64")), g, f"{kind} {res}")


@pytest.mark.parametrize("kind,res", FIXTURES, ids=IDS)
def test_torch_path_fp32_within_the_reference_error_budget(kind, res):
    g = fixture(kind, res)
    gate_fp32(fixture_flow(g, kind, ctx("f32")), g, f"{kind} {res}")


def test_observable_reporter_takes_the_spectrum():
    flow = lt.TaylorGreenVortex(ctx("f64"), [16, 16], 100, 0.05, lt.D2Q9())
    reporter = lt.ObservableReporter(lt.EnergySpectrum(flow), interval=2, out=None)
    lt.Simulation(flow, lt.BGKCollision(0.6), [reporter])(4)
    assert [len(row) for row in reporter.out] == [2 + 11] * 3 and np.isfinite(reporter.out).all()


def test_slab_simulation_refuses_the_spectrum_by_name():
    slab = lt.ZSlab([8, 8, 8], 0, 1)
    flow = lt.TaylorGreenVortex(ctx("f32"), slab.extended_resolution, 100, 0.05, lt.D3Q19(), slab=slab)
    reporter = lt.ObservableReporter(lt.EnergySpectrum(flow), interval=1, out=None)
    with pytest.raises(lt.LettuceException, match="reporter ObservableReporter reads flow.f"):
        lt.SlabSimulation(flow, lt.BGKCollision(0.8), slab, reporter=[reporter])


# -------------------------------------------------------------------------------- DecayingTurbulence
@pytest.mark.parametrize("res", DECAY, ids=["x".join(map(str, r)) for r in DECAY])
def test_decaying_turbulence_equals_the_reference(res):
    g = fixture("decay", res)
    flow = fixture_flow(g, "decay", ctx("f64"))
    p, u = flow.initial_pu()
    assert u.dtype == np.float64 and np.array_equal(u, g["u_init"])                 # bit for bit
    assert p.shape == (1, *res) and not p.any()
    spectrum, wavenumbers = flow.energy_spectrum
    assert np.array_equal(wavenumbers, g["wavenumbers"])
    assert spectrum.shape == g["spectrum"].shape
    nonzero = g["spectrum"] != 0                      # bin 0 holds the mean mode alone, whose energy is exactly 0
    rel = per_bin(spectrum[nonzero], g["spectrum"][nonzero])
    print(f"decay {res}: spectrum per-bin relative error {rel:.3e} (bound {FP64:.0e})")
    assert rel <= FP64 and np.array_equal(spectrum[~nonzero], g["spectrum"][~nonzero])
    assert float(flow.units.characteristic_velocity_pu) == float(g["char_velocity_pu"])
    assert flow.units.characteristic_length_pu == 2 * np.pi and flow.units.characteristic_length_lu == res[0]
    x = flow.grid
    assert len(x) == len(res) and float(x[0].max()) == pytest.approx(2 * np.pi * (1 - 1 / res[0]))
    # the spectrum of the flow's own initial state against the reference's observable on its own.  The mean mode is
    # zeroed, so bin 0 holds rounding noise only: bins below 6e-7 of the peak (the floor of the noisy fixtures) are held
    # to 2e-14 of the peak instead of 2e-14 of themselves
    got = lt.EnergySpectrum(flow)().numpy()
    want = g["spec_init_f64"]
    strong = want >= 6e-7 * want.max()
    print(f"decay {res}: initial state, per-bin relative error {per_bin(got[strong], want[strong]):.3e}")
    assert per_bin(got[strong], want[strong]) <= FP64
    assert np.abs(got - want)[~strong].max(initial=0.0) <= FP64 * want.max()


def test_decaying_turbulence_refusals_and_registration():
    with pytest.raises(lt.LettuceException, match="DecayingTurbulence: the first two extents must be equal"):
        lt.DecayingTurbulence(ctx("f64"), [8, 10], 100, 0.05, k0=2, stencil=lt.D2Q9(), initialize_pressure=False)
    with pytest.raises(lt.LettuceException, match="DecayingTurbulence: the first two extents must be equal"):
        lt.DecayingTurbulence(ctx("f64"), [6, 8, 8], 100, 0.05, k0=2, stencil=lt.D3Q19())
    flow = lt.DecayingTurbulence(ctx("f64"), [8, 8, 6], 100, 0.05, k0=2, stencil=lt.D3Q19(), randseed=1)
    assert list(flow.f.shape) == [19, 8, 8, 6] and bool(torch.isfinite(flow.f).all())
    assert all(entry[0] is not lt.DecayingTurbulence for entry in lt.flow_by_name.values())
    assert lt.DecayingTurbulence is lt.ext.DecayingTurbulence


# ------------------------------------------------------------------------------------------- plumbing
def test_binding_header_and_library(engine_library):
    from lettuce_amd import _native
    assert _native.SYMBOLS["lt_energy_spectrum"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double,
                                                                    ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
                                                                    ctypes.c_void_p])
    assert hasattr(_native.Plan, "energy_spectrum")
    header = open(os.path.join(ROOT, "include", "lettuce_hip.h")).read()
    assert re.search(r"int\s+lt_energy_spectrum\s*\(\s*lt_plan\s*\*\s*plan\s*,\s*const\s+void\s*\*\s*uhat_dev\s*,\s*double\s+scale\s*,"
                     r"\s*int32_t\s+n_bins\s*,\s*double\s*\*\s*partial_scratch_dev\s*,\s*double\s*\*\s*out_dev\s*,"
                     r"\s*void\s*\*\s*stream\s*\)\s*;", header)
    assert re.search(r"#define\s+LT_ABI_VERSION\s+2\b", header)
    assert re.search(rf"#define\s+LT_SPECTRUM_BLOCKS\s+{_native.SPECTRUM_BLOCKS}\b", header)
    assert re.search(rf"#define\s+LT_SPECTRUM_MAX_BINS\s+{_native.SPECTRUM_MAX_BINS}\b", header)
    lib = ctypes.CDLL(engine_library)
    lib.lt_abi_version.restype = ctypes.c_int
    assert lib.lt_abi_version() == 2
    lib.lt_energy_spectrum.restype = ctypes.c_int
    lib.lt_energy_spectrum.argtypes = _native.SYMBOLS["lt_energy_spectrum"][1]
    assert lib.lt_energy_spectrum(None, None, 1.0, 4, None, None, None) == 1      # LT_ERR_INVALID, nothing dereferenced
    lib.lt_last_error.restype = ctypes.c_char_p
    assert b"null plan" in lib.lt_last_error()
