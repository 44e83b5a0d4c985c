"""The EnergySpectrum observable on the HIP path against the reference's mask expression, IN ONE PROCESS ON THE SAME
STATE, alternating samples, five per side.
  "hip"   lt.EnergySpectrum(flow)() on a native context: lt_macroscopic, one torch.fft.fftn, lt_energy_spectrum
  "mask"  the reference's expression (observable_reporter.py:99-137) in torch on the same device: the same u and FFT,
          divided by the norm, ekin[..., None] * wavemask summed over the grid; the boolean mask [*res, K] is built
          once, as the reference's constructor does, and its bytes are reported with the peak
D3Q19 Taylor-Green vortex with 5 % noise, fp32, at 64^3 and 128^3 where the mask and its product (0.9 GB at 128^3)
fit; the HIP path alone at 256^3, where the mask would be 3.7 GB and the product 14.8 GB per call.  Also the
binning kernels alone (lt_energy_spectrum on a transformed field).  ms_per_call = one evaluation of the observable,
device events around CALLS evaluations; peak_mib = torch.cuda.max_memory_allocated over the side's samples less
what was allocated before them.  No pass/fail number: the claim is that the observable runs at the engine's grid sizes.
usage: spectrum_ab.py [--sizes 64,128] [--alone 256] [--out profiles/spectrum_ab.jsonl]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import lettuce_amd as lt
from lettuce_amd.ext._reporter import spectrum_bins

CALLS, SAMPLES = 10, 5


def option(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


SIZES = [int(n) for n in option("--sizes", "64,128").split(",") if n]
ALONE = [int(n) for n in option("--alone", "256").split(",") if n]
OUT = option("--out", os.path.join(ROOT, "profiles", "spectrum_ab.jsonl"))


def noisy_flow(n):
    ctx = lt.Context(device="cuda:0", dtype=torch.float32, use_native=True)
    flow = lt.TaylorGreenVortex(ctx, [n] * 3, 1600, 0.1, lt.D3Q19())
    g = torch.Generator(device="cuda").manual_seed(n)
    flow.f = flow.f * (1 + 0.05 * (2 * torch.rand(flow.f.shape, generator=g, device="cuda", dtype=torch.float32) - 1))
    return flow


class MaskSpectrum:
    """the reference's observable, restated: mask in the constructor, masked product per call"""

    def __init__(self, flow, norm):
        self.flow, self.norm = flow, norm
        dtype, device = flow.context.dtype, flow.context.device
        freq = [torch.fft.fftfreq(n, d=1 / n, dtype=dtype, device=device) for n in flow.resolution]
        wavenorms = torch.norm(torch.stack(torch.meshgrid(*freq, indexing="ij")), dim=0)
        k = torch.arange(int(torch.max(wavenorms)), dtype=dtype, device=device)
        self.wavemask = (wavenorms[..., None] > k - 0.5) & (wavenorms[..., None] <= k + 0.5)

    def __call__(self):
        flow = self.flow
        u = flow.units.convert_velocity_to_pu(flow.u())
        uh = torch.stack([torch.fft.fftn(u[i], dim=(0, 1, 2)) for i in range(3)]) / self.norm
        ekin = torch.sum(0.5 * (uh.imag ** 2 + uh.real ** 2), dim=0)
        ek = ekin[..., None] * self.wavemask.to(dtype=flow.context.dtype)
        return ek.sum([0, 1, 2])


def sample(call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    call()
    e0.record()
    for _ in range(CALLS):
        call()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) / CALLS, 4)


def measure(sides):
    """alternating samples; peak memory per side in a pass of its own"""
    times = {name: [] for name in sides}
    for _ in range(SAMPLES):
        for name, call in sides.items():
            times[name].append(sample(call))
    peaks = {}
    for name, call in sides.items():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        before = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        call()
        torch.cuda.synchronize()
        peaks[name] = round((torch.cuda.max_memory_allocated() - before) / 2 ** 20, 1)
    return times, peaks


def kernel_alone(flow, obs):
    plan = flow._engine_plan(flow.f)
    uh = torch.view_as_real(torch.fft.fftn(flow.units.convert_velocity_to_pu(flow.u()), dim=(1, 2, 3))).contiguous()
    K = len(obs.wavenumbers)
    return [sample(lambda: plan.energy_spectrum(uh, 1.0 / float(obs.norm) ** 2, K)) for _ in range(SAMPLES)]


def main():
    assert torch.cuda.is_available(), "spectrum_ab.py measures on the GPU"
    lines, mask = [], None
    for n in SIZES + ALONE:
        flow = noisy_flow(n)
        obs = lt.EnergySpectrum(flow)
        sides = {"hip": obs}
        record = {"what": "EnergySpectrum D3Q19 fp32, Taylor-Green vortex with 5 % noise", "resolution": [n] * 3,
                  "bins": len(obs.wavenumbers), "calls_per_sample": CALLS}
        if n in SIZES:
            mask = MaskSpectrum(flow, obs.norm)
            sides["mask"] = mask
            record["mask_mib"] = round(mask.wavemask.numel() / 2 ** 20, 1)
            a, b = obs().double(), mask().double()
            record["max_difference_of_peak"] = float((a - b).abs().max() / b.max())
        times, peaks = measure(sides)
        record.update(ms_per_call=times, median_ms={k: statistics.median(v) for k, v in times.items()}, peak_mib=peaks)
        kernel = kernel_alone(flow, obs)
        record.update(kernel_ms_per_call=kernel, kernel_median_ms=statistics.median(kernel))
        if "mask" in sides:
            record["mask_over_hip"] = round(record["median_ms"]["mask"] / record["median_ms"]["hip"], 2)
        lines.append(json.dumps(record))
        print(lines[-1], flush=True)
        del flow, obs, sides
        mask = None
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as out:
        out.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
