// Energy spectrum (observable_reporter.py:71-108) without the reference's [*res, K] wave mask: one binning reduction
// over the Fourier modes of the velocity field.  Instantiated by the units' part spectrum only (unit.inc).
#pragma once
#include <hip/hip_runtime.h>

namespace lt {

constexpr int kSpectrumThreads = 256;                 // four waves per workgroup
constexpr int kSpectrumWaves = kSpectrumThreads / 64;
// == LT_SPECTRUM_MAX_BINS: a table of bins per wave, in doubles, within the 64 KiB of LDS a launch gets without asking
constexpr int kSpectrumMaxBins = 64 * 1024 / (kSpectrumWaves * (int)sizeof(double));

// integer wavenumber of index i on an axis of extent n: np.fft.fftfreq(n, d = 1 / n), odd n too
__device__ __forceinline__ long long wavenumber(int i, int n) { return i < (n + 1) / 2 ? i : i - n; }

// Bin of a mode with m = |k|^2: 0 for m = 0, else the n >= 1 with n^2 - n < m <= n^2 + n -- the reference's
// n - 0.5 < |k| <= n + 0.5, squared (an integer m never ties with n^2 + n + 1/4).  The floating-point root is a
// first guess only; the two integer comparisons decide.
__device__ __forceinline__ long long spectrum_bin(long long m) {
  if (m == 0) return 0;
  long long n = (long long)sqrt((double)m);
  while (n * n + n < m) ++n;
  while (n * n - n >= m) --n;
  return n;
}

// First launch.  uhat: D complex fields [D][n2][n1][n0], interleaved (re, im).  Workgroup b owns the modes
// [b * chunk, (b + 1) * chunk) (chunk: a multiple of the workgroup's 256, at least 1024), each wave 64 consecutive modes
// per pass.  Along the fastest axis neighbouring modes mostly share a bin, so a pass is reduced in runs: a lane whose
// left neighbour has another bin heads a run, a segmented suffix sum (a fixed shuffle tree of six steps, for all runs
// at once) leaves each run's sum in its head, and the heads are then added to the wave's own table in LDS one after
// the other in lane order -- by lane 0 alone, from values read out of the heads' lanes, so that the table has one
// writer and needs no atomics.  Then the four tables are added in wave order into partial [gridDim.x][n_bins].  Modes
// whose bin is >= n_bins are dropped.  Squares and sums in fp64.
template <typename T, int D>
__global__ void __launch_bounds__(kSpectrumThreads) energy_spectrum_kernel(const T *__restrict__ uhat, int n0, int n1,
                                                                         int n2, long long chunk, int n_bins,
                                                                         double *__restrict__ partial) {
#pragma clang fp contract(off)
  extern __shared__ double spectrum_bins[];      // [kSpectrumWaves][n_bins]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int n = threadIdx.x; n < kSpectrumWaves * n_bins; n += kSpectrumThreads) spectrum_bins[n] = 0.0;
  __syncthreads();
  double *mine = spectrum_bins + wave * n_bins;
  const long long M = (long long)n0 * n1 * n2;
  const long long begin = (long long)blockIdx.x * chunk, end = begin + chunk < M ? begin + chunk : M;
  // the bounds are the wave's, so that every lane stays in the loop for the shuffles
  for (long long base = begin + wave * 64; base < end; base += kSpectrumThreads) {
    const long long i = base + lane;
    int bin = -1;
    double e = 0.0;
    if (i < end) {
      const int c0 = (int)(i % n0), c1 = (int)((i / n0) % n1), c2 = (int)(i / ((long long)n0 * n1));
      const long long k0 = wavenumber(c0, n0), k1 = wavenumber(c1, n1), k2 = wavenumber(c2, n2);
      const long long b = spectrum_bin(k0 * k0 + k1 * k1 + k2 * k2);
      if (b < n_bins) {
        bin = (int)b;
#pragma unroll
        for (int a = 0; a < D; ++a) {
          const double re = (double)uhat[2 * (a * M + i)], im = (double)uhat[2 * (a * M + i) + 1];
          const double t = 0.5 * (re * re + im * im);
          e = a == 0 ? t : e + t;
        }
      }
    }
    const int left = __shfl_up(bin, 1);
    const bool head = lane == 0 || left != bin;
    const unsigned long long heads = __ballot(head);
    const int run = __popcll(heads & ((2ull << lane) - 1ull));      // runs are contiguous: the number of heads up to here
    double v = e;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const double o = __shfl_down(v, off);
      const int other = __shfl_down(run, off);
      if (lane + off < 64 && other == run) v += o;
    }
    unsigned long long todo = __ballot(head && bin >= 0);
    while (todo) {
      const int h = __ffsll((long long)todo) - 1;
      const int b = __shfl(bin, h);
      const double sum = __shfl(v, h);
      if (lane == 0) mine[b] += sum;
      todo &= todo - 1;
    }
  }
  __syncthreads();
  for (int n = threadIdx.x; n < n_bins; n += kSpectrumThreads) {
    double s = spectrum_bins[n];
#pragma unroll
    for (int w = 1; w < kSpectrumWaves; ++w) s += spectrum_bins[w * n_bins + n];
    partial[(long long)blockIdx.x * n_bins + n] = s;
  }
}

// Second launch: out[n] = scale * (partial[0][n] + partial[1][n] + ...), the workgroups in index order -- one thread per
// bin; the loads of 16 workgroups are issued together (they do not depend on the sum), the additions stay in index order.
// (A template on the unit's scalar type only so that the objects that do not launch it do not hold it.)
template <typename T>
__global__ void __launch_bounds__(kSpectrumThreads) finish_spectrum_kernel(const double *__restrict__ partial,
                                                                          int blocks, int n_bins, double scale,
                                                                          double *__restrict__ out) {
#pragma clang fp contract(off)
  const int n = blockIdx.x * kSpectrumThreads + threadIdx.x;
  if (n >= n_bins) return;
  constexpr int kBatch = 16;
  double s = 0.0;
  int b = 0;
  for (; b + kBatch <= blocks; b += kBatch) {
    double v[kBatch];
#pragma unroll
    for (int j = 0; j < kBatch; ++j) v[j] = partial[(long long)(b + j) * n_bins + n];
#pragma unroll
    for (int j = 0; j < kBatch; ++j) s += v[j];
  }
  for (; b < blocks; ++b) s += partial[(long long)b * n_bins + n];
  out[n] = scale * s;
}

}  // namespace lt
