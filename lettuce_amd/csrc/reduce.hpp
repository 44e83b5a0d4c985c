// The fixed-order fp64 reduction of every observable: the one place that knows the summation order.  Device only.
//
//   thread     adds its own terms in the order its kernel documents (not here)
//   wave       wave_reduce: the six-step shuffle tree, v += v(lane + 32), (lane + 16), ... (lane + 1); lane 0 holds it
//   workgroup  block_reduce: the four waves in wave order, for C components at once
//   grid       finish_sum_kernel (a scalar) / finish_components_kernel (C components): one workgroup takes the
//              workgroups' partials in index order
// No atomics anywhere, so a result depends on the launch geometry alone: the same bits on every run.
#pragma once
#include <hip/hip_runtime.h>

namespace lt {

constexpr int kReduceThreads = 256;                  // the workgroup of every kernel that reduces: four waves
constexpr int kReduceWaves = kReduceThreads / 64;
constexpr int kFinishMaxBlocks = 1024;               // the most partials per component finish_components_kernel stages

// maximum that propagates NaN like torch.max: a NaN on either side wins and then stays (`m > acc` alone is false
// for a NaN m, which would drop it); without a NaN the larger value, as before
__device__ __forceinline__ double nan_max(double m, double acc) { return (m > acc || m != m) ? m : acc; }

// the wave tree (sum, or NaN-propagating maximum when MAX); the result is lane 0's
template <bool MAX = false>
__device__ __forceinline__ double wave_reduce(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double o = __shfl_down(v, off);
    v = MAX ? nan_max(o, v) : v + o;
  }
  return v;
}

// The workgroup step over C components: lane 0 of each wave leaves its tree's result in LDS, one barrier, thread c adds
// the waves of component c in ascending order.  Valid in thread c < C (0.0 in the others).  Every thread of the
// workgroup calls it.
// The sum starts from the first wave's value and not from 0.0.  Both give the same bits: no accumulator that arrives
// here can be -0.0 -- each starts at +0.0, and in round-to-nearest a sum is -0.0 only if both operands are -- so
// 0.0 + part[0] == part[0] bit for bit (a NaN comes out of either form as the same quiet NaN once the next wave is
// added).  The maximum keeps nan_max(part[w], s) from s = 0.0: the values are norms, >= 0 or NaN.
template <int C, bool MAX = false>
__device__ __forceinline__ double block_reduce(const double (&v)[C]) {
  static_assert(C >= 1 && C <= 64, "thread c of the first wave finishes component c");
  __shared__ double part[C][kReduceWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const double w = wave_reduce<MAX>(v[c]);
    if (lane == 0) part[c][wave] = w;
  }
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x < C) {
    if constexpr (MAX) {
#pragma unroll
      for (int w = 0; w < kReduceWaves; ++w) s = nan_max(part[threadIdx.x][w], s);
    } else {
      s = part[threadIdx.x][0];
#pragma unroll
      for (int w = 1; w < kReduceWaves; ++w) s += part[threadIdx.x][w];
    }
  }
  return s;
}
// ... of one value; valid in thread 0
template <bool MAX = false>
__device__ __forceinline__ double block_sum(double v) {
  const double one[1] = {v};
  return block_reduce<1, MAX>(one);
}

// The scalar finish, one workgroup: thread t takes the partials t, t + 256, ... in that order, then the workgroup step
template <bool MAX>
static __global__ void __launch_bounds__(kReduceThreads) finish_sum_kernel(const double *__restrict__ partial,
                                                                    int n, double *__restrict__ out) {
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += kReduceThreads) acc = MAX ? nan_max(partial[i], acc) : acc + partial[i];
  const double s = block_sum<MAX>(acc);
  if (threadIdx.x == 0) *out = s;
}

// The finish of C = 3 components with partials laid out [3][blocks], one workgroup: out[c] = partial[c][0] +
// partial[c][1] + ... in index order from 0.0, c < D; out[c] = 0 for the components beyond D.  All threads copy the
// D * blocks partials into LDS (coalesced), then one thread per component adds them one after the other.  Writes all
// three outputs whatever the first launch found; blocks = 0 reads nothing and writes zeros.
// (A template on the unit's scalar type only so that the objects that do not launch it do not hold it.)
template <typename T, int D>
__global__ void __launch_bounds__(kReduceThreads) finish_components_kernel(const double *__restrict__ partial,
                                                                           int blocks, double *__restrict__ out) {
#pragma clang fp contract(off)
  __shared__ double staged[3 * kFinishMaxBlocks];
  if (blocks > kFinishMaxBlocks) blocks = kFinishMaxBlocks;
  for (int n = threadIdx.x; n < D * blocks; n += kReduceThreads) staged[n] = partial[n];
  __syncthreads();
  if (threadIdx.x < 3) {
    double s = 0.0;
    if (threadIdx.x < D) {
      const double *mine = staged + threadIdx.x * blocks;
      for (int b = 0; b < blocks; ++b) s += mine[b];
    }
    out[threadIdx.x] = s;
  }
}

}  // namespace lt
