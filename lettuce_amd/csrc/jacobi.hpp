// Jacobi solver of the periodic pressure-Poisson equation (lettuce/util/utility.py:119-156, torch_jacobi): one fused
// sweep (the next iterate and the residuum of the input iterate from one neighbour sum), the residuum's mean square in
// fp64 in a fixed order, and the stopping rule on the device.  No lattice: built into an object of its own (jacobi.hip),
// launched by lt_jacobi.  The per-node arithmetic and the launch geometry also compile for the host (no HIP headers
// then), which is how tests/aux/jacobi_host.cpp runs them without a GPU.
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>

#include "reduce.hpp"
#define LT_JACOBI_HD __host__ __device__ __forceinline__
#else
#define LT_JACOBI_HD inline
#endif

namespace lt {

constexpr int kJacobiThreads = 256;                  // four waves per workgroup
constexpr int kJacobiWaves = kJacobiThreads / 64;
constexpr int kJacobiBlocks = 1024;                  // == LT_JACOBI_BLOCKS: the most workgroup partials

// what the finish launch leaves for the host (and for every later sweep): in the caller's work buffer behind the
// kJacobiBlocks partials
struct JacobiState {
  int done;                   // 1: the iterate `iterations` met the tolerance; sweeps and finish launches return at once
  int pad;
  long long iterations;       // the iterate `error` belongs to
  double error;               // mean(r^2) of that iterate
};

// Fixed launch geometry: workgroup b owns the nodes [b * chunk, (b + 1) * chunk), chunk a multiple of the workgroup's
// 256 nodes, in at most kJacobiBlocks workgroups.
LT_JACOBI_HD long long jacobi_chunk(long long N) {
  const long long pass = kJacobiThreads;
  return ((N + kJacobiBlocks - 1) / kJacobiBlocks + pass - 1) / pass * pass;
}
LT_JACOBI_HD int jacobi_blocks(long long N) { const long long c = jacobi_chunk(N); return (int)((N + c - 1) / c); }

// Node i of a dense periodic field [n0][n1]([n2]) in C order (torch's layout; n2 = 1 in 2-D): the next iterate and the
// residuum of this one.  The reference's arithmetic, operation for operation in T:
//   S      = roll(+1, 0) + roll(+1, 1) [+ roll(+1, 2)] + roll(-1, 0) + roll(-1, 1) [+ roll(-1, 2)], added from the left
//   p_next = (rhs * dx2 - S) * -1 / (2 D)        (a true division: by 6 in 3-D)
//   r      = rhs - (S - (2 D) * p) / dx2
// Extent 1 makes a node its own neighbour, extent 2 both neighbours the same node, as roll does.
template <typename T, int D>
LT_JACOBI_HD void jacobi_node(const T *p, const T *rhs, long long i, int n0, int n1, int n2, T dx2, T &p_next, T &r) {
#pragma clang fp contract(off)
  static_assert(D == 2 || D == 3, "2-D and 3-D fields");
  const long long s1 = n2, s0 = (long long)n1 * n2;
  const int c2 = D == 3 ? (int)(i % n2) : 0;
  const long long row = D == 3 ? i / n2 : i;
  const int c1 = (int)(row % n1), c0 = (int)(row / n1);
  const long long m0 = (c0 == 0 ? (long long)(n0 - 1) : -1LL) * s0, q0 = (c0 == n0 - 1 ? -(long long)(n0 - 1) : 1LL) * s0;
  const long long m1 = (c1 == 0 ? (long long)(n1 - 1) : -1LL) * s1, q1 = (c1 == n1 - 1 ? -(long long)(n1 - 1) : 1LL) * s1;
  T S = p[i + m0] + p[i + m1];
  if (D == 3) S = S + p[i + (c2 == 0 ? n2 - 1 : -1)];
  S = S + p[i + q0];
  S = S + p[i + q1];
  if (D == 3) S = S + p[i + (c2 == n2 - 1 ? -(n2 - 1) : 1)];
  const T f = rhs[i], two_d = (T)(2 * D);
  p_next = ((f * dx2 - S) * T(-1)) / two_d;
  r = f - (S - two_d * p[i]) / dx2;
}

#ifdef __HIPCC__
static_assert(kJacobiThreads == kReduceThreads, "the workgroup reduce.hpp adds up");

// One sweep.  Reads the done flag first and returns without writing once it is set.  Otherwise: p_out = the next iterate
// (p_out == nullptr: not kept -- the sweep behind the last iteration, which is there for the error alone) and
// partial[blockIdx.x] = the sum of r^2 over the workgroup's nodes, r widened to fp64: every thread adds its nodes in
// index order, then the wave tree and the workgroup step of reduce.hpp.
template <typename T, int D>
__global__ void __launch_bounds__(kJacobiThreads) jacobi_sweep_kernel(const T *__restrict__ p_in, const T *__restrict__ rhs,
                                                                      T *__restrict__ p_out, int n0, int n1, int n2,
                                                                      long long chunk, T dx2,
                                                                      const JacobiState *__restrict__ state,
                                                                      double *__restrict__ partial) {
#pragma clang fp contract(off)
  if (state->done) return;
  const long long N = (long long)n0 * n1 * n2;
  const long long begin = (long long)blockIdx.x * chunk, end = begin + chunk < N ? begin + chunk : N;
  double sum = 0.0;
  for (long long i = begin + threadIdx.x; i < end; i += kJacobiThreads) {
    T next, r;
    jacobi_node<T, D>(p_in, rhs, i, n0, n1, n2, dx2, next, r);
    if (p_out) p_out[i] = next;
    const double rd = (double)r;
    sum += rd * rd;
  }
  const double s = block_sum(sum);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// One workgroup after sweep `sweep` (>= 2): error = (partial[0] + partial[1] + ...) / N is the error of iterate
// sweep - 1 -- thread t adds the partials t, t + 256, ... in that order, then the tree and the waves as above -- and is
// held against the tolerance here: !(error > tol) raises the done flag (a NaN error does), as the reference's
// `while error > tol_abs` ends.  Returns at once when the flag is already up: the record keeps the iterate that stopped.
__global__ void __launch_bounds__(kJacobiThreads) jacobi_finish_kernel(const double *__restrict__ partial, int blocks,
                                                                       long long N, long long sweep, double tol,
                                                                       JacobiState *__restrict__ state) {
#pragma clang fp contract(off)
  if (state->done) return;
  double sum = 0.0;
  for (int b = threadIdx.x; b < blocks; b += kJacobiThreads) sum += partial[b];
  const double s = block_sum(sum);
  if (threadIdx.x == 0) {
    const double error = s / (double)N;
    state->iterations = sweep - 1;
    state->error = error;
    if (!(error > tol)) state->done = 1;
  }
}
#endif  // __HIPCC__

}  // namespace lt
