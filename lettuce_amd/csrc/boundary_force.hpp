// Momentum-exchange force on the solid nodes of a full-way bounce-back boundary: one masked reduction over the links
// between a solid node and a fluid neighbour.  Instantiated by the units' part boundary_force only (unit.inc).
#pragma once
#include <hip/hip_runtime.h>

#include "lattice.hpp"
#include "reduce.hpp"

namespace lt {

constexpr int kForceThreads = kReduceThreads;     // four waves per workgroup
constexpr int kForceMaxBlocks = 1024;             // == LT_BOUNDARY_FORCE_BLOCKS: the most workgroups of the first launch
static_assert(kForceMaxBlocks <= kFinishMaxBlocks, "finish_components_kernel stages the partials of every workgroup");
constexpr int kForceBatch = 16;                   // nodes of a thread whose bytes are in flight together
constexpr int kForceSkew = 61;                    // slots a workgroup moves on from one pass to the next

// periodic index of a shifted coordinate: a modulo n in [0, n) for every extent n >= 1, as torch.roll wraps (an extent
// of 1 or 2 is not larger than the stencil's reach) -- kernels.hpp, wrap_index
__device__ __forceinline__ int force_wrap(int a, int n) {
  a %= n;
  return a < 0 ? a + n : a;
}

// First launch.  f: populations [Q][N] post-streaming, reference layout (a0 fastest); solid: one byte per node, nonzero
// on the nodes of the body.  A solid node x_s holds in f_q the population that arrived from x_s - e_q and leaves again
// along -e_q in the same step, so the body takes 2 e_q f_q(x_s) from it -- counted when x_s - e_q (periodic on every
// axis, as streaming wraps) is not solid; links between two solid nodes carry nothing.
//   acc[c] += 2 e_{q,c} f_q(x_s),   c a LOGICAL axis
// A fixed grid; pass k covers the nodes [k P, (k + 1) P), P = gridDim.x * 256, one node per thread, consecutive threads
// along a0: a fluid node costs its one coalesced byte.  Workgroup b takes the 256 nodes of slot (b + k kForceSkew) mod
// gridDim.x of pass k -- with the plain grid stride a thread would meet the same (a0, a1) in every pass (256^3: P is four
// planes of a2) and the threads under the body would do all the work, one node after the other.  A thread reads the
// bytes of kForceBatch passes before it looks at the first (256^3: 4 waits for 64 nodes).  A solid node walks
// q = 1 .. Q - 1 at compile time three times: the neighbours' bytes (independent loads); then, unless every neighbour is
// solid, f_q of the fluid neighbours only (independent again: the other q re-read the node's f_0, one cached word, and
// drop it); then the sums -- a link that carries nothing adds an exact 0.  fp64 from the first operation:
// 2 * (double)f_q and the sign are exact.  Every thread adds its terms in the order of its nodes and of q, then the
// workgroup step of reduce.hpp over the three sums.  partial [3][gridDim.x]; no atomics; the order depends on the grid
// alone.  Second launch: finish_components_kernel (reduce.hpp).
template <typename T, class S>
__global__ void __launch_bounds__(kForceThreads) boundary_force_kernel(const T *__restrict__ f,
                                                                      const unsigned char *__restrict__ solid,
                                                                      long long N, int n0, int n1, int n2,
                                                                      double *__restrict__ partial) {
#pragma clang fp contract(off)
  using M = MemMap<S, 0>;
  static_assert(S::Q <= 32, "a bit per population");
  double acc[3] = {0.0, 0.0, 0.0};
  const long long pass = (long long)gridDim.x * kForceThreads;
  const long long passes = (N + pass - 1) / pass;
  // node of this thread in pass k
  auto node_of = [&](long long k) -> long long {
    const unsigned slot = (unsigned)((blockIdx.x + (unsigned long long)k * kForceSkew) % gridDim.x);
    return k * pass + (long long)slot * kForceThreads + threadIdx.x;
  };
  for (long long k0 = 0; k0 < passes; k0 += kForceBatch) {
    unsigned todo = 0;
#pragma unroll
    for (int j = 0; j < kForceBatch; ++j) {
      // no branch around the load, so that the batch is in flight together: past the end it re-reads the last node
      const long long i = node_of(k0 + j);
      const bool mine = k0 + j < passes && i < N;
      const unsigned char s = solid[mine ? i : N - 1];
      todo |= (unsigned)(mine && s != 0) << j;
    }
    while (todo) {                          // the solid ones, in the order of the passes
      const long long i = node_of(k0 + __ffs(todo) - 1);
      todo &= todo - 1;
      const int c0 = (int)(i % n0), c1 = (int)((i / n0) % n1), c2 = (int)(i / ((long long)n0 * n1));
      unsigned fluid = 0;                   // bit q: the node x_s - e_q is not solid
      static_for<S::Q - 1>([&](auto qc) {
        constexpr int q = decltype(qc)::value + 1;
        const int a0 = M::e(q, 0) ? force_wrap(c0 - M::e(q, 0), n0) : c0;
        const int a1 = M::e(q, 1) ? force_wrap(c1 - M::e(q, 1), n1) : c1;
        const int a2 = M::e(q, 2) ? force_wrap(c2 - M::e(q, 2), n2) : c2;
        fluid |= (unsigned)(solid[((long long)a2 * n1 + a1) * n0 + a0] == 0) << q;
      });
      if (fluid == 0) continue;             // inside the body
      T g[S::Q];
      static_for<S::Q - 1>([&](auto qc) {
        constexpr int q = decltype(qc)::value + 1;
        // a load for every q, so that none waits for the one before: where the link carries nothing it reads the
        // node's rest population instead (one word per surface node, and the same for all such q) and is dropped
        const bool link = fluid >> q & 1u;
        const T v = f[(link ? (long long)q * N : 0ll) + i];
        g[q] = link ? v : T(0);
      });
      static_for<S::Q - 1>([&](auto qc) {
        constexpr int q = decltype(qc)::value + 1;
        const double v = 2.0 * (double)g[q];
        static_for<S::D>([&](auto cc) {
          constexpr int c = decltype(cc)::value;
          if constexpr (S::E[q][c] > 0) acc[c] += v;
          if constexpr (S::E[q][c] < 0) acc[c] -= v;
        });
      });
    }
  }
  const double s = block_reduce<3>(acc);
  if (threadIdx.x < 3) partial[(long long)threadIdx.x * gridDim.x + blockIdx.x] = s;
}

}  // namespace lt
