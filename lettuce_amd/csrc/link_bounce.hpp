// Interpolated (and half-way) bounce-back on a compact list of links, and the momentum-exchange force over the same
// list.  Instantiated by the units' part links only (unit.inc).
//
// A link is (r, x_s): x_s a solid node, r >= 1 a direction with x_f = x_s + e_r not solid; q = opposite(r),
// x_ff = x_f + e_r, neighbours wrapped periodically on every axis as streaming wraps them.  The pass runs on the
// post-collision populations and writes the mirror slot (r, x_s), which plain streaming then carries to (r, x_f).
#pragma once
#include <hip/hip_runtime.h>

#include "lattice.hpp"
#include "reduce.hpp"

namespace lt {

constexpr int kLinkThreads = kReduceThreads;      // four waves per workgroup
constexpr int kLinkMaxBlocks = 1024;              // == LT_LINK_FORCE_BLOCKS: the most workgroups of the force's first launch
static_assert(kLinkMaxBlocks <= kFinishMaxBlocks, "finish_components_kernel stages the partials of every workgroup");

// the lattice as the link kernels index it at run time (the direction of a link is data): the velocities along the
// memory axes a0, a1, a2 of the reference layout, along the logical axes, and the opposite directions
struct LinkTable {
  signed char em[27][3];
  signed char el[27][3];
  unsigned char opp[27];
};
template <class S>
LinkTable link_table() {
  LinkTable t = {};
  for (int q = 0; q < S::Q; ++q) {
    for (int m = 0; m < 3; ++m) {
      t.em[q][m] = (signed char)MemMap<S, 0>::e(q, m);
      t.el[q][m] = (signed char)S::E[q][m];
    }
    t.opp[q] = (unsigned char)S::OPP[q];
  }
  return t;
}

// the compact list, in plan-owned device memory (api.hip, lt_plan_set_links): sorted by node, then by direction
template <typename T>
struct LinkList {
  const int *node;               // x_s, index within a population
  const unsigned char *dir;      // r, 1 .. Q - 1
  const T *c1, *c2;              // the two coefficients, as torch rounded them in T
  const unsigned char *second;   // 0: B = f_q(x_ff) (d < 1/2), 1: B = f_r(x_f) (d >= 1/2)
  int n;
};

// periodic index of a shifted coordinate: a modulo n in [0, n) for every extent n >= 1 (kernels.hpp, wrap_index)
__device__ __forceinline__ int link_wrap(int a, int n) {
  a %= n;
  return a < 0 ? a + n : a;
}

// x_f = x_s + e_r and, with twice = true, x_ff = x_s + 2 e_r, as indices within a population
struct LinkNodes {
  long long xf, xff;
};
__device__ __forceinline__ LinkNodes link_nodes(int xs, int r, int n0, int n1, int n2, const LinkTable &t) {
  const int c0 = xs % n0, c1 = (xs / n0) % n1, c2 = xs / (n0 * n1);
  const int e0 = t.em[r][0], e1 = t.em[r][1], e2 = t.em[r][2];
  const int f0 = link_wrap(c0 + e0, n0), f1 = link_wrap(c1 + e1, n1), f2 = link_wrap(c2 + e2, n2);
  const int g0 = link_wrap(f0 + e0, n0), g1 = link_wrap(f1 + e1, n1), g2 = link_wrap(f2 + e2, n2);
  return {((long long)f2 * n1 + f1) * n0 + f0, ((long long)g2 * n1 + g1) * n0 + g0};
}

// One thread per link.  f: post-collision populations [Q][stride]; reads A = f_q(x_f) and B (two fluid nodes), writes
// f_r(x_s) = c1 A + c2 B -- two products and one sum, each rounded on its own as the torch expression rounds them.
// Every slot has one writer (the list holds a link once) and no thread reads a slot another writes (sources are fluid
// nodes, destinations solid ones), so the pass is in place.
template <typename T, class S>
__global__ void __launch_bounds__(kLinkThreads) link_bounce_kernel(T *__restrict__ f, long long stride,
                                                                   const LinkList<T> l, int n0, int n1, int n2,
                                                                   const LinkTable t) {
#pragma clang fp contract(off)
  const int i = (int)(blockIdx.x * kLinkThreads + threadIdx.x);
  if (i >= l.n) return;
  const int xs = l.node[i], r = l.dir[i];
  const bool second = l.second[i] != 0;
  const T c1 = l.c1[i], c2 = l.c2[i];
  const LinkNodes x = link_nodes(xs, r, n0, n1, n2, t);
  const int q = t.opp[r];
  const T a = f[(long long)q * stride + x.xf];
  const T b = f[(long long)(second ? r : q) * stride + (second ? x.xf : x.xff)];
  const T pa = c1 * a;
  const T pb = c2 * b;
  f[(long long)r * stride + xs] = pa + pb;
}

// Momentum-exchange force over the list, on POST-STREAMING populations: f_q(x_s) is what left the fluid along the link,
// f_r(x_f) what came back;   acc[c] += e_{q,c} f_q(x_s);  acc[c] += e_{q,c} f_r(x_f),   c a LOGICAL axis
// (for d = 1/2 the two are equal: the 2 e_q f_q(x_s) of boundary_force.hpp).  fp64 from the first operation, the sign
// is exact.  A fixed grid: workgroup b, thread t takes the links b 256 + t + k gridDim.x 256, k = 0, 1, ..., and adds its
// terms in that order; then the workgroup step of reduce.hpp over the three sums.  partial [3][gridDim.x]; no atomics;
// the order depends on the list's length alone.  Second launch: finish_components_kernel (reduce.hpp; an empty list
// launches it alone, with blocks = 0).
template <typename T, class S>
__global__ void __launch_bounds__(kLinkThreads) link_force_kernel(const T *__restrict__ f, long long stride,
                                                                  const LinkList<T> l, int n0, int n1, int n2,
                                                                  const LinkTable t, double *__restrict__ partial) {
#pragma clang fp contract(off)
  double acc[3] = {0.0, 0.0, 0.0};
  const long long pass = (long long)gridDim.x * kLinkThreads;
  for (long long i = (long long)blockIdx.x * kLinkThreads + threadIdx.x; i < l.n; i += pass) {
    const int xs = l.node[i], r = l.dir[i];
    const LinkNodes x = link_nodes(xs, r, n0, n1, n2, t);
    const int q = t.opp[r];
    const double out = (double)f[(long long)q * stride + xs];
    const double back = (double)f[(long long)r * stride + x.xf];
#pragma unroll
    for (int c = 0; c < S::D; ++c) {
      const int e = t.el[q][c];
      if (e > 0) { acc[c] += out; acc[c] += back; }
      if (e < 0) { acc[c] -= out; acc[c] -= back; }
    }
  }
  const double s = block_reduce<3>(acc);
  if (threadIdx.x < 3) partial[(long long)threadIdx.x * gridDim.x + blockIdx.x] = s;
}

}  // namespace lt
