// Hand-written gfx950 kernels of the stream-and-collide hot path.
//
// One kernel template covers the three operators the host composes
// (see include/lettuce_hip.h):
//   STREAM && COLLIDE   f*_out = B(C(S(f*_in)))   fused pull scheme (the hot kernel)
//   !STREAM && COLLIDE  f*_out = B(C(f_in))       prologue of lt_run
//   STREAM && !COLLIDE  f_out  = S(f*_in)         epilogue of lt_run
// where S = Simulation._stream (lettuce/_simulation.py:160-175), C = the collision operator
// (bgk_collision.py:17-22 / kbc_collision.py:96-160 with quadratic_equilibrium.py:11-25 and
// Flow.rho/j/u, _flow.py:136-172) and B = the boundaries applied in index order
// (_simulation.py:177-189).
//
// Design for MI355X (HBM-bound: 2*q*sizeof(T) bytes per node, ~2-4 flop/byte, no MFMA):
//  * SoA per velocity; a thread owns one node, so consecutive lanes read and write consecutive
//    elements of every population, fully coalesced (16-byte accesses of several nodes per thread
//    measured 8-13 % slower in round 1: fewer waves per SIMD).
//  * Pull scheme: each slot of f*_in is read by exactly one thread, each slot of the output
//    is written by exactly one thread (no atomics, no write races, no halo re-reads), so HBM
//    traffic stays at the algorithmic 2*q*sizeof(T) per node.
//  * Everything between the loads and the stores lives in VGPRs; the lattice is a template
//    parameter so e_q, w_q and the opposite table are folded into the instruction stream.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dispatch.hpp"
#include "lattice.hpp"
#include "launch_limits.hpp"
#include "mrt.hpp"
#include "reduce.hpp"
#include "twostep_roles.hpp"

namespace lt {

constexpr int kThreads = 256;
static_assert(kThreads == kReduceThreads, "the reducing kernels launch the workgroup reduce.hpp adds up");
constexpr int kMaxB = 127;   // == LT_MAX_BOUNDARIES: what the node byte's seven index bits can name

// boundary kinds (== lt_boundary_kind)
constexpr int kBounceBack = 1, kEquilibrium = 2, kAbbOutlet = 3;
// ... and the constant-pressure equilibrium outlet.  Only kernels instantiated for it know this kind: an outlet depth
// (the kernels' ABBD, neighbour_moments' DEPTH) of kOutletsP + chain, the reserved range above the depths 0-2 of the
// plans with anti-bounce-back outlets alone, whose kernels are compiled from the same text as before
constexpr int kPressureOutlet = 4;
constexpr int kOutletsP = 4;

template <typename T>
struct BoundaryTable {
  int kind[kMaxB + 1];       // [1..nb]
  int mem_axis[kMaxB + 1];   // ABB: memory axis of the outlet normal
  int side[kMaxB + 1];       // ABB: +1 / -1 along that memory axis
  int plane[kMaxB + 1];      // ABB: memory coordinate of the outlet plane
  int nbr[kMaxB + 1];        // ABB: memory coordinate of the plane next to it (inside)
  T feq[kMaxB + 1][27];      // EQUILIBRIUM, uniform
  const T *field[kMaxB + 1]; // EQUILIBRIUM, per node [q][N] (or null)
  T rho_outlet[kMaxB + 1];   // PRESSURE OUTLET: the density it imposes, in the plan's scalar type
};

template <typename T>
struct KParams {
  const T *in;
  T *out;
  int n0, n1, n2;            // memory extents; n2 includes ghost planes
  int nv0;                   // one-step kernels: threads per row (n0)
  int p_begin;               // first a2 plane of this launch
  int p_end;                 // two-step kernel: one past the last output plane
  int p_begin2, p_end2;      // two-step kernel: optional second range of output planes (slab edges)
  int p_stride;              // distance between consecutive planes of this launch (normally 1)
  int wrap2;                 // periodic wrap along a2 (0 with ghost planes)
  long long N;               // n0*n1*n2: nodes per population (and the stride of a boundary's per-node field)
  long long Ni, No;          // distance between consecutive populations of `in` / of `out`, in elements (>= N:
                             // engine-owned buffers are padded so that the q streams of a node do not meet in the
                             // same memory channels, DESIGN.md section 4 "population stride")
  unsigned nvec_total;       // threads doing work: nv0 * n1 * planes
  T tau_inv;                 // BGK: 1/tau
  T beta, inv_beta;          // KBC: 1/(2 tau), 1/beta; TRT reads beta as 1/(2 tau_plus)
  T tau, smag_c2;            // Smagorinsky: tau and the squared constant.  smag_c2 is the collision's own scalar: what
                             // it means to TRT and the regularised collision is said once, at collide_node
  const unsigned char *node; // [N] boundary index | 0x80 if any no-streaming bit (or null)
  const unsigned *nsm_bits;  // [N] bit q set: population q keeps its value (or null)
  const BoundaryTable<T> *bt;
  int nb;
  // slab boundary launch (PACK kernels): the crossing populations of plane pack_lo_plane
  // (e along a2 = -1) / pack_hi_plane (+1) are also written to contiguous send buffers
  // [k][n1*n0], k = rank of q among the populations with that e (ascending q)
  T *pack_lo, *pack_hi;
  int pack_lo_plane, pack_hi_plane;
  // one-step kernels: slot of the plan's only anti-bounce-back outlet when its normal is the contiguous axis
  // and the rows are whole waves (n0 % 64 == 0): the node next to an outlet node then sits in the next lane
  // (lbm_body); 0: none
  int abb0_slot;
  // two-step slab launch that covers the whole slab and releases the exchange while it runs (slab layout):
  // edge_first != 0: the workgroups of the second plane range (the upper edge) and of the first segment of
  // the first range (the lower edge) get the lowest block indices; each of them adds 1 to *signal once its
  // two planes next to the cut are in memory (wait_counter_kernel on the communication stream polls it)
  unsigned long long *signal;
  int edge_first;
  // two-step slab EDGE launch that takes the neighbours' planes straight from the receive buffers (MODE 1 of
  // lbm2_kernel): ghost_lo / ghost_hi = the halo message that arrived from the rank below / above (layout of
  // halo2_kernel), read wherever the pull reaches below plane `lo` / beyond plane `hi - 1`; null = the ghost planes
  // of the field hold them (they were unpacked)
  const T *ghost_lo, *ghost_hi;
  int lo, hi;                // first interior plane, one past the last interior plane
};

// The parameters of a kernel with a body force (COLL & 4): KParams and, behind it, the uniform acceleration.  A type of
// its own, taken by overloads of the kernels, so that the argument block of every unforced kernel -- and with it that
// kernel's code -- stays what it was.
template <typename T>
struct KParamsF : KParams<T> {
  T accel[3];                // acceleration along the MEMORY axes a0, a1, a2 (the units permute it; 0 beyond the lattice's d)
  T shift[3];                // ueq_scale * accel (Guo 1/2, Shan-Chen force.tau): u* = j / rho + shift / rho
  T source_scale;            // Guo: 1 - 1 / (2 force.tau), Shan-Chen: 0
};

// The parameters of a kernel with a body force whose acceleration is a per-node field (COLL & 32; dispatch.hpp,
// kCollField): KParams and, behind it, the field and the two scales of the scheme.  A type of its own again: the
// kernels of the uniform force keep their argument block.
template <typename T>
struct KParamsFF : KParams<T> {
  const T *accel_field;      // [D][N]: component c (LOGICAL axis) of node `own` at c * N + own; dense, read-only
  T ueq_scale;               // Guo 1/2, Shan-Chen force.tau: the node's shift is ueq_scale * a(x), formed in T
  T source_scale;            // Guo: 1 - 1 / (2 force.tau), Shan-Chen: 0
};

// The acceleration of one node and its velocity shift, along the MEMORY axes: what collide_forced takes.  The kernels of
// the uniform force hand over KParamsF's two arrays, those of a field load theirs (load_node_force).
template <typename T>
struct NodeForce {
  T accel[3], shift[3];
};

// The parameters of a kernel with the multiple-relaxation-time collision (COLL 10, 11; mrt.hpp): KParams and, behind it,
// the reciprocal relaxation rates of the q moments.  A type of its own for the same reason.
template <typename T>
struct KParamsM : KParams<T> {
  T r[kMrtMaxQ];             // r_i = 1 / s_i, formed in T (unit.inc); 0 beyond the lattice's q
};

// The parameters of a kernel with the incompressible equilibrium (COLL & 16; dispatch.hpp, kCollIncompressible): KParams
// -- with a body force KParamsF -- and, behind it, the equilibrium's reference density.  Types of their own once more.
template <typename T>
struct KParamsI : KParams<T> {
  T rho0;                    // rho0 of IncompressibleQuadraticEquilibrium, rounded to T once on the host (unit.inc)
};
template <typename T>
struct KParamsFI : KParamsF<T> {
  T rho0;
};

// ---- constants the reference builds from cs = 1/np.sqrt(3.0) (lettuce/_stencil.py:17) ----
// cs**2 evaluates to 0.33333333333333337 in double; keep that value, not 1/3.
constexpr double kCs = 0.57735026918962584;   // 1/sqrt(3) rounded to double
constexpr double kCs2 = kCs * kCs;
constexpr double kCs4 = kCs2 * kCs2;

// ---- population access ----------------------------------------------------------------------
// NT = nontemporal hint: the populations are streamed once per step and the working set
// (2.5 GB at 256^3) is far beyond L2 + Infinity Cache, so nothing is gained by keeping lines.
template <typename T, bool NT = false>
__device__ __forceinline__ T load(const T *__restrict__ p) {
  return NT ? __builtin_nontemporal_load(p) : *p;
}
template <typename T, bool NT = false>
__device__ __forceinline__ void store(T *__restrict__ p, T v) {
  if constexpr (NT) __builtin_nontemporal_store(v, p); else *p = v;
}

// ---- node coordinates -----------------------------------------------------------------------
struct Coord {
  int c0, c1, c2;      // own
  int c1m, c1p;        // periodic neighbours along a1
  int c2m, c2p;        // neighbours along a2 (periodic iff wrap2)
};

template <typename T>
__device__ __forceinline__ Coord make_coord(const KParams<T> &p, int c0, int c1, int c2) {
  Coord c;
  c.c0 = c0; c.c1 = c1; c.c2 = c2;
  c.c1m = c1 == 0 ? p.n1 - 1 : c1 - 1;
  c.c1p = c1 == p.n1 - 1 ? 0 : c1 + 1;
  c.c2m = c2 - 1;
  c.c2p = c2 + 1;
  if (p.wrap2) {
    if (c.c2m < 0) c.c2m = p.n2 - 1;
    if (c.c2p == p.n2) c.c2p = 0;
  }
  return c;
}

// ---- gather: post-streaming populations of one node ------------------------------------
// f_q(x) = f*_q(x - e_q), periodic (Simulation._stream: torch.roll by +e_q,
// lettuce/_simulation.py:156-158,164-175)
template <typename T, class S, int LAYOUT, bool STREAM, bool NTL = false>
__device__ __forceinline__ void gather(const KParams<T> &p, const Coord &c, T (&f)[S::Q][1]) {
  using M = MemMap<S, LAYOUT>;
  const int n0 = p.n0, n1 = p.n1;
  const unsigned own = (unsigned)(c.c2 * n1 + c.c1) * (unsigned)n0 + (unsigned)c.c0;
  static_for<S::Q>([&](auto qc) {
    constexpr int q = decltype(qc)::value;
    const T *__restrict__ src = p.in + (long long)q * p.Ni;
    if constexpr (!STREAM) {
      f[q][0] = load<T, NTL>(src + own);
    } else {
      constexpr int e0 = M::e(q, 0), e1 = M::e(q, 1), e2 = M::e(q, 2);
      const int s1 = e1 == 0 ? c.c1 : (e1 > 0 ? c.c1m : c.c1p);
      const int s2 = e2 == 0 ? c.c2 : (e2 > 0 ? c.c2m : c.c2p);
      const unsigned row = (unsigned)(s2 * n1 + s1) * (unsigned)n0;
      if constexpr (e0 == 0) {
        f[q][0] = load<T, NTL>(src + row + c.c0);
      } else {
        const int s0 = e0 > 0 ? (c.c0 == 0 ? n0 - 1 : c.c0 - 1) : (c.c0 == n0 - 1 ? 0 : c.c0 + 1);
        f[q][0] = src[row + s0];
      }
    }
  });
}

// destination-side no-streaming mask: slot (q, x) keeps the value it had before streaming
// (lettuce/_simulation.py:171-174)
template <typename T, class S, int VEC, int k>
__device__ __forceinline__ void keep_unstreamed(const KParams<T> &p, unsigned own,
                                                T (&f)[S::Q][VEC]) {
  const unsigned bits = p.nsm_bits[own + k];
  static_for<S::Q>([&](auto qc) {
    constexpr int q = decltype(qc)::value;
    if constexpr (q > 0) {   // population 0 never moves (_simulation.py:165)
      if (bits & (1u << q)) f[q][k] = p.in[(long long)q * p.Ni + own + k];
    }
  });
}

// ---- moments (Flow.rho / Flow.j / Flow.u, lettuce/_flow.py:136-138,152-172) ---------------
// j += e_q * v along the three memory axes, all signs folded at compile time
template <class S, int LAYOUT, int q, typename T>
__device__ __forceinline__ void add_momentum(T (&j)[3], T v) {
  using M = MemMap<S, LAYOUT>;
  static_for<3>([&](auto mc) {
    constexpr int m = decltype(mc)::value;
    constexpr int e = M::e(q, m);
    if constexpr (e > 0) j[m] += v;
    else if constexpr (e < 0) j[m] -= v;
  });
}
// e_q . u, accumulated over the logical axes x, y, z from zero (the GEMM order of the reference's
// tensordot(e, u); matters for the three-component velocities of D3Q15 / D3Q27)
template <class S, int LAYOUT, int q, typename T>
__device__ __forceinline__ T dot_e(const T (&u)[3]) {
  using M = MemMap<S, LAYOUT>;
  T r = T(0);
  static_for<S::D>([&](auto ac) {
    constexpr int a = decltype(ac)::value;
    constexpr int e = S::E[q][a];
    if constexpr (e > 0) r += u[M::memory(a)];
    else if constexpr (e < 0) r -= u[M::memory(a)];
  });
  return r;
}

// Sum over q in the order of torch.sum(f, dim=0) on the CPU (ATen cascade_sum: the first 16
// terms are accumulated from zero, then the remaining terms from zero, then the two partial sums
// are added) -- bit-identical to the reference's Flow.rho() for every lattice; sum_q e_q f_q is a
// GEMM in the reference and accumulates sequentially in q, as add_momentum does.
template <int Q, typename T>
struct CascadeSum {
  T head = T(0), tail = T(0);
  template <int q>
  __device__ __forceinline__ void add(T v) {
#pragma clang fp contract(off)
    if constexpr (q < 16) head += v; else tail += v;      // (never fused with the product that made v)
  }
  __device__ __forceinline__ T result() const {
    if constexpr (Q > 16) return tail + head; else return head;
  }
};

template <typename T, class S, int LAYOUT, int VEC, int k>
__device__ __forceinline__ void moments(const T (&f)[S::Q][VEC], T &rho, T (&j)[3]) {
  CascadeSum<S::Q, T> mass;
  j[0] = j[1] = j[2] = T(0);
  static_for<S::Q>([&](auto qc) {
    constexpr int q = decltype(qc)::value;
    const T v = f[q][k];
    mass.template add<q>(v);
    add_momentum<S, LAYOUT, q>(j, v);
  });
  rho = mass.result();
}

__device__ __forceinline__ float fma_t(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fma_t(double a, double b, double c) { return __builtin_fma(a, b, c); }

// value barrier: the optimiser may not assume anything about x afterwards
__device__ __forceinline__ float launder(float x) { asm volatile("" : "+v"(x)); return x; }
__device__ __forceinline__ double launder(double x) { asm volatile("" : "+v"(x)); return x; }

// u.u summed in the logical order x, y, z with separately rounded products and sums -- what
// torch's einsum("d...,d...->...") produces on the CPU (checked bit for bit against the reference's
// vectors), so that feq(rho, u) is reproduced exactly, not just to an ulp
template <class S, int LAYOUT, typename T>
__device__ __forceinline__ T square_norm(const T (&u)[3]) {
#pragma clang fp contract(off)
  using M = MemMap<S, LAYOUT>;
  T r = u[M::memory(0)] * u[M::memory(0)];
  if constexpr (S::D > 1) r = r + u[M::memory(1)] * u[M::memory(1)];
  if constexpr (S::D > 2) r = r + u[M::memory(2)] * u[M::memory(2)];
  return r;
}

// x / D for the constants D = 2 cs^2 and cs^2 of the equilibrium.  The reference divides the fp32
// field by the python double cast to fp32 (D_f = 0.66666669 / 0.33333334, 3e-8 above 2/3 and 1/3);
// that systematic 3e-8 is what makes its fp32 kinetic energy drift by -1.1e-7 per step against its
// fp64 run.  To track the reference's fp32 path (not just fp64 truth) the same IEEE quotient is
// formed, in three instructions instead of the ~10 of a division: q = RN(x r) with r = RN(1 / D),
// the exact remainder x - q D by FMA, one correction step (Markstein).  Equal to x / D for every
// fp32 x with |x / D| >= 1e-30 (exhaustive, tests/aux/exact_division_check.c) and in 6.4e9 random
// fp64 quotients.
// fp32 (round 3): TWO instructions -- x r_hi + RN(x r_lo) with r_hi + r_lo = 1 / D to twice the precision, one
// rounding of a sum that is x / D to 2^-47 -- equal to x / D for EVERY fp32 x with |x / D| >= 1e-30 for these two
// constants (exhaustive as well: exact_division_check f32two 1; the general argument does not exclude a quotient that
// close to a rounding boundary, so fp64 keeps the three-instruction form, which Markstein's theorem covers).  The
// equilibrium calls this 28 times per node: 7 % of the collision's issue slots.
template <int WHICH, typename T>   // 0: D = 2 cs^2, 1: D = cs^2
__device__ __forceinline__ T div_cs(T x) {
  constexpr T d = (T)(WHICH == 0 ? 2.0 * kCs2 : kCs2);
  constexpr T r = (T)(1.0 / (double)d);
  if constexpr (sizeof(T) == 4) {
    constexpr T r_lo = (T)(1.0 / (double)d - (double)r);
    const T low = x * r_lo;                           // rounded on its own: a product feeding an fma's addend
    return fma_t(x, r, low);
  } else {
    const T q = x * r;
    const T rem = fma_t(-q, d, x);
    return fma_t(rem, r, q);
  }
}

// QuadraticEquilibrium (lettuce/ext/_equilibrium/quadratic_equilibrium.py:15-24), u along
// memory axes (the dot products are invariant under the axis permutation)
template <typename T, class S, int LAYOUT, int q>
__device__ __forceinline__ T feq_q(T rho, const T (&u)[3], T uxu) {
  // every operation rounds separately, as the reference's whole-field torch ops do: with
  // mul+add fused the 1-ulp differences are correlated with the sign of e.u and halve the
  // (reference-inherent) fp32 momentum deficit of the equilibrium
#pragma clang fp contract(off)
  const T exu = dot_e<S, LAYOUT, q>(u);
  const T a = div_cs<0>(T(2) * exu - uxu);
  const T b = div_cs<1>(exu);
  return T(S::W[q]) * (rho * (a + T(0.5) * (b * b) + T(1)));
}

// the same for population q and its opposite o (q < o) together: e_o = -e_q, so e_o.u, 2 e_o.u
// and (e_o.u) / cs^2 are the exact negatives and the quadratic term is shared -- the two values
// are bit for bit what feq_q<q> and feq_q<o> return, for a third less arithmetic
template <typename T, class S, int LAYOUT, int q>
__device__ __forceinline__ void feq_pair(T rho, const T (&u)[3], T uxu, T &fq, T &fo) {
#pragma clang fp contract(off)
  const T exu = dot_e<S, LAYOUT, q>(u);
  const T b = div_cs<1>(exu);
  const T h = T(0.5) * (b * b);
  // 2 e.u is exact, so one fused multiply-add IS the reference's "2 * exu - uxu" (two roundings of which the first
  // does nothing): one instruction instead of two per population
  const T two = T(2) * exu;
  const T aq = div_cs<0>(two - uxu);
  const T ao = div_cs<0>(-two - uxu);
  fq = T(S::W[q]) * (rho * (aq + h + T(1)));
  fo = T(S::W[q]) * (rho * (ao + h + T(1)));
}

// fn(q, feq_q) for every q (opposite pairs back to back, not in index order)
template <typename T, class S, int LAYOUT, class F>
__device__ __forceinline__ void for_each_feq(T rho, const T (&u)[3], T uxu, F &&fn) {
  static_for<S::Q>([&](auto qc) {
    constexpr int q = decltype(qc)::value;
    constexpr int o = S::OPP[q];
    if constexpr (q == o) {
      fn(qc, feq_q<T, S, LAYOUT, q>(rho, u, uxu));
    } else if constexpr (q < o) {
      T a, b;
      feq_pair<T, S, LAYOUT, q>(rho, u, uxu, a, b);
      fn(qc, a);
      fn(std::integral_constant<int, o>{}, b);
    }
  });
}

// IncompressibleQuadraticEquilibrium (lettuce/ext/_equilibrium/incompressible_quadratic_equilibrium.py:14-26):
//   feq_q = w_q (rho + rho0 ((2 e_q.u - u.u) / (2 cs^2) + (e_q.u / cs^2)^2 / 2)),
// with u = j / rho as the reference has it.  The three functions above once more, every operation rounded on its own.
template <typename T, class S, int LAYOUT, int q>
__device__ __forceinline__ T feq_inc_q(T rho, T rho0, const T (&u)[3], T uxu) {
#pragma clang fp contract(off)
  const T exu = dot_e<S, LAYOUT, q>(u);
  const T a = div_cs<0>(T(2) * exu - uxu);
  const T b = div_cs<1>(exu);
  return T(S::W[q]) * (rho + rho0 * (a + T(0.5) * (b * b)));
}

// population q and its opposite o (q < o) together: the quadratic term is shared, as in feq_pair
template <typename T, class S, int LAYOUT, int q>
__device__ __forceinline__ void feq_inc_pair(T rho, T rho0, const T (&u)[3], T uxu, T &fq, T &fo) {
#pragma clang fp contract(off)
  const T exu = dot_e<S, LAYOUT, q>(u);
  const T b = div_cs<1>(exu);
  const T h = T(0.5) * (b * b);
  const T two = T(2) * exu;
  const T aq = div_cs<0>(two - uxu);
  const T ao = div_cs<0>(-two - uxu);
  fq = T(S::W[q]) * (rho + rho0 * (aq + h));
  fo = T(S::W[q]) * (rho + rho0 * (ao + h));
}

// fn(q, feq_q) for every q, in the order of for_each_feq
template <typename T, class S, int LAYOUT, class F>
__device__ __forceinline__ void for_each_feq_inc(T rho, T rho0, const T (&u)[3], T uxu, F &&fn) {
  static_for<S::Q>([&](auto qc) {
    constexpr int q = decltype(qc)::value;
    constexpr int o = S::OPP[q];
    if constexpr (q == o) {
      fn(qc, feq_inc_q<T, S, LAYOUT, q>(rho, rho0, u, uxu));
    } else if constexpr (q < o) {
      T a, b;
      feq_inc_pair<T, S, LAYOUT, q>(rho, rho0, u, uxu, a, b);
      fn(qc, a);
      fn(std::integral_constant<int, o>{}, b);
    }
  });
}

// ---- collisions ---------------------------------------------------------------------------
// EQ (last and defaulted, with rho0 behind the collision's scalars): 0 = the quadratic equilibrium, 1 = the
// incompressible one, which does not conserve momentum (sum_q e_q feq_q = rho0 u): where a kernel reads a neighbour's
// moments after its collision, it collides that neighbour (neighbour_moments).
template <typename T, class S, int LAYOUT, int VEC, int k, int EQ = 0>
__device__ __forceinline__ void collide_bgk(T (&f)[S::Q][VEC], T tau_inv, T rho0 = T(0)) {
  T rho, j[3], u[3];
  moments<T, S, LAYOUT, VEC, k>(f, rho, j);
  u[0] = j[0] / rho; u[1] = j[1] / rho; u[2] = j[2] / rho;
  const T uxu = square_norm<S, LAYOUT>(u);
  if constexpr (EQ == 0) {
    for_each_feq<T, S, LAYOUT>(rho, u, uxu, [&](auto qc, T feq) {
#pragma clang fp contract(off)
      constexpr int q = decltype(qc)::value;
      f[q][k] = f[q][k] - tau_inv * (f[q][k] - feq);
    });
  } else {
    for_each_feq_inc<T, S, LAYOUT>(rho, rho0, u, uxu, [&](auto qc, T feq) {
#pragma clang fp contract(off)
      constexpr int q = decltype(qc)::value;
      f[q][k] = f[q][k] - tau_inv * (f[q][k] - feq);
    });
  }
}

// KBC.  The reference forms s(f) and s(feq) from the second moments m/rho of f and of feq
// (lettuce/ext/_collision/kbc_collision.py:25-39 moments, :44-94 s_i), each s_i being rho times a
// linear combination of the normalised moments -- i.e. a linear function of the populations -- and
// then ds = s(f) - s(feq).  Here ds is evaluated as s(f - feq) from the raw second moments of
// x = f - feq: no division by rho and re-multiplication, one moment pass instead of two, and the
// opposite pairs (equal e_a e_b) are summed first.  Same value up to rounding; KBC is compared with
// the reference at rounding level, not bit for bit.
template <typename T, class S>
struct KbcS {
  T s0, sa, sb, sc, pxy, pxz, pyz;   // 3-D: s0, s1(=s2), s3(=s4), s5(=s6), s15, s11, s7
  template <int q>
  static constexpr int sign() {       // get<q>() == sign * component, 0: this s_q is zero
    if constexpr (S::D == 3) return q >= 19 ? 0 : ((q >= 9 && q <= 10) || (q >= 13 && q <= 14) || q >= 17) ? -1 : 1;
    else return (q == 6 || q == 8) ? -1 : 1;
  }
  template <int q>
  __device__ __forceinline__ T magnitude() const {
    if constexpr (S::D == 3) {
      if constexpr (q == 0) return s0;
      else if constexpr (q <= 2) return sa;
      else if constexpr (q <= 4) return sb;
      else if constexpr (q <= 6) return sc;
      else if constexpr (q <= 10) return pyz;
      else if constexpr (q <= 14) return pxz;
      else if constexpr (q <= 18) return pxy;
      else return T(0);
    } else {
      if constexpr (q == 0) return s0;
      else if constexpr (q == 1 || q == 3) return sa;
      else if constexpr (q == 2 || q == 4) return sb;
      else return pxy;
    }
  }
  __device__ __forceinline__ KbcS scaled(T c) const {
    return KbcS{c * s0, c * sa, c * sb, c * sc, c * pxy, c * pxz, c * pyz};
  }
};

// s(g) for a population set given as g(q), from raw second moments (logical axes x, y, z)
template <typename T, class S, class G>
__device__ __forceinline__ KbcS<T, S> kbc_s(const G &g) {
#pragma clang fp contract(off)
  T xx = T(0), yy = T(0), zz = T(0), xy = T(0), xz = T(0), yz = T(0);
  static_for<S::Q>([&](auto qc) {
    constexpr int q = decltype(qc)::value;
    constexpr int o = S::OPP[q];
    if constexpr (q < o) {
      constexpr int ex = S::E[q][0], ey = S::E[q][1], ez = S::E[q][2];
      const T v = g(qc) + g(std::integral_constant<int, o>{});
      if constexpr (ex != 0) xx += v;
      if constexpr (ey != 0) yy += v;
      if constexpr (ez != 0) zz += v;
      if constexpr (ex * ey > 0) xy += v; else if constexpr (ex * ey < 0) xy -= v;
      if constexpr (ex * ez > 0) xz += v; else if constexpr (ex * ez < 0) xz -= v;
      if constexpr (ey * ez > 0) yz += v; else if constexpr (ey * ez < 0) yz -= v;
    }
  });
  KbcS<T, S> s;
  if constexpr (S::D == 3) {
    const T Tr = xx + yy + zz, nxz = xx - zz, nyz = yy - zz;
    s.s0 = -Tr;
    s.sa = T(1. / 6.) * (T(2) * nxz - nyz + Tr);
    s.sb = T(1. / 6.) * (T(2) * nyz - nxz + Tr);
    s.sc = T(1. / 6.) * (-nxz - nyz + Tr);
    s.pyz = T(0.25) * yz;
    s.pxz = T(0.25) * xz;
    s.pxy = T(0.25) * xy;
  } else {
    const T Tr = xx + yy, n = xx - yy;
    s.s0 = -Tr;
    s.sa = T(0.5) * (T(0.5) * (Tr + n));
    s.sb = T(0.5) * (T(0.5) * (Tr - n));
    s.sc = T(0);
    s.pxy = T(0.25) * xy;
    s.pxz = s.pyz = T(0);
  }
  return s;
}

// x / y for the two entropic sums of KBC.  The reference divides twice per population
// (ds*dh/feq and dh*dh/feq, kbc_collision.py:150-151); here dh/feq is formed once and, in fp32,
// with the hardware reciprocal (<= 1 ulp) instead of the ~10-instruction IEEE sequence: the sums
// feed only gamma, whose own rounding noise (dh is a difference of nearly equal numbers) is three
// orders of magnitude larger.
__device__ __forceinline__ float kbc_ratio(float x, float y) { return x * __builtin_amdgcn_rcpf(y); }
__device__ __forceinline__ double kbc_ratio(double x, double y) { return x / y; }

// f' = f - beta (2 ds + gamma dh), dh = f - feq - ds (kbc_collision.py:130-158), evaluated as
// f - (beta gamma) (f - feq) - (beta (2 - gamma)) ds with the seven distinct ds values scaled once.
// No contraction by the compiler anywhere in the collision (round 4): which multiply-adds hipcc fused depended on the
// kernel the function was inlined into, so the fused, the collide-only, the many-step and the two-step KBC kernels
// agreed at rounding level only.  The two multiply-adds worth an instruction are written as fma_t.
template <typename T, class S, int LAYOUT, int VEC, int k>
__device__ __forceinline__ void collide_kbc(T (&f)[S::Q][VEC], T beta, T inv_beta) {
#pragma clang fp contract(off)
  static_assert(S::Q == 9 || S::Q == 27, "KBC exists for D2Q9 and D3Q27 only (kbc_collision.py:100-128)");
  T rho, j[3], u[3];
  moments<T, S, LAYOUT, VEC, k>(f, rho, j);
  u[0] = j[0] / rho; u[1] = j[1] / rho; u[2] = j[2] / rho;
  const T uxu = square_norm<S, LAYOUT>(u);
  T feq[S::Q];
  for_each_feq<T, S, LAYOUT>(rho, u, uxu, [&](auto qc, T v) { feq[decltype(qc)::value] = v; });
  const KbcS<T, S> ds = kbc_s<T, S>([&](auto qc) {
    constexpr int q = decltype(qc)::value;
    return f[q][k] - feq[q];
  });
  CascadeSum<S::Q, T> acc_s, acc_h;
  static_for<S::Q>([&](auto qc) {
    constexpr int q = decltype(qc)::value;
    constexpr int sg = KbcS<T, S>::template sign<q>();
    const T x = f[q][k] - feq[q];
    const T m = ds.template magnitude<q>();
    const T dh = sg == 0 ? x : (sg > 0 ? x - m : x + m);
    const T t = kbc_ratio(dh, feq[q]);
    if constexpr (sg > 0) acc_s.template add<q>(m * t);
    if constexpr (sg < 0) acc_s.template add<q>(-(m * t));
    acc_h.template add<q>(dh * t);
  });
  const T sum_s = acc_s.result(), sum_h = acc_h.result();
  T gamma = inv_beta - (T(2) - inv_beta) * sum_s / sum_h;
  if (gamma < T(1e-15)) gamma = T(2);
  if (gamma != gamma) gamma = T(2);
  const T bg = beta * gamma;
  const KbcS<T, S> dsc = ds.scaled(beta * (T(2) - gamma));
  static_for<S::Q>([&](auto qc) {
    constexpr int q = decltype(qc)::value;
    constexpr int sg = KbcS<T, S>::template sign<q>();
    const T x = f[q][k] - feq[q];
    const T y = fma_t(-bg, x, f[q][k]);
    const T m = dsc.template magnitude<q>();
    f[q][k] = sg == 0 ? y : (sg > 0 ? y - m : y + m);
  });
}

// Smagorinsky LES on top of BGK (lettuce/ext/_collision/smagorinsky_collision.py:19-36): the relaxation time of a
// node grows with the second moments of its non-equilibrium part,
//   Pi_ab = sum_q e_qa e_qb (f_q - feq_q),  S_shear = Pi / (2 rho cs^2),  nu = (tau - 1/2) / 3,
//   twice:  S = S_shear / tau_eff;  nu_t = C^2 (S : S);  tau_eff = 3 (nu + nu_t) + 1/2     (from tau_eff = tau),
// then f - (1 / tau_eff) (f - feq).  The contraction runs over all d x d components, so the off-diagonal ones count
// twice, and nu_t has no square root: the reference's model, kept as it is.  rho, u and feq are BGK's, bit for bit.
// The six distinct moments are raw sums over the opposite pairs (equal e_a e_b, as in kbc_s); S : S is formed as
// (Pi / D : Pi / D) / tau_eff^2 with one division by D = 2 rho cs^2 and one reciprocal per iteration, where the
// reference divides the d x d components each time: same value up to rounding, so -- like KBC -- this collision is
// compared with the reference at rounding level.  No contraction by the compiler (every kernel it is inlined into
// returns the same bits); the two multiply-adds of the iteration are written as fma_t.
// The Q differences f - feq stay in registers for the relaxation (the two-step kernel of D3Q19 fp32 fits its
// 168 VGPRs with them, without scratch: DESIGN.md section 4).
template <typename T, class S, int LAYOUT, int VEC, int k>
__device__ __forceinline__ void collide_smagorinsky(T (&f)[S::Q][VEC], T tau, T c2) {
#pragma clang fp contract(off)
  T rho, j[3], u[3];
  moments<T, S, LAYOUT, VEC, k>(f, rho, j);
  u[0] = j[0] / rho; u[1] = j[1] / rho; u[2] = j[2] / rho;
  const T uxu = square_norm<S, LAYOUT>(u);
  T x[S::Q];
  T pair[S::Q];                                   // [q], q < opposite(q): x_q + x_opposite
  for_each_feq<T, S, LAYOUT>(rho, u, uxu, [&](auto qc, T feq) {
    constexpr int q = decltype(qc)::value;
    constexpr int o = S::OPP[q];
    const T d = f[q][k] - feq;
    x[q] = d;
    if constexpr (q < o) pair[q] = d;             // (for_each_feq hands out q, then its opposite)
    else if constexpr (q > o) pair[o] = pair[o] + d;
  });
  T xx = T(0), yy = T(0), zz = T(0), xy = T(0), xz = T(0), yz = T(0);
  static_for<S::Q>([&](auto qc) {
    constexpr int q = decltype(qc)::value;
    if constexpr (q < S::OPP[q]) {
      constexpr int ex = S::E[q][0], ey = S::E[q][1], ez = S::E[q][2];
      const T v = pair[q];
      if constexpr (ex != 0) xx += v;
      if constexpr (ey != 0) yy += v;
      if constexpr (ez != 0) zz += v;
      if constexpr (ex * ey > 0) xy += v; else if constexpr (ex * ey < 0) xy -= v;
      if constexpr (ex * ez > 0) xz += v; else if constexpr (ex * ez < 0) xz -= v;
      if constexpr (ey * ez > 0) yz += v; else if constexpr (ey * ez < 0) yz -= v;
    }
  });
  const T inv_d = T(1) / (T(2) * rho * T(kCs2));
  xx = xx * inv_d;
  T ss = xx * xx;                                 // S_shear : S_shear
  if constexpr (S::D > 1) {
    yy = yy * inv_d; xy = xy * inv_d;
    ss = ss + yy * yy + T(2) * (xy * xy);
  }
  if constexpr (S::D > 2) {
    zz = zz * inv_d; xz = xz * inv_d; yz = yz * inv_d;
    ss = ss + zz * zz + T(2) * (xz * xz) + T(2) * (yz * yz);
  }
  const T nu = (tau - T(0.5)) / T(3);
  T r = T(1) / tau;                               // 1 / tau_eff
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const T nu_eff = fma_t(c2, ss * (r * r), nu);
    r = T(1) / fma_t(nu_eff, T(3), T(0.5));
  }
  static_for<S::Q>([&](auto qc) {
    constexpr int q = decltype(qc)::value;
    f[q][k] = f[q][k] - r * x[q];
  });
}

// Two relaxation times (lettuce/ext/_collision/trt_collision.py:16-27): the symmetric part of f - feq over an opposite
// pair relaxes with tau_plus (the `tau` of the call), the antisymmetric part with tau_minus,
//   sp = (f_q + f_o) - (feq_q + feq_o),  sm = (f_q - f_o) - (feq_q - feq_o),
//   f_q -= sp a + sm b,  f_o -= sp a - sm b,   a = 1 / (2 tau_plus), b = 1 / (2 tau_minus).
// The reference evaluates the expression of f_o on its own: its sp is the same sums with the operands swapped and its
// sm the exact negative, so one evaluation per pair returns both values as the reference's order of operations gives
// them.  The rest population has sm = 0.  rho, u and feq are BGK's, bit for bit.  The reference divides by 2.0 * tau
// where a and b are reciprocals formed once on the host in double: compared with the reference at rounding level.  No
// contraction by the compiler (every kernel this is inlined into returns the same bits).
template <typename T, class S, int LAYOUT, int VEC, int k, int EQ = 0>
__device__ __forceinline__ void collide_trt(T (&f)[S::Q][VEC], T a, T b, T rho0 = T(0)) {
#pragma clang fp contract(off)
  T rho, j[3], u[3];
  moments<T, S, LAYOUT, VEC, k>(f, rho, j);
  u[0] = j[0] / rho; u[1] = j[1] / rho; u[2] = j[2] / rho;
  const T uxu = square_norm<S, LAYOUT>(u);
  T held = T(0);                                  // feq_q while for_each_feq forms feq_o (it hands out q, then o)
  const auto relax = [&](auto qc, T feq) {
#pragma clang fp contract(off)
    constexpr int q = decltype(qc)::value;
    constexpr int o = S::OPP[q];
    if constexpr (q == o) {
      const T sp = (f[q][k] + f[q][k]) - (feq + feq);
      f[q][k] = f[q][k] - sp * a;
    } else if constexpr (q < o) {
      held = feq;
    } else {                                      // o < q: the pair (o, q) with feq_o held
      const T sp = (f[o][k] + f[q][k]) - (held + feq);
      const T sm = (f[o][k] - f[q][k]) - (held - feq);
      const T spa = sp * a, smb = sm * b;
      f[o][k] = f[o][k] - (spa + smb);
      f[q][k] = f[q][k] - (spa - smb);
    }
  };
  if constexpr (EQ == 0) for_each_feq<T, S, LAYOUT>(rho, u, uxu, relax);
  else for_each_feq_inc<T, S, LAYOUT>(rho, rho0, u, uxu, relax);
}

// Regularised collision of Latt and Chopard (lettuce/ext/_collision/regularized_collision.py:17-44): the
// non-equilibrium part is rebuilt from its second moments alone,
//   Pi_ab = sum_q e_qa e_qb (f_q - feq_q),
//   f_q = feq_q + (1 - 1 / tau) w_q / (2 cs^4) (sum_ab e_qa e_qb Pi_ab - cs^2 tr Pi),
// the contraction over all d x d components (the off-diagonal ones count twice).  Pi is summed over the opposite pairs
// as collide_smagorinsky sums it (the reference's is a GEMM over q), and `c` = 1 - 1 / tau is formed once on the host
// in double: compared with the reference at rounding level.  rho, u and feq are BGK's, bit for bit; the equilibria
// take the registers of f once the differences are summed, so nothing but the six moments is held beside them.  No
// contraction by the compiler; the one multiply-add per population is written as fma_t.
template <typename T, class S, int LAYOUT, int VEC, int k, int EQ = 0>
__device__ __forceinline__ void collide_regularized(T (&f)[S::Q][VEC], T c, T rho0 = T(0)) {
#pragma clang fp contract(off)
  T rho, j[3], u[3];
  moments<T, S, LAYOUT, VEC, k>(f, rho, j);
  u[0] = j[0] / rho; u[1] = j[1] / rho; u[2] = j[2] / rho;
  const T uxu = square_norm<S, LAYOUT>(u);
  T xx = T(0), yy = T(0), zz = T(0), xy = T(0), xz = T(0), yz = T(0);
  T first = T(0);                                 // f_q - feq_q while for_each_feq forms feq_o
  const auto moments_of = [&](auto qc, T feq) {
#pragma clang fp contract(off)
    constexpr int q = decltype(qc)::value;
    constexpr int o = S::OPP[q];
    const T d = f[q][k] - feq;
    f[q][k] = feq;
    if constexpr (q < o) {
      first = d;
    } else if constexpr (q > o) {                 // e_a e_b is the pair's
      constexpr int ex = S::E[q][0], ey = S::E[q][1], ez = S::E[q][2];
      const T v = first + d;
      if constexpr (ex != 0) xx += v;
      if constexpr (ey != 0) yy += v;
      if constexpr (ez != 0) zz += v;
      if constexpr (ex * ey > 0) xy += v; else if constexpr (ex * ey < 0) xy -= v;
      if constexpr (ex * ez > 0) xz += v; else if constexpr (ex * ez < 0) xz -= v;
      if constexpr (ey * ez > 0) yz += v; else if constexpr (ey * ez < 0) yz -= v;
    }
  };
  if constexpr (EQ == 0) for_each_feq<T, S, LAYOUT>(rho, u, uxu, moments_of);
  else for_each_feq_inc<T, S, LAYOUT>(rho, rho0, u, uxu, moments_of);
  T tr = xx;
  if constexpr (S::D > 1) tr = tr + yy;
  if constexpr (S::D > 2) tr = tr + zz;
  const T ctr = T(kCs2) * tr;
  const T xy2 = T(2) * xy, xz2 = T(2) * xz, yz2 = T(2) * yz;
  static_for<S::Q>([&](auto qc) {
    constexpr int q = decltype(qc)::value;
    constexpr int o = S::OPP[q];
    if constexpr (q <= o) {
      constexpr int ex = S::E[q][0], ey = S::E[q][1], ez = S::E[q][2];
      T t = T(0);
      if constexpr (ex != 0) t = t + xx;
      if constexpr (ey != 0) t = t + yy;
      if constexpr (ez != 0) t = t + zz;
      if constexpr (ex * ey > 0) t = t + xy2; else if constexpr (ex * ey < 0) t = t - xy2;
      if constexpr (ex * ez > 0) t = t + xz2; else if constexpr (ex * ez < 0) t = t - xz2;
      if constexpr (ey * ez > 0) t = t + yz2; else if constexpr (ey * ez < 0) t = t - yz2;
      const T g = c * (t - ctr);
      constexpr T wc = (T)(S::W[q] / (2.0 * kCs4));
      f[q][k] = fma_t(wc, g, f[q][k]);
      if constexpr (q < o) f[o][k] = fma_t(wc, g, f[o][k]);
    }
  });
}

// BGK (BASE 1) or Smagorinsky (BASE 3) with a uniform body force (lettuce/ext/_collision/bgk_collision.py:17-22,
// smagorinsky_collision.py:19-36, lettuce/ext/_force/guo.py:14-31, shan_chen.py:14-25):
//   u*   = j / rho + (ueq_scale a) / rho
//   f'_q = f_q - (1 / tau_eff) (f_q - feq_q(rho, u*))
//          + source_scale w_q sum_c [ (e_qc - u*_c) / cs^2 + (e_q . u*) e_qc / cs^4 ] a_c
// with tau_eff = tau (BGK) or the Smagorinsky relaxation time formed from f - feq(rho, u*) exactly as
// collide_smagorinsky forms it from f - feq(rho, u).  The sum over c is evaluated as
//   sum_c e_qc (a_c h_q) - (u* . a) / cs^2,   h_q = 1 / cs^2 + (e_q . u*) / cs^4,
// with u* . a formed once per node.  Every product has a per-node factor: a product of two launch constants (e_q . a,
// ueq_scale a -- the units form the latter) would be hoisted out of the two-step kernel's sweep into vector registers,
// one per population, and the sweep has none to spare.  Compared with the reference at rounding level.  No
// contraction by the compiler (every kernel this is inlined into returns the same bits); the multiply-adds of the
// source term are written as fma_t.
// accel, shift: the node's acceleration and ueq_scale times it along the memory axes -- KParamsF's arrays (uniform
// force), or the values a field kernel loaded for this node (NodeForce).  p: the block with tau_inv, tau, smag_c2 and
// source_scale (KParamsF, KParamsFI, KParamsFF)
template <typename T, class S, int LAYOUT, int VEC, int k, int BASE, int EQ = 0, class P>
__device__ __forceinline__ void collide_forced(T (&f)[S::Q][VEC], const P &p, const T (&accel)[3], const T (&shift)[3],
                                               T rho0 = T(0)) {
#pragma clang fp contract(off)
  static_assert(BASE == 1 || BASE == 3, "a body force exists for BGK and Smagorinsky");
  static_assert(EQ == 0 || BASE == 1, "the incompressible equilibrium exists under BGK with a force, not Smagorinsky");
  using M = MemMap<S, LAYOUT>;
  T rho, j[3], u[3];
  moments<T, S, LAYOUT, VEC, k>(f, rho, j);
  static_for<3>([&](auto mc) {
    constexpr int m = decltype(mc)::value;
    u[m] = j[m] / rho + shift[m] / rho;
  });
  const T uxu = square_norm<S, LAYOUT>(u);
  // u* . a over the logical axes
  T ua = u[M::memory(0)] * accel[M::memory(0)];
  if constexpr (S::D > 1) ua = ua + u[M::memory(1)] * accel[M::memory(1)];
  if constexpr (S::D > 2) ua = ua + u[M::memory(2)] * accel[M::memory(2)];
  constexpr T inv_cs2 = (T)(1.0 / kCs2), inv_cs4 = (T)(1.0 / kCs4);
  const T ua_cs2 = ua * inv_cs2;
  // relaxed = f_q - (1 / tau_eff) (f_q - feq_q)  ->  relaxed + source_q
  auto with_source = [&](auto qc, T relaxed) {
    constexpr int q = decltype(qc)::value;
    const T h = fma_t(dot_e<S, LAYOUT, q>(u), inv_cs4, inv_cs2);
    T t = -ua_cs2;
    static_for<S::D>([&](auto cc) {
      constexpr int c = decltype(cc)::value;
      constexpr int e = S::E[q][c];
      if constexpr (e > 0) t = fma_t(accel[M::memory(c)], h, t);
      else if constexpr (e < 0) t = fma_t(-accel[M::memory(c)], h, t);
    });
    return fma_t(p.source_scale, T(S::W[q]) * t, relaxed);
  };
  if constexpr (BASE == 1 && EQ == 1) {
    for_each_feq_inc<T, S, LAYOUT>(rho, rho0, u, uxu, [&](auto qc, T feq) {
      constexpr int q = decltype(qc)::value;
      f[q][k] = with_source(qc, f[q][k] - p.tau_inv * (f[q][k] - feq));
    });
  } else if constexpr (BASE == 1) {
    for_each_feq<T, S, LAYOUT>(rho, u, uxu, [&](auto qc, T feq) {
      constexpr int q = decltype(qc)::value;
      f[q][k] = with_source(qc, f[q][k] - p.tau_inv * (f[q][k] - feq));
    });
  } else {
    T x[S::Q];
    T pair[S::Q];                                 // [q], q < opposite(q): x_q + x_opposite
    for_each_feq<T, S, LAYOUT>(rho, u, uxu, [&](auto qc, T feq) {
      constexpr int q = decltype(qc)::value;
      constexpr int o = S::OPP[q];
      const T d = f[q][k] - feq;
      x[q] = d;
      if constexpr (q < o) pair[q] = d;
      else if constexpr (q > o) pair[o] = pair[o] + d;
    });
    T xx = T(0), yy = T(0), zz = T(0), xy = T(0), xz = T(0), yz = T(0);
    static_for<S::Q>([&](auto qc) {
      constexpr int q = decltype(qc)::value;
      if constexpr (q < S::OPP[q]) {
        constexpr int ex = S::E[q][0], ey = S::E[q][1], ez = S::E[q][2];
        const T v = pair[q];
        if constexpr (ex != 0) xx += v;
        if constexpr (ey != 0) yy += v;
        if constexpr (ez != 0) zz += v;
        if constexpr (ex * ey > 0) xy += v; else if constexpr (ex * ey < 0) xy -= v;
        if constexpr (ex * ez > 0) xz += v; else if constexpr (ex * ez < 0) xz -= v;
        if constexpr (ey * ez > 0) yz += v; else if constexpr (ey * ez < 0) yz -= v;
      }
    });
    const T inv_d = T(1) / (T(2) * rho * T(kCs2));
    xx = xx * inv_d;
    T ss = xx * xx;                               // S_shear : S_shear
    if constexpr (S::D > 1) {
      yy = yy * inv_d; xy = xy * inv_d;
      ss = ss + yy * yy + T(2) * (xy * xy);
    }
    if constexpr (S::D > 2) {
      zz = zz * inv_d; xz = xz * inv_d; yz = yz * inv_d;
      ss = ss + zz * zz + T(2) * (xz * xz) + T(2) * (yz * yz);
    }
    const T nu = (p.tau - T(0.5)) / T(3);
    T r = T(1) / p.tau;                           // 1 / tau_eff
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const T nu_eff = fma_t(p.smag_c2, ss * (r * r), nu);
      r = T(1) / fma_t(nu_eff, T(3), T(0.5));
    }
    static_for<S::Q>([&](auto qc) {
      constexpr int q = decltype(qc)::value;
      f[q][k] = with_source(qc, f[q][k] - r * x[q]);
    });
  }
}
// ... with the uniform acceleration of the block: what the kernels of lt_plan_set_force call
template <typename T, class S, int LAYOUT, int VEC, int k, int BASE, int EQ = 0>
__device__ __forceinline__ void collide_forced(T (&f)[S::Q][VEC], const KParamsF<T> &p, T rho0 = T(0)) {
  collide_forced<T, S, LAYOUT, VEC, k, BASE, EQ>(f, p, p.accel, p.shift, rho0);
}

// ---- boundaries -------------------------------------------------------------------------
// BounceBackBoundary: f <- f[opposite] (lettuce/ext/_boundary/bounce_back_boundary.py:17-18)
template <typename T, class S, int VEC, int k>
__device__ __forceinline__ void bounce_back(T (&f)[S::Q][VEC]) {
  static_for<S::Q>([&](auto qc) {
    constexpr int q = decltype(qc)::value;
    constexpr int o = S::OPP[q];
    if constexpr (q < o) {
      const T t = f[q][k];
      f[q][k] = f[o][k];
      f[o][k] = t;
    }
  });
}

// EquilibriumOutletP (lettuce/ext/_boundary/equilibrium_outlet_p.py:63-73) on one node of the outlet plane, given
// (rho, j) of the node next to it (neighbour_moments): ALL populations become feq(rho_outlet, u_n), u_n = j_n / rho_n
// -- the quadratic equilibrium of the collisions, bit for bit (for_each_feq; the reference's cs^2).  The outlet's axis
// does not enter: nothing of the node's own state survives, whichever way the plane faces.  No contraction by the
// compiler (every kernel this is inlined into returns the same bits).
template <typename T, class S, int LAYOUT, int VEC = 1, int k = 0>
__device__ __forceinline__ void pressure_outlet_apply(T rho_outlet, T rn, const T (&jn)[3], T (&f)[S::Q][VEC]) {
#pragma clang fp contract(off)
  T u[3];
  u[0] = jn[0] / rn; u[1] = jn[1] / rn; u[2] = jn[2] / rn;
  const T uxu = square_norm<S, LAYOUT>(u);
  for_each_feq<T, S, LAYOUT>(rho_outlet, u, uxu, [&](auto qc, T feq) { f[decltype(qc)::value][k] = feq; });
}

// What the boundaries with an index below `slot` do to (rho, j) of a node whose no_collision_mask index
// is b (collision conserves both): bounce-back negates j, an equilibrium boundary replaces the moments
// by those of its populations (neighbour_moments; also the two-step kernel's phase B).  A constant-pressure outlet
// (kPressureOutlet) does nothing here: it writes its plane, whatever the nodes' indices, and a node of that plane never
// reaches this function -- the kernels of such plans rebuild it in full (neighbour_moments, DEPTH) -- while a node that
// carries the outlet's index off its plane is left alone by the reference too (the in-place write, then a masked
// torch.where that changes nothing)
template <typename T, class S, int LAYOUT>
__device__ __forceinline__ void lower_boundaries_on_moments(const KParams<T> &p, int b, int slot, unsigned own,
                                                            T &rho, T (&j)[3]) {
  if (b > 0 && b < slot) {
    const int kind = p.bt->kind[b];
    if (kind == kBounceBack) {
      j[0] = -j[0]; j[1] = -j[1]; j[2] = -j[2];
    } else if (kind == kEquilibrium) {
      const T *fld = p.bt->field[b];
      rho = T(0); j[0] = j[1] = j[2] = T(0);
      static_for<S::Q>([&](auto qc) {
        constexpr int q = decltype(qc)::value;
        const T v = fld ? fld[(long long)q * p.N + own] : p.bt->feq[b][q];
        rho += v;
        add_momentum<S, LAYOUT, q>(j, v);
      });
    }
  }
}

// AntiBounceBackOutlet (lettuce/ext/_boundary/anti_bounce_back_outlet.py:72-91) on one node of the outlet
// plane, whose normal is memory axis AX, given (rho, j) of the node next to it (neighbour_moments, or the
// two-step kernels' saved / shuffled moments).  Only the populations leaving through the plane (e.n = +1)
// are read and only their opposites written, so nothing is computed for the others.  No FMA contraction
// here: the function is inlined into one-step and two-step kernels that must agree bit for bit, and which
// products the backend fuses depends on the surrounding code (the reference's CPU ops do not fuse either).
template <typename T, class S, int LAYOUT, int AX, int VEC = 1, int k = 0>
__device__ __forceinline__ void abb_apply_ax(int side, T rn, const T (&jn)[3], T (&f)[S::Q][VEC]) {
#pragma clang fp contract(off)
  using M = MemMap<S, LAYOUT>;
  T rho, j[3];
  moments<T, S, LAYOUT, VEC, k>(f, rho, j);
  T uw[3];
#pragma unroll
  for (int m = 0; m < 3; ++m) {
    const T u = j[m] / rho, un = jn[m] / rn;
    uw[m] = u + T(0.5) * (u - un);
  }
  const T nrm = sqrt(uw[0] * uw[0] + uw[1] * uw[1] + uw[2] * uw[2]) / T(kCs);
  const T nrm2 = nrm * nrm;
  static_for<S::Q>([&](auto qc) {
    constexpr int q = decltype(qc)::value;
    constexpr int en = AX < S::D ? M::e(q, AX) : 0;
    if constexpr (en != 0) {
      if (en * side == 1) {
        const T eu = dot_e<S, LAYOUT, q>(uw);
        f[S::OPP[q]][k] = -f[q][k] + T(S::W[q]) * rho * (T(2) + eu * eu / T(kCs4) - nrm2);
      }
    }
  });
}
// the same for the outlet with index `slot` of the plan
template <typename T, class S, int LAYOUT, int VEC, int k>
__device__ __forceinline__ void abb_apply(const KParams<T> &p, int slot, T rn, const T (&jn)[3],
                                          T (&f)[S::Q][VEC]) {
  const int ax = p.bt->mem_axis[slot], side = p.bt->side[slot];
  if (ax == 0) abb_apply_ax<T, S, LAYOUT, 0, VEC, k>(side, rn, jn, f);
  else if (ax == 1) abb_apply_ax<T, S, LAYOUT, 1, VEC, k>(side, rn, jn, f);
  else abb_apply_ax<T, S, LAYOUT, 2, VEC, k>(side, rn, jn, f);
}

// ---- the collision of a kernel ------------------------------------------------------------
// The collision with number COLL (dispatch.hpp, kColl*) on node k of f: the one place that says which function a
// number means and which fields of the parameter block P it reads.  smag_c2 is the collision's own scalar (unit.inc,
// params_of): Smagorinsky's squared constant, TRT's 1 / (2 tau_minus) beside beta = 1 / (2 tau_plus), the regularised
// collision's 1 - 1 / tau.  A body force and MRT read their own blocks (KParamsF, KParamsM).  kCollNone: nothing.
// nf: the node's acceleration and shift, for the two numbers with a force field only (load_node_force; KParamsFF).
template <typename T, class S, int LAYOUT, int VEC, int k, int COLL, class P>
__device__ __forceinline__ void collide_node(T (&f)[S::Q][VEC], const P &p, const NodeForce<T> *nf = nullptr) {
  if constexpr (COLL == kCollBgk) collide_bgk<T, S, LAYOUT, VEC, k>(f, p.tau_inv);
  if constexpr (COLL == kCollKbc) collide_kbc<T, S, LAYOUT, VEC, k>(f, p.beta, p.inv_beta);
  if constexpr (COLL == kCollSmagorinsky) collide_smagorinsky<T, S, LAYOUT, VEC, k>(f, p.tau, p.smag_c2);
  if constexpr (COLL == kCollTrt) collide_trt<T, S, LAYOUT, VEC, k>(f, p.beta, p.smag_c2);
  if constexpr (COLL == kCollRegularized) collide_regularized<T, S, LAYOUT, VEC, k>(f, p.smag_c2);
  if constexpr (coll_forced(COLL) && !coll_incompressible(COLL)) collide_forced<T, S, LAYOUT, VEC, k, coll_base(COLL)>(f, p);
  if constexpr (coll_field(COLL)) collide_forced<T, S, LAYOUT, VEC, k, coll_field_base(COLL)>(f, p, nf->accel, nf->shift);
  // ... with the incompressible equilibrium (KParamsI / KParamsFI: rho0)
  if constexpr (COLL == (kCollBgk | kCollIncompressible)) collide_bgk<T, S, LAYOUT, VEC, k, 1>(f, p.tau_inv, p.rho0);
  if constexpr (COLL == (kCollTrt | kCollIncompressible)) collide_trt<T, S, LAYOUT, VEC, k, 1>(f, p.beta, p.smag_c2, p.rho0);
  if constexpr (COLL == (kCollRegularized | kCollIncompressible)) collide_regularized<T, S, LAYOUT, VEC, k, 1>(f, p.smag_c2, p.rho0);
  if constexpr (COLL == (kCollBgk | kCollForce | kCollIncompressible)) collide_forced<T, S, LAYOUT, VEC, k, kCollBgk, 1>(f, p, p.rho0);
  if constexpr (coll_mrt(COLL)) collide_mrt<T, S, mrt_transform_of<S, COLL>(), LAYOUT, VEC, k>(f, p.r);
}

// The acceleration of node `own` from a plan's force field (KParamsFF) and its velocity shift: component c of the
// LOGICAL axes lies at c * N + own -- consecutive lanes, consecutive addresses -- and goes to the memory axis the layout
// gives it, as set_force (unit.inc) permutes the uniform acceleration.  The shift is the product the host forms for the
// uniform force, ueq_scale * a in T and not contracted into anything: a field that is constant in space gives the bits
// of the uniform kernels.  own < N for every node of a launch (the field has no ghost planes: reference layout only).
template <typename T, class S, int LAYOUT>
__device__ __forceinline__ void load_node_force(const KParamsFF<T> &p, unsigned own, NodeForce<T> &nf) {
#pragma clang fp contract(off)
  using M = MemMap<S, LAYOUT>;
  nf.accel[0] = nf.accel[1] = nf.accel[2] = T(0);
  nf.shift[0] = nf.shift[1] = nf.shift[2] = T(0);
  static_for<S::D>([&](auto cc) {
    constexpr int c = decltype(cc)::value;
    const T a = load<T>(p.accel_field + (long long)c * p.N + own);
    nf.accel[M::memory(c)] = a;
    nf.shift[M::memory(c)] = p.ueq_scale * a;
  });
}

// (rho, j) of the node (c0, c1, c2), as Flow.rho()/Flow.u() would see it when the AntiBounceBackOutlet with
// index `slot` is evaluated: after collision (which conserves both) and after the boundaries with a lower
// index (anti_bounce_back_outlet.py:77-80).  DEPTH = how many OTHER outlets with a lower index may touch
// this node (plans with several outlets whose planes meet in an edge): there the lower outlet has already
// rewritten some of this node's populations, so the node's state is rebuilt in full -- pull, collision,
// boundaries below `slot` in order, the lower outlet with ITS neighbour's moments at DEPTH - 1 -- instead
// of being read off the conserved moments.  DEPTH = 0 is the kernel of plans with one outlet.
// DEPTH = kOutletsP + chain: plans with a constant-pressure outlet, which asks for the same moments of its neighbour.
// Outlets of both kinds count as "lower outlets"; a node in a lower pressure outlet's plane has ALL its populations
// from that outlet, so a lower index of its own (b < slot) is not looked at twice: the rebuild walks the slots in order.
template <typename T, class S, int LAYOUT, bool STREAM, bool MASKED, int COLL = 0, int DEPTH = 0, class P = KParams<T>>
__device__ __forceinline__ void neighbour_moments(const P &p, int c0, int c1, int c2, int slot,
                                                  T &rho, T (&j)[3]) {
  const Coord c = make_coord(p, c0, c1, c2);
  T g[S::Q][1];
  gather<T, S, LAYOUT, STREAM>(p, c, g);
  const unsigned own = (unsigned)(c2 * p.n1 + c1) * (unsigned)p.n0 + (unsigned)c0;
  int b = 0;
  if constexpr (MASKED) {
    const unsigned char nd = p.node[own];
    b = nd & 0x7f;
    if constexpr (STREAM) {
      if (nd & 0x80) keep_unstreamed<T, S, 1, 0>(p, own, g);
    }
  }
  constexpr bool POUT = DEPTH >= kOutletsP;
  if constexpr ((DEPTH & (kOutletsP - 1)) > 0) {
    bool touched = false;                      // does an outlet with a lower index rewrite this node?
    for (int t = 1; t < slot; ++t)
      if (p.bt->kind[t] == kAbbOutlet || (POUT && p.bt->kind[t] == kPressureOutlet)) {
        const int ax = p.bt->mem_axis[t];
        touched = touched || (ax == 0 ? c0 : (ax == 1 ? c1 : c2)) == p.bt->plane[t];
      }
    if (touched) {
      if (b == 0) collide_node<T, S, LAYOUT, 1, 0, COLL>(g, p);
      for (int t = 1; t < slot; ++t) {
        const int kind = p.bt->kind[t];
        if (kind == kAbbOutlet || (POUT && kind == kPressureOutlet)) {
          const int ax = p.bt->mem_axis[t], nbr = p.bt->nbr[t];
          if ((ax == 0 ? c0 : (ax == 1 ? c1 : c2)) == p.bt->plane[t]) {
            T rn, jn[3];
            neighbour_moments<T, S, LAYOUT, STREAM, MASKED, COLL, DEPTH - 1>(
                p, ax == 0 ? nbr : c0, ax == 1 ? nbr : c1, ax == 2 ? nbr : c2, t, rn, jn);
            // (one call for both kinds: the chain is inlined once per level)
            if (POUT && kind == kPressureOutlet) pressure_outlet_apply<T, S, LAYOUT, 1, 0>(p.bt->rho_outlet[t], rn, jn, g);
            else abb_apply<T, S, LAYOUT, 1, 0>(p, t, rn, jn, g);
          }
        } else if (b == t) {
          if (kind == kBounceBack) {
            bounce_back<T, S, 1, 0>(g);
          } else if (kind == kEquilibrium) {
            const T *fld = p.bt->field[t];
            static_for<S::Q>([&](auto qc) {
              constexpr int q = decltype(qc)::value;
              g[q][0] = fld ? fld[(long long)q * p.N + own] : p.bt->feq[t][q];
            });
          }
        }
      }
      moments<T, S, LAYOUT, 1, 0>(g, rho, j);
      return;
    }
  }
  // a body force adds momentum in the collision (a per step with BGK; with Smagorinsky an amount that depends on the
  // node's tau_eff): the moments are those of the collided populations
  if constexpr (coll_incompressible(COLL)) {   // ... and so does the incompressible equilibrium (sum_q e_q feq_q = rho0 u)
    if (b == 0) collide_node<T, S, LAYOUT, 1, 0, COLL>(g, p);
  } else if constexpr ((COLL & 4) != 0) {
    if (b == 0) collide_forced<T, S, LAYOUT, 1, 0, (COLL & 3)>(g, p);
  }
  moments<T, S, LAYOUT, 1, 0>(g, rho, j);
  lower_boundaries_on_moments<T, S, LAYOUT>(p, b, slot, own, rho, j);
}

template <typename T, class S, int LAYOUT, bool STREAM, bool MASKED, int VEC, int k, int COLL = 0, int ABBD = 0,
          class P = KParams<T>>
__device__ __forceinline__ void abb_outlet(const P &p, int slot, int c0k, int c1,
                                           int c2, T (&f)[S::Q][VEC]) {
  const int ax = p.bt->mem_axis[slot], nbr = p.bt->nbr[slot];
  T rn, jn[3];
  neighbour_moments<T, S, LAYOUT, STREAM, MASKED, COLL, ABBD>(p, ax == 0 ? nbr : c0k, ax == 1 ? nbr : c1,
                                                               ax == 2 ? nbr : c2, slot, rn, jn);
  abb_apply<T, S, LAYOUT, VEC, k>(p, slot, rn, jn, f);
}

// The boundaries of one node in index order (lettuce/_simulation.py:183-188); b = the node's index in
// no_collision_mask, (c0k, c1, c2) its memory coordinates, ownk its index within a population.
// lane_slot != 0: (lane_rho, lane_j) are the moments of the node next to this one along a0 as outlet `lane_slot`
// sees them, handed over by the neighbouring lane (lbm_body) instead of being gathered again.
template <typename T, class S, int LAYOUT, bool STREAM, int VEC, int k, int COLL = 0, int ABBD = 0, class P = KParams<T>>
__device__ __forceinline__ void apply_boundaries(const P &p, int b, int c0k, int c1, int c2,
                                                 unsigned ownk, T (&f)[S::Q][VEC], int lane_slot = 0,
                                                 T lane_rho = T(1), const T *lane_j = nullptr) {
  for (int slot = 1; slot <= p.nb; ++slot) {
    const int kind = p.bt->kind[slot];
    if (kind == kAbbOutlet || (ABBD >= kOutletsP && kind == kPressureOutlet)) {
      // applies on the whole outlet plane, whatever the node's index: the reference
      // mutates flow.f in place and the masked torch.where is then a no-op
      // (anti_bounce_back_outlet.py:81-91, _simulation.py:186-188).  The constant-pressure outlet as well, for the same
      // reason (equilibrium_outlet_p.py:70-73): a bounce-back or inlet node of its plane has had its own boundary
      // applied at its (lower) index and is overwritten here
      // (no outlet on a plan with a force field: lt_plan_set_force_field refuses the pair, and its kernels hold no
      // gather of the neighbour)
      if constexpr (!coll_field(COLL)) {
      const int ax = p.bt->mem_axis[slot];
      const int coord = ax == 0 ? c0k : (ax == 1 ? c1 : c2);
      if (coord == p.bt->plane[slot]) {
        if (slot == lane_slot) {
          const T jn[3] = {lane_j[0], lane_j[1], lane_j[2]};
          abb_apply<T, S, LAYOUT, VEC, k>(p, slot, lane_rho, jn, f);
        } else if constexpr (ABBD >= kOutletsP) {
          // plans with a constant-pressure outlet: one gather of the neighbour serves both kinds
          const int nbr = p.bt->nbr[slot];
          T rn, jn[3];
          neighbour_moments<T, S, LAYOUT, STREAM, true, COLL, ABBD>(p, ax == 0 ? nbr : c0k, ax == 1 ? nbr : c1,
                                                                    ax == 2 ? nbr : c2, slot, rn, jn);
          if (kind == kPressureOutlet) pressure_outlet_apply<T, S, LAYOUT, VEC, k>(p.bt->rho_outlet[slot], rn, jn, f);
          else abb_apply<T, S, LAYOUT, VEC, k>(p, slot, rn, jn, f);
        } else {
          abb_outlet<T, S, LAYOUT, STREAM, true, VEC, k, COLL, ABBD>(p, slot, c0k, c1, c2, f);
        }
      }
      }
    } else if (b == slot) {
      if (kind == kBounceBack) {
        bounce_back<T, S, VEC, k>(f);
      } else if (kind == kEquilibrium) {
        const T *fld = p.bt->field[slot];
        static_for<S::Q>([&](auto qc) {
          constexpr int q = decltype(qc)::value;
          f[q][k] = fld ? fld[(long long)q * p.N + ownk] : p.bt->feq[slot][q];
        });
      }
    }
  }
}

// ---- the kernel ---------------------------------------------------------------------------
// TUNE bit 0: nontemporal loads, bit 1: nontemporal stores.  One thread per node, the grid
// covers the work exactly (a capped grid with a grid-stride loop measured 7 % slower and cost
// 20-30 VGPRs in the KBC kernels).
// number of populations q' < q with the same velocity component along memory axis a2
template <class S, int LAYOUT, int q>
constexpr int crossing_rank() {
  int r = 0;
  for (int k = 0; k < q; ++k)
    if (MemMap<S, LAYOUT>::e(k, 2) == MemMap<S, LAYOUT>::e(q, 2)) ++r;
  return r;
}

// ABBD: plans with ABBD + 1 anti-bounce-back outlets (neighbour_moments, DEPTH); kOutletsP + chain: plans with a
// constant-pressure outlet (no lane hand-over there: every such outlet gathers its neighbour)
template <typename T, class S, int LAYOUT, int COLL, bool STREAM, bool COLLIDE, bool MASKED,
          int TUNE = 0, bool PACK = false, int ABBD = 0, class P = KParams<T>>
__device__ __forceinline__ void lbm_body(const P &p) {
  const unsigned v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= p.nvec_total) return;
  {
  const unsigned rowid = v / (unsigned)p.nv0;
  const int c0 = (int)(v - rowid * (unsigned)p.nv0);
  const int r2 = (int)(rowid / (unsigned)p.n1);
  const int c1 = (int)(rowid - (unsigned)r2 * (unsigned)p.n1);
  const int c2 = p.p_begin + r2 * p.p_stride;
  const Coord c = make_coord(p, c0, c1, c2);
  const unsigned own = (unsigned)(c2 * p.n1 + c1) * (unsigned)p.n0 + (unsigned)c0;

  T f[S::Q][1];
  gather<T, S, LAYOUT, STREAM, (TUNE & 1) != 0>(p, c, f);
  // a force field: the node's acceleration, D coalesced loads issued with the gather's (a boundary node loads its
  // values too and does not use them: the field is dense, and the loads need not wait for the node's byte)
  [[maybe_unused]] NodeForce<T> nf;
  if constexpr (COLLIDE && coll_field(COLL)) load_node_force<T, S, LAYOUT>(p, own, nf);

  unsigned char nd;
  if constexpr (MASKED) {
    nd = p.node[own];
    if constexpr (STREAM) {
      if (nd & 0x80) keep_unstreamed<T, S, 1, 0>(p, own, f);
    }
  }

  // An outlet whose normal is the contiguous axis: the node next to an outlet node is held by the next lane of
  // the same wave (rows are whole waves), whose populations at this point -- pulled, no-streaming slots kept,
  // not yet collided -- are exactly what neighbour_moments would gather again (19-27 single-lane loads and
  // their latency in every wave that ends a row: 0.48 -> 0.60 ms at 512 x 512 x 64 with the Obstacle's outlet)
  int lane_slot = 0;
  T lane_rho = T(1), lane_j[3] = {T(0), T(0), T(0)};
  // (not with a body force: the neighbour's collision changes its momentum -- neighbour_moments collides it)
  // (nor with the incompressible equilibrium, for the same reason)
  if constexpr (COLLIDE && MASKED && ABBD == 0 && (COLL & 4) == 0 && !coll_incompressible(COLL)) {   // (COLL 8 and 9 conserve rho and j, as 1-3 do)
    if (p.abb0_slot != 0) {
      const int slot = p.abb0_slot, plane = p.bt->plane[slot];
      const int lane = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
      const int first = c0 - lane;                                 // a0 coordinate of lane 0: same in all lanes
      if (plane >= first && plane < first + 64) {
        moments<T, S, LAYOUT, 1, 0>(f, lane_rho, lane_j);
        lower_boundaries_on_moments<T, S, LAYOUT>(p, nd & 0x7f, slot, own, lane_rho, lane_j);
        const int from = (lane - p.bt->side[slot]) & 63;
        lane_rho = __shfl(lane_rho, from);
        lane_j[0] = __shfl(lane_j[0], from); lane_j[1] = __shfl(lane_j[1], from); lane_j[2] = __shfl(lane_j[2], from);
        lane_slot = slot;
      }
    }
  }

  if constexpr (COLLIDE) {
    // (a lambda, as the former loop over a thread's nodes was: inlined in that order, the masked kernels keep their
    // register allocation)
    [&] {
      int b = 0;
      if constexpr (MASKED) b = nd & 0x7f;
      if constexpr (coll_field(COLL)) {
        if (b == 0) collide_node<T, S, LAYOUT, 1, 0, COLL>(f, p, &nf);
      } else {
        if (b == 0) collide_node<T, S, LAYOUT, 1, 0, COLL>(f, p);
      }
      if constexpr (MASKED)
        apply_boundaries<T, S, LAYOUT, STREAM, 1, 0, COLL, ABBD>(p, b, c0, c1, c2, own, f, lane_slot, lane_rho, lane_j);
    }();
  }

  static_for<S::Q>([&](auto qc) {
    constexpr int q = decltype(qc)::value;
    store<T, (TUNE & 2) != 0>(p.out + (long long)q * p.No + own, f[q][0]);
  });
  if constexpr (PACK) {
    // halo packing fused into the boundary-plane launch of the slab driver (saves two pack
    // launches on the critical path of the exchange)
    using M = MemMap<S, LAYOUT>;
    const unsigned in_plane = (unsigned)c1 * (unsigned)p.n0 + (unsigned)c0;
    const unsigned plane_nodes = (unsigned)p.n1 * (unsigned)p.n0;
    static_for<S::Q>([&](auto qc) {
      constexpr int q = decltype(qc)::value;
      constexpr int e2 = M::e(q, 2);
      if constexpr (e2 != 0) {
        constexpr int rank = crossing_rank<S, LAYOUT, q>();
        T *buf = e2 < 0 ? p.pack_lo : p.pack_hi;
        const int plane = e2 < 0 ? p.pack_lo_plane : p.pack_hi_plane;
        if (c2 == plane) store<T>(buf + (size_t)rank * plane_nodes + in_plane, f[q][0]);
      }
    });
  }
  }
}

// VEC (nodes per thread) and SHIFT (how a 16-byte access resolves the a0 shift) name variants that lost their A/B
// (DESIGN.md section 4); they stay in the signature because kernel names and profiles are keyed on them
template <typename T, class S, int LAYOUT, int COLL, bool STREAM, bool COLLIDE, bool MASKED,
          int VEC, int SHIFT, int TUNE = 0, bool PACK = false, int ABBD = 0>
__global__ void __launch_bounds__(kThreads) lbm_kernel(const KParams<T> p) {
  static_assert(VEC == 1 && SHIFT == 0, "one node per thread");
  lbm_body<T, S, LAYOUT, COLL, STREAM, COLLIDE, MASKED, TUNE, PACK, ABBD>(p);
}

// ... with a body force (COLL = 4 + the collision): the same body on KParamsF
template <typename T, class S, int LAYOUT, int COLL, bool STREAM, bool COLLIDE, bool MASKED,
          int VEC, int SHIFT, int TUNE = 0, bool PACK = false, int ABBD = 0>
__global__ void __launch_bounds__(kThreads) lbm_kernel(const KParamsF<T> p) {
  static_assert(VEC == 1 && SHIFT == 0, "one node per thread");
  static_assert(coll_forced(COLL), "a body force exists for BGK (5) and Smagorinsky (7)");
  lbm_body<T, S, LAYOUT, COLL, STREAM, COLLIDE, MASKED, TUNE, PACK, ABBD>(p);
}

// ... with a body force whose acceleration is a per-node field (COLL = 36 + the collision: 37, 39): the same body on
// KParamsFF.  One-step kernels of the reference layout, no outlet depth, no packing (unit.inc, part force_field)
template <typename T, class S, int LAYOUT, int COLL, bool STREAM, bool COLLIDE, bool MASKED,
          int VEC, int SHIFT, int TUNE = 0, bool PACK = false, int ABBD = 0>
__global__ void __launch_bounds__(kThreads) lbm_kernel(const KParamsFF<T> p) {
  static_assert(VEC == 1 && SHIFT == 0, "one node per thread");
  static_assert(coll_field(COLL) && LAYOUT == 0 && !PACK && ABBD == 0,
                "a force field exists for BGK (37) and Smagorinsky (39), reference layout, plans without outlets");
  lbm_body<T, S, LAYOUT, COLL, STREAM, COLLIDE, MASKED, TUNE, PACK, ABBD>(p);
}

// ... with the multiple-relaxation-time collision (COLL 10: Dellar on D2Q9, Hermite on D3Q27; 11: Lallemand): the same
// body on KParamsM
template <typename T, class S, int LAYOUT, int COLL, bool STREAM, bool COLLIDE, bool MASKED,
          int VEC, int SHIFT, int TUNE = 0, bool PACK = false, int ABBD = 0>
__global__ void __launch_bounds__(kThreads) lbm_kernel(const KParamsM<T> p) {
  static_assert(VEC == 1 && SHIFT == 0, "one node per thread");
  static_assert(coll_mrt(COLL), "MRT is collision 10 (Dellar / Hermite) or 11 (Lallemand)");
  lbm_body<T, S, LAYOUT, COLL, STREAM, COLLIDE, MASKED, TUNE, PACK, ABBD>(p);
}

// ... with the incompressible equilibrium (COLL = 16 + the collision: BGK 17, BGK with a body force 21, TRT 24, the
// regularised collision 25): the same body on KParamsI / KParamsFI
template <typename T, class S, int LAYOUT, int COLL, bool STREAM, bool COLLIDE, bool MASKED,
          int VEC, int SHIFT, int TUNE = 0, bool PACK = false, int ABBD = 0>
__global__ void __launch_bounds__(kThreads) lbm_kernel(const KParamsI<T> p) {
  static_assert(VEC == 1 && SHIFT == 0, "one node per thread");
  static_assert(coll_incompressible(COLL) && !coll_forced(COLL), "the incompressible equilibrium is COLL & 16");
  lbm_body<T, S, LAYOUT, COLL, STREAM, COLLIDE, MASKED, TUNE, PACK, ABBD>(p);
}
template <typename T, class S, int LAYOUT, int COLL, bool STREAM, bool COLLIDE, bool MASKED,
          int VEC, int SHIFT, int TUNE = 0, bool PACK = false, int ABBD = 0>
__global__ void __launch_bounds__(kThreads) lbm_kernel(const KParamsFI<T> p) {
  static_assert(VEC == 1 && SHIFT == 0, "one node per thread");
  static_assert(coll_incompressible(COLL) && coll_forced(COLL), "BGK with a body force and the incompressible equilibrium is COLL 21");
  lbm_body<T, S, LAYOUT, COLL, STREAM, COLLIDE, MASKED, TUNE, PACK, ABBD>(p);
}

// same kernel with the register allocator told to fit 4 waves per SIMD (<= 128 VGPRs): the masked
// D3Q27-KBC kernel sits at 131 VGPRs otherwise and loses a wave per SIMD (cfg4: 0.735 -> ms below)
template <typename T, class S, int LAYOUT, int COLL, bool STREAM, bool COLLIDE, bool MASKED,
          int VEC, int SHIFT, int TUNE = 0, bool PACK = false>
__global__ void __launch_bounds__(kThreads, 4) lbm_kernel_occ4(const KParams<T> p) {
  static_assert(VEC == 1 && SHIFT == 0, "one node per thread");
  lbm_body<T, S, LAYOUT, COLL, STREAM, COLLIDE, MASKED, TUNE, PACK>(p);
}

// ---- two fused steps per launch (periodic, no masks) -----------------------------------------
// f*_out = (C S)^2 f*_in with the intermediate state held in LDS, so that HBM sees one read and one
// write of the populations per TWO lattice updates.  A workgroup owns a T0 x T1 column of nodes in
// (a0, a1) and sweeps seg_len planes along a2:
//   phase A(j):   every thread pulls one node of the (T0+2) x (T1+2) halo'd tile of plane j from
//                 global memory, collides it and writes its populations to LDS;
//   phase B(k):   the first T0*T1 threads pull their node of plane k from the LDS planes k-1, k,
//                 k+1, collide and store to global memory.
// B(k) reads the populations moving up (e2 = +1, "U") only from plane k-1, the in-plane ones ("C")
// only from plane k and those moving down ("D") only from plane k+1.  With 4 LDS slots for U, 3 for
// C and 2 for D -- 57 population planes, as many as three whole planes -- A(k+2) can write while
// other waves still read for B(k), and ONE barrier per plane is enough:
//   barrier; issue the LDS reads of B(k); collide A(k+2) -> LDS (the reads fly behind it); issue
//   the global loads of A(k+3) (they land during the next plane); collide B(k); store B(k).
// The barrier waits for LDS traffic only (an ordinary __syncthreads() would drain the prefetch); the
// loads are issued as early as the registers allow and before the stores, so that the vmcnt waits
// in front of the next A never meet stores issued just before them.  The order was found by
// measurement: each of these placements is worth 3-10 %.
// Arithmetic per node is the one-step kernel's (same pull, same collide): results are bit for bit
// those of two lbm_kernel launches.  Redundant work: (T0+2)(T1+2)/(T0 T1) in the first step and
// two extra planes per segment.  HBM traffic (PMC, 256^3): reads 1.05x one pass, writes 1.00x.
// PACK: slab edge launches that also write the halo message.
// The tile geometry (TwoStep<T, S, T0, T1>) and its LDS footprint: launch_limits.hpp.

__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// MODE (slab layout): 0 = plain sweep; 1 = edge launch: every workgroup also writes the halo messages, and the
// planes beyond the cuts are read from the receive buffers when p.ghost_lo / p.ghost_hi are given; 2 = launch
// over the whole slab whose edge workgroups start first and count themselves done (p.signal).
// NPT / NPB: intermediate / output nodes per thread.  Two of either lost their A/B; they stay
// in the signature because kernel names and profiles are keyed on them.
// SCHED (plain sweep): 0 = every wave runs both phases; 1 = producer waves run phase A, consumer waves phase B
// (twostep_roles.hpp).
template <typename T, class S, int LAYOUT, int COLL, int T0_, int T1, int NPT = 1, int MODE = 0,
          int NPB = NPT, int SCHED = 0>
__global__ void __launch_bounds__((SCHED == 0 ? (TwoStep<T, S, T0_, T1>::NI / NPT + 63) / 64 * 64
                                              : RoleWaves<TwoStep<T, S, T0_, T1>::NI, TwoStep<T, S, T0_, T1>::NO>::THREADS))
lbm2_kernel(const KParams<T> p, const int seg_len) {
  static_assert(!coll_forced(COLL), "kernels with a body force take KParamsF");
#include "twostep_sweep.inc"
}

// ... with a body force (COLL = 4 + the collision): the plain one-role sweep on KParamsF.  The sweep is one text
// (twostep_sweep.inc) in both kernels rather than a function both call: inlined from a function the unforced kernels
// came out with another register allocation (156 -> 162 VGPRs for the BGK sweep of D3Q19 fp32), and they are to stay
// instruction for instruction what they were.
template <typename T, class S, int LAYOUT, int COLL, int T0_, int T1, int NPT = 1, int MODE = 0,
          int NPB = NPT, int SCHED = 0>
__global__ void __launch_bounds__((TwoStep<T, S, T0_, T1>::NI / NPT + 63) / 64 * 64)
lbm2_kernel(const KParamsF<T> p, const int seg_len) {
  static_assert(coll_forced(COLL), "a body force exists for BGK (5) and Smagorinsky (7)");
#include "twostep_sweep.inc"
}

// One wave on the communication stream: returns when *counter has reached `target` (the edge workgroups of
// the launch running on the compute stream have stored the planes next to the cuts), or after about a second, setting
// *timed_out -- an exit every launch reaches.  17 us from the last increment to the next kernel of the stream
// (tools/experiments/stream_wait.hip; hipStreamWaitValue64 needs signal memory, where 256 device atomics
// drained in 280 us).
static __global__ void wait_counter_kernel(const unsigned long long *counter, unsigned long long target,
                                           unsigned *timed_out) {
  // relaxed polls (one uncached load each): an ACQUIRE per poll would invalidate this XCD's L2 every
  // microsecond under the sweep that runs beside it -- measured 0.63 instead of 0.37 ms per step
  const long long t0 = wall_clock64();
  while (__hip_atomic_load(counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
    __builtin_amdgcn_s_sleep(127);
    if (wall_clock64() - t0 > 100000000ll) {           // 100 MHz
      *timed_out = 1u;
      break;
    }
  }
  __atomic_thread_fence(__ATOMIC_ACQUIRE);
}

// ---- up to KMAX steps per launch on small 2-D grids ---------------------------------------------
// A 128^2 grid is launch-bound (3.5 us per step against < 1 us of work).  Here a workgroup loads the
// (TO0 + 2(K-1)) x (TO1 + 2(K-1)) neighbourhood of its TO0 x TO1 tile, performs K stream-collide
// steps on it in LDS (two buffers, one __syncthreads per step; after step s only the nodes at
// distance >= s-1 from the border of the neighbourhood are still valid, after step K exactly the
// tile) and stores the tile.  The neighbourhood is recomputed by every workgroup that needs it --
// free while the GPU waits for launches, which is why lt_run only uses this on small grids.
// Same pull and same collide as the one-step kernel: K launches of lbm_kernel give the same bits.
template <int TO0, int TO1, int KMAX>
struct ManyStep2D {
  static constexpr int R0 = TO0 + 2 * (KMAX - 1), R1 = TO1 + 2 * (KMAX - 1);
  static constexpr int NR = R0 * R1;
  static constexpr int THREADS = (NR + 63) / 64 * 64;
};

// MASKED: plans with boundaries.  A thread keeps its node for all K steps, so the node byte, the no-streaming
// bits and -- on an equilibrium node -- the populations the boundary writes are fetched once.  A slot with a
// no-streaming bit keeps the node's own value of the step before (global memory in step 1, the LDS buffer
// afterwards).  The anti-bounce-back outlet needs (rho, j) of the node next to it as the one-step kernel sees
// them: the moments of that node's pulled populations, which are rebuilt from the same source as the thread's
// own pull (neighbour_moments in step 1, the LDS buffer afterwards).  That neighbour must itself be valid, so
// plans with an outlet recompute one more ring (halo = K instead of K - 1: at most KMAX - 1 steps per launch).
// Same functions in the same order as lbm_body: K launches of the masked lbm_kernel give the same bits.
template <typename T, class S, int COLL, int TO0, int TO1, int KMAX, bool MASKED = false>
__global__ void __launch_bounds__((ManyStep2D<TO0, TO1, KMAX>::THREADS))
lbm_many_kernel(const KParams<T> p, const int K) {
  static_assert(S::D == 2, "2-D lattices");
  using M = MemMap<S, 0>;
  using G = ManyStep2D<TO0, TO1, KMAX>;
  __shared__ T lds[2][S::Q][G::NR];
  const int tid = threadIdx.x;
  const int halo = K - 1 + (MASKED ? p.abb0_slot : 0);        // abb0_slot: 1 = the plan has an outlet
  const int r0 = TO0 + 2 * halo, r1 = TO1 + 2 * halo;        // neighbourhood of this launch
  const int tiles0 = p.n0 / TO0;
  const int t0 = (blockIdx.x % tiles0) * TO0, t1 = (blockIdx.x / tiles0) * TO1;
  const bool in_region = tid < r0 * r1;
  const int i1 = tid / r0, i0 = tid - i1 * r0;
  auto wrap = [](int x, int n) { x %= n; return x < 0 ? x + n : x; };
  const int g0 = wrap(t0 - halo + i0, p.n0), g1 = wrap(t1 - halo + i1, p.n1);
  const unsigned own = (unsigned)g1 * (unsigned)p.n0 + (unsigned)g0;
  auto collide = [&](T (&f)[S::Q][1]) { collide_node<T, S, 0, 1, 0, COLL>(f, p); };
  // ---- boundaries (MASKED) ----
  int bidx = 0;
  unsigned bits = 0;
  T eqv[S::Q];                                          // what this node's equilibrium boundary writes
  if constexpr (MASKED) {
    if (in_region) {
      const unsigned char nd = p.node[own];
      bidx = nd & 0x7f;
      if (nd & 0x80) bits = p.nsm_bits[own];
      if (bidx != 0 && p.bt->kind[bidx] == kEquilibrium) {
        const T *fld = p.bt->field[bidx];
        static_for<S::Q>([&](auto qc) {
          constexpr int q = decltype(qc)::value;
          eqv[q] = fld ? fld[(long long)q * p.N + own] : p.bt->feq[bidx][q];
        });
      }
    }
  }
  // What the boundaries do to this node is the same in every step: its own boundary (bounce-back / equilibrium,
  // index bidx) and, on the outlet's plane, the outlet (index out_slot) -- in index order.  Everything the
  // plan's table says about them is fetched once; for an outlet node also the index, node byte and
  // no-streaming bits of the node next to it.
  int my_kind = 0, out_slot = 0, out_axis = 0, out_side = 1;
  unsigned nown = 0, nbits = 0;
  int nbidx = 0;
  if constexpr (MASKED) {
    if (in_region) {
      if (bidx != 0) my_kind = p.bt->kind[bidx];
      if (p.abb0_slot) {
        for (int slot = 1; slot <= p.nb; ++slot)
          if (p.bt->kind[slot] == kAbbOutlet) {
            const int ax = p.bt->mem_axis[slot];
            if ((ax == 0 ? g0 : g1) == p.bt->plane[slot]) {
              out_slot = slot; out_axis = ax; out_side = p.bt->side[slot];
              const int ng0 = ax == 0 ? p.bt->nbr[slot] : g0, ng1 = ax == 1 ? p.bt->nbr[slot] : g1;
              nown = (unsigned)ng1 * (unsigned)p.n0 + (unsigned)ng0;
              const unsigned char nnd = p.node[nown];
              nbidx = nnd & 0x7f;
              nbits = (nnd & 0x80) ? p.nsm_bits[nown] : 0u;
            }
          }
      }
    }
  }
  // collision and the boundaries in index order; nbr(rho, j): moments of the node next to an outlet node
  auto collide_and_bound = [&](T (&f)[S::Q][1], auto &&nbr) {
    if constexpr (!MASKED) {
      collide(f);
    } else {
      if (bidx == 0) collide(f);
      auto outlet = [&]() {
        T rn, jn[3];
        nbr(rn, jn);
        if (out_axis == 0) abb_apply_ax<T, S, 0, 0>(out_side, rn, jn, f);
        else abb_apply_ax<T, S, 0, 1>(out_side, rn, jn, f);
      };
      // the outlet rewrites its whole plane, whatever the node's own index (apply_boundaries)
      if (out_slot != 0 && (bidx == 0 || out_slot <= bidx)) outlet();
      if (my_kind == kBounceBack) {
        bounce_back<T, S, 1, 0>(f);
      } else if (my_kind == kEquilibrium) {
        static_for<S::Q>([&](auto qc) { f[decltype(qc)::value][0] = eqv[decltype(qc)::value]; });
      }
      if (out_slot != 0 && bidx != 0 && out_slot > bidx) outlet();
    }
  };
  T f[S::Q][1];
  // step 1: pull from global memory, every node of the neighbourhood
  if (in_region) {
    static_for<S::Q>([&](auto qc) {
      constexpr int q = decltype(qc)::value;
      constexpr int e0 = M::e(q, 0), e1 = M::e(q, 1);
      const int s0 = e0 == 0 ? g0 : wrap(g0 - e0, p.n0), s1 = e1 == 0 ? g1 : wrap(g1 - e1, p.n1);
      f[q][0] = p.in[(long long)q * p.Ni + (long long)s1 * p.n0 + s0];
      if constexpr (MASKED && q > 0) {
        if (bits & (1u << q)) f[q][0] = p.in[(long long)q * p.Ni + own];
      }
    });
    collide_and_bound(f, [&](T &rn, T (&jn)[3]) {
      const int nb = p.bt->nbr[out_slot];
      neighbour_moments<T, S, 0, true, true, COLL, 0>(p, out_axis == 0 ? nb : g0, out_axis == 1 ? nb : g1, 0, out_slot,
                                                     rn, jn);
    });
  }
  for (int s = 1; s < K; ++s) {                 // f holds the state after step s
    const int buf = s & 1;
    if (in_region) {
      static_for<S::Q>([&](auto qc) {
        constexpr int q = decltype(qc)::value;
        lds[buf][q][i1 * G::R0 + i0] = f[q][0];
      });
    }
    __syncthreads();
    // step s + 1 is valid for nodes at distance >= s from the border
    const bool valid = in_region && i0 >= s && i0 < r0 - s && i1 >= s && i1 < r1 - s;
    if (valid) {
      static_for<S::Q>([&](auto qc) {
        constexpr int q = decltype(qc)::value;
        constexpr int e0 = M::e(q, 0), e1 = M::e(q, 1);
        f[q][0] = lds[buf][q][(i1 - e1) * G::R0 + (i0 - e0)];
        if constexpr (MASKED && q > 0) {
          if (bits & (1u << q)) f[q][0] = lds[buf][q][i1 * G::R0 + i0];
        }
      });
      collide_and_bound(f, [&](T &rn, T (&jn)[3]) {
        // the node next to this outlet node, inside the domain: its pull from the same LDS state
        const int n0i = out_axis == 0 ? i0 - out_side : i0, n1i = out_axis == 1 ? i1 - out_side : i1;
        T g[S::Q][1];
        static_for<S::Q>([&](auto qc) {
          constexpr int q = decltype(qc)::value;
          constexpr int e0 = M::e(q, 0), e1 = M::e(q, 1);
          g[q][0] = lds[buf][q][(n1i - e1) * G::R0 + (n0i - e0)];
          if constexpr (q > 0) {
            if (nbits & (1u << q)) g[q][0] = lds[buf][q][n1i * G::R0 + n0i];
          }
        });
        moments<T, S, 0, 1, 0>(g, rn, jn);
        lower_boundaries_on_moments<T, S, 0>(p, nbidx, out_slot, nown, rn, jn);
      });
    }
  }
  // after K steps the valid nodes are the tile
  if (in_region && i0 >= halo && i0 < r0 - halo && i1 >= halo && i1 < r1 - halo) {
    static_for<S::Q>([&](auto qc) {
      constexpr int q = decltype(qc)::value;
      p.out[(long long)q * p.No + own] = f[q][0];
    });
  }
}

// ---- auxiliary kernels --------------------------------------------------------------------
// rho [N], u [d][N] (logical axis order; u_stride elements between components) from f  -- Flow.rho / Flow.u
template <typename T, class S, int LAYOUT>
__global__ void __launch_bounds__(kThreads) macroscopic_kernel(const T *__restrict__ f,
                                                               T *__restrict__ rho_out,
                                                               T *__restrict__ u_out,
                                                               long long N, long long stride,
                                                               long long u_stride) {
  using M = MemMap<S, LAYOUT>;
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= N) return;
  T g[S::Q][1];
  static_for<S::Q>([&](auto qc) {
    constexpr int q = decltype(qc)::value;
    g[q][0] = f[(long long)q * stride + i];
  });
  T rho, j[3];
  moments<T, S, LAYOUT, 1, 0>(g, rho, j);
  if (rho_out) rho_out[i] = rho;
  if (u_out) {
#pragma unroll
    for (int a = 0; a < S::D; ++a) u_out[(long long)a * u_stride + i] = j[M::memory(a)] / rho;
  }
}

// feq [q][N] from rho [N], u [d][N]  -- QuadraticEquilibrium.__call__
template <typename T, class S, int LAYOUT>
__global__ void __launch_bounds__(kThreads) equilibrium_kernel(const T *__restrict__ rho_in,
                                                               const T *__restrict__ u_in,
                                                               T *__restrict__ feq_out,
                                                               long long N) {
  using M = MemMap<S, LAYOUT>;
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= N) return;
  const T rho = rho_in[i];
  T u[3] = {T(0), T(0), T(0)};
#pragma unroll
  for (int a = 0; a < S::D; ++a) u[M::memory(a)] = u_in[(long long)a * N + i];
  const T uxu = square_norm<S, LAYOUT>(u);
  for_each_feq<T, S, LAYOUT>(rho, u, uxu, [&](auto qc, T v) {
    feq_out[(long long)decltype(qc)::value * N + i] = v;
  });
}

// ... and IncompressibleQuadraticEquilibrium.__call__ (rho0 in the plan's scalar type)
template <typename T, class S, int LAYOUT>
__global__ void __launch_bounds__(kThreads) equilibrium_inc_kernel(const T *__restrict__ rho_in,
                                                                   const T *__restrict__ u_in,
                                                                   T *__restrict__ feq_out,
                                                                   long long N, T rho0) {
  using M = MemMap<S, LAYOUT>;
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= N) return;
  const T rho = rho_in[i];
  T u[3] = {T(0), T(0), T(0)};
#pragma unroll
  for (int a = 0; a < S::D; ++a) u[M::memory(a)] = u_in[(long long)a * N + i];
  const T uxu = square_norm<S, LAYOUT>(u);
  for_each_feq_inc<T, S, LAYOUT>(rho, rho0, u, uxu, [&](auto qc, T v) {
    feq_out[(long long)decltype(qc)::value * N + i] = v;
  });
}

// periodic index of a shifted coordinate: a modulo n in [0, n) for every extent n >= 1 and any shift, as
// torch.roll wraps (an extent of 1 or 2 is smaller than the stencil's reach of 3)
__device__ __forceinline__ int wrap_index(int a, int n) {
  a %= n;
  return a < 0 ? a + n : a;
}

// f = feq(rho, u) - w_q Pi1:Q_q  -- initialize_f_neq (lettuce/_flow.py:309-336), reference layout,
// periodic.  S[a][b] = d u_a / d x_b: torch_gradient's 6th-order central differences (dx = 1), term
// order of the reference's expression; Pi1 = ((1.0 tau) rho) S / cs^2; Q_q,ab = e_qa e_qb - eye_cs2 d_ab.
template <typename T, class S>
__global__ void __launch_bounds__(kThreads) fneq_kernel(const T *__restrict__ rho_in, const T *__restrict__ u_in,
                                                       T *__restrict__ f_out, int n0, int n1, int n2, T tau,
                                                       T eye_cs2) {
#define LT_FNEQ_FOR_EACH_FEQ for_each_feq<T, S, 0>(rho, u, uxu,
#include "fneq_body.inc"
#undef LT_FNEQ_FOR_EACH_FEQ
}
// ... with the incompressible equilibrium (rho0 in the plan's scalar type)
template <typename T, class S>
__global__ void __launch_bounds__(kThreads) fneq_inc_kernel(const T *__restrict__ rho_in, const T *__restrict__ u_in,
                                                           T *__restrict__ f_out, int n0, int n1, int n2, T tau,
                                                           T eye_cs2, T rho0) {
#define LT_FNEQ_FOR_EACH_FEQ for_each_feq_inc<T, S, 0>(rho, rho0, u, uxu,
#include "fneq_body.inc"
#undef LT_FNEQ_FOR_EACH_FEQ
}

// per-block partial sums of 0.5*u.u (MODE 0) or of sum_q f (MODE 1), or per-block maximum of |u|
// (MODE 2), over the planes
// [p_begin, p_begin + planes) of a2; fixed grid -> fixed summation order.
template <typename T, class S, int LAYOUT, int MODE>
__global__ void __launch_bounds__(kThreads) reduce_kernel(const T *__restrict__ f, long long N,
                                                          long long first, long long count,
                                                          double *__restrict__ partial) {
  double acc = 0.0;
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < count;
       i += (long long)gridDim.x * kThreads) {
    T g[S::Q][1];
    static_for<S::Q>([&](auto qc) {
      constexpr int q = decltype(qc)::value;
      g[q][0] = f[(long long)q * N + first + i];
    });
    T rho, j[3];
    moments<T, S, LAYOUT, 1, 0>(g, rho, j);
    if constexpr (MODE == 0) {
      const T uu[3] = {j[0] / rho, j[1] / rho, j[2] / rho};
      acc += (double)(T(0.5) * square_norm<S, LAYOUT>(uu));
    } else if constexpr (MODE == 1) {
      acc += (double)rho;
    } else {
      const T ux = j[0] / rho, uy = j[1] / rho, uz = j[2] / rho;
      const double m = (double)sqrt(ux * ux + uy * uy + uz * uz);
      acc = nan_max(m, acc);
    }
  }
  const double s = block_sum<MODE == 2>(acc);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// Enstrophy (observable_reporter.py:45-68) from the velocity field u [d][N] (lattice units, logical
// component order, reference layout): per node the 6th-order periodic central differences of
// torch_gradient (util/utility.py:37-99) of u_pu = scale * u, the squared vorticity, fp64 partial sums.
// d(u_c)/d(axis): sum_k w_k u_c(x - s_k e_axis), s = 3, 2, 1, -1, -2, -3, times 1 / dx -- the order of
// the reference's expression (roll by +s reads x - s).
//
// SLAB: u is a rank's velocity field in the slab layout, [3][n2][n1][n0] with x fastest (logical axis a on memory axis
// a) and n2 = the rank's planes + THREE planes of the neighbours on either side; the sum runs over the planes
// [3, n2 - 3) and nothing wraps along a2.
template <typename T, int D, bool SLAB = false>
__global__ void __launch_bounds__(kThreads) enstrophy_kernel(const T *__restrict__ u, int n0, int n1, int n2,
                                                            T scale, T inv_dx, double *__restrict__ partial) {
#pragma clang fp contract(off)
  const long long N = (long long)n0 * n1 * n2;
  const long long first = SLAB ? 3ll * n0 * n1 : 0ll, count = SLAB ? N - 2 * first : N;
  const T w[6] = {T(-1. / 60.), T(3. / 20.), T(-3. / 4.), T(3. / 4.), T(-3. / 20.), T(1. / 60.)};
  const int sh[6] = {3, 2, 1, -1, -2, -3};
  double acc = 0.0;
  for (long long k = (long long)blockIdx.x * kThreads + threadIdx.x; k < count; k += (long long)gridDim.x * kThreads) {
    const long long i = first + k;
    const int c0 = (int)(i % n0), c1 = (int)((i / n0) % n1), c2 = (int)(i / ((long long)n0 * n1));
    // derivative of component c along MEMORY axis m
    auto ddx = [&](int c, int m) -> T {
      const T *uc = u + (long long)c * N;
      T r = T(0);
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        int a0 = c0, a1 = c1, a2 = c2;
        if (m == 0) { a0 = c0 - sh[k]; a0 = wrap_index(a0, n0); }
        if (m == 1) { a1 = c1 - sh[k]; a1 = wrap_index(a1, n1); }
        if (m == 2) { a2 = c2 - sh[k]; if (!SLAB) a2 = wrap_index(a2, n2); }
        const T v = w[k] * (uc[((long long)a2 * n1 + a1) * n0 + a0] * scale);
        r = k == 0 ? v : r + v;
      }
      return r * inv_dx;
    };
    // logical axis a lives on memory axis D - 1 - a (reference layout) / a (slab layout)
    auto grad = [&](int c, int a) -> T { return ddx(c, SLAB ? a : D - 1 - a); };
    const T wz = grad(0, 1) - grad(1, 0);
    T node = wz * wz;
    if constexpr (D == 3) {
      const T wx = grad(2, 1) - grad(1, 2), wy = grad(0, 2) - grad(2, 0);
      node = node + (wx * wx + wy * wy);
    }
    acc += (double)node;
  }
  const double s = block_sum<false>(acc);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// Mass observable (observable_reporter.py:140-158): sum of all populations over the nodes off the first /
// last index of the two fastest axes, minus the populations of the nodes flagged by `mask` (anywhere)
template <typename T, int Q>
__global__ void __launch_bounds__(kThreads) interior_mass_kernel(const T *__restrict__ f, long long N, int n0, int n1,
                                                                const unsigned char *__restrict__ mask,
                                                                double *__restrict__ partial) {
  double acc = 0.0;
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < N; i += (long long)gridDim.x * kThreads) {
    const int c0 = (int)(i % n0), c1 = (int)((i / n0) % n1);
    const bool inner = c0 > 0 && c0 < n0 - 1 && c1 > 0 && c1 < n1 - 1;
    const bool masked = mask != nullptr && mask[i] != 0;
    if (!inner && !masked) continue;
    double node = 0.0;
#pragma unroll
    for (int q = 0; q < Q; ++q) node += (double)f[(long long)q * N + i];
    acc += (inner ? node : 0.0) - (masked ? node : 0.0);
  }
  const double s = block_sum<false>(acc);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// The same over a rank's slab (slab layout, `stride` elements between populations): nodes [first, first + count) are
// the rank's own planes, plane `first / (n0 n1)` is plane z_begin of the nz_global planes of the whole grid; the
// reference's two fastest axes are y and z, i.e. a1 and the GLOBAL a2 here.  `mask` is indexed like the nodes of f.
template <typename T, int Q>
__global__ void __launch_bounds__(kThreads) interior_mass_slab_kernel(const T *__restrict__ f, long long stride,
                                                                     long long first, long long count, int n0, int n1,
                                                                     int z_begin, int nz_global,
                                                                     const unsigned char *__restrict__ mask,
                                                                     double *__restrict__ partial) {
  double acc = 0.0;
  for (long long k = (long long)blockIdx.x * kThreads + threadIdx.x; k < count; k += (long long)gridDim.x * kThreads) {
    const long long i = first + k;
    const int c1 = (int)((i / n0) % n1), z = z_begin + (int)(k / ((long long)n0 * n1));
    const bool inner = c1 > 0 && c1 < n1 - 1 && z > 0 && z < nz_global - 1;
    const bool masked = mask != nullptr && mask[i] != 0;
    if (!inner && !masked) continue;
    double node = 0.0;
#pragma unroll
    for (int q = 0; q < Q; ++q) node += (double)f[(long long)q * stride + i];
    acc += (inner ? node : 0.0) - (masked ? node : 0.0);
  }
  const double s = block_sum<false>(acc);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// halo pack / unpack of the slab driver: the populations that cross a z cut (5 of 19, 9 of 27)
// of one a2 plane <-> one contiguous buffer [n][n1*n0], so that a ghost exchange is a single
// send and a single receive per direction
struct QList {
  int n;
  int q[9];
};
template <typename T, bool PACK>
__global__ void __launch_bounds__(kThreads) plane_pack_kernel(T *__restrict__ f, T *__restrict__ buf,
                                                              long long N, long long plane_off,
                                                              int plane_nodes, QList ql) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= plane_nodes) return;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    if (k < ql.n) {
      T *slot = f + (long long)ql.q[k] * N + plane_off + i;
      if (PACK) buf[(long long)k * plane_nodes + i] = *slot;
      else *slot = buf[(long long)k * plane_nodes + i];
    }
  }
}

// Halo message of the two-step slab driver: [in-plane populations of the plane next to the cut |
// crossing populations of that plane | crossing populations of the plane behind it | plans with masks: the
// populations of the near plane that move AWAY from the cut, which a no-streaming node of the ghost plane
// keeps], each a contiguous block of plane_nodes values.  PACK: f -> buf, else buf -> f.
template <typename T, bool PACK>
__global__ void __launch_bounds__(kThreads) halo2_kernel(T *__restrict__ f, T *__restrict__ buf, long long N,
                                                         long long off_near, long long off_far,
                                                         int plane_nodes, QList in_plane, QList cross, QList away) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= plane_nodes) return;
  auto move = [&](int slot, int q, long long off) {
    T *at = f + (long long)q * N + off + i;
    if (PACK) buf[(long long)slot * plane_nodes + i] = *at;
    else *at = buf[(long long)slot * plane_nodes + i];
  };
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    if (k < in_plane.n) move(k, in_plane.q[k], off_near);
    if (k < cross.n) {
      move(in_plane.n + k, cross.q[k], off_near);
      move(in_plane.n + cross.n + k, cross.q[k], off_far);
    }
    if (k < away.n) move(in_plane.n + 2 * cross.n + k, away.q[k], off_near);
  }
}

// The masked two-step kernel's admission tests (twostep_masked.hpp) on node i (descriptor slot `slot`, no-streaming
// bits b), as mismatch bits:
//  bit 0: the no-streaming bits of a node differ from `expected` on the outlet -- a2 plane `plane` (axis = 2)
//         or a0 column `plane` (axis = 0) -- or from zero elsewhere (axis < 0: no bits anywhere);
//  bit 1: a node of a0 column `face` (>= 0: the face opposite an a0 outlet) is not an equilibrium node
//         (eq_slots: bit s set = boundary s is an EquilibriumBoundaryPU; slots from 32 on are never one of them).
__device__ inline unsigned admission_mismatch(long long i, int slot, unsigned b, long long plane_nodes, int n0, int axis,
                                              int plane, unsigned expected, int face, unsigned eq_slots) {
  const int c0 = (int)(i % n0);
  const bool on_outlet = axis == 2 ? i / plane_nodes == plane : (axis == 0 ? c0 == plane : false);
  unsigned bad = b != (on_outlet ? expected : 0u) ? 1u : 0u;
  if (face >= 0 && c0 == face && !(slot < 32 && ((eq_slots >> slot) & 1u))) bad |= 2u;
  return bad;
}

// node descriptor byte + sparse streaming-mask bits from the reference's two mask tensors, and the admission tests
// above collected in *mismatch
static __global__ void __launch_bounds__(kThreads) compile_masks_kernel(
    const unsigned char *__restrict__ ncm, const unsigned char *__restrict__ nsm, int q,
    long long N, unsigned char *__restrict__ node, unsigned *__restrict__ bits, long long plane_nodes, int n0,
    int axis, int plane, unsigned expected, int face, unsigned eq_slots, unsigned *__restrict__ mismatch) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= N) return;
  unsigned b = 0;
  if (nsm) {
    for (int k = 1; k < q; ++k)
      if (nsm[(long long)k * N + i] == 1) b |= 1u << k;
  }
  const int slot = ncm ? (ncm[i] & 0x7f) : 0;
  node[i] = (unsigned char)(slot | (b ? 0x80 : 0));
  if (bits) bits[i] = b;
  const unsigned bad = admission_mismatch(i, slot, b, plane_nodes, n0, axis, plane, expected, face, eq_slots);
  if (bad) atomicOr(mismatch, bad);
}

// the same admission tests on masks compiled before (lt_plan_update_boundary: an outlet moved after
// lt_plan_set_masks); bits is read only where the node byte says the node has no-streaming bits
static __global__ void __launch_bounds__(kThreads) recheck_masks_kernel(
    const unsigned char *__restrict__ node, const unsigned *__restrict__ bits, long long N, long long plane_nodes,
    int n0, int axis, int plane, unsigned expected, int face, unsigned eq_slots, unsigned *__restrict__ mismatch) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= N) return;
  const unsigned char n = node[i];
  const unsigned b = (bits && (n & 0x80)) ? bits[i] : 0u;
  const unsigned bad = admission_mismatch(i, n & 0x7f, b, plane_nodes, n0, axis, plane, expected, face, eq_slots);
  if (bad) atomicOr(mismatch, bad);
}

}  // namespace lt
