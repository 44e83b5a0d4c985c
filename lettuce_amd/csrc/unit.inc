// The kernels of one unit (a lattice and a scalar type: dispatch.hpp, LT_UNITS) and the host code that picks and
// launches them.  inst.hip includes this once per object, with -DLT_UNIT=<tag> -DLT_PART=<name> from the Makefile.
#include <cstdio>
#include <algorithm>
#include <type_traits>

#include "dispatch.hpp"
#include "kernels.hpp"
#include "launch_limits.hpp"
#include "twostep_masked.hpp"
#include "twostep2d.hpp"
#include "spectrum.hpp"
#include "boundary_force.hpp"
#include "link_bounce.hpp"

#define LT_CAT_(a, b) a##b
#define LT_CAT(a, b) LT_CAT_(a, b)
#define LT_TAG LT_UNIT
#define LT_S lt::LT_FIELD(lattice, LT_UNIT)
#define LT_T LT_FIELD(scalar, LT_UNIT)
#define LT_IS_3D (LT_FIELD(d, LT_UNIT) == 3)
#define LT_HAS_KBC LT_FIELD(kbc, LT_UNIT)
#define LT_HAS_ROLES LT_FIELD(roles, LT_UNIT)
// the lattices of the moment transforms with an equilibrium of their own (mrt.hpp): D2Q9 and D3Q27
#define LT_HAS_MRT (LT_FIELD(q, LT_UNIT) == 9 || LT_FIELD(q, LT_UNIT) == 27)

// LT_PART names the object of the unit that is being built (Makefile: build/inst<N>_<tag>.o):
//   main (inst_)          dispatch(), the auxiliary kernels and the three entry points api.hip calls; the one-step
//                         kernels without a body force, the many-step, the 2-D and the masked two-step launches.  A 3-D
//                         unit (LT_IS_3D) leaves its unmasked two-step launches and its Smagorinsky kernels to the next
//                         three objects and calls them
//   sweeps (inst2_)       3-D units: the unmasked two-step launches (lbm2_kernel) -- an object of its own, so that it
//                         builds beside the rest and can carry its own scheduler setting (Makefile: fp64 D3Q19 is 2.4 %
//                         faster with max-ilp, the masked one-step kernels of the same lattice 8 % slower)
//   roles (inst3_)        units with LT_HAS_ROLES: the two-step launches with separate producer and consumer waves (the
//                         kernel's SCHED = 1) -- that schedule wants another scheduler setting than the one-role kernels
//   smagorinsky (inst4_)  3-D units: the one-step kernels of the Smagorinsky collision -- an object of its own so that
//                         the build takes no longer than before (D3Q27 fp32 with its KBC kernels is the longest job)
//   forced (inst5_)       every unit: the kernels with a body force (the kernels' COLL | kCollForce: BGK, Smagorinsky) -- every
//                         one-step variant BGK has and, where a unit has it (D3Q19 fp32), the plain two-step sweep; objects
//                         of their own, so that the objects of the unforced kernels are what they were
//   relaxations (inst6_)  every unit: the TRT and the regularised collision (kCollTrt, kCollRegularized) -- every
//                         one-step variant BGK has and, where a unit has it (D3Q19 fp32), the plain two-step sweep; again
//                         objects of their own: the earlier objects stay what they were and none of these is the longest job
//   outlets (inst7_)      every unit: the one-step kernels of plans with a constant-pressure outlet (EquilibriumOutletP;
//                         the kernels' ABBD = kOutletsP + chain) -- every collision and every one-step variant the masked
//                         kernels have, at the deepest chain of the layout only; objects of their own once more, so that
//                         every plan without such an outlet launches the code it launched before.  This object: no
//                         collision, BGK and KBC, and the entry point that passes on to the next two
//   outlets2 (inst8_)     ... Smagorinsky, TRT and the regularised collision
//   outlets3 (inst9_)     ... BGK and Smagorinsky with a body force -- three objects, because the chain of depth 2 inlines
//                         the gather and the collision three times and one object per unit would be the longest job
//   mrt (inst10_)         units with LT_HAS_MRT: the multiple-relaxation-time collision (kCollMrt: Dellar on D2Q9,
//                         Hermite on D3Q27; kCollMrtLallemand: Lallemand on D2Q9) -- every one-step variant BGK has, on
//                         a parameter block of their own (KParamsM); no launch of several steps
//   mrt_outlets (inst11_) ... and its kernels of plans with a constant-pressure outlet
//   incompressible (inst12_)  every unit: the kernels of the incompressible equilibrium (the kernels' COLL |
//                         kCollIncompressible: BGK, BGK with a body force, TRT, the regularised collision) -- the
//                         one-step variants of the reference layout, on parameter
//                         blocks of their own (KParamsI, KParamsFI), and the equilibrium and f_neq kernels; no launch of
//                         several steps.  Objects of their own again: every other plan launches what it launched before
//   spectrum (inst13_)    2-D and 3-D units: the two launches of the energy spectrum (spectrum.hpp), which depend on the
//                         scalar type and the dimension only -- an object of its own, so that no other object changes
//   boundary_force (inst14_)  2-D and 3-D units: the two launches of the momentum-exchange force on a bounce-back body
//                         (boundary_force.hpp) -- an object of its own again
//   links (inst15_)       2-D and 3-D units: the pass of the interpolated bounce-back over a plan's link list and the two
//                         launches of the momentum-exchange force over it (link_bounce.hpp) -- an object of its own again
//   force_field (inst16_) every unit: the kernels with a body force whose acceleration is a per-node field (the kernels'
//                         COLL | kCollForce | kCollField: BGK 37, Smagorinsky 39) -- the one-step variants of the
//                         reference layout without the outlet depths, on a parameter block of their own (KParamsFF); no
//                         launch of several steps.  Objects of their own again: every other plan launches what it did
// LT_ONE_STEP: the object holds the one-step launcher and its ladder; LT_SWEEP: the two-step sweep launcher
#define LT_PART_main 1
#define LT_PART_sweeps 2
#define LT_PART_roles 3
#define LT_PART_smagorinsky 4
#define LT_PART_forced 5
#define LT_PART_relaxations 6
#define LT_PART_outlets 7
#define LT_PART_outlets2 8
#define LT_PART_outlets3 9
#define LT_PART_mrt 10
#define LT_PART_mrt_outlets 11
#define LT_PART_incompressible 12
#define LT_PART_spectrum 13
#define LT_PART_boundary_force 14
#define LT_PART_links 15
#define LT_PART_force_field 16
#define LT_PART_IS_OUTLETS (LT_PART_IS(outlets) || LT_PART_IS(outlets2) || LT_PART_IS(outlets3) || LT_PART_IS(mrt_outlets))
#define LT_PART_IS(name) (LT_CAT(LT_PART_, LT_PART) == LT_PART_##name)
#if LT_PART_IS(main)
#define LT_ONE_STEP 1
#define LT_SWEEP 0
#elif LT_PART_IS(sweeps)
#define LT_ONE_STEP 0
#define LT_SWEEP 1
#elif LT_PART_IS(roles)
#define LT_ONE_STEP 0
#define LT_SWEEP 1
#elif LT_PART_IS(smagorinsky)
#define LT_ONE_STEP 1
#define LT_SWEEP 0
#elif LT_PART_IS(forced)
#define LT_ONE_STEP 1
#define LT_SWEEP 1
#elif LT_PART_IS(relaxations)
#define LT_ONE_STEP 1
#define LT_SWEEP 1
#elif LT_PART_IS_OUTLETS || LT_PART_IS(mrt) || LT_PART_IS(incompressible) || LT_PART_IS(force_field)
#define LT_ONE_STEP 1
#define LT_SWEEP 0
#elif LT_PART_IS(spectrum) || LT_PART_IS(boundary_force) || LT_PART_IS(links)
#define LT_ONE_STEP 0
#define LT_SWEEP 0
#else
#error "LT_PART: main, sweeps, roles, smagorinsky, forced, relaxations, outlets, outlets2, outlets3, mrt, mrt_outlets, incompressible, spectrum, boundary_force, links or force_field"
#endif
#if (LT_PART_IS(mrt) || LT_PART_IS(mrt_outlets)) && !LT_HAS_MRT
#error "the MRT collision exists on D2Q9 and D3Q27"
#endif
#if LT_PART_IS(spectrum) && LT_FIELD(d, LT_UNIT) < 2
#error "the energy spectrum exists in 2-D and 3-D"
#endif
#if LT_PART_IS(boundary_force) && LT_FIELD(d, LT_UNIT) < 2
#error "the boundary force kernel exists in 2-D and 3-D"
#endif
#if LT_PART_IS(links) && LT_FIELD(d, LT_UNIT) < 2
#error "the link kernels exist in 2-D and 3-D"
#endif

namespace lt {
namespace {

using S = LT_S;
using T = LT_T;
// the unit's 3-D two-step tile (launch_limits.hpp)
constexpr UnitTile kTile = two_step_tile<S, T>();

// The parameter block of a kernel with collision COLL, and a launch's: zeroed, then every field that means the same
// to all launchers.  A launcher sets what is its own on top.  n2: the planes of the field (the 2-D launchers: 1)
template <int COLL>
using ParamsOfQuadratic = std::conditional_t<coll_mrt(COLL), KParamsM<T>, std::conditional_t<coll_forced(COLL), KParamsF<T>,
                                             std::conditional_t<coll_field(COLL), KParamsFF<T>, KParams<T>>>>;
template <int COLL>
using ParamsOf = std::conditional_t<coll_incompressible(COLL), std::conditional_t<coll_forced(COLL), KParamsFI<T>, KParamsI<T>>,
                                    ParamsOfQuadratic<COLL>>;
template <class P>
P params_of(const StepArgs &a, int n2) {
  P p{};
  p.in = static_cast<const T *>(a.in);
  p.out = static_cast<T *>(a.out);
  p.n0 = a.n0; p.n1 = a.n1; p.n2 = n2;
  p.nv0 = a.n0;
  p.p_begin = a.p_begin;
  p.p_stride = a.p_stride;
  p.wrap2 = a.wrap2;
  p.N = (long long)a.n0 * a.n1 * n2;
  p.Ni = a.stride_in > 0 ? a.stride_in : p.N;
  p.No = a.stride_out > 0 ? a.stride_out : p.N;
  p.tau_inv = (T)(1.0 / a.tau);
  const double beta = 1. / (2 * a.tau);          // kbc_collision.py:97-99
  p.beta = (T)beta;
  p.inv_beta = (T)(1. / beta);
  p.tau = (T)a.tau;
  p.smag_c2 = (T)(a.smagorinsky * a.smagorinsky);   // smagorinsky_collision.py:32: constant ** 2 in double
  // the collision's own scalar (kernels.hpp, collide_node): TRT 1 / (2 tau_minus) beside beta = 1 / (2 tau_plus)
  // (trt_collision.py:22,25), the regularised collision 1 - 1 / tau (regularized_collision.py:42)
  if ((a.coll & ~kCollIncompressible) == kCollTrt) p.smag_c2 = (T)(1.0 / (2.0 * a.tau_minus));
  if ((a.coll & ~kCollIncompressible) == kCollRegularized) p.smag_c2 = (T)(1.0 - 1.0 / a.tau);
  p.node = a.node;
  p.nsm_bits = a.nsm_bits;
  p.bt = static_cast<const BoundaryTable<T> *>(a.bt);
  p.nb = a.nb;
  p.pack_lo = static_cast<T *>(a.pack_lo);
  p.pack_hi = static_cast<T *>(a.pack_hi);
  p.pack_lo_plane = a.pack_lo_plane;
  p.pack_hi_plane = a.pack_hi_plane;
  return p;
}

// uniform body force (lt_plan_set_force): the acceleration permuted from the logical order x, y, z to the memory axes
// of the layout, as the kernels read the velocity
template <int LAYOUT>
void set_force(KParamsF<T> &p, const StepArgs &a) {
  using M = MemMap<S, LAYOUT>;
  p.accel[0] = p.accel[1] = p.accel[2] = T(0);
  p.shift[0] = p.shift[1] = p.shift[2] = T(0);
  for (int c = 0; c < S::D; ++c) {
    p.accel[M::memory(c)] = (T)a.accel[c];
    p.shift[M::memory(c)] = (T)a.ueq_scale * (T)a.accel[c];     // guo.py:27-29: the product in the tensor's precision
  }
  p.source_scale = (T)a.source_scale;
}

// per-node body force (lt_plan_set_force_field): the field and the two scales, each rounded to T once as set_force
// rounds them; the kernels form the node's shift (kernels.hpp, load_node_force)
void set_force_field(KParamsFF<T> &p, const StepArgs &a) {
  p.accel_field = static_cast<const T *>(a.accel_field);
  p.ueq_scale = (T)a.ueq_scale;
  p.source_scale = (T)a.source_scale;
}

// the rates of an MRT plan (lt_plan_set_mrt): r_i = 1 / s_i with both the rate and the quotient in T -- the reference
// converts the rates to the context's dtype and divides there on every call (mrt_collision.py:18-24)
void set_mrt(KParamsM<T> &p, const StepArgs &a) {
  for (int i = 0; i < kMrtMaxQ; ++i) p.r[i] = i < S::Q ? T(1) / (T)a.mrt_rates[i] : T(0);
}

// Kernel names, as lt_plan_kernel_name reports them: the kernel's identifier and its template arguments behind the
// scalar type and the lattice, "lbm2m_kernel<float, lt::D3Q19, 0, 1, 64, 8, 2>".  An argument wrapped in elided() is a
// trailing one that the name leaves out while it has its default (0 / false).
template <class V>
struct Elided {
  V v;
};
template <class V>
Elided<V> elided(V v) { return {v}; }
inline int name_arg(char *s, size_t n, int v) { return snprintf(s, n, ", %d", v); }
inline int name_arg(char *s, size_t n, bool v) { return snprintf(s, n, v ? ", true" : ", false"); }
template <class V>
int name_arg(char *s, size_t n, Elided<V> e) { return e.v == V() ? 0 : name_arg(s, n, e.v); }

// always 0: the launchers return it for "there is such a kernel".  A buffer too short holds the name's beginning
template <class... A>
int kernel_name(const NameBuf &out, const char *kernel, A... args) {
  size_t len = (size_t)snprintf(out.s, out.cap, "%s<%s, lt::%s", kernel, sizeof(T) == 4 ? "float" : "double", S::NAME);
  const auto put = [&](auto v) { if (len < out.cap) len += (size_t)name_arg(out.s + len, out.cap - len, v); };
  (put(args), ...);
  if (len < out.cap) snprintf(out.s + len, out.cap - len, ">");
  return 0;
}

#if LT_ONE_STEP

// one node per thread: the kernels' VEC = 1, SHIFT = 0
template <int LAYOUT, int COLL, int MODE, bool MASKED, int TUNE = 0, bool PACK = false, int ABBD = 0>
int launch(const StepArgs &a, const NameBuf *name) {
  constexpr bool STREAM = MODE != kCollideOnly, COLLIDE = MODE != kStreamOnly;
  constexpr bool OCC4 = (COLL == kCollKbc && MASKED && sizeof(T) == 4 && S::Q == 27 && ABBD == 0);
  using P = ParamsOf<COLL>;
  if (name)
    return kernel_name(*name, OCC4 ? "lbm_kernel_occ4" : "lbm_kernel", LAYOUT, COLL, STREAM, COLLIDE, MASKED, 1, 0, TUNE,
                       PACK, elided(ABBD));
  void (*kern)(const P);
  if constexpr (OCC4)
    kern = lbm_kernel_occ4<T, S, LAYOUT, COLL, STREAM, COLLIDE, MASKED, 1, 0, TUNE, PACK>;
  else
    kern = lbm_kernel<T, S, LAYOUT, COLL, STREAM, COLLIDE, MASKED, 1, 0, TUNE, PACK, ABBD>;
  P p = params_of<P>(a, a.n2);
  p.nvec_total = (unsigned)((long long)p.nv0 * a.n1 * a.planes);
  if constexpr (coll_forced(COLL)) set_force<LAYOUT>(p, a);
  if constexpr (coll_field(COLL)) set_force_field(p, a);
  if constexpr (coll_mrt(COLL)) set_mrt(p, a);
  // the incompressible equilibrium's rho0: rounded once, as a Python float times a tensor of the plan's dtype is
  if constexpr (coll_incompressible(COLL)) p.rho0 = (T)a.rho0;
  p.abb0_slot = a.n0 % 64 == 0 ? a.abb0_slot : 0;
  if (p.nvec_total == 0) return 0;
  const unsigned grid = (p.nvec_total + kThreads - 1) / kThreads;
  // a.lds_bytes of dynamic LDS that no kernel touches: caps the workgroups resident per CU
  // (lt_plan_set_residency)
  hipLaunchKernelGGL(kern, dim3(grid), dim3(kThreads), (unsigned)a.lds_bytes, a.stream, p);
  return (int)hipGetLastError();
}

// Product kernels: one node per thread (VEC = 1).  Measured on MI355X (profiles/r01_variant_sweep*):
// for this 2q-stream kernel 8 waves/SIMD of scalar accesses beat 16-byte accesses at 3-4
// waves/SIMD by 8-13 %, and nontemporal stores (+3-4 %) and loads (+1.6 %) help once the
// populations exceed the caches (TUNE 3).  TUNE 0 (cached accesses) is kept for grids that fit in
// L2 / Infinity Cache.
#define LT_TRY(LAYOUT, COLL, MODE, MASKED)                                    \
  if (a.layout == LAYOUT && a.mode == MODE && a.masked == MASKED) {           \
    if (a.tune == 0) return launch<LAYOUT, COLL, MODE, (MASKED != 0), 0>(a, name); \
    if (a.tune == 3) return launch<LAYOUT, COLL, MODE, (MASKED != 0), 3>(a, name); \
  }

// slab boundary-plane launch with fused halo packing (fused mode, slab layout)
#define LT_TRY_PACK(COLL, MASKED)                                                                             \
  if (a.layout == 1 && a.mode == kFused && a.masked == MASKED && a.pack_lo != nullptr && a.abb_depth == 0)    \
    return launch<1, COLL, kFused, (MASKED != 0), 0, true>(a, name);

// plans with two anti-bounce-back outlets (kernels.hpp, neighbour_moments DEPTH 1): masked kernels that
// apply boundaries, i.e. fused and collide-only
#define LT_TRY_TWO_OUTLETS(LAYOUT, COLL, MODE)                                 \
  if (a.layout == LAYOUT && a.mode == MODE && a.masked && a.abb_depth == 1)    \
    return launch<LAYOUT, COLL, MODE, true, 0, false, 1>(a, name);

// outlets on all three axes of a 3-D flow (their planes meet in corners: DEPTH 2), reference layout
#define LT_TRY_THREE_AXES(COLL, MODE)                                   \
  if (a.layout == 0 && a.mode == MODE && a.masked && a.abb_depth == 2)  \
    return launch<0, COLL, MODE, true, 0, false, 2>(a, name);

#define LT_COLLISION_SET(LAYOUT, COLL, MASKED) \
  LT_TRY(LAYOUT, COLL, kFused, MASKED)         \
  LT_TRY(LAYOUT, COLL, kCollideOnly, MASKED)

// The one-step kernels of collision C, fused and collide-only: main has them for 0 (none), 1 (BGK) and, with
// LT_HAS_KBC, 2; Smagorinsky (3) has every variant BGK has, and so have BGK and Smagorinsky with a body force (5, 7),
// TRT (8), the regularised collision (9) and MRT (10, 11).
// The order matters where the conditions overlap: the outlet depths before the rest, packed before the plain slab set.
template <int C>
int one_step_of(const StepArgs &a, const NameBuf *name) {
#if LT_IS_3D
  LT_TRY_THREE_AXES(C, kFused) LT_TRY_THREE_AXES(C, kCollideOnly)
#endif
  if (a.abb_depth > 1) return kNoKernel;
  LT_TRY_TWO_OUTLETS(0, C, kFused) LT_TRY_TWO_OUTLETS(0, C, kCollideOnly)
#if LT_IS_3D
  LT_TRY_TWO_OUTLETS(1, C, kFused) LT_TRY_TWO_OUTLETS(1, C, kCollideOnly)
#endif
  // reference layout
  LT_COLLISION_SET(0, C, 0)
  LT_COLLISION_SET(0, C, 1)
#if LT_IS_3D
  // slab layout (multi-GPU z-slabs)
  LT_TRY_PACK(C, 0)
  LT_TRY_PACK(C, 1)
  LT_COLLISION_SET(1, C, 0)
  LT_COLLISION_SET(1, C, 1)
#endif
  return kNoKernel;
}

#if LT_PART_IS(incompressible)
// The one-step kernels of collision C with the incompressible equilibrium: every variant of the reference layout that
// one_step_of has (lt_plan_set_equilibrium refuses slab plans and the constant-pressure outlet)
template <int C>
int one_step_incompressible_of(const StepArgs &a, const NameBuf *name) {
  if (a.n_pout > 0 || a.pack_lo || a.pack_hi) return kNoKernel;
#if LT_IS_3D
  LT_TRY_THREE_AXES(C, kFused) LT_TRY_THREE_AXES(C, kCollideOnly)
#endif
  if (a.abb_depth > 1) return kNoKernel;
  LT_TRY_TWO_OUTLETS(0, C, kFused) LT_TRY_TWO_OUTLETS(0, C, kCollideOnly)
  LT_COLLISION_SET(0, C, 0)
  LT_COLLISION_SET(0, C, 1)
  return kNoKernel;
}
#endif

#if LT_PART_IS(force_field)
// The one-step kernels of collision C with a force field: the variants of the reference layout that one_step_of gives
// the uniform force, without the outlet depths (lt_plan_set_force_field refuses slab plans and every outlet)
template <int C>
int one_step_field_of(const StepArgs &a, const NameBuf *name) {
  if (!a.accel_field && !name) return kNoKernel;      // a launch reads the field
  if (a.n_pout > 0 || a.n_abb > 0 || a.abb_depth > 0 || a.pack_lo || a.pack_hi) return kNoKernel;
  LT_COLLISION_SET(0, C, 0)
  LT_COLLISION_SET(0, C, 1)
  return kNoKernel;
}
#endif

#if LT_PART_IS_OUTLETS
// Plans with a constant-pressure outlet, alone or beside anti-bounce-back outlets: masked kernels that apply boundaries
// (fused and collide-only), both cache policies, the packed plane launch of the slabs.  One chain depth per layout, the
// deepest a plan of that layout can need (api.hip, abb_depth_of): outlets on all three axes in the reference layout of a
// 3-D unit (2), on two axes in the slab layout and in 2-D (1); two outlets on the one axis of a 1-D lattice count as depth 1
// too (on a lattice of two nodes each outlet's neighbour lies in the other's plane).  A plan with fewer axes or one outlet
// takes the same kernel: the chain is followed only where a lower outlet's plane holds the neighbour.
template <int LAYOUT>
constexpr int kOutletChain = S::D == 3 && LAYOUT == 0 ? 2 : 1;

template <int C, int LAYOUT>
int pressure_outlets_in(const StepArgs &a, const NameBuf *name) {
  constexpr int ABBD = kOutletsP + kOutletChain<LAYOUT>;
  if (a.abb_depth > kOutletChain<LAYOUT>) return kNoKernel;
  if constexpr (LAYOUT == 1) {
    if (a.mode == kFused && a.pack_lo != nullptr) return launch<1, C, kFused, true, 0, true, ABBD>(a, name);
  }
  if (a.mode == kFused && a.tune == 0) return launch<LAYOUT, C, kFused, true, 0, false, ABBD>(a, name);
  if (a.mode == kFused && a.tune == 3) return launch<LAYOUT, C, kFused, true, 3, false, ABBD>(a, name);
  if (a.mode == kCollideOnly && a.tune == 0) return launch<LAYOUT, C, kCollideOnly, true, 0, false, ABBD>(a, name);
  if (a.mode == kCollideOnly && a.tune == 3) return launch<LAYOUT, C, kCollideOnly, true, 3, false, ABBD>(a, name);
  return kNoKernel;
}

template <int C>
int pressure_outlets_of(const StepArgs &a, const NameBuf *name) {
  if (!a.masked) return kNoKernel;
  if (a.layout == 0) return pressure_outlets_in<C, 0>(a, name);
#if LT_IS_3D
  if (a.layout == 1) return pressure_outlets_in<C, 1>(a, name);
#endif
  return kNoKernel;
}
#endif

#endif  // LT_ONE_STEP

#if LT_SWEEP
// Two fused steps per launch (kernels.hpp, lbm2_kernel): whole periodic grid, no masks.
// returns kNoKernel when this (lattice, dtype) has no instantiation or the grid does not tile.
// one node per thread and per block: the kernel's NPT = NPB = 1
// SCHED 1: separate producer and consumer waves (twostep_roles.hpp)
// Smagorinsky (COLL 3), BGK with a body force (COLL 5), TRT (8) and the regularised collision (9): the plain one-role
// sweep of D3Q19 fp32
template <int LAYOUT, int COLL, int T0, int T1, int MODE = 0, int SCHED = 0>
int launch_twice(const StepArgs &a, const NameBuf *name) {
  if constexpr (S::D == 3 && T0 > 0 &&
                (COLL == kCollNone || COLL == kCollBgk ||
                 ((COLL == kCollSmagorinsky || COLL == (kCollBgk | kCollForce) || COLL == kCollTrt || COLL == kCollRegularized) &&
                  S::Q == 19 && sizeof(T) == 4 && MODE == 0 && SCHED == 0))) {
    using B = TwoStep<T, S, T0, T1>;
    if (name) return kernel_name(*name, "lbm2_kernel", LAYOUT, COLL, T0, T1, 1, MODE, 1, elided(SCHED));
    if (a.n0 % T0 != 0 || a.n1 % T1 != 0 || a.seg_len < min_segment(false) || a.masked || a.planes < 1 || a.p_stride != 1 ||
        !plane_addressable(a.n0, a.n1, sizeof(T)))
      return kNoKernel;
    if (MODE == 2 && (!a.signal || a.planes2 < 2 || a.planes2 > a.seg_len || a.seg_len < 2)) return kNoKernel;
    using P = ParamsOf<COLL>;
    P p = params_of<P>(a, a.n2);
    // the output planes: [p_begin, p_end) and, at a slab's other edge, [p_begin2, p_end2); a.seg_len of them per workgroup
    p.p_end = a.p_begin + a.planes;
    p.p_begin2 = a.p_begin2;
    p.p_end2 = a.p_begin2 + a.planes2;
    if constexpr (coll_forced(COLL)) set_force<LAYOUT>(p, a);
    p.nb = a.shift == 3 ? 1 : (a.shift == 4 ? 2 : 0);   // A/B: 1 = no XCD-aware renumbering of the workgroups, 2 = per segment layer
    // MODE 2: the edge workgroups first, each adds 1 to *signal (kernels.hpp, KParams)
    p.signal = MODE == 2 ? a.signal : nullptr;
    p.edge_first = MODE == 2 ? 1 : 0;
    p.ghost_lo = static_cast<const T *>(a.ghost_lo);
    p.ghost_hi = static_cast<const T *>(a.ghost_hi);
    p.lo = a.interior_begin; p.hi = a.interior_end;
    const unsigned grid = (unsigned)((a.n0 / T0) * (a.n1 / T1) * ((a.planes + a.seg_len - 1) / a.seg_len +
                                                                   (a.planes2 + a.seg_len - 1) / a.seg_len));
    constexpr int threads = SCHED ? RoleWaves<B::NI, B::NO>::THREADS : (B::NI + 63) / 64 * 64;
    void (*kern)(const P, const int) = lbm2_kernel<T, S, LAYOUT, COLL, T0, T1, 1, MODE, 1, SCHED>;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(threads), 0, a.stream, p, a.seg_len);
    return (int)hipGetLastError();
  } else {
    return kNoKernel;
  }
}

// the sweeps of this object
int sweep(const StepArgs &a, const NameBuf *name) {
  constexpr int W = kTile.width, R = kTile.rows;
  if constexpr (R > 0) {
#if LT_PART_IS(roles)
    // BGK with separate producer and consumer waves, where they won their A/B (DESIGN.md section 7)
    if (a.layout == 0) return launch_twice<0, kCollBgk, W, R, 0, 1>(a, name);
    return launch_twice<1, kCollBgk, W, R, 0, 1>(a, name);
#elif LT_PART_IS(forced)
    // with a body force: plain sweeps of periodic plans (no packing, no signalling launch)
    if (a.masked || a.pack_lo || a.pack_hi || a.signal) return kNoKernel;
    if (a.layout == 0 && a.coll == (kCollBgk | kCollForce)) return launch_twice<0, kCollBgk | kCollForce, W, R>(a, name);
    if (a.layout == 1 && a.coll == (kCollBgk | kCollForce)) return launch_twice<1, kCollBgk | kCollForce, W, R>(a, name);
    // (Smagorinsky with a force, COLL 7: 168 VGPRs and 84-92 bytes of scratch per lane under every scheduler setting
    // where the unforced sweep has 168 and none -- not built, the plan keeps the one-step kernel: DESIGN.md section 4)
#elif LT_PART_IS(relaxations)
    // TRT and the regularised collision: plain sweeps of periodic plans (no packing, no signalling launch)
    if (a.masked || a.pack_lo || a.pack_hi || a.signal) return kNoKernel;
    if (a.layout == 0 && a.coll == kCollTrt) return launch_twice<0, kCollTrt, W, R>(a, name);
    if (a.layout == 1 && a.coll == kCollTrt) return launch_twice<1, kCollTrt, W, R>(a, name);
    if (a.layout == 0 && a.coll == kCollRegularized) return launch_twice<0, kCollRegularized, W, R>(a, name);
    if (a.layout == 1 && a.coll == kCollRegularized) return launch_twice<1, kCollRegularized, W, R>(a, name);
#else
    // the unmasked two-step launches of a 3-D unit
    const int coll = a.coll;
#if LT_HAS_ROLES
    // the plain BGK sweep: part roles; shift policy 6 runs the one-role schedule (A/B)
    if (coll == kCollBgk && a.shift != 6 && (a.layout == 0 || !(a.pack_lo || a.pack_hi || a.signal)))
      return LT_CAT(roles_, LT_TAG)(a, name);
#endif
    if (a.layout == 0 && coll == kCollNone) return launch_twice<0, kCollNone, W, R>(a, name);
    if (a.layout == 0 && coll == kCollBgk) return launch_twice<0, kCollBgk, W, R>(a, name);
    if (a.layout == 0 && coll == kCollSmagorinsky) return launch_twice<0, kCollSmagorinsky, W, R>(a, name);
    // Smagorinsky has the plain sweep only: no edge launch with packing, no signalling launch
    if (coll == kCollSmagorinsky && (a.pack_lo || a.pack_hi || a.signal)) return kNoKernel;
    if (a.layout == 1 && (a.pack_lo || a.pack_hi)) {     // slab edge launch with fused halo packing
      if (coll == kCollNone) return launch_twice<1, kCollNone, W, R, 1>(a, name);
      if (coll == kCollBgk) return launch_twice<1, kCollBgk, W, R, 1>(a, name);
    }
    if (a.layout == 1 && a.signal) {                     // whole slab, edge workgroups first
      if (coll == kCollNone) return launch_twice<1, kCollNone, W, R, 2>(a, name);
      if (coll == kCollBgk) return launch_twice<1, kCollBgk, W, R, 2>(a, name);
    }
    if (a.layout == 1 && coll == kCollNone) return launch_twice<1, kCollNone, W, R>(a, name);
    if (a.layout == 1 && coll == kCollBgk) return launch_twice<1, kCollBgk, W, R>(a, name);
    if (a.layout == 1 && coll == kCollSmagorinsky) return launch_twice<1, kCollSmagorinsky, W, R>(a, name);
#endif
  }
  return kNoKernel;
}
#endif  // LT_SWEEP

#if LT_PART_IS(main)
// Two fused steps per launch for plans with boundaries (twostep_masked.hpp, lbm2m_kernel): whole periodic
// grid, reference layout.  api.hip admits the plan (masked_two_step_ok); here: the grid tiles and the field can be
// addressed (launch_limits.hpp: fields beyond 4 GiB run the instantiation with a descriptor per population).
// T1: the unit's rows with masks, 0 where the kernel's LDS does not fit
template <int LAYOUT, int COLL, int T0, int T1, int AX = 2>
int launch_twice_masked(const StepArgs &a, const NameBuf *name) {
  // BGK / streaming.  KBC inside this kernel (256 VGPRs, spills: not faster than one update per launch) lost its A/B
  // (DESIGN.md section 4)
  if constexpr (S::D == 3 && T1 > 0 && (COLL == kCollNone || COLL == kCollBgk)) {
    static_assert(two_step_masked_lds<T, S, LAYOUT, T0, T1>() <= kLdsBudget, "the unit's tile with masks fits the LDS");
    using B = TwoStep<T, S, T0, T1>;
    if (name) return kernel_name(*name, "lbm2m_kernel", LAYOUT, COLL, T0, T1, AX);
    // (D3Q27: 26.7 GLUPS at 384^3 against 27.2 with one update per launch -- its 2 x 27 population bases spill;
    // D3Q19: 52-55 GLUPS at 384^3 / 512^3 against 38: profiles/r04y_large_obstacle.jsonl)
    constexpr bool kHasBig = masked_per_population(LAYOUT, COLL, S::Q);
    const long long distance = std::max(std::max(a.stride_in, a.stride_out), (long long)a.n0 * a.n1 * a.n2);
    if (a.n0 % T0 != 0 || a.n1 % T1 != 0 || a.seg_len < min_segment(true) || !a.masked || a.planes < min_segment(true) ||
        a.p_stride != 1 || a.planes2 != 0 || a.pack_lo || a.pack_hi || !field_addressable(S::Q, distance, sizeof(T), kHasBig))
      return kNoKernel;
    KParams<T> p = params_of<KParams<T>>(a, a.n2);
    p.p_end = a.p_begin + a.planes;      // the output planes, a.seg_len of them per workgroup
    const unsigned grid = (unsigned)((a.n0 / T0) * (a.n1 / T1) * ((a.planes + a.seg_len - 1) / a.seg_len));
    if constexpr (kHasBig) {
      if (!field_addressable(S::Q, distance, sizeof(T), false)) {
        hipLaunchKernelGGL((lbm2m_kernel<T, S, LAYOUT, COLL, T0, T1, AX, true>), dim3(grid), dim3(B::THREADS), 0,
                           a.stream, p, a.seg_len);
        return (int)hipGetLastError();
      }
    }
    hipLaunchKernelGGL((lbm2m_kernel<T, S, LAYOUT, COLL, T0, T1, AX>), dim3(grid), dim3(B::THREADS), 0, a.stream,
                       p, a.seg_len);
    return (int)hipGetLastError();
  } else {
    return kNoKernel;
  }
}

// Two fused steps per launch on 2-D lattices (twostep2d.hpp): whole periodic grid, a.seg_len rows per workgroup,
// strips of W columns (api.hip picks W and the segment length).  Without masks lbm2d2_kernel, with boundaries
// lbm2d2m_kernel: api.hip admits the plan (masked_two_step_axis)
template <int COLL, int W, bool MASKED>
int launch_twice2d(const StepArgs &a, const NameBuf *name) {
  if constexpr (S::D == 2 && (COLL == kCollNone || COLL == kCollBgk)) {
    if (name) return kernel_name(*name, MASKED ? "lbm2d2m_kernel" : "lbm2d2_kernel", COLL, W);
    if (a.layout != 0 || (a.masked != 0) != MASKED || a.n0 % W != 0 || a.seg_len < min_segment(MASKED) ||
        a.n1 < (MASKED ? kOutletSweepMin : 1) || a.n2 != 1)
      return kNoKernel;
    const KParams<T> p = params_of<KParams<T>>(a, 1);      // n2 = 1: the field is one plane
    const unsigned grid = (unsigned)((a.n0 / W) * ((a.n1 + a.seg_len - 1) / a.seg_len));
    void (*kern)(const KParams<T>, const int);
    if constexpr (MASKED) kern = lbm2d2m_kernel<T, S, COLL, W>; else kern = lbm2d2_kernel<T, S, COLL, W>;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(TwoStep2D<T, W>::THREADS), 0, a.stream, p, a.seg_len);
    return (int)hipGetLastError();
  } else {
    return kNoKernel;
  }
}

// Up to kManyMax steps per launch on small 2-D grids (kernels.hpp, lbm_many_kernel; launch_limits.hpp)
template <int COLL, bool MASKED>
int launch_many(const StepArgs &a, const NameBuf *name) {
  if constexpr (S::D == 2 && (COLL != kCollKbc || LT_HAS_KBC)) {
    using G = ManyStep2D<kManyTile, kManyTile, kManyMax>;
    if (name) return kernel_name(*name, "lbm_many_kernel", COLL, kManyTile, kManyTile, kManyMax, elided(MASKED));
    const int outlets = MASKED ? a.n_abb : 0;
    if (a.layout != 0 || (a.masked != 0) != MASKED || a.n0 % kManyTile != 0 || a.n1 % kManyTile != 0 || a.seg_len < 1 ||
        a.seg_len > many_steps_max(outlets > 0) || a.planes != a.n2 || outlets > 1)
      return kNoKernel;
    KParams<T> p = params_of<KParams<T>>(a, 1);      // n2 = 1: the field is one plane ...
    p.wrap2 = 1;                                     // ... which is its own neighbour along a2
    p.abb0_slot = outlets;                           // here: 1 = the plan has an outlet (one more ring)
    const unsigned grid = (unsigned)((a.n0 / kManyTile) * (a.n1 / kManyTile));
    hipLaunchKernelGGL((lbm_many_kernel<T, S, COLL, kManyTile, kManyTile, kManyMax, MASKED>), dim3(grid),
                       dim3(G::THREADS), 0, a.stream, p, a.seg_len);
    return (int)hipGetLastError();
  } else {
    return kNoKernel;
  }
}

template <int C>
int many_of(const StepArgs &a, const NameBuf *name) {
  return a.masked ? launch_many<C, true>(a, name) : launch_many<C, false>(a, name);
}

// strips of a.strip columns (launch_limits.hpp, strip_width)
template <int C>
int strips_of(const StepArgs &a, const NameBuf *name) {
#define LT_TRY_STRIP(W) \
  if (a.strip == W) return a.masked ? launch_twice2d<C, W, true>(a, name) : launch_twice2d<C, W, false>(a, name);
  LT_STRIP_WIDTHS(LT_TRY_STRIP)
#undef LT_TRY_STRIP
  return kNoKernel;
}

#if LT_IS_3D
// two steps per launch of a 3-D unit: with boundaries here, without in the unit's part sweeps
int twice_3d(const StepArgs &a, const NameBuf *name) {
  constexpr int W = kTile.width, R = kTile.rows;
  if constexpr (R > 0) {
    if (!a.masked) return LT_CAT(twice_, LT_TAG)(a, name);
    // a.abb_axis: memory axis of the plan's outlet (2 also for plans without one)
    constexpr int RM = kTile.rows_masked;
#define LT_TRY_MASKED_TWICE(LAYOUT_, COLL_, AX_)                       \
  if (a.layout == LAYOUT_ && a.coll == COLL_ && a.abb_axis == AX_)     \
    return launch_twice_masked<LAYOUT_, COLL_, W, RM, AX_>(a, name);
    LT_TRY_MASKED_TWICE(0, kCollNone, 2) LT_TRY_MASKED_TWICE(0, kCollBgk, 2)
    LT_TRY_MASKED_TWICE(0, kCollNone, 0) LT_TRY_MASKED_TWICE(0, kCollBgk, 0)
    LT_TRY_MASKED_TWICE(1, kCollNone, 2) LT_TRY_MASKED_TWICE(1, kCollBgk, 2)
    LT_TRY_MASKED_TWICE(1, kCollNone, 0) LT_TRY_MASKED_TWICE(1, kCollBgk, 0)
#undef LT_TRY_MASKED_TWICE
  }
  return kNoKernel;
}
#endif

int dispatch(const StepArgs &a, const NameBuf *name) {
  const int coll = a.mode == kStreamOnly ? kCollNone : a.coll;   // streaming does not depend on it
  if (coll_incompressible(coll)) return LT_CAT(incompressible_, LT_TAG)(a, name);   // part incompressible
  // a constant-pressure outlet: part outlets has the kernels that apply boundaries (streaming alone applies none)
  if (a.n_pout > 0 && a.mode != kStreamOnly) return LT_CAT(outlets_, LT_TAG)(a, name);
  if (coll_forced(coll)) return LT_CAT(forced_, LT_TAG)(a, name);   // body force: part forced
  if (coll_field(coll)) return LT_CAT(force_field_, LT_TAG)(a, name);   // ... as a per-node field: part force_field
  if (coll == kCollTrt || coll == kCollRegularized) return LT_CAT(relax_, LT_TAG)(a, name);   // part relaxations
#if LT_HAS_MRT
  if (coll_mrt(coll)) return LT_CAT(mrt_, LT_TAG)(a, name);   // MRT: part mrt
#endif
  if (a.mode == kFusedMany) {
    if (coll == kCollNone) return many_of<kCollNone>(a, name);
    if (coll == kCollBgk) return many_of<kCollBgk>(a, name);
    if (coll == kCollKbc) return many_of<kCollKbc>(a, name);
    return kNoKernel;
  }
  if (a.mode == kFusedTwice) {
#if LT_IS_3D
    return twice_3d(a, name);
#else
    if (S::D != 2 || a.layout != 0) return kNoKernel;
    if (coll == kCollNone) return strips_of<kCollNone>(a, name);
    if (coll == kCollBgk) return strips_of<kCollBgk>(a, name);
    return kNoKernel;
#endif
  }
  if (a.mode == kStreamOnly) {      // the one kernel that does not collide: no check of the outlet depth
    LT_TRY(0, kCollNone, kStreamOnly, 0)
    LT_TRY(0, kCollNone, kStreamOnly, 1)
#if LT_IS_3D
    LT_TRY(1, kCollNone, kStreamOnly, 0)
    LT_TRY(1, kCollNone, kStreamOnly, 1)
#endif
    return kNoKernel;
  }
  if (coll == kCollNone) return one_step_of<kCollNone>(a, name);
  if (coll == kCollBgk) return one_step_of<kCollBgk>(a, name);
#if LT_HAS_KBC
  if (coll == kCollKbc) return one_step_of<kCollKbc>(a, name);
#endif
#if LT_IS_3D
  if (coll == kCollSmagorinsky) return LT_CAT(smag_, LT_TAG)(a, name);       // part smagorinsky
#else
  if (coll == kCollSmagorinsky) return one_step_of<kCollSmagorinsky>(a, name);
#endif
  return kNoKernel;
}

// A scalar observable: `kern` over the plan's fixed grid leaves a partial per workgroup, then one workgroup takes the
// partials in index order (reduce.hpp; MAX: the NaN-propagating maximum)
template <bool MAX = false, class K, class... A>
void reduced(const AuxArgs &a, K kern, A... args) {
  hipLaunchKernelGGL(kern, dim3(a.reduce_blocks), dim3(kThreads), 0, a.stream, args..., a.partial);
  hipLaunchKernelGGL(finish_sum_kernel<MAX>, dim3(1), dim3(kThreads), 0, a.stream, a.partial, a.reduce_blocks, a.out);
}

template <int LAYOUT>
int aux_impl(const AuxArgs &a) {
  // feq with another equilibrium than the quadratic one: part incompressible
  if (a.equilibrium != 0 && (a.what == kAuxEquilibrium || a.what == kAuxFneq)) return LT_CAT(incompressible_aux_, LT_TAG)(a);
  const T *f = static_cast<const T *>(a.f);
  const unsigned grid = (unsigned)((a.N + kThreads - 1) / kThreads);
  constexpr bool kWholeGrid = S::D >= 2 && LAYOUT == 0, kSlab = S::D == 3 && LAYOUT == 1;
  switch (a.what) {
    case kAuxMacroscopic:
      hipLaunchKernelGGL((macroscopic_kernel<T, S, LAYOUT>), dim3(grid), dim3(kThreads), 0,
                         a.stream, f, static_cast<T *>(a.rho), static_cast<T *>(a.u), a.N, a.stride,
                         a.u_stride ? a.u_stride : a.N);
      break;
    case kAuxEquilibrium:
      hipLaunchKernelGGL((equilibrium_kernel<T, S, LAYOUT>), dim3(grid), dim3(kThreads), 0,
                         a.stream, static_cast<const T *>(a.rho), static_cast<const T *>(a.u),
                         const_cast<T *>(f), a.N);
      break;
    case kAuxKineticEnergy:
      reduced(a, reduce_kernel<T, S, LAYOUT, 0>, f, a.stride, a.first, a.count);
      break;
    case kAuxMass:
      reduced(a, reduce_kernel<T, S, LAYOUT, 1>, f, a.stride, a.first, a.count);
      break;
    case kAuxMaxVelocity:
      reduced<true>(a, reduce_kernel<T, S, LAYOUT, 2>, f, a.stride, a.first, a.count);
      break;
    case kAuxEnstrophy:     // u into the scratch field, then the vorticity stencil over it
      if constexpr (!kWholeGrid) return kNoKernel;
      else {
        hipLaunchKernelGGL((macroscopic_kernel<T, S, LAYOUT>), dim3(grid), dim3(kThreads), 0,
                           a.stream, f, static_cast<T *>(nullptr), static_cast<T *>(a.u), a.N, a.N, a.N);
        reduced(a, enstrophy_kernel<T, S::D>, static_cast<const T *>(a.u), a.n0, a.n1, a.n2, (T)a.scale, (T)a.inv_dx);
      }
      break;
    case kAuxInteriorMass:
      if constexpr (!kWholeGrid) return kNoKernel;
      else reduced(a, interior_mass_kernel<T, S::Q>, f, a.N, a.n0, a.n1, a.mask);
      break;
    case kAuxFneq:
      if constexpr (!kWholeGrid) return kNoKernel;
      else
        hipLaunchKernelGGL((fneq_kernel<T, S>), dim3(grid), dim3(kThreads), 0, a.stream,
                           static_cast<const T *>(a.rho), static_cast<const T *>(a.u), const_cast<T *>(f), a.n0, a.n1,
                           a.n2, (T)a.scale, (T)a.inv_dx);
      break;
    case kAuxSlabEnstrophy:
      if constexpr (!kSlab) return kNoKernel;
      else reduced(a, enstrophy_kernel<T, 3, true>, static_cast<const T *>(a.u), a.n0, a.n1, a.n2, (T)a.scale, (T)a.inv_dx);
      break;
    case kAuxSlabInteriorMass:
      if constexpr (!kSlab) return kNoKernel;
      else
        reduced(a, interior_mass_slab_kernel<T, S::Q>, f, a.stride, a.first, a.count, a.n0, a.n1, a.z_begin,
                a.nz_global, a.mask);
      break;
    case kAuxSpectrum:
#if LT_FIELD(d, LT_UNIT) >= 2
      if constexpr (LAYOUT == 0) return LT_CAT(spectrum_, LT_TAG)(a);
#endif
      return kNoKernel;
    case kAuxBoundaryForce:
#if LT_FIELD(d, LT_UNIT) >= 2
      if constexpr (LAYOUT == 0) return LT_CAT(boundary_force_, LT_TAG)(a);
#endif
      return kNoKernel;
    default:
      return kNoKernel;
  }
  return (int)hipGetLastError();
}

#endif  // LT_PART_IS(main)

}  // namespace

// what the object exports (dispatch.hpp, LT_DECLARE_UNIT)
#if LT_PART_IS(main)
int LT_CAT(step_, LT_TAG)(const StepArgs &a) { return dispatch(a, nullptr); }

const char *LT_CAT(name_, LT_TAG)(const StepArgs &a, const NameBuf &name) {
  return dispatch(a, &name) == 0 ? name.s : nullptr;
}

int LT_CAT(aux_, LT_TAG)(const AuxArgs &a) {
#if LT_IS_3D
  if (a.layout == 1) return aux_impl<1>(a);
#endif
  return aux_impl<0>(a);
}
#elif LT_PART_IS(sweeps)
int LT_CAT(twice_, LT_TAG)(const StepArgs &a, const NameBuf *name) { return sweep(a, name); }
#elif LT_PART_IS(roles)
int LT_CAT(roles_, LT_TAG)(const StepArgs &a, const NameBuf *name) { return sweep(a, name); }
#elif LT_PART_IS(smagorinsky)
int LT_CAT(smag_, LT_TAG)(const StepArgs &a, const NameBuf *name) { return one_step_of<kCollSmagorinsky>(a, name); }
#elif LT_PART_IS(forced)
int LT_CAT(forced_, LT_TAG)(const StepArgs &a, const NameBuf *name) {
  if (a.mode == kFusedTwice) return S::D == 3 ? sweep(a, name) : kNoKernel;
  if (a.coll == (kCollBgk | kCollForce)) return one_step_of<kCollBgk | kCollForce>(a, name);
  if (a.coll == (kCollSmagorinsky | kCollForce)) return one_step_of<kCollSmagorinsky | kCollForce>(a, name);
  return kNoKernel;
}
#elif LT_PART_IS(relaxations)
// one-step kernels and the plain sweep only: no many-step, 2-D or masked two-step launch
int LT_CAT(relax_, LT_TAG)(const StepArgs &a, const NameBuf *name) {
  if (a.mode == kFusedTwice) return S::D == 3 ? sweep(a, name) : kNoKernel;
  if (a.mode != kFused && a.mode != kCollideOnly) return kNoKernel;
  if (a.coll == kCollTrt) return one_step_of<kCollTrt>(a, name);
  if (a.coll == kCollRegularized) return one_step_of<kCollRegularized>(a, name);
  return kNoKernel;
}
#elif LT_PART_IS(outlets)
// one-step kernels only: no many-step, 2-D, masked two-step or slab two-step launch takes this boundary
int LT_CAT(outlets_, LT_TAG)(const StepArgs &a, const NameBuf *name) {
  if (a.mode != kFused && a.mode != kCollideOnly) return kNoKernel;
  switch (a.coll) {
    case kCollNone: return pressure_outlets_of<kCollNone>(a, name);
    case kCollBgk: return pressure_outlets_of<kCollBgk>(a, name);
#if LT_HAS_KBC
    case kCollKbc: return pressure_outlets_of<kCollKbc>(a, name);
#endif
    case kCollSmagorinsky: case kCollTrt: case kCollRegularized: return LT_CAT(outlets2_, LT_TAG)(a, name);
    case kCollBgk | kCollForce: case kCollSmagorinsky | kCollForce: return LT_CAT(outlets3_, LT_TAG)(a, name);
#if LT_HAS_MRT
    case kCollMrt: case kCollMrtLallemand: return LT_CAT(mrt_outlets_, LT_TAG)(a, name);
#endif
    default: return kNoKernel;
  }
}
#elif LT_PART_IS(outlets2)
int LT_CAT(outlets2_, LT_TAG)(const StepArgs &a, const NameBuf *name) {
  if (a.coll == kCollSmagorinsky) return pressure_outlets_of<kCollSmagorinsky>(a, name);
  if (a.coll == kCollTrt) return pressure_outlets_of<kCollTrt>(a, name);
  if (a.coll == kCollRegularized) return pressure_outlets_of<kCollRegularized>(a, name);
  return kNoKernel;
}
#elif LT_PART_IS(outlets3)
int LT_CAT(outlets3_, LT_TAG)(const StepArgs &a, const NameBuf *name) {
  if (a.coll == (kCollBgk | kCollForce)) return pressure_outlets_of<kCollBgk | kCollForce>(a, name);
  if (a.coll == (kCollSmagorinsky | kCollForce)) return pressure_outlets_of<kCollSmagorinsky | kCollForce>(a, name);
  return kNoKernel;
}
#elif LT_PART_IS(mrt)
// one-step kernels only; the transform picks the kernels' COLL (api.hip, kernel_coll)
int LT_CAT(mrt_, LT_TAG)(const StepArgs &a, const NameBuf *name) {
  if (a.mode != kFused && a.mode != kCollideOnly) return kNoKernel;
  if (a.coll == kCollMrt) return one_step_of<kCollMrt>(a, name);
#if !LT_IS_3D
  if (a.coll == kCollMrtLallemand) return one_step_of<kCollMrtLallemand>(a, name);
#endif
  return kNoKernel;
}
#elif LT_PART_IS(incompressible)
// one-step kernels only; a.coll carries kCollIncompressible (api.hip, kernel_coll)
int LT_CAT(incompressible_, LT_TAG)(const StepArgs &a, const NameBuf *name) {
  if (a.mode != kFused && a.mode != kCollideOnly) return kNoKernel;
  if (a.coll == (kCollBgk | kCollIncompressible)) return one_step_incompressible_of<kCollBgk | kCollIncompressible>(a, name);
  if (a.coll == (kCollBgk | kCollForce | kCollIncompressible))
    return one_step_incompressible_of<kCollBgk | kCollForce | kCollIncompressible>(a, name);
  if (a.coll == (kCollTrt | kCollIncompressible)) return one_step_incompressible_of<kCollTrt | kCollIncompressible>(a, name);
  if (a.coll == (kCollRegularized | kCollIncompressible))
    return one_step_incompressible_of<kCollRegularized | kCollIncompressible>(a, name);
  return kNoKernel;
}

// lt_equilibrium (kAuxEquilibrium) and lt_init_fneq (kAuxFneq) of a plan with the incompressible equilibrium, reference layout
int LT_CAT(incompressible_aux_, LT_TAG)(const AuxArgs &a) {
  if (a.equilibrium != 1 || a.layout != 0) return kNoKernel;
  const unsigned grid = (unsigned)((a.N + kThreads - 1) / kThreads);
  if (a.what == kAuxEquilibrium) {
    hipLaunchKernelGGL((equilibrium_inc_kernel<T, S, 0>), dim3(grid), dim3(kThreads), 0, a.stream,
                       static_cast<const T *>(a.rho), static_cast<const T *>(a.u),
                       const_cast<T *>(static_cast<const T *>(a.f)), a.N, (T)a.rho0);
    return (int)hipGetLastError();
  }
  if constexpr (S::D >= 2) {
    if (a.what == kAuxFneq) {
      hipLaunchKernelGGL((fneq_inc_kernel<T, S>), dim3(grid), dim3(kThreads), 0, a.stream, static_cast<const T *>(a.rho),
                         static_cast<const T *>(a.u), const_cast<T *>(static_cast<const T *>(a.f)), a.n0, a.n1, a.n2,
                         (T)a.scale, (T)a.inv_dx, (T)a.rho0);
      return (int)hipGetLastError();
    }
  }
  return kNoKernel;
}
#elif LT_PART_IS(force_field)
// one-step kernels only; a.coll carries kCollField (api.hip, kernel_coll)
int LT_CAT(force_field_, LT_TAG)(const StepArgs &a, const NameBuf *name) {
  if (a.mode != kFused && a.mode != kCollideOnly) return kNoKernel;
  if (a.coll == (kCollBgk | kCollForce | kCollField)) return one_step_field_of<kCollBgk | kCollForce | kCollField>(a, name);
  if (a.coll == (kCollSmagorinsky | kCollForce | kCollField))
    return one_step_field_of<kCollSmagorinsky | kCollForce | kCollField>(a, name);
  return kNoKernel;
}
#elif LT_PART_IS(spectrum)
// lt_energy_spectrum (kAuxSpectrum): a.f the transformed fields, a.partial the caller's [a.reduce_blocks][a.n_bins] scratch;
// a.count modes per workgroup
int LT_CAT(spectrum_, LT_TAG)(const AuxArgs &a) {
  if (a.what != kAuxSpectrum || a.layout != 0 || a.n_bins < 1 || a.n_bins > kSpectrumMaxBins) return kNoKernel;
  hipLaunchKernelGGL((energy_spectrum_kernel<T, S::D>), dim3(a.reduce_blocks), dim3(kSpectrumThreads),
                     kSpectrumWaves * a.n_bins * sizeof(double), a.stream, static_cast<const T *>(a.f), a.n0, a.n1, a.n2,
                     a.count, a.n_bins, a.partial);
  hipLaunchKernelGGL(finish_spectrum_kernel<T>, dim3((a.n_bins + kSpectrumThreads - 1) / kSpectrumThreads),
                     dim3(kSpectrumThreads), 0, a.stream, a.partial, a.reduce_blocks, a.n_bins, a.scale, a.out);
  return (int)hipGetLastError();
}
#elif LT_PART_IS(boundary_force)
// lt_boundary_force (kAuxBoundaryForce): a.f the dense populations, a.mask the solid bytes, a.partial the caller's
// [3][a.reduce_blocks] scratch, a.out three doubles
int LT_CAT(boundary_force_, LT_TAG)(const AuxArgs &a) {
  if (a.what != kAuxBoundaryForce || a.layout != 0 || a.reduce_blocks < 1 || a.reduce_blocks > kForceMaxBlocks) return kNoKernel;
  hipLaunchKernelGGL((boundary_force_kernel<T, S>), dim3(a.reduce_blocks), dim3(kForceThreads), 0, a.stream,
                     static_cast<const T *>(a.f), a.mask, a.N, a.n0, a.n1, a.n2, a.partial);
  hipLaunchKernelGGL((finish_components_kernel<T, S::D>), dim3(1), dim3(kForceThreads), 0, a.stream, a.partial,
                     a.reduce_blocks, a.out);
  return (int)hipGetLastError();
}
#elif LT_PART_IS(links)
// lt_apply_links and step() (kLinkBounce), lt_link_force (kLinkForce): a.f the populations, the list in plan-owned memory
int LT_CAT(links_, LT_TAG)(const LinkArgs &a) {
  const LinkList<T> l = {a.node, a.dir, static_cast<const T *>(a.c1), static_cast<const T *>(a.c2), a.second, a.n_links};
  const LinkTable t = link_table<S>();
  if (a.what == kLinkBounce) {
    if (a.n_links < 1) return 0;
    const unsigned grid = ((unsigned)a.n_links + kLinkThreads - 1) / kLinkThreads;
    hipLaunchKernelGGL((link_bounce_kernel<T, S>), dim3(grid), dim3(kLinkThreads), 0, a.stream, static_cast<T *>(a.f),
                       a.stride, l, a.n0, a.n1, a.n2, t);
    return (int)hipGetLastError();
  }
  if (a.what != kLinkForce || a.blocks < 0 || a.blocks > kLinkMaxBlocks) return kNoKernel;
  if (a.blocks > 0)
    hipLaunchKernelGGL((link_force_kernel<T, S>), dim3(a.blocks), dim3(kLinkThreads), 0, a.stream,
                       static_cast<const T *>(a.f), a.stride, l, a.n0, a.n1, a.n2, t, a.partial);
  hipLaunchKernelGGL((finish_components_kernel<T, S::D>), dim3(1), dim3(kLinkThreads), 0, a.stream, a.partial, a.blocks,
                     a.out);
  return (int)hipGetLastError();
}
#elif LT_PART_IS(mrt_outlets)
int LT_CAT(mrt_outlets_, LT_TAG)(const StepArgs &a, const NameBuf *name) {
  if (a.coll == kCollMrt) return pressure_outlets_of<kCollMrt>(a, name);
#if !LT_IS_3D
  if (a.coll == kCollMrtLallemand) return pressure_outlets_of<kCollMrtLallemand>(a, name);
#endif
  return kNoKernel;
}
#endif

}  // namespace lt
