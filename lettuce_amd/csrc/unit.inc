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

// LT_PART names the object of the unit that is being built (Makefile: build/inst<N>_<tag>.o).  Which collisions a part
// holds: its list below; which kernels of a collision exist: one_step_exists and sweep_exists.  Here: why it is an object
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
//   forced (inst5_)       every unit: the kernels with a uniform body force (the kernels' COLL | kCollForce), one-step
//                         and the plain two-step sweep -- objects of their own, so that the objects of the unforced
//                         kernels are what they were
//   relaxations (inst6_)  every unit: the TRT and the regularised collision, one-step and the plain two-step sweep -- the
//                         earlier objects stay what they were and none of these is the longest job
//   outlets (inst7_)      every unit: the one-step kernels of plans with a constant-pressure outlet (EquilibriumOutletP;
//                         the kernels' ABBD = kOutletsP + chain), so that every plan without such an outlet launches the
//                         code it launched before.  This object: the entry point, which passes on to the next three
//   outlets2 (inst8_), outlets3 (inst9_)  ... three objects, because the chain of depth 2 inlines the gather and the
//                         collision three times and one object per unit would be the longest job
//   mrt (inst10_)         units with LT_HAS_MRT: the multiple-relaxation-time collision (kCollMrt: Dellar on D2Q9,
//                         Hermite on D3Q27; kCollMrtLallemand: Lallemand on D2Q9); no launch of several steps
//   mrt_outlets (inst11_) ... and its kernels of plans with a constant-pressure outlet
//   incompressible (inst12_)  every unit: the kernels of the incompressible equilibrium (the kernels' COLL |
//                         kCollIncompressible), and the equilibrium and f_neq kernels; no launch of several steps
//   spectrum (inst13_)    2-D and 3-D units: the two launches of the energy spectrum (spectrum.hpp), which depend on the
//                         scalar type and the dimension only
//   boundary_force (inst14_)  2-D and 3-D units: the two launches of the momentum-exchange force on a bounce-back body
//                         (boundary_force.hpp)
//   links (inst15_)       2-D and 3-D units: the pass of the interpolated bounce-back over a plan's link list and the two
//                         launches of the momentum-exchange force over it (link_bounce.hpp)
//   force_field (inst16_) every unit: the kernels with a body force whose acceleration is a per-node field (the kernels'
//                         COLL | kCollForce | kCollField); no launch of several steps
// (parts 12 to 16: objects of their own so that every other plan launches what it launched before)
// A part states the collision numbers it holds once: LT_COLLS_<part> those of its one-step kernels (which of their
// variants exist: one_step_exists, below; a collision the unit lacks, unit_has, is skipped), LT_SWEEPS_<part> those of its
// two-step sweeps (sweep_exists).  A new family: its list here, and its struct among the families below.
#if LT_IS_3D
#define LT_COLLS_main kCollNone, kCollBgk, kCollKbc
#else
#define LT_COLLS_main kCollNone, kCollBgk, kCollKbc, kCollSmagorinsky
#endif
#define LT_COLLS_smagorinsky kCollSmagorinsky
#define LT_COLLS_forced kCollBgk | kCollForce, kCollSmagorinsky | kCollForce
#define LT_COLLS_relaxations kCollTrt, kCollRegularized
#define LT_COLLS_outlets kCollNone, kCollBgk, kCollKbc
#define LT_COLLS_outlets2 kCollSmagorinsky, kCollTrt, kCollRegularized
#define LT_COLLS_outlets3 LT_COLLS_forced
#define LT_COLLS_mrt kCollMrt, kCollMrtLallemand
#define LT_COLLS_mrt_outlets LT_COLLS_mrt
#define LT_COLLS_incompressible                                                                               \
  kCollBgk | kCollIncompressible, kCollBgk | kCollForce | kCollIncompressible, kCollTrt | kCollIncompressible, \
      kCollRegularized | kCollIncompressible
#define LT_COLLS_force_field kCollBgk | kCollForce | kCollField, kCollSmagorinsky | kCollForce | kCollField
#define LT_SWEEPS_sweeps kCollNone, kCollBgk, kCollSmagorinsky
#define LT_SWEEPS_roles kCollBgk
#define LT_SWEEPS_forced kCollBgk | kCollForce
#define LT_SWEEPS_relaxations kCollTrt, kCollRegularized
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
// LT_ONE_STEP: the object holds the one-step launcher and its ladder; LT_SWEEP: the two-step sweep launcher
#define LT_ONE_STEP                                                                                                  \
  (LT_PART_IS(main) || LT_PART_IS(smagorinsky) || LT_PART_IS(forced) || LT_PART_IS(relaxations) || LT_PART_IS_OUTLETS || \
   LT_PART_IS(mrt) || LT_PART_IS(incompressible) || LT_PART_IS(force_field))
#define LT_SWEEP (LT_PART_IS(sweeps) || LT_PART_IS(roles) || LT_PART_IS(forced) || LT_PART_IS(relaxations))
#if !LT_ONE_STEP && !LT_SWEEP && !LT_PART_IS(spectrum) && !LT_PART_IS(boundary_force) && !LT_PART_IS(links)
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

// A launch's parameter block: zeroed, then every field that means the same to all launchers.  A launcher sets what is
// its own on top (the one-step kernels: their family's fill, below).  n2: the planes of the field (the 2-D launchers: 1)
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

// ---- The families of collisions ----
// A family: the parameter block its kernels take (kernels.hpp: a type of its own each, so that every other kernel keeps
// its argument block and with it its code), what a launch fills in beyond params_of, and which one-step variants the family
// has beside the plain kernels of the reference layout:
//   slab      the slab layout of a 3-D unit (multi-GPU z-slabs), and with it the packed plane launch
//   depths    the deepest chain of anti-bounce-back outlets (kernels.hpp, neighbour_moments DEPTH): 2 = all of them
//   pressure  the kernels of plans with a constant-pressure outlet (ABBD = kOutletsP + chain)
// A new family is one struct here, one line in FamilyOf and one list for its part (LT_COLLS_<part>, above).
struct Quadratic {      // none, BGK, KBC, Smagorinsky, TRT, the regularised collision: every variant there is
  using P = KParams<T>;
  static constexpr bool slab = true, pressure = true;
  static constexpr int depths = 2;
  template <int LAYOUT>
  static void fill(P &, const StepArgs &) {}
};
// uniform body force (lt_plan_set_force; 5, 7): every variant BGK has.  The acceleration permuted from the logical order
// x, y, z to the memory axes of the layout, as the kernels read the velocity
struct Forced : Quadratic {
  using P = KParamsF<T>;
  template <int LAYOUT>
  static void fill(P &p, const StepArgs &a) {
    using M = MemMap<S, LAYOUT>;
    p.accel[0] = p.accel[1] = p.accel[2] = T(0);
    p.shift[0] = p.shift[1] = p.shift[2] = T(0);
    for (int c = 0; c < S::D; ++c) {
      p.accel[M::memory(c)] = (T)a.accel[c];
      p.shift[M::memory(c)] = (T)a.ueq_scale * (T)a.accel[c];     // guo.py:27-29: the product in the tensor's precision
    }
    p.source_scale = (T)a.source_scale;
  }
};
// MRT (lt_plan_set_mrt; 10, 11): every variant BGK has.  r_i = 1 / s_i with both the rate and the quotient in T -- the
// reference converts the rates to the context's dtype and divides there on every call (mrt_collision.py:18-24)
struct Mrt : Quadratic {
  using P = KParamsM<T>;
  template <int LAYOUT>
  static void fill(P &p, const StepArgs &a) {
    for (int i = 0; i < kMrtMaxQ; ++i) p.r[i] = i < S::Q ? T(1) / (T)a.mrt_rates[i] : T(0);
  }
};
// the incompressible equilibrium (lt_plan_set_equilibrium, which refuses slab plans and the constant-pressure outlet; 17,
// 24, 25 and with a body force 21): the reference layout with its outlet depths.  rho0 rounded once, as a Python float
// times a tensor of the plan's dtype is
template <class Base, class Block>
struct Incompressible : Base {
  using P = Block;
  static constexpr bool slab = false, pressure = false;
  template <int LAYOUT>
  static void fill(P &p, const StepArgs &a) {
    Base::template fill<LAYOUT>(p, a);
    p.rho0 = (T)a.rho0;
  }
};
// per-node body force (lt_plan_set_force_field, which refuses slab plans and every outlet; 37, 39): the reference layout
// without the outlet depths.  The field and the two scales, each rounded to T once as the uniform force rounds them; the
// kernels form the node's shift (kernels.hpp, load_node_force)
struct ForceField : Quadratic {
  using P = KParamsFF<T>;
  static constexpr bool slab = false, pressure = false;
  static constexpr int depths = 0;
  template <int LAYOUT>
  static void fill(P &p, const StepArgs &a) {
    p.accel_field = static_cast<const T *>(a.accel_field);
    p.ueq_scale = (T)a.ueq_scale;
    p.source_scale = (T)a.source_scale;
  }
};
template <int COLL>
using FamilyOf =
    std::conditional_t<coll_field(COLL), ForceField,
    std::conditional_t<coll_incompressible(COLL), std::conditional_t<coll_forced(COLL), Incompressible<Forced, KParamsFI<T>>,
                                                                     Incompressible<Quadratic, KParamsI<T>>>,
    std::conditional_t<coll_forced(COLL), Forced, std::conditional_t<coll_mrt(COLL), Mrt, Quadratic>>>>;
template <int COLL>
using ParamsOf = typename FamilyOf<COLL>::P;

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

// ---- Which one-step kernels exist ----
// The collisions of the unit: KBC where the lattice has it, the MRT transforms of mrt.hpp (Lallemand on D2Q9 only)
constexpr bool unit_has(int coll) {
  if (coll == kCollKbc) return LT_HAS_KBC;
  if (coll_mrt(coll)) return LT_HAS_MRT && (coll == kCollMrt || !LT_IS_3D);
  return true;
}

// Plans with a constant-pressure outlet, alone or beside anti-bounce-back outlets, have one chain depth per layout, the
// deepest a plan of that layout can need (api.hip, abb_depth_of): outlets on all three axes in the reference layout of a
// 3-D unit (2), on two axes in the slab layout and in 2-D (1); two outlets on the one axis of a 1-D lattice count as
// depth 1 too (on a lattice of two nodes each outlet's neighbour lies in the other's plane).  A plan with fewer axes or
// one outlet takes the same kernel: the chain is followed only where a lower outlet's plane holds the neighbour.
constexpr int outlet_chain(int d, int layout) { return d == 3 && layout == 0 ? 2 : 1; }

// Whether the library has lbm_kernel<T, S, LAYOUT, COLL, MODE's STREAM and COLLIDE, MASKED, 1, 0, TUNE, PACK, ABBD> on a
// lattice of d dimensions: the one statement of the set.  one_step_of instantiates what holds here and nothing else.
// Product kernels, one node per thread (VEC = 1).  Measured on MI355X (profiles/r01_variant_sweep*): for this 2q-stream
// kernel 8 waves/SIMD of scalar accesses beat 16-byte accesses at 3-4 waves/SIMD by 8-13 %, and nontemporal stores
// (+3-4 %) and loads (+1.6 %) help once the populations exceed the caches (TUNE 3).  TUNE 0 (cached accesses) is kept
// for grids that fit in L2 / Infinity Cache.
template <int COLL>
constexpr bool one_step_exists(int d, int layout, int mode, bool masked, int tune, bool pack, int abbd) {
  using F = FamilyOf<COLL>;
  if (!unit_has(COLL)) return false;
  // the slab layout: 3-D units
  if (layout != 0 && !(layout == 1 && d == 3 && F::slab)) return false;
  // the slab boundary-plane launch with fused halo packing: fused, cached accesses; otherwise both cache policies
  if (pack ? !(layout == 1 && mode == kFused && tune == 0) : !(tune == 0 || tune == 3)) return false;
  // the one kernel that does not collide: no outlet depth (streaming alone applies no boundary)
  if (mode == kStreamOnly) return COLL == kCollNone && abbd == 0;
  if (mode != kFused && mode != kCollideOnly) return false;
  if (abbd == 0) return true;
  // the outlet depths: masked kernels that apply boundaries, i.e. fused and collide-only
  if (!masked) return false;
  // plans with a constant-pressure outlet: both cache policies and the packed launch
  if (abbd == kOutletsP + outlet_chain(d, layout)) return F::pressure;
  if (abbd > F::depths || tune != 0 || pack) return false;
  // two anti-bounce-back outlets (DEPTH 1): both layouts; outlets on all three axes of a 3-D flow (their planes meet in
  // corners: DEPTH 2): reference layout
  return abbd == 1 || (abbd == 2 && d == 3 && layout == 0);
}

// one node per thread: the kernels' VEC = 1, SHIFT = 0
template <int LAYOUT, int COLL, int MODE, bool MASKED, int TUNE = 0, bool PACK = false, int ABBD = 0>
int launch(const StepArgs &a, const NameBuf *name) {
  static_assert(one_step_exists<COLL>(S::D, LAYOUT, MODE, MASKED, TUNE, PACK, ABBD), "a kernel of the set above");
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
  FamilyOf<COLL>::template fill<LAYOUT>(p, a);
  p.abb0_slot = a.n0 % 64 == 0 ? a.abb0_slot : 0;
  if (p.nvec_total == 0) return 0;
  const unsigned grid = (p.nvec_total + kThreads - 1) / kThreads;
  // a.lds_bytes of dynamic LDS that no kernel touches: caps the workgroups resident per CU
  // (lt_plan_set_residency)
  hipLaunchKernelGGL(kern, dim3(grid), dim3(kThreads), (unsigned)a.lds_bytes, a.stream, p);
  return (int)hipGetLastError();
}

// ---- The one ladder ----
// A one-step kernel's template axes as one number: the variant is the cache policy 0 or 3, or the packed launch; the
// depth slot is ABBD 0, 1, 2 or kOutletsP + 1, kOutletsP + 2
// how many values each axis has: layouts, modes (fused, collide-only, stream-only), masked, variants, depth slots
constexpr int kLayouts = 2, kModes = 3, kMaskings = 2, kVariants = 3, kSlots = 5;
constexpr int kOneSteps = kLayouts * kModes * kMaskings * kVariants * kSlots;
struct OneStep {
  int layout, mode, masked, variant, slot;
  constexpr int index() const { return (((layout * kModes + mode) * kMaskings + masked) * kVariants + variant) * kSlots + slot; }
  constexpr int tune() const { return variant == 1 ? 3 : 0; }
  constexpr bool pack() const { return variant == 2; }
  constexpr int abbd() const { return slot < 3 ? slot : kOutletsP + slot - 2; }
};
constexpr OneStep one_step_at(int i) {
  return {i / (kSlots * kVariants * kMaskings * kModes), i / (kSlots * kVariants * kMaskings) % kModes,
          i / (kSlots * kVariants) % kMaskings, i / kSlots % kVariants, i % kSlots};
}
constexpr bool one_steps_numbered() {
  for (int i = 0; i < kOneSteps; ++i)
    if (one_step_at(i).index() != i || one_step_at(i).layout >= kLayouts) return false;
  return true;
}
static_assert(one_steps_numbered(), "index() and one_step_at() are inverses over all candidates");

// candidate I of collision C: launched (or named) if this object has it and the arguments want it.  An outlets part
// holds the kernels of the plans with a constant-pressure outlet, every other part the rest
template <int C, int I>
bool take(int wanted, const StepArgs &a, const NameBuf *name, int &result) {
  constexpr OneStep k = one_step_at(I);
  if constexpr ((k.abbd() > kOutletsP) == (LT_PART_IS_OUTLETS != 0) &&
                one_step_exists<C>(S::D, k.layout, k.mode, k.masked != 0, k.tune(), k.pack(), k.abbd())) {
    if (wanted != I) return false;
    result = launch<k.layout, C, k.mode, (k.masked != 0), k.tune(), k.pack(), k.abbd()>(a, name);
    return true;
  } else {
    return false;
  }
}
template <int C, int... I>
int take_any(int wanted, const StepArgs &a, const NameBuf *name, std::integer_sequence<int, I...>) {
  int result = kNoKernel;
  (void)(take<C, I>(wanted, a, name, result) || ...);
  return result;
}

// The one-step kernel of collision C that the arguments select: what they want, derived once, then the walk over the
// set.  Launching and naming are the same path down to launch(), so a plan's kernel name is the kernel a launch takes.
template <int C>
int one_step_of(const StepArgs &a, const NameBuf *name) {
  using F = FamilyOf<C>;
  if (a.layout < 0 || a.layout > 1 || a.mode < kFused || a.mode > kStreamOnly) return kNoKernel;
  if constexpr (coll_field(C)) {
    if (!a.accel_field && !name) return kNoKernel;      // a launch reads the field
  }
  OneStep w = {a.layout, a.mode, a.masked != 0, a.tune == 0 ? 0 : (a.tune == 3 ? 1 : -1), 0};
  if (a.mode != kStreamOnly) {      // streaming alone applies no boundary: no check of the outlets
    // a family without the slab layout takes no message buffer, one without outlet depths no outlet
    if (!F::slab && (a.pack_lo || a.pack_hi)) return kNoKernel;
    if (F::depths == 0 && (a.n_abb > 0 || a.abb_depth > 0)) return kNoKernel;
    if (a.abb_depth < 0 || a.abb_depth > 2) return kNoKernel;
    const int chain = outlet_chain(S::D, a.layout);
    if (a.n_pout > 0) {
      // a constant-pressure outlet: the chain kernel of the layout, which covers every depth up to its own
      if (!a.masked || a.abb_depth > chain) return kNoKernel;
      w.slot = 2 + chain;
    } else if (a.masked || a.abb_depth > 1) {
      // without masks nothing applies an outlet: depth 1 takes the plain kernel, depth 2 has none
      w.slot = a.abb_depth;
    }
    // the depths of the anti-bounce-back outlets and the packed launch ignore a.tune; a.tune == 1 has no plain kernel.
    // Packed comes before the plain slab set, and only at depth 0 or with a constant-pressure outlet
    if (w.slot == 1 || w.slot == 2) w.variant = 0;
    else if (a.layout == 1 && a.mode == kFused && a.pack_lo != nullptr && (a.abb_depth == 0 || a.n_pout > 0)) w.variant = 2;
  }
  if (w.variant < 0) return kNoKernel;
  return take_any<C>(w.index(), a, name, std::make_integer_sequence<int, kOneSteps>());
}

template <int... C>
constexpr bool is_one_of(int coll) { return ((coll == C) || ...); }

// the collision of the list that is `coll` (the arguments', or none for a launch that only streams)
template <int... C>
int one_step_in(int coll, const StepArgs &a, const NameBuf *name) {
  int result = kNoKernel;
  (void)((coll == C && ((result = one_step_of<C>(a, name)), true)) || ...);
  return result;
}

#endif  // LT_ONE_STEP

#if LT_SWEEP
// ---- Which two-step sweeps exist ----
// Whether the unit has lbm2_kernel<T, S, LAYOUT, COLL, W, R, 1, MODE, 1, SCHED> on its tile of W x R nodes (kTile): the
// one statement of the set.  sweep_in instantiates what holds here and nothing else.
constexpr bool sweep_exists(int coll, int layout, int mode, int sched) {
  if (S::D != 3 || kTile.rows == 0 || layout < 0 || layout > 1) return false;
  // MODE 1: the slab edge launch with fused halo packing; MODE 2: the whole slab, edge workgroups first -- slab layout
  if (mode != 0 && !(layout == 1 && (mode == 1 || mode == 2))) return false;
  // SCHED 1: separate producer and consumer waves (twostep_roles.hpp) -- plain BGK, where they won their A/B (DESIGN.md
  // section 7)
  if (sched != 0) return sched == 1 && LT_HAS_ROLES && coll == kCollBgk && mode == 0;
  if (coll == kCollNone || coll == kCollBgk) return true;
  // Smagorinsky, BGK with a body force, TRT and the regularised collision: the plain one-role sweep of D3Q19 fp32 -- no
  // edge launch with packing, no signalling launch.  (Smagorinsky with a force, COLL 7: 168 VGPRs and 84-92 bytes of
  // scratch per lane under every scheduler setting where the unforced sweep has 168 and none -- not built, the plan
  // keeps the one-step kernel: DESIGN.md section 4)
  return (coll == kCollSmagorinsky || coll == (kCollBgk | kCollForce) || coll == kCollTrt || coll == kCollRegularized) &&
         S::Q == 19 && sizeof(T) == 4 && mode == 0;
}

// Two fused steps per launch (kernels.hpp, lbm2_kernel): whole periodic grid, no masks.
// returns kNoKernel when the grid does not tile.
// one node per thread and per block: the kernel's NPT = NPB = 1
template <int LAYOUT, int COLL, int T0, int T1, int MODE, int SCHED>
int launch_twice(const StepArgs &a, const NameBuf *name) {
  static_assert(sweep_exists(COLL, LAYOUT, MODE, SCHED) && T0 == kTile.width && T1 == kTile.rows, "a sweep of the set above");
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
  FamilyOf<COLL>::template fill<LAYOUT>(p, a);
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
}

// candidate I (layout and mode) of collision C, in this object's schedule
template <int C, int I>
bool take_sweep(int wanted, const StepArgs &a, const NameBuf *name, int &result) {
  constexpr int SCHED = LT_PART_IS(roles) ? 1 : 0;
  if constexpr (sweep_exists(C, I / 3, I % 3, SCHED)) {
    if (wanted != I) return false;
    result = launch_twice<I / 3, C, kTile.width, kTile.rows, I % 3, SCHED>(a, name);
    return true;
  } else {
    return false;
  }
}
template <int C, int... I>
bool sweep_of(int wanted, const StepArgs &a, const NameBuf *name, int &result, std::integer_sequence<int, I...>) {
  return a.coll == C && (take_sweep<C, I>(wanted, a, name, result) || ...);
}

// the sweep of the list's collisions that the arguments select
template <int... C>
int sweep_in(const StepArgs &a, const NameBuf *name) {
#if LT_PART_IS(forced) || LT_PART_IS(relaxations)
  // plain sweeps of periodic plans (no packing, no signalling launch)
  if (a.masked || a.pack_lo || a.pack_hi || a.signal) return kNoKernel;
#elif LT_PART_IS(sweeps) && LT_HAS_ROLES
  // the plain BGK sweep: part roles; shift policy 6 runs the one-role schedule (A/B)
  if (a.coll == kCollBgk && a.shift != 6 && (a.layout == 0 || !(a.pack_lo || a.pack_hi || a.signal)))
    return LT_CAT(roles_, LT_TAG)(a, name);
#endif
  if (a.layout < 0 || a.layout > 1) return kNoKernel;
  // the slab's edge launch where there is a message buffer, else its signalling launch where there is a signal
  const int mode = a.layout == 0 ? 0 : ((a.pack_lo || a.pack_hi) ? 1 : (a.signal ? 2 : 0));
  int result = kNoKernel;
  (void)(sweep_of<C>(a.layout * 3 + mode, a, name, result, std::make_integer_sequence<int, 6>()) || ...);
  return result;
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
#if LT_IS_3D
  if (coll == kCollSmagorinsky) return LT_CAT(smag_, LT_TAG)(a, name);       // part smagorinsky
#endif
  return one_step_in<LT_COLLS_main>(coll, a, name);
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
int LT_CAT(twice_, LT_TAG)(const StepArgs &a, const NameBuf *name) { return sweep_in<LT_SWEEPS_sweeps>(a, name); }
#elif LT_PART_IS(roles)
int LT_CAT(roles_, LT_TAG)(const StepArgs &a, const NameBuf *name) { return sweep_in<LT_SWEEPS_roles>(a, name); }
#elif LT_PART_IS(smagorinsky)
int LT_CAT(smag_, LT_TAG)(const StepArgs &a, const NameBuf *name) { return one_step_in<LT_COLLS_smagorinsky>(a.coll, a, name); }
#elif LT_PART_IS(forced)
int LT_CAT(forced_, LT_TAG)(const StepArgs &a, const NameBuf *name) {
  if (a.mode == kFusedTwice) return sweep_in<LT_SWEEPS_forced>(a, name);
  return one_step_in<LT_COLLS_forced>(a.coll, a, name);
}
#elif LT_PART_IS(relaxations)
int LT_CAT(relax_, LT_TAG)(const StepArgs &a, const NameBuf *name) {
  if (a.mode == kFusedTwice) return sweep_in<LT_SWEEPS_relaxations>(a, name);
  return one_step_in<LT_COLLS_relaxations>(a.coll, a, name);
}
#elif LT_PART_IS(outlets)
// the entry point of the outlets parts: its own collisions, else on to the part whose list has a.coll
int LT_CAT(outlets_, LT_TAG)(const StepArgs &a, const NameBuf *name) {
  if (is_one_of<LT_COLLS_outlets2>(a.coll)) return LT_CAT(outlets2_, LT_TAG)(a, name);
  if (is_one_of<LT_COLLS_outlets3>(a.coll)) return LT_CAT(outlets3_, LT_TAG)(a, name);
#if LT_HAS_MRT
  if (is_one_of<LT_COLLS_mrt_outlets>(a.coll)) return LT_CAT(mrt_outlets_, LT_TAG)(a, name);
#endif
  return one_step_in<LT_COLLS_outlets>(a.coll, a, name);
}
#elif LT_PART_IS(outlets2)
int LT_CAT(outlets2_, LT_TAG)(const StepArgs &a, const NameBuf *name) { return one_step_in<LT_COLLS_outlets2>(a.coll, a, name); }
#elif LT_PART_IS(outlets3)
int LT_CAT(outlets3_, LT_TAG)(const StepArgs &a, const NameBuf *name) { return one_step_in<LT_COLLS_outlets3>(a.coll, a, name); }
#elif LT_PART_IS(mrt_outlets)
int LT_CAT(mrt_outlets_, LT_TAG)(const StepArgs &a, const NameBuf *name) { return one_step_in<LT_COLLS_mrt_outlets>(a.coll, a, name); }
#elif LT_PART_IS(mrt)
int LT_CAT(mrt_, LT_TAG)(const StepArgs &a, const NameBuf *name) { return one_step_in<LT_COLLS_mrt>(a.coll, a, name); }
#elif LT_PART_IS(force_field)
int LT_CAT(force_field_, LT_TAG)(const StepArgs &a, const NameBuf *name) { return one_step_in<LT_COLLS_force_field>(a.coll, a, name); }
#elif LT_PART_IS(incompressible)
int LT_CAT(incompressible_, LT_TAG)(const StepArgs &a, const NameBuf *name) { return one_step_in<LT_COLLS_incompressible>(a.coll, a, name); }

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
#endif

}  // namespace lt
