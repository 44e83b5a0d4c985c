// What a launch of several steps needs from a lattice, a scalar type and a grid: the one statement that both the
// admission of a plan (api.hip) and the launchers of a unit (unit.inc) read.  Host / constexpr code only; the kernels
// take their tile geometry (TwoStep) from here.
#pragma once
#include <stddef.h>

#include "dispatch.hpp"
#include "lattice.hpp"

namespace lt {

// ---- LDS ----
// what a workgroup can have of a CU's LDS; also what the residency cap of the one-step kernels divides (api.hip, resolve_lds)
constexpr size_t kLdsBudget = 160 * 1024;

// geometry of a two-step tile of T0 x T1 output nodes (kernels.hpp, lbm2_kernel; twostep_masked.hpp, lbm2m_kernel)
template <typename T, class S, int T0_, int T1>
struct TwoStep {
  static constexpr int T0 = T0_, H0 = T0 + 2, H1 = T1 + 2;
  static constexpr int NI = H0 * H1;                    // intermediate nodes per plane
  static constexpr int NO = T0 * T1;                    // output nodes per plane
  static constexpr int THREADS = (NI + 63) / 64 * 64;
  template <int LAYOUT, int E2>
  static constexpr int count() {                        // populations with e along a2 == E2
    int n = 0;
    for (int q = 0; q < S::Q; ++q) n += MemMap<S, LAYOUT>::e(q, 2) == E2 ? 1 : 0;
    return n;
  }
};

// LDS bytes of lbm2_kernel: 4 slots of the upward, 3 of the in-plane, 2 of the downward populations -- as many upward as
// downward ones (asserted below), so three planes of all populations
template <typename T, class S, int T0, int T1>
constexpr size_t two_step_lds() {
  return sizeof(T) * 3 * S::Q * (size_t)TwoStep<T, S, T0, T1>::NI;
}

// LDS bytes of lbm2m_kernel: 4 slots of the upward, 3 of the in-plane, 3 of the downward populations, and the
// populations of two uniform equilibrium boundaries
constexpr int kEqCached = 2;
template <typename T, class S, int LAYOUT, int T0, int T1>
constexpr size_t two_step_masked_lds() {
  using B = TwoStep<T, S, T0, T1>;
  return sizeof(T) * ((size_t)B::NI * (4 * B::template count<LAYOUT, 1>() + 3 * B::template count<LAYOUT, 0>() +
                                       3 * B::template count<LAYOUT, -1>()) + (size_t)kEqCached * S::Q);
}

// the footprints do not depend on the layout: both sweep axes (x and z) cross the same number of populations
template <class S>
constexpr bool crossing_counts_agree() {
  using B = TwoStep<float, S, 64, 8>;
  return B::template count<0, 1>() == B::template count<1, 1>() && B::template count<0, 0>() == B::template count<1, 0>() &&
         B::template count<0, -1>() == B::template count<1, -1>() && B::template count<0, 1>() == B::template count<0, -1>();
}
static_assert(crossing_counts_agree<D3Q15>() && crossing_counts_agree<D3Q19>() && crossing_counts_agree<D3Q27>(),
              "a lattice crosses its planes alike in both layouts and in both directions");

// ---- the 3-D two-step tile of a unit ----
// Rows of 256 bytes (64 fp32 / 32 fp64 nodes -- narrower rows measured 12-39 % slower) and 8 of them if the kernel's LDS
// fits the budget, otherwise 4 in fp32 only (D3Q27 fp32: 0.63 -> 0.49 ms per update at 256^3; D3Q27 fp64 would fit 32 x 4
// tiles but measured slower than one step, 1.40 against 1.23 ms, and is not built), otherwise none.  With masks the
// downward populations have a third slot: where the same rows then exceed the budget there is no masked kernel (D3Q19
// fp64: 8 rows need 168 944 B, and 4-row fp64 tiles lost their A/B).  rows = 0: no kernel.
struct UnitTile {
  int width, rows, rows_masked;
};
template <class S, typename T>
constexpr UnitTile two_step_tile() {
  if constexpr (S::D != 3) {
    return {0, 0, 0};
  } else {
    constexpr int W = 256 / (int)sizeof(T);
    constexpr int R = two_step_lds<T, S, W, 8>() <= kLdsBudget ? 8
                      : (sizeof(T) == 4 && two_step_lds<T, S, W, 4>() <= kLdsBudget ? 4 : 0);
    if constexpr (R == 0) return {W, 0, 0};
    else return {W, R, two_step_masked_lds<T, S, 0, W, R>() <= kLdsBudget ? R : 0};
  }
}

// ---- the 2-D two-step strips (twostep2d.hpp) ----
// columns per workgroup, widest first: a launch takes the widest that divides the contiguous extent
#define LT_STRIP_WIDTHS(X) X(512) X(256) X(128) X(64)
#define LT_STRIP_ITEM(W) W,
constexpr int kStripWidths[] = {LT_STRIP_WIDTHS(LT_STRIP_ITEM)};
#undef LT_STRIP_ITEM
constexpr int strip_width(int n0) {
  for (const int w : kStripWidths)
    if (n0 % w == 0) return w;
  return 0;
}

// the tile of a two-step launch on a grid of contiguous extent n0: a 3-D unit's own, a 2-D unit's strip as one "row"
struct TwoStepTile {
  int width, rows;
};
constexpr TwoStepTile two_step_tile_on(const UnitTile &unit, int d, int n0, bool masked) {
  if (d == 2) return strip_width(n0) ? TwoStepTile{strip_width(n0), 1} : TwoStepTile{0, 0};
  return {unit.width, masked ? unit.rows_masked : unit.rows};
}
constexpr bool tiles(const TwoStepTile &t, int n0, int n1) { return t.rows > 0 && n0 % t.width == 0 && n1 % t.rows == 0; }

// ---- several steps per launch on small 2-D grids (kernels.hpp, lbm_many_kernel) ----
// tiles of kManyTile x kManyTile nodes and up to kManyMax steps; a plan with an outlet recomputes one more ring of nodes
// around each tile: one step fewer
constexpr int kManyTile = 8, kManyMax = 8;
constexpr int many_steps_max(bool outlet) { return kManyMax - (outlet ? 1 : 0); }

// ---- addressing: the 3-D two-step kernels form 32-bit byte offsets ----
constexpr long long kOffsetRange = 1ll << 32;
// lbm2_kernel: within a plane
constexpr bool plane_addressable(long long n0, long long n1, long long esize) { return n0 * n1 * esize < kOffsetRange; }
// lbm2m_kernel (buffer instructions): within the whole field of q populations `distance` elements apart, or -- where the
// instantiation with a descriptor per population exists (BIG: BGK in the reference layout, up to 19 populations; D3Q27's
// 2 x 27 population bases spill) -- within a population
constexpr bool masked_per_population(int layout, int coll, int q) { return layout == 0 && coll == kCollBgk && q <= 19; }
constexpr bool field_addressable(int q, long long distance, long long esize, bool per_population) {
  return (per_population ? 1ll : (long long)q) * distance * esize < kOffsetRange;
}

// ---- the small minima ----
// planes (2-D: rows) per workgroup of a sweep: with masks the outlet's plane never opens a segment
constexpr int min_segment(bool masked) { return masked ? 2 : 1; }
// planes / rows of the sweep axis where an outlet may lie on it (the outlet's plane, its neighbour, and one more)
constexpr int kOutletSweepMin = 3;
// boundaries of a masked two-step plan: slot 0 is "no boundary", and MaskedPlanInfo packs two bits of kind per slot
constexpr int kMaskedTwoStepBoundaries = 15;

}  // namespace lt
