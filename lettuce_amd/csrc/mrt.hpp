// Multiple-relaxation-time collision (lettuce/ext/_collision/mrt_collision.py:21-27) for the three moment transforms
// of the reference that have an equilibrium of their own (lettuce/util/moments.py: D2Q9Dellar, D2Q9Lallemand,
// D3Q27Hermite):
//   m = M f,   m_i <- m_i - r_i (m_i - meq_i(m)),   f = M^-1 m.
// The matrices are compile-time tables, walked by static_for: a zero entry costs nothing, +-1 is an add / subtract,
// every other entry is the double of the reference's table rounded to T (as Context.convert_to_tensor rounds it).  The
// sums run in ascending index; the reference's are GEMMs whose order is not specified, so MRT is compared with the
// reference at rounding level, not bit for bit (one engine kernel against another is bit for bit).  meq follows the
// reference's closed forms in its order of operations, oddities included.  The conserved moments (rho, j) have
// meq_i = m_i: their relaxation is skipped, whatever their rate.  r_i = 1 / s_i is formed on the host in the plan's
// scalar type (unit.inc), as the reference divides in the context's dtype.
//
// Needs nothing but lattice.hpp, so that tests/aux/mrt_host.cpp compiles it for the host.
#pragma once
#include "lattice.hpp"

namespace lt {

// == lt_mrt_transform (include/lettuce_hip.h)
constexpr int kMrtDellar = 1, kMrtLallemand = 2, kMrtHermite = 3;
constexpr int kMrtMaxQ = 27;

template <int TRANSFORM>
struct MrtTables;

// Dellar's D2Q9 basis: rho, jx, jy, Pi_xx, Pi_xy, Pi_yy, N, Jx, Jy
template <>
struct MrtTables<kMrtDellar> {
  static constexpr int Q = 9, CONSERVED = 3;
  static constexpr double M[9][9] = {
      {1, 1, 1, 1, 1, 1, 1, 1, 1},
      {0, 1, 0, -1, 0, 1, -1, -1, 1},
      {0, 0, 1, 0, -1, 1, 1, -1, -1},
      {-3.0 / 2, 3, -3.0 / 2, 3, -3.0 / 2, 3, 3, 3, 3},
      {0, 0, 0, 0, 0, 9, -9, 9, -9},
      {-3.0 / 2, -3.0 / 2, 3, -3.0 / 2, 3, 3, 3, 3, 3},
      {1, -2, -2, -2, -2, 4, 4, 4, 4},
      {0, -2, 0, 2, 0, 4, -4, -4, 4},
      {0, 0, -2, 0, 2, 4, 4, -4, -4}};
  static constexpr double MINV[9][9] = {
      {4.0 / 9, 0, 0, -4.0 / 27, 0, -4.0 / 27, 1.0 / 9, 0, 0},
      {1.0 / 9, 1.0 / 3, 0, 2.0 / 27, 0, -1.0 / 27, -1.0 / 18, -1.0 / 12, 0},
      {1.0 / 9, 0, 1.0 / 3, -1.0 / 27, 0, 2.0 / 27, -1.0 / 18, 0, -1.0 / 12},
      {1.0 / 9, -1.0 / 3, 0, 2.0 / 27, 0, -1.0 / 27, -1.0 / 18, 1.0 / 12, 0},
      {1.0 / 9, 0, -1.0 / 3, -1.0 / 27, 0, 2.0 / 27, -1.0 / 18, 0, 1.0 / 12},
      {1.0 / 36, 1.0 / 12, 1.0 / 12, 1.0 / 54, 1.0 / 36, 1.0 / 54, 1.0 / 36, 1.0 / 24, 1.0 / 24},
      {1.0 / 36, -1.0 / 12, 1.0 / 12, 1.0 / 54, -1.0 / 36, 1.0 / 54, 1.0 / 36, -1.0 / 24, 1.0 / 24},
      {1.0 / 36, -1.0 / 12, -1.0 / 12, 1.0 / 54, 1.0 / 36, 1.0 / 54, 1.0 / 36, -1.0 / 24, -1.0 / 24},
      {1.0 / 36, 1.0 / 12, -1.0 / 12, 1.0 / 54, -1.0 / 36, 1.0 / 54, 1.0 / 36, 1.0 / 24, -1.0 / 24}};
  static constexpr double m(int i, int q) { return M[i][q]; }
  static constexpr double minv(int q, int i) { return MINV[q][i]; }
};

// Lallemand and Luo's D2Q9 basis: rho, jx, jy, pxx, pxy, e, qx, qy, eps
template <>
struct MrtTables<kMrtLallemand> {
  static constexpr int Q = 9, CONSERVED = 3;
  static constexpr double M[9][9] = {
      {1, 1, 1, 1, 1, 1, 1, 1, 1},
      {0, 1, 0, -1, 0, 1, -1, -1, 1},
      {0, 0, 1, 0, -1, 1, 1, -1, -1},
      {0, 1, -1, 1, -1, 0, 0, 0, 0},
      {0, 0, 0, 0, 0, 1, -1, 1, -1},
      {-4, -1, -1, -1, -1, 2, 2, 2, 2},
      {0, -2, 0, 2, 0, 1, -1, -1, 1},
      {0, 0, -2, 0, 2, 1, 1, -1, -1},
      {4, -2, -2, -2, -2, 1, 1, 1, 1}};
  static constexpr double MINV[9][9] = {
      {1.0 / 9, 0, 0, 0, 0, -1.0 / 9, 0, 0, 1.0 / 9},
      {1.0 / 9, 1.0 / 6, 0, 1.0 / 4, 0, -1.0 / 36, -1.0 / 6, 0, -1.0 / 18},
      {1.0 / 9, 0, 1.0 / 6, -1.0 / 4, 0, -1.0 / 36, 0, -1.0 / 6, -1.0 / 18},
      {1.0 / 9, -1.0 / 6, 0, 1.0 / 4, 0, -1.0 / 36, 1.0 / 6, 0, -1.0 / 18},
      {1.0 / 9, 0, -1.0 / 6, -1.0 / 4, 0, -1.0 / 36, 0, 1.0 / 6, -1.0 / 18},
      {1.0 / 9, 1.0 / 6, 1.0 / 6, 0, 1.0 / 4, 1.0 / 18, 1.0 / 12, 1.0 / 12, 1.0 / 36},
      {1.0 / 9, -1.0 / 6, 1.0 / 6, 0, -1.0 / 4, 1.0 / 18, -1.0 / 12, 1.0 / 12, 1.0 / 36},
      {1.0 / 9, -1.0 / 6, -1.0 / 6, 0, 1.0 / 4, 1.0 / 18, -1.0 / 12, -1.0 / 12, 1.0 / 36},
      {1.0 / 9, 1.0 / 6, -1.0 / 6, 0, -1.0 / 4, 1.0 / 18, 1.0 / 12, -1.0 / 12, 1.0 / 36}};
  static constexpr double m(int i, int q) { return M[i][q]; }
  static constexpr double minv(int q, int i) { return MINV[q][i]; }
};

// The Hermite basis of D3Q27: moment i is the product over the axes of the Hermite polynomial of degree A[i][axis] in
// the velocity component, H_0 = 1, H_1 = c, H_2 = c^2 - 1/3.  The basis is orthogonal under the lattice weights, so
// M^-1[q][i] = w_q H_i(e_q) / |H_i|^2, again a product over the axes: w(c) H_a(c) / |H_a|^2 with w(0) = 2/3,
// w(+-1) = 1/6 and |H_a|^2 = 1, 1/3, 2/9.  Every entry is a ratio of small integers, formed exactly and divided once:
// the same double as the literal "p / q" of the reference's table.
template <>
struct MrtTables<kMrtHermite> {
  static constexpr int Q = 27, CONSERVED = 4;
  // rho; jx jy jz; Pi_xx xy xz yy yz zz; J_xxy xxz xyy xyz xzz yyz yzz; J_xxyy xxyz xxzz xyyz xyzz yyzz;
  // J_xxyyz xxyzz xyyzz; J_xxyyzz
  static constexpr int A[27][3] = {
      {0, 0, 0}, {1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {2, 0, 0}, {1, 1, 0}, {1, 0, 1}, {0, 2, 0}, {0, 1, 1},
      {0, 0, 2}, {2, 1, 0}, {2, 0, 1}, {1, 2, 0}, {1, 1, 1}, {1, 0, 2}, {0, 2, 1}, {0, 1, 2}, {2, 2, 0},
      {2, 1, 1}, {2, 0, 2}, {1, 2, 1}, {1, 1, 2}, {0, 2, 2}, {2, 2, 1}, {2, 1, 2}, {1, 2, 2}, {2, 2, 2}};
  static constexpr double m(int i, int q) {
    long long num = 1, den = 1;
    for (int a = 0; a < 3; ++a) {
      const int c = D3Q27::E[q][a];
      if (A[i][a] == 1) num *= c;
      if (A[i][a] == 2) { num *= 3 * c * c - 1; den *= 3; }
    }
    return (double)num / (double)den;
  }
  static constexpr double minv(int q, int i) {
    long long num = 1, den = 1;
    for (int a = 0; a < 3; ++a) {
      const int c = D3Q27::E[q][a];
      if (A[i][a] == 0) { num *= c == 0 ? 2 : 1; den *= c == 0 ? 3 : 6; }
      if (A[i][a] == 1) { num *= c; den *= 2; }
      if (A[i][a] == 2) { num *= c == 0 ? -1 : 1; den *= c == 0 ? 1 : 2; }
    }
    return (double)num / (double)den;
  }
};

// first column of row `row` with a non-zero entry: the sum starts there instead of at zero
template <class Tb, bool INVERSE>
constexpr int mrt_first(int row) {
  for (int c = 0; c < Tb::Q; ++c)
    if ((INVERSE ? Tb::minv(row, c) : Tb::m(row, c)) != 0.0) return c;
  return Tb::Q;
}

// out_row = sum_col table[row][col] in[col], ascending col
template <class Tb, bool INVERSE, int ROW, typename T, class In>
__device__ __forceinline__ T mrt_row(In &&in) {
#pragma clang fp contract(off)
  constexpr int first = mrt_first<Tb, INVERSE>(ROW);
  T acc = T(0);
  static_for<Tb::Q>([&](auto cc) {
#pragma clang fp contract(off)
    constexpr int col = decltype(cc)::value;
    constexpr double c = INVERSE ? Tb::minv(ROW, col) : Tb::m(ROW, col);
    if constexpr (c != 0.0) {
      const T v = in(cc);
      if constexpr (col == first) {
        if constexpr (c == 1.0) acc = v;
        else if constexpr (c == -1.0) acc = -v;
        else acc = T(c) * v;
      } else {
        if constexpr (c == 1.0) acc = acc + v;
        else if constexpr (c == -1.0) acc = acc - v;
        else acc = acc + T(c) * v;
      }
    }
  });
  return acc;
}

// the transform of a lattice's kernels with COLL 10 (Dellar on D2Q9, Hermite on D3Q27) and 11 (Lallemand)
template <class S, int COLL>
constexpr int mrt_transform_of() {
  return COLL == 11 ? kMrtLallemand : (S::Q == 27 ? kMrtHermite : kMrtDellar);
}

template <typename T, class S, int TRANSFORM, int LAYOUT, int VEC, int k>
__device__ __forceinline__ void collide_mrt(T (&f)[S::Q][VEC], const T (&r)[kMrtMaxQ]) {
#pragma clang fp contract(off)
  using Tb = MrtTables<TRANSFORM>;
  static_assert(Tb::Q == S::Q, "the transform belongs to another lattice");
  constexpr int Q = S::Q;
  // (the populations are indexed by the logical q in both layouts, and the moments are those of the logical axes:
  // LAYOUT does not enter)
  T m[Q], meq[Q];
  static_for<Q>([&](auto ic) {
    constexpr int i = decltype(ic)::value;
    m[i] = mrt_row<Tb, false, i, T>([&](auto qc) { return f[decltype(qc)::value][k]; });
    meq[i] = T(0);
  });
  const T rho = m[0], jx = m[1], jy = m[2];
  if constexpr (TRANSFORM == kMrtDellar) {
    // moments.py:195-197: jx * jx / rho * 9 / 2, left to right; N, Jx, Jy relax towards zero
    meq[3] = jx * jx / rho * T(9) / T(2);
    meq[4] = jx * jy / rho * T(9);
    meq[5] = jy * jy / rho * T(9) / T(2);
  } else if constexpr (TRANSFORM == kMrtLallemand) {
    // moments.py:252-264: python scalars multiplied out in double first, then times the field; jx ** 2 without a
    // division by rho, as there
    constexpr double c1 = -2, alpha2 = -8, alpha3 = 4, gamma1 = 2.0 / 3, gamma2 = 18, gamma3 = 2.0 / 3, gamma4 = -18;
    const T jj = jx * jx + jy * jy;
    meq[3] = T(1.0 / 2 * gamma1) * (jx * jx - jy * jy);
    meq[4] = T(1.0 / 2 * gamma3) * (jx * jy);
    meq[5] = T(1.0 / 4 * alpha2) * rho + T(1.0 / 6 * gamma2) * jj;
    meq[6] = T(1.0 / 2 * c1) * jx;
    meq[7] = T(1.0 / 2 * c1) * jy;
    meq[8] = T(1.0 / 4 * alpha3) * rho + T(1.0 / 6 * gamma4) * jj;
  } else {
    // moments.py:556-578: products left to right, one division by the power of rho
    const T jz = m[3];
    const T rho2 = rho * rho, rho3 = rho2 * rho, rho4 = rho2 * rho2, rho5 = rho4 * rho;
    const T xx = jx * jx, xy = jx * jy, xz = jx * jz, yy = jy * jy, yz = jy * jz, zz = jz * jz;
    const T xxy = xx * jy, xxz = xx * jz, xyy = xy * jy, xyz = xy * jz, xzz = xz * jz, yyz = yy * jz, yzz = yz * jz;
    const T xxyy = xxy * jy, xxyz = xxy * jz, xxzz = xxz * jz, xyyz = xyy * jz, xyzz = xyz * jz, yyzz = yyz * jz;
    meq[4] = xx / rho; meq[5] = xy / rho; meq[6] = xz / rho; meq[7] = yy / rho; meq[8] = yz / rho; meq[9] = zz / rho;
    meq[10] = xxy / rho2; meq[11] = xxz / rho2; meq[12] = xyy / rho2; meq[13] = xyz / rho2; meq[14] = xzz / rho2;
    meq[15] = yyz / rho2; meq[16] = yzz / rho2;
    meq[17] = xxyy / rho3; meq[18] = xxyz / rho3; meq[19] = xxzz / rho3; meq[20] = xyyz / rho3; meq[21] = xyzz / rho3;
    meq[22] = yyzz / rho3;
    meq[23] = xxyy * jz / rho4; meq[24] = xxyz * jz / rho4; meq[25] = xyyz * jz / rho4;
    meq[26] = xy * jx * jz * jy * jz / rho5;          // jx * jy * jx * jz * jy * jz / rho ** 5, as written there
  }
  static_for<Q>([&](auto ic) {
#pragma clang fp contract(off)
    constexpr int i = decltype(ic)::value;
    if constexpr (i >= Tb::CONSERVED) m[i] = m[i] - r[i] * (m[i] - meq[i]);
  });
  static_for<Q>([&](auto qc) {
    constexpr int q = decltype(qc)::value;
    f[q][k] = mrt_row<Tb, true, q, T>([&](auto ic) { return m[decltype(ic)::value]; });
  });
}

}  // namespace lt
