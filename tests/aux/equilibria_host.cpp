// The collide functions of lettuce_amd/csrc/kernels.hpp with the incompressible equilibrium, compiled for the HOST:
// tests/test_equilibria_kernel_host.py cuts the text between the markers "// ---- moments" and "// ---- boundaries" (and
// the constants) out of kernels.hpp into collide_excerpt.inc, as tests/aux/collide_host.cpp has it, so that the
// arithmetic of the new kernels is held against the reference's vectors without a GPU.
// usage: equilibria_host <bgk|trt|regularized|guo> <lattice> <f32|f64> <in> <out> <nodes> <tau> <tau_minus>
//                        <acceleration along x> <equilibrium: 0 quadratic, 1 incompressible> <rho0>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>
#define __device__
#define __forceinline__ inline
#include "lattice.hpp"
namespace lt {
template <typename T>
struct KParamsF {            // what collide_forced reads
  T accel[3], shift[3], source_scale, tau_inv, tau, smag_c2;
};
#include "collide_excerpt.inc"
}  // namespace lt

template <typename T, class S, int EQ>
void collide(const char *op, T (&g)[S::Q][1], double tau, double tau_minus, double ax, double rho0_) {
  // the scalars as params_of and the families' fill (unit.inc) form them
  const T rho0 = (T)rho0_;
  if (!strcmp(op, "trt")) {
    lt::collide_trt<T, S, 0, 1, 0, EQ>(g, (T)(1. / (2 * tau)), (T)(1.0 / (2.0 * tau_minus)), rho0);
  } else if (!strcmp(op, "regularized")) {
    lt::collide_regularized<T, S, 0, 1, 0, EQ>(g, (T)(1.0 - 1.0 / tau), rho0);
  } else if (!strcmp(op, "guo")) {
    using M = lt::MemMap<S, 0>;
    lt::KParamsF<T> p{};
    p.accel[M::memory(0)] = (T)ax;
    p.shift[M::memory(0)] = (T)0.5 * (T)ax;
    p.source_scale = (T)(1.0 - 1.0 / (2.0 * tau));
    p.tau_inv = (T)(1.0 / tau);
    lt::collide_forced<T, S, 0, 1, 0, 1, EQ>(g, p, rho0);
  } else {
    lt::collide_bgk<T, S, 0, 1, 0, EQ>(g, (T)(1.0 / tau), rho0);
  }
}

template <typename T, class S>
int run(const char *op, const char *in, const char *out, long n, double tau, double tau_minus, double ax, int eq,
        double rho0) {
  std::vector<T> f((size_t)S::Q * n);
  FILE *fp = fopen(in, "rb");
  if (!fp || fread(f.data(), sizeof(T), f.size(), fp) != f.size()) return 2;
  fclose(fp);
  for (long i = 0; i < n; ++i) {
    T g[S::Q][1];
    for (int q = 0; q < S::Q; ++q) g[q][0] = f[(size_t)q * n + i];
    if (eq == 1) collide<T, S, 1>(op, g, tau, tau_minus, ax, rho0);
    else collide<T, S, 0>(op, g, tau, tau_minus, ax, rho0);
    for (int q = 0; q < S::Q; ++q) f[(size_t)q * n + i] = g[q][0];
  }
  fp = fopen(out, "wb");
  if (!fp || fwrite(f.data(), sizeof(T), f.size(), fp) != f.size()) return 2;
  fclose(fp);
  return 0;
}

int main(int argc, char **argv) {
  if (argc != 12) return 3;
  const char *op = argv[1], *lat = argv[2];
  const bool f32 = !strcmp(argv[3], "f32");
  const long n = atol(argv[6]);
  const double tau = atof(argv[7]), tm = atof(argv[8]), ax = atof(argv[9]), rho0 = atof(argv[11]);
  const int eq = atoi(argv[10]);
#define GO(NAME, S)                                                                          \
  if (!strcmp(lat, NAME))                                                                    \
    return f32 ? run<float, lt::S>(op, argv[4], argv[5], n, tau, tm, ax, eq, rho0)           \
               : run<double, lt::S>(op, argv[4], argv[5], n, tau, tm, ax, eq, rho0);
  GO("d1q3", D1Q3) GO("d2q9", D2Q9) GO("d3q15", D3Q15) GO("d3q19", D3Q19) GO("d3q27", D3Q27)
  return 3;
}
