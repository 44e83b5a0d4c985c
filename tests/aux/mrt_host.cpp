// collide_mrt of lettuce_amd/csrc/mrt.hpp compiled for the HOST (tests/test_mrt_kernel_host.py): the header needs
// nothing but lattice.hpp, so the arithmetic of the MRT kernels is held against the reference's vectors without a GPU.
// usage: mrt_host <dellar|lallemand|hermite> <f32|f64> <in> <out> <nodes> <rate 0> ... <rate q-1>
//        mrt_host tables <dellar|lallemand|hermite>     prints M, then M^-1, one row per line (%.17g)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#define __device__
#define __forceinline__ inline
#include "mrt.hpp"

template <typename T, class S, int TRANSFORM>
int run(const char *in, const char *out, long n, char **rates) {
  std::vector<T> f((size_t)S::Q * n);
  FILE *fp = fopen(in, "rb");
  if (!fp || fread(f.data(), sizeof(T), f.size(), fp) != f.size()) return 2;
  fclose(fp);
  // r_i as Mrt::fill (unit.inc) forms them: the rate rounded to T, the reciprocal in T
  T r[lt::kMrtMaxQ] = {};
  for (int i = 0; i < S::Q; ++i) r[i] = T(1) / (T)atof(rates[i]);
  for (long i = 0; i < n; ++i) {
    T g[S::Q][1];
    for (int q = 0; q < S::Q; ++q) g[q][0] = f[(size_t)q * n + i];
    lt::collide_mrt<T, S, TRANSFORM, 0, 1, 0>(g, r);
    for (int q = 0; q < S::Q; ++q) f[(size_t)q * n + i] = g[q][0];
  }
  fp = fopen(out, "wb");
  if (!fp || fwrite(f.data(), sizeof(T), f.size(), fp) != f.size()) return 2;
  fclose(fp);
  return 0;
}

template <int TRANSFORM>
int tables() {
  using Tb = lt::MrtTables<TRANSFORM>;
  for (int inverse = 0; inverse < 2; ++inverse)
    for (int i = 0; i < Tb::Q; ++i) {
      for (int j = 0; j < Tb::Q; ++j) printf("%.17g ", inverse ? Tb::minv(i, j) : Tb::m(i, j));
      printf("\n");
    }
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 3 && !strcmp(argv[1], "tables")) {
    if (!strcmp(argv[2], "dellar")) return tables<lt::kMrtDellar>();
    if (!strcmp(argv[2], "lallemand")) return tables<lt::kMrtLallemand>();
    if (!strcmp(argv[2], "hermite")) return tables<lt::kMrtHermite>();
    return 3;
  }
  if (argc < 6) return 3;
  const bool f32 = !strcmp(argv[2], "f32");
  const long n = atol(argv[5]);
#define GO(NAME, S, TRANSFORM)                                                        \
  if (!strcmp(argv[1], NAME)) {                                                       \
    if (argc != 6 + lt::S::Q) return 3;                                               \
    return f32 ? run<float, lt::S, lt::TRANSFORM>(argv[3], argv[4], n, argv + 6)      \
               : run<double, lt::S, lt::TRANSFORM>(argv[3], argv[4], n, argv + 6);    \
  }
  GO("dellar", D2Q9, kMrtDellar) GO("lallemand", D2Q9, kMrtLallemand) GO("hermite", D3Q27, kMrtHermite)
  return 3;
}
