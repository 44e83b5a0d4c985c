// pressure_outlet_apply of lettuce_amd/csrc/kernels.hpp compiled for the HOST: tests/test_outlet_p_kernel_host.py cuts
// the constants, the text between the markers "// ---- moments" and "// ---- boundaries" and the function itself (from
// "// EquilibriumOutletP" to "// What the boundaries with an index below") out of kernels.hpp into outlet_p_excerpt.inc,
// so that the arithmetic the kernels inline is held against the reference's outlet planes without a GPU.
// usage: outlet_p_host <lattice> <f32|f64> <in> <out> <nodes> <rho_outlet>
//   in: the populations [Q][nodes] of the nodes next to the outlet plane as the outlet sees them; out: the plane's
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
struct KParamsF {            // what collide_forced reads (not exercised here)
  T accel[3], shift[3], source_scale, tau_inv, tau, smag_c2;
};
#include "outlet_p_excerpt.inc"
}  // namespace lt

template <typename T, class S>
int run(const char *in, const char *out, long n, double rho_outlet) {
  std::vector<T> f((size_t)S::Q * n);
  FILE *fp = fopen(in, "rb");
  if (!fp || fread(f.data(), sizeof(T), f.size(), fp) != f.size()) return 2;
  fclose(fp);
  for (long i = 0; i < n; ++i) {
    T g[S::Q][1], rn, jn[3];
    for (int q = 0; q < S::Q; ++q) g[q][0] = f[(size_t)q * n + i];
    lt::moments<T, S, 0, 1, 0>(g, rn, jn);                            // as neighbour_moments hands them over
    lt::pressure_outlet_apply<T, S, 0, 1, 0>((T)rho_outlet, rn, jn, g);   // rho_outlet rounded as upload_boundaries does
    for (int q = 0; q < S::Q; ++q) f[(size_t)q * n + i] = g[q][0];
  }
  fp = fopen(out, "wb");
  if (!fp || fwrite(f.data(), sizeof(T), f.size(), fp) != f.size()) return 2;
  fclose(fp);
  return 0;
}

int main(int argc, char **argv) {
  if (argc != 7) return 3;
  const char *lat = argv[1];
  const bool f32 = !strcmp(argv[2], "f32");
  const long n = atol(argv[5]);
  const double rho = atof(argv[6]);
#define GO(NAME, S)       \
  if (!strcmp(lat, NAME)) \
    return f32 ? run<float, lt::S>(argv[3], argv[4], n, rho) : run<double, lt::S>(argv[3], argv[4], n, rho);
  GO("d1q3", D1Q3) GO("d2q9", D2Q9) GO("d3q15", D3Q15) GO("d3q19", D3Q19) GO("d3q27", D3Q27)
  return 3;
}
