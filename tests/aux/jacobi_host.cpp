// Host harness of lettuce_amd/csrc/jacobi.hpp (tests/test_jacobi_kernel_host.py): jacobi_node over whole fields, sweep
// after sweep, and the squared residuum summed in the order of the two launches (a thread its nodes, a wave its lanes in
// the shuffle tree, a workgroup its waves, then the workgroups: 256 threads again, tree, waves).
//   jacobi_host <f32|f64> <dims> <n0> <n1> <n2> <dx> <sweeps> <in.bin> <out.bin>
// in.bin: rhs then p0; out.bin: p after 1 ... <sweeps> sweeps, then the residuum of the last of them (one sweep more,
// whose p_next is dropped), all in the working type; then one double: the ordered sum of r^2 of that residuum.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "jacobi.hpp"

namespace {

// lane 0 of `sum += shfl_down(sum, off)` for off = 32 ... 1: a lane whose partner lies outside the wave adds its own value
double wave_tree(const double *lane) {
  double v[64];
  memcpy(v, lane, sizeof v);
  for (int off = 32; off > 0; off >>= 1) {
    double next[64];
    for (int l = 0; l < 64; ++l) next[l] = v[l] + (l + off < 64 ? v[l + off] : v[l]);
    memcpy(v, next, sizeof v);
  }
  return v[0];
}

double workgroup_sum(const double *thread) {
  double s = wave_tree(thread);
  for (int w = 1; w < lt::kJacobiWaves; ++w) s += wave_tree(thread + 64 * w);
  return s;
}

template <typename T, int D>
int run(int n0, int n1, int n2, double dx, int sweeps, const char *in, const char *out) {
  const long long N = (long long)n0 * n1 * n2;
  std::vector<T> rhs(N), p(N), next(N), r(N);
  FILE *fi = fopen(in, "rb");
  if (!fi || fread(rhs.data(), sizeof(T), N, fi) != (size_t)N || fread(p.data(), sizeof(T), N, fi) != (size_t)N) return 2;
  fclose(fi);
  FILE *fo = fopen(out, "wb");
  if (!fo) return 2;
  const T dx2 = (T)(dx * dx);
  for (int s = 1; s <= sweeps + 1; ++s) {
    for (long long i = 0; i < N; ++i) lt::jacobi_node<T, D>(p.data(), rhs.data(), i, n0, n1, n2, dx2, next[i], r[i]);
    if (s <= sweeps) {
      p.swap(next);
      fwrite(p.data(), sizeof(T), N, fo);
    }
  }
  fwrite(r.data(), sizeof(T), N, fo);
  // the first launch's partials ...
  const long long chunk = lt::jacobi_chunk(N);
  const int blocks = lt::jacobi_blocks(N);
  std::vector<double> partial(blocks);
  for (int b = 0; b < blocks; ++b) {
    double thread[lt::kJacobiThreads];
    const long long begin = b * chunk, end = begin + chunk < N ? begin + chunk : N;
    for (int t = 0; t < lt::kJacobiThreads; ++t) {
      double sum = 0.0;
      for (long long i = begin + t; i < end; i += lt::kJacobiThreads) {
        const double rd = (double)r[i];
        sum += rd * rd;
      }
      thread[t] = sum;
    }
    partial[b] = workgroup_sum(thread);
  }
  // ... and the second launch's sum of them
  double thread[lt::kJacobiThreads];
  for (int t = 0; t < lt::kJacobiThreads; ++t) {
    double sum = 0.0;
    for (int b = t; b < blocks; b += lt::kJacobiThreads) sum += partial[b];
    thread[t] = sum;
  }
  const double total = workgroup_sum(thread);
  fwrite(&total, sizeof total, 1, fo);
  fclose(fo);
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 10) return 1;
  const bool f32 = !strcmp(argv[1], "f32");
  const int d = atoi(argv[2]), n0 = atoi(argv[3]), n1 = atoi(argv[4]), n2 = atoi(argv[5]), sweeps = atoi(argv[7]);
  const double dx = atof(argv[6]);
  if (d == 2) return f32 ? run<float, 2>(n0, n1, 1, dx, sweeps, argv[8], argv[9]) : run<double, 2>(n0, n1, 1, dx, sweeps, argv[8], argv[9]);
  if (d == 3) return f32 ? run<float, 3>(n0, n1, n2, dx, sweeps, argv[8], argv[9]) : run<double, 3>(n0, n1, n2, dx, sweeps, argv[8], argv[9]);
  return 1;
}
