// The launches of the Jacobi solver (jacobi.hpp): fp32 and fp64, 2-D and 3-D.  No lattice, no plan.
#include "dispatch.hpp"
#include "jacobi.hpp"
#include "lettuce_hip.h"

namespace lt {

static_assert(sizeof(JacobiState) == 24, "lt_jacobi reads the record as {int32 done, int32, int64 iterations, double error}");
static_assert(LT_JACOBI_BLOCKS == kJacobiBlocks && LT_JACOBI_WORK_BYTES >= kJacobiBlocks * 8 + sizeof(JacobiState),
              "the work buffer of lt_jacobi: the partials, then the record");

void *jacobi_state(void *work) { return static_cast<double *>(work) + kJacobiBlocks; }

namespace {
template <typename T, int D>
int launch(const JacobiArgs &a) {
  const long long N = (long long)a.n0 * a.n1 * a.n2;
  const int blocks = jacobi_blocks(N);
  double *partial = static_cast<double *>(a.work);
  JacobiState *state = static_cast<JacobiState *>(jacobi_state(a.work));
  hipLaunchKernelGGL((jacobi_sweep_kernel<T, D>), dim3(blocks), dim3(kJacobiThreads), 0, a.stream,
                     static_cast<const T *>(a.p_in), static_cast<const T *>(a.rhs), static_cast<T *>(a.p_out), a.n0, a.n1,
                     a.n2, jacobi_chunk(N), (T)a.dx2, state, partial);
  if (a.finish)
    hipLaunchKernelGGL(jacobi_finish_kernel, dim3(1), dim3(kJacobiThreads), 0, a.stream, partial, blocks, N, a.sweep,
                       a.tol, state);
  return (int)hipGetLastError();
}
}  // namespace

int jacobi_sweep(const JacobiArgs &a) {
  if (a.dtype == 0) return a.d == 2 ? launch<float, 2>(a) : launch<float, 3>(a);
  return a.d == 2 ? launch<double, 2>(a) : launch<double, 3>(a);
}

}  // namespace lt
