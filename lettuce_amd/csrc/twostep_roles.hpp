// Control skeleton of the two-step sweep with separate producer and consumer waves (kernels.hpp, lbm2_kernel,
// SCHED = 1).  Plain C++: tests/test_two_step_roles_skeleton.py compiles it for the host with counting operations.
//
// A workgroup sweeps the output planes s .. last - 1 and needs the intermediate planes s - 1 .. last (relative
// indices 0 .. last - s + 1; output plane k has relative index r = k - s + 1).  Producer waves run phase A only
// (load a plane from global memory, collide, write it to LDS), consumer waves phase B only (read from LDS, collide,
// store).  BOTH roles run this one function and differ in the operations they pass -- a producer's drain / emit and
// a consumer's load / fill do nothing -- so every wave of the workgroup meets the same number of barriers whatever
// the segment length: the barrier count depends on s and last alone.
//   load(plane, set)   issue the global loads of an intermediate plane into register set 0 or 1
//   fill(r, r3, set)   collide that register set and write it to the LDS slots of relative plane r (r3 = r % 3)
//   sync()             wait for this wave's LDS traffic, then the workgroup barrier
//   drain(r, r3)       issue the LDS reads of the output plane with relative index r
//   emit(k)            collide and store output plane k
// Two register sets: the loads of plane k + 3 are issued BEFORE the collide of plane k + 2, into the set that the
// collide of plane k + 1 freed, so a producer has one plane of loads in flight at every moment of the sweep.  The
// set is a compile-time constant (the loop is peeled by two).  LDS slots are those of the one-role schedule: 4 for
// the populations moving up, 3 in-plane, 2 moving down; fill(r + 2) shares no slot with drain(r), and the barrier
// separates it from drain(r - 1).  (Reloading a set right after its collide -- two planes of loads in flight --
// measured 4 % slower, a raised priority for the consumer waves 5 % slower: DESIGN.md section 7.)
#pragma once
#include <type_traits>

#if defined(__HIPCC__)
#define LT_ROLE_FN __host__ __device__ __forceinline__
#else
#define LT_ROLE_FN inline
#endif

namespace lt {

template <int SET>
using RegSet = std::integral_constant<int, SET>;

template <class Load, class Fill, class Sync, class Drain, class Emit>
LT_ROLE_FN void role_sweep(const int s, const int last, Load &&load, Fill &&fill, Sync &&sync, Drain &&drain,
                           Emit &&emit) {
  load(s - 1, RegSet<0>{});
  load(s, RegSet<1>{});
  fill(0, 0, RegSet<0>{});
  load(s + 1, RegSet<0>{});
  fill(1, 1, RegSet<1>{});
  int k = s, r = 1, r3 = 1;
  // one interval = one output plane; WITH_LOAD / WITH_FILL are compile-time so that no path on which loads were
  // issued joins one on which they were not: the compiler's wait in front of the collide would have to serve both,
  // i.e. wait for the loads just issued
  auto interval = [&](auto cur, auto with_load, auto with_fill) {      // cur: the register set that holds plane k + 2
    constexpr int CUR = decltype(cur)::value;
    sync();                                           // planes up to k + 1 complete; reads of k - 1 done
    drain(r, r3);
    if constexpr (decltype(with_load)::value) load(k + 3, RegSet<1 - CUR>{});
    if constexpr (decltype(with_fill)::value) fill(r + 2, r3 == 0 ? 2 : r3 - 1, cur);      // (r + 2) % 3
    emit(k);
    ++k;
    ++r;
    r3 = r3 == 2 ? 0 : r3 + 1;
  };
  using Yes = std::true_type;
  using No = std::false_type;
  if (s + 2 > last) {                                 // a single output plane
    fill(2, 2, RegSet<0>{});
    interval(RegSet<1>{}, No{}, No{});
    return;
  }
  load(s + 2, RegSet<1>{});
  fill(2, 2, RegSet<0>{});
  // steady state while plane k + 3 exists, peeled by two for the register sets; then plane k + 2 = last is filled
  // without a load behind it, and the last output plane needs no new plane at all
  for (;;) {
    if (k + 3 > last) { interval(RegSet<1>{}, No{}, Yes{}); break; }
    interval(RegSet<1>{}, Yes{}, Yes{});
    if (k + 3 > last) { interval(RegSet<0>{}, No{}, Yes{}); break; }
    interval(RegSet<0>{}, Yes{}, Yes{});
  }
  while (k < last) interval(RegSet<0>{}, No{}, No{});
}

// Wave layout of a workgroup: PW producer waves cover the NI intermediate nodes one per thread (the mapping of the
// one-role schedule), then CW consumer waves with CPB output nodes per thread -- two where one would not fit into
// the 16 waves of a workgroup.  Waves go to the four SIMDs in the cyclic order 0, 2, 1, 3 by wave id; the consumers
// are the LAST CW wave ids, consecutive, so that each lands on a SIMD of its own (CW <= 4).  64 x 8 fp32: 11 + 4
// waves; a consumer wave does two collide passes per plane, a producer one: 5 / 5 / 5 / 4 passes on SIMD 0 / 2 / 1 / 3.
template <int NI, int NO>
struct RoleWaves {
  static constexpr int PW = (NI + 63) / 64;
  static constexpr int CPB = PW + NO / 64 > 16 ? 2 : 1;
  static constexpr int CW = NO / CPB / 64;
  static constexpr int THREADS = (PW + CW) * 64;
  static_assert(NO % (CPB * 64) == 0, "whole consumer waves");
  static_assert(PW + CW <= 16, "a workgroup has at most 1024 threads");
};

}  // namespace lt
