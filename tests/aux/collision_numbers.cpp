// The kernels' collision numbers (lettuce_amd/csrc/dispatch.hpp, kColl*) and what coll_forced, coll_mrt and coll_base
// say of each, held against the values written out: 5 and 7 carry a body force (on BGK and on Smagorinsky), 10 and 11
// are MRT, and 8 and 9 -- TRT and the regularised collision -- are neither: the operators after Smagorinsky were numbered
// from 8 so that none of them has the force's bit (4) set.  Nothing here launches or touches a device.
#include <cstdio>

#include "dispatch.hpp"
#include "lettuce_hip.h"

namespace {

struct Row {
  int coll, named;
  bool forced, mrt;
  int base;
};

}  // namespace

int main() {
  const Row rows[] = {{0, lt::kCollNone, false, false, 0},
                      {1, lt::kCollBgk, false, false, 1},
                      {2, lt::kCollKbc, false, false, 2},
                      {3, lt::kCollSmagorinsky, false, false, 3},
                      {5, lt::kCollBgk | lt::kCollForce, true, false, 1},
                      {7, lt::kCollSmagorinsky | lt::kCollForce, true, false, 3},
                      {8, lt::kCollTrt, false, false, 8},
                      {9, lt::kCollRegularized, false, false, 9},
                      {10, lt::kCollMrt, false, true, 10},
                      {11, lt::kCollMrtLallemand, false, true, 11}};
  int bad = 0;
  for (const Row &r : rows) {
    const bool ok = r.named == r.coll && lt::coll_forced(r.coll) == r.forced && lt::coll_mrt(r.coll) == r.mrt &&
                    lt::coll_base(r.coll) == r.base;
    printf("%d: named %d forced %d mrt %d base %d%s\n", r.coll, r.named, (int)lt::coll_forced(r.coll),
           (int)lt::coll_mrt(r.coll), lt::coll_base(r.coll), ok ? "" : "  <- wrong");
    bad += ok ? 0 : 1;
  }
  if (lt::kCollForce != 4) { printf("kCollForce is %d\n", lt::kCollForce); ++bad; }
  // the ABI's numbers where the ABI has the operator
  const int abi[][2] = {{lt::kCollNone, LT_COLLISION_NONE}, {lt::kCollBgk, LT_COLLISION_BGK}, {lt::kCollKbc, LT_COLLISION_KBC},
                        {lt::kCollSmagorinsky, LT_COLLISION_SMAGORINSKY}, {lt::kCollTrt, LT_COLLISION_TRT},
                        {lt::kCollRegularized, LT_COLLISION_REGULARIZED}, {lt::kCollMrt, LT_COLLISION_MRT}};
  for (const auto &pair : abi)
    if (pair[0] != pair[1]) { printf("kernel number %d, ABI %d\n", pair[0], pair[1]); ++bad; }
  return bad ? 1 : 0;
}
