// The one-step kernels with nontemporal loads and stores (the kernels' TUNE = 3), unit by unit
// (tests/test_tune3_census.py holds the output against tests/tune3_census.txt; tests/test_gpu_tune3_vs_cpu.py launches
// every line).  Calls the units' name functions only: nothing here launches or touches a device.
// Asks for cache policy 3 with every combination of the arguments that pick a one-step kernel: both layouts, the modes
// fused, collide-only and stream-only, with and without masks, with and without a constant-pressure outlet, the three
// outlet depths, the outlet slot of the contiguous axis, and every collision number of dispatch.hpp.
// Per unit: each distinct kernel name whose TUNE is 3, sorted, with the first selector (in the order of the loops
// below: the plainest) that reaches it; then how many selectors were asked, how many have a kernel, and how many of
// those get a kernel of policy 0 although they asked for 3 (plans with outlets on two or three axes).
#include <cstdio>
#include <cstring>
#include <map>
#include <string>

#include "dispatch.hpp"

namespace {

// the TUNE argument of a one-step kernel's name: "lbm_kernel<T, lt::S, LAYOUT, COLL, STREAM, COLLIDE, MASKED, 1, 0, TUNE, ..."
int tune_of(const char *name) {
  const char *c = name;
  for (int commas = 0; *c && commas < 9; ++c) commas += *c == ',';
  int tune = -1;
  return sscanf(c, " %d", &tune) == 1 ? tune : -1;
}

void census_of(const char *tag, lt::NameFn name_of) {
  const int colls[] = {lt::kCollNone, lt::kCollBgk, lt::kCollKbc, lt::kCollSmagorinsky, lt::kCollBgk | lt::kCollForce,
                       lt::kCollSmagorinsky | lt::kCollForce, lt::kCollTrt, lt::kCollRegularized, lt::kCollMrt,
                       lt::kCollMrtLallemand, lt::kCollBgk | lt::kCollIncompressible,
                       lt::kCollBgk | lt::kCollForce | lt::kCollIncompressible, lt::kCollTrt | lt::kCollIncompressible,
                       lt::kCollRegularized | lt::kCollIncompressible};
  const int modes[] = {lt::kFused, lt::kCollideOnly, lt::kStreamOnly};
  std::map<std::string, std::string> first;
  long long selectors = 0, with_kernel = 0, other_policy = 0;
  lt::StepArgs a;
  memset(&a, 0, sizeof a);
  a.tune = 3;
  for (a.layout = 0; a.layout < 2; ++a.layout)
    for (int coll : colls)
      for (int mode : modes)
        for (a.masked = 0; a.masked < 2; ++a.masked)
          for (a.n_pout = 0; a.n_pout < 2; ++a.n_pout)
            for (a.abb_depth = 0; a.abb_depth < 3; ++a.abb_depth)
              for (a.abb0_slot = 0; a.abb0_slot < 2; ++a.abb0_slot) {
                a.coll = coll; a.mode = mode;
                char name[192], selector[128];
                ++selectors;
                if (!name_of(a, lt::NameBuf{name, sizeof name})) continue;
                ++with_kernel;
                if (tune_of(name) != 3) { ++other_policy; continue; }
                snprintf(selector, sizeof selector, "layout=%d coll=%d mode=%d masked=%d n_pout=%d abb_depth=%d abb0_slot=%d",
                         a.layout, a.coll, a.mode, a.masked, a.n_pout, a.abb_depth, a.abb0_slot);
                first.emplace(name, selector);
              }
  printf("unit %s\n", tag);
  for (const auto &line : first) printf("  %s | %s\n", line.first.c_str(), line.second.c_str());
  printf("  kernels of policy 3: %zu; selectors with a kernel: %lld of %lld, %lld of them of policy 0\n", first.size(),
         with_kernel, selectors, other_policy);
}

}  // namespace

int main() {
#define LT_CENSUS(tag) census_of(#tag, lt::name_##tag);
  LT_UNITS(LT_CENSUS)
  return 0;
}
