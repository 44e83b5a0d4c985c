// The dispatch table of every unit, selector by selector (tests/test_dispatch_table.py holds the output against
// tests/dispatch_table.txt).  Calls the units' name functions only: nothing here launches or touches a device.
// Per unit: the distinct kernel names, sorted; how many selectors have a kernel; FNV-1a (64 bit) over the names
// ("-": no kernel) of all selectors in the order of the loops below, each followed by a newline.
//
// A selector is every field the name-only path of unit.inc reads before a launcher's `if (name)`.  The loops, outermost
// first: layout 0, 1; every collision number of dispatch.hpp in ascending order; mode 0 .. 4; masked 0, 1; tune 0, 1, 3;
// abb_depth 0, 1, 2; n_pout 0, 1; the message buffers pack_lo (bit 0) and pack_hi (bit 1), 0 .. 3.  Below these
//   mode != kFusedTwice:  n_abb 0, 1 (a force-field plan has no kernel beside an outlet); abb_axis, strip, shift and
//                         signal, which only the two-step path reads, stay 0 / null
//   mode == kFusedTwice:  abb_axis 0, 1, 2; strip 0, 64, 128, 256, 512; shift 0, 3, 6; signal null, set; n_abb stays 0
// -- 4 608 combinations of the outer loops, times 2 in four modes and times 90 in one: 451 584 selectors per unit.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <set>
#include <string>

#include "dispatch.hpp"

namespace {

struct Table {
  std::set<std::string> names;
  long long selectors = 0, with_kernel = 0;
  uint64_t hash = 0xcbf29ce484222325ull;
  void add(const char *name) {
    ++selectors;
    if (name) { ++with_kernel; names.insert(name); }
    for (const char *c = name ? name : "-"; *c; ++c) hash = (hash ^ (unsigned char)*c) * 0x100000001b3ull;
    hash = (hash ^ (unsigned char)'\n') * 0x100000001b3ull;
  }
};

// the message buffers are never dereferenced
void table_of(const char *tag, lt::NameFn name_of) {
  static char lo[1], hi[1];
  static unsigned long long signal[1];
  const int colls[] = {0, 1, 2, 3, 5, 7, 8, 9, 10, 11, 17, 21, 24, 25, 37, 39};
  const int tunes[] = {0, 1, 3}, strips[] = {0, 64, 128, 256, 512}, shifts[] = {0, 3, 6};
  Table t;
  lt::StepArgs a;
  memset(&a, 0, sizeof a);
  const auto add = [&] {
    char name[192];
    t.add(name_of(a, lt::NameBuf{name, sizeof name}));
  };
  for (a.layout = 0; a.layout < 2; ++a.layout)
    for (int coll : colls)
      for (a.mode = 0; a.mode < 5; ++a.mode)
        for (a.masked = 0; a.masked < 2; ++a.masked)
          for (int tune : tunes)
            for (a.abb_depth = 0; a.abb_depth < 3; ++a.abb_depth)
              for (a.n_pout = 0; a.n_pout < 2; ++a.n_pout)
                for (int buffers = 0; buffers < 4; ++buffers) {
                  a.coll = coll; a.tune = tune;
                  a.pack_lo = (buffers & 1) ? lo : nullptr;
                  a.pack_hi = (buffers & 2) ? hi : nullptr;
                  a.n_abb = a.abb_axis = a.strip = a.shift = 0;
                  a.signal = nullptr;
                  if (a.mode != lt::kFusedTwice) {
                    for (a.n_abb = 0; a.n_abb < 2; ++a.n_abb) add();
                    continue;
                  }
                  for (a.abb_axis = 0; a.abb_axis < 3; ++a.abb_axis)
                    for (int strip : strips)
                      for (int shift : shifts)
                        for (int signalled = 0; signalled < 2; ++signalled) {
                          a.strip = strip; a.shift = shift;
                          a.signal = signalled ? signal : nullptr;
                          add();
                        }
                }
  printf("unit %s\n", tag);
  for (const std::string &n : t.names) printf("  %s\n", n.c_str());
  printf("  selectors with a kernel: %lld of %lld\n  hash %016llx\n", t.with_kernel, t.selectors, (unsigned long long)t.hash);
}

}  // namespace

int main() {
#define LT_TABLE(tag) table_of(#tag, lt::name_##tag);
  LT_UNITS(LT_TABLE)
  return 0;
}
