// The dispatch table of every unit, selector by selector (tests/test_dispatch_table.py holds the output against
// tests/dispatch_table.txt).  Calls the units' name functions only: nothing here launches or touches a device.
// Per unit: the distinct kernel names, sorted; how many selectors have a kernel; FNV-1a (64 bit) over the names
// ("-": no kernel) of all selectors in the order of the loops below, each followed by a newline.
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

// every field the name-only path of unit.inc reads; the message buffers are never dereferenced
void table_of(const char *tag, lt::NameFn name_of) {
  static char lo[1], hi[1];
  static unsigned long long signal[1];
  const int colls[] = {0, 1, 2, 3, 5, 7}, tunes[] = {0, 1, 3}, strips[] = {0, 64, 128, 256, 512}, shifts[] = {0, 3, 6};
  Table t;
  lt::StepArgs a;
  memset(&a, 0, sizeof a);
  for (a.layout = 0; a.layout < 2; ++a.layout)
    for (int coll : colls)
      for (a.mode = 0; a.mode < 5; ++a.mode)
        for (a.masked = 0; a.masked < 2; ++a.masked)
          for (int tune : tunes)
            for (a.abb_depth = 0; a.abb_depth < 3; ++a.abb_depth)
              for (a.abb_axis = 0; a.abb_axis < 3; ++a.abb_axis)
                for (int strip : strips)
                  for (int shift : shifts)
                    for (int buffers = 0; buffers < 8; ++buffers) {
                      a.coll = coll; a.tune = tune; a.strip = strip; a.shift = shift;
                      a.pack_lo = (buffers & 1) ? lo : nullptr;
                      a.signal = (buffers & 2) ? signal : nullptr;
                      a.pack_hi = (buffers & 4) ? hi : nullptr;
                      char name[192];
                      t.add(name_of(a, lt::NameBuf{name, sizeof name}));
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
