// What a launch of several steps needs from a lattice, a scalar type and a grid (lettuce_amd/csrc/launch_limits.hpp),
// held against numbers written out here: every unit's two-step tile without and with masks, the LDS footprints the tiles
// follow from, the strips of the 2-D sweep, the many-step limits and the 32-bit addressing predicates at their edges.
// The header is what both the admission of a plan (api.hip) and the launchers (unit.inc) read, so these are the numbers
// of both.  Nothing here launches or touches a device.
#include <cstdio>

#include "launch_limits.hpp"

namespace {

int bad = 0;

void check(const char *what, long long got, long long want) {
  const bool ok = got == want;
  printf("%s: %lld%s", what, got, ok ? "\n" : "");
  if (!ok) printf(", expected %lld  <- wrong\n", want);
  bad += ok ? 0 : 1;
}

template <class S, typename T>
void tile(const char *unit, int width, int rows, int rows_masked) {
  constexpr lt::UnitTile t = lt::two_step_tile<S, T>();
  char what[64];
  snprintf(what, sizeof what, "%s tile width", unit); check(what, t.width, width);
  snprintf(what, sizeof what, "%s rows", unit); check(what, t.rows, rows);
  snprintf(what, sizeof what, "%s rows with masks", unit); check(what, t.rows_masked, rows_masked);
  if (S::D != 3) return;
  // what a launch on a 256^3 grid takes
  check("  on 256^3: width", lt::two_step_tile_on(t, S::D, 256, false).width, width);
  check("  on 256^3: rows", lt::two_step_tile_on(t, S::D, 256, false).rows, rows);
  check("  on 256^3 with masks: rows", lt::two_step_tile_on(t, S::D, 256, true).rows, rows_masked);
  check("  256^3 tiles", lt::tiles(lt::two_step_tile_on(t, S::D, 256, false), 256, 256), rows > 0);
}

}  // namespace

int main() {
  using namespace lt;
  check("LDS budget", (long long)kLdsBudget, 163840);
  tile<D3Q15, float>("d3q15_f32", 64, 8, 8);
  tile<D3Q15, double>("d3q15_f64", 32, 8, 8);
  tile<D3Q19, float>("d3q19_f32", 64, 8, 8);
  tile<D3Q19, double>("d3q19_f64", 32, 8, 0);
  tile<D3Q27, float>("d3q27_f32", 64, 4, 4);
  tile<D3Q27, double>("d3q27_f64", 32, 0, 0);
  tile<D2Q9, float>("d2q9_f32", 0, 0, 0);      // (a 2-D launch takes a strip, below)
  tile<D1Q3, double>("d1q3_f64", 0, 0, 0);

  // LDS bytes.  Without masks 4 + 3 + 2 slots of the upward, in-plane and downward populations -- 5 + 9 + 5 of D3Q19's,
  // 57 planes of 66 x 10 nodes: the 150 480 B the ISA of lbm2_kernel reports
  check("lbm2_kernel d3q19 f32 64 x 8", (long long)two_step_lds<float, D3Q19, 64, 8>(), 4ll * 57 * 660);
  check("  = ", (long long)two_step_lds<float, D3Q19, 64, 8>(), 150480);
  check("lbm2_kernel d3q19 f64 32 x 8", (long long)two_step_lds<double, D3Q19, 32, 8>(), 155040);
  check("lbm2_kernel d3q27 f32 64 x 8", (long long)two_step_lds<float, D3Q27, 64, 8>(), 213840);
  check("lbm2_kernel d3q27 f32 64 x 4", (long long)two_step_lds<float, D3Q27, 64, 4>(), 128304);
  check("lbm2_kernel d3q27 f64 32 x 8", (long long)two_step_lds<double, D3Q27, 32, 8>(), 220320);
  // with masks 4 + 3 + 3 slots and two cached equilibria: 660 x 62 + 38 values for D3Q19 fp32
  check("lbm2m_kernel d3q19 f32 64 x 8", (long long)two_step_masked_lds<float, D3Q19, 0, 64, 8>(), 163832);
  check("lbm2m_kernel d3q19 f32 64 x 8, slab layout", (long long)two_step_masked_lds<float, D3Q19, 1, 64, 8>(), 163832);
  check("lbm2m_kernel d3q19 f64 32 x 8", (long long)two_step_masked_lds<double, D3Q19, 0, 32, 8>(), 168944);
  check("lbm2m_kernel d3q27 f32 64 x 4", (long long)two_step_masked_lds<float, D3Q27, 0, 64, 4>(), 142776);
  check("lbm2m_kernel d3q15 f32 64 x 8", (long long)two_step_masked_lds<float, D3Q15, 0, 64, 8>(), 132120);
  check("lbm2m_kernel d3q15 f64 32 x 8", (long long)two_step_masked_lds<double, D3Q15, 1, 32, 8>(), 136240);
  check("d3q15 crosses a plane with", TwoStep<float, D3Q15, 64, 8>::count<0, 1>(), 5);
  check("d3q19 crosses a plane with", TwoStep<float, D3Q19, 64, 8>::count<1, -1>(), 5);
  check("d3q27 crosses a plane with", TwoStep<float, D3Q27, 64, 4>::count<0, 1>(), 9);

  // 2-D strips: the widest of 512 / 256 / 128 / 64 columns that divides the contiguous extent
  check("strips", (long long)(sizeof kStripWidths / sizeof kStripWidths[0]), 4);
  check("strip of 4096", strip_width(4096), 512);
  check("strip of 768", strip_width(768), 256);
  check("strip of 128", strip_width(128), 128);
  check("strip of 192", strip_width(192), 64);
  check("strip of 64", strip_width(64), 64);
  check("strip of 96", strip_width(96), 0);
  constexpr UnitTile none = two_step_tile<D2Q9, double>();
  check("d2q9 on 4096: width", two_step_tile_on(none, 2, 4096, true).width, 512);
  check("d2q9 on 4096: rows", two_step_tile_on(none, 2, 4096, true).rows, 1);
  check("d2q9 on 192: width", two_step_tile_on(none, 2, 192, false).width, 64);
  check("d2q9 on 192: rows", two_step_tile_on(none, 2, 192, false).rows, 1);
  check("d2q9 on 96: width", two_step_tile_on(none, 2, 96, false).width, 0);
  check("d2q9 on 96: rows", two_step_tile_on(none, 2, 96, false).rows, 0);
  check("d2q9 96 x 5 tiles", tiles(two_step_tile_on(none, 2, 96, false), 96, 5), 0);
  check("d2q9 192 x 5 tiles", tiles(two_step_tile_on(none, 2, 192, false), 192, 5), 1);
  check("d1q3 on 256: rows", two_step_tile_on(two_step_tile<D1Q3, float>(), 1, 256, false).rows, 0);
  // a grid tiles where both extents are multiples: one row more, half a tile more
  constexpr TwoStepTile t19 = two_step_tile_on(two_step_tile<D3Q19, float>(), 3, 64, false);
  check("d3q19 f32 64 x 8 tiles", tiles(t19, 64, 8), 1);
  check("d3q19 f32 64 x 9 tiles", tiles(t19, 64, 9), 0);
  check("d3q19 f32 96 x 8 tiles", tiles(t19, 96, 8), 0);

  // many-step launches
  check("many-step tile", kManyTile, 8);
  check("many-step steps", many_steps_max(false), 8);
  check("many-step steps with an outlet", many_steps_max(true), 7);
  check("kManyMax", kManyMax, 8);

  // addressing.  2^32 = 4 294 967 296
  const long long n384 = 384ll * 384 * 384, n344 = 344ll * 344 * 344, n341 = 341ll * 341 * 341;
  check("per-population kernel: reference layout, BGK, D3Q19", masked_per_population(0, kCollBgk, 19), 1);
  check("per-population kernel: D3Q15", masked_per_population(0, kCollBgk, 15), 1);
  check("per-population kernel: D3Q27", masked_per_population(0, kCollBgk, 27), 0);
  check("per-population kernel: slab layout", masked_per_population(1, kCollBgk, 19), 0);
  check("per-population kernel: streaming only", masked_per_population(0, kCollNone, 19), 0);
  // D3Q19 fp32 384^3: 19 x 384^3 x 4 B = 4 303 355 904 B, a population 226 492 416 B
  check("d3q19 f32 384^3 as a field", field_addressable(19, n384, 4, false), 0);
  check("d3q19 f32 384^3 per population", field_addressable(19, n384, 4, masked_per_population(0, kCollBgk, 19)), 1);
  // a population of 1024 x 1024 x 1020 fp32 nodes: 4 278 190 080 B; of 1024^3: 2^32 B
  check("1024 x 1024 x 1020 f32 per population", field_addressable(19, 1024ll * 1024 * 1020, 4, true), 1);
  check("1024^3 f32 per population", field_addressable(19, 1024ll * 1024 * 1024, 4, true), 0);
  // D3Q27 fp32 344^3: 27 x 40 707 584 x 4 B = 4 396 419 072 B, and no kernel per population
  check("d3q27 f32 344^3", field_addressable(27, n344, 4, masked_per_population(0, kCollBgk, 27)), 0);
  // the distance between populations counts, not the nodes.  D3Q27 fp32 341^3: 27 x 39 651 821 x 4 B = 4 282 396 668 B,
  // and 32 832 elements further apart 4 285 942 524 B: both below; 320 x 352 x 353 = 39 761 920 nodes: 4 294 287 360 B
  // dense, 4 297 833 216 B with populations 39 794 752 elements apart
  check("d3q27 f32 341^3", field_addressable(27, n341, 4, false), 1);
  check("d3q27 f32 341^3, 32 832 elements further apart", field_addressable(27, n341 + 32832, 4, false), 1);
  check("d3q27 f32 320 x 352 x 353", field_addressable(27, 39761920, 4, false), 1);
  check("d3q27 f32 320 x 352 x 353, 32 832 elements further apart", field_addressable(27, 39794752, 4, false), 0);
  // without masks: a plane.  32768 x 32768 fp32 nodes are 2^32 B
  check("plane 32768 x 32768 f32", plane_addressable(32768, 32768, 4), 0);
  check("plane 32768 x 32764 f32", plane_addressable(32768, 32764, 4), 1);
  check("plane 32768 x 16384 f64", plane_addressable(32768, 16384, 8), 0);

  // the small minima
  check("planes per workgroup", min_segment(false), 1);
  check("planes per workgroup with masks", min_segment(true), 2);
  check("planes where the outlet lies on the sweep axis", kOutletSweepMin, 3);
  check("boundaries of a masked two-step plan", kMaskedTwoStepBoundaries, 15);
  printf("%d mismatches\n", bad);
  return bad ? 1 : 0;
}
