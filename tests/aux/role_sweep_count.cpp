/* Host instantiation of the control skeleton of the role-separated two-step sweep (csrc/twostep_roles.hpp) with
 * counting operations.  For every segment n = last - s in [1, 130] and two values of s it runs the producer's and
 * the consumer's set of operations and checks
 *   - both meet the same number of barriers, n of them;
 *   - the producer fills the relative planes 0 .. n + 1 once each and in order, from the register set its load went
 *     to, each load issued before the fill of the plane in front of it (one plane of loads in flight), and no set is
 *     loaded again before it was filled;
 *   - the consumer drains and emits the output planes s .. last - 1 once each and in order;
 *   - LDS slots (4 up, 3 in-plane, 2 down): when plane r is drained, the slots it reads hold the planes r - 1, r,
 *     r + 1, written before the preceding barrier; a fill never writes a slot that the drain of the same interval
 *     (not separated from it by a barrier) reads.
 * Prints "ok <cases>" and exits 0, or the first violation and exits 1.
 * Build: g++ -std=c++17 -O1 -I lettuce_amd/csrc role_sweep_count.cpp */
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "twostep_roles.hpp"

struct Event {
  char what;   // 'L'oad, 'F'ill, 'S'ync, 'D'rain, 'E'mit
  int a, b, set;
};

static int fail(const char *msg, int s, int n, int at) {
  printf("s = %d, n = %d, event %d: %s\n", s, n, at, msg);
  return 1;
}

static std::vector<Event> run(int s, int last, bool producer) {
  std::vector<Event> ev;
  auto load = [&](int plane, auto set) { ev.push_back({'L', plane, 0, decltype(set)::value}); };
  auto fill = [&](int r, int r3, auto set) { ev.push_back({'F', r, r3, decltype(set)::value}); };
  auto sync = [&]() { ev.push_back({'S', 0, 0, 0}); };
  auto drain = [&](int r, int r3) { ev.push_back({'D', r, r3, 0}); };
  auto emit = [&](int k) { ev.push_back({'E', k, 0, 0}); };
  if (producer)
    lt::role_sweep(s, last, load, fill, sync, [](int, int) {}, [](int) {});
  else
    lt::role_sweep(s, last, [](int, auto) {}, [](int, int, auto) {}, sync, drain, emit);
  return ev;
}

int main() {
  int cases = 0;
  for (int s : {0, 7})
    for (int n = 1; n <= 130; ++n, ++cases) {
      const int last = s + n;
      const std::vector<Event> pe = run(s, last, true), ce = run(s, last, false);
      // --- barriers
      int pb = 0, cb = 0;
      for (const Event &e : pe) pb += e.what == 'S';
      for (const Event &e : ce) cb += e.what == 'S';
      if (pb != cb || pb != n) return fail("barrier counts differ between the roles or from n", s, n, pb * 1000 + cb);
      // --- producer: loads and fills
      int holds[2] = {-1, -1};          // relative plane a register set holds, -1 = free
      int filled = 0, loaded = 0;
      for (size_t i = 0; i < pe.size(); ++i) {
        const Event &e = pe[i];
        if (e.what == 'L') {
          if (e.a != s - 1 + loaded) return fail("loads out of order", s, n, (int)i);
          if (e.a > last) return fail("load beyond the last intermediate plane", s, n, (int)i);
          if (holds[e.set] != -1) return fail("load into a register set that was not filled yet", s, n, (int)i);
          holds[e.set] = loaded++;
        } else if (e.what == 'F') {
          if (e.a != filled || e.b != filled % 3) return fail("fills out of order or wrong r3", s, n, (int)i);
          if (holds[e.set] != filled) return fail("fill from a register set that does not hold the plane", s, n, (int)i);
          // a plane of loads in flight behind every collide but the last one
          if (filled + 1 <= n + 1 && holds[1 - e.set] != filled + 1) return fail("no load in flight behind the fill", s, n, (int)i);
          holds[e.set] = -1;
          ++filled;
        }
      }
      if (filled != n + 2 || loaded != n + 2) return fail("not every intermediate plane was loaded and filled", s, n, filled);
      // --- consumer: drains and emits
      int drained = 0, emitted = 0;
      for (size_t i = 0; i < ce.size(); ++i) {
        const Event &e = ce[i];
        if (e.what == 'D') {
          if (e.a != drained + 1 || e.b != (drained + 1) % 3) return fail("drains out of order or wrong r3", s, n, (int)i);
          ++drained;
        } else if (e.what == 'E') {
          if (e.a != s + emitted || emitted != drained - 1) return fail("emits out of order", s, n, (int)i);
          ++emitted;
        }
      }
      if (drained != n || emitted != n) return fail("not every output plane was drained and emitted", s, n, drained);
      // --- LDS slots, interval by interval (interval j = what lies between barrier j and barrier j + 1; interval 0 is
      // the prologue).  u[4], c[3], d[2] hold the relative plane written last.
      std::vector<std::vector<Event>> pi(n + 1), ci(n + 1);
      { int j = 0; for (const Event &e : pe) { if (e.what == 'S') ++j; else pi[j].push_back(e); } }
      { int j = 0; for (const Event &e : ce) { if (e.what == 'S') ++j; else ci[j].push_back(e); } }
      int u[4] = {-1, -1, -1, -1}, c[3] = {-1, -1, -1}, d[2] = {-1, -1};
      for (int j = 0; j <= n; ++j) {
        // the waves of one interval run concurrently: reads first against the state BEFORE this interval's writes ...
        for (const Event &e : ci[j])
          if (e.what == 'D') {
            const int r = e.a;
            if (u[(r - 1) & 3] != r - 1 || c[e.b] != r || d[(r + 1) & 1] != r + 1)
              return fail("drain reads a slot that does not hold its plane", s, n, j);
          }
        // ... then the writes, none of which may touch a slot this interval's drain reads
        for (const Event &e : pi[j])
          if (e.what == 'F') {
            const int r = e.a;
            for (const Event &x : ci[j])
              if (x.what == 'D' && (((x.a - 1) & 3) == (r & 3) || x.b == e.b || ((x.a + 1) & 1) == (r & 1)))
                return fail("fill writes a slot that the drain of the same interval reads", s, n, j);
            u[r & 3] = r; c[e.b] = r; d[r & 1] = r;
          }
      }
    }
  printf("ok %d\n", cases);
  return 0;
}
