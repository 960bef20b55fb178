// CPU test of the host arithmetic the sweep steps share (lpopc_amd/csrc/rpm_engine.hpp): deal_columns, clamp_tile, halve_tile,
// split_columns, lds_budget and the overlap rule over every small input, against the properties the planners and argument checks
// of the batched steps rely on.  Compiled and run by tests/test_sweep_plan_cpu.py.
#include <cstdio>
#include <cstdlib>

#include "../../lpopc_amd/csrc/rpm_engine.hpp"

#define CHECK(c)                                                         \
  do {                                                                   \
    if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } \
  } while (0)

// the halving of `start` one step larger than r (r itself when r is start); 0 when r is neither start nor one of its halvings
static int halving_above(int start, int r) {
  for (int v = start, above = start; v >= 1; above = v, v >>= 1)
    if (v == r) return above;
  return 0;
}

int main() {
  long cases = 0;
  for (int most = 1; most <= 48; ++most) {
    const auto none = rpm::deal_columns(0, most);   // a phase without columns: one workgroup that stages none
    CHECK(none.first == 1 && none.second == 0);
    for (int cols = 1; cols <= 96; ++cols, ++cases) {
      const auto [n_groups, per] = rpm::deal_columns(cols, most);
      CHECK(n_groups >= 1 && (n_groups - 1) * most < cols);   // the fewest workgroups: one fewer could not hold the columns
      CHECK(per >= 1 && per <= most);               // a workgroup's share fits
      CHECK(n_groups * per >= cols);                // every column is dealt
      CHECK((n_groups - 1) * per < cols);           // no workgroup is left without a column
      int walked = 0;                               // the planners' walk: col0 += per until the columns run out
      for (int col0 = 0; col0 < cols; col0 += per) ++walked;
      CHECK(walked == n_groups);
    }
  }
  for (int TB0 = 1; TB0 <= 64; TB0 <<= 1)
    for (int B = 1; B <= 200; ++B, ++cases) {
      const int TB = rpm::clamp_tile(TB0, B);
      CHECK(TB >= 1 && TB <= TB0 && TB0 % TB == 0);   // the tile itself or one of its halvings
      CHECK(TB == 1 || TB / 2 < B);                 // half the tile would not hold the instances
      CHECK(TB == TB0 || TB >= B);                  // a halved tile still holds them all
    }
  CHECK(rpm::clamp_tile(3, 1) == 1 && rpm::clamp_tile(6, 2) == 3);   // tiles that are no power of two halve the same way

  // halve_tile under every threshold predicate, in both orders the planners use: clamped first (carry, roll-out, extraction) and
  // clamped afterwards (mesh-error estimate).  3 and 6 are among the start tiles: they halve 3, 1 and 6, 3, 1.
  for (int TB0 = 1; TB0 <= 64; ++TB0)
    for (int B = 1; B <= 200; ++B)
      for (int t = 0; t <= 64; ++t, ++cases) {
        auto fits = [t](int TB) { return TB <= t; };
        const int start = rpm::clamp_tile(TB0, B), r = rpm::halve_tile(start, fits);
        if (t == 0) {
          CHECK(r == 0 && rpm::halve_tile(TB0, fits) == 0);   // not even one instance per workgroup: refused
          continue;
        }
        const int above = halving_above(start, r);
        CHECK(r >= 1 && above != 0 && fits(r));     // the start tile or one of its halvings, and it fits
        CHECK(above == r || !fits(above));          // the halving one step larger does not
        const int h = rpm::halve_tile(TB0, fits), above_h = halving_above(TB0, h), late = rpm::clamp_tile(h, B);
        CHECK(h >= 1 && above_h != 0 && fits(h) && (above_h == h || !fits(above_h)));
        CHECK(halving_above(h, late) != 0 && fits(late) && (late == 1 || late / 2 < B));   // the clamp only halves further
      }
  CHECK(rpm::halve_tile(3, [](int TB) { return TB <= 2; }) == 1 && rpm::halve_tile(6, [](int TB) { return TB <= 5; }) == 3);

  // split_columns under every threshold predicate
  for (int t = 1; t <= 48; ++t)
    for (int cols = 0; cols <= 96; ++cols, ++cases) {
      const auto groups = rpm::split_columns(cols, [t](int ncols) { return ncols <= t; });
      if (cols == 0) {   // the carry's phase without columns: one group of none (the extraction skips such a phase itself)
        CHECK(groups.size() == 1 && groups[0].first == 0 && groups[0].second == 0);
        continue;
      }
      int next = 0;
      for (const auto& [col0, ncols] : groups) {
        CHECK(col0 == next && ncols >= 1 && ncols <= t);   // disjoint, contiguous, and each group fits
        next += ncols;
      }
      CHECK(next == cols);                          // every column is covered
      CHECK(int(groups.size()) == rpm::deal_columns(cols, t < cols ? t : cols).first);   // the largest fitting width's count
    }

  CHECK(rpm::lds_budget(0, 1000) == 1000 && rpm::lds_budget(-1, 1000) == 1000 && rpm::lds_budget(999, 1000) == 999 &&
        rpm::lds_budget(1001, 1000) == 1000);
  cases += 4;

  // the overlap rule on one buffer: a = doubles [10, 20)
  static double buf[64];
  auto range = [](const char* name, int first, int count) { return rpm::ByteRange{name, buf + first, size_t(count) * sizeof(double)}; };
  const rpm::ByteRange a = range("a", 10, 10);
  CHECK(rpm::ranges_overlap(a, range("b", 19, 10)) && rpm::ranges_overlap(range("b", 19, 10), a));   // by one double at a's end
  CHECK(rpm::ranges_overlap(a, range("b", 0, 11)) && rpm::ranges_overlap(range("b", 0, 11), a));     // by one double at its start
  CHECK(rpm::ranges_overlap(a, a) && rpm::ranges_overlap(a, range("b", 12, 2)));                     // the same array, one inside
  CHECK(!rpm::ranges_overlap(a, range("b", 20, 10)) && !rpm::ranges_overlap(a, range("b", 0, 10)));  // abutting exactly
  CHECK(!rpm::ranges_overlap(a, rpm::ByteRange{"b", nullptr, 80}) && !rpm::ranges_overlap(rpm::ByteRange{"b", nullptr, 80}, a));
  CHECK(!rpm::ranges_overlap(a, range("b", 12, 0)) && !rpm::ranges_overlap(range("b", 12, 0), a));   // an empty range
  cases += 12;
  {
    const rpm::ByteRange* hit[2] = {nullptr, nullptr};
    const rpm::ByteRange in[2] = {range("i0", 0, 8), range("i1", 8, 8)};
    const rpm::ByteRange apart[3] = {range("o0", 16, 8), rpm::ByteRange{"o1", nullptr, 64}, range("o2", 24, 8)};
    CHECK(!rpm::first_overlap(apart, 3, in, 2, hit) && !rpm::first_overlap(apart, 0, in, 2, hit));
    // two pairs at once: the walk is output by output, each against the inputs in order, then against the later outputs
    const rpm::ByteRange both_in[2] = {range("o0", 7, 2), range("o1", 32, 8)};             // (o0, i0) and (o0, i1)
    CHECK(rpm::first_overlap(both_in, 2, in, 2, hit) && hit[0] == &both_in[0] && hit[1] == &in[0]);
    const rpm::ByteRange in_then_out[2] = {range("o0", 15, 9), range("o1", 23, 8)};        // (o0, i1) and (o0, o1)
    CHECK(rpm::first_overlap(in_then_out, 2, in, 2, hit) && hit[0] == &in_then_out[0] && hit[1] == &in[1]);
    const rpm::ByteRange out_then_in[3] = {range("o0", 16, 8), range("o1", 4, 2), range("o2", 23, 8)};   // (o0, o2) and (o1, i0)
    CHECK(rpm::first_overlap(out_then_in, 3, in, 2, hit) && hit[0] == &out_then_in[0] && hit[1] == &out_then_in[2]);
    CHECK(rpm::first_overlap(out_then_in, 3, in, 0, hit) && hit[1] == &out_then_in[2]);    // outputs only
    CHECK(rpm::first_overlap(&out_then_in[1], 1, in, 2, hit) && hit[0] == &out_then_in[1] && hit[1] == &in[0]);
    CHECK(!rpm::first_overlap(&out_then_in[1], 1, in + 1, 1, hit));                        // an input left out of the walk
    cases += 8;
  }
  std::printf("ok: %ld cases\n", cases);
  return 0;
}
