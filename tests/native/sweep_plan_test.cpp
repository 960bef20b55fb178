// CPU test of the launch-planning arithmetic the sweep steps share (lpopc_amd/csrc/rpm_engine.hpp): deal_columns and clamp_tile
// over every small input, against the properties the planners of the batched carry and extraction rely on.  Compiled and run by
// tests/test_sweep_plan_cpu.py.
#include <cstdio>
#include <cstdlib>

#include "../../lpopc_amd/csrc/rpm_engine.hpp"

#define CHECK(c)                                                         \
  do {                                                                   \
    if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } \
  } while (0)

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
  std::printf("ok: %ld cases\n", cases);
  return 0;
}
