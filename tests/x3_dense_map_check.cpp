// Host check of the dense-row index map of the x3 layer kernels (csrc/x3_dense_map.h) against brute
// force.  Stand-alone: built and run by tests/test_x3_dense_map_cpu.py with the host compiler.
//   * every valid (window, step) of a group is a row of exactly one tile, at the (w, t) the map says;
//   * every LDS row the staging writes lies inside the buffer, is no fixed zero row, and is written once;
//   * every LDS row a tap of a valid tile row reads is the staged row of (w, t + j), or a fixed zero row
//     exactly where t + j falls outside the window.
#include <cstdio>
#include <vector>

#include "x3_dense_map.h"

namespace dm = apneauq::x3::dense;

static int failures = 0;
#define CHECK(cond, ...)                         \
  do {                                           \
    if (!(cond)) {                               \
      if (failures++ < 20) {                     \
        std::printf("FAIL %s: ", #cond);         \
        std::printf(__VA_ARGS__);                \
        std::printf("\n");                       \
      }                                          \
    }                                            \
  } while (0)

static bool zero_row(int row, int rows) {
  if (row < dm::kHaloRows || row >= dm::lds_rows(rows) - dm::kHaloRows) return true;
  return (row - dm::kHaloRows) % dm::kSlot >= dm::kLen;
}

static void check(int n_win, int rows, int pad) {
  const long long total = 60ll * n_win;
  const long long tiles = dm::tiles(n_win, rows);
  CHECK(tiles * rows >= total && (tiles - 1) * rows < total, "n_win %d rows %d", n_win, rows);
  std::vector<int> cover(total, 0);
  for (long long tl = 0; tl < tiles; ++tl) {
    const long long d0 = dm::first_row(tl, rows);
    const int wf = dm::first_window(tl, rows), off = dm::offset(tl, rows);
    CHECK(60ll * wf + off == d0 && off >= 0 && off < 60, "tile %lld", tl);
    CHECK(dm::windows(off, rows) <= dm::max_windows(rows), "tile %lld off %d rows %d", tl, off, rows);
    // what the staging writes: LDS row -> global dense row (or -1)
    std::vector<long long> lds(dm::lds_rows(rows), -1);
    for (int ri = 0; ri < dm::staged_units(rows, pad); ++ri) {
      const int dl = off - pad + ri;
      if (!dm::staged(dl, off, rows, pad)) continue;
      const int row = dm::lds_row(dl);
      CHECK(row >= 0 && row < dm::lds_rows(rows), "tile %lld dl %d row %d", tl, dl, row);
      if (row < 0 || row >= dm::lds_rows(rows)) continue;
      CHECK(!zero_row(row, rows), "tile %lld dl %d writes zero row %d", tl, dl, row);
      CHECK(lds[row] < 0, "tile %lld LDS row %d written twice", tl, row);
      CHECK(row == dm::kHaloRows + dm::kSlot * dm::slot_of(dl) + dm::step_of(dl), "tile %lld dl %d", tl, dl);
      lds[row] = 60ll * wf + dl;
    }
    for (int r = 0; r < rows; ++r) {
      const long long d = d0 + r;
      const int dl = off + r, w = wf + dm::slot_of(dl), t = dm::step_of(dl);
      CHECK(w == d / 60 && t == d % 60, "tile %lld row %d", tl, r);
      CHECK(dm::slot_of(dl) < dm::max_windows(rows), "tile %lld row %d slot", tl, r);
      const int row = dm::lds_row(dl);
      for (int j = -pad; j <= pad; ++j)  // in bounds for the rows past the group's end too
        CHECK(row + j >= 0 && row + j < dm::lds_rows(rows), "tile %lld row %d tap %d", tl, r, j);
      if (d >= total) continue;
      ++cover[d];
      CHECK(dm::staged(dl, off, rows, pad) && lds[row] == d, "tile %lld row %d not staged", tl, r);
      for (int j = -pad; j <= pad; ++j) {
        const bool inside = t + j >= 0 && t + j < 60;
        if (inside)
          CHECK(lds[row + j] == d + j, "tile %lld row %d tap %d reads %lld", tl, r, j, lds[row + j]);
        else
          CHECK(zero_row(row + j, rows) && lds[row + j] < 0, "tile %lld row %d tap %d: no zero row", tl, r, j);
      }
    }
  }
  for (long long d = 0; d < total; ++d) CHECK(cover[d] == 1, "n_win %d rows %d: row %lld covered %d times", n_win, rows, d, cover[d]);
}

int main() {
  static_assert(dm::max_windows(128) == 4 && dm::max_windows(256) == 6, "window slots per tile");
  static_assert(dm::lds_rows(128) == 264 && dm::lds_rows(256) == 392, "LDS rows per chunk buffer");
  for (int dl = 0; dl < 1024; ++dl)  // the multiply-and-shift division of the map
    CHECK(dm::slot_of(dl) == dl / 60 && dm::step_of(dl) == dl % 60, "dl %d", dl);
  const int wins[] = {1, 7, 67}, sizes[] = {128, 256};
  int cases = 0;
  for (int n_win : wins)
    for (int rows : sizes)
      for (int pad = 1; pad <= 4; ++pad, ++cases) check(n_win, rows, pad);
  std::printf("%d cases, %d failures\n", cases, failures);
  return failures ? 1 : 0;
}
