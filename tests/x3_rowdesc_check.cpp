// Host check of the per-tile row descriptors of the x3 layer kernels (csrc/x3_dense_map.h) against brute
// force.  Stand-alone: built and run by tests/test_x3_rowdesc_cpu.py with the host compiler, once plain
// and once with -fsanitize=address,undefined.
//   * desc_pack / desc_* round-trip every field over its whole range;
//   * for every tile offset (0, 4, .., 56), both tile sizes and PAD 1..4, every row rel = -PAD ..
//     rows + PAD - 1 has the descriptor brute force gives it: 0 exactly where the row is not staged, else
//     LDS row 4 + 64 (dl / 60) + dl % 60, step dl % 60, window slot dl / 60, and valid iff rel < rows_left;
//   * over whole groups (1, 7, 67 windows), the linear forms the kernels use agree with (window, step):
//     the global row of row rel is first_row + rel, and valid is window < n_win;
//   * whole-window slot tiles (row 60 s + t) likewise;
//   * mask_word(key, t) ^ (c >> 1) is the hash input key ^ (t << 9 | c >> 1) of the dropout stream.
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

// brute force: is row dl (relative to the tile's first window) staged by a tile at `off` of `rows` rows?
static bool staged_brute(int rel, int off, int rows, int pad) {
  const int dl = off + rel;
  if (rel < -pad || rel >= rows + pad || dl < 0) return false;
  const int last_window = (off + rows - 1) / 60;  // the last window that owns a row of the tile
  return dl / 60 <= last_window;
}

static void check_tile(int off, int rows, int pad, int rows_left) {
  std::vector<int> seen(dm::lds_rows(rows), 0);
  for (int rel = -pad - 2; rel < rows + pad + 2; ++rel) {
    const unsigned d = dm::row_desc(rel, off, rows, pad, rows_left);
    if (!staged_brute(rel, off, rows, pad)) {
      CHECK(d == 0u, "off %d rows %d pad %d rel %d: unstaged row has descriptor %u", off, rows, pad, rel, d);
      continue;
    }
    const int dl = off + rel, s = dl / 60, t = dl % 60, lrow = 4 + 64 * s + t;
    CHECK(d != 0u, "off %d rows %d pad %d rel %d: staged row without descriptor", off, rows, pad, rel);
    CHECK(dm::desc_lds_row(d) == lrow, "off %d rows %d rel %d: LDS row %d, want %d", off, rows, rel, dm::desc_lds_row(d), lrow);
    CHECK(dm::desc_step(d) == t, "off %d rows %d rel %d: step %d, want %d", off, rows, rel, dm::desc_step(d), t);
    CHECK(dm::desc_slot(d) == s, "off %d rows %d rel %d: slot %d, want %d", off, rows, rel, dm::desc_slot(d), s);
    CHECK(dm::desc_valid(d) == (rel < rows_left), "off %d rows %d rel %d left %d: valid", off, rows, rel, rows_left);
    CHECK(lrow >= dm::kHaloRows && lrow < dm::lds_rows(rows) - dm::kHaloRows, "off %d rows %d rel %d: LDS row %d", off, rows, rel, lrow);
    if (lrow >= 0 && lrow < dm::lds_rows(rows)) CHECK(seen[lrow]++ == 0, "off %d rows %d: LDS row %d twice", off, rows, lrow);
  }
}

// whole groups: the descriptors of every tile against (window, step) of the global dense row
static void check_group(int n_win, int rows, int pad) {
  const long long total = 60ll * n_win;
  for (long long tl = 0; tl < dm::tiles(n_win, rows); ++tl) {
    const long long d0 = dm::first_row(tl, rows);
    const int wf = dm::first_window(tl, rows), off = dm::offset(tl, rows);
    const long long left = total - d0;
    const int rows_left = (int)(left < 1024 ? left : 1024);  // the kernels' clamp
    CHECK(rows_left > 0, "n_win %d tile %lld starts past the group", n_win, tl);
    for (int rel = -pad; rel < rows + pad; ++rel) {
      const unsigned d = dm::row_desc(rel, off, rows, pad, rows_left);
      if (d == 0u) continue;
      const long long grow = d0 + rel;  // the linear global row the kernels address
      CHECK(grow >= 0, "n_win %d tile %lld rel %d: staged row before the group", n_win, tl, rel);
      const int w = wf + dm::desc_slot(d), t = dm::desc_step(d);
      CHECK(60ll * w + t == grow, "n_win %d tile %lld rel %d: (%d, %d) is not row %lld", n_win, tl, rel, w, t, grow);
      CHECK(dm::desc_valid(d) == (w < n_win), "n_win %d tile %lld rel %d: valid", n_win, tl, rel);
    }
  }
}

int main() {
  // the packed fields
  static_assert(dm::lds_rows(256) <= (1 << dm::kDescStepShift), "LDS row field");
  static_assert(dm::max_windows(256) <= 8, "window slot field");
  for (int lrow = 0; lrow < 512; lrow += 3)
    for (int t = 0; t < 60; ++t)
      for (int s = 0; s < 8; ++s)
        for (int v = 0; v < 2; ++v) {
          const unsigned d = dm::desc_pack(lrow, t, s, v != 0);
          CHECK(dm::desc_lds_row(d) == lrow && dm::desc_step(d) == t && dm::desc_slot(d) == s && dm::desc_valid(d) == (v != 0),
                "pack (%d, %d, %d, %d)", lrow, t, s, v);
          CHECK((d == 0u) == (lrow == 0 && t == 0 && s == 0 && v == 0), "zero descriptor (%d, %d, %d, %d)", lrow, t, s, v);
        }
  int cases = 0;
  const int sizes[] = {128, 256};
  for (int rows : sizes)
    for (int pad = 1; pad <= 4; ++pad)
      for (int off = 0; off < 60; off += 4, ++cases) {
        const int lefts[] = {1, 37, 60, rows - 1, rows, rows + pad, 1024};
        for (int left : lefts) check_tile(off, rows, pad, left);
      }
  const int wins[] = {1, 7, 67};
  for (int n_win : wins)
    for (int rows : sizes)
      for (int pad = 1; pad <= 4; ++pad) check_group(n_win, rows, pad);
  // whole-window slot tiles: S = 2 or 4 windows, row ri = 60 s + t
  for (int S = 2; S <= 4; S += 2)
    for (int left = 0; left <= 60 * S; left += 60)
      for (int ri = 0; ri < 60 * S; ++ri) {
        const unsigned d = dm::slot_row_desc(ri, left);
        CHECK(dm::desc_lds_row(d) == 4 + 64 * (ri / 60) + ri % 60 && dm::desc_step(d) == ri % 60 && dm::desc_slot(d) == ri / 60 &&
                  dm::desc_valid(d) == (ri / 60 < left / 60) && d != 0u,
              "slot tile S %d left %d row %d", S, left, ri);
      }
  // the mask word
  const unsigned keys[] = {0u, 1u, 0x9E3779B9u, 0xFFFFFFFFu, 0x12345678u};
  for (unsigned key : keys)
    for (int t = 0; t < 60; ++t)
      for (unsigned c = 0; c < 1024; c += 2)
        CHECK((dm::mask_word(key, t) ^ (c >> 1)) == (key ^ (((unsigned)t << 9) | (c >> 1))), "mask word key %u t %d c %u", key, t, c);
  std::printf("%d tile cases, %d failures\n", cases, failures);
  return failures ? 1 : 0;
}
