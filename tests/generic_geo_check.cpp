// Host check of the launch geometry of the generic path's bf16 and exact-fp32 kernels (csrc/generic_geo.h)
// against brute force.
// Stand-alone: built and run by tests/test_generic_geo_cpu.py with the host compiler, plain and with
// -fsanitize=address,undefined.  Without arguments it sweeps n in 1..40 plus 130, 1000 and 4099 samples, L in
// {1, 3, 7, 8, 9, 15, 30, 45, 60}, k in 1..15, the channel counts below and the row layouts in_rs = L, L + p
// and L + 2 p, for the two conv engines and their modes, and checks what kernels and workspace rely on:
//   * conv coverage: every output row and every 16-channel tile on exactly one (workgroup, wave, tile slot);
//   * conv span: walking every (row, tap) of every workgroup as conv_lds_kernel does, every input row read
//     lies in [xbase, xbase + span); LDS bytes = span * stride within the limit; a span at the limit stages
//     and one row past it gathers;
//   * conv slots: the deterministic slots (workgroup, wave row) are distinct, det_slots of them;
//   * wgrad (gf32): the row groups partition [0, R) in whole chunks, fit part_floats and the grid limits; a
//     slice minus one float is rejected;
//   * wgrad (bf16): chunk ranges partition the chunks; nco has the fewest padded tile slots (largest on
//     ties) by enumeration; KMAX is the smallest instantiation holding k; deterministic slices fit part;
//   * the pack launch: frag_elems by enumeration, the grid within its cap.
// "--table conv|wgrad|gt_wgrad|const ..." prints one launch's plan as JSON: how the Python tests learn it.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string_view>
#include <utility>
#include <vector>

#include "generic_geo.h"

using namespace apneauq::ggeo;

static int failures = 0;
static long long cases = 0;
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

static const int kLs[] = {1, 3, 7, 8, 9, 15, 30, 45, 60};
static const int kChs[] = {1, 3, 4, 8, 12, 20, 32, 36, 64, 96, 100, 132, 224, 256};
static std::vector<int> sweep_n() {
  std::vector<int> v;
  for (int n = 1; n <= 40; ++n) v.push_back(n);
  v.insert(v.end(), {130, 1000, 4099});
  return v;
}
static const char* kEngine[] = {"bf16", "gf32"};
static const char* kKind[] = {"staged", "vec", "elem"};

// ------------------------------------------------------------------------------------------------ conv
// rows: every row of [0, rows) on exactly one (workgroup, wave row, row tile, lane); slots distinct
static void check_rows(const ConvPlan& p, int engine) {
  std::vector<char> seen(p.rows, 0);
  std::set<int> slots;
  for (int bx = 0; bx < p.grid_x; ++bx)
    for (int wr = 0; wr < kWaveRows; ++wr) {
      const int slot = bx * kWaveRows + wr;
      CHECK(slots.insert(slot).second && slot < p.det_slots, "%s rows %lld: slot %d", kEngine[engine], p.rows, slot);
      for (int r = 0; r < kRT; ++r)
        for (int m = 0; m < 16; ++m) {
          const long long row = (long long)bx * kTileRows + wr * (kRT * 16) + r * 16 + m;
          if (row < p.rows) ++seen[row];
        }
    }
  for (long long r = 0; r < p.rows; ++r) CHECK(seen[r] == 1, "%s rows %lld: row %lld covered %d times", kEngine[engine], p.rows, r, seen[r]);
  CHECK((int)slots.size() == p.det_slots, "%s rows %lld: %d slots", kEngine[engine], p.rows, p.det_slots);
}

static void check_tiles(const ConvPlan& p, int engine, int cout) {
  std::vector<int> seen(p.nct, 0);
  for (int by = 0; by < p.grid_y; ++by)
    for (int wc = 0; wc < kWaveCols; ++wc)
      for (int c = 0; c < p.ct; ++c)
        if (conv_ct0(p.ct, by, wc) + c < p.nct) ++seen[conv_ct0(p.ct, by, wc) + c];
  for (int t = 0; t < p.nct; ++t) CHECK(seen[t] == 1, "%s cout %d: tile %d on %d waves", kEngine[engine], cout, t, seen[t]);
  CHECK(p.nct * 16 >= cout && (p.nct - 1) * 16 < cout, "%s cout %d: %d tiles", kEngine[engine], cout, p.nct);
  // no workgroup column without a tile; CT = 3 exactly where it leaves no empty tile slot and 4 would
  CHECK(conv_ct0(p.ct, p.grid_y - 1, 0) < p.nct, "%s cout %d: empty workgroup column", kEngine[engine], cout);
  CHECK(p.ct == 4 || (engine != kBf16 && p.ct == 3 && p.nct % 6 == 0), "%s cout %d: CT %d", kEngine[engine], cout, p.ct);
}

// the staging kernels' walk: rows the workgroups read, relative to their xbase -> the span they need
static long long span_needed(long long rows, int L, int Lp, int k, int in_rs) {
  const int pad = (k - 1) / 2;
  long long need = 0;
  for (long long row0 = 0; row0 < rows; row0 += kTileRows) {
    const long long n0 = row0 / Lp, t0 = row0 - n0 * Lp;
    const long long xbase = n0 * in_rs + t0 - pad;  // (+ in_off on both sides)
    for (long long row = row0; row < std::min(rows, row0 + kTileRows); ++row) {
      const long long rn = row / Lp, rt = row - rn * Lp;
      if (rt >= L) continue;  // the odd pooled step: no reads
      for (int tap = 0; tap < k; ++tap) {
        const long long ts = rt + tap - pad;
        if (ts < 0 || ts >= L) continue;
        const long long lr = rn * in_rs + ts - xbase;
        if (lr < 0) return -1;
        need = std::max(need, lr + 1);
      }
      // the kernels also ASSERT tap 0 .. k - 1 of the row inside the staged rows (masked taps read row 0)
      const long long lr0 = rn * in_rs + rt - pad - xbase;
      if (lr0 < 0) return -1;
      need = std::max(need, lr0 + k);
    }
  }
  return need;
}

static void check_conv() {
  const std::vector<int> ns = sweep_n();
  for (int L : kLs)
    for (int n : ns) {
      for (int engine = 0; engine < 2; ++engine)
        for (int pool = 0; pool <= (engine == kBf16); ++pool) {
          const ConvPlan p = conv_plan(engine, pool ? kInfer : kTrain, n, L, 8, 16, 3, pool, 0, true);
          CHECK(p.rows == (long long)n * p.Lp && p.Lp >= L && p.Lp - L == (pool ? L % 2 : 0) && p.lout == (pool ? L / 2 : L), "Lp %d of L %d", p.Lp, L);
          check_rows(p, engine);
          ++cases;
        }
      for (int k = 1; k <= 15; k += 2) {
        const int pad = (k - 1) / 2;
        for (int layout = 0; layout < 4; ++layout) {  // in_rs = L, L + p, L + 2 p; L with the pooled row pairs
          const bool pool = layout == 3;
          if (layout == 1 && pad == 0) continue;
          const int in_rs = pool ? L : L + (layout % 3) * pad, Lp = pool ? (L + 1) / 2 * 2 : L;
          const long long need = span_needed((long long)n * Lp, L, Lp, k, in_rs);
          for (int cin : kChs)
            for (int engine = 0; engine < (pool ? 1 : 2); ++engine) {
              const int mode = pool ? kInfer : (n % 2 ? kTrain : kLinear);
              const ConvPlan p = conv_plan(engine, mode, n, L, cin, 96, k, pool, in_rs, true);
              CHECK(need >= 0 && need <= p.span, "%s n %d L %d k %d in_rs %d: reads %lld rows, span %lld", kEngine[engine], n, L, k, in_rs, need, p.span);
              if (engine == kBf16) {
                const long long bytes = p.span * bf16_row_stride(cin);
                CHECK(p.lds_rows == p.span && p.lds_stride == bf16_row_stride(cin), "bf16 lds rows");
                CHECK((p.kind == kStaged) == (cin % 8 == 0 && bytes <= kLdsLimit) && (p.kind == kElem) == (cin % 8 != 0), "bf16 cin %d span %lld: %s", cin, p.span, kKind[p.kind]);
                CHECK(p.lds_bytes == (p.kind == kStaged ? bytes : 0) && p.lds_bytes <= kLdsLimit, "bf16 lds bytes %lld", p.lds_bytes);
                CHECK(conv_plan(engine, mode, n, L, cin, 96, k, pool, in_rs, false).kind != kStaged, "bf16 stages without a row bound");
              } else {
                CHECK(p.kind == kStaged && p.lds_bytes == 0, "gf32 has one kernel");
              }
              ++cases;
            }
        }
      }
    }
  for (int cout : {4, 12, 20, 36, 48, 96, 100, 128, 132, 192, 224, 256, 288, 1024})
    for (int engine = 0; engine < 2; ++engine) {
      check_tiles(conv_plan(engine, kTrain, 9, 60, 64, cout, 5, 0, 68, true), engine, cout);
      ++cases;
    }
  // the limit, as literals: span 160 x 512 B = 80 KB stages, one row more gathers
  const ConvPlan a = conv_plan(kBf16, kTrain, 3, 127, 248, 16, 9, 0, 151, true), b = conv_plan(kBf16, kTrain, 3, 127, 248, 16, 9, 0, 152, true);
  CHECK(a.span == 160 && a.lds_bytes == 80 * 1024 && a.kind == kStaged && b.span == 161 && b.kind == kVec && b.lds_bytes == 0, "bf16 LDS limit");
  cases += 1;
}

// ------------------------------------------------------------------------------------------------ wgrad
static void check_row_groups(long long R, int cin, int cout, int k, long long part_floats) {
  const RowGroups g = wgrad_row_groups(R, cin, cout, k, part_floats);
  const long long wfl = (long long)k * cin * cout;
  if (part_floats < wfl) {
    CHECK(g.groups == 0, "R %lld: a part of %lld floats holds no slice of %lld", R, part_floats, wfl);
    return;
  }
  CHECK(g.groups >= 1 && g.groups <= 65535 && g.wfl == wfl && g.groups * wfl <= part_floats, "R %lld (%d, %d, %d): %lld groups in %lld floats", R, cin, k, cout, g.groups, part_floats);
  CHECK(g.rpg % kWgRC == 0 && (g.groups - 1) * g.rpg < R && R <= g.groups * g.rpg, "R %lld: %lld groups of %lld rows", R, g.groups, g.rpg);
  CHECK(g.ci_t * 32 >= cin && (g.ci_t - 1) * 32 < cin && g.co_g * 64 >= cout && (g.co_g - 1) * 64 < cout && g.co_g <= 65535, "grid of cin %d cout %d", cin, cout);
  CHECK(g.groups <= ceil_div(R, 256) && g.groups <= wgrad_want_groups(cin, cout), "R %lld: %lld groups", R, g.groups);
}

static void check_gt_wgrad(long long R, int cin, int cout, int k, bool det, long long part_floats) {
  const GtWgradPlan p = gt_wgrad_plan(R, cin, cout, k, det, part_floats);
  const long long wfl = (long long)k * cin * cout;
  // nco by enumeration: fewest padded tile slots, the largest on ties
  const int tiles = (cout + 15) / 16, nmax = k <= 5 ? 4 : k <= 9 ? 3 : 2;
  std::pair<int, int> best{1 << 30, 0};
  for (int c = 1; c <= nmax; ++c) {
    int blocks = 0;
    while (blocks * 4 * c < tiles) ++blocks;
    best = std::min(best, std::make_pair(blocks * 4 * c, -c));
  }
  CHECK(p.nco == -best.second && p.n_co * 4 * p.nco == best.first, "cout %d k %d: nco %d, enumeration %d", cout, k, p.nco, -best.second);
  CHECK(p.im2col == (cin * k <= 32) && p.n_ci == (p.im2col ? 1 : (cin + 15) / 16), "cin %d k %d: im2col", cin, k);
  int kmax = 0;
  for (int c : {15, 9, 5, 3})
    if (c >= k) kmax = c;
  CHECK(p.kmax == (p.im2col ? 1 : kmax), "k %d: KMAX %d", k, p.kmax);
  if (det && part_floats < wfl) {
    CHECK(!p.ok, "a part of %lld floats holds no slice of %lld", part_floats, wfl);
    return;
  }
  CHECK(p.ok && p.wfl == wfl && p.grid == (long long)p.n_ci * p.n_co * p.rgs && p.rgs >= 1, "R %lld (%d, %d, %d): grid", R, cin, k, cout);
  CHECK(p.chunks * kChunk >= R && (p.chunks - 1) * kChunk < R, "R %lld: %lld chunks", R, p.chunks);
  CHECK((p.rgs - 1) * p.chunks_per_wg < p.chunks && p.chunks <= p.rgs * p.chunks_per_wg, "R %lld: %lld groups of %d chunks", R, p.rgs, p.chunks_per_wg);
  CHECK(!det || p.rgs * wfl <= part_floats, "R %lld: %lld slices in %lld floats", R, p.rgs, part_floats);
}

static void check_wgrad() {
  const std::vector<int> ns = sweep_n();
  for (int k = 1; k <= 15; ++k)
    for (int cin : kChs)
      for (int cout : {4, 12, 20, 36, 96, 100, 132, 224, 256}) {
        const long long wfl = (long long)k * cin * cout;
        for (int L : kLs)
          for (int n : ns) {
            const long long R = (long long)n * (L + k - 1);
            check_row_groups(R, cin, cout, k, wgrad_want_groups(cin, cout) * wfl);
            check_row_groups(R, cin, cout, k, wfl);
            check_row_groups(R, cin, cout, k, 3 * wfl + 1);
            check_row_groups(R, cin, cout, k, wfl - 1);
            check_gt_wgrad(R, cin, cout, k, false, 0);
            check_gt_wgrad(R, cin, cout, k, true, 16 * wfl);
            check_gt_wgrad(R, cin, cout, k, true, wfl);
            check_gt_wgrad(R, cin, cout, k, true, wfl - 1);
            cases += 8;
          }
      }
  // dispatch_k reaches each tap count once and nothing else
  for (int k = -1; k <= kWgKMax + 2; ++k) {
    int got = 0, calls = 0;
    const bool ok = dispatch_k<1, kWgKMax>(k, [&](auto K) { got = decltype(K)::value, ++calls; });
    CHECK(ok == (k >= 1 && k <= kWgKMax) && calls == (ok ? 1 : 0) && (!ok || got == k), "dispatch_k %d", k);
  }
}

// ------------------------------------------------------------------------------------------------ small launches
static void check_small() {
  for (long long n : {0LL, 1LL, 256LL, 257LL, 1027LL, 1LL << 20, 1LL << 34}) {
    CHECK(pack_grid(n) <= kPackGrid && pack_grid(n) * 256LL >= std::min(n, 256LL * kPackGrid), "pack grid of %lld", n);
    ++cases;
  }
  // fragments, enumerated: the (32-k step, 16-channel tile) cells that hold an element of the kernel
  for (int k = 1; k <= 15; ++k)
    for (int cin : kChs)
      for (int cout : {1, 4, 12, 20, 96, 100, 132, 256}) {
        std::vector<char> cell(((k * cin) / 32 + 1) * (cout / 16 + 1), 0);
        for (int kk = 0; kk < k * cin; ++kk)
          for (int co = 0; co < cout; ++co) cell[(kk / 32) * (cout / 16 + 1) + co / 16] = 1;
        const long long cells = std::count(cell.begin(), cell.end(), 1);
        CHECK(frag_elems(k, cin, cout) == cells * 64 * 8, "fragments of (%d, %d, %d): %lld, %lld cells", k, cin, cout, frag_elems(k, cin, cout), cells);
        ++cases;
      }
}

// ------------------------------------------------------------------------------------------------ tables
static int table_conv(char** a) {
  const int engine = std::atoi(a[0]), mode = std::atoi(a[1]), n = std::atoi(a[2]), L = std::atoi(a[3]), cin = std::atoi(a[4]),
            cout = std::atoi(a[5]), k = std::atoi(a[6]), pool = std::atoi(a[7]), in_rs = std::atoi(a[8]);
  const ConvPlan p = conv_plan(engine, mode, n, L, cin, cout, k, pool, in_rs, true);
  std::printf("{\"engine\": \"%s\", \"kind\": \"%s\", \"rows\": %lld, \"Lp\": %d, \"lout\": %d, \"in_rs\": %d, \"nstep\": %d, \"nct\": %d, \"ct\": %d,\n",
              kEngine[engine], kKind[p.kind], p.rows, p.Lp, p.lout, p.in_rs, p.nstep, p.nct, p.ct);
  std::printf(" \"grid\": [%d, %d], \"threads\": %d, \"span\": %lld, \"lds_rows\": %d, \"lds_stride\": %d, \"lds_bytes\": %lld,\n", p.grid_x, p.grid_y,
              kThreads, p.span, p.lds_rows, p.lds_stride, p.lds_bytes);
  std::printf(" \"lds_limit_bytes\": %d, \"det_slots\": %d,\n", kLdsLimit, p.det_slots);
  std::printf(" \"nc\": [");  // channel tiles of each (workgroup column, wave column)
  for (int by = 0; by < p.grid_y; ++by)
    std::printf("%s[%d, %d]", by ? ", " : "", std::clamp(p.nct - conv_ct0(p.ct, by, 0), 0, p.ct), std::clamp(p.nct - conv_ct0(p.ct, by, 1), 0, p.ct));
  std::printf("]}\n");
  return 0;
}

static int table_wgrad(char** a) {
  const long long R = std::atoll(a[0]), part = std::atoll(a[4]);
  const int cin = std::atoi(a[1]), cout = std::atoi(a[2]), k = std::atoi(a[3]);
  const RowGroups g = wgrad_row_groups(R, cin, cout, k, part);
  std::printf("{\"groups\": %lld, \"rpg\": %lld, \"grid\": [%d, %d, %lld], \"wfl\": %lld, \"want\": %lld}\n", g.groups, g.rpg, g.ci_t, g.co_g, g.groups, g.wfl,
              wgrad_want_groups(cin, cout));
  return 0;
}

static int table_gt_wgrad(char** a) {
  const long long R = std::atoll(a[0]), part = std::atoll(a[5]);
  const int cin = std::atoi(a[1]), cout = std::atoi(a[2]), k = std::atoi(a[3]), det = std::atoi(a[4]);
  const GtWgradPlan p = gt_wgrad_plan(R, cin, cout, k, det != 0, part);
  std::printf("{\"ok\": %s, \"im2col\": %s, \"nco\": %d, \"kmax\": %d, \"n_ci\": %d, \"n_co\": %d, \"chunks\": %lld, \"chunks_per_wg\": %d, \"rgs\": %lld, "
              "\"grid\": %lld, \"wfl\": %lld}\n",
              p.ok ? "true" : "false", p.im2col ? "true" : "false", p.nco, p.kmax, p.n_ci, p.n_co, p.chunks, p.chunks_per_wg, p.rgs, p.grid, p.wfl);
  return 0;
}

static int table_const() {
  std::printf("{\"tile_rows\": %d, \"stat_slots\": %d, \"lds_limit_bytes\": %d, \"wg_rc\": %d, \"chunk\": %d, \"wg_kmax\": %d}\n", kTileRows, kStatSlots,
              kLdsLimit, kWgRC, kChunk, kWgKMax);
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 3 && std::string_view(argv[1]) == "--table") {
    const std::string_view what(argv[2]);
    if (what == "conv" && argc == 12) return table_conv(argv + 3);
    if (what == "wgrad" && argc == 8) return table_wgrad(argv + 3);
    if (what == "gt_wgrad" && argc == 9) return table_gt_wgrad(argv + 3);
    if (what == "const" && argc == 3) return table_const();
  }
  if (argc != 1) {
    std::printf("usage: %s [--table conv ENGINE MODE n L cin cout k pool in_rs | --table wgrad R cin cout k part_floats |\n"
                "          --table gt_wgrad R cin cout k det part_floats | --table const]\n", argv[0]);
    return 2;
  }
  check_conv();
  check_wgrad();
  check_small();
  std::printf("%lld cases, %d failures\n", cases, failures);
  return failures ? 1 : 0;
}
