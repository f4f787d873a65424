// Host check of the x3 layer kernel's geometry (csrc/x3_geo.h) against brute force.  Stand-alone: built and run
// by tests/test_x3_geo_cpu.py with the host compiler, once plain and once with -fsanitize=address,undefined, and
// once per A/B table under tools/probes/x3_tables/ (-DAPNEAUQ_X3_TABLE=...).  No device code, no GPU.
// For every row of the layer table, in every variant the launch code instantiates (per-sample prescale with LW,
// batch moments with LWB, dense rows where DENSE && !LAST):
//   * carve: the LDS regions are in order, disjoint, aligned for their element type and end at `bytes`;
//     WPC * bytes <= 160 KiB; bytes is what the formula the launch code used before x3_geo.h gives (restated);
//   * staging cover: every (row, channel quad) of a chunk that must be staged is held by exactly one (staging
//     thread, unit) and no unit names another row -- slot tiles: the S * 60 valid rows; dense tiles: the tile's
//     rows plus the edge rows dense::staged admits, for every tile offset 0, 4, .., 56; the edge waves are
//     staging waves, and Cfg::edge_wave is the formula the kernel writes out;
//   * row tables: kTabRows rows written by kST threads in ceil(kTabRows / kST) steps, each row once;
//   * mask table: over chunk iterations 0 .. NCH - 2 every word of [kRows][COUT / 16] is written exactly once;
//   * wave tiling: the MFMA waves' (ct0, rt0) blocks tile the NCTA x 4 S accumulator tiles exactly once, RG
//     divides NRT, the workgroup fits 1024 threads and waves_per_eu is the waves per SIMD of WPC workgroups;
//   * tile walk: the workgroups' [tile_begin(wg), tile_begin(wg + 1)) partition [0, tiles) evenly for every grid
//     1 .. 600, and tile_geo equals a brute-force walk over the groups' windows;
//   * the per-layer record (layer_info) says what the row's Cfg says.
#include <cstdio>
#include <vector>

#include "x3_geo.h"

namespace x3 = apneauq::x3;
namespace dm = apneauq::x3::dense;

static int failures = 0, configs = 0;
#define CHECK(cond, ...)                 \
  do {                                   \
    if (!(cond)) {                       \
      if (failures++ < 30) {             \
        std::printf("FAIL %s: ", #cond); \
        std::printf(__VA_ARGS__);        \
        std::printf("\n");               \
      }                                  \
    }                                    \
  } while (0)

// the launch size as the launch code computed it before the carve was stated in x3_geo.h
static int lds_bytes_before(int S, int cin, int cout, int ck, int ks, int lw, bool dense_rows) {
  const int row_b = 4 * ck + 32;
  const int buf = (dense_rows ? dm::lds_rows(64 * S) : 4 + 64 * S + 4) * row_b;
  const bool mask_tab = dense_rows && lw > 0 && cin == 96 && cout == 256 && ks == 9;
  return 2 * buf + 2 * cout * 8 + 2 * S * 4 + (dense_rows ? 2 * 64 * S * 4 + 2 * (64 * S + (ks - 1)) * 8 : 0) +
         (mask_tab ? 64 * S * (cout / 16) * 2 : 0);
}

// brute force: is row rel of a dense tile at `off` of `rows` rows staged?  The tile's rows, and up to `pad` rows
// past either edge where their window also owns a row of the tile.
static bool staged_brute(int rel, int off, int rows, int pad) {
  const int dl = off + rel;
  if (rel < -pad || rel >= rows + pad || dl < 0) return false;
  return dl / 60 <= (off + rows - 1) / 60;
}

template <bool DENSE, int S>
static void check_tile_walk(const char* tag) {
  const int wins[] = {1, 7, 67, 16384}, grps[] = {1, 3, 50};
  const int tile_rows = 64 * S;
  for (int n_win : wins)
    for (int groups : grps) {
      // tiles per group, brute force: count tile starts below the group's end
      int tpg = 0;
      if (DENSE) {
        for (long long d = 0; d < 60ll * n_win; d += tile_rows) ++tpg;
      } else {
        for (int w = 0; w < n_win; w += S) ++tpg;
      }
      CHECK(x3::tiles_per_group(DENSE, n_win, S) == tpg, "%s n_win %d: tiles per group %d, want %d", tag, n_win,
            x3::tiles_per_group(DENSE, n_win, S), tpg);
      CHECK(x3::tiles_per_group<long long>(DENSE, n_win, S) == tpg, "%s n_win %d: 64-bit tiles per group", tag, n_win);
      const int total = tpg * groups;
      for (int grid = 1; grid <= 600; ++grid) {
        CHECK(x3::tile_begin(0, total, grid) == 0 && x3::tile_begin(grid, total, grid) == total,
              "%s n_win %d groups %d grid %d: ends", tag, n_win, groups, grid);
        for (int wg = 0; wg < grid; ++wg) {
          const int n = x3::tile_begin(wg + 1, total, grid) - x3::tile_begin(wg, total, grid);
          CHECK(n == total / grid || n == (total + grid - 1) / grid, "%s n_win %d groups %d grid %d wg %d: %d tiles", tag,
                n_win, groups, grid, wg, n);
        }
      }
      if (n_win > 67 || groups > 3) continue;
      int tile = 0;
      for (int g = 0; g < groups; ++g)
        for (int tl = 0; tl < tpg; ++tl, ++tile) {
          const x3::Geo G = x3::tile_geo<DENSE, S>(tile, tpg, n_win);
          const int w0 = tl * (DENSE ? tile_rows : S);  // first dense row / first window
          const int wf = DENSE ? w0 / 60 : w0, off = DENSE ? w0 % 60 : 0;
          int left = 0;  // rows from the tile's first row to the end of the group, counted
          for (long long d = 60ll * wf + off; d < 60ll * n_win && left < 1024; ++d) ++left;
          CHECK(G.g == g && G.w0 == w0 && G.wf == wf && G.off == off && G.rows_left == left,
                "%s n_win %d groups %d tile %d: (%d %d %d %d %d), want (%d %d %d %d %d)", tag, n_win, groups, tile, G.g, G.w0,
                G.wf, G.off, G.rows_left, g, w0, wf, off, left);
          CHECK(left > 0 && wf < n_win, "%s n_win %d tile %d starts past the group", tag, n_win, tile);
        }
    }
}

template <int CIN, int COUT, int KS, int S, int WM, int WN, bool LAST, int LW, int CK, int WPC, bool PS, bool DENSE>
static void check_cfg(int layer, const char* variant) {
  using C = x3::Cfg<CIN, COUT, KS, S, WM, WN, LAST, LW, CK, WPC, PS, DENSE>;
  char tag[64];
  std::snprintf(tag, sizeof tag, "layer %d %s", layer, variant);
  ++configs;
  constexpr int kRows = 64 * S, PAD = (KS - 1) / 2, kQ = CK / 4;
  static_assert(KS % 2 == 1, "odd kernel sizes");
  CHECK(C::kRows == kRows && C::PAD == PAD && C::kQ == kQ, "%s: basic constants", tag);

  // ---- carve
  const int lds_rows = DENSE ? dm::lds_rows(kRows) : 4 + 64 * S + 4;
  CHECK(C::kBufB == lds_rows * (4 * CK + 32) && C::kBufB % 16 == 0, "%s: chunk buffer %d B", tag, C::kBufB);
  const int off[7] = {C::buf, C::st, C::wsc, C::ektab, C::stab, C::mtab, C::bytes};
  const int size[6] = {2 * C::kBufB,
                       2 * COUT * 8,
                       2 * S * 4,
                       DENSE ? 2 * kRows * 4 : 0,
                       DENSE ? 2 * (kRows + 2 * PAD) * 8 : 0,
                       C::kMaskTab ? kRows * (COUT / 16) * 2 : 0};
  const int align[6] = {16, 8, 4, 4, 8, 2};
  const char* name[6] = {"buf", "st", "wsc", "ektab", "stab", "mtab"};
  CHECK(off[0] == 0, "%s: carve starts at %d", tag, off[0]);
  for (int i = 0; i < 6; ++i) {
    CHECK(off[i] + size[i] == off[i + 1], "%s: %s at %d + %d B, next region at %d", tag, name[i], off[i], size[i], off[i + 1]);
    CHECK(off[i] % align[i] == 0, "%s: %s at %d is not %d-B aligned", tag, name[i], off[i], align[i]);
  }
  CHECK(WPC * C::bytes <= 160 * 1024, "%s: %d x %d B of LDS", tag, WPC, C::bytes);
  const int before = lds_bytes_before(S, CIN, COUT, CK, KS, LW, DENSE);
  CHECK(C::bytes == before, "%s: %d B, the earlier formula gives %d", tag, C::bytes, before);
  std::printf("%s: LDS %d B\n", tag, C::bytes);

  // ---- staging cover
  const int w_first = C::kSBase / 64;  // first staging wave
  CHECK(C::kST == 64 * C::SW && C::SW >= 1 && w_first + C::SW <= C::NW, "%s: staging waves %d + %d of %d", tag, w_first, C::SW,
        C::NW);
  CHECK(C::kSBase == (LW > 0 ? 64 * WM * WN : 0), "%s: first staging thread", tag);
  CHECK(C::kEdgeWaves <= C::SW, "%s: %d edge waves, %d staging waves", tag, C::kEdgeWaves, C::SW);
  for (int wave = 0; wave < C::NW; ++wave)  // the kernel writes the formula out
    CHECK(C::edge_wave(wave) == (DENSE && wave >= C::kSBase / 64 && wave - C::kSBase / 64 < C::kEdgeWaves), "%s: edge wave %d", tag,
          wave);
  if (!DENSE) {
    std::vector<int> held(S * 60 * kQ, 0);
    for (int i = 0; i < C::kST; ++i)
      for (int u = 0; u < C::kNU; ++u) {
        const int ri = C::slot_unit_row(u, i);
        CHECK(ri >= 0, "%s: thread %d unit %d row %d", tag, i, u, ri);
        if (ri >= 0 && ri < S * 60) ++held[ri * kQ + i % kQ];  // (the kernel skips ri >= kValidRows)
      }
    CHECK(C::kValidRows == S * 60, "%s: valid rows", tag);
    for (int x = 0; x < S * 60 * kQ; ++x) CHECK(held[x] == 1, "%s: row %d quad %d held %d times", tag, x / kQ, x % kQ, held[x]);
  } else {
    for (int toff = 0; toff < 60; toff += 4) {
      std::vector<int> held((kRows + 2 * PAD) * kQ, 0);
      for (int i = 0; i < C::kST; ++i) {
        const bool edge = C::edge_wave(w_first + i / 64);
        for (int u = 0; u < C::kNU; ++u) {
          int rel = 0;
          bool have = C::unit_row(u, i, edge, rel);
          if (u >= C::kMainU) have = have && dm::staged(toff + rel, toff, kRows, PAD);  // as load_chunk does
          if (!have) continue;
          CHECK(rel >= -PAD && rel < kRows + PAD, "%s off %d: thread %d unit %d names row %d", tag, toff, i, u, rel);
          if (rel >= -PAD && rel < kRows + PAD) ++held[(rel + PAD) * kQ + i % kQ];
        }
      }
      for (int rel = -PAD; rel < kRows + PAD; ++rel)
        for (int q = 0; q < kQ; ++q) {
          const int want = staged_brute(rel, toff, kRows, PAD) ? 1 : 0;
          CHECK((rel < 0 || rel >= kRows || want == 1), "%s off %d: tile row %d not staged", tag, toff, rel);
          CHECK(held[(rel + PAD) * kQ + q] == want, "%s off %d: row %d quad %d held %d times, want %d", tag, toff, rel, q,
                held[(rel + PAD) * kQ + q], want);
        }
    }
  }

  // ---- row tables
  {
    CHECK(C::kTabRows == kRows + 2 * PAD, "%s: %d table rows", tag, C::kTabRows);
    std::vector<int> written(C::kTabRows, 0);
    int steps = 0;
    for (int i0 = 0; i0 < C::kTabRows; i0 += C::kST, ++steps)  // write_tables' loop
      for (int t = 0; t < C::kST; ++t)
        if (i0 + t < C::kTabRows) ++written[i0 + t];
    CHECK(steps == (C::kTabRows + C::kST - 1) / C::kST, "%s: %d table steps", tag, steps);
    for (int r = 0; r < C::kTabRows; ++r) CHECK(written[r] == 1, "%s: table row %d written %d times", tag, r, written[r]);
    CHECK(!DENSE || C::NCH >= 2, "%s: row tables need two chunks per tile", tag);
  }

  // ---- mask table
  CHECK(C::kMaskTab == (DENSE && LW > 0 && CIN == 96 && COUT == 256 && KS == 9), "%s: mask-table layer", tag);
  if (C::kMaskTab) {
    const int row_w = COUT / 16;
    CHECK(C::kMtT * kRows == C::kST && C::kMtT * C::kMtW == row_w && C::kMtRowW == row_w, "%s: mask table shares %d x %d", tag,
          C::kMtT, C::kMtW);
    std::vector<int> written(kRows * row_w, 0);
    for (int t = 0; t < C::kST; ++t) {
      const int row = t / C::kMtT, w0 = (t % C::kMtT) * C::kMtW;
      for (int c = 0; c <= C::NCH - 2; ++c)
        for (int j = 0; j < C::kMtPhase; ++j) {
          const int i = c * C::kMtPhase + j;
          if (i >= C::kMtW) continue;
          CHECK(row < kRows && w0 + i < row_w, "%s: thread %d writes word (%d, %d)", tag, t, row, w0 + i);
          if (row < kRows && w0 + i < row_w) ++written[row * row_w + w0 + i];
        }
    }
    for (int x = 0; x < kRows * row_w; ++x) CHECK(written[x] == 1, "%s: mask word (%d, %d) written %d times", tag, x / row_w, x % row_w, written[x]);
  }

  // ---- wave tiling
  {
    CHECK(C::NCTA == COUT / 16 && C::NWM == WM * WN, "%s: accumulator tiles", tag);
    std::vector<int> owned(C::NCTA * 4 * S, 0);
    for (int wave = 0; wave < C::NWM; ++wave) {
      const int wn = wave % WN, wm = (wave / WN) % WM, ct0 = wn * C::NCT, rt0 = wm * C::NRT;
      for (int ct = 0; ct < C::NCT; ++ct)
        for (int rt = 0; rt < C::NRT; ++rt) {
          CHECK(ct0 + ct < C::NCTA && rt0 + rt < 4 * S, "%s: wave %d tile (%d, %d)", tag, wave, ct0 + ct, rt0 + rt);
          if (ct0 + ct < C::NCTA && rt0 + rt < 4 * S) ++owned[(ct0 + ct) * 4 * S + rt0 + rt];
        }
    }
    for (int x = 0; x < C::NCTA * 4 * S; ++x) CHECK(owned[x] == 1, "%s: accumulator tile (%d, %d) owned %d times", tag, x / (4 * S), x % (4 * S), owned[x]);
    CHECK(C::RG >= 1 && C::NRT % C::RG == 0, "%s: row-tile groups of %d in %d", tag, C::RG, C::NRT);
    CHECK(C::NSTEP * 32 == CIN * KS, "%s: %d k-steps", tag, C::NSTEP);
    const int waves = WM * WN + (LW > 0 ? LW : 0);
    CHECK(C::NW == waves && C::kThreads == 64 * waves && C::kThreads <= 1024, "%s: %d threads", tag, C::kThreads);
    // waves per SIMD of the WPC workgroups that share a CU's 4 SIMDs: at least 2, or 1 when 4 waves have the CU
    const int per_simd = (waves * WPC + 3) / 4, want = waves * WPC <= 4 ? 1 : per_simd < 2 ? 2 : per_simd;
    const int got = x3::waves_per_eu<WM * WN + x3::loaders(LW), WPC>();
    CHECK(got == want && got <= 8, "%s: %d waves per SIMD, want %d", tag, got, want);
  }

  check_tile_walk<DENSE, S>(tag);
}

template <bool HAVE, int CIN, int COUT, int KS, int S, int WM, int WN, int LW, int CK, int WPC>
static int check_dense(int layer) {
  if constexpr (HAVE) {
    constexpr int lw = LW > 0 ? LW : -(WM * WN);  // the dense instantiation's staging rule
    static_assert(x3::dense_lw(LW, WM, WN) == lw, "dense staging rule");
    check_cfg<CIN, COUT, KS, S, WM, WN, false, lw, CK, WPC, false, true>(layer, "dense");
    return x3::Cfg<CIN, COUT, KS, S, WM, WN, false, lw, CK, WPC, false, true>::bytes;
  } else {
    (void)layer;
    return 0;
  }
}

// the per-layer record against the Cfg of the row's variants
template <int CIN, int COUT, int KS, int S, int WM, int WN, bool LAST, int LW, int LWB, int CK, int WPC, bool DENSE>
static void check_row(int layer) {
  check_cfg<CIN, COUT, KS, S, WM, WN, LAST, LW, CK, WPC, true, false>(layer, "prescale");
  check_cfg<CIN, COUT, KS, S, WM, WN, LAST, LWB, CK, WPC, false, false>(layer, "batch");
  const int dense_bytes = check_dense<DENSE && !LAST, CIN, COUT, KS, S, WM, WN, LWB, CK, WPC>(layer);
  const int ps_bytes = x3::Cfg<CIN, COUT, KS, S, WM, WN, LAST, LW, CK, WPC, true>::bytes;
  const int batch_bytes = x3::Cfg<CIN, COUT, KS, S, WM, WN, LAST, LWB, CK, WPC, false>::bytes;
  const x3::LayerInfo info = x3::layer_info(layer);
  CHECK(info.S == S && info.WPC == WPC && info.has_dense == (DENSE && !LAST), "layer %d: record", layer);
  CHECK(info.lds_ps == ps_bytes && info.lds_batch == batch_bytes && info.lds_dense == dense_bytes,
        "layer %d: record LDS %d %d %d", layer, info.lds_ps, info.lds_batch, info.lds_dense);
}

int main() {
#define APNEAUQ_X3_CHECK_ROW(L, CI, CO, K, S, WM, WN, LAST, LW, LWB, CK, WPC, DENSE) \
  check_row<CI, CO, K, S, WM, WN, LAST, LW, LWB, CK, WPC, DENSE>(L);
  APNEAUQ_X3_LAYERS(APNEAUQ_X3_CHECK_ROW)
#undef APNEAUQ_X3_CHECK_ROW
  const x3::LayerInfo none = x3::layer_info(0);
  CHECK(none.S == 0 && none.WPC == 1 && !none.has_dense, "layer 0 has a record");
  std::printf("%d configurations, %d failures\n", configs, failures);
  return failures ? 1 : 0;
}
