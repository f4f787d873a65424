// Host check of the training path's launch geometry (csrc/train_geo.h) against brute force.  Stand-alone:
// built and run by tests/test_train_geo_cpu.py with the host compiler.  Without arguments it sweeps every
// batch B in 1..4200 plus 8192 and 16384, M in {1, 2, 3, 4, 8} members and the six blocks, and checks what
// the kernels and the workspace rely on:
//   * wgrad: the row groups, walked as wgrad_kernel walks them (rt = ceil(tiles / rgs), group rg = tiles
//     [rg * rt, min(tiles, (rg + 1) * rt))), partition the row tiles: contiguous, none empty, none longer
//     than the cap in force; nci * nco * rgs is the grid; deterministic mode groups as M = 1; a member-
//     batched launch never has more row groups than the single one (each member's partial buffer is sized
//     for M = 1);
//   * partial buffer: wgrad_part_floats(B) is the maximum over n <= B of wg_main_floats(n) + wgrad<0>'s
//     region, non-decreasing in B, and wgrad<0>'s region of the fused step starts behind every wgrad<1..5> region;
//   * deterministic scratch: 16-byte aligned, behind every user's partial table (forward, head, dgrad),
//     no row wider than kDetMaxW, det_floats = base + the two-pass fp64 scratch;
//   * reduction: J a power of two <= 64 with rgs >= 8 J when J > 1, blocks <= 2048, and the walk of
//     wgrad_reduce_cols over (blocks, J) visits each of the s4 float4 columns exactly once;
//   * head: 4 * spw * grid >= B, spw in {1, 2, 4}, one sample per wave without the backward pass;
//   * dgrad: one workgroup per tile unless the block persists, 1 <= grid <= max(tiles, 1), grid * M <= kDgGrid
//     for the persistent blocks;
//   * forward: the persistent variant never in deterministic mode, with groups != 1 or with shared0, and
//     grid * ceil(tiles / grid) >= tiles for the contiguous tile ranges;
//   * the cases tests/test_train_kernels_gpu.py is built around, as literals.
// "--table B M det" prints that launch's geometry for all six blocks as one JSON object: the only way the
// Python tests learn these numbers.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string_view>
#include <tuple>
#include <vector>

#include "train_geo.h"

using namespace apneauq;
using namespace apneauq::train;

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

static const int kMs[] = {1, 2, 3, 4, 8};

// the (blocks, J) walk of wgrad_reduce_cols over s4 float4 columns: each column exactly once
static void check_reduce_walk(int l, int s4, int J, int blocks) {
  static std::set<std::tuple<int, int, int>> done;
  if (!done.insert({s4, J, blocks}).second) return;
  std::vector<int> seen(s4, 0);
  const int ncol = 256 / J;
  for (int bx = 0; bx < blocks; ++bx)
    for (int base = bx * ncol; base < s4; base += blocks * ncol)
      for (int cl = 0; cl < ncol; ++cl)
        if (base + cl < s4) ++seen[base + cl];
  for (int e = 0; e < s4; ++e) CHECK(seen[e] == 1, "block %d J %d blocks %d: column %d summed %d times", l, J, blocks, e, seen[e]);
}

static void check_wgrad(int l, int B, int M, bool det) {
  const WgShape s = wg_shape(l, B, M, det);
  const int tiles = tiles_of(B);
  CHECK(s.nci * s.cib == (l == 0 ? s.cib : arch::C[l]) && s.nco * s.cob == arch::C[l + 1], "block %d: blocks tile Cin x Cout", l);
  CHECK(s.grid == s.nci * s.nco * s.rgs && s.rgs >= 1, "block %d B %d M %d: grid %d", l, B, M, s.grid);
  // the cap in force, stated here and not read from the header: the table's row tiles up to 1024 tiles per
  // launch (all members; one in deterministic mode), at least 64 beyond
  const int want_cap = tiles * (det ? 1 : M) > 1024 ? std::max(s.rtiles, 64) : s.rtiles;
  CHECK(s.cap == want_cap, "block %d B %d M %d: cap %d, not %d", l, B, M, s.cap, want_cap);
  // the kernel's walk
  const int rt = (tiles + s.rgs - 1) / s.rgs;
  CHECK(rt == s.rt, "block %d B %d M %d: rt %d != %d", l, B, M, s.rt, rt);
  int next = 0;
  for (int rg = 0; rg < s.rgs; ++rg) {
    const int tile0 = rg * rt, nt = std::min(rt, tiles - tile0);
    CHECK(tile0 == next && nt >= 1 && nt <= s.cap, "block %d B %d M %d: group %d = tiles [%d, +%d), cap %d", l, B, M, rg, tile0, nt, s.cap);
    next = tile0 + std::max(nt, 0);
  }
  CHECK(next == tiles, "block %d B %d M %d: groups end at tile %d of %d", l, B, M, next, tiles);
  const WgShape one = wg_shape(l, B, 1, false);
  if (det) CHECK(s.rgs == one.rgs && s.rt == one.rt && s.J == one.J, "block %d B %d M %d: deterministic grouping", l, B, M);
  CHECK(s.rgs <= one.rgs, "block %d B %d M %d: %d row groups, %d slots per member", l, B, M, s.rgs, one.rgs);
  // reduction
  CHECK(s.s4 * 4 == s.kcc + s.cout && s.cout % 4 == 0 && s.kcc == arch::KS[l] * arch::C[l] * arch::C[l + 1], "block %d: s4", l);
  CHECK(s.J >= 1 && s.J <= 64 && (s.J & (s.J - 1)) == 0, "block %d B %d M %d: J %d", l, B, M, s.J);
  CHECK(s.J == 1 || s.rgs >= 8 * s.J, "block %d B %d M %d: J %d for %d row groups", l, B, M, s.J, s.rgs);
  CHECK(s.blocks >= 1 && s.blocks <= 2048, "block %d B %d M %d: %d reduce blocks", l, B, M, s.blocks);
  check_reduce_walk(l, s.s4, s.J, s.blocks);
}

// floats the fused step's partial layout needs at batch n: wgrad<1..5> at 0, wgrad<0> behind them
static long long fused_need(int n) {
  // what each launch writes, from its own shape: slot rg < rgs of K * Cin * Cout + Cout floats, wgrad<1..5>
  // from offset 0, wgrad<0> from wg_main_floats(n)
  const long long part[6] = {wg_part_floats<0>(n), wg_part_floats<1>(n), wg_part_floats<2>(n), wg_part_floats<3>(n),
                             wg_part_floats<4>(n), wg_part_floats<5>(n)};
  const long long main = wg_main_floats(n);
  long long end0 = 0;
  for (int l = 0; l < 6; ++l) {
    const WgShape s = wg_shape(l, n, 1, false);
    const long long written = (long long)s.rgs * (arch::KS[l] * arch::C[l] * arch::C[l + 1] + arch::C[l + 1]);
    CHECK(written == part[l], "B %d block %d: writes %lld floats, wg_part_floats %lld", n, l, written, part[l]);
    if (l == 0)
      end0 = main + written;
    else
      CHECK(main >= written, "B %d: wgrad<0> region at %lld, wgrad<%d> ends at %lld", n, main, l, written);
  }
  return end0;
}

static void check_det(int B) {
  const long long base = det_scratch_base(B);
  const int tiles = tiles_of(B);
  CHECK(base % 4 == 0, "B %d: scratch base %lld", B, base);
  CHECK(det_floats(B) == base + 2LL * kDetSeg * kDetMaxW, "B %d: det floats", B);
  for (int l = 0; l < 6; ++l) {
    const DetRows f = det_rows_fwd(B, l);
    CHECK(f.n == fwd_grid(B) && f.w == 2 * arch::C[l + 1] && f.w <= kDetMaxW && (long long)f.n * f.w <= base, "B %d fwd %d: %d x %d", B, l, f.n, f.w);
    if (l == 0) continue;
    const DetRows d = det_rows_dgrad(B, l);
    // dgrad_kernel<l> writes row tile * WM + wm, wm < WM = the wave row blocks of its Tiling<C[l]>
    const int wm = for_block(l, [](auto L) { return Tiling<arch::C[decltype(L)::value ? decltype(L)::value : 1]>::WM; });
    CHECK(d.n == tiles * wm && d.w == 2 * arch::C[l] && d.w <= kDetMaxW && (long long)d.n * d.w <= base, "B %d dgrad %d: %d x %d", B, l, d.n, d.w);
  }
  const DetRows h = det_rows_head(B);
  CHECK(h.n == B && h.w == kHeadRec && h.w <= kDetMaxW && (long long)h.n * h.w <= base, "B %d head: %d x %d", B, h.n, h.w);
}

static void check_launches(int B, int M) {
  const int tiles = tiles_of(B);
  for (int bw = 0; bw < 2; ++bw) {
    const int spw = head_spw(B, M, bw), grid = head_grid(B, M, bw);
    CHECK((spw == 1 || spw == 2 || spw == 4) && (bw || spw == 1), "B %d M %d: spw %d", B, M, spw);
    CHECK((long long)grid * 4 * spw >= B && (long long)(grid - 1) * 4 * spw < B, "B %d M %d: head grid %d x spw %d", B, M, grid, spw);
  }
  for (int l = 1; l < 6; ++l) {
    const int g = dg_grid(B, M, l);
    CHECK(g >= 1 && g <= std::max(tiles, 1), "B %d M %d dgrad %d: grid %d", B, M, l, g);
    if (dg_persist(l))
      CHECK(M > kDgGrid || g * M <= kDgGrid, "B %d M %d dgrad %d: grid %d persists", B, M, l, g);
    else  // one trip per workgroup
      CHECK(g == tiles, "B %d M %d dgrad %d: grid %d for %d tiles", B, M, l, g, tiles);
  }
  for (int l = 0; l < 6; ++l)
    for (int flags = 0; flags < 8; ++flags) {
      const bool det = flags & 1, shared0 = flags & 2;
      const int groups = (flags & 4) ? 2 : 1;
      const bool pf = fwd_pf(B, M, l, det, groups, shared0);
      CHECK(!pf || (!det && groups == 1 && !shared0 && FwdPF<1>::v > 0 && (l == 1 || l == 3)), "B %d M %d fwd %d flags %d: persistent", B, M, l, flags);
      CHECK(!pf || (long long)tiles * M > kFwdTrainGrid, "B %d M %d fwd %d: persistent on %d tiles", B, M, l, tiles);
      const int g = fwd_launch_grid(B, M, pf);
      const int tpw = (tiles + g - 1) / g;  // fwd_kernel's contiguous tile range per workgroup
      CHECK(g >= 1 && (long long)g * tpw >= tiles && (pf || g == fwd_grid(B)), "B %d M %d fwd %d: grid %d", B, M, l, g);
      CHECK(!det || g == det_rows_fwd(B, l).n, "B %d M %d fwd %d: deterministic grid %d", B, M, l, g);
    }
}

static int sweep() {
  int cases = 0;
  std::vector<int> Bs;
  for (int B = 1; B <= 4200; ++B) Bs.push_back(B);
  Bs.push_back(8192);
  Bs.push_back(16384);
  long long run_max = 0, prev = 0;
  int n_done = 0;  // fused_need folded into run_max for every n <= n_done
  for (int B : Bs) {
    for (; n_done < B; ++n_done) run_max = std::max(run_max, fused_need(n_done + 1));
    const long long have = wgrad_part_floats(B);
    CHECK(have == run_max, "B %d: %lld partial floats, the batches up to it need %lld", B, have, run_max);
    CHECK(have >= prev, "B %d: partial floats shrink, %lld after %lld", B, have, prev);
    prev = have;
    check_det(B);
    ++cases;
    for (int M : kMs) {
      check_launches(B, M);
      ++cases;
      for (int l = 0; l < 6; ++l)
        for (int det = 0; det < 2; ++det) {
          check_wgrad(l, B, M, det);
          // a non-fused launch writes its slots from offset 0 of the member's buffer
          CHECK((long long)wg_shape(l, B, M, det).rgs * (arch::KS[l] * arch::C[l] * arch::C[l + 1] + arch::C[l + 1]) <= have,
                "B %d M %d block %d: partial slots past the buffer", B, M, l);
          ++cases;
        }
    }
  }
  // the cases the GPU tests are built around
  CHECK(kFwdTrainGrid == 512 && kDgGrid == 512, "thresholds");
  CHECK(tiles_of(1026) == 513 && fwd_pf(1026, 1, 1, false, 1, false) && fwd_pf(1026, 1, 3, false, 1, false) &&
            fwd_launch_grid(1026, 1, true) == 512 && !fwd_pf(1024, 1, 1, false, 1, false) && fwd_launch_grid(1024, 1, false) == 512,
        "513 forward tiles on a 512 grid at 1026");
  CHECK(dg_grid(1026, 1, 1) == 512 && dg_grid(1024, 1, 1) == 512 && dg_grid(1026, 1, 3) == 513, "513 dgrad tiles on a 512 grid at 1026");
  CHECK(head_spw(2048, 1, 1) == 1 && head_spw(2051, 1, 1) == 2 && head_spw(4099, 1, 1) == 4 && 2051 % 8 && 4099 % 16, "head spw at 2051 / 4099");
#ifndef APNEAUQ_WG_TABLE  // the default table's boundaries
  CHECK(wg_shape(4, 2050, 1, false).rt > wg_shape(4, 2050, 1, false).rtiles && wg_shape(4, 2048, 1, false).rtiles >= wg_shape(4, 2048, 1, false).rt, "row-tile cap of block 5 between 2048 and 2050");
  CHECK(wg_shape(0, 37, 1, false).J > 1 && wg_shape(0, 37, 1, false).rgs % wg_shape(0, 37, 1, false).J != 0, "wgrad<0> at 37: rgs %% J");
#endif
  cases += 4;
  return cases;
}

static int table(int B, int M, bool det) {
  std::printf("{\"B\": %d, \"M\": %d, \"det\": %s, \"tiles\": %d, \"fwd_train_grid\": %d, \"dg_grid\": %d,\n", B, M, det ? "true" : "false",
              tiles_of(B), kFwdTrainGrid, kDgGrid);
  std::printf(" \"head\": {\"spw\": %d, \"grid\": %d, \"spw_fwd\": %d},\n", head_spw(B, M, 1), head_grid(B, M, 1), head_spw(B, M, 0));
  std::printf(" \"wpart_floats\": %lld, \"wg_main_floats\": %lld, \"det_floats\": %d, \"det_scratch_base\": %lld,\n", wgrad_part_floats(B),
              wg_main_floats(B), det_floats(B), det_scratch_base(B));
  std::printf(" \"lds\": {\"fwd\": %d, \"head\": %d, \"dgrad\": %d},\n \"blocks\": [\n", lds_fwd(), lds_head(), lds_dgrad());
  for (int l = 0; l < 6; ++l) {
    const bool pf = fwd_pf(B, M, l, det, 1, false);
    const WgShape s = wg_shape(l, B, M, det);
    std::printf("  {\"fwd\": {\"pf\": %s, \"grid\": %d}, \"dgrad\": {\"persist\": %s, \"grid\": %d},\n", pf ? "true" : "false",
                fwd_launch_grid(B, M, pf), dg_persist(l) ? "true" : "false", l ? dg_grid(B, M, l) : 0);
    std::printf("   \"wgrad\": {\"cib\": %d, \"cob\": %d, \"rtiles\": %d, \"minwg\": %d, \"nci\": %d, \"nco\": %d, \"cap\": %d, \"rgs\": %d, "
                "\"rt\": %d, \"grid\": %d, \"threads\": %d, \"lds\": %d, \"s4\": %d, \"J\": %d, \"blocks\": %d}}%s\n",
                s.cib, s.cob, s.rtiles, s.minwg, s.nci, s.nco, s.cap, s.rgs, s.rt, s.grid, s.threads, s.lds, s.s4, s.J, s.blocks,
                l < 5 ? "," : "");
  }
  std::printf(" ]}\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 5 && std::string_view(argv[1]) == "--table") return table(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]) != 0);
  if (argc != 1) {
    std::printf("usage: %s [--table B M det]\n", argv[0]);
    return 2;
  }
  const int cases = sweep();
  std::printf("%d cases, %d failures\n", cases, failures);
  return failures ? 1 : 0;
}
