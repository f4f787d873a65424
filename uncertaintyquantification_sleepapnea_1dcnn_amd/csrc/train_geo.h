// Launch geometry of the layer-wise training path (train_launch.hip and the train_*.hip kernel files): how a
// batch of B samples and M ensemble members becomes grids, row groups, partial slots, LDS and scratch
// sizes.  Stated once: the kernels take their compile-time tables from here, the launch code reads every
// number from here, and the tests learn them by running tests/train_geo_check.cpp, which also checks this
// header against brute force on the host.  Plain constexpr / inline C++17: no HIP header, no Args.
#pragma once
#include <algorithm>
#include <type_traits>

#include "arch_tables.h"

namespace apneauq {
namespace train {

// padded-row layout (see train_launch.hip): kL time steps in a kSR-row slot, kSlots samples = kR rows per tile,
// kRows staged rows with the conv halo
constexpr int kL = 60, kSR = 64, kSlots = 2, kR = 128, kRT = 8, kHalo = 4, kRows = 136;
constexpr int kRS = 256 * 2 + 32;  // LDS row stride (bytes) of the staged activation tiles
constexpr int kThreads = 256;
constexpr int kHeadRec = 2 + 3 * 96;  // deterministic head record per sample: loss, dlogit, dW, sum dY, sum dY xhat
// deterministic column sums: kDetSeg row segments (pass 1, fp64 scratch [kDetSeg][w] behind the partial
// table), then the segments in order (pass 2); w <= kDetMaxW
constexpr int kDetSeg = 32, kDetMaxW = 512;

constexpr int tiles_of(int B) { return (B + 1) / 2; }  // 2-sample row tiles of a batch

// f(std::integral_constant<int, l>) for a runtime block index l (0..5; anything else runs block 5's)
template <class F>
inline auto for_block(int l, F&& f) {
  switch (l) {
    case 0: return f(std::integral_constant<int, 0>{});
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    case 4: return f(std::integral_constant<int, 4>{});
    default: return f(std::integral_constant<int, 5>{});
  }
}

// ------------------------------------------------------------------------------------------------ forward
// Forward input staging of block l in two row batches instead of all of a tile's row loads in flight
// at once (ActStager): blocks 3 and 6 spilled 22 / 44 VGPRs with one batch; split, neither spills and
// the batch-BN MC-Dropout chunk is ~2 % faster (profiles/batch_bn_fwd_r2.md, session 3).
template <int l> struct FwdStageSplit { static constexpr bool v = l == 2 || l == 5; };
// Large training launches (more row tiles than kFwdTrainGrid workgroups: batch >= 2048, or the
// member-batched step) run the PF instantiation of the forward: kFwdTrainGrid persistent workgroups over
// contiguous tile ranges, the first FwdPF<l>::v input-row loads per thread of the NEXT tile issued before
// this tile's conv (registers each block leaves: 8 of 8 on block 2, 14 of 14 on block 4).  Batch 1024 (one
// tile per workgroup anyway) keeps the plain instantiation: the PF one measured +1 % there.
template <int l> struct FwdPF { static constexpr int v = l == 1 ? 8 : l == 3 ? 14 : 0; };
constexpr int kFwdTrainGrid = 512;

// wave tilings (WM, WN) per output-channel count
template <int COUT> struct Tiling;
template <> struct Tiling<128> { static constexpr int WM = 1, WN = 4; };
template <> struct Tiling<192> { static constexpr int WM = 1, WN = 4; };
template <> struct Tiling<224> { static constexpr int WM = 2, WN = 2; };
template <> struct Tiling<96> { static constexpr int WM = 2, WN = 2; };
template <> struct Tiling<256> { static constexpr int WM = 1, WN = 4; };

// Persistent forward: workgroups per CU (2 are resident at a time), each over a contiguous tile range.
// Batch-BN MC Dropout (409,600 tiles per layer launch) measured 8 / 16 / 32 / 64 per CU: MCD phase
// 91.9 / 91.1-91.4 / 91.0-91.4 / 90.5-90.9 ms (tools/probes/so_bench1.sh, one box), and 64 / 128 / 256
// on another: 90.8-90.9 / 91.2-91.8 / 91.9-92.1 ms: shorter ranges
// balance the launch tail.  Batches of <= 16384 tiles (training) get one tile per workgroup anyway.
constexpr int kFwdWgPerCu = 64;
inline int fwd_grid(int B) { return std::min(tiles_of(B), 256 * kFwdWgPerCu); }
// the PF forward (FwdPF) for a training launch of M members x B samples: persistent workgroups, only
// when the tiles outnumber kFwdTrainGrid (never in deterministic mode: its moment partials are per
// workgroup of the fwd_grid layout, which the member-batched step must share with the single one)
inline bool fwd_pf(int B, int M, int l, bool det, int groups, bool shared0) {
  const bool has = (l == 1 && FwdPF<1>::v > 0) || (l == 3 && FwdPF<3>::v > 0);
  return has && !det && groups == 1 && !shared0 && (long long)tiles_of(B) * M > kFwdTrainGrid;
}
// workgroups per member of a forward launch: the persistent variant shares kFwdTrainGrid among the members
inline int fwd_launch_grid(int B, int M, bool pf) { return pf ? std::max(1, kFwdTrainGrid / M) : fwd_grid(B); }

// ------------------------------------------------------------------------------------------------ head
// training head samples per wave: 1 while that leaves <= 512 workgroups, else up to 4 (batch 8192:
// 512 workgroups instead of 2048, a quarter of the per-workgroup global sums onto the same 16 slots);
// the forward-only head (MC Dropout, no sums) keeps one sample per wave
inline int head_spw(int B, int M, int backward) {
  int spw = 1;
  while (backward && spw < 4 && (long long)B * M > 512LL * 4 * spw) spw *= 2;
  return spw;
}
// workgroups per member (4 waves of spw samples each), without the table's extra workgroups
inline int head_grid(int B, int M, int backward) {
  const int spw = head_spw(B, M, backward);
  return (B + 4 * spw - 1) / (4 * spw);
}

// ------------------------------------------------------------------------------------------------ dgrad
// dgrad: prefetch the epilogue's R_{l-1} loads ahead of the conv (every block; block 6 has had the
// registers for it since its staging became DzStager: dgrad<5> b8192 -0.6 %, 8 members -0.5..-1.9 %)
template <int l> struct DgPre { static constexpr bool v = l >= 1 && l <= 5; };
// Persistent dgrad: a workgroup runs row tiles tile, tile + grid, ...; the first DgPF<l>::v staging items
// per thread of the NEXT tile (R_l and dY_l rows, 8 channels each) are loaded into registers before this
// tile's conv, so their latency hides under the MFMAs (the rest load at staging time, as before).
// Sized to the registers each block leaves with DgPre (tools/kernel_resources.py: no spills); trading
// DgPre for a deeper staging prefetch measured slower (profiles/train_step_r5.md).
template <int l> struct DgPF { static constexpr int v = l == 1 ? 8 : l == 2 ? 2 : l == 4 ? 12 : 0; };
// workgroups of a single-model dgrad launch: two per CU (larger batches loop over their tiles)
constexpr int kDgGrid = 512;
// Weight-fragment prefetch depth of the dgrad conv (k-steps in flight): 2 where it fits the 256-VGPR budget
// without spilling (blocks 3 / 6 spill at 2: 56 / 12 B of scratch)
template <int l> struct DgPD { static constexpr int v = (l == 1 || l == 2 || l == 4) ? 2 : 1; };

// persistent blocks (DgPF > 0): at most kDgGrid workgroups over all members, each looping over its
// member's tiles; the others one workgroup per tile
inline bool dg_persist(int l) {
  return (l == 1 && DgPF<1>::v > 0) || (l == 2 && DgPF<2>::v > 0) || (l == 3 && DgPF<3>::v > 0) ||
         (l == 4 && DgPF<4>::v > 0) || (l == 5 && DgPF<5>::v > 0);
}
inline int dg_grid(int B, int M, int l) {
  const int tiles = tiles_of(B);
  return dg_persist(l) ? std::max(1, std::min(tiles, kDgGrid / std::max(1, M))) : tiles;
}

// ------------------------------------------------------------------------------------------------ wgrad
template <int l> struct WgCfg;
// CI_BLK CO_BLK WCO WCI, RTILES = 128-row tiles summed in registers per workgroup (sized so a
// batch of 1024 gives >= 256 workgroups without multiplying the output atomics needlessly)
// MINWG: the launcher lowers the row tiles per workgroup until at least this many workgroups
// exist (measured at batch 1024: blocks 2-3 prefer fewer, longer workgroups, blocks 4-6 more)
// U: dZ staging loads in flight per thread; MINB: workgroups per CU the register budget targets
// (batch-8192 probes, tools/probes/so_variants.sh: U 4 -> 8 saves 10-13 % on blocks 2, 3, 5; three
// workgroups per CU save 17 % on block 4 and spill on block 6)
// wgrad LDS tiles: the row stride is an odd multiple of 32 B (conflict-free tr_frag reads)
constexpr int wg_rs(int width_bytes) { return (width_bytes / 32) % 2 ? width_bytes : width_bytes + 32; }
// MINWG values: batch-1024 step measured with tools/probes/train_variants.sh (block 5 512 -> 768 took
// the step 0.795 -> 0.786 ms, block 2 256 -> 512 0.766-0.775 -> 0.758-0.768 ms, three interleaved rounds;
// round 4, with the straggler-free grouping: block 3 256 -> 512 batch 8192 4.20-4.22 -> 4.13-4.16 ms,
// batch 1024 / 8 members unchanged; block 4 512 -> 1024 slower)
#ifdef APNEAUQ_WG_TABLE  // A/B builds swap the complete table (tools/probes/wg_tables/)
#include APNEAUQ_WG_TABLE
#else
// WAVES: 4 (two workgroups per CU) or 8 (one per CU: the output block over twice the waves, so each
// wave holds half the accumulators and the next row tile's dZ / A rows fit in registers); PF / PFA: those
// rows (dZ / A) are loaded into registers during this tile's MFMAs and written to LDS after them.
// Blocks 2, 3, 5, 6 at 8 waves with both prefetches (tools/probes/wg_tables/w8a.h, profiles/train_step_r5.md):
// batch 1024 0.725 -> 0.687 ms, batch 8192 4.12 -> 3.94 ms, 8 members 4.21 -> 4.07 ms (two rounds each);
// block 4 keeps 4 waves (no 8-way split of its 224 x 96 block), block 1 its im2col.
template <> struct WgCfg<0> { static constexpr int CIB = 32, COB = 128, WCO = 4, WCI = 1, RTILES = 2, MINWG = 512, U = 4, MINB = 2, WAVES = 4; static constexpr bool PF = false, PFA = false; };  // im2col kk=32
template <> struct WgCfg<1> { static constexpr int CIB = 32, COB = 192, WCO = 4, WCI = 2, RTILES = 8, MINWG = 256, U = 8, MINB = 1, WAVES = 8; static constexpr bool PF = true, PFA = true; };
template <> struct WgCfg<2> { static constexpr int CIB = 64, COB = 224, WCO = 2, WCI = 4, RTILES = 8, MINWG = 256, U = 8, MINB = 1, WAVES = 8; static constexpr bool PF = true, PFA = true; };
template <> struct WgCfg<3> { static constexpr int CIB = 32, COB = 96, WCO = 2, WCI = 2, RTILES = 16, MINWG = 512, U = 8, MINB = 2, WAVES = 4; static constexpr bool PF = true, PFA = true; };
template <> struct WgCfg<4> { static constexpr int CIB = 32, COB = 128, WCO = 4, WCI = 2, RTILES = 16, MINWG = 256, U = 8, MINB = 1, WAVES = 8; static constexpr bool PF = true, PFA = true; };
template <> struct WgCfg<5> { static constexpr int CIB = 64, COB = 96, WCO = 2, WCI = 4, RTILES = 16, MINWG = 256, U = 4, MINB = 1, WAVES = 8; static constexpr bool PF = true, PFA = true; };
#endif

// ci x co blocks of wgrad<l>'s output (block 1: one im2col block)
template <int l> constexpr int wg_nci() { return (l == 0) ? 1 : arch::C[l] / WgCfg<l>::CIB; }
template <int l> constexpr int wg_nco() { return arch::C[l + 1] / WgCfg<l>::COB; }
// floats of one row group's partial slot: dW (k, Cin, Cout), then db
template <int l> constexpr int wg_kcc() { return arch::KS[l] * arch::C[l] * arch::C[l + 1]; }
template <int l> constexpr int wg_slot_floats() { return wg_kcc<l>() + arch::C[l + 1]; }
// most row tiles a workgroup may sum: RTILES up to 2048 samples per launch; beyond, up to 64
template <int l>
inline int wg_cap(int B, int M = 1) {
  return tiles_of(B) * M > 1024 ? std::max(WgCfg<l>::RTILES, 64) : WgCfg<l>::RTILES;
}
// row groups of wgrad<l> for M members of B samples (a deterministic launch passes M = 1: wg_members)
template <int l>
inline int wg_rgs(int B, int M = 1) {
  using W = WgCfg<l>;
  const int nci = wg_nci<l>();
  const int nco = wg_nco<l>();
  const int tiles = tiles_of(B);
  // ~MINWG workgroups (over all M members of a member-batched launch) while tiles remain, at most RTILES
  // row tiles each up to 2048 samples per launch; beyond, up to 64: fewer row groups, so fewer partial
  // slots to write and reduce (batch 8192: step 4.74 -> 4.52 ms; the small-batch caps were tuned at
  // batch 1024, where block 3 prefers more, shorter workgroups)
  const int nblk = nci * nco;
  const int cap = wg_cap<l>(B, M);
  int rt = std::max(1, std::min(cap, (tiles * M * nblk + W::MINWG - 1) / W::MINWG));
  // no straggler round: rounding the row groups up could leave a few workgroups past MINWG (one
  // CU-slot's worth), which then run as a second round of their own -- block 4 at batch 1024 / 8192:
  // 518 workgroups on 512 slots, 244 us at batch 8192 vs 178 us with 448
  while (rt < cap && (long long)M * nblk * ((tiles + rt - 1) / rt) > W::MINWG) ++rt;
  return (tiles + rt - 1) / rt;
}
// deterministic mode: the single-model row grouping (M = 1), so a member-batched step sums every
// gradient in the same order as the member's own step
inline int wg_members(int M, bool det) { return det ? 1 : M; }

template <int l>
inline long long wg_part_floats(int B) {
  return (long long)wg_rgs<l>(B) * wg_slot_floats<l>();
}
// floats of the partial region wgrad<1..5> share, and of wgrad<0>'s own region behind it (fused step)
inline long long wg_main_floats(int B) {
  return std::max({wg_part_floats<1>(B), wg_part_floats<2>(B), wg_part_floats<3>(B), wg_part_floats<4>(B),
                   wg_part_floats<5>(B)});
}
// Partial floats a workspace of batch capacity B needs: the shared region plus wgrad<0>'s region of the
// fused step, for EVERY batch n <= B (a partial last batch runs the row grouping of its own size, which
// is not monotone in n: the row-tile cap changes at 2048 samples)
inline long long wgrad_part_floats(int B) {
  long long mx = 0;
  for (int n = 2; n < B + 2; n += 2) {  // the grouping depends on the tile count (n + 1) / 2 only
    const int b = std::min(n, B);
    mx = std::max(mx, wg_main_floats(b) + wg_part_floats<0>(b));
  }
  return mx;
}

// One wgrad<l> launch (M = the members of the launch; det: deterministic mode) and the reduction of its
// partials.  rt = the row tiles per group the kernel walks, ceil(tiles / rgs).
struct WgShape {
  int cib, cob, rtiles, minwg;  // WgCfg<l>
  int nci, nco, cap, rgs, rt;
  int grid, threads, lds;       // per member
  // reduction (wgrad_reduce_cols): J threads per float4 column, s4 columns, blocks = the reduce launch's grid
  int kcc, cout, s4, J, blocks;
};

// ------------------------------------------------------------------------------------------------ LDS
constexpr int lds_fwd() { return kRows * kRS + (1024 + 2 * 256) * 4; }  // tile + affine + lstat
constexpr int lds_head() { return (8 * arch::C[6] + 2) * 4; }
constexpr int lds_dgrad() { return kRows * kRS + 1792 * 4; }
static_assert(2 * lds_dgrad() <= 160 * 1024, "dgrad must fit two workgroups per CU");
template <int l>
constexpr int lds_wgrad() {
  return kR * wg_rs(WgCfg<l>::COB * 2) + kRows * wg_rs(l == 0 ? 64 : WgCfg<l>::CIB * 2) + 1792 * 4;
}
template <int l>
constexpr bool wg_lds_fits() {
  return WgCfg<l>::WAVES == 8 ? lds_wgrad<l>() <= 160 * 1024 : 2 * lds_wgrad<l>() <= 160 * 1024;
}
static_assert(wg_lds_fits<0>() && wg_lds_fits<1>() && wg_lds_fits<2>() && wg_lds_fits<3>() && wg_lds_fits<4>() &&
                  wg_lds_fits<5>(),
              "wgrad tiles must fit two 4-wave (or one 8-wave) workgroups per CU");

template <int l>
inline WgShape wg_shape(int B, int M, bool det) {
  using W = WgCfg<l>;
  WgShape s = {};
  s.cib = W::CIB, s.cob = W::COB, s.rtiles = W::RTILES, s.minwg = W::MINWG;
  s.nci = wg_nci<l>(), s.nco = wg_nco<l>();
  s.cap = wg_cap<l>(B, wg_members(M, det));
  s.rgs = wg_rgs<l>(B, wg_members(M, det));
  s.rt = (tiles_of(B) + s.rgs - 1) / s.rgs;
  s.grid = s.nci * s.nco * s.rgs, s.threads = W::WAVES * 64, s.lds = lds_wgrad<l>();
  s.kcc = wg_kcc<l>(), s.cout = arch::C[l + 1];
  s.s4 = wg_slot_floats<l>() / 4;
  // threads per column: enough columns x row-group splits to fill ~1024 workgroups' worth of lanes, at
  // least 8 row groups per thread (one batch of 8 loads in flight).  Block 1 (928 float4 columns, 512
  // row groups at batch 1024): J 16 -> 64, 58 -> 232 workgroups, one load batch per thread instead of 4
  int J = 1;
  while (J < 64 && s.rgs >= 8 * (2 * J) && (long long)s.s4 * J < 256LL * 1024) J *= 2;
  s.J = J;
  s.blocks = std::min(2048, (s.s4 * J + 255) / 256);
  return s;
}
inline WgShape wg_shape(int l, int B, int M, bool det) {
  return for_block(l, [&](auto L) { return wg_shape<decltype(L)::value>(B, M, det); });
}

// ------------------------------------------------------------------------------------------------ deterministic mode
// The partial table one deterministic reduction sums: n rows of w floats (Args::det).
struct DetRows {
  int n, w;
};
inline DetRows det_rows_fwd(int B, int l) { return {fwd_grid(B), 2 * arch::C[l + 1]}; }  // per workgroup: sum r, sum r^2
inline DetRows det_rows_head(int B) { return {B, kHeadRec}; }                            // per sample
// block l's backward sums (of BN l-1's output) per (tile, wave row block); l = 1..5
inline DetRows det_rows_dgrad(int B, int l) {
  constexpr int wm[6] = {0, Tiling<arch::C[1]>::WM, Tiling<arch::C[2]>::WM, Tiling<arch::C[3]>::WM,
                         Tiling<arch::C[4]>::WM, Tiling<arch::C[5]>::WM};
  return {tiles_of(B) * wm[l], 2 * arch::C[l]};
}
// floats of the partial table (fwd / head / dgrad reuse it), then the fp64 scratch of the two-pass reduce
inline long long det_scratch_base(int B) {
  const int tiles = tiles_of(B);
  const long long t = std::max({(long long)fwd_grid(B) * 2 * 256, (long long)B * kHeadRec,
                                (long long)tiles * 2 * 2 * 256});
  return (t + 3) / 4 * 4;  // 16-B aligned scratch
}
inline int det_floats(int B) { return (int)(det_scratch_base(B) + 2LL * kDetSeg * kDetMaxW); }

}  // namespace train
}  // namespace apneauq
