// Geometry of the x3 layer kernel (x3_layers.hip layer_kernel), stated once: the constants derived from a
// layer's template parameters, the LDS carve, the layer table, the tile walk and the staging-unit map.  Plain
// constexpr C++ of ints and bools (no HIP types): the kernel takes its constants and LDS pointers from here,
// the launch code its LDS size, the bindings the tile counts, and tests/x3_geo_check.cpp checks all of it
// against brute force with the host compiler (tests/test_x3_geo_cpu.py), for the committed table and for every
// A/B table under tools/probes/x3_tables/.
//
// A persistent workgroup (WM x WN MFMA waves + loader waves) walks a contiguous range of tiles.  A tile is S
// samples of one group (MC-Dropout pass or ensemble member) = 64 S GEMM rows: every sample a 64-row slot
// (60 time steps + 4 zero rows, the 'same' padding halo), or, with DENSE, 64 S consecutive rows of the
// group's dense row space (x3_dense_map.h: no GEMM row is a halo row).  The input channels stream through
// two LDS chunk buffers, CK at a time.
#pragma once

#include "x3_dense_map.h"

#ifndef __host__
#define APNEAUQ_X3_GEO_PLAIN 1
#define __host__
#define __device__
#endif

namespace apneauq {
namespace x3 {

// Staging waves of a layer without loader waves: the HBM loads of the next chunk are issued by MFMA
// waves 0..kStagers-1 only (one per SIMD), so that the partner wave keeps the matrix pipe busy while the
// stager's in-order vmcnt holds it at its next weight-fragment wait.
constexpr int kStagers = 4;
constexpr int kL = 60, kSR = 64, kHalo = 4;
// A chunk = CK input channels (32 or 64) of the tile's rows; LDS row: hi 2CK B | lo 2CK B | pad 32 B
// (row stride 2 mod 4 16-B slots for either CK: the ds_read_b128 lane groups of a 16x16x32 B fragment hit 16
// distinct slots at any row offset).  Layers with few taps take 64-channel chunks: twice the k-steps per
// chunk barrier.
__host__ __device__ constexpr int row_bytes(int ck) { return 4 * ck + 32; }
// per tile of S samples (S x 64 GEMM rows): LDS rows and chunk-buffer bytes of the slot mapping
__host__ __device__ constexpr int lds_rows(int S) { return kHalo + S * kSR + kHalo; }
__host__ __device__ constexpr int buf_bytes(int S, int ck) { return lds_rows(S) * row_bytes(ck); }
// rows of a dense tile's descriptor table: the tile's rows + PAD either side
__host__ __device__ constexpr int tab_rows(int S, int ks) { return kSR * S + (ks - 1); }
// output keep-bits of a tile: [64 S rows][cout / 16] 16-bit words, bit c % 16 of word c / 16 = keep (row, c)
__host__ __device__ constexpr int mask_tab_bytes(int S, int cout) { return kSR * S * (cout / 16) * 2; }
// The layers whose loader waves draw the output mask into that table: a dense-row kernel with loader waves
// where it measured faster, which is block 5 (96 -> 256, k 9: +1 %).  Block 3 (192 -> 224, k 3: 18 k-steps per
// tile and the most VALU per MFMA of all layers) lost 0.5 - 2.4 % with the same draw on its loader waves, and
// block 4's mask stays with its consumer (profiles/x3_epilogue_offload.md); the kernel is written for any.
__host__ __device__ constexpr bool mask_tab_layer(int cin, int cout, int ks, int lw, bool dense_rows) {
  return dense_rows && lw > 0 && cin == 96 && cout == 256 && ks == 9;
}

// Waves: WM x WN MFMA waves, plus LW loader waves (LW > 0) that do all the input staging: HBM loads of
// chunk c+2, BN affine + dropout + fp16 split of chunk c+1 into LDS.  vmcnt retires in order, so an MFMA
// wave that issued HBM loads would stall its next weight-fragment wait on them; loader waves take that
// latency instead, and wait at the chunk barrier without using issue slots.
// Register budget: the waves of WPC workgroups per CU over the 4 SIMDs, at least 2 per SIMD.
// A single workgroup of <= 4 waves per CU runs one wave per SIMD with the whole 512-register file
// (VGPR + AGPR): accumulators of twice the rows per weight fragment.
template <int NW, int WPC>
constexpr int waves_per_eu() { return NW * WPC > 8 ? (NW * WPC + 3) / 4 : NW * WPC <= 4 ? 1 : 2; }
// LW > 0: LW loader waves; LW <= 0: no loaders, MFMA waves 0 .. -LW-1 stage (LW = 0: kStagers of them)
constexpr int loaders(int lw) { return lw > 0 ? lw : 0; }
// The dense-row instantiation of a layer without loader waves (block 2) stages on all its MFMA waves: the
// extra edge unit beside four stagers' eight units and the NRT B-fragment bases spilled (52 B / lane), with
// eight stagers' five units the kernel fits (253 VGPRs, no scratch).
constexpr int dense_lw(int lw, int wm, int wn) { return lw > 0 ? lw : -(wm * wn); }

// first window / first dense row w0 of a tile, its group g, its first window wf, its start off inside it,
// and the rows from its first row to the end of the group (clamped: only rows of the tile are compared)
struct Geo {
  int g, w0, wf, off, rows_left;
};

// ---- tile walk.  Tiles per group at a layer's tile size, and the tiles [tile_begin(wg), tile_begin(wg + 1))
// of workgroup wg of a grid (a partition of [0, total_tiles) into contiguous, near-equal ranges)
template <typename I>
__host__ __device__ constexpr I tiles_per_group(bool dense_rows, I n_win, int S) {
  return dense_rows ? (I)dense::tiles(n_win, kSR * S) : (n_win + S - 1) / S;
}
__host__ __device__ constexpr int tile_begin(int wg, int total_tiles, unsigned grid) {
  return (int)((long long)wg * total_tiles / grid);
}
template <bool DENSE, int S>
__host__ __device__ constexpr Geo tile_geo(int tile, int tpg, int n_win) {
  Geo G{};
  G.g = tile / tpg;
  G.w0 = (tile - G.g * tpg) * (DENSE ? kSR * S : S);
  G.wf = DENSE ? G.w0 / kL : G.w0, G.off = DENSE ? G.w0 - G.wf * kL : 0;
  const long long left = (long long)(n_win - G.wf) * kL - G.off;
  G.rows_left = (int)(left < 1024 ? left : 1024);
  return G;
}

// PS: the per-sample prescale (moving statistics) is compiled in; without it (batch moments: per-group
// prescale folded into the affine) the kernel has the registers of its tracking for other uses.
// DENSE: dense-row tiles; the batch-moment kernels of blocks 2..5 only (block 6's per-sample masked sums and
// the per-sample prescale's bitwise chunk invariance keep whole slots).
template <int CIN, int COUT, int KS, int S, int WM, int WN, bool LAST, int LW, int CK, int WPC, bool PS, bool DENSE = false>
struct Cfg {
  static constexpr int NWM = WM * WN, NW = NWM + loaders(LW), kThreads = NW * 64;
  static constexpr int kRowB = row_bytes(CK), NQ = CK / 32, kQ = CK / 4;  // 32-ch sub-chunks, quads / row
  static constexpr int PAD = (KS - 1) / 2, kRows = kSR * S;                // GEMM rows per tile
  static_assert(!DENSE || (!PS && !LAST), "dense rows: batch-moment blocks 2..5 only");
  static_assert(kThreads <= 1024, "workgroup size");
  // dense rows: in LDS the windows a tile touches (at most 4 / 6 for 128 / 256 rows) keep fixed 64-row slots
  // relative to the first one, so the zero rows never move and are never written
  static constexpr int kBufB = DENSE ? dense::lds_rows(kRows) * kRowB : buf_bytes(S, CK);
  // staged rows per chunk: the samples' time steps (dense rows: every row of the tile, see kMainU)
  static constexpr int kValidRows = DENSE ? kRows : S * kL, kUnits = kValidRows * kQ;
  // staging waves: the LW loader waves, else MFMA waves 0..SW-1 (one per SIMD by default)
  static constexpr int SW = LW > 0 ? LW : LW < 0 ? (-LW < NW ? -LW : NW) : (kStagers < NW ? kStagers : NW);
  static constexpr int kSBase = LW > 0 ? NWM * 64 : 0;  // first staging thread
  static constexpr int kST = SW * 64;                   // staging threads
  // 16-B staging units per staging thread: thread i keeps channel quad i % kQ of rows i / kQ + (kST / kQ) u.
  // Dense rows: kMainU units tile the rows of the tile exactly, and one more holds the PAD edge rows either
  // side of it, on the first staging wave(s) only
  static constexpr int kMainU = (kUnits + kST - 1) / kST, kNU = kMainU + (DENSE ? 1 : 0);
  static constexpr int kEdgeWaves = (2 * PAD * kQ + 63) / 64;
  static_assert(!DENSE || (kUnits % kST == 0 && kEdgeWaves <= SW), "dense rows: whole staging steps per tile");
  static_assert(kST % kQ == 0 && (CK == 32 || CK == 64), "a staging thread keeps one channel quad");
  // Each MFMA wave owns NRT 16-row tiles x NCT 16-channel tiles of the NCTA x 4 S accumulator tiles
  static constexpr int NCH = CIN / CK, NCTA = COUT / 16, NCT = NCTA / WN, NRT = 4 * S / WM;
  static constexpr int NSTEP = NCH * NQ * KS;  // k-steps (32 input channels x one tap) per tile
  // MFMA issue order: row tiles in groups of RG so that >= 4 accumulators rotate (dependent-issue
  // latency); B fragments double-buffered one group ahead when the accumulators leave room
  static constexpr int RG = NCT >= 4                       ? 1
                            : (NCT >= 3 && NCT * NRT > 16) ? 1
                            : NCT == 1                     ? 4
                                                           : 2;
  static constexpr bool BDB = NCT * NRT <= 24 && RG < 4;
  static_assert(NRT % RG == 0, "row-tile groups");
  static constexpr long long FRAG_STEP = (long long)NCTA * 128;  // f16x8 per (chunk, tap) k-step
  static_assert(CIN % CK == 0 && COUT % 16 == 0, "channel tiling");
  static_assert(NCTA % WN == 0 && (4 * S) % WM == 0, "wave tiling");
  static_assert(NRT % 4 == 0, "whole 64-row sample slots per wave row (epilogue keys, block 6 sums)");
  static_assert(S <= 8, "packed per-sample exponents");
  static constexpr int kSP = (S + 3) / 4;  // registers of the S samples' prescale exponents, a signed byte each

  // Row tables of the dense-row kernels: one staging thread per row, in steps of kST rows
  static constexpr int kTabRows = tab_rows(S, KS);
  static_assert(!DENSE || NCH >= 2, "row tables: a tile's tables are written one chunk of the same workgroup ahead");
  // Mask table (mask_tab_layer): mtab[row][COUT / 16], bit c % 16 of word c / 16 keeps channel c, so the
  // 16-bit word of an accumulator tile's row holds the lane's four bits at 4 h.  kMtT loader threads share a
  // row, kMtW words each, kMtPhase of them per chunk iteration 0 .. NCH - 2 of the tile.
  static constexpr bool kMaskTab = mask_tab_layer(CIN, COUT, KS, LW, DENSE);
  static constexpr int kMtRowW = COUT / 16, kMtT = kMaskTab ? kST / kRows : 1, kMtW = kMtRowW / kMtT;
  static constexpr int kMtPhase = (kMtW + (NCH > 1 ? NCH - 2 : 0)) / (NCH > 1 ? NCH - 1 : 1);
  static_assert(!kMaskTab || NCH >= 2, "mask table: written in the chunk iterations ahead of the tile's last");
  static_assert(!kMaskTab || (kST % kRows == 0 && kMtRowW % kMtT == 0), "mask table: whole words per loader thread");

  // ---- the LDS carve: byte offsets of the regions of the workgroup's dynamic LDS, in order
  //   buf    char [2][kBufB]        the two chunk buffers
  //   st     double [2][COUT]       the workgroup's fp64 moment sums
  //   wsc    float [2][S]           [tile & 1][sample]: wscale x 2^-sa, the epilogue's undo of both prescales
  // and for dense rows (x3_dense_map.h): what staging and epilogue need to know about a row depends on
  // (tile, row) only, so the staging waves compute it once per tile and every chunk and channel tile looks it up
  //   ektab  unsigned [2][kRows]    [tile & 1][tile row]: output-mask word, where the layer draws the block's mask
  //   stab   uint2 [2][kTabRows]    [tile & 1][staged row]: descriptor (LDS row, step, window slot, valid),
  //                                 input-mask word key ^ (t << 9)
  //   mtab   ushort [kRows][COUT / 16]  kMaskTab: the output keep-bits of the current tile
  static constexpr int buf = 0, st = buf + 2 * kBufB, wsc = st + 2 * COUT * 8, ektab = wsc + 2 * S * 4;
  static constexpr int stab = ektab + (DENSE ? 2 * kRows * 4 : 0), mtab = stab + (DENSE ? 2 * kTabRows * 8 : 0);
  static constexpr int bytes = mtab + (kMaskTab ? mask_tab_bytes(S, COUT) : 0);
  static_assert(buf % 16 == 0 && st % 8 == 0 && wsc % 4 == 0 && ektab % 4 == 0 && stab % 8 == 0 && mtab % 2 == 0,
                "LDS carve: alignment");
  static_assert(WPC * bytes <= 160 * 1024, "LDS of the workgroups sharing a CU");

  // ---- staging units.  Slot tiles: row ri = 60 s + t of unit u of staging thread i (staged iff ri < kValidRows)
  __host__ __device__ static constexpr int slot_unit_row(int u, int i) { return i / kQ + (kST / kQ) * u; }
  // the waves that keep the dense-row edge unit: the first kEdgeWaves staging waves
  __host__ __device__ static constexpr bool edge_wave(int wave) {
    return DENSE && wave >= kSBase / 64 && wave - kSBase / 64 < kEdgeWaves;
  }
  // Dense rows, unit u of staging thread i (of a wave with edge = edge_wave(wave)): its row relative to the
  // tile's first row (the edge unit holds the PAD rows either side of the tile); false where the thread has
  // no such unit
  __host__ __device__ static constexpr bool unit_row(int u, int i, bool edge, int& rel) {
    const int r = i / kQ;
    if (u < kMainU) {
      rel = r + (kST / kQ) * u;
      return true;
    }
    rel = r < PAD ? r - PAD : kRows - PAD + r;
    return edge && r < 2 * PAD;
  }
};

}  // namespace x3
}  // namespace apneauq

// Layer table of the reference architecture (cnn_baseline_train.py:59-86), blocks 2..6:
//   <layer, Cin, Cout, k, samples per tile, wave rows WM, wave channel groups WN, block 6, loader waves LW
//    (<= 0: no loaders, -LW MFMA waves stage) with / LWB without the per-sample prescale,
//    input channels per staged chunk CK, persistent workgroups per CU WPC, DENSE: the dense-row
//    instantiation (batch moments, blocks 2..5) is compiled in and can be picked per call>
// The 64-accumulator-tile layers (Cout 224 / 256) run 2-sample tiles so that the next k-step's weight
// fragments and the B double-buffer fit beside the accumulators without spilling.  Loader waves (ablation table
// in profiles/x3_loader_waves.md) on every layer but block 2, whose 96-accumulator tile needs the 256-VGPR
// budget of 8 waves (loaders at 2-sample tiles: slower; at 4: 99 VGPRs spilled); its staging runs on
// MFMA waves 0..3, or on all 8 where the per-sample prescale's registers would otherwise spill.  64-channel
// chunks for blocks 3 and 6 (block 2 would spill; Cin 224 / 96 are not multiples of 64).  The Cout-96 blocks 4
// and 6 run 4 MFMA waves of 24 accumulator tiles (WM 2 x WN 2) rather than 8 of 12: each weight fragment
// is re-read by 2 wave rows instead of 4 (their texture path was the busy one), -1.2 % MCD.
// Measurements: profiles/x3_epilogue_ab_r3.md, profiles/x3_mask_side_r4.md.
// A/B builds may substitute another table (APNEAUQ_X3_TABLE=<path.h> in csrc/build.py, tools/probes/x3_tables/):
// every entry is a complete, correct configuration, only the speed differs.  The define reaches the HIP
// translation unit only, so host code asks x3_layer_info() (x3_api.h) and never reads the table itself.
#ifdef APNEAUQ_X3_TABLE
#include APNEAUQ_X3_TABLE
#else
#define APNEAUQ_X3_LAYERS(X)                            \
  X(1, 128, 192, 5, 4, 2, 4, false, -8, 0, 32, 1, true) \
  X(2, 192, 224, 3, 2, 1, 7, false, 4, 4, 64, 1, true)  \
  X(3, 224, 96, 7, 4, 2, 2, false, 4, 4, 32, 1, true)   \
  X(4, 96, 256, 9, 2, 1, 8, false, 4, 4, 32, 1, true)   \
  X(5, 256, 96, 9, 4, 2, 2, true, 4, 4, 64, 1, false)
#endif

namespace apneauq {
namespace x3 {

// What the host needs to know about a row of the table: its tile size, workgroups per CU, whether the
// dense-row kernel is compiled, and the dynamic LDS of each compiled variant (per-sample prescale with LW,
// batch moments with LWB, dense rows; 0: no such kernel).  S == 0: no such layer.
struct LayerInfo {
  int S, WPC;
  bool has_dense;
  int lds_ps, lds_batch, lds_dense;
};
template <bool HAVE, int CIN, int COUT, int KS, int S, int WM, int WN, int LW, int CK, int WPC>
constexpr int dense_lds_bytes() {
  if constexpr (HAVE) {
    return Cfg<CIN, COUT, KS, S, WM, WN, false, dense_lw(LW, WM, WN), CK, WPC, false, true>::bytes;
  } else {
    return 0;
  }
}
constexpr LayerInfo layer_info(int layer) {
#define APNEAUQ_X3_INFO(L, CI, CO, K, S, WM, WN, LAST, LW, LWB, CK, WPC, DENSE)                              \
  if (layer == L)                                                                                            \
    return LayerInfo{S, WPC, DENSE && !LAST, Cfg<CI, CO, K, S, WM, WN, LAST, LW, CK, WPC, true>::bytes,      \
                     Cfg<CI, CO, K, S, WM, WN, LAST, LWB, CK, WPC, false>::bytes,                            \
                     dense_lds_bytes<DENSE && !LAST, CI, CO, K, S, WM, WN, LWB, CK, WPC>()};
  APNEAUQ_X3_LAYERS(APNEAUQ_X3_INFO)
#undef APNEAUQ_X3_INFO
  return LayerInfo{0, 1, false, 0, 0, 0};
}

}  // namespace x3
}  // namespace apneauq

#ifdef APNEAUQ_X3_GEO_PLAIN
#undef __host__
#undef __device__
#undef APNEAUQ_X3_GEO_PLAIN
#endif
