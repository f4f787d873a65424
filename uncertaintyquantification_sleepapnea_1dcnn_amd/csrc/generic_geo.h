// Launch geometry of the bf16 and exact-fp32 ("gf32") kernels of the generic layer-wise path (generic_conv.hip,
// the wgrad and pack launches of generic_wgrad.hip, gf32_conv.hip): how a launch of n samples x L steps becomes
// tiles, grids, LDS bytes and row groups.  Stated once: these kernels take their constants from here, their
// launchers fill their Args and pick their instantiation from the plans below, and the tests learn every number
// by running tests/generic_geo_check.cpp, which also checks this header against brute force on the host.
// (The fp16x3 engine, gx3_conv.hip, and the elementwise launches of generic_train.hip still state their own.)
// Plain constexpr / inline C++17 over ints: no HIP header, no Args.
#pragma once
#include <type_traits>

namespace apneauq {
namespace ggeo {

// ------------------------------------------------------------------------------------------------ constants
constexpr int kThreads = 256;
// conv tile of both engines: 2 x 2 waves, each kRT 16-row tiles x CT 16-channel tiles -> 128 rows
constexpr int kRT = 4, kWaveRows = 2, kWaveCols = 2;
constexpr int kTileRows = kWaveRows * kRT * 16;
// BN moment sums: kStatSlots interleaved atomic copies, or (deterministic) one plain-store slot per
// (workgroup, wave row), slot = blockIdx.x * kWaveRows + wave row
constexpr int kStatSlots = 16;
constexpr int det_conv_slots(int grid_x) { return kWaveRows * grid_x; }
// LDS rows of conv_lds_kernel's staged B operand (16 B of padding: 16 rows on different banks)
constexpr int bf16_row_stride(int cin) { return 2 * cin + 16; }
constexpr int kLdsLimit = 80 * 1024;  // stage while span * stride fits (3 workgroups per CU)
// wgrad: rows per LDS chunk of the gf32 kernel (kWgRC) and of the bf16 kernel (kChunk); most taps
constexpr int kWgRC = 64, kChunk = 64, kWgKMax = 15;

enum Engine { kBf16 = 0, kGf32 = 1 };
enum Mode { kInfer = 0, kTrain = 1, kLinear = 2 };
// bf16: conv_lds_kernel / conv_block_kernel<true> / <false>; gf32 has one kernel (kStaged, static LDS)
enum Kind { kStaged = 0, kVec = 1, kElem = 2 };

constexpr long long ceil_div(long long a, long long b) { return (a + b - 1) / b; }

// elements of one bf16 MFMA A-fragment array of a (k, cin, cout) kernel: (k-steps of 32, 16-channel tiles, 64
// lanes, 8); the pack launch covers the largest block's elements with at most kPackGrid workgroups per block
constexpr long long frag_elems(long long k, long long cin, long long cout) {
  return ((k * cin + 31) / 32) * 512 * ((cout + 15) / 16);
}
constexpr int kPackGrid = 1024;
constexpr int pack_grid(long long most) {
  const long long g = ceil_div(most, 256);
  return (int)(g > kPackGrid ? kPackGrid : g);
}

// ------------------------------------------------------------------------------------------------ conv
struct ConvPlan {
  long long rows;             // GEMM rows n * Lp
  int Lp, lout, pool, in_rs;  // Lp = L rounded up to even when pooling (kInfer only); rows of a sample's slot
  int nstep, nct, ct;         // k-steps of 32, 16-channel tiles of cout, channel tiles per wave
  int grid_x, grid_y;
  int kind;
  // input rows a 128-row tile can touch: 127 + ceil(127 / Lp) sample gaps of (in_rs - Lp) rows + the halo
  long long span;
  int lds_rows, lds_stride;  // bf16: what the kernel is told (lds_rows = span)
  long long lds_bytes;       // dynamic LDS of the launch
  int det_slots;             // moment slots a deterministic launch writes
};

// first channel tile of wave column wc of workgroup column by (the wave owns [ct0, min(ct0 + ct, nct)))
constexpr int conv_ct0(int ct, int by, int wc) { return (by * kWaveCols + wc) * ct; }

// cout: the channel count the tiles cover (bf16: Cout padded to 16).  has_rows: the input's row count is
// known (bf16 staging bound).
inline ConvPlan conv_plan(int engine, int mode, int n, int L, int cin, int cout, int ksize, int pool, int in_rs,
                          bool has_rows) {
  ConvPlan p = {};
  p.pool = (engine == kBf16 && mode == kInfer) ? pool : 0;
  p.Lp = p.pool ? (L + 1) / 2 * 2 : L;
  p.lout = p.pool ? L / 2 : L;
  p.in_rs = in_rs > 0 ? in_rs : L;
  p.rows = (long long)n * p.Lp;
  if (p.rows == 0) return p;  // nothing to launch
  p.nstep = (ksize * cin + 31) / 32;
  p.nct = (cout + 15) / 16;
  p.ct = (engine != kBf16 && p.nct % 6 == 0) ? 3 : 4;  // Cout a multiple of 96: no quarter of zero tiles
  p.grid_x = (int)ceil_div(p.rows, kTileRows);
  p.grid_y = (int)ceil_div(p.nct, kWaveCols * p.ct);
  p.det_slots = det_conv_slots(p.grid_x);
  const int pad = (ksize - 1) / 2;
  p.span = kTileRows + (long long)(kTileRows - 1 + p.Lp - 1) / p.Lp * (p.in_rs > p.Lp ? p.in_rs - p.Lp : 0) + 2 * pad;
  if (engine == kBf16) {
    p.lds_rows = (int)p.span, p.lds_stride = bf16_row_stride(cin);
    const bool lds = cin % 8 == 0 && p.span * p.lds_stride <= kLdsLimit && has_rows;
    p.kind = lds ? kStaged : cin % 8 == 0 ? kVec : kElem;
    p.lds_bytes = lds ? p.span * p.lds_stride : 0;
  } else {
    p.kind = kStaged;
  }
  return p;
}

// ------------------------------------------------------------------------------------------------ wgrad
// gf32: a workgroup = 32 ci x 64 co x one row group of whole kWgRC-row chunks; every group writes its own
// (k, cin, cout) slice of part, summed in order afterwards.  ~2 workgroups per CU in total, at least
// 256 rows per group, as many groups as part_floats has slices for.  groups == 0: rejected (no slice fits).
struct RowGroups {
  int ci_t, co_g;
  long long wfl, groups, rpg;  // floats of a slice, row groups (grid.z, = rows of the reduce), rows per group
};
constexpr long long wgrad_want_groups(int cin, int cout) {
  return ceil_div(512, ceil_div(cin, 32) * ceil_div(cout, 64));
}
inline RowGroups wgrad_row_groups(long long R, int cin, int cout, int k, long long part_floats) {
  RowGroups g = {};
  g.ci_t = (cin + 31) / 32, g.co_g = (cout + 63) / 64;
  g.wfl = (long long)k * cin * cout;
  long long groups = part_floats / g.wfl, want = wgrad_want_groups(cin, cout);
  if (want > (R + 255) / 256) want = (R + 255) / 256;
  if (groups > want) groups = want;
  if (groups > 65535) groups = 65535;
  if (groups < 1) return g;
  g.rpg = ceil_div(ceil_div(R, groups), kWgRC) * kWgRC;
  g.groups = ceil_div(R, g.rpg);
  return g;
}

// bf16 (generic_wgrad.hip): a workgroup = one 16-channel ci tile (im2col: kk = tap * cin + ci < 32 as the M
// dimension) x 64 nco co x a contiguous range of kChunk-row chunks; block order (ci tile, co block, row group).
struct GtWgradPlan {
  bool ok, im2col;
  int nco, kmax;  // co tiles per wave; taps held in accumulators (the KMAX instantiation; im2col: 1)
  int n_ci, n_co, chunks_per_wg;
  long long wfl, chunks, rgs, grid;  // rgs: row groups (deterministic: slices of part, rows of the reduce)
};
// co tiles per wave: the fewest padded tile slots (4 waves x nco per block), then the largest nco; the
// accumulators (k x nco tiles) are capped so a workgroup keeps >= 2 waves per SIMD
constexpr int gt_wgrad_nco(int cout, int k) {
  const int tiles = (cout + 15) / 16, nmax = k <= 5 ? 4 : k <= 9 ? 3 : 2;
  int nco = 1;
  for (int c = 2; c <= nmax; ++c)
    if (ceil_div(tiles, 4 * c) * 4 * c <= ceil_div(tiles, 4 * nco) * 4 * nco) nco = c;
  return nco;
}
// det: the row groups write slices of part (part_floats floats) instead of atomics
inline GtWgradPlan gt_wgrad_plan(long long R, int cin, int cout, int k, bool det, long long part_floats) {
  GtWgradPlan p = {};
  p.im2col = cin * k <= 32;
  p.nco = gt_wgrad_nco(cout, k);
  p.kmax = p.im2col ? 1 : k <= 3 ? 3 : k <= 5 ? 5 : k <= 9 ? 9 : 15;
  p.n_ci = p.im2col ? 1 : (cin + 15) / 16;
  p.n_co = (int)ceil_div((cout + 15) / 16, 4 * p.nco);
  p.chunks = ceil_div(R, kChunk);
  p.wfl = (long long)k * cin * cout;
  // ~2048 workgroups (8 per CU over the 256 CUs), but at least minc chunks each: every workgroup ends
  // with k * 16 * 64 * NCO fp32 atomics, and the chip adds ~1.3 TB/s of atomic bytes, so at 4 chunks
  // per workgroup the k = 9 blocks of ModelSpec(30, 1) spent ~100 us of a ~106 us wgrad on them.
  const long long minc = k <= 3 ? 4 : 2 * k, blocks = (long long)p.n_ci * p.n_co;
  long long rg = 2048 / blocks;
  if (rg < 1) rg = 1;
  if (rg > ceil_div(p.chunks, minc)) rg = ceil_div(p.chunks, minc);
  if (det && rg > part_floats / p.wfl) rg = part_floats / p.wfl;  // one partial slice per row group
  if (rg < 1) rg = 1;
  p.chunks_per_wg = (int)ceil_div(p.chunks, rg);
  p.rgs = ceil_div(p.chunks, p.chunks_per_wg);
  p.grid = blocks * p.rgs;
  p.ok = p.grid <= 0x7FFFFFFF && !(det && p.rgs * p.wfl > part_floats);
  return p;
}

// f(std::integral_constant<int, k>) for a runtime tap count k in [K, KMAX]; false: out of range
template <int K, int KMAX, class F>
inline bool dispatch_k(int k, F&& f) {
  if (k == K) {
    f(std::integral_constant<int, K>{});
    return true;
  }
  if constexpr (K < KMAX) return dispatch_k<K + 1, KMAX>(k, f);
  return false;
}

}  // namespace ggeo
}  // namespace apneauq
