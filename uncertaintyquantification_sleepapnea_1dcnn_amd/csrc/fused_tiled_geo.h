// Geometry of the fused tiled whole-network kernels, once for both precisions: fused_tiled.hip (bf16)
// and fused_tiled_x3.hip (fp16x3) are the same kernel with different LDS rows.
//
// The first part is plain constexpr C++ (no HIP types), shared by the kernels and a host test
// (tests/tiled_geo_check.cpp): the net tables, the per-block geometry Geo, the slot-row map and the
// compile-time checks.  The second part (hipcc only) is the device and launch scaffolding the two kernels
// share: Args, Ctx, drop4, the dropout-key setup, the logit write and the host launch.  Each .hip file
// keeps its own LDS carve (Lay), its wave-to-tile prologue, K loop, B-fragment loads and epilogue (the
// prologue is the same text in both: moving it into a shared struct changed the instruction stream of
// all four bf16 kernels, profiles/shared_device_helpers.md).
//
// Slot layout: block l's input lives in LDS in per-sample slots of SIN rows: LIN valid rows, then zero
// rows that double as the 'same' padding of the next slot (SIN >= LIN + PAD), so the implicit-GEMM conv
// needs no bounds checks.  A computed GEMM row o is slot row (o / OPS) * SIN + o % OPS: all slot rows
// where OPS == SIN, else only the prefix a block needs (pooled blocks 4 / 5 compute the 8 of 12 / 2 of 8
// rows their pool keeps; the single-channel net computes 32 rows per 34-row slot, so a sample is exactly
// two row tiles).  Taps that can never reach a valid input row are skipped (T0 .. T1-1 run): pooled
// block 5 (3 rows, k = 9) runs taps 3..6 for its 2 kept rows, block 6 (1 row) only the centre tap.
#pragma once

#include "arch_tables.h"

#ifndef __host__
#define APNEAUQ_TILED_GEO_PLAIN 1
#define __host__
#define __device__
#endif

namespace apneauq {
namespace tgeo {

using arch::C;
using arch::KS;

constexpr int kThreads = 256;  // 4 waves

// LDS row of a block input with c channels.  bf16: c values + 16 B (conflict-free rows).  fp16x3:
// [hi c x fp16 | lo c x fp16 | 16 B] (c/4 + 1 16-B slots, odd: the ds_read_b128 lane groups of a B
// fragment hit distinct slots).  x0 row: block 1's staged input, an im2col row (8 k) or CIN0 = 4 channels.
// kGuardsTail: the kernel never stores rows past its last sample, so the last row tile may be partly
// discarded (the x3 kernel's `smp < NS` guards; the bf16 kernel has none and needs an exact cover).
struct Bf16Rows {
  static constexpr bool kGuardsTail = false;
  __host__ __device__ static constexpr int row_bytes(int c) { return 2 * c + 16; }
  __host__ __device__ static constexpr int x0_row_bytes(bool im2col, int cin0) { return im2col ? 16 : cin0 * 2; }
};
struct X3Rows {
  static constexpr bool kGuardsTail = true;
  __host__ __device__ static constexpr int row_bytes(int c) { return 4 * c + 16; }
  __host__ __device__ static constexpr int x0_row_bytes(bool im2col, int) { return im2col ? 32 : 16; }  // [hi | lo]
};

// Per-net tables, precision-independent part.  WM: wave rows (4 / WM wave columns over the channel
// tiles); NF: full channel tiles per wave; HALF: Cout tiles that do not split 4 ways (224 -> 14, 96 -> 6
// = 2 pairs x (2 NF + 1)) -- each wave pair shares its middle tile, one wave per half of the row tiles,
// so every weight fragment is requested once per workgroup and all waves issue the same MFMA count.
struct PooledBase {  // MaxPool1D(2, valid) after blocks 1-5: lengths 60 -> 30 -> 15 -> 7 -> 3 -> 1
  static constexpr int L = 60, CIN0 = 4;
  static constexpr bool IM2COL = false;  // block 1 reads 2 rows x 4 channels per lane from x0
  static constexpr int X0ROWS = 64;      // x0 slot rows per sample
  static constexpr int LIN[6] = {60, 30, 15, 7, 3, 1};
  static constexpr int SIN[6] = {64, 32, 16, 12, 8, 1};
  static constexpr int OPS[6] = {64, 32, 16, 8, 2, 1};
  static constexpr int LOUT[6] = {30, 15, 7, 3, 1, 1};  // rows stored (after the pool)
  static constexpr bool POOL[6] = {true, true, true, true, true, false};
  static constexpr int T0[6] = {0, 0, 0, 0, 3, 4}, T1[6] = {7, 5, 3, 7, 7, 5};
  static constexpr int WM[6] = {1, 1, 1, 1, 1, 1}, NF[6] = {2, 3, 3, 1, 4, 2};
  static constexpr bool HALF[6] = {false, false, true, true, false, false};
};
struct Single30Base {  // the 30 s single-channel window, no pooling
  static constexpr int L = 30, CIN0 = 1;
  static constexpr bool IM2COL = true;  // x0 row t holds x[t-3 .. t+4]: the 8 k of lane group h = 0
  static constexpr int X0ROWS = 32;
  static constexpr int LIN[6] = {30, 30, 30, 30, 30, 30};
  static constexpr int SIN[6] = {32, 34, 34, 34, 34, 34};
  static constexpr int OPS[6] = {32, 32, 32, 32, 32, 32};
  static constexpr int LOUT[6] = {30, 30, 30, 30, 30, 30};
  static constexpr bool POOL[6] = {false, false, false, false, false, false};
  static constexpr int T0[6] = {0, 0, 0, 0, 0, 0}, T1[6] = {7, 5, 3, 7, 9, 9};
  static constexpr int WM[6] = {1, 1, 1, 1, 1, 2}, NF[6] = {2, 3, 3, 1, 4, 3};
  static constexpr bool HALF[6] = {false, false, true, true, false, false};
};

}  // namespace tgeo

// Per precision: P the row policy, NS samples per workgroup, RG / NG row tiles per row group / row
// groups (bf16: blocks 1-2 of the pooled net are split into row groups of 8 tiles to bound the
// accumulators; the doubled x3 rows halve NS so that two workgroups still share a CU, one group per
// block), PD (bf16): k-steps of weight fragments in flight (depths 2-6 measured 0.8-1.9 % slower than 1
// on the pooled net: weight latency does not bound these kernels).
namespace tiled {
struct PooledNet : tgeo::PooledBase {
  using P = tgeo::Bf16Rows;
  static constexpr int NS = 8;
  static constexpr int RG[6] = {8, 8, 8, 4, 1, 1}, NG[6] = {4, 2, 1, 1, 1, 1};
  static constexpr int PD[6] = {1, 1, 1, 1, 1, 1};
};
struct Single30Net : tgeo::Single30Base {
  using P = tgeo::Bf16Rows;
  static constexpr int NS = 4;
  static constexpr int RG[6] = {8, 8, 8, 8, 8, 8}, NG[6] = {1, 1, 1, 1, 1, 1};
  static constexpr int PD[6] = {1, 1, 1, 1, 1, 1};
};
}  // namespace tiled
namespace tiled3 {
struct PooledNet : tgeo::PooledBase {
  using P = tgeo::X3Rows;
  static constexpr int NS = 4;
  static constexpr int RG[6] = {16, 8, 4, 2, 1, 1}, NG[6] = {1, 1, 1, 1, 1, 1};
};
struct Single30Net : tgeo::Single30Base {
  using P = tgeo::X3Rows;
  static constexpr int NS = 2;
  static constexpr int RG[6] = {4, 4, 4, 4, 4, 4}, NG[6] = {1, 1, 1, 1, 1, 1};
};
}  // namespace tiled3

namespace tgeo {

__host__ __device__ constexpr int cmax(int a, int b) { return a > b ? a : b; }

// block 6 of a net whose last length is 1: one GEMM row per sample, GAP is the identity
template <class N>
__host__ __device__ constexpr bool rowhead() { return N::OPS[5] == 1; }
// computed GEMM rows of block l (all row groups)
template <class N>
__host__ __device__ constexpr int gemm_rows(int l) { return N::RG[l] * N::NG[l] * 16; }
// slot row that GEMM row o of block l >= 1 reads at the centre tap
template <class N>
__host__ __device__ constexpr int slot_row(int l, int o) {
  return (N::OPS[l] == N::SIN[l] || (rowhead<N>() && l == 5)) ? o : (o / N::OPS[l]) * N::SIN[l] + o % N::OPS[l];
}
// bytes of the largest block input (blocks 2-6; block 1 reads x0)
template <class N>
__host__ __device__ constexpr int max_act() {
  int m = 0;
  for (int l = 1; l < 6; ++l) m = cmax(m, N::NS * N::SIN[l] * N::P::row_bytes(C[l]));
  return m;
}
// Bytes in front of the first slot that a tap of a computed row can read (the taps before row 0 that a
// block runs), and bytes past max_act() (the discarded rows of the last row tile: finite, never stored);
// both rounded up to 16.  The LDS carve of a kernel reserves at least these (Lay).
template <class N>
__host__ __device__ constexpr int lead_bytes() {
  int m = 0;
  for (int l = 1; l < 6; ++l) m = cmax(m, cmax(0, (KS[l] - 1) / 2 - N::T0[l]) * N::P::row_bytes(C[l]));
  return (m + 15) / 16 * 16;
}
template <class N>
__host__ __device__ constexpr int trail_bytes() {
  int m = 0;
  for (int l = 1; l < 6; ++l) {
    const int last = slot_row<N>(l, gemm_rows<N>(l) - 1) + N::T1[l] - 1 - (KS[l] - 1) / 2 + 1;
    m = cmax(m, last * N::P::row_bytes(C[l]) - max_act<N>());
  }
  return (m + 15) / 16 * 16;
}
// x0: kX0Lead zero rows, NS slots of X0ROWS rows, kX0Trail zero rows
template <class N>
__host__ __device__ constexpr int x0_lead() { return N::IM2COL ? 0 : 4; }
constexpr int kX0Trail = 8;
template <class N>
__host__ __device__ constexpr int x0_row_bytes() { return N::P::x0_row_bytes(N::IM2COL, N::CIN0); }

template <class N, int L>
struct Geo {
  static constexpr int CIN = C[L], COUT = C[L + 1], K = KS[L], PAD = (KS[L] - 1) / 2;
  static constexpr bool FIRST = L == 0, HEAD = L == 5, POOL = N::POOL[L];
  static constexpr int NCT = COUT / 16;
  static constexpr int CB = FIRST ? 1 : CIN / 32;
  static constexpr int S0 = FIRST ? 0 : N::T0[L] * CB, S1 = FIRST ? 1 : N::T1[L] * CB;  // k-steps run
  static constexpr int NWC = 4 / N::WM[L];             // wave columns
  static constexpr int NRW = N::RG[L] / N::WM[L];      // row tiles per wave per group
  static constexpr int SI = FIRST ? x0_row_bytes<N>() : N::P::row_bytes(CIN);
  static constexpr int SOUT = L < 5 ? N::SIN[L + 1] : 1, SO = N::P::row_bytes(COUT);
  static constexpr int SPG = N::RG[L] * 16 / N::OPS[L];  // samples per row group
};

// compile-time checks of the slot geometry and the in-place hand-over
template <class N, int L>
__host__ __device__ constexpr bool geometry_ok() {
  using G = Geo<N, L>;
  const int rows = gemm_rows<N>(L), want = N::NS * N::OPS[L];
  if (L < 5 || !rowhead<N>()) {
    // the row groups tile the computed rows; a kernel that guards its stores may discard part of the
    // last row tile of a single group
    if (rows != want && !(N::P::kGuardsTail && N::NG[L] == 1 && rows > want && rows < want + 16)) return false;
  } else if (N::RG[L] * 16 < N::NS) {
    return false;
  }
  if (N::OPS[L] > N::SIN[L] && !(L == 5 && rowhead<N>())) return false;
  if (G::POOL && (N::OPS[L] % 2 != 0 || 2 * N::LOUT[L] > N::OPS[L] || N::SIN[L] % 2 != 0)) return false;
  if (L == 0 && (N::OPS[L] != N::SIN[L] || N::SIN[L] != N::X0ROWS)) return false;
  if (N::HALF[L] ? (N::WM[L] != 1 || G::NCT != 2 * (2 * N::NF[L] + 1) || G::NRW % 2 != 0)
                 : (G::NWC * N::NF[L] < G::NCT || N::RG[L] % N::WM[L] != 0))
    return false;  // wave tiling covers the block
  if (L > 0 && N::LIN[L] > 1 && N::SIN[L] < N::LIN[L] + G::PAD) return false;  // zero rows = next slot's padding
  if (L < 5 && (N::LOUT[L] > G::SOUT || N::LOUT[L] > N::OPS[L])) return false;
  // row group g's output ends before group g+1's first input row (minus the padding)
  if (L >= 1 && N::NG[L] > 1 && G::SPG * G::SOUT * G::SO > (G::SPG * N::SIN[L] - G::PAD) * G::SI) return false;
  if (L >= 1 && N::NS * N::SIN[L] * G::SI > max_act<N>()) return false;
  // GAP head: a wave's rows are whole samples (two row tiles each)
  if (L == 5 && !rowhead<N>() &&
      (N::OPS[5] % 16 != 0 || N::NG[5] != 1 || N::HALF[5] || G::NRW % (N::OPS[5] / 16) != 0))
    return false;
  return true;
}
template <class N>
__host__ __device__ constexpr bool net_ok() {
  return geometry_ok<N, 0>() && geometry_ok<N, 1>() && geometry_ok<N, 2>() && geometry_ok<N, 3>() &&
         geometry_ok<N, 4>() && geometry_ok<N, 5>() && C[1] % 32 == 0 && C[2] % 32 == 0 && C[3] % 32 == 0 &&
         C[4] % 32 == 0 && C[5] % 32 == 0 && (N::IM2COL ? N::CIN0 * KS[0] <= 8 : N::CIN0 == 4);
}
static_assert(net_ok<tiled::PooledNet>() && net_ok<tiled::Single30Net>(), "bf16 geometry");
static_assert(net_ok<tiled3::PooledNet>() && net_ok<tiled3::Single30Net>(), "fp16x3 geometry");

}  // namespace tgeo
}  // namespace apneauq

#ifdef APNEAUQ_TILED_GEO_PLAIN
#undef __host__
#undef __device__
#undef APNEAUQ_TILED_GEO_PLAIN
#endif

// ---------------------------------------------------------------------------------------------
// Device and launch scaffolding shared by the two kernels
// ---------------------------------------------------------------------------------------------
#ifdef __HIPCC__
#include "common.h"

namespace apneauq {
namespace tgeo {

template <class XT>
struct Args {
  const XT* x;             // (n_win, L, CIN0), channels-last: bf16 / fp32 (x3)
  const uint8_t* blob;     // (n_member, blob bytes) packed parameters (ops/fused.py:pack_blob / pack_blob_x3)
  float* out;              // (n_member, n_pass, n_win)
  long long blob_stride;
  int n_win, n_pass, n_member;
  int tiles_per_member, total_items;
  unsigned window_offset, pass_offset;
  unsigned long long seed;
  int out_logits;
  unsigned thr[6];
};

struct Ctx {
  const guint8* blob;
  unsigned thr;
};

// 32-bit dropout decisions of channels (c0 .. c0+3) at step t applied to v (fp32 selects)
__device__ __forceinline__ void drop4(f32x4& v, unsigned key, unsigned t, unsigned c0, unsigned thr) {
  const unsigned b01 = dropout_bits2(key, t, c0), b23 = dropout_bits2(key, t, c0 + 2);
  v[0] = (b01 & 0xFFFFu) >= thr ? v[0] : 0.f;
  v[1] = (b01 >> 16) >= thr ? v[1] : 0.f;
  v[2] = (b23 & 0xFFFFu) >= thr ? v[2] : 0.f;
  v[3] = (b23 >> 16) >= thr ? v[3] : 0.f;
}

// keys[l * NS + s]: per-(block, sample) dropout keys of the tile, the same (seed, layer, pass, window)
// streams as every path
template <class N, class XT>
__device__ __forceinline__ void stage_keys(unsigned* keys, const Args<XT>& A, int tile, long long samples) {
  if (threadIdx.x < 6 * N::NS) {
    const int l = threadIdx.x / N::NS, sl = threadIdx.x % N::NS;
    const long long gs = (long long)tile * N::NS + sl;
    const long long gg = gs < samples ? gs : 0;
    const unsigned pass = (unsigned)(gg / A.n_win), win = (unsigned)(gg % A.n_win);
    keys[threadIdx.x] = sample_key(stream_key(A.seed, (unsigned)l, A.pass_offset + pass), A.window_offset + win);
  }
}

// The tile's logits from block 6's head partials (fixed order: bitwise sharding invariance), + the dense
// bias (dense: the blob's Dense weights, bias last), sigmoid unless out_logits.
template <class N, class XT>
__device__ __forceinline__ void write_logits(const float* head, const gfloat* dense, const Args<XT>& A, int member,
                                             int tile, long long samples) {
  constexpr int NS = N::NS;
  if (threadIdx.x < NS) {
    const int sl = threadIdx.x;
    const long long gs = (long long)tile * NS + sl;
    if (gs < samples) {
      float logit;
      if constexpr (rowhead<N>())  // [wave][sample], L = 1: GAP is the identity
        logit = head[sl] + head[NS + sl] + head[2 * NS + sl] + head[3 * NS + sl];
      else {  // [sample][wave column] sums over the L rows
        constexpr int NWC5 = 4 / N::WM[5];
        float s = 0.f;
#pragma unroll
        for (int w = 0; w < NWC5; ++w) s += head[NWC5 * sl + w];
        logit = s * (1.0f / N::L);
      }
      logit += dense[C[6]];
      const int pass = (int)(gs / A.n_win), win = (int)(gs % A.n_win);
      A.out[((long long)member * A.n_pass + pass) * A.n_win + win] =
          A.out_logits ? logit : 1.0f / (1.0f + __expf(-logit));
    }
  }
}

// One workgroup per tile of N::NS samples of one member; kern: the kernel instance (with or without
// dropout), lds_bytes: its Lay<N>::kLdsBytes.
template <class N, class XT>
hipError_t launch(void (*kern)(Args<XT>), int lds_bytes, const XT* x, const uint8_t* blob, long long blob_stride,
                  float* out, int n_win, int n_pass, int n_member, unsigned window_offset, unsigned pass_offset,
                  unsigned long long seed, int out_logits, const unsigned* thr, hipStream_t stream) {
  Args<XT> A;
  A.x = x;
  A.blob = blob;
  A.out = out;
  A.blob_stride = blob_stride;
  A.n_win = n_win;
  A.n_pass = n_pass;
  A.n_member = n_member;
  const long long samples = (long long)n_pass * n_win;
  const long long tiles = (samples + N::NS - 1) / N::NS;
  if (tiles < 1 || n_member < 1) return hipSuccess;
  if (tiles * n_member >= (1LL << 31)) return hipErrorInvalidValue;
  A.tiles_per_member = (int)tiles;
  A.total_items = (int)(tiles * n_member);
  A.window_offset = window_offset;
  A.pass_offset = pass_offset;
  A.seed = seed;
  A.out_logits = out_logits;
  for (int l = 0; l < 6; ++l) A.thr[l] = thr ? thr[l] : 0u;
  hipLaunchKernelGGL(kern, dim3(A.total_items), dim3(kThreads), lds_bytes, stream, A);
  return hipGetLastError();
}

}  // namespace tgeo
}  // namespace apneauq
#endif  // __HIPCC__
