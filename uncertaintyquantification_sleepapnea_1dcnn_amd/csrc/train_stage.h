// Device code shared by the training kernel families (train_fwd / train_head / train_dgrad / train_wgrad.hip):
// batched staging loops, the A = dropout(BN(R)) and dZ staging, the implicit-GEMM conv tile and the
// transposing fragment read.  Device-only; see train_launch.hip for the design (layout, sign-bit mask, what is
// recomputed where).
#pragma once
#include "train_args.h"

namespace apneauq {
namespace train {

// Staging loops issue a batch of up to kStageU global loads per thread before the first LDS
// write, so a tile's staging pays the memory latency ceil(items / (256 * kStageU)) times instead of
// once per item (a plain load->use loop waits vmcnt(0) on every iteration).
constexpr int kStageU = 8;

struct bf16x16 {
  bf16x8 a, b;
};

template <int N, int UMAX = kStageU, int NT = kThreads, typename Load, typename Store>
__device__ __forceinline__ void staged_loop(Load load, Store store) {
  constexpr int IT = (N + NT - 1) / NT;
  constexpr int U = IT < UMAX ? IT : UMAX;
  using P = decltype(load(0));
  // opaque thread index: inside a tile loop (wgrad) LICM would otherwise hoist every per-item
  // index/address out of the loop and keep them live across the MFMAs (VGPR spills)
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));
#pragma unroll
  for (int b = 0; b < IT; b += U) {
    P v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = tid + (b + u) * NT;
      if (b + u < IT && i < N) v[u] = load(i);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = tid + (b + u) * NT;
      if (b + u < IT && i < N) store(i, v[u]);
    }
  }
}

__device__ __forceinline__ bf16x8 zero8() {
  bf16x8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = (__bf16)0.f;
  return o;
}

// 8 consecutive per-channel floats of an LDS table (c0 a multiple of 8) times a scale: two 16-B LDS
// reads issued together (element-wise reads were 8 dependent round trips per table per tile)
__device__ __forceinline__ void lds_row8(const float* tab, int c0, float scale, float (&o)[8]) {
  const f32x4 a = *reinterpret_cast<const f32x4*>(tab + c0);
  const f32x4 b = *reinterpret_cast<const f32x4*>(tab + c0 + 4);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    o[j] = a[j] * scale;
    o[4 + j] = b[j] * scale;
  }
}

// Stage A_l (= dropout(BN(R_l))) rows [row0, row0 + NR) x channels [c0, c0 + NCW*8) of global
// PL buffer into LDS (row stride ldsrs bytes).  Pad rows and rows outside the batch become 0.
// row0 is a tile start (a multiple of 128), so the rows hold samples smp0 = row0/64 and smp0 + 1
// (plus the halo rows of the neighbours: pad rows, or rows whose outputs are discarded).
//
// Each thread owns one 8-channel chunk (cw = tid % NCW) for all its rows, so the BN affine of the
// chunk (x 1/(1-rate) when dropping) is loaded once per call instead of per 16-B item; the affine of
// the second stats group (a tile straddling an MC-Dropout pass boundary, g1 = s/t + 256) is selected
// per row only when it differs.  The dropout mask is R_l's sign bit (set by the producer), so the
// transform is  a = sign ? 0 : |r| * s + t  on the packed bf16 pairs.
template <int l, int NR, int NCW, int UMAX = kStageU, int NT = kThreads>
__device__ __forceinline__ void stage_act(const Args& A, char* lds, int ldsrs, int row0, int c0, const float* s,
                                          const float* t, int g0) {
  constexpr int Cc = C[l + 1];
  constexpr int RP = NT / NCW;  // rows per pass over the workgroup
  constexpr int NK = (NR + RP - 1) / RP;
  constexpr int U = NK < UMAX ? NK : UMAX;
  const Layer& Ly = A.L[l];
  // opaque thread index (see staged_loop): keeps the per-row addresses out of enclosing tile loops
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));
  const int cw = tid % NCW, rin = tid / NCW;
  const bool active = rin < RP;
  const int c = c0 + cw * 8;
  const int smp0 = row0 >> 6;
  const int g1 = min(smp0 + 1, A.B - 1) / A.n_win;
  const bool two = g1 != g0;  // workgroup-uniform
  const bool drop = A.dropout != 0;
  const float dsc = drop ? Ly.dsc : 1.f;
  float s0[8], t0[8], s1[8], t1[8];
  lds_row8(s, c, dsc, s0);
  lds_row8(t, c, dsc, t0);
  if (two) {  // workgroup-uniform; the tables of callers with one stats group end at s + 256
    lds_row8(s, 256 + c, dsc, s1);
    lds_row8(t, 256 + c, dsc, t1);
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      s1[j] = s0[j];
      t1[j] = t0[j];
    }
  }
  {
    // Every staged row exists in the padded buffer, and pad rows / rows past the batch / the
    // buffer's halo rows hold -0.0, which decodes to 0 like a dropped element: no per-row checks.
    auto run = [&](auto two_groups) {
#pragma unroll
      for (int b = 0; b < NK; b += U) {
        u32x4 v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int rc = rin + (b + u) * RP;
          if (b + u < NK && active && rc < NR) v[u] = gld<u32x4>(Ly.R + (long long)(row0 + rc) * Cc + c);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int rc = rin + (b + u) * RP;
          if (b + u >= NK || !active || rc >= NR) continue;
          const int r = rc;
          u32x4 o;
          if constexpr (decltype(two_groups)::value) {  // rare: a tile straddling an MC-Dropout pass boundary
            const bool hi = row_sample(row0 + r) != smp0;
#pragma unroll
            for (int q = 0; q < 4; ++q)
              o[q] = decode_pair(v[u][q], hi ? s1[2 * q] : s0[2 * q], hi ? t1[2 * q] : t0[2 * q],
                                 hi ? s1[2 * q + 1] : s0[2 * q + 1], hi ? t1[2 * q + 1] : t0[2 * q + 1]);
          } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) o[q] = decode_pair(v[u][q], s0[2 * q], t0[2 * q], s0[2 * q + 1], t0[2 * q + 1]);
          }
          *reinterpret_cast<u32x4*>(lds + lds_off(r, cw * 16, ldsrs)) = o;
        }
      }
    };
    if (two)
      run(std::true_type{});
    else
      run(std::false_type{});
  }
}

// The forward kernels' input staging split in two phases so that a tile's global loads overlap the
// previous tile's moments and copy-out: load() issues every row load of a tile into registers (no
// wait), store() decodes A = dropout(BN(R)) from them into LDS (same transform as stage_act, all
// CIN channels, 136 rows).
//
// HASH_IN (batch-BN MC Dropout, block 2 reading the pass-shared block-1 output): R_0 holds one
// unencoded copy per WINDOW.  Branch-free: every staged row maps to a row of R_0 -- rows of the
// tile's two samples to their window's rows, all other rows (halo rows of the neighbours) to pad
// row 60, which holds -0.0 and decodes to 0 -- and block 1's dropout mask is drawn here from the
// counter hash on every row, as sign bits (pad rows stay -0.0 whatever it draws).
//
// Only the tile's 2 x 60 valid rows are loaded; the 16 halo / pad rows of the LDS tile (0-3, 64-67,
// 128-135) are written as zeros instead (no global load, no decode).
template <int l, bool HASH_IN>  // HASH_IN: may run in hash_in mode (runtime flag, workgroup-uniform)
struct ActStager {
  static constexpr int Cc = C[l + 1];
  static constexpr int NCW = Cc / 8;
  static constexpr int RP = kThreads / NCW;  // rows per pass over the workgroup
  static constexpr int NR = kSlots * kL;  // rows loaded from memory (the two samples' valid rows)
  static constexpr int NK = (NR + RP - 1) / RP;
  u32x4 v[NK];

  // LDS row of loaded row rc: the slot's time step, skipping halo and pad rows
  __device__ __forceinline__ static int lds_row(int rc) {
    const int slot = rc >= kL;
    return kHalo + slot * kSR + (rc - kL * slot);
  }

  __device__ __forceinline__ static int tid() {
    int t = threadIdx.x;
    asm volatile("" : "+v"(t));  // opaque: keeps the per-row addresses out of the tile loop
    return t;
  }

  // every v[u] is assigned on every path (zeros where unused), so v is dead between store() and the
  // next load() -- in particular across the conv MFMAs
  // [U0, U1): the row batch to load / store (a split staging keeps fewer loads in flight)
  template <int U0 = 0, int U1 = NK>
  __device__ __forceinline__ void load(const Args& A, int row0, bool hash_in) {
    const int t = tid(), cw = t % NCW, rin = t / NCW;
#pragma unroll
    for (int u = U0; u < U1; ++u) v[u] = u32x4{0u, 0u, 0u, 0u};
    if (rin >= RP) return;
    const __bf16* R = A.L[l].R + cw * 8;
    if (HASH_IN && hash_in) {
      const int smp0 = row0 >> 6;
      const int n0 = min(smp0, A.B - 1), n1 = min(smp0 + 1, A.B - 1);
      const int g0 = n0 / A.n_win, g1 = n1 / A.n_win;
      const __bf16* src0 = R + (long long)(kHalo + (n0 - g0 * A.n_win) * kSR) * Cc;
      const __bf16* src1 = R + (long long)(kHalo + (n1 - g1 * A.n_win) * kSR) * Cc;
#pragma unroll
      for (int u = U0; u < U1; ++u) {
        const int rc = rin + u * RP;
        if (rc >= NR) continue;
        const int slot = rc >= kL;
        v[u] = gld<u32x4>((slot ? src1 : src0) + (long long)(rc - kL * slot) * Cc);
      }
    } else {
#pragma unroll
      for (int u = U0; u < U1; ++u) {
        const int rc = rin + u * RP;
        if (rc < NR)
          v[u] = gld<u32x4>(R + (long long)(row0 + lds_row(rc)) * Cc);
      }
    }
  }

  // s, t: the affine of stats group g0 (s + 256, t + 256: group g1 when the tile straddles two)
  template <int U0 = 0, int U1 = NK>
  __device__ __forceinline__ void store(const Args& A, char* lds, int row0, const float* s, const float* t,
                                        int g0, bool hash_in) const {
    const int tt_ = tid(), cw = tt_ % NCW, rin = tt_ / NCW;
    if (U0 == 0)  // the 16 halo / pad rows of the LDS tile: zeros (0-3, 64-67, 128-135)
      for (int i = tt_; i < 16 * NCW; i += kThreads) {
        const int pi = i / NCW, pr = pi < 4 ? pi : (pi < 8 ? kL + pi : 2 * kL + pi);
        *reinterpret_cast<u32x4*>(lds + pr * kRS + (i - pi * NCW) * 16) = u32x4{0u, 0u, 0u, 0u};
      }
    if (rin >= RP) return;
    const Layer& Ly = A.L[l];
    const int c = cw * 8;
    const int smp0 = row0 >> 6;
    const int g1 = min(smp0 + 1, A.B - 1) / A.n_win;
    const bool two = g1 != g0;  // workgroup-uniform
    const bool drop = A.dropout != 0;
    const float dsc = drop ? Ly.dsc : 1.f;
    float s0[8], t0[8], s1[8], t1[8];
    lds_row8(s, c, dsc, s0);
    lds_row8(t, c, dsc, t0);
    lds_row8(s, 256 + c, dsc, s1);  // second group (used only when two): unconditional, read together
    lds_row8(t, 256 + c, dsc, t1);
    unsigned key0 = 0u, key1 = 0u;
    if (HASH_IN && hash_in) {
      key0 = layer_sample_key(A, l, min(smp0, A.B - 1));
      key1 = layer_sample_key(A, l, min(smp0 + 1, A.B - 1));
    }
    const uint32_t thr2 = drop ? Ly.thr * 0x10001u : 0u;  // thr 0: nothing dropped
    auto run = [&](auto two_groups, auto hashed) {
#pragma unroll
      for (int u = U0; u < U1; ++u) {
        const int rc = rin + u * RP;
        if (rc >= NR) continue;
        const int r = lds_row(rc);
        const bool hi = rc >= kL;
        const int tstep = rc - kL * (rc >= kL);
        u32x4 o;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          uint32_t d = v[u][q];
          if constexpr (decltype(hashed)::value) d |= drop_signs2(dropout_bits2(hi ? key1 : key0, tstep, c + 2 * q), thr2);
          if constexpr (decltype(two_groups)::value)  // rare: a tile straddling an MC-Dropout pass boundary
            o[q] = decode_pair(d, hi ? s1[2 * q] : s0[2 * q], hi ? t1[2 * q] : t0[2 * q],
                               hi ? s1[2 * q + 1] : s0[2 * q + 1], hi ? t1[2 * q + 1] : t0[2 * q + 1]);
          else
            o[q] = decode_pair(d, s0[2 * q], t0[2 * q], s0[2 * q + 1], t0[2 * q + 1]);
        }
        *reinterpret_cast<u32x4*>(lds + r * kRS + cw * 16) = o;
      }
    };
    auto dispatch = [&](auto hashed) {
      if (two)
        run(std::true_type{}, hashed);
      else
        run(std::false_type{}, hashed);
    };
    if (HASH_IN && hash_in)
      dispatch(std::integral_constant<bool, HASH_IN>{});
    else
      dispatch(std::false_type{});
  }
};

// dZ_l rows into LDS (rows [row0, row0+NR), channels [c0, c0+NCW*8)); rows [own_lo, own_hi) are
// also written to ``gout`` (dgrad materialises dZ_l for wgrad).
//   l == 5: dY_6 = dlogit[n] * w[c] / 60 * mask6 * dsc6 (recomputed; never stored; mask6 = R_6's sign)
// As in stage_act, each thread owns one 8-channel chunk, and the BN backward
//   dz = relu'(r) * g*rstd * (dy - mean(dy) - xhat * mean(dy*xhat)),  xhat = (r - mean) * rstd
// is folded per channel into dz = relu'(r) * (al * dy + be * r + ga), evaluated from registers
// (r = |R_l|: the sign bit carries block l's dropout mask).
template <int l, int NR, int NCW>
__device__ __forceinline__ void stage_dz(const Args& A, char* lds, int ldsrs, int row0, int c0,
                                         const float* gam_rstd, const float* mean, const float* rstd, const float* mdy,
                                         const float* mdyx, __bf16* gout = nullptr,
                                         int own_lo = 0, int own_hi = 0) {
  constexpr int Cc = C[l + 1];
  constexpr int RP = kThreads / NCW;
  constexpr int NK = (NR + RP - 1) / RP;
  constexpr int U = NK < kStageU ? NK : kStageU;  // R + dY payloads in flight per thread
  const Layer& Ly = A.L[l];
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));
  const int cw = tid % NCW, rin = tid / NCW;
  const bool active = rin < RP;
  const int c = c0 + cw * 8;
  const int smp0 = (row0 >> 7) * 2;  // row0 is a tile start, or a tile start + kHalo
  float al[8], be[8], ga[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float g = gam_rstd[c + j], q = rstd[c + j] * mdyx[c + j];
    al[j] = g;
    be[j] = -g * q;
    ga[j] = g * (q * mean[c + j] - mdy[c + j]);
  }
  // block 6: dY is recomputed from dlogit, the dense weights and the dropout mask of block 6
  float dw[8] = {}, dl0 = 0.f, dl1 = 0.f;
  if constexpr (l == 5) {
    const float dsc = A.dropout ? Ly.dsc : 1.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) dw[j] = A.dense_w[c + j] * dsc;
    dl0 = A.dlogit[min(smp0, A.B - 1)] * (1.0f / kL);
    dl1 = A.dlogit[min(smp0 + 1, A.B - 1)] * (1.0f / kL);
  }
  auto valid = [&](int grow) {
    const int n = row_sample(grow), tt = row_time(grow);
    return !(grow < kHalo || n >= A.B || tt >= kL);
  };
#pragma unroll
  for (int b = 0; b < NK; b += U) {
    // payload: R_l (pre-BN activation) and dY_l, both loaded in the batched first phase
    bf16x16 q[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int r = rin + (b + u) * RP;
      const int grow = row0 + r;
      if (b + u >= NK) continue;
      const bool ok = active && r < NR && valid(grow);
      q[u].a = ok ? gld<bf16x8>(Ly.R + (long long)grow * Cc + c) : zero8();
      if constexpr (l < 5) q[u].b = ok ? gld<bf16x8>(Ly.dY + (long long)grow * Cc + c) : zero8();
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int r = rin + (b + u) * RP;
      if (b + u >= NK || !active || r >= NR) continue;
      const int grow = row0 + r;
      bf16x8 o = zero8();
      if (valid(grow)) {
        float dy[8];
        if constexpr (l == 5) {
          const bool hi = row_sample(grow) != smp0;
          const float dl = hi ? dl1 : dl0;
#pragma unroll
          for (int j = 0; j < 8; ++j) dy[j] = bf_dropped(q[u].a[j]) ? 0.f : dl * dw[j];
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) dy[j] = (float)q[u].b[j];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float rr = bf_abs(q[u].a[j]);
          const float dz = __builtin_fmaf(al[j], dy[j], __builtin_fmaf(be[j], rr, ga[j]));
          o[j] = (__bf16)(rr > 0.f ? dz : 0.f);
        }
      }
      *reinterpret_cast<bf16x8*>(lds + lds_off(r, cw * 16, ldsrs)) = o;
      if (gout != nullptr && r >= own_lo && r < own_hi)
        *reinterpret_cast<bf16x8*>(gout + (long long)grow * Cc + c) = o;  // pad rows get their zeros too
    }
  }
}

// dZ_l rows [row0, row0+NR) x channels [c0, c0+NCW*8) into LDS (wgrad; dgrad materialised them)
template <int l, int NR, int NCW, int UMAX, int NT = kThreads>
__device__ __forceinline__ void stage_dz_copy(const Args& A, char* lds, int ldsrs, int row0, int c0) {
  constexpr int Cc = C[l + 1];
  const Layer& Ly = A.L[l];
  staged_loop<NR * NCW, UMAX, NT>(
      [&](int i) -> bf16x8 {
        const int rc = i / NCW, cw = i - rc * NCW;
        return gld<bf16x8>(Ly.dZ + (long long)(row0 + rc) * Cc + c0 + cw * 8);
      },
      [&](int i, const bf16x8& o) {
        const int rc = i / NCW, cw = i - rc * NCW;
        *reinterpret_cast<bf16x8*>(lds + lds_off(rc, cw * 16, ldsrs)) = o;
      });
}

// Implicit-GEMM conv tile: D^T[co][row] over the 128-row tile, weights = packed A fragments.
template <int CIN, int COUT, int K, int WM, int WN, bool FIRST>
struct Conv {
  static constexpr int NSTEP = (CIN * K + 31) / 32;
  static constexpr int NCT = COUT / 16;
  static constexpr int CT = NCT / WN;
  static constexpr int RT = kRT / WM;
  static constexpr int PAD = (K - 1) / 2;
  static_assert(NCT % WN == 0 && kRT % WM == 0 && WM * WN == 4, "wave tiling");

  template <int PD = 1, bool RING = true>
  __device__ __forceinline__ static void run(const gbf16x8* wfrag, const char* lds, int ldsrs, f32x4 (&acc)[CT][RT]) {
#pragma unroll
    for (int c = 0; c < CT; ++c)
#pragma unroll
      for (int r = 0; r < RT; ++r) acc[c][r] = f32x4{0.f, 0.f, 0.f, 0.f};
    steps<0, NSTEP, PD, RING>(wfrag, lds, ldsrs, acc);
  }

  // steps [S0, S1) accumulated into acc; the wave's place in its 4-wave team is (threadIdx.x >> 6) & 3,
  // so 512-thread kernels run two teams.  PD = weight-fragment prefetch depth (k-steps in flight).
  template <int S0, int S1, int PD = 1, bool RING = true>
  __device__ __forceinline__ static void steps(const gbf16x8* wfrag, const char* lds, int ldsrs,
                                               f32x4 (&acc)[CT][RT]) {
    static_assert(S0 < S1 && PD >= 1, "step range");
    const int lane = threadIdx.x & 63, wave = (threadIdx.x >> 6) & 3;
    const int wm = wave / WN, wn = wave % WN;
    const int m = lane & 15, h = lane >> 4;
    const gbf16x8* wp = wfrag + (wn * CT) * 64 + lane;
    const int row0 = wm * RT * 16 + m;
    const char* bbase = lds + (kHalo + row0 - PAD) * ldsrs + 16 * h;
    auto load_b = [&](int s, int r) -> bf16x8 {
      if constexpr (FIRST) {
        const char* base = lds + (kHalo + row0 + r * 16 - PAD) * ldsrs + (32 * s + 8 * h) * 2;
        const bf16x4 lo = *reinterpret_cast<const bf16x4*>(base);
        const bf16x4 hi = *reinterpret_cast<const bf16x4*>(base + 8);
        return bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      } else {
        // lane base + uniform step offset + compile-time row-tile offset (see fused_forward.hip)
        constexpr int CB = CIN / 32;
        const int tap = s / CB, cb = s - tap * CB;
        const int soff = __builtin_amdgcn_readfirstlane(tap * ldsrs + cb * 64);
        return *reinterpret_cast<const bf16x8*>(bbase + soff + r * 16 * ldsrs);
      }
    };
    auto load_a = [&](int s, bf16x8 (&a)[CT]) {
#pragma unroll
      for (int c = 0; c < CT; ++c) a[c] = wp[(s * NCT + c) * 64];
    };
    // Weight fragments (A, from L2) run through a ring of PD + 1 stages: step s + PD's loads are issued
    // before step s's MFMAs (the fused kernel's scheme; see FwdPD for the measured depths).
    // B fragments (activations, LDS) run through a ring of NB registers over the (step, row tile)
    // sequence: the read of fragment i + NB is issued right after the CT MFMAs of fragment i, so
    // NB - 1 LDS reads stay in flight.  RING = false reads each B fragment just in time (dgrad: one
    // tile per workgroup, two workgroups per CU, measured 5-17 % faster per layer without the ring).
    constexpr int NSA = PD + 1;
    constexpr int NB = RT < 4 ? RT : 4;  // B-fragment ring depth (2 and 8 measured equal / slower)
    static_assert(RT % NB == 0, "B ring phase restarts at every step");
    constexpr int DSN = FIRST ? 2 : 1;  // LDS reads per B fragment
    bf16x8 bq[NB];
    if constexpr (RING) {
#pragma unroll
      for (int i = 0; i < NB; ++i) bq[i] = load_b(S0, i);
    }
    // step s at position j of its group (group base sb = s - j); tail: no refills past S1
    auto step = [&](int s, const bf16x8 (&a)[CT], int j, bool tail) {
      if constexpr (!RING) {
#pragma unroll
        for (int r = 0; r < RT; ++r) {
          const bf16x8 b = load_b(s, r);
#pragma unroll
          for (int c = 0; c < CT; ++c) acc[c][r] = mfma16(a[c], b, acc[c][r]);
        }
        return;
      }
#pragma unroll
      for (int r = 0; r < RT; ++r) {
        const int i = j * RT + r;
        const bf16x8 b = bq[i % NB];
#pragma unroll
        for (int c = 0; c < CT; ++c) acc[c][r] = mfma16(a[c], b, acc[c][r]);
        const int nx = i + NB;               // ring successor within the group
        const int sn = s - j + nx / RT;       // its step
        if (!tail || sn < S1) bq[i % NB] = load_b(sn < S1 ? sn : S1 - 1, nx % RT);  // clamped: unconditional
        __builtin_amdgcn_sched_group_barrier(0x008, CT, 0);   // the fragment's MFMAs ...
        __builtin_amdgcn_sched_group_barrier(0x100, DSN, 0);  // ... then its successor's read
      }
    };
    // unconditional (clamped) prefetch keeps hipcc's vmcnt accounting exact (see fused_forward.hip)
    bf16x8 a[NSA][CT];
#pragma unroll
    for (int j = 0; j < PD; ++j) load_a(S0 + j < S1 ? S0 + j : S1 - 1, a[j]);
    constexpr int NFULL = (S1 - S0) / NSA * NSA;
#pragma unroll 1
    for (int s0 = S0; s0 < S0 + NFULL; s0 += NSA) {
#pragma unroll
      for (int j = 0; j < NSA; ++j) {
        const int s = s0 + j;
        load_a(s + PD < S1 ? s + PD : S1 - 1, a[(j + PD) % NSA]);
        __builtin_amdgcn_sched_barrier(0);  // keep the prefetch ahead of this step's MFMAs
        step(s, a[j], j, false);
      }
    }
#pragma unroll
    for (int j = 0; j < (S1 - S0) - NFULL; ++j) step(S0 + NFULL + j, a[j], j, true);
  }
};

__device__ __forceinline__ bf16x8 tr_frag(const char* lds, int ldsrs, int row_base, int col0) {
  // fragment for a 16x16x32 operand whose K index is the LDS row, 32 rows from row_base.  Lane
  // group h (16 lanes) reads 4 rows x 16 cols per ds_read_b64_tr_b16; k-slot (h, j) of the fragment
  // holds row row_base + 4h + j (j < 4, first read) or row_base + 16 + 4h + j - 4 (second read).
  // Any k-permutation is exact as long as both operands use it, and this one makes each 32-lane
  // bank group read 8 CONSECUTIVE rows: with a row stride that is an odd multiple of 32 B they fall
  // on 8 distinct 8-bank groups, conflict-free for any row_base (the natural order, rows
  // r0..r0+3 and r0+8..r0+11, is 2-way for every stride: 37-42 % conflict cycles in round 1).
  const int lane = threadIdx.x & 63;
  const int h = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;
  const int ra = row_base + 4 * h + q;
  const char* a0 = lds + lds_off(ra, (col0 + 4 * p) * 2, ldsrs);
  const char* a1 = lds + lds_off(ra + 16, (col0 + 4 * p) * 2, ldsrs);
  const v4i16 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4i16*)a0);
  const v4i16 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4i16*)a1);
  // one 8 x 16-bit register quad: no per-element moves
  typedef short v8i16 __attribute__((ext_vector_type(8)));
  const v8i16 r = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(bf16x8, r);
}

extern __shared__ __attribute__((aligned(16))) char smem[];

// Reduce per-lane partial sums over the 16 rows of a lane group and add them to a global
// per-channel accumulator (fp32 atomics; one per channel per wave row-group).
__device__ __forceinline__ void atomic_channel_sums(double* dst, int co0, const f32x4& a, bool leader) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float v = group16_sum(a[i]);
    if (leader) atomicAdd(dst + co0 + i, (double)v);
  }
}

}  // namespace train
}  // namespace apneauq
