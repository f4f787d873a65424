// dgrad kernels of the layer-wise training path: dY_{l-1} and the backward sums of block l-1.
// See train_launch.hip for the design (layout, sign-bit mask, what is recomputed where) and train_geo.h for
// the launch geometry.
#include "train_launch.h"
#include "train_stage.h"

namespace apneauq {
namespace train {

// ------------------------------------------------------------------------------------------------
// dgrad of block l (l >= 1): dA_{l-1} = conv^T(dZ_l, W_l);  epilogue -> dY_{l-1} = dA * mask_{l-1}
// plus the backward sums of block l-1.
// ------------------------------------------------------------------------------------------------
// stage_dz for dgrad (all CIN channels of 136 rows, dZ_l also written to global for wgrad) split into
// load() (the prefetched items, into registers) and store() (every item: the prefetched ones from
// registers, the rest loaded in batches there), so the next tile's loads can overlap this tile's conv.
template <int l, int NPF>
struct DzStager {
  static constexpr int Cc = C[l + 1], NCW = Cc / 8, RP = kThreads / NCW, NR = kRows;
  static constexpr int NK = (NR + RP - 1) / RP;
  static constexpr int NP = NPF < NK ? NPF : NK;
  static constexpr int U = kStageU;
  bf16x8 r[NP > 0 ? NP : 1];
  bf16x8 d[(NP > 0 && l < 5) ? NP : 1];

  __device__ __forceinline__ static int tid() {
    int t = threadIdx.x;
    asm volatile("" : "+v"(t));
    return t;
  }
  __device__ __forceinline__ static bool valid(const Args& A, int grow) {
    const int n = row_sample(grow), tt = row_time(grow);
    return !(grow < kHalo || n >= A.B || tt >= kL);
  }
  __device__ __forceinline__ void load(const Args& A, int row0) {
    const int t = tid(), cw = t % NCW, rin = t / NCW;
    const bool active = rin < RP;
    const Layer& Ly = A.L[l];
#pragma unroll
    for (int u = 0; u < NP; ++u) {
      const int rc = rin + u * RP, grow = row0 + rc;
      const bool ok = active && rc < NR && valid(A, grow);
      r[u] = ok ? gld<bf16x8>(Ly.R + (long long)grow * Cc + cw * 8) : zero8();
      if constexpr (l < 5) d[u] = ok ? gld<bf16x8>(Ly.dY + (long long)grow * Cc + cw * 8) : zero8();
    }
  }
  // dz = relu'(r) * (al * dy + be * r + ga) per element (see stage_dz); rows [kHalo, kHalo + kR) to dZ_l too
  __device__ __forceinline__ void store(const Args& A, char* lds, int row0, const float* gam_rstd, const float* mean,
                                        const float* rstd, const float* mdy, const float* mdyx) const {
    const int t = tid(), cw = t % NCW, rin = t / NCW;
    if (rin >= RP) return;
    const Layer& Ly = A.L[l];
    const int c = cw * 8;
    const int smp0 = (row0 >> 7) * 2;
    float al[8], be[8], ga[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float g = gam_rstd[c + j], q = rstd[c + j] * mdyx[c + j];
      al[j] = g;
      be[j] = -g * q;
      ga[j] = g * (q * mean[c + j] - mdy[c + j]);
    }
    float dw[8] = {}, dl0 = 0.f, dl1 = 0.f;
    if constexpr (l == 5) {
      const float dsc = A.dropout ? Ly.dsc : 1.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) dw[j] = A.dense_w[c + j] * dsc;
      dl0 = A.dlogit[min(smp0, A.B - 1)] * (1.0f / kL);
      dl1 = A.dlogit[min(smp0 + 1, A.B - 1)] * (1.0f / kL);
    }
    auto emit = [&](int rc, const bf16x8& rv, const bf16x8& dv) {
      const int grow = row0 + rc;
      bf16x8 o = zero8();
      if (valid(A, grow)) {
        float dy[8];
        if constexpr (l == 5) {
          const float dl = row_sample(grow) != smp0 ? dl1 : dl0;
#pragma unroll
          for (int j = 0; j < 8; ++j) dy[j] = bf_dropped(rv[j]) ? 0.f : dl * dw[j];
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) dy[j] = (float)dv[j];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float rr = bf_abs(rv[j]);
          const float dz = __builtin_fmaf(al[j], dy[j], __builtin_fmaf(be[j], rr, ga[j]));
          o[j] = (__bf16)(rr > 0.f ? dz : 0.f);
        }
      }
      *reinterpret_cast<bf16x8*>(lds + lds_off(rc, cw * 16, kRS)) = o;
      if (rc >= kHalo && rc < kHalo + kR)
        *reinterpret_cast<bf16x8*>(Ly.dZ + (long long)grow * Cc + c) = o;  // pad rows get their zeros too
    };
#pragma unroll
    for (int u = 0; u < NP; ++u) {
      const int rc = rin + u * RP;
      if (rc >= NR) continue;
      if constexpr (l < 5)
        emit(rc, r[u], d[u]);
      else
        emit(rc, r[u], r[u]);  // block 6: dY recomputed, no payload
    }
#pragma unroll
    for (int b = NP; b < NK; b += U) {
      bf16x8 qr[U], qd[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int rc = rin + (b + u) * RP, grow = row0 + rc;
        if (b + u >= NK) continue;
        const bool ok = rc < NR && valid(A, grow);
        qr[u] = ok ? gld<bf16x8>(Ly.R + (long long)grow * Cc + c) : zero8();
        if constexpr (l < 5) qd[u] = ok ? gld<bf16x8>(Ly.dY + (long long)grow * Cc + c) : zero8();
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int rc = rin + (b + u) * RP;
        if (b + u >= NK || rc >= NR) continue;
        if constexpr (l < 5)
          emit(rc, qr[u], qd[u]);
        else
          emit(rc, qr[u], qr[u]);
      }
    }
  }
};

template <int l, bool MB>
__global__ __launch_bounds__(kThreads, 2) void dgrad_kernel(Args A_, const Args* __restrict__ Am, RedJob rj) {
  const MbPos pos = mb_pos<MB>();
  const Args& A = member_args<MB>(A_, Am, pos);
  constexpr int CIN = C[l + 1], COUT = C[l];  // conv^T: input = dZ_l channels, output = block l-1 channels
  using T = Tiling<COUT>;
  using CV = Conv<CIN, COUT, KS[l], T::WM, T::WN, false>;
  // LDS: the staged tile + 7 x 256 per-channel floats = 79.25 KiB, so TWO workgroups fit per CU
  // (with the previous 9 x 256 floats it was 81.25 KiB and dgrad ran one workgroup per CU)
  char* act = smem;
  float* prm = reinterpret_cast<float*>(smem + kRows * kRS);
  float* gr = prm;           // gamma*rstd of block l
  float* mean = prm + 256;
  float* rstd = prm + 512;
  float* mdy = prm + 768;
  float* mdyx = prm + 1024;
  float* mean_prev = prm + 1280;  // block l-1 mean / rstd for xhat
  float* rstd_prev = prm + 1536;
  const int ntiles = (A.B + 1) / 2;
  APNEAUQ_DASSERT(blockDim.x == kThreads);
  if (A.tab != nullptr) {  // single-device training: T[l] (block 6: backward sums), T[l-1]
    const int c = threadIdx.x;
    if (c < CIN) {
      gr[c] = tab_row(A, l, kTabS)[c];
      mean[c] = tab_row(A, l, kTabMean)[c];
      rstd[c] = tab_row(A, l, kTabRstd)[c];
      if (l == 5 || A.bwd_self) {  // block 6's backward sums come from the head, no table job in between
        mdy[c] = (float)(slot_sumd(A.L[l].bst + c, 2 * CIN) * A.inv_count);
        mdyx[c] = (float)(slot_sumd(A.L[l].bst + CIN + c, 2 * CIN) * A.inv_count);
      } else {
        mdy[c] = tab_row(A, l, kTabMdy)[c];
        mdyx[c] = tab_row(A, l, kTabMdyx)[c];
      }
    }
    if (c < COUT) {
      mean_prev[c] = tab_row(A, l - 1, kTabMean)[c];
      rstd_prev[c] = tab_row(A, l - 1, kTabRstd)[c];
    }
  } else {
    // one channel per thread (CIN, COUT <= 256 = kThreads): block l's moments and backward sums and
    // block l-1's moments, all 96 slot loads independent (clamped indices, stores predicated)
    static_assert(CIN <= kThreads && COUT <= kThreads, "one channel per thread");
    const Layer& Ly = A.L[l];
    const int c = threadIdx.x, ci = c < CIN ? c : 0, cp = c < COUT ? c : 0;
    float mu, var, mup, varp;
    bn_moments(A, l, 0, ci, mu, var);
    const double b0 = slot_sumd(Ly.bst + ci, 2 * CIN), b1 = slot_sumd(Ly.bst + CIN + ci, 2 * CIN);
    bn_moments(A, l - 1, 0, cp, mup, varp);
    if (c < CIN) {
      const float rs = rsqrtf(var + A.eps);
      mean[c] = mu;
      rstd[c] = rs;
      gr[c] = Ly.gamma[c] * rs;
      mdy[c] = (float)(b0 * A.inv_count);
      mdyx[c] = (float)(b1 * A.inv_count);
    }
    if (c < COUT) {
      mean_prev[c] = mup;
      rstd_prev[c] = rsqrtf(varp + A.eps);
    }
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = wave / T::WN, wn = wave % T::WN;
  const int m = lane & 15, h = lane >> 4;
  const Layer& Lp = A.L[l - 1];
  DzStager<l, DgPF<l>::v> stager;
  if (DgPF<l>::v > 0 && pos.bx < ntiles) stager.load(A, kR * pos.bx);
  // blocks without a prefetch keep one tile per workgroup (a constant one-trip loop: the persistent form
  // keeps more values live and spilled block 4's dgrad)
  constexpr bool PERSIST = DgPF<l>::v > 0;
  for (int tile = pos.bx, it = 0; PERSIST ? tile < ntiles : it < 1; tile += gridDim.x, ++it) {
  const int row0 = kR * tile;
  const int smp0 = 2 * tile;
  stager.store(A, act, row0, gr, mean, rstd, mdy, mdyx);
  __syncthreads();
  // R_{l-1} at this lane's epilogue elements (|R| for xhat, sign = block l-1's dropout mask), loaded
  // before the conv so the MFMAs cover their latency (DgPre: where the registers allow)
  constexpr bool PRE = DgPre<l>::v;
  bf16x4 rpre[PRE ? CV::CT : 1][PRE ? CV::RT : 1];
  if constexpr (PRE) {
#pragma unroll
    for (int c = 0; c < CV::CT; ++c)
#pragma unroll
      for (int r = 0; r < CV::RT; ++r) {
        const int row = wm * CV::RT * 16 + r * 16 + m;
        const bool valid = (row & 63) < kL && (smp0 + (row >> 6)) < A.B;
        const int co0 = (wn * CV::CT + c) * 16 + 4 * h;
        rpre[c][r] = valid ? gld<bf16x4>(Lp.R + (long long)(row0 + kHalo + row) * COUT + co0)
                           : bf16x4{(__bf16)0.f, (__bf16)0.f, (__bf16)0.f, (__bf16)0.f};
      }
  }
  if constexpr (DgPF<l>::v > 0) {
    if (tile + (int)gridDim.x < ntiles) stager.load(A, kR * (tile + gridDim.x));  // in flight during the conv
  }
  f32x4 acc[CV::CT][CV::RT];
  CV::template run<DgPD<l>::v, false>(A.L[l].wd, act, kRS, acc);  // (B ring at batch 8192: -0.6 %, batch 1024: +-0)
  __syncthreads();
  const float dscp = A.dropout ? Lp.dsc : 1.f;
#pragma unroll
  for (int c = 0; c < CV::CT; ++c) {
    const int co0 = (wn * CV::CT + c) * 16 + 4 * h;
    f32x4 b0 = {}, b1 = {};
#pragma unroll
    for (int r = 0; r < CV::RT; ++r) {
      const int row = wm * CV::RT * 16 + r * 16 + m;
      const int slot = row >> 6, tt = row & 63;
      const bool valid = tt < kL && (smp0 + slot) < A.B;
      // R_{l-1}: |R| for xhat, its sign bit = the dropout mask of block l-1
      bf16x4 rr = {(__bf16)0.f, (__bf16)0.f, (__bf16)0.f, (__bf16)0.f};
      if constexpr (PRE)
        rr = rpre[c][r];
      else if (valid)
        rr = gld<bf16x4>(Lp.R + (long long)(row0 + kHalo + row) * COUT + co0);
      f32x4 v = acc[c][r];
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = (!valid || bf_dropped(rr[i])) ? 0.f : v[i] * dscp;
      bf16x4 o = {(__bf16)v[0], (__bf16)v[1], (__bf16)v[2], (__bf16)v[3]};
      *reinterpret_cast<bf16x4*>(act + row * kRS + co0 * 2) = o;
      if (valid) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float q = (float)o[i];
          const float xh = (bf_abs(rr[i]) - mean_prev[co0 + i]) * rstd_prev[co0 + i];
          b0[i] += q;
          b1[i] += q * xh;
        }
      }
    }
    if (A.det != nullptr) {  // deterministic mode: this wave's row-block partial, reduced in order later
      float* dp = A.det + (long long)(tile * T::WM + wm) * 2 * COUT;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float s0 = group16_sum(b0[i]), s1 = group16_sum(b1[i]);
        if (m == 0) {
          dp[co0 + i] = s0;
          dp[COUT + co0 + i] = s1;
        }
      }
    } else {
      double* bst = Lp.bst + (tile % kStatSlots) * 2 * COUT;
      atomic_channel_sums(bst, co0, b0, m == 0);
      atomic_channel_sums(bst + COUT, co0, b1, m == 0);
    }
  }
  __syncthreads();
  constexpr int CW = COUT / 8;
  for (int i = threadIdx.x; i < kR * CW; i += kThreads) {
    const int r = i / CW, cw = i - r * CW;
    *reinterpret_cast<bf16x8*>(Lp.dY + (long long)(row0 + kHalo + r) * COUT + cw * 8) =
        *reinterpret_cast<const bf16x8*>(act + r * kRS + cw * 16);
  }
  __syncthreads();  // the next tile's staging overwrites act
  }
  // fused step (single device): wgrad<l+1>'s partials, which ran just before this launch, reduced by the
  // workgroups as they finish their tiles -- the separate reduce launch's ramp and drain are gone
  if (rj.part != nullptr) wgrad_reduce_cols(rj, pos.bx, gridDim.x, reinterpret_cast<f32x4*>(smem));
}

// ------------------------------------------------------------------------------------------------ host
template <bool MB>
static hipError_t dgrad_launch_t(const Args& A, const Args* Am, int M, int l, const RedJob& rj, hipStream_t st) {
  const dim3 g(dg_grid(A.B, M, l), 1, M);
  switch (l) {
    case 1: hipLaunchKernelGGL(HIP_KERNEL_NAME(dgrad_kernel<1, MB>), g, dim3(256), lds_dgrad(), st, A, Am, rj); break;
    case 2: hipLaunchKernelGGL(HIP_KERNEL_NAME(dgrad_kernel<2, MB>), g, dim3(256), lds_dgrad(), st, A, Am, rj); break;
    case 3: hipLaunchKernelGGL(HIP_KERNEL_NAME(dgrad_kernel<3, MB>), g, dim3(256), lds_dgrad(), st, A, Am, rj); break;
    case 4: hipLaunchKernelGGL(HIP_KERNEL_NAME(dgrad_kernel<4, MB>), g, dim3(256), lds_dgrad(), st, A, Am, rj); break;
    case 5: hipLaunchKernelGGL(HIP_KERNEL_NAME(dgrad_kernel<5, MB>), g, dim3(256), lds_dgrad(), st, A, Am, rj); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t dgrad_launch(const Args& A, const Args* Am, int M, int l, const RedJob& rj, hipStream_t st) {
  return Am != nullptr ? dgrad_launch_t<true>(A, Am, M, l, rj, st) : dgrad_launch_t<false>(A, nullptr, 1, l, rj, st);
}

}  // namespace train
}  // namespace apneauq
