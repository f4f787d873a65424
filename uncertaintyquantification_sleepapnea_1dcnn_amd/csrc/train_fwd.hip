// Forward kernels of the layer-wise training path: R_l = relu(conv(A_{l-1}) + b) and its channel moments.
// See train_launch.hip for the design (layout, sign-bit mask, what is recomputed where) and train_geo.h for
// the launch geometry.
#include "train_launch.h"
#include "train_stage.h"

namespace apneauq {
namespace train {

// Weight-fragment prefetch depth of the forward conv (k-steps in flight): depth 1 everywhere 29.8 ms
// per 16-pass x 16384-window batch-BN chunk, depth 2 30.0, per-layer (1,3,2,3,2,3) 30.4, depth 4 38.7
// (spills) -- the conv is not bound by the L2 round trip of its weight fragments
// (profiles/batch_bn_fwd_r2.md).
constexpr int kFwdPD = 1;

// ------------------------------------------------------------------------------------------------
// Forward of block l:  R_l = relu(conv(A_{l-1}) + b), fwd sums of R_l per stats group.
// ------------------------------------------------------------------------------------------------
template <int l, bool MB, bool PFT = false>
__global__ __launch_bounds__(kThreads, 2) void fwd_kernel(Args A_, const Args* __restrict__ Am) {
  const MbPos pos = mb_pos<MB>();
  const Args& A = member_args<MB>(A_, Am, pos);
  constexpr int CIN = C[l], COUT = C[l + 1];
  using T = Tiling<COUT>;
  using CV = Conv<CIN, COUT, KS[l], T::WM, T::WN, l == 0>;
  char* act = smem;                                  // staged input, then staged output
  float* prm = reinterpret_cast<float*>(smem + kRows * kRS);  // [s 512 | t 512]
  constexpr int IN_RS = (l == 0) ? 8 : kRS;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = wave / T::WN, wn = wave % T::WN;
  const int m = lane & 15, h = lane >> 4;
  const Layer& Ly = A.L[l];
  // Each workgroup owns a contiguous range of tiles (so the stats group changes rarely).  The channel
  // moments of a stored tile come from the matrix cores: per 16-channel tile ct, sum_rows r^2 is the
  // diagonal of R_ct^T R_ct and sum_rows r is ones^T R_ct, 8 MFMAs over the 128 rows on operands read
  // with ds_read_b64_tr_b16 (no per-element VALU: the layer kernels are VALU-issue bound).  The lanes
  // holding a diagonal keep fp32 partials across the run of tiles of one stats group, merged (LDS
  // atomics, then fp64 global slots) only when the group changes.
  const int tiles = (A.B + 1) / 2;
  const int tpw = (tiles + gridDim.x - 1) / gridDim.x;
  const int t_begin = pos.bx * tpw;
  const int t_end = min(tiles, t_begin + tpw);
  float* lstat = prm + 1024;  // [2][COUT]: sum r, sum r^2 of the current group run
  for (int c = threadIdx.x; c < 2 * COUT; c += kThreads) lstat[c] = 0.f;
  int gcur = -1;
  double* st = Ly.st + (pos.bx % kStatSlots) * st_stride(A, COUT);
  constexpr int CW = COUT / 8;             // 16-B chunks per output row
  constexpr int RPo = kThreads / CW;       // rows per copy-out pass
  // copy-out rows: the tile's 2 x 60 valid time steps only (the R buffers are allocated filled with
  // -0.0 and their pad rows are never written)
  constexpr int kOutRows = kSlots * kL;
  constexpr int NPo = (kOutRows + RPo - 1) / RPo;
  const int ocw = threadIdx.x % CW, orin = threadIdx.x / CW;
  const bool oact = orin < RPo;
  constexpr int NCTo = COUT / 16, CPW = (NCTo + 3) / 4;  // moment channel tiles: ct = wave + 4j
  const int sn = lane & 15;
  const bool diag_lane = (lane >> 4) == (sn >> 2);        // holds D[sn][sn] of a 16x16 tile
  float ps1[CPW], ps2[CPW];
#pragma unroll
  for (int j = 0; j < CPW; ++j) ps1[j] = ps2[j] = 0.f;
  auto flush = [&]() {  // workgroup-uniform: fp32 run partials (<= ~10^4 rows / lane) merged in fp64
    if (gcur >= 0 && diag_lane) {
#pragma unroll
      for (int j = 0; j < CPW; ++j) {
        const int ct = wave + 4 * j;
        if (ct < NCTo) {
          atomicAdd(&lstat[ct * 16 + sn], ps1[j]);
          atomicAdd(&lstat[COUT + ct * 16 + sn], ps2[j]);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < CPW; ++j) ps1[j] = ps2[j] = 0.f;
    __syncthreads();
    if (gcur >= 0 && A.det == nullptr) {
      for (int c = threadIdx.x; c < COUT; c += kThreads) {
        atomicAdd(st + (gcur * 2 + 0) * COUT + c, (double)lstat[c]);
        atomicAdd(st + (gcur * 2 + 1) * COUT + c, (double)lstat[COUT + c]);
        lstat[c] = lstat[COUT + c] = 0.f;
      }
    }
    __syncthreads();
  };
  // this block's dropout mask goes into the sign bit of R_l (not for the pass-shared block 1)
  const bool enc = A.dropout != 0 && !(l == 0 && A.shared0);
  const bool hash_in = l == 1 && A.shared0;  // workgroup-uniform
  int gaff = -1;  // stats group whose BN affine (of block l-1) is in prm
  // input staging: loads of a tile's rows, then A = dropout(BN(R)) decoded into LDS
  ActStager<(l > 0 ? l - 1 : 0), l == 1> stg;
  constexpr int NPF = !PFT || l == 0 || FwdStageSplit<l>::v ? 0
                      : (FwdPF<l>::v < decltype(stg)::NK ? FwdPF<l>::v : decltype(stg)::NK);
  if constexpr (NPF > 0) {
    if (t_begin < t_end) stg.template load<0, NPF>(A, kR * t_begin, hash_in);
  }
  for (int tile = t_begin; tile < t_end; ++tile) {
    APNEAUQ_DASSERT(2 * tile < A.B + 1 && blockDim.x == kThreads);
    const int row0 = kR * tile;                        // first staged row (global PL index)
    const int smp0 = 2 * tile;
    const int g0 = min(smp0, A.B - 1) / A.n_win, g1 = min(smp0 + 1, A.B - 1) / A.n_win;
    __syncthreads();  // previous tile's copy-out has read the LDS tile
    if constexpr (l == 0) {
      staged_loop<kRows * 8 / 16>(
          [&](int i) -> bf16x8 { return gld<bf16x8>(A.x + (long long)row0 * 4 + i * 8); },
          [&](int i, const bf16x8& v) { reinterpret_cast<bf16x8*>(act)[i] = v; });
    } else {
      if (g0 != gaff || g1 != g0) {  // (re)load the affine of block l-1 for this tile's group(s)
        bn_affine_to_lds(A, l - 1, g0, prm, prm + 512, nullptr, nullptr);
        if (g1 != g0) bn_affine_to_lds(A, l - 1, g1, prm + 256, prm + 768, nullptr, nullptr);
        gaff = (g1 == g0) ? g0 : -1;
        __syncthreads();
      }
      if constexpr (FwdStageSplit<l>::v) {  // two row batches: fewer loads in flight, no spills
        constexpr int NK = decltype(stg)::NK, H = (NK + 1) / 2;
        stg.template load<0, H>(A, row0, hash_in);
        stg.template store<0, H>(A, act, row0, prm, prm + 512, g0, hash_in);
        stg.template load<H, NK>(A, row0, hash_in);
        stg.template store<H, NK>(A, act, row0, prm, prm + 512, g0, hash_in);
      } else if constexpr (NPF > 0) {  // items [0, NPF) were loaded during the previous tile's conv
        stg.template load<NPF, decltype(stg)::NK>(A, row0, hash_in);
        stg.store(A, act, row0, prm, prm + 512, g0, hash_in);
      } else {
        stg.load(A, row0, hash_in);
        stg.store(A, act, row0, prm, prm + 512, g0, hash_in);
      }
    }
    __syncthreads();
    if constexpr (NPF > 0) {
      if (tile + 1 < t_end) stg.template load<0, NPF>(A, kR * (tile + 1), hash_in);
    }
    // epilogue of one 16 x 16 accumulator tile: bias + ReLU -> bf16 LDS tile (rows outside the batch /
    // pad rows: 0).  Only the row tiles holding t = 48..63 (pad rows on lanes m >= 12) and the batch's
    // last tile need the select.
    const bool last_tile = smp0 + 1 >= A.B;  // workgroup-uniform
    auto epi = [&](const f32x4& a4, int co0, int rtg, const f32x4& bias) {
      const int row = rtg * 16 + m;  // 0..127 within the tile (rtg wave-uniform)
      f32x4 v;
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = fmaxf(a4[i] + bias[i], 0.f);
      if ((rtg & 3) == 3 || last_tile) {
        const bool valid = (row & 63) < kL && (smp0 + (row >> 6)) < A.B;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          v[i] = valid ? v[i] : 0.f;
          asm volatile("" : "+v"(v[i]));  // keep the select in fp32 (no per-element cvt + v_perm repack)
        }
      }
      bf16x4 o = {(__bf16)v[0], (__bf16)v[1], (__bf16)v[2], (__bf16)v[3]};
      *reinterpret_cast<bf16x4*>(act + row * kRS + co0 * 2) = o;
    };
    f32x4 acc[CV::CT][CV::RT];
    if constexpr (kFwdPrio) __builtin_amdgcn_s_setprio(1);
    CV::template run<kFwdPD, true>(Ly.wf, act, IN_RS, acc);
    if constexpr (kFwdPrio) __builtin_amdgcn_s_setprio(0);
    __syncthreads();  // all waves done reading the staged input; reuse it for the output tile
#pragma unroll
    for (int c = 0; c < CV::CT; ++c) {
      const int co0 = (wn * CV::CT + c) * 16 + 4 * h;
      const f32x4 bias = gld<f32x4>(Ly.bias + co0);
#pragma unroll
      for (int r = 0; r < CV::RT; ++r) epi(acc[c][r], co0, wm * CV::RT + r, bias);
    }
    __syncthreads();
    // channel moments of the stored tile (zero rows add nothing) on the matrix cores
    auto moments = [&](int sel) {  // sel: sample slot (rows 64*sel .. +64 = 32-row chunks 2sel, 2sel+1), -1: both
      {
        bf16x8 ones;
#pragma unroll
        for (int j = 0; j < 8; ++j) ones[j] = (__bf16)1.f;
        const int si = sn & 3;
#pragma unroll
        for (int j = 0; j < CPW; ++j) {
          const int ct = wave + 4 * j;
          if (ct >= NCTo) break;  // wave-uniform
          f32x4 g = {0.f, 0.f, 0.f, 0.f}, sm = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int kc = 0; kc < kR / 32; ++kc) {
            if (sel >= 0 && (kc >> 1) != sel) continue;
            const bf16x8 f = tr_frag(act, kRS, kc * 32, ct * 16);
            g = mfma16(f, f, g);       // R^T R
            sm = mfma16(ones, f, sm);  // ones^T R
          }
          const float dg = si == 0 ? g[0] : si == 1 ? g[1] : si == 2 ? g[2] : g[3];
          const float s1v = si == 0 ? sm[0] : si == 1 ? sm[1] : si == 2 ? sm[2] : sm[3];
          ps1[j] += s1v;
          ps2[j] += dg;
        }
      }
    };
    // coalesced copy-out of the 128 tile rows (16 B per thread-iteration) with this block's dropout
    // mask in the sign bits (drawn here, where no accumulators are live)
    unsigned key[kSlots] = {0u, 0u};
    if (enc) {
      key[0] = layer_sample_key(A, l, min(smp0, A.B - 1));
      key[1] = layer_sample_key(A, l, min(smp0 + 1, A.B - 1));
    }
    const uint32_t thr2 = Ly.thr * 0x10001u;
    auto copy_out = [&]() {
      // opaque row index (see staged_loop): keeps the NPo per-row addresses out of the tile loop
      int rin = orin;
      asm volatile("" : "+v"(rin));
#pragma unroll 2
      for (int k = 0; k < NPo; ++k) {
        const int rc = rin + k * RPo;
        if (!oact || rc >= kOutRows) continue;
        const int slot = rc >= kL, tt = rc - kL * slot;
        const int r = slot * kSR + tt;
        bf16x8 o = *reinterpret_cast<const bf16x8*>(act + r * kRS + ocw * 16);
        uint32_t* ow = reinterpret_cast<uint32_t*>(&o);
        if (!(tt < kL && smp0 + slot < A.B)) {  // pad / out-of-batch rows: -0.0, decoded as A = 0
#pragma unroll
          for (int q = 0; q < 4; ++q) ow[q] = kNegZero2;
        } else if (enc) {
#pragma unroll
          for (int q = 0; q < 4; ++q) ow[q] |= drop_signs2(dropout_bits2(key[slot], tt, ocw * 8 + 2 * q), thr2);
        }
        *reinterpret_cast<bf16x8*>(Ly.R + (long long)(row0 + kHalo + r) * COUT + ocw * 8) = o;
      }
    };
    if (g0 == g1) {
      if (g0 != gcur) {
        flush();
        gcur = g0;
      }
      moments(-1);
    } else {  // a tile straddling two stats groups (MC-Dropout pass boundary): moments per slot
      flush();
      gcur = g0;
      moments(0);
      flush();
      gcur = g1;
      moments(1);
    }
    copy_out();
  }
  flush();
  if (A.det != nullptr) {  // deterministic mode (one stats group): this workgroup's moment partials
    float* dp = A.det + (long long)pos.bx * 2 * COUT;
    for (int c = threadIdx.x; c < 2 * COUT; c += kThreads) dp[c] = lstat[c];
  }
}

// ------------------------------------------------------------------------------------------------ host
template <bool MB>
static hipError_t fwd_launch_t(const Args& A, const Args* Am, int M, int l, int grid, bool pf, hipStream_t st) {
  const dim3 g(grid, 1, M);
  switch (l) {
    case 0: hipLaunchKernelGGL(HIP_KERNEL_NAME(fwd_kernel<0, MB>), g, dim3(256), lds_fwd(), st, A, Am); break;
    case 1:
      if (pf)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(fwd_kernel<1, MB, true>), g, dim3(256), lds_fwd(), st, A, Am);
      else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(fwd_kernel<1, MB>), g, dim3(256), lds_fwd(), st, A, Am);
      break;
    case 2: hipLaunchKernelGGL(HIP_KERNEL_NAME(fwd_kernel<2, MB>), g, dim3(256), lds_fwd(), st, A, Am); break;
    case 3:
      if (pf)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(fwd_kernel<3, MB, true>), g, dim3(256), lds_fwd(), st, A, Am);
      else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(fwd_kernel<3, MB>), g, dim3(256), lds_fwd(), st, A, Am);
      break;
    case 4: hipLaunchKernelGGL(HIP_KERNEL_NAME(fwd_kernel<4, MB>), g, dim3(256), lds_fwd(), st, A, Am); break;
    case 5: hipLaunchKernelGGL(HIP_KERNEL_NAME(fwd_kernel<5, MB>), g, dim3(256), lds_fwd(), st, A, Am); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t fwd_launch(const Args& A, const Args* Am, int M, int l, bool pf, hipStream_t st) {
  const int grid = fwd_launch_grid(A.B, M, pf);
  return Am != nullptr ? fwd_launch_t<true>(A, Am, M, l, grid, pf, st) : fwd_launch_t<false>(A, nullptr, 1, l, grid, pf, st);
}

}  // namespace train
}  // namespace apneauq
