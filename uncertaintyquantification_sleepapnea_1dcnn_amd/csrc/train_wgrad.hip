// wgrad kernels of the layer-wise training path: per-row-group partials of dW_l, db_l.
// See train_launch.hip for the design (layout, sign-bit mask, what is recomputed where) and train_geo.h for
// the launch geometry.
#include "train_launch.h"
#include "train_stage.h"

namespace apneauq {
namespace train {

// ------------------------------------------------------------------------------------------------
// wgrad of block l: dW_l[tap][ci][co] = sum_rows A_{l-1}[row + tap - pad][ci] * dZ_l[row][co],
// db_l = sum_rows dZ_l.  MFMA: D[co][ci] (16x16 tiles), A-op = dZ^T, B-op = A^shift; both read
// with ds_read_b64_tr_b16 from row-major LDS tiles.  Block 1 stages an im2col (kk = tap*4+ci).
// ------------------------------------------------------------------------------------------------
// launch extras of a single-device fused step: the partial region's offset (wgrad<0> writes behind the
// region wgrad<1> leaves for step_reduce_kernel) and the table job (tb.bst == nullptr: none)
struct WgExt {
  long long part_off;
  TabBwd tb;
};

template <int l, bool MB>
__global__ __launch_bounds__(WgCfg<l>::WAVES * 64, WgCfg<l>::MINB) void wgrad_kernel(Args A_, const Args* __restrict__ Am,
                                                                                     WgExt ext) {
  const MbPos pos = mb_pos<MB>();
  const Args& A = member_args<MB>(A_, Am, pos);
  // fused step: the table's backward rows of block l-1 (bst[l-1] is complete: dgrad<l> ran before) for
  // dgrad<l-1> / wgrad<l-1>, the job of the separate reduce launch's extra workgroup
  if (ext.tb.bst != nullptr && blockIdx.x == 0) tab_bwd_rows(ext.tb);
  using W = WgCfg<l>;
  constexpr int NT = W::WAVES * 64;
  constexpr int CIN = C[l], COUT = C[l + 1], K = KS[l], PAD = (K - 1) / 2;
  constexpr bool FIRST = (l == 0);
  constexpr int NTAP = FIRST ? 1 : K;           // block 1: taps folded into the im2col columns
  constexpr int NCO = W::COB / 16 / W::WCO;     // co tiles per wave
  constexpr int NCI = W::CIB / 16 / W::WCI;     // ci tiles per wave
  constexpr int DZRS = wg_rs(W::COB * 2);       // LDS row strides (bytes): odd multiples of 32 B
  constexpr int ARS = wg_rs(FIRST ? 64 : W::CIB * 2);
  static_assert(W::WCO * W::WCI == W::WAVES && (W::WAVES == 4 || !(l == 0)), "one output sub-block per wave");
  static_assert((FIRST || CIN % W::CIB == 0) && COUT % W::COB == 0 && W::CIB % (16 * W::WCI) == 0 &&
                    W::COB % (16 * W::WCO) == 0,
                "wgrad blocks must tile Cin x Cout exactly (e.g. CIB 64 on Cin 224 dropped channels)");
  char* dz_lds = smem;                                   // 128 rows x COB
  char* a_lds = smem + kR * DZRS;                        // 136 rows x CIB (or 128 x 32 im2col)
  float* prm = reinterpret_cast<float*>(a_lds + kRows * ARS);
  float* gr = prm;
  float* mean = prm + 256;
  float* rstd = prm + 512;
  float* mdy = prm + 768;
  float* mdyx = prm + 1024;
  float* sp = prm + 1280;   // block l-1 affine (scale | shift) for staging A_{l-1}
  float* tp = prm + 1536;
  const int nci_blk = FIRST ? 1 : CIN / W::CIB;
  const int nco_blk = COUT / W::COB;
  // XCD-aware remap: hardware dispatch round-robins blockIdx over the 8 XCDs, so the nci*nco
  // workgroups of one row group (which stage the same dZ / A rows) would land on 8 different L2s
  // and each re-read the rows from HBM.  Contiguous logical ids per XCD keep a row group's blocks
  // on one XCD, running together, so its rows come from HBM once.  This is xcd_order(pos.bx, gridDim.x,
  // pos.nxcd) of xcd_order.h written out (member-batched: the same remap over the XCDs the member spans);
  // calling the helper here swaps the operands of one scalar add in six kernels, so the text stays until
  // these kernels change for another reason (profiles/shared_device_helpers.md).
  const int nwg = gridDim.x, bid = pos.bx, nx = pos.nxcd;
  const int xq = nwg / nx, xr = nwg % nx, xcd = bid % nx;
  const int wg = (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + bid / nx;
  const int blk = wg % (nci_blk * nco_blk);
  const int rg = wg / (nci_blk * nco_blk);
  const int ci0 = (blk % nci_blk) * W::CIB, co0 = (blk / nci_blk) * W::COB;
  const bool do_bias = (ci0 == 0);
  if (A.tab != nullptr) {  // single-device training: T[l] (block 6: backward sums), T[l-1]
    const int c = threadIdx.x;
    if (c < COUT) {
      gr[c] = tab_row(A, l, kTabS)[c];
      mean[c] = tab_row(A, l, kTabMean)[c];
      rstd[c] = tab_row(A, l, kTabRstd)[c];
      if (l == 5 || A.bwd_self) {
        mdy[c] = (float)(slot_sumd(A.L[l].bst + c, 2 * COUT) * A.inv_count);
        mdyx[c] = (float)(slot_sumd(A.L[l].bst + COUT + c, 2 * COUT) * A.inv_count);
      } else {
        mdy[c] = tab_row(A, l, kTabMdy)[c];
        mdyx[c] = tab_row(A, l, kTabMdyx)[c];
      }
    }
    if constexpr (!FIRST) {
      if (c < CIN) {
        sp[c] = tab_row(A, l - 1, kTabS)[c];
        tp[c] = tab_row(A, l - 1, kTabT)[c];
      }
    }
  } else {
    // one channel per thread, every slot load independent (see dgrad_kernel's prologue)
    static_assert(COUT <= kThreads && CIN <= kThreads, "one channel per thread");
    const Layer& Ly = A.L[l];
    const int c = threadIdx.x, co = c < COUT ? c : 0, cp = c < CIN ? c : 0;
    float mu, var, mup = 0.f, varp = 0.f;
    bn_moments(A, l, 0, co, mu, var);
    const double b0 = slot_sumd(Ly.bst + co, 2 * COUT), b1 = slot_sumd(Ly.bst + COUT + co, 2 * COUT);
    if constexpr (!FIRST) bn_moments(A, l - 1, 0, cp, mup, varp);
    if (c < COUT) {
      const float rs = rsqrtf(var + A.eps);
      mean[c] = mu;
      rstd[c] = rs;
      gr[c] = Ly.gamma[c] * rs;
      mdy[c] = (float)(b0 * A.inv_count);
      mdyx[c] = (float)(b1 * A.inv_count);
    }
    if constexpr (!FIRST) {
      if (c < CIN) {
        const float sc = A.L[l - 1].gamma[c] * rsqrtf(varp + A.eps);
        sp[c] = sc;
        tp[c] = A.L[l - 1].beta[c] - mup * sc;
      }
    }
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wco = wave % W::WCO, wci = wave / W::WCO;
  // D[ci][co] tiles: A-op = A_shift^T (rows of D = ci), B-op = dZ (cols of D = co); K = tile rows
  f32x4 acc[NTAP][NCI][NCO];
#pragma unroll
  for (int k = 0; k < NTAP; ++k)
#pragma unroll
    for (int b = 0; b < NCI; ++b)
#pragma unroll
      for (int a = 0; a < NCO; ++a) acc[k][b][a] = f32x4{0.f, 0.f, 0.f, 0.f};
  // bias gradient on the matrix cores (a column sum of dZ = ones^T dZ): the waves of ci-block 0 with
  // wci == 0 carry NCO extra accumulators.  (Per-element LDS atomics for these sums contended on the
  // same 128-256 addresses and cost 3-4x the whole wgrad.)
  const bool bias_wave = do_bias && wci == 0;
  bf16x8 ones;
#pragma unroll
  for (int j = 0; j < 8; ++j) ones[j] = (__bf16)1.f;
  f32x4 accb[NCO];
#pragma unroll
  for (int a = 0; a < NCO; ++a) accb[a] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int ntiles = (A.B + 1) / 2;
  // row tiles per workgroup: RTILES at large batches, fewer when the batch is small (the launcher
  // sizes the grid for >= ~512 workgroups)
  const int rgs = gridDim.x / (nci_blk * nco_blk);
  const int rt = (ntiles + rgs - 1) / rgs;
  const int tile0 = rg * rt, nt = min(rt, ntiles - tile0);
  // Blocks 4 and 6 (kWgPrefetch, PF below): the next tile's dZ_l and R_{l-1} rows are loaded into registers
  // before this tile's MFMAs and written to LDS (A decoded) after them, so the global-load latency
  // of a tile hides under the previous tile's matrix work instead of being paid between barriers.
  // One stats group (training): A_{l-1} = dropout(BN(R_{l-1})) with the table's single affine.
  // blocks 4 and 6 (dZ only): blocks 2 and 3 have no registers left for it (spills), and block 5
  // loses more from 2 instead of 3 workgroups per CU than the prefetch gains (wgrad<4> 276 -> 333 us
  // at batch 8192; wgrad<3>: 278 -> 243 us; profiles/train_step_r4.md)
  constexpr bool PF = W::PF;
  constexpr bool PFA = W::PFA;  // block 6: dZ only (the A rows would spill)
  constexpr int NCWD = W::COB / 8, ITD = PF ? kR * NCWD / NT : 1;
  constexpr int NCWA = W::CIB / 8, RPA = NT / NCWA, ITA = PFA ? (kRows + RPA - 1) / RPA : 1;
  static_assert(!PF || (kR * NCWD) % NT == 0, "dZ rows split evenly over the threads");
  bf16x8 pd[ITD];
  u32x4 pa[ITA];
  // the thread index is made opaque per call (see staged_loop): otherwise LICM keeps every item's
  // offset live across the tile loop (~100 VGPRs of spills)
  auto opaque_tid = [] {
    int t = threadIdx.x;
    asm volatile("" : "+v"(t));
    return t;
  };
  auto pf_load = [&](int tile) {
    const int ptid = opaque_tid(), cwa = ptid % NCWA, rina = ptid / NCWA;
    const int row0 = kR * tile;
    const __bf16* dz = A.L[l].dZ + (long long)(row0 + kHalo) * COUT + co0;
#pragma unroll
    for (int i = 0; i < ITD; ++i) {
      const int idx = ptid + i * NT, rc = idx / NCWD, cw = idx - rc * NCWD;
      pd[i] = gld<bf16x8>(dz + (long long)rc * COUT + cw * 8);
    }
    if constexpr (PFA) {
      const __bf16* R = A.L[l - 1].R + (long long)row0 * CIN + ci0 + cwa * 8;
#pragma unroll
      for (int j = 0; j < ITA; ++j) {
        const int rc = rina + j * RPA;
        if (rc < kRows) pa[j] = gld<u32x4>(R + (long long)rc * CIN);
      }
    }
  };
  auto pf_store = [&]() {
    const int ptid = opaque_tid(), cwa = ptid % NCWA, rina = ptid / NCWA;
#pragma unroll
    for (int i = 0; i < ITD; ++i) {
      const int idx = ptid + i * NT, rc = idx / NCWD, cw = idx - rc * NCWD;
      *reinterpret_cast<bf16x8*>(dz_lds + lds_off(rc, cw * 16, DZRS)) = pd[i];
    }
    if constexpr (PFA) {
      const float dsc = A.dropout != 0 ? A.L[l - 1].dsc : 1.f;
      float s0[8], t0[8];
      lds_row8(sp, ci0 + cwa * 8, dsc, s0);
      lds_row8(tp, ci0 + cwa * 8, dsc, t0);
#pragma unroll
      for (int j = 0; j < ITA; ++j) {
        const int rc = rina + j * RPA;
        if (rc >= kRows) continue;
        u32x4 o;
#pragma unroll
        for (int q = 0; q < 4; ++q) o[q] = decode_pair(pa[j][q], s0[2 * q], t0[2 * q], s0[2 * q + 1], t0[2 * q + 1]);
        *reinterpret_cast<u32x4*>(a_lds + lds_off(rc, cwa * 16, ARS)) = o;
      }
    }
  };
  if constexpr (PF) {
    if (nt > 0) pf_load(tile0);
  }
  for (int it = 0; it < nt; ++it) {
    const int tile = tile0 + it;
    const int row0 = kR * tile;
    __syncthreads();
    if constexpr (PF) {
      pf_store();
      if constexpr (!PFA) stage_act<l - 1, kRows, W::CIB / 8, 4, NT>(A, a_lds, ARS, row0, ci0, sp, tp, 0);
    } else if constexpr (FIRST) {  // no dgrad for block 1: dZ_1 is recomputed here (a single ci block)
      stage_dz<l, kR, W::COB / 8>(A, dz_lds, DZRS, row0 + kHalo, co0, gr, mean, rstd, mdy, mdyx);
      // im2col of the raw input: col kk = tap*4 + ci (kk < 28), rows = tile rows; one 8-B load per
      // (row, tap) -- the 4 channels of an input row are contiguous
      for (int i = threadIdx.x; i < kR * 8; i += kThreads) {
        const int r = i >> 3, tap = i & 7;
        bf16x4 v = {(__bf16)0.f, (__bf16)0.f, (__bf16)0.f, (__bf16)0.f};
        if (tap < K) v = gld<bf16x4>(A.x + (long long)(row0 + kHalo + r + tap - PAD) * 4);
        *reinterpret_cast<bf16x4*>(a_lds + lds_off(r, tap * 8, ARS)) = v;
      }
    } else {
      stage_dz_copy<l, kR, W::COB / 8, W::U, NT>(A, dz_lds, DZRS, row0 + kHalo, co0);
      stage_act<l - 1, kRows, W::CIB / 8, 4, NT>(A, a_lds, ARS, row0, ci0, sp, tp, 0);
    }
    __syncthreads();
    if constexpr (PF) {
      if (it + 1 < nt) pf_load(tile + 1);
    }
#pragma unroll
    for (int ks = 0; ks < kR / 32; ++ks) {
      bf16x8 fb[NCO];
#pragma unroll
      for (int a = 0; a < NCO; ++a) fb[a] = tr_frag(dz_lds, DZRS, ks * 32, (wco * NCO + a) * 16);
      if (bias_wave) {  // db[co] = sum_rows dZ[row][co]: one MFMA with an all-ones A fragment
#pragma unroll
        for (int a = 0; a < NCO; ++a) accb[a] = mfma16(ones, fb[a], accb[a]);
      }
#pragma unroll
      for (int k = 0; k < NTAP; ++k) {
#pragma unroll
        for (int b = 0; b < NCI; ++b) {
          const int arow = FIRST ? ks * 32 : kHalo + ks * 32 + k - PAD;
          const bf16x8 fa = tr_frag(a_lds, ARS, arow, (wci * NCI + b) * 16);
#pragma unroll
          for (int a = 0; a < NCO; ++a) acc[k][b][a] = mfma16(fa, fb[a], acc[k][b][a]);
        }
      }
    }
  }
  // lane (m, h) holds D[ci = 4h + i][co = m] of each tile: 16 consecutive co per row -> 64-B runs
  const int m = lane & 15, h = lane >> 4;
  const Layer& Ly = A.L[l];
  float* part = A.wpart != nullptr ? A.wpart + ext.part_off + (long long)rg * (K * CIN * COUT + COUT) : nullptr;
#pragma unroll
  for (int k = 0; k < NTAP; ++k)
#pragma unroll
    for (int b = 0; b < NCI; ++b)
#pragma unroll
      for (int a = 0; a < NCO; ++a) {
        const int co = co0 + (wco * NCO + a) * 16 + m;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int rowi = (wci * NCI + b) * 16 + 4 * h + i;  // ci (or kk for block 1)
          int e;  // element of dW (k, Cin, Cout)
          if constexpr (FIRST) {
            const int tap = rowi >> 2, ci = rowi & 3;
            if (tap >= K) continue;
            e = (tap * CIN + ci) * COUT + co;
          } else {
            e = (k * CIN + ci0 + rowi) * COUT + co;
          }
          if (part != nullptr)
            part[e] = acc[k][b][a][i];  // this row group's exclusive slot: summed in order by wgrad_reduce
          else
            atomicAdd(Ly.gw + e, acc[k][b][a][i]);
        }
      }
  if (bias_wave && h == 0) {  // row 0 of each ones^T dZ tile: lanes 0-15 hold its 16 column sums
#pragma unroll
    for (int a = 0; a < NCO; ++a) {
      const int co = co0 + (wco * NCO + a) * 16 + m;
      if (part != nullptr)
        part[K * CIN * COUT + co] = accb[a][0];
      else
        atomicAdd(Ly.gb + co, accb[a][0]);
    }
  }
}

// ------------------------------------------------------------------------------------------------ host
// fused: the single-device step whose reductions run inside other launches (train_launch_dgrad /
// train_launch_finalize with fused set): no reduce launch here; the table job in workgroup 0; wgrad<0>'s
// partials behind the shared region
template <int l, bool MB>
static void wg_launch(const Args& A, const Args* Am, int M, hipStream_t st, bool fused) {
  const WgShape s = wg_shape<l>(A.B, M, A.det != nullptr);
  // the table's backward rows of block l-1 (bst[l-1] is complete after dgrad<l>, which ran before this
  // wgrad) for dgrad<l-1> / wgrad<l-1>: the reduce launch's extra workgroup, or (fused) wgrad's workgroup 0
  const bool side = A.tab != nullptr && l >= 1 && !A.bwd_self;
  TabBwd tb = {};
  if constexpr (l >= 1) {
    if (side) {
      tb.bst = A.L[l - 1].bst;
      tb.cc = C[l];
      tb.mdy = A.tab + ((l - 1) * kTabRows + kTabMdy) * 256;
      tb.mdyx = A.tab + ((l - 1) * kTabRows + kTabMdyx) * 256;
      tb.inv_count = A.inv_count;
    }
  }
  WgExt ext = {};
  if (fused) {
    ext.part_off = (l == 0) ? wg_main_floats(A.B) : 0;
    ext.tb = tb;
  }
  hipLaunchKernelGGL(HIP_KERNEL_NAME(wgrad_kernel<l, MB>), dim3(s.grid, 1, M), dim3(s.threads), s.lds, st, A, Am, ext);
  if (A.wpart != nullptr && !fused) {
    if constexpr (MB) {
      hipLaunchKernelGGL(wgrad_reduce_mb_kernel, dim3(s.blocks + (side ? 1 : 0), 1, M), dim3(256), 0, st, Am, l, s.rgs,
                         s.kcc, s.cout, s.J, side ? 1 : 0);
    } else {
      hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(s.blocks, side ? 2 : 1), dim3(256), 0, st, A.wpart, s.rgs, s.kcc,
                         s.cout, A.L[l].gw, A.L[l].gb, s.J, tb);
    }
  }
}

template <bool MB>
static hipError_t wgrad_launch_t(const Args& A, const Args* Am, int M, int l, bool fused, hipStream_t st) {
  if (l < 0 || l > 5) return hipErrorInvalidValue;
  for_block(l, [&](auto L) { wg_launch<decltype(L)::value, MB>(A, Am, M, st, fused); });
  return hipGetLastError();
}

hipError_t wgrad_launch(const Args& A, const Args* Am, int M, int l, bool fused, hipStream_t st) {
  return Am != nullptr ? wgrad_launch_t<true>(A, Am, M, l, fused, st) : wgrad_launch_t<false>(A, nullptr, 1, l, fused, st);
}

}  // namespace train
}  // namespace apneauq
