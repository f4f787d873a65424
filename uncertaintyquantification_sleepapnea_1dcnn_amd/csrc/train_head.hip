// Parameter table and head (GAP + Dense + BCE + its gradient) of the layer-wise training path.
// See train_launch.hip for the design (layout, sign-bit mask, what is recomputed where) and train_geo.h for
// the launch geometry.
#include "train_launch.h"
#include "train_stage.h"

namespace apneauq {
namespace train {

// Parameter table (Args::tab) of single-device training: mode 0 = the forward rows of every block
// (one workgroup per block, launched after the six forward kernels; read by the head, dgrad and wgrad),
// mode 1 = the backward rows of block l (not on the default step: the backward kernels sum bst[l]
// themselves, 2 x 16 slots per channel, which measured cheaper than one more graph node per block).
template <bool MB>
__global__ __launch_bounds__(256) void tab_kernel(Args A_, const Args* __restrict__ Am, int mode, int l) {
  const MbPos pos = mb_pos<MB>();
  const Args& A = member_args<MB>(A_, Am, pos);
  if (mode == 0)
    tab_write_fwd(A, pos.bx);
  else
    tab_write_bwd(A, l);
}

// ------------------------------------------------------------------------------------------------
// Head: A_6 = dropout(BN(R_6)) -> GAP -> Dense(96->1) -> logit, BCE, dlogit = (sigmoid - y)/B,
// dense gradients, and the backward sums of dY_6 (sum dY, sum dY * xhat) — one sample per wave,
// each lane owning channels (lane, lane + 64).
// ------------------------------------------------------------------------------------------------
template <bool MB>
__global__ __launch_bounds__(kThreads) void head_kernel(Args A_, const Args* __restrict__ Am, int backward, int spw,
                                                      int tabx) {
  const MbPos pos = mb_pos<MB>();
  const Args& A = member_args<MB>(A_, Am, pos);
  // tabx > 0: the last tabx workgroups write the forward rows of the parameter table (what a tab_kernel
  // launch did before the head), the head computes block 6's rows itself with the same arithmetic
  if (tabx > 0 && pos.bx >= (int)gridDim.x - tabx) {
    tab_write_fwd(A, pos.bx - ((int)gridDim.x - tabx));
    return;
  }
  // One sample at a time per wave, spw samples per wave (4 * spw per workgroup: fewer workgroups'
  // sums to merge at large batches).  Lane (cw, ph) = (lane % 12, lane / 12), lanes 0..59: channels
  // [8cw, 8cw+8) of rows ph, ph+5, ..., ph+55 — twelve 16-B loads per lane, all in flight at once
  // (the previous per-channel/per-row scalar loop was load-latency bound: ~50 us at any batch size).
  constexpr int Cc = C[6], NCW = Cc / 8, NPH = 5, NJ = kL / NPH;
  static_assert(NCW * NPH <= 64 && NJ * NPH == kL, "head lane map");
  float* prm = reinterpret_cast<float*>(smem);  // [mu | rs | sc | sh | w] x 96, then sums
  float* pmu = prm, *prs = prm + Cc, *psc = prm + 2 * Cc, *psh = prm + 3 * Cc, *pw = prm + 4 * Cc;
  float* dw = prm + 5 * Cc;     // dense-weight gradient sums
  float* bsum0 = dw + Cc;       // sum dY, sum dY * xhat (backward BN sums of block 6)
  float* bsum1 = bsum0 + Cc;
  float* red = bsum1 + Cc;      // per-workgroup loss / dense-bias sums: one global atomic per workgroup
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nwg0 = pos.bx * 4 * spw;  // the workgroup's first sample
  const Layer& Ly = A.L[5];
  const int g_first = min(nwg0, A.B - 1) / A.n_win;
  const int g_last = min(nwg0 + 4 * spw - 1, A.B - 1) / A.n_win;
  for (int c = threadIdx.x; c < 3 * Cc + 2; c += kThreads) dw[c] = 0.f;
  auto params = [&](int g) {
    if (A.tab != nullptr && tabx == 0) {  // single-device training (one group): the forward rows of T[5]
      for (int c = threadIdx.x; c < Cc; c += kThreads) {
        pmu[c] = tab_row(A, 5, kTabMean)[c];
        prs[c] = tab_row(A, 5, kTabRstd)[c];
        psc[c] = tab_row(A, 5, kTabS)[c];
        psh[c] = tab_row(A, 5, kTabT)[c];
        pw[c] = A.dense_w[c];
      }
      return;
    }
    for (int c = threadIdx.x; c < Cc; c += kThreads) {
      float m1, var;
      bn_moments(A, 5, g, c, m1, var);
      const float r = rsqrtf(var + A.eps), sc = Ly.gamma[c] * r;  // as tab_write_fwd
      pmu[c] = m1;
      prs[c] = r;
      psc[c] = sc;
      psh[c] = Ly.beta[c] - m1 * sc;
      pw[c] = A.dense_w[c];
    }
  };
  params(g_first);
  __syncthreads();
  // (a workgroup whose samples span two stats groups — an MC-Dropout pass boundary — recomputes
  //  its per-lane parameters of the other group from the global sums directly)
  const bool mixed = g_first != g_last;
  const int cw = lane % NCW, ph = lane / NCW;
  const int c0 = cw * 8;
  const float dsc6 = A.dropout ? Ly.dsc : 1.f;
  for (int s = 0; s < spw; ++s) {  // wave-uniform
    const int n = nwg0 + s * 4 + wave;
    const bool active = n < A.B && lane < NCW * NPH;
    float mu[8], rs[8], sc[8], sh[8], w[8];
    if (active) {
      const int g = n / A.n_win;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int c = c0 + j;
        if (mixed && g != g_first) {
          float m1, var;
          bn_moments(A, 5, g, c, m1, var);
          rs[j] = rsqrtf(var + A.eps);
          mu[j] = m1;
          sc[j] = Ly.gamma[c] * rs[j];
          sh[j] = Ly.beta[c] - m1 * sc[j];
        } else {
          mu[j] = pmu[c];
          rs[j] = prs[c];
          sc[j] = psc[c];
          sh[j] = psh[c];
        }
        w[j] = pw[c];
      }
    }
    bf16x8 v[NJ];
    float gap[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (active) {
      const __bf16* base = Ly.R + (long long)(kHalo + n * kSR) * Cc + c0;
#pragma unroll
      for (int k = 0; k < NJ; ++k) v[k] = gld<bf16x8>(base + (long long)(ph + NPH * k) * Cc);
#pragma unroll
      for (int k = 0; k < NJ; ++k) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {  // block 6's dropout mask is R_6's sign bit
          const float a = bf_abs(v[k][j]) * sc[j] + sh[j];
          gap[j] += bf_dropped(v[k][j]) ? 0.f : a * dsc6;
        }
      }
    }
    float part = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) part += gap[j] * w[j];
    const float z = wave_sum(active ? part : 0.f) * (1.0f / kL) + A.dense_b[0];
    if (n < A.B && lane == 0) A.logits[n] = z;
    if (backward && n < A.B) {
      // e = exp(-|z|) in (0, 1] (expf: __expf rounds z log2(e) first, a relative error of ~|z| 2^-24 in the
      // result); q = e / (1 + e) is the sigmoid's small side at full relative accuracy, and prob - y comes
      // from the side that does not cancel (a saturated 1.0f minus a label of 1 is 0 where the gradient is -q)
      const float e = expf(-fabsf(z));
      const float q = e / (1.0f + e);
      const float yv = A.y[n];
      const float dl = (z >= 0.f ? (1.0f - yv) - q : q - yv) * A.inv_batch;
      float* rec = A.det != nullptr ? A.det + (long long)n * kHeadRec : nullptr;  // deterministic mode
      if (lane == 0) {
        const float loss = fmaxf(z, 0.f) - z * yv + log1pf(e);  // BCE on logits
        A.dlogit[n] = dl;
        if (rec != nullptr) {
          rec[0] = loss;
          rec[1] = dl;
        } else {
          atomicAdd(&red[0], loss);
          atomicAdd(&red[1], dl);
        }
      }
      if (active) {
        float b0[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, b1[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < NJ; ++k) {
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const float dy = bf_dropped(v[k][j]) ? 0.f : dl * w[j] * (1.0f / kL) * dsc6;
            const float xh = (bf_abs(v[k][j]) - mu[j]) * rs[j];
            b0[j] += dy;
            b1[j] += dy * xh;
          }
        }
        // the sample's sums over its 5 row-phase lanes (lanes cw + 12 ph), in a fixed order; then
        // one LDS atomic per channel from the ph = 0 lanes (not 5)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float sdw = 0.f, sb0 = 0.f, sb1 = 0.f;
          const float pdw = dl * gap[j] * (1.0f / kL);
#pragma unroll
          for (int q = 0; q < NPH; ++q) {
            sdw += __shfl(pdw, cw + NCW * q, kWave);
            sb0 += __shfl(b0[j], cw + NCW * q, kWave);
            sb1 += __shfl(b1[j], cw + NCW * q, kWave);
          }
          if (ph == 0) {
            if (rec != nullptr) {
              rec[2 + c0 + j] = sdw;
              rec[2 + Cc + c0 + j] = sb0;
              rec[2 + 2 * Cc + c0 + j] = sb1;
            } else {
              atomicAdd(&dw[c0 + j], sdw);
              atomicAdd(&bsum0[c0 + j], sb0);
              atomicAdd(&bsum1[c0 + j], sb1);
            }
          }
        }
      }
    }
  }
  if (backward) {
    if (A.det != nullptr) return;  // det_reduce_kernel sums the per-sample records
    __syncthreads();
    float* hp = A.hpart != nullptr ? A.hpart + (pos.bx % kStatSlots) * (Cc + 2) : nullptr;
    for (int c = threadIdx.x; c < Cc; c += kThreads) {
      if (hp != nullptr) {  // slotted: summed by bn_finalize_kernel
        if (c == 0) {
          atomicAdd(hp + Cc, red[0]);
          atomicAdd(hp + Cc + 1, red[1]);
        }
        atomicAdd(hp + c, dw[c]);
      } else {
        if (c == 0) {
          atomicAdd(A.loss_sum, red[0]);
          atomicAdd(A.g_dense_b, red[1]);
        }
        atomicAdd(A.g_dense_w + c, dw[c]);
      }
      double* bst = Ly.bst + (pos.bx % kStatSlots) * 2 * Cc;
      atomicAdd(bst + c, (double)bsum0[c]);
      atomicAdd(bst + Cc + c, (double)bsum1[c]);
    }
  }
}

// ------------------------------------------------------------------------------------------------ host
hipError_t tab_launch(const Args& A, const Args* Am, int M, int mode, int l, hipStream_t st) {
  const dim3 g(mode == 0 ? 6 : 1, 1, M);
  if (Am != nullptr)
    hipLaunchKernelGGL(tab_kernel<true>, g, dim3(256), 0, st, A, Am, mode, l);
  else
    hipLaunchKernelGGL(tab_kernel<false>, g, dim3(256), 0, st, A, nullptr, mode, l);
  return hipGetLastError();
}

// tabx: extra workgroups writing the table's forward rows, one per block (single launches only)
hipError_t head_launch(const Args& A, const Args* Am, int M, int backward, int tabx, hipStream_t st) {
  const int spw = head_spw(A.B, M, backward);
  const dim3 g(head_grid(A.B, M, backward) + tabx, 1, M);
  if (Am != nullptr)
    hipLaunchKernelGGL(head_kernel<true>, g, dim3(256), lds_head(), st, A, Am, backward, spw, tabx);
  else
    hipLaunchKernelGGL(head_kernel<false>, g, dim3(256), lds_head(), st, A, nullptr, backward, spw, tabx);
  return hipGetLastError();
}

}  // namespace train
}  // namespace apneauq
