// Rank statistics (ROC / PR AUC, Mann-Whitney U) of all bootstrap replicates from one sort (gfx950).
//
// Resampling does not change the order of the scores, so the windows are sorted once (torch.sort in
// ops/rank.py) and a replicate is a vector of integer weights over the sorted windows.
//
// rank_count   replicate b: w[b, pos[draw]] += 1 for every draw (idx[b, j] or the counter hash of
//              bootstrap_kernel), pos = sorted position of a window (negative: the window was dropped).
//              No-return 32-bit integer atomics at the memory side; a row is n int32, so one replicate's
//              draws hit n distinct addresses at random and a per-wave pre-reduction has nothing to merge.
// rank_totals  replicate b, split g: weighted positives / negatives of sorted windows [bounds[g], bounds[g+1]).
// rank_scan    replicate b, split g: a segmented scan over the tie groups of the split.  With P_g, N_g the
//              weighted positives / negatives of tie group g in ascending score order it adds, per group of
//              non-zero weight,
//                U2      += P_g (2 cumN_before_g + N_g)                      (twice the Mann-Whitney U)
//                groups  += 1
//                prauc_q += rint(2^56 dR_g (prec_g + prec_prev_g) / 2)      (trapezoid of the PR curve)
//                ap_q    += rint(2^56 dR_g prec_g)                          (average precision)
//              where TP_g = P - cumP_before_g, FP_g = N - cumN_before_g, prec_g = TP_g / (TP_g + FP_g),
//              prec_prev_g the precision of the next higher non-empty group ((TP_g - P_g) / (TP_g - P_g +
//              FP_g - N_g), 1 for the highest) and dR_g = P_g / P.
//
// Grid invariance: the split bounds are tie-group starts (ops/rank.py:split_bounds), so no group straddles
// a split; a split's prefix (positives / negatives before it) is the sum of the totals of the splits
// before it, added in index order in integers; every group's term depends only on integers that are the
// same for every split count, and is quantised before it is added.  All sums are integer.
//
// Limits: n <= 2^27 sorted windows, every replicate's total weight W < 2^31 (so U2 <= W^2 / 2 < 2^61 and a
// (positives, negatives) pair fits one 64-bit word, 32 bits each), at most 64 splits.  The fixed-point
// scale 2^56 (ops/rank.py S_BITS) keeps the quantisation n 2^-57 <= 1e-9 at n = 2^27 and the sum (the terms
// add up to at most 1) at 2^56.
#include "common.h"
#include "uq_api.h"

namespace apneauq {

typedef unsigned long long u64;

constexpr int kRankThreads = 256;
constexpr int kRankWaves = kRankThreads / kWave;
constexpr int kRankItems = 8;                             // consecutive sorted windows per thread: two 16-B loads
constexpr int kRankTile = kRankThreads * kRankItems;
constexpr int kRankMaxSplits = 64;
constexpr double kRankQScale = 72057594037927936.0;       // 2^56
constexpr int kRankTot = 3;                               // rank_totals columns: positives, negatives, negative weights
constexpr int kRankPart = 4;                              // rank_scan columns: U2, groups, prauc_q, ap_q

constexpr int kCountThreads = 256;
constexpr int kCountUnroll = 4;

// packed byte per sorted window: bit 0 = target z, bit 1 = first window of a tie group
constexpr unsigned kRankZ = 1u, kRankStart = 2u;

__global__ __launch_bounds__(kCountThreads) void rank_count_kernel(const int* __restrict__ pos,
                                                                   const int* __restrict__ idx, unsigned seed,
                                                                   int n_draw, int n_sorted, int b0, long long stride,
                                                                   int* __restrict__ w) {
  const int b = blockIdx.x;
  APNEAUQ_DASSERT(blockDim.x == kCountThreads && n_draw > 0 && n_sorted >= 0 && stride >= n_sorted);
  const unsigned bkey = boot_key(seed, (unsigned)(b0 + b));
  const int* idx_b = idx ? idx + (long long)b * n_draw : nullptr;
  int* w_b = w + (long long)b * stride;
  const long long step = (long long)gridDim.y * kCountThreads * kCountUnroll;
  for (long long jb = (long long)blockIdx.y * kCountThreads * kCountUnroll + threadIdx.x; jb < n_draw; jb += step) {
    unsigned raw[kCountUnroll];
#pragma unroll
    for (int u = 0; u < kCountUnroll; ++u) {
      const long long j = jb + (long long)u * kCountThreads;
      raw[u] = 0xFFFFFFFFu;
      if (j < n_draw) {
        if (idx_b) {
          raw[u] = (unsigned)idx_b[j];
        } else {
          raw[u] = boot_draw(bkey, (unsigned)j, n_draw);
        }
      }
    }
    int p[kCountUnroll];
#pragma unroll
    for (int u = 0; u < kCountUnroll; ++u) p[u] = raw[u] < (unsigned)n_draw ? pos[raw[u]] : -1;
#pragma unroll
    for (int u = 0; u < kCountUnroll; ++u)
      if ((unsigned)p[u] < (unsigned)n_sorted)
        (void)__hip_atomic_fetch_add(w_b + p[u], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// Weights and packed bytes of sorted windows [base, base + 8), base a multiple of 4; windows outside
// [lo, hi) come back with weight 0 and code 0.  16-B / 4-B loads where the quad lies inside the row.
__device__ __forceinline__ void rank_load(const int* __restrict__ w_b, const unsigned char* __restrict__ packed, int base,
                                          int lo, int hi, int n, int (&wv)[kRankItems], unsigned (&code)[kRankItems]) {
#pragma unroll
  for (int h = 0; h < kRankItems / 4; ++h) {
    const int e = base + 4 * h;
    int4 v = make_int4(0, 0, 0, 0);
    unsigned c = 0u;
    if (e < hi && e + 4 > lo) {
      if (e + 4 <= n) {
        v = *reinterpret_cast<const int4*>(w_b + e);
        c = *reinterpret_cast<const unsigned*>(packed + e);
      } else {
        int t[4] = {0, 0, 0, 0};
        for (int q = 0; q < 4; ++q)
          if (e + q < n) {
            t[q] = w_b[e + q];
            c |= (unsigned)packed[e + q] << (8 * q);
          }
        v = make_int4(t[0], t[1], t[2], t[3]);
      }
    }
    const int t[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const bool in = e + q >= lo && e + q < hi;
      wv[4 * h + q] = in ? t[q] : 0;
      code[4 * h + q] = in ? (c >> (8 * q)) & 3u : 0u;
    }
  }
}

__device__ __forceinline__ void rank_range(const int* __restrict__ bounds, int g, int n, int& lo, int& hi) {
  lo = min(max(bounds[g], 0), n);
  hi = min(max(bounds[g + 1], lo), n);
}

__global__ __launch_bounds__(kRankThreads) void rank_totals_kernel(const int* __restrict__ w, long long stride,
                                                                   const unsigned char* __restrict__ packed,
                                                                   const int* __restrict__ bounds, int n,
                                                                   long long* __restrict__ tot) {
  __shared__ u64 red[kRankWaves][kRankTot];
  const int b = blockIdx.x, g = blockIdx.y;
  APNEAUQ_DASSERT(blockDim.x == kRankThreads && n >= 1 && (stride & 3) == 0 && stride >= n);
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  int lo, hi;
  rank_range(bounds, g, n, lo, hi);
  const int* w_b = w + (long long)b * stride;
  u64 acc[kRankTot] = {0ull, 0ull, 0ull};
  for (int t0 = lo & ~3; t0 < hi; t0 += kRankTile) {
    int wv[kRankItems];
    unsigned code[kRankItems];
    rank_load(w_b, packed, t0 + (int)threadIdx.x * kRankItems, lo, hi, n, wv, code);
#pragma unroll
    for (int k = 0; k < kRankItems; ++k) {
      const u64 x = (u64)(unsigned)max(wv[k], 0);
      acc[0] += (code[k] & kRankZ) ? x : 0ull;
      acc[1] += (code[k] & kRankZ) ? 0ull : x;
      acc[2] += wv[k] < 0 ? 1ull : 0ull;
    }
  }
#pragma unroll
  for (int c = 0; c < kRankTot; ++c) {
    const u64 v = wave_sum(acc[c]);
    if (lane == 0) red[wave][c] = v;
  }
  __syncthreads();
  if ((int)threadIdx.x < kRankTot) {
    u64 v = 0ull;
    for (int ww = 0; ww < kRankWaves; ++ww) v += red[ww][threadIdx.x];
    tot[((long long)b * gridDim.y + g) * kRankTot + threadIdx.x] = (long long)v;
  }
}

// A (positives, negatives) pair in one word: positives in the low, negatives in the high 32 bits.  Both
// stay below 2^31, so sums of pairs never carry across, pairs of prefix sums are ordered like either
// field, and "+ 1" / "- 1" on the word touch the low field only.
__device__ __forceinline__ u64 rank_pair(unsigned weight, unsigned code) {
  return (code & kRankZ) ? (u64)weight : (u64)weight << 32;
}

__global__ __launch_bounds__(kRankThreads) void rank_scan_kernel(const int* __restrict__ w, long long stride,
                                                                 const unsigned char* __restrict__ packed,
                                                                 const int* __restrict__ bounds,
                                                                 const long long* __restrict__ tot, int n,
                                                                 long long* __restrict__ part) {
  __shared__ u64 s_add[2][kRankWaves], s_max[2][kRankWaves];
  __shared__ u64 s_head[2];
  __shared__ long long s_red[kRankWaves][kRankPart];
  const int b = blockIdx.x, g = blockIdx.y, n_split = gridDim.y;
  APNEAUQ_DASSERT(blockDim.x == kRankThreads && n >= 1 && n_split <= kRankMaxSplits && (stride & 3) == 0 && stride >= n);
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  int lo, hi;
  rank_range(bounds, g, n, lo, hi);
  if (threadIdx.x == 0) {
    // positives / negatives before this split and in the whole replicate: integer adds in split order
    u64 before = 0ull, all = 0ull;
    const long long* t = tot + (long long)b * n_split * kRankTot;
    for (int h = 0; h < n_split; ++h) {
      const u64 x = ((u64)t[h * kRankTot] & 0xFFFFFFFFull) | ((u64)t[h * kRankTot + 1] << 32);
      all += x;
      before += h < g ? x : 0ull;
    }
    s_head[0] = before;
    s_head[1] = all;
  }
  __syncthreads();
  const unsigned p_tot = (unsigned)s_head[1], n_tot = (unsigned)(s_head[1] >> 32);
  u64 carry_add = s_head[0];   // pair before the current tile
  u64 carry_start = s_head[0]; // pair before the tie group that is open at the current tile's first window
  const int* w_b = w + (long long)b * stride;
  u64 acc_u2 = 0ull;
  long long acc_groups = 0, acc_pr = 0, acc_ap = 0;
  int buf = 0;
  for (int t0 = lo & ~3; t0 < hi; t0 += kRankTile, buf ^= 1) {
    const int base = t0 + (int)threadIdx.x * kRankItems;
    int wv[kRankItems];
    unsigned code[kRankItems];
    rank_load(w_b, packed, base, lo, hi, n, wv, code);
    // is the window after this thread's last one the start of a group (or past the split)?
    const bool next_start = base + kRankItems >= hi || (packed[base + kRankItems] & kRankStart);
    // inclusive add-scan of the pairs, thread-relative
    u64 c[kRankItems], run = 0ull;
#pragma unroll
    for (int k = 0; k < kRankItems; ++k) {
      run += rank_pair((unsigned)max(wv[k], 0), code[k]);
      c[k] = run;
    }
    u64 inc = run;  // wave-inclusive scan of the thread totals
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
      const u64 v = __shfl_up(inc, o, kWave);
      if (lane >= o) inc += v;
    }
    const u64 excl_w = inc - run;  // wave-relative pair before this thread
    // running maximum of (wave-relative pair before a group start) + 1: the latest start so far, 0 = none
    u64 m[kRankItems], mrun = 0ull;
#pragma unroll
    for (int k = 0; k < kRankItems; ++k) {
      const bool start = (code[k] & kRankStart) || base + k == lo;  // a split begins at a group start
      const bool in = base + k >= lo && base + k < hi;
      const u64 before = excl_w + (k ? c[k - 1] : 0ull);
      if (in && start) mrun = before + 1ull;  // prefix pairs never decrease: the latest start is the maximum
      m[k] = mrun;
    }
    u64 minc = mrun;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
      const u64 v = __shfl_up(minc, o, kWave);
      if (lane >= o) minc = max(minc, v);
    }
    u64 mexcl = __shfl_up(minc, 1, kWave);
    if (lane == 0) mexcl = 0ull;
    if (lane == kWave - 1) {
      s_add[buf][wave] = inc;
      s_max[buf][wave] = minc;
    }
    __syncthreads();
    // cross-wave combine in wave order (integers)
    u64 off = carry_add, wave_off = carry_add, start_before = carry_start, tile_start = carry_start;
#pragma unroll
    for (int ww = 0; ww < kRankWaves; ++ww) {
      if (ww == wave) {
        wave_off = off;
        start_before = tile_start;
      }
      if (s_max[buf][ww] != 0ull) tile_start = off + s_max[buf][ww] - 1ull;
      off += s_add[buf][ww];
    }
    const u64 thread_start = mexcl != 0ull ? wave_off + mexcl - 1ull : start_before;
#pragma unroll
    for (int k = 0; k < kRankItems; ++k) {
      const int i = base + k;
      if (i < lo || i >= hi) continue;
      const bool last = k + 1 < kRankItems ? (i + 1 >= hi || (code[k + 1] & kRankStart)) : next_start;
      if (!last) continue;
      const u64 st = m[k] != 0ull ? wave_off + m[k] - 1ull : thread_start;
      const u64 in = wave_off + excl_w + c[k];
      const unsigned p_in = (unsigned)in, n_in = (unsigned)(in >> 32), p_st = (unsigned)st, n_st = (unsigned)(st >> 32);
      const unsigned p_g = p_in - p_st, n_g = n_in - n_st;
      if (p_g + n_g == 0u) continue;  // a group of weight 0 is no curve point
      acc_groups += 1;
      acc_u2 += (u64)p_g * (2ull * n_st + n_g);
      if (p_g) {
        const unsigned tp = p_tot - p_st, fp = n_tot - n_st, tp_prev = p_tot - p_in, fp_prev = n_tot - n_in;
        const double prec = (double)tp / (double)(tp + fp);
        const double prec_prev = tp_prev + fp_prev ? (double)tp_prev / (double)(tp_prev + fp_prev) : 1.0;
        const double d_recall = (double)p_g / (double)p_tot;
        acc_pr += __double2ll_rn(d_recall * (prec + prec_prev) * 0.5 * kRankQScale);
        acc_ap += __double2ll_rn(d_recall * prec * kRankQScale);
      }
    }
    carry_add = off;
    carry_start = tile_start;
  }
  const u64 r[kRankPart] = {acc_u2, (u64)acc_groups, (u64)acc_pr, (u64)acc_ap};
#pragma unroll
  for (int q = 0; q < kRankPart; ++q) {
    const u64 v = wave_sum(r[q]);
    if (lane == 0) s_red[wave][q] = (long long)v;
  }
  __syncthreads();
  if ((int)threadIdx.x < kRankPart) {
    long long v = 0;
    for (int ww = 0; ww < kRankWaves; ++ww) v += s_red[ww][threadIdx.x];
    part[((long long)b * n_split + g) * kRankPart + threadIdx.x] = v;
  }
}

int rank_max_splits() { return kRankMaxSplits; }

hipError_t launch_rank_count(const int* pos, const int* idx, unsigned seed, int n_draw, int n_sorted, int b0, int n_boot,
                             long long stride, int* w, hipStream_t stream) {
  if (n_boot <= 0 || n_draw <= 0 || n_sorted <= 0) return hipSuccess;
  const int per_block = kCountThreads * kCountUnroll * 4;
  int slices = (n_draw + per_block - 1) / per_block;
  slices = slices < 1 ? 1 : (slices > 1024 ? 1024 : slices);
  hipLaunchKernelGGL(rank_count_kernel, dim3(n_boot, slices), dim3(kCountThreads), 0, stream, pos, idx, seed, n_draw,
                     n_sorted, b0, stride, w);
  return hipGetLastError();
}

hipError_t launch_rank_totals(const int* w, long long stride, const unsigned char* packed, const int* bounds, int n,
                              int n_boot, int splits, long long* tot, hipStream_t stream) {
  if (n_boot <= 0 || n <= 0) return hipSuccess;
  hipLaunchKernelGGL(rank_totals_kernel, dim3(n_boot, splits), dim3(kRankThreads), 0, stream, w, stride, packed, bounds, n,
                     tot);
  return hipGetLastError();
}

hipError_t launch_rank_scan(const int* w, long long stride, const unsigned char* packed, const int* bounds,
                            const long long* tot, int n, int n_boot, int splits, long long* part, hipStream_t stream) {
  if (n_boot <= 0 || n <= 0) return hipSuccess;
  hipLaunchKernelGGL(rank_scan_kernel, dim3(n_boot, splits), dim3(kRankThreads), 0, stream, w, stride, packed, bounds, tot,
                     n, part);
  return hipGetLastError();
}

}  // namespace apneauq
