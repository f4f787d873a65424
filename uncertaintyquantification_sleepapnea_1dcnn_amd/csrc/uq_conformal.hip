// Split conformal prediction over random calibration / test splits from one sort (gfx950).
//
// A split does not change the order of the scores, so the windows are sorted once (ops/rank.py:prep) and a
// split is a role per sorted window: calibration, test or (cluster = "subsample") neither.  The role is a
// counter hash of (seed, split, unit) (common.h split_hash), evaluated where it is needed: no (R, n) array
// exists.  Every conformal threshold is then a rank selection among the calibration windows and every
// coverage / set-size count a prefix count of the test windows:
//
// conformal_select  split r: totals (cal0, cal1, test0, test1) and, per stratum and miscoverage level, the
//                   sorted position of the calibration window of rank k(n_cal) = ceil((n_cal + 1)(1 - alpha))
//                   in integers (stratum 0 / single stratum: k-th smallest; stratum 1: k-th largest, i.e. the
//                   (n_cal - k + 1)-th smallest; -1 where k > n_cal).
// conformal_count   split r, cut c: the test windows of class 0 / 1 among sorted positions [0, c).
//
// One workgroup per split, one walk over the row per kernel.  The row is cut into S <= kConfMaxSeg segments
// of span * kConfTile windows; a wave takes every 4th segment, counts its role members per class as a packed
// (class 0, class 1) pair and leaves the pair in LDS.  A block scan turns the pairs into prefixes; a rank or
// a cut is then located by a binary search / a division, and only the one segment that holds it is walked
// again (by one wave).  All results are integers: they do not depend on span or on the order of the waves.
//
// Limits: n <= 2^27 (a count fits 31 bits, so sums of pairs never carry across), A <= 32, Q <= 64.
#include "common.h"
#include "uq_api.h"

namespace apneauq {

typedef unsigned long long u64;

constexpr int kConfThreads = 256;
constexpr int kConfWaves = kConfThreads / kWave;
constexpr int kConfItems = 8;                       // consecutive sorted windows per lane: two 16-B loads of units
constexpr int kConfTile = kWave * kConfItems;       // windows per wave step
constexpr int kConfMaxSeg = 4096;                   // segments per row: 32 KiB of pairs in LDS
constexpr int kConfPerThread = kConfMaxSeg / kConfThreads;
constexpr int kConfMaxAlpha = 32, kConfMaxCuts = 64;
constexpr long long kConfPpm = 1000000;

struct ConfRow {
  const int* unit;             // (n,) unit of every sorted window
  const unsigned char* packed; // (n,) bit 0 = class
  const int* within;           // (n,) index of the window within its unit, or nullptr (cluster = "pooled")
  const int* ucount;           // (n_units,) windows per unit (with within)
  int n_units;
  int n;
  int span;                    // wave steps per segment
  u64 cal_thr;                 // a unit calibrates iff split_hash < cal_thr, in [0, 2^32]
};

// Roles of sorted windows [base, base + 8) below lim (<= n), base a multiple of 8: one bit per window in
// cal (calibrates), test and zm (class 1).
template <bool kSub>
__device__ __forceinline__ void conf_flags(const ConfRow& a, unsigned k1, unsigned k2, int base, int lim, unsigned& cal,
                                           unsigned& test, unsigned& zm) {
  cal = test = zm = 0u;
  if (base >= lim) return;
  int u[kConfItems], wi[kConfItems];
  u64 pk = 0ull;
  if (base + kConfItems <= a.n) {
    const int4 u0 = *reinterpret_cast<const int4*>(a.unit + base), u1 = *reinterpret_cast<const int4*>(a.unit + base + 4);
    u[0] = u0.x, u[1] = u0.y, u[2] = u0.z, u[3] = u0.w, u[4] = u1.x, u[5] = u1.y, u[6] = u1.z, u[7] = u1.w;
    pk = *reinterpret_cast<const u64*>(a.packed + base);
    if (kSub) {
      const int4 w0 = *reinterpret_cast<const int4*>(a.within + base), w1 = *reinterpret_cast<const int4*>(a.within + base + 4);
      wi[0] = w0.x, wi[1] = w0.y, wi[2] = w0.z, wi[3] = w0.w, wi[4] = w1.x, wi[5] = w1.y, wi[6] = w1.z, wi[7] = w1.w;
    }
  } else {
#pragma unroll
    for (int k = 0; k < kConfItems; ++k) {
      const bool ok = base + k < a.n;
      u[k] = ok ? a.unit[base + k] : 0;
      pk |= ok ? (u64)a.packed[base + k] << (8 * k) : 0ull;
      wi[k] = (kSub && ok) ? a.within[base + k] : 0;
    }
  }
#pragma unroll
  for (int k = 0; k < kConfItems; ++k) {
    if (base + k >= lim) continue;
    const unsigned mu = mix32((unsigned)u[k]);
    const bool cal_unit = (u64)mix32(k1 ^ mu) < a.cal_thr;
    bool c = cal_unit;
    if (kSub && cal_unit) {
      const unsigned cnt = (unsigned)u[k] < (unsigned)a.n_units ? (unsigned)a.ucount[u[k]] : 0u;
      c = wi[k] == (int)(((u64)mix32(k2 ^ mu) * (u64)cnt) >> 32);
    }
    cal |= (c ? 1u : 0u) << k;
    test |= (cal_unit ? 0u : 1u) << k;
    zm |= (unsigned)((pk >> (8 * k)) & 1ull) << k;
  }
}

// (class 0, class 1) counts of the windows in mask: class 0 in the low, class 1 in the high 32 bits
__device__ __forceinline__ u64 conf_pair(unsigned mask, unsigned zm) {
  return (u64)__popc(mask & ~zm) | ((u64)__popc(mask & zm) << 32);
}

// In-place exclusive scan of seg[0, n_seg) (n_seg <= kConfMaxSeg) by the whole block; returns the total.
__device__ __forceinline__ u64 conf_block_scan(u64* seg, int n_seg, u64* s_wave) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  const int first = (int)threadIdx.x * kConfPerThread;
  u64 loc = 0ull;
  for (int e = 0; e < kConfPerThread; ++e) loc += first + e < n_seg ? seg[first + e] : 0ull;
  u64 inc = loc;
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const u64 v = __shfl_up(inc, o, kWave);
    if (lane >= o) inc += v;
  }
  if (lane == kWave - 1) s_wave[wave] = inc;
  __syncthreads();
  u64 run = inc - loc, total = 0ull;
#pragma unroll
  for (int ww = 0; ww < kConfWaves; ++ww) {
    run += ww < wave ? s_wave[ww] : 0ull;
    total += s_wave[ww];
  }
  for (int e = 0; e < kConfPerThread; ++e)
    if (first + e < n_seg) {
      const u64 v = seg[first + e];
      seg[first + e] = run;
      run += v;
    }
  __syncthreads();
  return total;
}

template <bool kSub>
__global__ __launch_bounds__(kConfThreads) void conformal_select_kernel(ConfRow a, unsigned seed, int r0,
                                                                        const int* __restrict__ alpha_ppm, int n_alpha,
                                                                        int strata, int* __restrict__ totals,
                                                                        int* __restrict__ member) {
  __shared__ u64 s_seg[kConfMaxSeg];
  __shared__ u64 s_wave[kConfWaves], s_tot[2][kConfWaves];
  __shared__ int s_hit_seg[2 * kConfMaxAlpha], s_hit_need[2 * kConfMaxAlpha];
  const int row = blockIdx.x, lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  const int seg_len = a.span * kConfTile;
  const int n_seg = (a.n + seg_len - 1) / seg_len;
  const int n_target = strata * n_alpha;
  APNEAUQ_DASSERT(blockDim.x == kConfThreads && a.n >= 1 && n_seg <= kConfMaxSeg && n_alpha >= 1 &&
                  n_alpha <= kConfMaxAlpha && (strata == 1 || strata == 2));
  const unsigned k1 = split_key(seed, (unsigned)(r0 + row), kSplitSalt), k2 = split_key(seed, (unsigned)(r0 + row), kSplitSalt2);

  // walk: calibration pairs per segment (one stratum: every calibration window counts in the low field)
  u64 cal_all = 0ull, test_all = 0ull;
  for (int s = wave; s < n_seg; s += kConfWaves) {
    u64 cal_s = 0ull;
    const int lim = min(a.n, (s + 1) * seg_len);
    for (int t = 0; t < a.span; ++t) {
      unsigned cal, test, zm;
      conf_flags<kSub>(a, k1, k2, s * seg_len + t * kConfTile + lane * kConfItems, lim, cal, test, zm);
      cal_s += conf_pair(cal, zm);
      test_all += conf_pair(test, zm);
    }
    cal_all += cal_s;
    const u64 v = wave_sum(strata == 2 ? cal_s : (cal_s & 0xFFFFFFFFull) + (cal_s >> 32));
    if (lane == 0) s_seg[s] = v;
  }
  cal_all = wave_sum(cal_all);
  test_all = wave_sum(test_all);
  if (lane == 0) {
    s_tot[0][wave] = cal_all;
    s_tot[1][wave] = test_all;
  }
  __syncthreads();
  const u64 total = conf_block_scan(s_seg, n_seg, s_wave);
  if (threadIdx.x < 2) {
    u64 v = 0ull;
    for (int ww = 0; ww < kConfWaves; ++ww) v += s_tot[threadIdx.x][ww];
    totals[(long long)row * 4 + 2 * threadIdx.x] = (int)(unsigned)v;
    totals[(long long)row * 4 + 2 * threadIdx.x + 1] = (int)(unsigned)(v >> 32);
  }

  // ranks: locate the segment of every target by a binary search over the prefixes
  if ((int)threadIdx.x < n_target) {
    const int st = (int)threadIdx.x / n_alpha, ai = (int)threadIdx.x % n_alpha;
    const long long n_cal = st ? (long long)(total >> 32) : (long long)(total & 0xFFFFFFFFull);
    const long long keep = kConfPpm - min(max((long long)alpha_ppm[ai], 1ll), kConfPpm - 1);
    const long long k = ((n_cal + 1) * keep + kConfPpm - 1) / kConfPpm;
    int hit = -1, need = 0;
    if (k <= n_cal) {
      const unsigned target = (unsigned)(st ? n_cal - k + 1 : k);
      int lo = 0, hi = n_seg - 1;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const u64 inc = s_seg[mid + 1];  // mid + 1 <= hi <= n_seg - 1
        if ((st ? (unsigned)(inc >> 32) : (unsigned)inc) >= target) {
          hi = mid;
        } else {
          lo = mid + 1;
        }
      }
      hit = lo;
      need = (int)(target - (st ? (unsigned)(s_seg[lo] >> 32) : (unsigned)s_seg[lo]));
    } else {
      member[(long long)row * n_target + threadIdx.x] = -1;
    }
    s_hit_seg[threadIdx.x] = hit;
    s_hit_need[threadIdx.x] = need;
  }
  __syncthreads();

  // one wave walks the segment of a target again and finds the window of that rank
  for (int q = wave; q < n_target; q += kConfWaves) {
    const int s = s_hit_seg[q], need = s_hit_need[q], st = q / n_alpha;
    if (s < 0) continue;
    const int lim = min(a.n, (s + 1) * seg_len);
    int before = 0, found = -1;
    for (int t = 0; t < a.span; ++t) {
      const int base = s * seg_len + t * kConfTile + lane * kConfItems;
      unsigned cal, test, zm;
      conf_flags<kSub>(a, k1, k2, base, lim, cal, test, zm);
      const unsigned mask = strata == 2 ? (st ? cal & zm : cal & ~zm) : cal;
      const int c = __popc(mask);
      int inc = c;
#pragma unroll
      for (int o = 1; o < kWave; o <<= 1) {
        const int v = __shfl_up(inc, o, kWave);
        if (lane >= o) inc += v;
      }
      const int excl = before + inc - c;
      if (excl < need && need <= excl + c) {
        int seen = excl;
#pragma unroll
        for (int k = 0; k < kConfItems; ++k)
          if ((mask >> k) & 1u) {
            ++seen;
            if (seen == need) found = base + k;
          }
      }
      before += __shfl(inc, kWave - 1, kWave);
    }
    if (found >= 0) member[(long long)row * n_target + q] = found;
  }
}

template <bool kSub>
__global__ __launch_bounds__(kConfThreads) void conformal_count_kernel(ConfRow a, unsigned seed, int r0,
                                                                       const int* __restrict__ cuts, int n_cuts,
                                                                       int* __restrict__ out) {
  __shared__ u64 s_seg[kConfMaxSeg];
  __shared__ u64 s_wave[kConfWaves];
  const int row = blockIdx.x, lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  const int seg_len = a.span * kConfTile;
  const int n_seg = (a.n + seg_len - 1) / seg_len;
  APNEAUQ_DASSERT(blockDim.x == kConfThreads && a.n >= 1 && n_seg <= kConfMaxSeg && n_cuts >= 1 && n_cuts <= kConfMaxCuts);
  const unsigned k1 = split_key(seed, (unsigned)(r0 + row), kSplitSalt), k2 = split_key(seed, (unsigned)(r0 + row), kSplitSalt2);

  for (int s = wave; s < n_seg; s += kConfWaves) {
    u64 test_s = 0ull;
    const int lim = min(a.n, (s + 1) * seg_len);
    for (int t = 0; t < a.span; ++t) {
      unsigned cal, test, zm;
      conf_flags<kSub>(a, k1, k2, s * seg_len + t * kConfTile + lane * kConfItems, lim, cal, test, zm);
      test_s += conf_pair(test, zm);
    }
    const u64 v = wave_sum(test_s);
    if (lane == 0) s_seg[s] = v;
  }
  __syncthreads();
  const u64 total = conf_block_scan(s_seg, n_seg, s_wave);

  // T_z(cut) = test windows of the segments before the cut's segment + those of its segment below the cut
  for (int q = wave; q < n_cuts; q += kConfWaves) {
    const int cut = min(max(cuts[(long long)row * n_cuts + q], 0), a.n);
    const int s = cut / seg_len;
    u64 v = total;
    if (s < n_seg) {
      u64 part = 0ull;
      for (int t = 0; t < a.span; ++t) {
        unsigned cal, test, zm;
        conf_flags<kSub>(a, k1, k2, s * seg_len + t * kConfTile + lane * kConfItems, cut, cal, test, zm);
        part += conf_pair(test, zm);
      }
      v = s_seg[s] + wave_sum(part);
    }
    if (lane == 0) {
      out[((long long)row * n_cuts + q) * 2] = (int)(unsigned)v;
      out[((long long)row * n_cuts + q) * 2 + 1] = (int)(unsigned)(v >> 32);
    }
  }
}

int conformal_tile() { return kConfTile; }
int conformal_max_segments() { return kConfMaxSeg; }
int conformal_max_alpha() { return kConfMaxAlpha; }
int conformal_max_cuts() { return kConfMaxCuts; }

static ConfRow conf_row(const int* unit, const unsigned char* packed, const int* within, const int* ucount, int n_units,
                        int n, int span, unsigned long long cal_thr) {
  ConfRow a;
  a.unit = unit;
  a.packed = packed;
  a.within = within;
  a.ucount = ucount;
  a.n_units = n_units;
  a.n = n;
  a.span = span;
  a.cal_thr = cal_thr;
  return a;
}

hipError_t launch_conformal_select(const int* unit, const unsigned char* packed, const int* within, const int* ucount,
                                   int n_units, int n, int span, unsigned seed, int r0, int n_splits,
                                   unsigned long long cal_thr, const int* alpha_ppm, int n_alpha, int strata, int* totals,
                                   int* member, hipStream_t stream) {
  if (n_splits <= 0 || n <= 0) return hipSuccess;
  const ConfRow a = conf_row(unit, packed, within, ucount, n_units, n, span, cal_thr);
  if (within) {
    hipLaunchKernelGGL(conformal_select_kernel<true>, dim3(n_splits), dim3(kConfThreads), 0, stream, a, seed, r0, alpha_ppm,
                       n_alpha, strata, totals, member);
  } else {
    hipLaunchKernelGGL(conformal_select_kernel<false>, dim3(n_splits), dim3(kConfThreads), 0, stream, a, seed, r0,
                       alpha_ppm, n_alpha, strata, totals, member);
  }
  return hipGetLastError();
}

hipError_t launch_conformal_count(const int* unit, const unsigned char* packed, const int* within, const int* ucount,
                                  int n_units, int n, int span, unsigned seed, int r0, int n_splits,
                                  unsigned long long cal_thr, const int* cuts, int n_cuts, int* out, hipStream_t stream) {
  if (n_splits <= 0 || n <= 0) return hipSuccess;
  const ConfRow a = conf_row(unit, packed, within, ucount, n_units, n, span, cal_thr);
  if (within) {
    hipLaunchKernelGGL(conformal_count_kernel<true>, dim3(n_splits), dim3(kConfThreads), 0, stream, a, seed, r0, cuts,
                       n_cuts, out);
  } else {
    hipLaunchKernelGGL(conformal_count_kernel<false>, dim3(n_splits), dim3(kConfThreads), 0, stream, a, seed, r0, cuts,
                       n_cuts, out);
  }
  return hipGetLastError();
}

}  // namespace apneauq
