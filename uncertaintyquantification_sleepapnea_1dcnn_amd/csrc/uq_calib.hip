// Calibration and selective-prediction sums with an on-device bootstrap (gfx950).
//
// calib_prep       turns each window's (mean probability, uncertainty score, label) into one 16-byte
//                  record of integers: quantised probability, confidence bin, uncertainty bucket,
//                  label / prediction / correctness bits, quantised squared error and log-loss.  None of
//                  these change under resampling (the trick of uq_reduce.hip:bootstrap_kernel).
// calib_bootstrap  replicate b, slice g: gathers the records of draws [g n / G, (g+1) n / G) and
//                  histograms them.  Every column is an integer sum, so the (B, G, S) slabs add up to
//                  the same bits for any G, any wave schedule and any sharding of the windows.
//
// The scale constants and the code-word layout are mirrored in ops/calib.py (the eager emulation).
#include "common.h"
#include "uq_api.h"

namespace apneauq {

constexpr int kCalibMaxBins = 32;   // K
constexpr int kCalibMaxThr = 64;    // J
constexpr double kCalibPScale = 1073741824.0;   // 2^30: p_q, brier_q
constexpr double kCalibNllScale = 134217728.0;  // 2^27: nll_q (nll <= 16.2, fits 32 unsigned bits)

// code word (record word 1): conf_bin | unc_bucket << 5 | y << 12 | pred << 13 | correct << 14
constexpr int kCodeBucketShift = 5, kCodeYShift = 12, kCodePredShift = 13, kCodeCorrectShift = 14;

__global__ __launch_bounds__(256) void calib_prep_kernel(const float* __restrict__ p, const float* __restrict__ score,
                                                          const int* __restrict__ y, const float* __restrict__ thr,
                                                          int n, int n_bins, int n_thr, int4* __restrict__ rec) {
  __shared__ float s_thr[kCalibMaxThr];
  APNEAUQ_DASSERT(n_bins >= 1 && n_bins <= kCalibMaxBins && n_thr >= 0 && n_thr <= kCalibMaxThr);
  if ((int)threadIdx.x < n_thr) s_thr[threadIdx.x] = thr[threadIdx.x];
  __syncthreads();
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float pf = fminf(fmaxf(p[i], 0.f), 1.f);  // NaN -> 0
  const double pd = (double)pf;
  const int yy = y[i] != 0;
  const unsigned p_q = (unsigned)__double2ll_rn(pd * kCalibPScale);
  int bin = (int)(((unsigned long long)p_q * (unsigned)n_bins) >> 30);
  bin = min(bin, n_bins - 1);
  const float sc = score[i];
  int bucket = 0;
  for (int j = 0; j < n_thr; ++j) bucket += s_thr[j] < sc ? 1 : 0;
  const int pred = pf > 0.5f;
  const int correct = pred == yy;
  const double d = pd - (double)yy;
  const unsigned brier_q = (unsigned)__double2ll_rn(d * d * kCalibPScale);
  const double pt = fmin(fmax(pd, 1e-7), 1.0 - 1e-7);  // Keras BCE epsilon
  const double nll = -log(yy ? pt : 1.0 - pt);
  const unsigned nll_q = (unsigned)__double2ll_rn(nll * kCalibNllScale);
  const unsigned code = (unsigned)bin | ((unsigned)bucket << kCodeBucketShift) | ((unsigned)yy << kCodeYShift) |
                        ((unsigned)pred << kCodePredShift) | ((unsigned)correct << kCodeCorrectShift);
  rec[i] = make_int4((int)p_q, (int)code, (int)brier_q, (int)nll_q);
}

constexpr int kCalibThreads = 512;
constexpr int kCalibWaves = kCalibThreads / kWave;
constexpr int kCalibUnroll = 4;

// One wave's private histogram.  Two 32-bit counts share a 64-bit word (low half first), so a draw
// costs four LDS adds; a block sees at most n <= 2^27 draws, so no half can carry into the other.
struct CalibWaveHist {
  unsigned long long conf_cp[kCalibMaxBins];      // {count, positives}
  unsigned long long conf_sp[kCalibMaxBins];      // sum p_q
  unsigned long long buck_cc[kCalibMaxThr + 1];   // {count, correct}
  unsigned long long buck_pt[kCalibMaxThr + 1];   // {positives, true positives}
};
constexpr int kCalibHistWords = sizeof(CalibWaveHist) / sizeof(unsigned long long);

// Output columns, S = 3 K + 4 (J + 1) + 2:
//   [3 k + {0, 1, 2}]            confidence bin k: count, positives, sum p_q
//   [3 K + 4 u + {0, 1, 2, 3}]   uncertainty bucket u: count, correct, positives, true positives
//   [S - 2], [S - 1]             sum brier_q, sum nll_q
// rec holds the records of global windows [lo, lo + n_loc); draws outside are skipped (bootstrap_kernel<true>).
__global__ __launch_bounds__(kCalibThreads) void calib_bootstrap_kernel(const int4* __restrict__ rec,
                                                                        const int* __restrict__ idx, unsigned seed,
                                                                        int n, int lo, int n_loc, int n_bins,
                                                                        int n_thr, long long* __restrict__ out) {
  __shared__ CalibWaveHist hist[kCalibWaves];
  __shared__ unsigned long long tot[2][kCalibWaves];
  const int b = blockIdx.x, g = blockIdx.y, n_slice = gridDim.y;
  APNEAUQ_DASSERT(blockDim.x == kCalibThreads && n > 0 && n_bins >= 1 && n_bins <= kCalibMaxBins && n_thr >= 0 &&
                  n_thr <= kCalibMaxThr && lo >= 0 && n_loc >= 0);
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  {
    unsigned long long* hw = reinterpret_cast<unsigned long long*>(hist);
    for (int q = threadIdx.x; q < kCalibWaves * kCalibHistWords; q += kCalibThreads) hw[q] = 0ull;
  }
  __syncthreads();
  CalibWaveHist& h = hist[wave];
  unsigned long long s_brier = 0ull, s_nll = 0ull;
  const unsigned bkey = boot_key(seed, (unsigned)b);
  const long long j0 = (long long)g * n / n_slice, j1 = (long long)(g + 1) * n / n_slice;
  const int* idx_b = idx ? idx + (long long)b * n : nullptr;
  for (long long jb = j0 + threadIdx.x; jb < j1; jb += (long long)kCalibUnroll * kCalibThreads) {
    unsigned k[kCalibUnroll];
    bool ok[kCalibUnroll];
#pragma unroll
    for (int u = 0; u < kCalibUnroll; ++u) {
      const long long j = jb + (long long)u * kCalibThreads;
      unsigned raw = 0xFFFFFFFFu;
      if (j < j1) {
        if (idx_b) {
          raw = (unsigned)idx_b[j];
        } else {
          raw = boot_draw(bkey, (unsigned)j, n);
        }
      }
      k[u] = raw - (unsigned)lo;
      ok[u] = j < j1 && raw < (unsigned)n && k[u] < (unsigned)n_loc;
    }
    int4 r[kCalibUnroll];
#pragma unroll
    for (int u = 0; u < kCalibUnroll; ++u) r[u] = ok[u] ? rec[k[u]] : make_int4(0, 0, 0, 0);
#pragma unroll
    for (int u = 0; u < kCalibUnroll; ++u) {
      if (!ok[u]) continue;
      const unsigned code = (unsigned)r[u].y;
      const int bin = min((int)(code & 31u), n_bins - 1);
      const int bucket = min((int)((code >> kCodeBucketShift) & 127u), n_thr);
      const unsigned long long yy = (code >> kCodeYShift) & 1u, pred = (code >> kCodePredShift) & 1u,
                               correct = (code >> kCodeCorrectShift) & 1u;
      atomicAdd(&h.conf_cp[bin], 1ull | (yy << 32));
      atomicAdd(&h.conf_sp[bin], (unsigned long long)(unsigned)r[u].x);
      atomicAdd(&h.buck_cc[bucket], 1ull | (correct << 32));
      if (yy) atomicAdd(&h.buck_pt[bucket], 1ull | (pred << 32));
      s_brier += (unsigned long long)(unsigned)r[u].z;
      s_nll += (unsigned long long)(unsigned)r[u].w;
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    s_brier += __shfl_xor(s_brier, o, kWave);
    s_nll += __shfl_xor(s_nll, o, kWave);
  }
  if (lane == 0) {
    tot[0][wave] = s_brier;
    tot[1][wave] = s_nll;
  }
  __syncthreads();
  // fixed-order combine of the wave histograms: one output column per thread
  const int n_conf = 3 * n_bins, n_buck = 4 * (n_thr + 1), n_col = n_conf + n_buck + 2;
  const int c = threadIdx.x;
  if (c < n_col) {
    unsigned long long v = 0ull;
    for (int w = 0; w < kCalibWaves; ++w) {
      unsigned long long x;
      if (c < n_conf) {
        const int bin = c / 3, f = c - 3 * bin;
        x = f == 2 ? hist[w].conf_sp[bin] : (f == 0 ? (hist[w].conf_cp[bin] & 0xFFFFFFFFull) : (hist[w].conf_cp[bin] >> 32));
      } else if (c < n_conf + n_buck) {
        const int q = c - n_conf, bucket = q >> 2, f = q & 3;
        const unsigned long long word = f < 2 ? hist[w].buck_cc[bucket] : hist[w].buck_pt[bucket];
        x = (f & 1) ? (word >> 32) : (word & 0xFFFFFFFFull);
      } else {
        x = tot[c - n_conf - n_buck][w];
      }
      v += x;
    }
    out[((long long)b * n_slice + g) * n_col + c] = (long long)v;
  }
}

hipError_t launch_calib_prep(const float* p, const float* score, const int* y, const float* thr, int n, int n_bins,
                             int n_thr, int* rec, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(calib_prep_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, p, score, y, thr, n, n_bins, n_thr,
                     reinterpret_cast<int4*>(rec));
  return hipGetLastError();
}

hipError_t launch_calib_bootstrap(const int* rec, const int* idx, unsigned seed, int n, int lo, int n_loc, int n_boot,
                                  int n_bins, int n_thr, int slices, long long* out, hipStream_t stream) {
  if (n_boot <= 0 || n <= 0) return hipSuccess;
  hipLaunchKernelGGL(calib_bootstrap_kernel, dim3(n_boot, slices), dim3(kCalibThreads), 0, stream,
                     reinterpret_cast<const int4*>(rec), idx, seed, n, lo, n_loc, n_bins, n_thr, out);
  return hipGetLastError();
}

}  // namespace apneauq
