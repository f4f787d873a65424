// Pass / member-count convergence of the uncertainty metrics from one (T, n) prediction set (gfx950).
//
// converge   for every order r (a permutation of the T passes; its first k entries are a k-subset) and
//            every requested count k, the sums over the windows of the subset's metrics: (R, K, 11) int64
//            with columns n_valid, n_y1, var_q, var_q | y = 0, var_q | y = 1, H_q, EH_q, MI_q, correct,
//            flips, shift_q.  Float quantities are computed per window in fp64 and quantised as
//            rint(x 2^40); every sum over windows is an integer add, so the result does not depend on the
//            grid, on rep_groups, on the schedule or on how the windows are sharded (shards add exactly).
//
// The scale constant, the column layout and the limits are mirrored in ops/converge.py (the eager
// emulation).
#include "common.h"
#include "uq_api.h"

namespace apneauq {

constexpr int kCvThreads = 256;
constexpr int kCvWaves = kCvThreads / kWave;
constexpr int kCvCols = 11;
constexpr int kCvMaxT = 128;
constexpr double kCvScale = 1099511627776.0;      // 2^40: a term is at most 2^40, 2^22 windows stay below 2^62
constexpr double kCvEntScale = 4503599627370496.0;   // 2^52: a pass's entropy (<= ln 2) as an integer, 128 fit int64
constexpr int kCvPlaneBytes = kWave * (8 + 4);    // one pass of a tile: 64 entropies (int64) and 64 probabilities

// rint(min(x, 1) 2^40) of x >= 0, round to nearest even: adding 1.5 * 2^52 leaves the integer in the low
// mantissa bits.  Every quantised quantity of probabilities in [0, 1] is at most 1 (var <= 1/4, H <= ln 2,
// |mean_k - mean_T| <= 1); the clamp keeps a term at 2^40 for any other input.
__device__ __forceinline__ long long cv_q(double x) {
  const double magic = 6755399441055744.0;
  return __double_as_longlong(fmin(x, 1.0) * kCvScale + magic) - __double_as_longlong(magic);
}

// Sums over the wave of seven per-lane values at once: each of the first three steps halves the values a
// lane carries (it keeps the half that its lane bit selects and hands the other half over), so ten 64-bit
// shuffles do the work of forty-two.  Lane l ends with the wave's sum of value (l >> 3) & 7.
__device__ __forceinline__ long long cv_wave_sum7(const long long (&a)[8], int lane) {
  long long b[4], c[2];
  const bool h5 = lane & 32, h4 = lane & 16, h3 = lane & 8;
#pragma unroll
  for (int i = 0; i < 4; ++i) b[i] = (h5 ? a[i + 4] : a[i]) + __shfl_xor(h5 ? a[i] : a[i + 4], 32, kWave);
#pragma unroll
  for (int i = 0; i < 2; ++i) c[i] = (h4 ? b[i + 2] : b[i]) + __shfl_xor(h4 ? b[i] : b[i + 2], 16, kWave);
  long long d = (h3 ? c[1] : c[0]) + __shfl_xor(h3 ? c[0] : c[1], 8, kWave);
#pragma unroll
  for (int o = 4; o >= 1; o >>= 1) d += __shfl_xor(d, o, kWave);
  return d;
}

// uq/metrics.py binary_entropy_nats in fp64: clip p and 1 - p to [1e-10, 1 - 1e-10], -sum x log x.  The
// renormalisation by pc + qc is left out: that sum is 1 within one ulp for every p (also for p outside
// [0, 1], where one side clips to 1e-10 and the other to 1 - 1e-10), which moves the entropy by less than
// 1e-15, a thousandth of a quantum.
__device__ __forceinline__ double cv_entropy(double p) {
  const double lo = 1e-10, hi = 1.0 - 1e-10;
  const double a = fmin(fmax(p, lo), hi), b = fmin(fmax(1.0 - p, lo), hi);
  return -(a * log(a) + b * log(b));
}

// A workgroup owns a tile of 64 windows (lane = window) and the replicate group blockIdx.y.  Its four
// waves stage the tile's T probabilities and their entropies into LDS as [t][64] planes (each row of probs
// is read once per replicate group, 256 B per wave-load).  A pass's entropy is kept as the integer
// rint(h 2^52): the entropy sum of a subset is then exact and does not depend on the order of its passes, as
// the sums of dyadic probabilities do not.  After the barrier wave w takes the orders
// blockIdx.y * 4 + w, + 4 gridDim.y, ...  It walks orders[r, 0..T): the pass index is wave-uniform, so the
// LDS address t * 64 + lane has no bank conflict and nothing is indexed dynamically in registers.  At each
// requested count the lane's window gives its eleven terms, the wave sums them (ballots for the counts,
// cv_wave_sum7 for the quantised columns) and eleven lanes add one column each to out[r, k, :].
//
// A window with a non-finite probability in any pass contributes to no column.  Pass indices are clamped
// to [0, T), so that no order can address LDS outside the planes; counts that are not ascending values in
// 1..T simply give no output for the entries that are never reached.
__global__ __launch_bounds__(kCvThreads) void converge_kernel(const float* __restrict__ probs,
                                                              const int* __restrict__ y,
                                                              const int* __restrict__ orders,
                                                              const int* __restrict__ counts, int t_count, int n,
                                                              int n_rep, int n_cnt, long long* __restrict__ out) {
  extern __shared__ long long cv_lds[];
  APNEAUQ_DASSERT(blockDim.x == kCvThreads && t_count >= 1 && t_count <= kCvMaxT && n >= 1 && n_cnt >= 1);
  long long* hs = cv_lds;                                                  // [T][64] int64
  float* ps = reinterpret_cast<float*>(cv_lds + (size_t)t_count * kWave);  // [T][64] fp32
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long long j = (long long)blockIdx.x * kWave + lane;
  const bool in = j < n;
  const long long jj = in ? j : n - 1;   // idle lanes read a valid element
  for (int t = wave; t < t_count; t += kCvWaves) {
    const float p = probs[(long long)t * n + jj];
    ps[t * kWave + lane] = p;
    const bool fin = fabsf(p) <= 3.402823466e38f;   // false for NaN and +-inf
    hs[t * kWave + lane] = __double2ll_rn(cv_entropy(fin ? (double)p : 0.5) * kCvEntScale);
  }
  __syncthreads();
  // all T passes in the canonical order 0..T-1: validity, mean and label
  bool ok = in;
  double s_all = 0.0;
  for (int t = 0; t < t_count; ++t) {
    const float p = ps[t * kWave + lane];
    ok = ok && (fabsf(p) <= 3.402823466e38f);   // false for NaN and +-inf
    s_all += (double)p;
  }
  const double t_d = (double)t_count;
  const double mean_all = s_all * (1.0 / t_d);
  const bool lab_all = 2.0 * s_all > t_d;
  const bool y1 = y[jj] != 0;
  const long long n_valid = __popcll(__ballot(ok));
  const long long n_y1 = __popcll(__ballot(ok && y1));
  if (n_valid == 0) return;
  // the column that this lane adds: lanes 0, 8, .., 48 hold the wave's sums of a[0..6] below, lanes 1..4 the counts
  const int slot = lane >> 3;
  const bool sum_lane = (lane & 7) == 0 && slot < 7;
  const int col = sum_lane ? (0x3A76542 >> (4 * slot)) & 15 : (lane >= 1 && lane <= 4) ? (0x9810 >> (4 * (lane - 1))) & 15 : -1;
  for (int r = blockIdx.y * kCvWaves + wave; r < n_rep; r += gridDim.y * kCvWaves) {
    const int* ord = orders + (long long)r * t_count;
    double s1 = 0.0, s2 = 0.0;
    long long sh = 0;
    int kc = 0;
    int next = counts[0];
    for (int i = 0; i < t_count; ++i) {
      const int t = min(max(ord[i], 0), t_count - 1);
      const double p = (double)ps[t * kWave + lane];
      s1 += p;
      s2 += p * p;   // exact in fp64: p is an fp32 value
      sh += hs[t * kWave + lane];
      if (i + 1 != next) continue;
      const double kd = (double)(i + 1), rk = 1.0 / kd;
      const double mean = s1 * rk;
      const double var = fmax((kd * s2 - s1 * s1) * (rk * rk), 0.0);
      const double ent = cv_entropy(mean);
      const double eh = (double)sh * (1.0 / kCvEntScale) * rk;
      const bool lab = 2.0 * s1 > kd;
      long long a[8];
      a[0] = ok ? cv_q(var) : 0;                          // column 2
      a[1] = y1 ? a[0] : 0;                               // 4
      a[2] = ok ? cv_q(ent) : 0;                          // 5
      a[3] = ok ? cv_q(eh) : 0;                           // 6
      a[4] = ok ? cv_q(fmax(ent - eh, 0.0)) : 0;          // 7
      a[5] = ok ? cv_q(fabs(mean - mean_all)) : 0;        // 10
      a[6] = y1 ? 0 : a[0];                               // 3
      a[7] = 0;
      const long long sum = cv_wave_sum7(a, lane);
      const long long correct = __popcll(__ballot(ok && lab == y1));
      const long long flips = __popcll(__ballot(ok && lab != lab_all));
      const long long v = sum_lane ? sum : lane == 1 ? n_valid : lane == 2 ? n_y1 : lane == 3 ? correct : flips;
      if (col >= 0 && v != 0)
        atomicAdd(reinterpret_cast<unsigned long long*>(&out[((long long)r * n_cnt + kc) * kCvCols + col]),
                  (unsigned long long)v);
      ++kc;
      next = kc < n_cnt ? counts[kc] : 0x7FFFFFFF;
    }
  }
}

int converge_lds_bytes(int t_count) { return t_count * kCvPlaneBytes; }

// out (R, K, 11) must be zero.  Limits (checked by the binding): T <= 128, K <= 32, R <= 4096, n <= 2^22.
hipError_t launch_converge(const float* probs, const int* y, const int* orders, const int* counts, int t_count, int n,
                           int n_rep, int n_cnt, int rep_groups, long long* out, hipStream_t stream) {
  if (n <= 0 || t_count <= 0 || n_rep <= 0 || n_cnt <= 0) return hipSuccess;
  if (t_count > kCvMaxT || rep_groups < 1 || rep_groups > 65535) return hipErrorInvalidValue;
  const int lds = converge_lds_bytes(t_count);
  if (lds > 64 * 1024) {  // above the default dynamic LDS limit: 98,304 B at T = 128
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(converge_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, kCvMaxT * kCvPlaneBytes);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(converge_kernel, dim3((n + kWave - 1) / kWave, rep_groups), dim3(kCvThreads), lds, stream, probs,
                     y, orders, counts, t_count, n, n_rep, n_cnt, out);
  return hipGetLastError();
}

}  // namespace apneauq
