// Signal corruptions of the shift sweep on gfx950 (MI355X): K degraded, re-standardised copies of every window from
// one read of the clean set.  ops/shift.py corrupt_eager is the same arithmetic in torch float64.
//
// A window is (L, C), time-major; one wave owns one window, lane l holds the rows t = l, l + 64, ... (R = ceil(L / 64)
// of them) with their C channels, and a copy of the clean window sits in LDS for the two kinds that read a
// neighbour (flatline, delay).  Per channel, in fp64: mu / sigma of the clean window; per condition the corrupted
// value x' (the table in ops/shift.py), then (x' - mean') / (std' + 1e-8) with the moments of x'.  One rounding, to
// fp32 at the store; plain vector stores, no atomics.
//
// Moments (wave_moments): mean = x_0 + sum(x_t - x_0) / L and std = sqrt(sum((x_t - mean)^2) / L).  Taking the sums
// relative to the first step makes a constant channel exactly mean = x_0, std = 0, so a dead channel comes out as
// exact zeros.  A sum is: each lane adds its rows in ascending t, then the xor butterfly of wave_sum.  The emulation
// performs the same operations in the same order and this file is compiled with contraction off (no fma), but the
// two are not guaranteed to agree to the bit: on an MI355X the fp32 results were bitwise the rounded emulation in
// most cases, not all.  The tests hold the kernel to |got - ref64| <= 2^-23 |ref64| + 1e-12.
#include "common.h"
#include "uq_api.h"

#pragma clang fp contract(off)

namespace apneauq {
namespace shift {

constexpr int kWaves = 4, kThreads = kWaves * kWave;
constexpr double kEps = 1e-8;
// g = (S - 131070) / kNoiseScale: S the sum of four 16-bit uniforms, variance (65536^2 - 1) / 3
constexpr double kNoiseMean = 131070.0, kNoiseScale = 37837.22723720648;

enum Kind { kNone = 0, kNoise = 1, kFlatline = 2, kSpikes = 3, kDrift = 4, kClip = 5, kDelay = 6, kQuantize = 7 };

template <typename T, int C>
__device__ __forceinline__ void load_row(const T* __restrict__ p, double (&v)[C]) {
  if constexpr (C == 1 || C == 3) {
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = (double)p[c];
  } else {  // one access of C sizeof(T) bytes (16 B for fp32 at C = 4); the binding checks the alignment
    typedef T vec __attribute__((ext_vector_type(C)));
    const vec r = *reinterpret_cast<const vec*>(p);
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = (double)r[c];
  }
}

template <int C>
__device__ __forceinline__ void store_row(float* __restrict__ p, const float (&v)[C]) {
  if constexpr (C == 1 || C == 3) {
#pragma unroll
    for (int c = 0; c < C; ++c) p[c] = v[c];
  } else {
    typedef float vec __attribute__((ext_vector_type(C)));
    vec r;
#pragma unroll
    for (int c = 0; c < C; ++c) r[c] = v[c];
    *reinterpret_cast<vec*>(p) = r;
  }
}

// mean and population std over the L steps of one channel, v = this lane's rows of it (rows it does not hold count
// as 0)
template <int R>
__device__ __forceinline__ void wave_moments(const double (&v)[R], const bool (&ok)[R], int L, double& mean,
                                             double& sd) {
  const double pivot = __shfl(v[0], 0, kWave);  // lane 0 holds t = 0
  double acc = 0.0;
#pragma unroll
  for (int j = 0; j < R; ++j) acc += ok[j] ? v[j] - pivot : 0.0;
  mean = pivot + wave_sum(acc) / (double)L;
  acc = 0.0;
#pragma unroll
  for (int j = 0; j < R; ++j) {
    const double d = v[j] - mean;
    acc += ok[j] ? d * d : 0.0;
  }
  sd = __builtin_sqrt(wave_sum(acc) / (double)L);
}

template <typename T, int C, int R>
__global__ __launch_bounds__(kThreads) void shift_kernel(const T* __restrict__ x, float* __restrict__ out, long long n,
                                                         int L, int K, unsigned base, unsigned long long w_off,
                                                         ShiftConds cd, int restd) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long w = (long long)blockIdx.x * kWaves + wave;
  const bool active = w < n;
  double* sx = reinterpret_cast<double*>(smem_raw) + wave * L * C;  // this wave's clean window, [t][c]

  double xv[C][R];  // channel-major: a channel's rows are one array
  bool ok[R];
#pragma unroll
  for (int j = 0; j < R; ++j) {
    const int t = lane + j * kWave;
    ok[j] = active && t < L;
    double row[C];
#pragma unroll
    for (int c = 0; c < C; ++c) row[c] = 0.0;
    if (ok[j]) {
      load_row<T, C>(x + (w * L + t) * C, row);
#pragma unroll
      for (int c = 0; c < C; ++c) sx[t * C + c] = row[c];
    }
#pragma unroll
    for (int c = 0; c < C; ++c) xv[c][j] = row[c];
  }
  __syncthreads();
  if (!active) return;

  double mu[C], sg[C];
  float z0[R][C];  // the severity-0 output: what an untouched channel gets
#pragma unroll
  for (int c = 0; c < C; ++c) {
    wave_moments<R>(xv[c], ok, L, mu[c], sg[c]);
    const double den = sg[c] + kEps;
#pragma unroll
    for (int j = 0; j < R; ++j) z0[j][c] = (float)(restd ? (xv[c][j] - mu[c]) / den : xv[c][j]);
  }
  const unsigned wg = (unsigned)((unsigned long long)w + w_off);  // global window index

  for (int k = 0; k < K; ++k) {
    const int kind = cd.kind[k];
    const unsigned mask = cd.mask[k];
    const double p = cd.p[k];
    float o[R][C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      if (kind == kNone || !((mask >> c) & 1u)) {  // wave-uniform
#pragma unroll
        for (int j = 0; j < R; ++j) o[j][c] = z0[j][c];
        continue;
      }
      const unsigned key = shift_key(base, (unsigned)kind, (unsigned)c, wg);
      const double m = mu[c], s = sg[c];
      double y[R];
      // per-window quantities of the kind
      int i0 = 0, i1 = 0;
      double a = 0.0, b = 0.0;
      if (kind == kFlatline) {
        const double lf = __builtin_fmin(__builtin_fmax(__builtin_floor(p * (double)L + 0.5), 1.0), (double)L);
        const int len = (int)lf;
        i0 = (int)(((unsigned long long)shift_word(key, kShiftWindowCtr) * (unsigned long long)(L - len + 1)) >> 32);
        i1 = i0 + len;
        a = sx[max(i0 - 1, 0) * C + c];
      } else if (kind == kSpikes) {
        i0 = (int)__builtin_fmin(__builtin_fmax(__builtin_rint(p * 65536.0), 0.0), 65536.0);
        a = 6.0 * s;
      } else if (kind == kDrift) {
        a = (shift_word(key, kShiftWindowCtr) & 1u) ? p * s : -(p * s);
      } else if (kind == kClip || kind == kNoise || kind == kQuantize) {
        a = p * s;
        b = m + a;  // clip: upper bound
      } else if (kind == kDelay) {
        i0 = (int)__builtin_fmin(p, (double)(L - 1));
      }
#pragma unroll
      for (int j = 0; j < R; ++j) {
        const int t = lane + j * kWave;
        const double xt = xv[c][j];
        double v = xt;
        if (ok[j]) {
          switch (kind) {
            case kNoise: {
              const unsigned h0 = shift_word(key, ((unsigned)t << 2) | 0u);
              const unsigned h1 = shift_word(key, ((unsigned)t << 2) | 1u);
              const unsigned sum = (h0 & 0xFFFFu) + (h0 >> 16) + (h1 & 0xFFFFu) + (h1 >> 16);
              const double g = ((double)sum - kNoiseMean) / kNoiseScale;
              v = xt + a * g;
              break;
            }
            case kFlatline:
              v = (t >= i0 && t < i1) ? a : xt;
              break;
            case kSpikes: {
              const unsigned h = shift_word(key, (unsigned)t << 2);
              const double spike = ((h >> 16) & 1u) ? m + a : m - a;
              v = (int)(h & 0xFFFFu) < i0 ? spike : xt;
              break;
            }
            case kDrift:
              v = L > 1 ? xt + (a * (double)t) / (double)(L - 1) : xt;
              break;
            case kClip:
              v = __builtin_fmin(__builtin_fmax(xt, m - a), b);
              break;
            case kDelay:
              v = sx[max(t - i0, 0) * C + c];
              break;
            case kQuantize:
              v = a > 0.0 ? m + a * __builtin_rint((xt - m) / a) : xt;
              break;
            default:
              break;
          }
        }
        y[j] = v;
      }
      if (restd) {
        double m2, s2;
        wave_moments<R>(y, ok, L, m2, s2);
        const double den = s2 + kEps;
#pragma unroll
        for (int j = 0; j < R; ++j) o[j][c] = (float)((y[j] - m2) / den);
      } else {
#pragma unroll
        for (int j = 0; j < R; ++j) o[j][c] = (float)y[j];
      }
    }
    float* dst = out + ((long long)k * n + w) * L * C;
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const int t = lane + j * kWave;
      if (ok[j]) store_row<C>(dst + t * C, o[j]);
    }
  }
}

template <typename T, int C>
hipError_t launch_c(const T* x, float* out, long long n, int L, int K, unsigned base, unsigned long long w_off,
                    const ShiftConds& cd, int restd, hipStream_t stream) {
  const dim3 grid((unsigned)((n + kWaves - 1) / kWaves)), block(kThreads);
  const size_t lds = (size_t)kWaves * L * C * sizeof(double);
#define APNEAUQ_SHIFT_LAUNCH(R) \
  hipLaunchKernelGGL((shift_kernel<T, C, R>), grid, block, lds, stream, x, out, n, L, K, base, w_off, cd, restd)
  switch ((L + kWave - 1) / kWave) {
    case 1: APNEAUQ_SHIFT_LAUNCH(1); break;
    case 2: APNEAUQ_SHIFT_LAUNCH(2); break;
    case 3: APNEAUQ_SHIFT_LAUNCH(3); break;
    default: APNEAUQ_SHIFT_LAUNCH(4); break;
  }
#undef APNEAUQ_SHIFT_LAUNCH
  return hipGetLastError();
}

template <typename T>
hipError_t launch_t(const T* x, float* out, long long n, int L, int C, int K, unsigned base, unsigned long long w_off,
                    const ShiftConds& cd, int restd, hipStream_t stream) {
  switch (C) {
    case 1: return launch_c<T, 1>(x, out, n, L, K, base, w_off, cd, restd, stream);
    case 2: return launch_c<T, 2>(x, out, n, L, K, base, w_off, cd, restd, stream);
    case 3: return launch_c<T, 3>(x, out, n, L, K, base, w_off, cd, restd, stream);
    default: return launch_c<T, 4>(x, out, n, L, K, base, w_off, cd, restd, stream);
  }
}

}  // namespace shift

hipError_t launch_shift_corrupt(const void* x, bool x_is_double, long long n, int L, int C, const ShiftConds& conds,
                                int K, unsigned long long seed, unsigned long long window_offset, bool restandardize,
                                float* out, hipStream_t stream) {
  if (n == 0 || K == 0) return hipSuccess;
  if (n < 0 || n > (1ll << 27) || L < 1 || L > kShiftMaxL || C < 1 || C > kShiftMaxC || K < 0 || K > kShiftMaxK)
    return hipErrorInvalidValue;
  for (int k = 0; k < K; ++k)
    if (conds.kind[k] >= kShiftKinds) return hipErrorInvalidValue;
  const unsigned base = shift_base(seed);
  const int restd = restandardize ? 1 : 0;
  if (x_is_double)
    return shift::launch_t<double>(static_cast<const double*>(x), out, n, L, C, K, base, window_offset, conds, restd,
                                   stream);
  return shift::launch_t<float>(static_cast<const float*>(x), out, n, L, C, K, base, window_offset, conds, restd,
                                stream);
}

}  // namespace apneauq
