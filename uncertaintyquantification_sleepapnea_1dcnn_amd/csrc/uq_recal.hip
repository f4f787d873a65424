// Post-hoc recalibration of a (T, n) prediction set (gfx950): the sums a damped Newton fit needs, at several
// candidate parameter vectors at once, and the one-pass application of the fitted map.
//
// With p_c = clip(p, 1e-7, 1 - 1e-7) (fp64 on the fp32 value), l1 = log p_c, l0 = log1p(-p_c), f = (l1, -l0, 1) and
// theta = (a, b, c):  u_t = a l1_t - b l0_t + c,  e = exp(-|u|),  q = sigmoid(u) and 1 - q both from e (no
// cancellation),  s = q (1 - q) = e / (1 + e)^2.
//
// recal_sums   out (F, Q, 12) fp64: n_valid, n_y1, loss, g_a, g_b, g_c, H_aa, H_ab, H_ac, H_bb, H_bc, H_cc summed over
//              the valid windows (all T values finite, label 0 or 1, fold code in [0, F)) of fold g at candidate q.
//              joint (0):  pbar = mean_t q_t, loss = -log pbar (y = 1) or -log(1 - pbar), gv = mean_t s f,
//                          G = mean_t s (1 - 2 q) f f^T, r = -1 / pbar or 1 / (1 - pbar), g = r gv, H = r^2 gv gv^T + r G.
//              member (1): loss = mean_t softplus(-/+ u_t), g = mean_t (q - y) f, H = mean_t s f f^T.
//              A workgroup of four waves owns a tile of 64 windows (lane = window): the waves compute l1 and l0 of
//              the tile's T rows once into [t][2][64] fp64 planes in LDS, then wave w walks the planes in the order
//              t = 0..T-1 for the candidates w, w + 4, ..., two candidates per walk.  Per fold code present in the
//              tile the twelve columns are reduced over the wave (xor butterfly: every lane ends with the same bits)
//              and lane j adds column j into the workgroup's (F, Q, 12) accumulator in LDS.
//              Every multiply-add of the walk is an explicit fma, and a product that reaches a plain add or subtract
//              (exp, log1p, e inv, s, w) first passes an empty register-constraint asm statement, which the build's FMA
//              contraction cannot see through: the one- and two-candidate walks round alike by construction, and a
//              candidate's column does not depend on its neighbours.
// recal_apply  out (T, n) fp32 = sigmoid(a l1 - b l0 + c) with the theta of the window's fold; NaN for a non-finite
//              input or a fold code outside [0, F).  One pass over the flat array, 16 bytes per lane.
//
// Grid invariance of recal_sums: the windows are cut into ranges of range_len windows (a function of n only,
// ops/recal.py range_len); a range is accumulated in tile order by whichever workgroup takes it and stored with
// plain stores into its own partial; recal_reduce adds the partials in range order.  No floating-point atomics.
#include "common.h"
#include "uq_api.h"

namespace apneauq {

constexpr int kRcThreads = 256;
constexpr int kRcWaves = kRcThreads / kWave;
constexpr int kRcWT = 64;      // windows per tile
constexpr int kRcCols = 12;    // columns of a (fold, candidate) slot
constexpr int kRcMaxT = 128;
constexpr int kRcMaxQ = 64;
constexpr int kRcMaxF = 16;
constexpr int kRcMaxLds = 160 * 1024;
constexpr double kRcEps = 1e-7;

// planes [T][2][64] fp64, accumulator [F][Q][12] fp64, non-finite flags [4][64] int
__host__ __device__ constexpr long long rc_lds_bytes(int T, int F, int Q) {
  return (long long)T * 2 * kRcWT * 8 + (long long)F * Q * kRcCols * 8 + kRcWaves * kRcWT * 4;
}

// A product that feeds a plain add or subtract is kept in a register of its own (the build contracts a * b + c into
// an FMA wherever it sees one; nothing is fused across the empty asm), as uq_laplace.hip does for its logit.
__device__ __forceinline__ double rc_rounded(double v) {
  asm volatile("" : "+v"(v));
  return v;
}

// One walk of the tile's planes for NC candidates; col[c] = loss, g (3), H (6 upper) of this lane's window.
template <int OBJ, int NC>
__device__ __forceinline__ void rc_walk(const double* __restrict__ pl, int T, int lane, const double (&th)[NC][3],
                                        bool y1, double (&col)[NC][10]) {
  double a0[NC], a1[NC], g0[NC], g1[NC], g2[NC], h00[NC], h01[NC], h02[NC], h11[NC], h12[NC], h22[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c)
    a0[c] = a1[c] = g0[c] = g1[c] = g2[c] = h00[c] = h01[c] = h02[c] = h11[c] = h12[c] = h22[c] = 0.0;
  for (int t = 0; t < T; ++t) {
    const double l1 = pl[(2 * t) * kRcWT + lane];
    const double m0 = -pl[(2 * t + 1) * kRcWT + lane];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const double u = fma(th[c][0], l1, fma(th[c][1], m0, th[c][2]));
      const double e = rc_rounded(exp(-fabs(u)));  // whatever the library's last operation is, it stays its own
      const double inv = 1.0 / (1.0 + e);
      const double ei = rc_rounded(e * inv);
      const bool pos = u >= 0.0;
      const double q = pos ? inv : ei;
      const double o = pos ? ei : inv;
      const double s = rc_rounded(ei * inv);
      if (OBJ == 0) {
        const double w = rc_rounded(s * (o - q));
        const double w1 = w * l1, w0 = w * m0;
        a0[c] += q;
        a1[c] += o;
        g0[c] = fma(s, l1, g0[c]);
        g1[c] = fma(s, m0, g1[c]);
        g2[c] += s;
        h00[c] = fma(w1, l1, h00[c]);
        h01[c] = fma(w1, m0, h01[c]);
        h02[c] = fma(w, l1, h02[c]);
        h11[c] = fma(w0, m0, h11[c]);
        h12[c] = fma(w, m0, h12[c]);
        h22[c] += w;
      } else {
        const double z = y1 ? -u : u;
        const double d = y1 ? -o : q;
        const double s1 = s * l1, s0 = s * m0;
        a0[c] += (z > 0.0 ? z : 0.0) + rc_rounded(log1p(e));
        g0[c] = fma(d, l1, g0[c]);
        g1[c] = fma(d, m0, g1[c]);
        g2[c] += d;
        h00[c] = fma(s1, l1, h00[c]);
        h01[c] = fma(s1, m0, h01[c]);
        h02[c] = fma(s, l1, h02[c]);
        h11[c] = fma(s0, m0, h11[c]);
        h12[c] = fma(s, m0, h12[c]);
        h22[c] += s;
      }
    }
  }
  const double td = (double)T;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const double v0 = g0[c] / td, v1 = g1[c] / td, v2 = g2[c] / td;
    const double m00 = h00[c] / td, m01 = h01[c] / td, m02 = h02[c] / td, m11 = h11[c] / td, m12 = h12[c] / td,
                 m22 = h22[c] / td;
    if (OBJ == 0) {
      const double pbar = a0[c] / td, obar = a1[c] / td;
      const double hit = y1 ? pbar : obar, miss = y1 ? obar : pbar;  // loss = -log(hit), hit + miss = 1
      const double r = y1 ? -1.0 / hit : 1.0 / hit;
      const double k = r * r;
      col[c][0] = hit > 0.5 ? -log1p(-miss) : -log(hit);
      col[c][1] = r * v0;
      col[c][2] = r * v1;
      col[c][3] = r * v2;
      const double k0 = k * v0, k1 = k * v1, k2 = k * v2;
      col[c][4] = fma(k0, v0, r * m00);
      col[c][5] = fma(k0, v1, r * m01);
      col[c][6] = fma(k0, v2, r * m02);
      col[c][7] = fma(k1, v1, r * m11);
      col[c][8] = fma(k1, v2, r * m12);
      col[c][9] = fma(k2, v2, r * m22);
    } else {
      col[c][0] = a0[c] / td;
      col[c][1] = v0;
      col[c][2] = v1;
      col[c][3] = v2;
      col[c][4] = m00;
      col[c][5] = m01;
      col[c][6] = m02;
      col[c][7] = m11;
      col[c][8] = m12;
      col[c][9] = m22;
    }
  }
}

// Adds this tile's windows into acc[fold][q][0..12): one wave reduction per fold code present in the tile.
__device__ __forceinline__ void rc_add(double* __restrict__ acc, int Q, int q, int lane, bool valid, bool y1, int fc,
                                       const double (&col)[10]) {
  unsigned long long m = __ballot(valid);
  while (m) {
    const int leader = __ffsll((long long)m) - 1;
    const int fcl = __shfl(fc, leader, kWave);
    const bool sel = valid && fc == fcl;
    m &= ~__ballot(sel);
    double mine = 0.0;
    {
      const double v = wave_sum(sel ? 1.0 : 0.0);
      if (lane == 0) mine = v;
    }
    {
      const double v = wave_sum(sel && y1 ? 1.0 : 0.0);
      if (lane == 1) mine = v;
    }
#pragma unroll
    for (int j = 0; j < 10; ++j) {
      const double v = wave_sum(sel ? col[j] : 0.0);
      if (lane == j + 2) mine = v;
    }
    // lane j is the only thread that ever touches column j of a slot this wave owns
    if (lane < kRcCols) acc[((long long)fcl * Q + q) * kRcCols + lane] += mine;
  }
}

template <int OBJ>
__global__ __launch_bounds__(kRcThreads) void recal_sums_kernel(const float* __restrict__ probs,
                                                                const uint8_t* __restrict__ y,
                                                                const int* __restrict__ fold,
                                                                const double* __restrict__ thetas, long long n, int T,
                                                                int Q, int F, long long range_len, int n_ranges,
                                                                double* __restrict__ part) {
  extern __shared__ double rc_lds[];
  APNEAUQ_DASSERT(blockDim.x == kRcThreads && T >= 1 && T <= kRcMaxT && Q >= 1 && Q <= kRcMaxQ && F >= 1 &&
                  F <= kRcMaxF && range_len >= 1);
  double* pl = rc_lds;                                         // [T][2][64]: l1, l0
  double* acc = pl + (long long)T * 2 * kRcWT;                 // [F][Q][12]
  int* bad = reinterpret_cast<int*>(acc + (long long)F * Q * kRcCols);  // [4][64] a row of the wave was not finite
  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long long slot = (long long)F * Q * kRcCols;

  for (int range = blockIdx.x; range < n_ranges; range += gridDim.x) {
    if (lane < kRcCols)
      for (int q = wave; q < Q; q += kRcWaves)
        for (int f = 0; f < F; ++f) acc[((long long)f * Q + q) * kRcCols + lane] = 0.0;
    const long long w0 = (long long)range * range_len;
    const long long w1 = w0 + range_len < n ? w0 + range_len : n;
    for (long long base = w0; base < w1; base += kRcWT) {
      const long long w = base + lane;
      const bool in = w < w1;
      __syncthreads();  // the previous tile's walks are done
      int nf = 0;
      for (int t0 = wave; t0 < T; t0 += 4 * kRcWaves) {
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int t = t0 + kRcWaves * j;
          v[j] = (in && t < T) ? probs[(long long)t * n + w] : 0.5f;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int t = t0 + kRcWaves * j;
          if (t < T) {
            const bool fin = isfinite(v[j]);
            double p = fin ? (double)v[j] : 0.5;
            p = p < kRcEps ? kRcEps : (p > 1.0 - kRcEps ? 1.0 - kRcEps : p);
            pl[(2 * t) * kRcWT + lane] = log(p);
            pl[(2 * t + 1) * kRcWT + lane] = log1p(-p);
            nf |= !fin;
          }
        }
      }
      bad[wave * kRcWT + lane] = nf;
      __syncthreads();
      const unsigned yv = in ? (unsigned)y[w] : 2u;
      const int fc = in ? (fold ? fold[w] : 0) : -1;
      const int anybad = bad[lane] | bad[kRcWT + lane] | bad[2 * kRcWT + lane] | bad[3 * kRcWT + lane];
      const bool valid = in && !anybad && yv <= 1u && fc >= 0 && fc < F;
      const bool y1 = yv == 1u;
      if (__ballot(valid) == 0) continue;
      for (int q0 = wave; q0 < Q; q0 += 2 * kRcWaves) {
        const int q1 = q0 + kRcWaves;
        if (q1 < Q) {
          double th[2][3], col[2][10];
#pragma unroll
          for (int i = 0; i < 3; ++i) {
            th[0][i] = thetas[q0 * 3 + i];
            th[1][i] = thetas[q1 * 3 + i];
          }
          rc_walk<OBJ, 2>(pl, T, lane, th, y1, col);
          rc_add(acc, Q, q0, lane, valid, y1, fc, col[0]);
          rc_add(acc, Q, q1, lane, valid, y1, fc, col[1]);
        } else {
          double th[1][3], col[1][10];
#pragma unroll
          for (int i = 0; i < 3; ++i) th[0][i] = thetas[q0 * 3 + i];
          rc_walk<OBJ, 1>(pl, T, lane, th, y1, col);
          rc_add(acc, Q, q0, lane, valid, y1, fc, col[0]);
        }
      }
    }
    double* out = part + (long long)range * slot;
    if (lane < kRcCols)
      for (int q = wave; q < Q; q += kRcWaves)
        for (int f = 0; f < F; ++f) {
          const long long i = ((long long)f * Q + q) * kRcCols + lane;
          out[i] = acc[i];
        }
  }
}

// out (F Q 12): the range partials added in range order
__global__ __launch_bounds__(kRcThreads) void recal_reduce_kernel(const double* __restrict__ part, int n_ranges,
                                                                  int n_out, double* __restrict__ out) {
  const int e = blockIdx.x * kRcThreads + threadIdx.x;
  if (e >= n_out) return;
  double s = 0.0;
  for (int r = 0; r < n_ranges; ++r) s += part[(long long)r * n_out + e];
  out[e] = s;
}

// Four consecutive values of the flat (T, n) array per thread; total = T n.
__global__ __launch_bounds__(kRcThreads) void recal_apply_kernel(const float* __restrict__ probs,
                                                                 const int* __restrict__ fold,
                                                                 const double* __restrict__ thetas, long long n,
                                                                 long long total, int F, float* __restrict__ out) {
  const long long i = ((long long)blockIdx.x * kRcThreads + threadIdx.x) * 4;
  if (i >= total) return;
  const bool full = i + 4 <= total;
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  if (full) {
    const f32x4 x = *reinterpret_cast<const f32x4*>(probs + i);
    v[0] = x[0];
    v[1] = x[1];
    v[2] = x[2];
    v[3] = x[3];
  } else {
    for (int j = 0; j < 4; ++j)
      if (i + j < total) v[j] = probs[i + j];
  }
  long long w = i % n;
  float r[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float res = __int_as_float(0x7FC00000);
    if (i + j < total) {
      const int fc = fold ? fold[w] : 0;
      if (isfinite(v[j]) && fc >= 0 && fc < F) {
        double p = (double)v[j];
        p = p < kRcEps ? kRcEps : (p > 1.0 - kRcEps ? 1.0 - kRcEps : p);
        const double* th = thetas + (long long)fc * 3;
        const double u = fma(th[0], log(p), fma(th[1], -log1p(-p), th[2]));
        const double e = exp(-fabs(u));
        const double inv = 1.0 / (1.0 + e);
        res = (float)(u >= 0.0 ? inv : e * inv);
      }
    }
    r[j] = res;
    if (++w == n) w = 0;
  }
  if (full) {
    *reinterpret_cast<f32x4*>(out + i) = (f32x4){r[0], r[1], r[2], r[3]};
  } else {
    for (int j = 0; j < 4; ++j)
      if (i + j < total) out[i + j] = r[j];
  }
}

int recal_max_t() { return kRcMaxT; }
int recal_max_q() { return kRcMaxQ; }
int recal_max_f() { return kRcMaxF; }
long long recal_lds_bytes(int T, int F, int Q) { return rc_lds_bytes(T, F, Q); }
int recal_max_lds() { return kRcMaxLds; }

template <int OBJ>
static hipError_t rc_sums_launch(const float* probs, const unsigned char* y, const int* fold, const double* thetas,
                                 long long n, int T, int Q, int F, long long range_len, int n_ranges, int grid, int lds,
                                 double* part, hipStream_t stream) {
  if (lds > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(recal_sums_kernel<OBJ>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(recal_sums_kernel<OBJ>, dim3(grid), dim3(kRcThreads), lds, stream, probs, y, fold, thetas, n, T, Q,
                     F, range_len, n_ranges, part);
  return hipGetLastError();
}

// part: n_ranges x (F Q 12); out: (F Q 12).  fold may be null (every window in fold 0).  grid: workgroups (0: one
// per range); the result does not depend on it.
hipError_t launch_recal_sums(const float* probs, const unsigned char* y, const int* fold, const double* thetas,
                             long long n, int T, int Q, int F, int objective, long long range_len, int grid,
                             double* part, double* out, hipStream_t stream) {
  if (T < 1 || T > kRcMaxT || Q < 1 || Q > kRcMaxQ || F < 1 || F > kRcMaxF || n < 1 || n > (1ll << 27) ||
      range_len < 1 || objective < 0 || objective > 1)
    return hipErrorInvalidValue;
  const long long nr = (n + range_len - 1) / range_len;
  const long long lds = rc_lds_bytes(T, F, Q);
  if (nr > (1 << 20) || lds > kRcMaxLds) return hipErrorInvalidValue;
  const int n_ranges = (int)nr;
  if (grid <= 0 || grid > n_ranges) grid = n_ranges;
  const hipError_t e = objective == 0 ? rc_sums_launch<0>(probs, y, fold, thetas, n, T, Q, F, range_len, n_ranges, grid,
                                                          (int)lds, part, stream)
                                      : rc_sums_launch<1>(probs, y, fold, thetas, n, T, Q, F, range_len, n_ranges, grid,
                                                          (int)lds, part, stream);
  if (e != hipSuccess) return e;
  const int n_out = F * Q * kRcCols;
  hipLaunchKernelGGL(recal_reduce_kernel, dim3((n_out + kRcThreads - 1) / kRcThreads), dim3(kRcThreads), 0, stream, part,
                     n_ranges, n_out, out);
  return hipGetLastError();
}

// probs and out: (T, n) fp32, 16-byte aligned; fold may be null; thetas (F, 3)
hipError_t launch_recal_apply(const float* probs, const int* fold, const double* thetas, long long n, int T, int F,
                              float* out, hipStream_t stream) {
  if (T < 1 || n < 1 || F < 1 || F > kRcMaxF) return hipErrorInvalidValue;
  const long long total = (long long)T * n;
  const long long blocks = ((total + 3) / 4 + kRcThreads - 1) / kRcThreads;
  if (blocks > 0x7FFFFFFFll) return hipErrorInvalidValue;
  hipLaunchKernelGGL(recal_apply_kernel, dim3((unsigned)blocks), dim3(kRcThreads), 0, stream, probs, fold, thetas, n,
                     total, F, out);
  return hipGetLastError();
}

}  // namespace apneauq
