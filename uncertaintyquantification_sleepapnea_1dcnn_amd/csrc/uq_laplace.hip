// Last-layer Laplace approximation (gfx950): the weighted Gram matrix of the fit set and the fp64 GEMM of a
// prediction call, both on v_mfma_f64_16x16x4_f64.
//
// With phi~_i = [phi_i; 1] (D + 1 values, fp64 copies of the fp32 features), f_i = theta . phi~_i,
// e_i = exp(-|f_i|), p_i = sigmoid(f_i) and w_i = p_i (1 - p_i) = e_i / (1 + e_i)^2:
//
// laplace_gram     H = sum_i w_i phi~_i phi~_i^T, g = sum_i (p_i - y_i) phi~_i, loglik = sum_i log p(y_i | f_i)
//                  (-softplus(-/+ f_i)) and n_valid over the valid windows (all features finite, y in {0, 1}).
//                  D + 1 is padded to DP = 16 NT <= 128.  A workgroup stages 64 windows' phi~ in LDS once (fp64),
//                  four lanes per window form f_i (lane j adds the features c = j mod 4 in ascending order with
//                  separately rounded multiply and add, then (a0 + a1) + (a2 + a3) + theta_D: ops/laplace.py
//                  gram_eager forms the same bits), and the four waves share the NT (NT + 1) / 2 upper-triangle
//                  16 x 16 tiles round robin: A = w phi~ (row = feature, k = window), B = phi~.
// laplace_predict  out = Phi~ Mx with Mx = [theta | theta_1 .. theta_T | L] (D + 1, 1 + T + D + 1): column 0 is
//                  mu, columns 1..T are sample logits (sigmoid -> preds (T, n) fp32), the squares of the last
//                  D + 1 columns add up to v; probit = sigmoid(mu / sqrt(1 + pi v / 8)).  A wave keeps its 16
//                  windows' phi~ in registers (A operand) and Mx passes through LDS in blocks of 64 columns.
//
// f64 MFMA lane maps: A[row = l & 15][k = l >> 4], B[k = l >> 4][col = l & 15], one f64 per lane; C/D col = l & 15,
// row = (l >> 4) + 4 reg (NOT the f32 map).
//
// Grid invariance of laplace_gram: the windows are cut into ranges of range_len windows (a function of n and D
// only, ops/laplace.py range_len); a range is accumulated in window order by whichever workgroup takes it, into
// its own partial; laplace_gram_reduce adds the partials in range order.  No floating-point atomics.
#include "common.h"
#include "uq_api.h"

namespace apneauq {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int kLapThreads = 256;
constexpr int kLapWaves = kLapThreads / kWave;
constexpr int kLapWT = 64;           // windows per staged tile
constexpr int kLapMaxDP = 128;       // D + 1 padded
constexpr int kLapCB = 64;           // Mx columns per LDS block
constexpr int kLapMS = kLapCB + 16;  // LDS row stride of the Mx block: consecutive k rows 128 B apart mod 256

// LDS row stride (doubles) of the staged phi~ tile: = 16 mod 32, so the four k rows of an operand read fall
// on different halves of the banks
__host__ __device__ constexpr int lap_stride(int dp) { return dp % 32 == 16 ? dp : dp + 16; }
// doubles of one range's partial: H (DP x DP, upper tiles written), g (DP), loglik, n_valid
__host__ __device__ constexpr long long lap_part_doubles(int dp) { return (long long)dp * dp + dp + 2; }

__device__ __forceinline__ double shfl_xor_f64(double v, int m) { return __shfl_xor(v, m, kWave); }

// Separately rounded fp64 multiply and add (the build contracts a * b + c into an FMA; the empty asm keeps the
// rounded operand in a register of its own, so nothing is fused across it): the order of operations that
// ops/laplace.py logits_eager reproduces bit for bit.
__device__ __forceinline__ double opaque_f64(double v) {
  asm volatile("" : "+v"(v));
  return v;
}
__device__ __forceinline__ double add_rn(double a, double b) { return opaque_f64(opaque_f64(a) + opaque_f64(b)); }
__device__ __forceinline__ double mul_rn(double a, double b) { return opaque_f64(opaque_f64(a) * opaque_f64(b)); }

// A wave's share of a 64-window tile of phi, global -> registers: rows wave, wave + 4, ..., lane l the columns l and
// l + 64.  Fully unrolled, so the loads are issued back to back and waited for once where the values are used
// (a loop of load -> convert -> LDS store pays the memory latency per row).  Rows past nw and columns past D: 0.
constexpr int kLapRows = kLapWT / kLapWaves;
template <int CPL>
__device__ __forceinline__ void lap_fetch(float (&pre)[kLapRows][CPL], const float* __restrict__ phi, long long base,
                                          int nw, int D, int wave, int lane) {
#pragma unroll
  for (int r = 0; r < kLapRows; ++r) {
    const int row = wave + kLapWaves * r;
    const float* src = phi + (base + row) * D;
#pragma unroll
    for (int cc = 0; cc < CPL; ++cc) {
      const int c = lane + kWave * cc;
      pre[r][cc] = (row < nw && c < D) ? src[c] : 0.f;
    }
  }
}

template <int NT>
__global__ __launch_bounds__(kLapThreads) void laplace_gram_kernel(const float* __restrict__ phi,
                                                                   const double* __restrict__ theta,
                                                                   const uint8_t* __restrict__ y, long long n, int D,
                                                                   long long range_len, int n_ranges,
                                                                   double* __restrict__ part) {
  constexpr int DP = 16 * NT, LS = lap_stride(DP), NTILE = NT * (NT + 1) / 2, MAXT = (NTILE + kLapWaves - 1) / kLapWaves;
  constexpr int CPL = (DP + kWave - 1) / kWave;
  extern __shared__ double lap_lds[];
  APNEAUQ_DASSERT(blockDim.x == kLapThreads && D >= 1 && D + 1 <= DP && D + 1 > DP - 16 && range_len >= 1);
  double* ph = lap_lds;           // [64][LS] phi~ (invalid windows zeroed)
  double* wv = ph + kLapWT * LS;  // [64] w
  double* rv = wv + kLapWT;       // [64] p - y
  double* lv = rv + kLapWT;       // [64] log-likelihood term
  double* ov = lv + kLapWT;       // [64] 1 = valid
  double* th = ov + kLapWT;       // [DP] theta, zero padded
  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  int ti[MAXT], tj[MAXT];
  bool has[MAXT];
#pragma unroll
  for (int k = 0; k < MAXT; ++k) {
    const int t = wave + kLapWaves * k;
    has[k] = t < NTILE;
    int i = 0, r = has[k] ? t : 0;
    while (r >= NT - i) {
      r -= NT - i;
      ++i;
    }
    ti[k] = i;
    tj[k] = i + r;
  }
  if (tid < DP) th[tid] = tid <= D ? theta[tid] : 0.0;

  for (int range = blockIdx.x; range < n_ranges; range += gridDim.x) {
    f64x4 acc[MAXT];
#pragma unroll
    for (int k = 0; k < MAXT; ++k) acc[k] = (f64x4){0.0, 0.0, 0.0, 0.0};
    double ga[4] = {0.0, 0.0, 0.0, 0.0}, la[4] = {0.0, 0.0, 0.0, 0.0}, cnt = 0.0;
    const long long w0 = (long long)range * range_len;
    const long long w1 = w0 + range_len < n ? w0 + range_len : n;
    float pre[kLapRows][CPL];  // the next tile's phi, in flight while this tile is accumulated
    lap_fetch<CPL>(pre, phi, w0, w1 - w0 < kLapWT ? (int)(w1 - w0) : kLapWT, D, wave, lane);
    for (long long base = w0; base < w1; base += kLapWT) {
      const int nw = w1 - base < kLapWT ? (int)(w1 - base) : kLapWT;
      __syncthreads();  // the previous tile's readers are done (and th is written)
#pragma unroll
      for (int r = 0; r < kLapRows; ++r) {
        const int row = wave + kLapWaves * r;
#pragma unroll
        for (int cc = 0; cc < CPL; ++cc) {
          const int c = lane + kWave * cc;
          if (c < DP) ph[row * LS + c] = (c == D && row < nw) ? 1.0 : (double)pre[r][cc];
        }
      }
      __syncthreads();
      if (base + kLapWT < w1) {
        const long long nb = base + kLapWT;
        lap_fetch<CPL>(pre, phi, nb, w1 - nb < kLapWT ? (int)(w1 - nb) : kLapWT, D, wave, lane);
      }
      {
        const int row = tid >> 2, j = tid & 3;
        double* pr = ph + row * LS;
        double a = 0.0;
        int fin = 1;
        for (int c = j; c < D; c += 4) {
          const double x = pr[c];
          fin &= (int)isfinite(x);
          a = add_rn(a, mul_rn(th[c], x));
        }
        a = add_rn(a, shfl_xor_f64(a, 1));
        a = add_rn(a, shfl_xor_f64(a, 2));
        fin &= __shfl_xor(fin, 1, kWave);
        fin &= __shfl_xor(fin, 2, kWave);
        const double f = add_rn(a, th[D]);
        const unsigned yv = row < nw ? (unsigned)y[base + row] : 2u;
        const bool valid = row < nw && fin && yv <= 1u;
        if (j == 0) {
          const double e = exp(-fabs(f));
          const double inv = 1.0 / (1.0 + e);
          const double p = f >= 0.0 ? inv : e * inv;
          const double q = f >= 0.0 ? e * inv : inv;
          const double z = yv ? -f : f;
          wv[row] = valid ? e * inv * inv : 0.0;
          rv[row] = valid ? (yv ? -q : p) : 0.0;
          lv[row] = valid ? -((z > 0.0 ? z : 0.0) + log1p(e)) : 0.0;
          ov[row] = valid ? 1.0 : 0.0;
        }
        if (!valid)
          for (int c = j; c < DP; c += 4) pr[c] = 0.0;
      }
      __syncthreads();
      if (tid < DP) {
        for (int i = 0; i < kLapWT; i += 4) {
#pragma unroll
          for (int u = 0; u < 4; ++u) ga[u] += rv[i + u] * ph[(i + u) * LS + tid];
        }
      } else if (tid == kLapThreads - 1) {
        for (int i = 0; i < kLapWT; i += 4) {
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            la[u] += lv[i + u];
            cnt += ov[i + u];
          }
        }
      }
      const int ksteps = (nw + 3) >> 2;
      for (int ks = 0; ks < ksteps; ++ks) {
        const int wr = ks * 4 + (lane >> 4);
        const double wgt = wv[wr];
        const double* rowp = ph + wr * LS + (lane & 15);
#pragma unroll
        for (int k = 0; k < MAXT; ++k) {
          if (has[k]) {
            const double a = wgt * rowp[16 * ti[k]];
            const double b = rowp[16 * tj[k]];
            acc[k] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[k], 0, 0, 0);
          }
        }
      }
    }
    double* out = part + (long long)range * lap_part_doubles(DP);
#pragma unroll
    for (int k = 0; k < MAXT; ++k) {
      if (has[k]) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          out[(16 * ti[k] + (lane >> 4) + 4 * r) * DP + 16 * tj[k] + (lane & 15)] = acc[k][r];
      }
    }
    if (tid < DP) out[DP * DP + tid] = (ga[0] + ga[1]) + (ga[2] + ga[3]);
    if (tid == kLapThreads - 1) {
      out[DP * DP + DP] = (la[0] + la[1]) + (la[2] + la[3]);
      out[DP * DP + DP + 1] = cnt;
    }
  }
}

// out (D1 D1 + D1 + 2): H row-major (the upper triangle mirrored), g, loglik, n_valid; partials added in range order
__global__ __launch_bounds__(kLapThreads) void laplace_gram_reduce_kernel(const double* __restrict__ part, int n_ranges,
                                                                          int DP, int D1, double* __restrict__ out) {
  const int e = blockIdx.x * kLapThreads + threadIdx.x;
  const int hh = D1 * D1;
  if (e >= hh + D1 + 2) return;
  int src;
  if (e < hh) {
    const int a = e / D1, b = e - a * D1;
    src = (a < b ? a : b) * DP + (a < b ? b : a);
  } else if (e < hh + D1) {
    src = DP * DP + (e - hh);
  } else {
    src = DP * DP + DP + (e - hh - D1);
  }
  const long long pd = lap_part_doubles(DP);
  double s = 0.0;
  for (int r = 0; r < n_ranges; ++r) s += part[r * pd + src];
  out[e] = s;
}

__device__ __forceinline__ double sigmoid_f64(double x) {
  const double e = exp(-fabs(x));
  const double inv = 1.0 / (1.0 + e);
  return x >= 0.0 ? inv : e * inv;
}

template <int NT>
__global__ __launch_bounds__(kLapThreads) void laplace_predict_kernel(const float* __restrict__ phi,
                                                                      const double* __restrict__ mx, long long n, int D,
                                                                      int T, long long ncols, float* __restrict__ preds,
                                                                      double* __restrict__ mu, double* __restrict__ vv,
                                                                      double* __restrict__ probit) {
  constexpr int DP = 16 * NT, KS = DP / 4, PS = DP + 1, OS = kLapWT + 1;
  constexpr int kStage = (kLapWT * PS > kLapCB * OS ? kLapWT * PS : kLapCB * OS);
  extern __shared__ double lap_lds[];
  APNEAUQ_DASSERT(blockDim.x == kLapThreads && D >= 1 && D + 1 <= DP && T >= 0 && ncols == (long long)T + D + 2);
  double* mb = lap_lds;                                      // [DP][kLapMS] block of Mx
  float* pf = reinterpret_cast<float*>(mb + DP * kLapMS);    // [64][PS] fp32 phi~ of the tile, then
  float* ot = pf;                                            // [64 cols][OS] sample probabilities of a block
  int* bad = reinterpret_cast<int*>(pf + kStage);            // [64] window has a non-finite feature
  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long long base = (long long)blockIdx.x * kLapWT;
  const int nw = n - base < kLapWT ? (int)(n - base) : kLapWT;

  {
    constexpr int CPL = (DP + kWave - 1) / kWave;
    float pre[kLapRows][CPL];
    lap_fetch<CPL>(pre, phi, base, nw, D, wave, lane);
#pragma unroll
    for (int r = 0; r < kLapRows; ++r) {
      const int row = wave + kLapWaves * r;
      int nf = 0;
#pragma unroll
      for (int cc = 0; cc < CPL; ++cc) {
        const int c = lane + kWave * cc;
        const float v = (c == D && row < nw) ? 1.f : pre[r][cc];
        nf |= !isfinite(v);
        if (c < DP) pf[row * PS + c] = v;
      }
      const int any = __any(nf);
      if (lane == 0) bad[row] = any;
    }
  }
  __syncthreads();
  double a[KS];
  {
    const float* pr = pf + (wave * 16 + (lane & 15)) * PS + (lane >> 4);
#pragma unroll
    for (int s = 0; s < KS; ++s) a[s] = (double)pr[4 * s];
  }
  double vacc[4] = {0.0, 0.0, 0.0, 0.0}, muv[4] = {0.0, 0.0, 0.0, 0.0};
  const double nanv = __longlong_as_double(0x7FF8000000000000ll);

  for (long long cb0 = 0; cb0 < ncols; cb0 += kLapCB) {
    __syncthreads();  // the A operands are in registers / the previous block's mb and ot readers are done
    {  // DP / 4 values per thread, eight loads in flight at a time
      constexpr int IT = DP * kLapCB / kLapThreads;
#pragma unroll
      for (int i0 = 0; i0 < IT; i0 += 8) {
        double tmp[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          if (i0 + j < IT) {
            const int idx = tid + kLapThreads * (i0 + j);
            const int k = idx >> 6;
            const long long col = cb0 + (idx & (kLapCB - 1));
            tmp[j] = (k <= D && col < ncols) ? mx[(long long)k * ncols + col] : 0.0;
          }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          if (i0 + j < IT) {
            const int idx = tid + kLapThreads * (i0 + j);
            mb[(idx >> 6) * kLapMS + (idx & (kLapCB - 1))] = tmp[j];
          }
        }
      }
    }
    __syncthreads();
    f64x4 acc[4];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) acc[ct] = (f64x4){0.0, 0.0, 0.0, 0.0};
    const double* bp = mb + (lane >> 4) * kLapMS + (lane & 15);
#pragma unroll
    for (int s = 0; s < KS; ++s) {
#pragma unroll
      for (int ct = 0; ct < 4; ++ct)
        acc[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s], bp[4 * s * kLapMS + 16 * ct], acc[ct], 0, 0, 0);
    }
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      const int c = 16 * ct + (lane & 15);
      const long long col = cb0 + c;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = wave * 16 + (lane >> 4) + 4 * r;
        const double val = acc[ct][r];
        if (col == 0) {
          muv[r] = val;
        } else if (col <= T) {
          ot[c * OS + row] = bad[row] ? __int_as_float(0x7FC00000) : (float)sigmoid_f64(val);
        } else if (col < ncols) {
          vacc[r] += val * val;
        }
      }
    }
    __syncthreads();
    for (int idx = tid; idx < kLapCB * kLapWT; idx += kLapThreads) {
      const int c = idx >> 6, row = idx & (kLapWT - 1);
      const long long col = cb0 + c;
      if (col >= 1 && col <= T && row < nw) preds[(col - 1) * n + base + row] = ot[c * OS + row];
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    double s = vacc[r];
    s += shfl_xor_f64(s, 1);
    s += shfl_xor_f64(s, 2);
    s += shfl_xor_f64(s, 4);
    s += shfl_xor_f64(s, 8);
    const int row = wave * 16 + (lane >> 4) + 4 * r;
    if ((lane & 15) == 0 && row < nw) {
      const long long i = base + row;
      const bool b = bad[row] != 0;
      mu[i] = b ? nanv : muv[r];
      vv[i] = b ? nanv : s;
      probit[i] = b ? nanv : sigmoid_f64(muv[r] / sqrt(1.0 + 0.39269908169872414 * s));  // pi / 8
    }
  }
}

int laplace_max_dp() { return kLapMaxDP; }
int laplace_tile_windows() { return kLapWT; }
int laplace_col_block() { return kLapCB; }
long long laplace_part_doubles(int D) { return lap_part_doubles((D + 1 + 15) / 16 * 16); }

template <int NT>
static hipError_t gram_launch(const float* phi, const double* theta, const uint8_t* y, long long n, int D,
                              long long range_len, int n_ranges, int grid, double* part, hipStream_t stream) {
  constexpr int DP = 16 * NT;
  const int lds = (kLapWT * lap_stride(DP) + 4 * kLapWT + DP) * (int)sizeof(double);
  if (lds > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(laplace_gram_kernel<NT>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(laplace_gram_kernel<NT>, dim3(grid), dim3(kLapThreads), lds, stream, phi, theta, y, n, D, range_len,
                     n_ranges, part);
  return hipGetLastError();
}

// part: n_ranges x laplace_part_doubles(D); out: (D + 1)^2 + (D + 1) + 2 doubles.  grid: workgroups (0: one per
// range); the result does not depend on it.
hipError_t launch_laplace_gram(const float* phi, const double* theta, const unsigned char* y, long long n, int D,
                               long long range_len, int grid, double* part, double* out, hipStream_t stream) {
  if (D < 1 || D + 1 > kLapMaxDP || n < 0 || range_len < 1) return hipErrorInvalidValue;
  const long long nr = (n + range_len - 1) / range_len;
  if (nr > (1 << 20)) return hipErrorInvalidValue;
  const int n_ranges = (int)nr;
  const int NT = (D + 1 + 15) / 16, DP = 16 * NT, D1 = D + 1;
  if (n_ranges > 0) {
    if (grid <= 0 || grid > n_ranges) grid = n_ranges;
    hipError_t e = hipErrorInvalidValue;
    switch (NT) {
#define LAP_CASE(N_)                                                                              \
  case N_:                                                                                        \
    e = gram_launch<N_>(phi, theta, y, n, D, range_len, n_ranges, grid, part, stream); \
    break;
      LAP_CASE(1) LAP_CASE(2) LAP_CASE(3) LAP_CASE(4) LAP_CASE(5) LAP_CASE(6) LAP_CASE(7) LAP_CASE(8)
#undef LAP_CASE
    }
    if (e != hipSuccess) return e;
  }
  const int n_out = D1 * D1 + D1 + 2;
  hipLaunchKernelGGL(laplace_gram_reduce_kernel, dim3((n_out + kLapThreads - 1) / kLapThreads), dim3(kLapThreads), 0,
                     stream, part, n_ranges, DP, D1, out);
  return hipGetLastError();
}

template <int NT>
static hipError_t predict_launch(const float* phi, const double* mx, long long n, int D, int T, float* preds, double* mu,
                                 double* vv, double* probit, hipStream_t stream) {
  constexpr int DP = 16 * NT, PS = DP + 1, OS = kLapWT + 1;
  constexpr int kStage = (kLapWT * PS > kLapCB * OS ? kLapWT * PS : kLapCB * OS);
  const int lds = DP * kLapMS * (int)sizeof(double) + kStage * (int)sizeof(float) + kLapWT * (int)sizeof(int);
  if (lds > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(laplace_predict_kernel<NT>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e != hipSuccess) return e;
  }
  const long long blocks = (n + kLapWT - 1) / kLapWT;
  hipLaunchKernelGGL(laplace_predict_kernel<NT>, dim3((unsigned)blocks), dim3(kLapThreads), lds, stream, phi, mx, n, D, T,
                     (long long)T + D + 2, preds, mu, vv, probit);
  return hipGetLastError();
}

// mx: (D + 1, 1 + T + D + 1) row-major [theta | samples | L]; preds (T, n); mu, vv, probit (n)
hipError_t launch_laplace_predict(const float* phi, const double* mx, long long n, int D, int T, float* preds,
                                  double* mu, double* vv, double* probit, hipStream_t stream) {
  if (D < 1 || D + 1 > kLapMaxDP || n < 0 || T < 0 || n > ((long long)1 << 36)) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  switch ((D + 1 + 15) / 16) {
#define LAP_CASE(N_) \
  case N_:           \
    return predict_launch<N_>(phi, mx, n, D, T, preds, mu, vv, probit, stream);
    LAP_CASE(1) LAP_CASE(2) LAP_CASE(3) LAP_CASE(4) LAP_CASE(5) LAP_CASE(6) LAP_CASE(7) LAP_CASE(8)
#undef LAP_CASE
  }
  return hipErrorInvalidValue;
}

}  // namespace apneauq
