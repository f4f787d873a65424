// Ensemble composition from one (T, n) prediction set (gfx950): which members differ, and what a chosen
// sub-ensemble would have scored.
//
// member_pairs   (T, T, 3) int64 over the pairs a <= b (the binding mirrors the triangle): the windows where
//                both members are correct, split by y = 0 / y = 1, and the residual Gram
//                sum_w rint(r_a r_b 2^40) with r_t = (double)p_t - (y != 0); plus the header (n_valid, n_y1).
// member_mix     (F, Q, 7) int64: per fold and per row of integer member counts c (Q, T), the sums over the
//                windows of the mixture m = (sum_t c_t p_t) / k: n_valid, n_y1, nll_q, brier_q, correct,
//                true_pos, pred_pos.
//
// Every float quantity is one fp64 value per window (and per pair / row), quantised to an integer with round
// to nearest even; every sum over windows is an integer add.  The results therefore do not depend on the
// grid, on slices, on the schedule, on the order of the windows or on how they are sharded, and shards add
// exactly.  The scales, the column layout and the limits are mirrored in ops/members.py (the emulation).
#include "common.h"
#include "uq_api.h"

namespace apneauq {

constexpr int kMbThreads = 256;
constexpr int kMbWaves = kMbThreads / kWave;
constexpr int kMbMaxT = 128;
constexpr int kMbMaxQ = 64;
constexpr int kMbMaxF = 16;
constexpr int kMbPatch = 4;                      // a thread owns a 4 x 4 patch of the pair matrix
constexpr int kMbRow = kWave + 1;                // doubles per residual plane: 64 windows and one of padding
constexpr int kMbMixCols = 7;
constexpr double kMbMagic = 6755399441055744.0;  // 1.5 * 2^52: x + magic leaves rint(x) in the low mantissa bits
constexpr double kMbHalfScale = 1048576.0;       // 2^20 on each residual: the product carries 2^40 exactly
constexpr double kMbBrierScale = 1099511627776.0;   // 2^40
constexpr double kMbNllScale = 68719476736.0;       // 2^36: nll <= 16.12 < 2^5, a term stays below 2^41

__device__ __forceinline__ bool mb_finite(float p) { return fabsf(p) <= 3.402823466e38f; }   // false for NaN, +-inf

// A product that feeds a plain add is kept in a register of its own: the build uses -ffp-contract=fast and contracts
// a * b + c into an FMA wherever it sees one; nothing is fused across the empty asm (uq_recal.hip and uq_laplace.hip
// do the same).
__device__ __forceinline__ double mb_rounded(double v) {
  asm volatile("" : "+v"(v));
  return v;
}

// rint(x) of |x| < 2^51 as an integer, round to nearest even (the magic-number form of cv_q)
__device__ __forceinline__ long long mb_rint(double x) {
  return __double_as_longlong(x + kMbMagic) - __double_as_longlong(kMbMagic);
}

// ---------------------------------------------------------------------------------------------------------
// member_pairs
//
// The pair matrix is cut into 4 x 4 patches; the patches on and above the diagonal are numbered row by row,
// P (P + 1) / 2 of them with P = ceil(T / 4).  A workgroup has 256 / slices of them (blockIdx.y walks the
// rest) and `slices` threads per patch, each with its own 64 / slices windows of a tile; a thread keeps the
// 16 Gram sums and 2 x 16 counts of its patch in registers over all the tiles of its workgroup
// (blockIdx.x, + gridDim.x, ...) and adds them to the output once, with integer atomics.
//
// Per tile the four waves first stage the T rows as fp32 planes and agree on the valid windows, then write
// the residual planes rs[t][65] = (p_t - y) 2^20 (0 for an invalid or absent window, so that it adds nothing)
// and, per member, the ballots of "correct and y = 0" and "correct and y = 1".  The plane stride of 65
// doubles moves lanes that read different members at one window to different banks (a stride of 64 doubles
// would put them all on one).  The counts are popcount(ballot_a & ballot_b), the Gram column is one fp64
// multiply and one fp64 add per pair and window: r_a 2^20 * r_b 2^20 is the correctly rounded r_a r_b scaled
// by 2^40 (a power of two commutes with the rounding), and adding 1.5 * 2^52 rounds it to an integer that
// sits in the low mantissa bits.  The bit patterns are summed as they are (modulo 2^64) and the windows'
// share of the magic constant's pattern is taken off at the end.  The multiply and the add must stay two
// roundings, as in the emulation (an FMA rounds the exact product once and differs where the rounded product
// is a half-integer and the exact one is not): mb_rounded keeps the product in a register of its own.
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kMbThreads) void member_pairs_kernel(const float* __restrict__ probs,
                                                                  const int* __restrict__ y, int t_count, int n,
                                                                  int n_tiles, int slices,
                                                                  unsigned long long* __restrict__ out,
                                                                  unsigned long long* __restrict__ head) {
  extern __shared__ double mp_lds[];
  APNEAUQ_DASSERT(blockDim.x == kMbThreads && t_count >= 1 && t_count <= kMbMaxT && n >= 1);
  APNEAUQ_DASSERT(slices >= 1 && slices <= kWave && (slices & (slices - 1)) == 0 && (int)gridDim.x <= n_tiles);
  double* rs = mp_lds;                                                                        // [T][65] fp64
  unsigned long long* m0 = reinterpret_cast<unsigned long long*>(rs + (size_t)t_count * kMbRow);   // [T]
  unsigned long long* m1 = m0 + t_count;                                                      // [T]
  int* flags = reinterpret_cast<int*>(m1 + t_count);                                          // [4][64]
  float* ps = reinterpret_cast<float*>(flags + kMbWaves * kWave);                             // [T][64] fp32
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);

  const int p_side = (t_count + kMbPatch - 1) / kMbPatch;
  const int n_patch = p_side * (p_side + 1) / 2;
  const int per_block = kMbThreads / slices;
  const int slice = threadIdx.x / per_block;
  const int patch = blockIdx.y * per_block + threadIdx.x % per_block;
  const bool active = patch < n_patch;
  int pi = 0, rem = active ? patch : 0;
  while (rem >= p_side - pi) {
    rem -= p_side - pi;
    ++pi;
  }
  const int pj = pi + rem;
  int ia[kMbPatch], ib[kMbPatch];   // members past T - 1 read the last plane; their sums are never written
#pragma unroll
  for (int i = 0; i < kMbPatch; ++i) {
    ia[i] = min(pi * kMbPatch + i, t_count - 1);
    ib[i] = min(pj * kMbPatch + i, t_count - 1);
  }
  const int w_len = kWave / slices, w_lo = slice * w_len;

  unsigned long long g[kMbPatch][kMbPatch];
  int c0[kMbPatch][kMbPatch], c1[kMbPatch][kMbPatch];
#pragma unroll
  for (int i = 0; i < kMbPatch; ++i)
#pragma unroll
    for (int j = 0; j < kMbPatch; ++j) {
      g[i][j] = 0;
      c0[i][j] = 0;
      c1[i][j] = 0;
    }
  unsigned long long windows_done = 0, n_valid = 0, n_y1 = 0;

  for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long long j = (long long)tile * kWave + lane;
    const bool in = j < n;
    const long long jj = in ? j : n - 1;   // idle lanes read a valid element
    bool fin = true;
    for (int t = wave; t < t_count; t += kMbWaves) {
      const float p = probs[(long long)t * n + jj];
      ps[t * kWave + lane] = p;
      fin = fin && mb_finite(p);
    }
    flags[wave * kWave + lane] = fin;
    __syncthreads();   // the planes and the flags are written; every wave is done with the previous tile
    bool valid = in;
#pragma unroll
    for (int w = 0; w < kMbWaves; ++w) valid = valid && flags[w * kWave + lane] != 0;
    const bool y1 = y[jj] != 0;
    const double yd = y1 ? 1.0 : 0.0;
    for (int t = wave; t < t_count; t += kMbWaves) {
      const float p = ps[t * kWave + lane];
      const double r = fmin(fmax((double)p - yd, -1.0), 1.0);   // |r| <= 1 for probabilities; the clamp bounds a term
      rs[t * kMbRow + lane] = valid ? r * kMbHalfScale : 0.0;
      const bool c = valid && ((p > 0.5f) == y1);
      const unsigned long long b0 = __ballot(c && !y1), b1 = __ballot(c && y1);
      if (lane == 0) {
        m0[t] = b0;
        m1[t] = b1;
      }
    }
    if (wave == 0 && blockIdx.y == 0) {
      n_valid += __popcll(__ballot(valid));
      n_y1 += __popcll(__ballot(valid && y1));
    }
    __syncthreads();   // residual planes and ballots are written
    if (active) {
      for (int w = w_lo; w < w_lo + w_len; ++w) {
        double ra[kMbPatch], rb[kMbPatch];
#pragma unroll
        for (int i = 0; i < kMbPatch; ++i) {
          ra[i] = rs[ia[i] * kMbRow + w];
          rb[i] = rs[ib[i] * kMbRow + w];
        }
#pragma unroll
        for (int i = 0; i < kMbPatch; ++i)
#pragma unroll
          for (int jx = 0; jx < kMbPatch; ++jx) {
            const double prod = mb_rounded(ra[i] * rb[jx]);
            g[i][jx] += (unsigned long long)__double_as_longlong(prod + kMbMagic);
          }
      }
      windows_done += w_len;
      if (slice == 0) {
#pragma unroll
        for (int i = 0; i < kMbPatch; ++i) {
          const unsigned long long a0 = m0[ia[i]], a1 = m1[ia[i]];
#pragma unroll
          for (int jx = 0; jx < kMbPatch; ++jx) {
            c0[i][jx] += __popcll(a0 & m0[ib[jx]]);
            c1[i][jx] += __popcll(a1 & m1[ib[jx]]);
          }
        }
      }
    }
  }

  if (active) {
    const unsigned long long bias = windows_done * (unsigned long long)__double_as_longlong(kMbMagic);
#pragma unroll
    for (int i = 0; i < kMbPatch; ++i)
#pragma unroll
      for (int jx = 0; jx < kMbPatch; ++jx) {
        const int a = pi * kMbPatch + i, b = pj * kMbPatch + jx;
        if (a > b || b >= t_count) continue;
        unsigned long long* o = out + ((long long)a * t_count + b) * 3;
        const unsigned long long gv = g[i][jx] - bias;   // modulo 2^64: the signed sum of the quantised products
        if (c0[i][jx] != 0) atomicAdd(o, (unsigned long long)c0[i][jx]);
        if (c1[i][jx] != 0) atomicAdd(o + 1, (unsigned long long)c1[i][jx]);
        if (gv != 0) atomicAdd(o + 2, gv);
      }
  }
  if (threadIdx.x == 0 && blockIdx.y == 0) {
    if (n_valid != 0) atomicAdd(head, n_valid);
    if (n_y1 != 0) atomicAdd(head + 1, n_y1);
  }
}

int member_max_t() { return kMbMaxT; }
int member_max_q() { return kMbMaxQ; }
int member_max_f() { return kMbMaxF; }

int member_pairs_lds_bytes(int t_count) {
  return t_count * (kMbRow * 8 + 16 + kWave * 4) + kMbWaves * kWave * 4;   // 102,400 B at T = 128
}

// The slices of a launch: as many threads per patch as keep every patch of T in one workgroup.
int member_pairs_auto_slices(int t_count) {
  const int p_side = (t_count + kMbPatch - 1) / kMbPatch, n_patch = p_side * (p_side + 1) / 2;
  int s = 1;
  while (s < kWave && n_patch * s * 2 <= kMbThreads) s *= 2;
  return s;
}

// out (T, T, 3) and head (2) must be zero; the triangle a <= b is written.  Limits (checked by the binding):
// T <= 128, n <= 2^22.  grid (0: auto) workgroups share the tiles of 64 windows; slices (0: auto) is a power
// of two up to 64.  Neither changes the result.
hipError_t launch_member_pairs(const float* probs, const int* y, int t_count, int n, int grid, int slices,
                               long long* out, long long* head, hipStream_t stream) {
  if (n <= 0 || t_count <= 0) return hipSuccess;
  if (t_count > kMbMaxT || grid < 0 || grid > 65535 || slices < 0 || slices > kWave || (slices & (slices - 1)) != 0)
    return hipErrorInvalidValue;
  if (slices == 0) slices = member_pairs_auto_slices(t_count);
  const int p_side = (t_count + kMbPatch - 1) / kMbPatch, n_patch = p_side * (p_side + 1) / 2;
  const int per_block = kMbThreads / slices;
  const int gy = (n_patch + per_block - 1) / per_block;
  const int n_tiles = (n + kWave - 1) / kWave;
  // A workgroup pays its 48 atomics per patch and slice once, whatever it has summed: it should own at least 8
  // tiles (32 with more than two slices, whose flush is that much larger), and one workgroup per CU is enough.
  if (grid == 0) grid = min(max(1, 256 / gy), max(1, n_tiles / (slices > 2 ? 32 : 8)));
  grid = min(grid, n_tiles);
  const int lds = member_pairs_lds_bytes(t_count);
  if (lds > 64 * 1024) {  // above the default dynamic LDS limit
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(member_pairs_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize,
                                             member_pairs_lds_bytes(kMbMaxT));
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(member_pairs_kernel, dim3(grid, gy), dim3(kMbThreads), lds, stream, probs, y, t_count, n, n_tiles,
                     slices, reinterpret_cast<unsigned long long*>(out), reinterpret_cast<unsigned long long*>(head));
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------
// member_mix
//
// A workgroup takes tiles of 64 windows (lane = window; blockIdx.x, + gridDim.x, ...) and stages a tile's T
// rows as [t][64] fp32 planes, as converge_kernel does.  Wave w takes the rows q = w, w + 4, ...: it walks
// counts[q, 0..T) with wave-uniform loads, skips the zeros (adding 0.0 changes nothing) and accumulates
// s += c_t p_t in fp64 in the order t = 0..T-1; c_t p_t is exact (8 bits times 24), so s is the same with and
// without a fused multiply-add.  m = s / k is one correctly rounded division.  The lane's window then gives
// its terms, the wave sums them per fold present in the tile, and lanes 0..6 add one column each to the
// workgroup's (F, Q, 7) sums in LDS: a row belongs to one wave, so these are plain adds.  The workgroup adds
// its non-zero sums to the output with integer atomics at the end.
//
// A window with a non-finite probability in any pass, or with a fold code >= F, contributes to nothing.
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kMbThreads) void member_mix_kernel(const float* __restrict__ probs,
                                                                const int* __restrict__ y,
                                                                const unsigned char* __restrict__ fold,
                                                                const int* __restrict__ counts, int t_count, int n,
                                                                int n_tiles, int n_rows, int n_folds,
                                                                unsigned long long* __restrict__ out) {
  extern __shared__ long long mm_lds[];
  APNEAUQ_DASSERT(blockDim.x == kMbThreads && t_count >= 1 && t_count <= kMbMaxT && n >= 1);
  APNEAUQ_DASSERT(n_rows >= 1 && n_rows <= kMbMaxQ && n_folds >= 1 && n_folds <= kMbMaxF && (int)gridDim.x <= n_tiles);
  const int n_acc = n_folds * n_rows * kMbMixCols;
  long long* acc = mm_lds;                                   // [F][Q][7] int64
  float* ps = reinterpret_cast<float*>(mm_lds + n_acc);      // [T][64] fp32
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int i = threadIdx.x; i < n_acc; i += kMbThreads) acc[i] = 0;

  for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long long j = (long long)tile * kWave + lane;
    const bool in = j < n;
    const long long jj = in ? j : n - 1;   // idle lanes read a valid element
    __syncthreads();   // every wave is done with the planes of the previous tile (and acc is zero)
    for (int t = wave; t < t_count; t += kMbWaves) ps[t * kWave + lane] = probs[(long long)t * n + jj];
    __syncthreads();
    bool ok = in;
    for (int t = 0; t < t_count; ++t) ok = ok && mb_finite(ps[t * kWave + lane]);
    const int f = fold != nullptr ? (int)fold[jj] : 0;
    ok = ok && f < n_folds;
    const bool y1 = y[jj] != 0;
    const double yd = y1 ? 1.0 : 0.0;
    const unsigned long long any = __ballot(ok);
    if (any == 0) continue;
    for (int q = wave; q < n_rows; q += kMbWaves) {
      const int* cq = counts + (long long)q * t_count;
      double s = 0.0;
      int k = 0;
      for (int t = 0; t < t_count; ++t) {
        const int c = cq[t];
        if (c == 0) continue;
        k += c;
        s = fma((double)c, (double)ps[t * kWave + lane], s);
      }
      if (k <= 0) continue;   // the binding rejects such a row
      const double kd = (double)k;
      const double m = s / kd;
      const bool lab = 2.0 * s > kd;
      const double pt = y1 ? m : 1.0 - m;
      const double nll = -log(fmin(fmax(pt, 1e-7), 1.0 - 1e-7));
      const double d = m - yd;
      const double sq = fmin(mb_rounded(d * d), 1.0);   // (m - y)^2 <= 1 for probabilities; the clamp bounds a term
      const long long bq = ok ? mb_rint(sq * kMbBrierScale) : 0;   // the scalings by a power of two are exact,
      const long long nq = ok ? mb_rint(nll * kMbNllScale) : 0;    // fused with the add or not
      unsigned long long todo = any;
      while (todo != 0) {
        const int leader = __builtin_ctzll(todo);
        const int ff = __builtin_amdgcn_readfirstlane(__shfl(f, leader, kWave));
        const bool sel = ok && f == ff;
        const unsigned long long mask = __ballot(sel);
        todo &= ~mask;
        const long long sn = wave_sum(sel ? nq : 0LL), sb = wave_sum(sel ? bq : 0LL);
        const long long cnt_y1 = __popcll(__ballot(sel && y1));
        const long long correct = __popcll(__ballot(sel && lab == y1));
        const long long true_pos = __popcll(__ballot(sel && lab && y1));
        const long long pred_pos = __popcll(__ballot(sel && lab));
        const long long v = lane == 0 ? (long long)__popcll(mask) : lane == 1 ? cnt_y1 : lane == 2 ? sn : lane == 3 ? sb
                            : lane == 4 ? correct : lane == 5 ? true_pos : pred_pos;
        if (lane < kMbMixCols && v != 0) acc[(ff * n_rows + q) * kMbMixCols + lane] += v;
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < n_acc; i += kMbThreads) {
    const long long v = acc[i];
    if (v != 0) atomicAdd(out + i, (unsigned long long)v);
  }
}

int member_mix_lds_bytes(int t_count, int n_rows, int n_folds) {
  return n_folds * n_rows * kMbMixCols * 8 + t_count * kWave * 4;   // 90,112 B at F = 16, Q = 64, T = 128
}

// out (F, Q, 7) must be zero.  Limits (checked by the binding): T <= 128, Q <= 64, F <= 16, n <= 2^21, counts in
// 0..255 with a positive row sum.  grid (0: auto) workgroups share the tiles; it does not change the result.
hipError_t launch_member_mix(const float* probs, const int* y, const unsigned char* fold, const int* counts,
                             int t_count, int n, int n_rows, int n_folds, int grid, long long* out,
                             hipStream_t stream) {
  if (n <= 0 || t_count <= 0 || n_rows <= 0) return hipSuccess;
  if (t_count > kMbMaxT || n_rows > kMbMaxQ || n_folds < 1 || n_folds > kMbMaxF || grid < 0 || grid > 65535)
    return hipErrorInvalidValue;
  const int n_tiles = (n + kWave - 1) / kWave;
  if (grid == 0) grid = 2048;
  grid = min(grid, n_tiles);
  const int lds = member_mix_lds_bytes(t_count, n_rows, n_folds);
  if (lds > 64 * 1024) {  // above the default dynamic LDS limit
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(member_mix_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize,
                                             member_mix_lds_bytes(kMbMaxT, kMbMaxQ, kMbMaxF));
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(member_mix_kernel, dim3(grid), dim3(kMbThreads), lds, stream, probs, y, fold, counts, t_count, n,
                     n_tiles, n_rows, n_folds, reinterpret_cast<unsigned long long*>(out));
  return hipGetLastError();
}

}  // namespace apneauq
