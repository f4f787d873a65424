// Patient-level sums of the (T, N) predictions and the patient-cluster bootstrap (gfx950).
//
// patient_reduce     one pass over probs (T, n): per pass t and patient, the number of windows with
//                    p > 0.5 (pass_pos), and per patient twelve int64 sums of the uq_reduce rows (rec):
//                    counts and fixed-point rint(x 2^30) sums.  Every accumulation is an integer add, so
//                    the result does not depend on the grid, the schedule, the window order or on how
//                    the windows are sharded (shards add exactly).
// patient_bootstrap  replicate b draws P patients with replacement and sums their (P, 25) int64 records
//                    plus the 4 x 4 severity confusion counts: P additions per replicate instead of N
//                    gathers, one launch for all B replicates.
//
// The scale constants and the column layouts are mirrored in ops/patient.py (the eager emulation).
#include "common.h"
#include "uq_api.h"

namespace apneauq {

constexpr int kPatThreads = 256;
constexpr int kPatWaves = kPatThreads / kWave;
constexpr int kPatChunks = 2;                     // 64-window chunks per wave: 128 consecutive windows
constexpr int kPatRec = 12;                       // R, columns of rec
constexpr double kPatScale = 1073741824.0;        // 2^30
constexpr float kPatClamp = 4.0f;                 // |x| <= 4 before quantisation: |x_q| <= 2^32
constexpr int kPatUnroll = 8;

// rows of m (uq_reduce.hip UqRow)
constexpr int kPmVar = 1, kPmEntNats = 2, kPmExpEnt = 3, kPmMI = 4, kPmEntBits = 5, kPmLabel = 6;

// rint(x 2^30) of a metric value; NaN counts as 0, the magnitude is clamped so that 2^27 windows fit int64
__device__ __forceinline__ long long pat_q(float x) {
  const float c = x == x ? fminf(fmaxf(x, -kPatClamp), kPatClamp) : 0.f;
  return __double2ll_rn((double)c * kPatScale);
}

// The running counts of passes [t0, t0 + 64) of patient cur (lane l holds pass t0 + l): one atomic per
// (pass, patient).
__device__ __forceinline__ void pat_flush_pass(int* __restrict__ pass_pos, int n_pat, int t_count, int t0, int cur,
                                               int lane, int& acc) {
  const int t = t0 + lane;
  if (cur >= 0 && t < t_count && acc != 0) atomicAdd(&pass_pos[(long long)t * n_pat + cur], acc);
  acc = 0;
}

// The per-lane record sums of patient cur: wave reduction, then lane k adds column k.
__device__ __forceinline__ void pat_flush_rec(long long* __restrict__ rec, int cur, int lane, long long (&a)[kPatRec]) {
  if (cur >= 0) {
#pragma unroll
    for (int k = 0; k < kPatRec; ++k) {
      const long long v = wave_sum(a[k]);
      if (lane == k && v != 0)
        atomicAdd(reinterpret_cast<unsigned long long*>(&rec[(long long)cur * kPatRec + k]), (unsigned long long)v);
    }
  }
#pragma unroll
  for (int k = 0; k < kPatRec; ++k) a[k] = 0;
}

// rec columns: n, n_y1, pred_pos, tp, correct, sum q(VAR), sum q(VAR | y = 0), sum q(VAR | y = 1),
//              sum q(ENT_NATS), sum q(EXP_ENT), sum q(MI), sum q(ENT_BITS)
//
// A wave owns 128 consecutive windows, 64 at a time (lane = window, so every row of probs is read once
// in 256-byte pieces).  While the 64 patient codes of a chunk are equal -- the usual layout, windows
// grouped by patient -- the positives of pass t are popcount(ballot(p > 0.5)), kept by lane t & 63, and
// the record columns are summed per lane; both are carried over the wave's chunks and go out with one
// atomic per (pass, patient) and per (patient, column) when the patient changes or the range ends.  A
// chunk with mixed codes uses one atomic per lane and nonzero value instead.  Passes are taken 64 at a
// time (T > 64 walks the wave's windows once per 64 passes; the codes are read again, probs is not).
// There is no workgroup table in LDS: every P T takes this same path, straight to global atomics.
// Windows whose code is outside [0, P) are skipped.
__global__ __launch_bounds__(kPatThreads) void patient_reduce_kernel(const float* __restrict__ probs,
                                                                     const float* __restrict__ m,
                                                                     const int* __restrict__ y,
                                                                     const int* __restrict__ code, int t_count, int n,
                                                                     int n_pat, int* __restrict__ pass_pos,
                                                                     long long* __restrict__ rec) {
  APNEAUQ_DASSERT(blockDim.x == kPatThreads && t_count >= 1 && n >= 1 && n_pat >= 1);
  const int lane = threadIdx.x & (kWave - 1);
  const long long w_lo = ((long long)blockIdx.x * kPatWaves + (threadIdx.x >> 6)) * (kPatChunks * kWave);
  if (w_lo >= n) return;
  const int j_lo = (int)w_lo;
  const int j_hi = (int)(w_lo + kPatChunks * kWave < (long long)n ? w_lo + kPatChunks * kWave : (long long)n);
  for (int t0 = 0; t0 < t_count; t0 += kWave) {
    const int tn = t_count - t0 < kWave ? t_count - t0 : kWave;
    const bool first = t0 == 0;  // the record columns are summed on the first walk only
    int cur = -1, acc = 0;
    long long a[kPatRec];
#pragma unroll
    for (int k = 0; k < kPatRec; ++k) a[k] = 0;
    for (int base = j_lo; base < j_hi; base += kWave) {
      const int j = base + lane;
      const bool in = j < j_hi;
      const int cj = in ? code[j] : -1;
      const bool valid = in && (unsigned)cj < (unsigned)n_pat;
      const unsigned long long vmask = __ballot(valid);
      if (vmask == 0ull) continue;
      const int c0 = __builtin_amdgcn_readlane(cj, __ffsll((long long)vmask) - 1);
      const bool uniform = __ballot(valid && cj != c0) == 0ull;
      if (!uniform || c0 != cur) {
        pat_flush_pass(pass_pos, n_pat, t_count, t0, cur, lane, acc);
        if (first) pat_flush_rec(rec, cur, lane, a);
        cur = uniform ? c0 : -1;
      }
      if (first) {
        long long v[kPatRec];
#pragma unroll
        for (int k = 0; k < kPatRec; ++k) v[k] = 0;
        if (valid) {
          const long long yy = y[j] != 0, pred = m[kPmLabel * (long long)n + j] > 0.5f;
          const long long vq = pat_q(m[kPmVar * (long long)n + j]);
          v[0] = 1;
          v[1] = yy;
          v[2] = pred;
          v[3] = yy & pred;
          v[4] = yy == pred;
          v[5] = vq;
          v[6] = yy ? 0 : vq;
          v[7] = yy ? vq : 0;
          v[8] = pat_q(m[kPmEntNats * (long long)n + j]);
          v[9] = pat_q(m[kPmExpEnt * (long long)n + j]);
          v[10] = pat_q(m[kPmMI * (long long)n + j]);
          v[11] = pat_q(m[kPmEntBits * (long long)n + j]);
        }
        if (uniform) {
#pragma unroll
          for (int k = 0; k < kPatRec; ++k) a[k] += v[k];
        } else if (valid) {
#pragma unroll
          for (int k = 0; k < kPatRec; ++k)
            if (v[k] != 0)
              atomicAdd(reinterpret_cast<unsigned long long*>(&rec[(long long)cj * kPatRec + k]),
                        (unsigned long long)v[k]);
        }
      }
      // idle lanes and the passes beyond tn read a valid element too, so that the eight loads of a round
      // are issued together and not one behind a branch each
      const float* pp = probs + (long long)t0 * n + (in ? j : j_hi - 1);
      for (int tt = 0; tt < tn; tt += kPatUnroll) {
        float p[kPatUnroll];
#pragma unroll
        for (int u = 0; u < kPatUnroll; ++u) p[u] = pp[(long long)(tt + u < tn ? tt + u : tn - 1) * n];
#pragma unroll
        for (int u = 0; u < kPatUnroll; ++u) {
          if (tt + u >= tn) break;
          const bool pos = valid && p[u] > 0.5f;  // NaN and exactly 0.5 are not positive
          if (uniform) {
            const int cnt = __popcll(__ballot(pos));
            acc += lane == tt + u ? cnt : 0;
          } else if (pos) {
            atomicAdd(&pass_pos[(long long)(t0 + tt + u) * n_pat + cj], 1);
          }
        }
      }
    }
    pat_flush_pass(pass_pos, n_pat, t_count, t0, cur, lane, acc);
    if (first) pat_flush_rec(rec, cur, lane, a);
  }
}

constexpr int kPatFields = 25;     // S_in, columns of the per-patient record (ops/patient.py PREC_*)
constexpr int kPatTrueCls = 12;    // column of the true severity class (0..3)
constexpr int kPatPredCls = 13;    // column of the predicted severity class
constexpr int kPatConf = 16;       // 4 x 4 confusion counts
constexpr int kPatOut = kPatFields + kPatConf;   // S_out

// One workgroup per replicate.  Draw j of replicate b is idx[b, j] or the counter hash of
// bootstrap_kernel / calib_bootstrap_kernel with n = P.  Output columns [0, 25): the sums of the
// record columns over the draws; [25 + 4 true + pred]: confusion counts.  Draws outside [0, P) are
// skipped.  Integer sums; the wave partials are combined in a fixed order.
__global__ __launch_bounds__(kPatThreads) void patient_bootstrap_kernel(const long long* __restrict__ prec,
                                                                        const int* __restrict__ idx, unsigned seed,
                                                                        int n_pat, long long* __restrict__ out) {
  __shared__ long long red[kPatWaves][kPatFields];
  __shared__ unsigned conf[kPatWaves][kPatConf];
  APNEAUQ_DASSERT(blockDim.x == kPatThreads && n_pat >= 1);
  const int b = blockIdx.x;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  if ((int)threadIdx.x < kPatWaves * kPatConf) (&conf[0][0])[threadIdx.x] = 0u;
  __syncthreads();
  long long acc[kPatFields];
#pragma unroll
  for (int f = 0; f < kPatFields; ++f) acc[f] = 0;
  const unsigned bkey = boot_key(seed, (unsigned)b);
  const int* idx_b = idx ? idx + (long long)b * n_pat : nullptr;
  for (int j = threadIdx.x; j < n_pat; j += kPatThreads) {
    unsigned k;
    if (idx_b) {
      k = (unsigned)idx_b[j];
    } else {
      k = boot_draw(bkey, (unsigned)j, n_pat);
    }
    if (k >= (unsigned)n_pat) continue;
    const long long* r = prec + (long long)k * kPatFields;
#pragma unroll
    for (int f = 0; f < kPatFields; ++f) acc[f] += r[f];
    const int tc = (int)r[kPatTrueCls] & 3, pc = (int)r[kPatPredCls] & 3;
    atomicAdd(&conf[wave][tc * 4 + pc], 1u);
  }
#pragma unroll
  for (int f = 0; f < kPatFields; ++f) {
    const long long v = wave_sum(acc[f]);
    if (lane == 0) red[wave][f] = v;
  }
  __syncthreads();
  const int c = threadIdx.x;
  if (c < kPatOut) {
    long long v = 0;
    for (int w = 0; w < kPatWaves; ++w) v += c < kPatFields ? red[w][c] : (long long)conf[w][c - kPatFields];
    out[(long long)b * kPatOut + c] = v;
  }
}

hipError_t launch_patient_reduce(const float* probs, const float* m, const int* y, const int* code, int t_count, int n,
                                 int n_pat, int* pass_pos, long long* rec, hipStream_t stream) {
  if (n <= 0 || t_count <= 0 || n_pat <= 0) return hipSuccess;
  const int per_block = kPatWaves * kPatChunks * kWave;
  hipLaunchKernelGGL(patient_reduce_kernel, dim3((n + per_block - 1) / per_block), dim3(kPatThreads), 0, stream, probs,
                     m, y, code, t_count, n, n_pat, pass_pos, rec);
  return hipGetLastError();
}

hipError_t launch_patient_bootstrap(const long long* prec, const int* idx, unsigned seed, int n_pat, int n_boot,
                                    long long* out, hipStream_t stream) {
  if (n_boot <= 0 || n_pat <= 0) return hipSuccess;
  hipLaunchKernelGGL(patient_bootstrap_kernel, dim3(n_boot), dim3(kPatThreads), 0, stream, prec, idx, seed, n_pat, out);
  return hipGetLastError();
}

}  // namespace apneauq
