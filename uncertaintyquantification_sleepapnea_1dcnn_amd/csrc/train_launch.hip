// Layer-wise training kernels of the Alarcón 1D-CNN on gfx950 (MI355X): forward with batch-
// statistics BatchNorm, head (GAP + Dense + BCE + its gradient), conv dgrad / wgrad, BN finalize.
//
// Replaces the TF/cuDNN work inside model.fit (cnn_baseline_train.py:210, train_deep_ensemble_cnns.py:158;
// SURVEY K1-K8).  Keras semantics: ReLU inside the conv, BN on biased batch moments (eps 1e-3,
// momentum 0.99), inverted dropout (counter-based masks, ops/rng.py), BCE on logits, batch mean.
//
// Data layout ("padded rows", PL): an activation buffer holds 4 leading zero rows, then every
// sample as a 64-row slot (60 time steps + 4 zero rows), channels contiguous, bf16.  A workgroup
// tile = 2 samples = rows [128*tile, 128*tile + 136) — one contiguous copy including the conv halo.
//
// Per block l the buffers are R_l = relu(conv(A_{l-1}) + b) (pre-BN, bf16) and dY_l = dL/dBN-output
// (bf16).  R_l >= 0, so its sign bit is free: the producer stores the dropout mask of block l there
// (sign set = dropped; |R_l| is the activation), hashing each element's mask exactly once.  BN apply
// + dropout of block l are never materialised: the consumer of A_l (the next forward, the wgrad of
// block l+1) recomputes  A_l = [sign clear] * (|R_l| * s + t) / (1-p)  while staging into LDS (no
// hash), and the consumers of dZ_l (dgrad / wgrad of block l) recompute
//   dZ_l = [R_l > 0] * gamma * rstd * (dY_l - mean(dY_l) - xhat * mean(dY_l * xhat))
// from the per-channel sums accumulated by the producer's epilogue (moments: fp32 per-workgroup
// partials merged into fp64 slots, so batch statistics over ~10^6 rows per channel (MC Dropout with
// the whole test set as one batch) keep ~1e-7 relative precision; backward sums: fp32).  dgrad_l also
// writes its staged dZ_l rows to global memory, so wgrad_l (whose ci-blocked workgroups would each
// recompute the whole dZ tile) stages it with a plain copy.
//
// Forward and dgrad are implicit GEMMs on v_mfma_f32_16x16x32_bf16 with the weights as the A operand
// (pre-packed fragments from global/L2) and the staged activations as the B operand (LDS,
// ds_read_b128).  wgrad reduces over rows, so both operands are read with the CDNA4 transposing
// LDS read ds_read_b64_tr_b16 from row-major tiles; each workgroup sums up to 16 row tiles in
// registers and writes its output block to a per-row-group partial slot (Args::wpart), which
// wgrad_reduce_kernel adds in a fixed order (deterministic, and cheaper than fp32 atomics).
//
// Files: the kernels are in train_fwd.hip, train_head.hip (parameter table + head), train_dgrad.hip and
// train_wgrad.hip, the device code they share in train_stage.h, the reductions in train_reduce.hip.  This
// file holds the host interface (train_api.h): which launches a step op is, and the deterministic-reduce
// glue.  Every grid, row grouping and buffer size is stated once, in train_geo.h.
#include "misc_api.h"
#include "train_api.h"
#include "train_launch.h"

namespace apneauq {
using train::Args;

long long train_wgrad_part_floats(int B) { return train::wgrad_part_floats(B); }
int train_det_floats(int B) { return train::det_floats(B); }

__global__ void bump_counters_kernel(int* c, int n) {
  if (threadIdx.x < n) c[threadIdx.x] += 1;
}

hipError_t train_bump_counters(int* c, int n, hipStream_t st) {
  hipLaunchKernelGGL(bump_counters_kernel, dim3(1), dim3(64), 0, st, c, n);
  return hipGetLastError();
}

// Dropout stream keys of one training step computed on the device from the step counter c[0]
// (keys[l] = stream_key(seed, l, pass_base + c[0])): a graph replay reads no host-written key array.
__global__ void stream_keys_kernel(unsigned* keys, const int* c, int n, unsigned long long seed, unsigned pass_base) {
  if (threadIdx.x < n) keys[threadIdx.x] = stream_key(seed, threadIdx.x, pass_base + (unsigned)c[0]);
}

hipError_t train_stream_keys(unsigned* keys, const int* c, int n, unsigned long long seed, unsigned pass_base,
                             hipStream_t st) {
  hipLaunchKernelGGL(stream_keys_kernel, dim3(1), dim3(64), 0, st, keys, c, n, seed, pass_base);
  return hipGetLastError();
}

// ---- deterministic mode: what each reduction sums (train::det_rows_*) and where the sums go
static train::DetDst det_dst(void* p0, int c0, int f0, void* p1 = nullptr, int c1 = 0, void* p2 = nullptr, int c2 = 0,
                             void* p3 = nullptr, int c3 = 0, int f3 = 0) {
  train::DetDst d;
  d.seg[0] = {p0, c0, f0};
  d.seg[1] = {p1, c1, 0};
  d.seg[2] = {p2, c2, 0};
  d.seg[3] = {p3, c3, f3};
  return d;
}
// The partial table at A.det (r.n rows of r.w) -> d, through the fp64 segment scratch behind the table.
// Am != nullptr: every member's table -> the destinations of its step op (op, l), picked on the device.
static hipError_t det_reduce(const Args& A, const Args* Am, int M, train::DetRows r, const train::DetDst& d, int op, int l,
                             hipStream_t st) {
  if (r.w > train::kDetMaxW) return hipErrorInvalidValue;
  const long long sb = train::det_scratch_base(A.B);
  if (Am != nullptr) {
    hipLaunchKernelGGL(train::det_pass1_mb_kernel, dim3((r.w + 63) / 64, train::kDetSeg, M), dim3(256), 0, st, Am, r.n,
                       r.w, sb);
    hipLaunchKernelGGL(train::det_pass2_mb_kernel, dim3((r.w + 255) / 256, 1, M), dim3(256), 0, st, Am, op, l, r.w, sb);
  } else {
    double* scr = reinterpret_cast<double*>(A.det + sb);
    hipLaunchKernelGGL(train::det_pass1_kernel, dim3((r.w + 63) / 64, train::kDetSeg), dim3(256), 0, st, A.det, r.n, r.w,
                       scr);
    hipLaunchKernelGGL(train::det_pass2_kernel, dim3((r.w + 255) / 256), dim3(256), 0, st, scr, r.w, d);
  }
  return hipGetLastError();
}

// ---- the step ops.  Am == nullptr: the single-model launch (train_launch_*), else M members (train_launch_mb)
static hipError_t op_fwd(const Args& A, const Args* Am, int M, int l, hipStream_t st) {
  const bool det = A.det != nullptr;
  if (det && (A.groups != 1 || A.shared0)) return hipErrorInvalidValue;  // deterministic: ordered moment reduction
  // persistent forward (never deterministic): each workgroup over a contiguous tile range
  const bool pf = train::fwd_pf(A.B, M, l, det, A.groups, A.shared0);
  const hipError_t e = train::fwd_launch(A, Am, M, l, pf, st);
  if (e != hipSuccess || !det) return e;
  const int cc = train::C[l + 1];
  return det_reduce(A, Am, M, train::det_rows_fwd(A.B, l), det_dst(A.L[l].st, 2 * cc, 1), 0, l, st);
}

static hipError_t op_head(const Args& A, const Args* Am, int M, int backward, int tabx, hipStream_t st) {
  const hipError_t e = train::head_launch(A, Am, M, backward, tabx, st);
  if (e != hipSuccess || !backward || A.det == nullptr) return e;
  constexpr int cc = train::C[6];  // per-sample records: loss, dlogit, dW, sum dY, sum dY xhat
  return det_reduce(A, Am, M, train::det_rows_head(A.B),
                    det_dst(A.loss_sum, 1, 0, A.g_dense_b, 1, A.g_dense_w, cc, A.L[5].bst, 2 * cc, 1), 1, 0, st);
}

static hipError_t op_dgrad(const Args& A, const Args* Am, int M, int l, const train::RedJob& rj, hipStream_t st) {
  const hipError_t e = train::dgrad_launch(A, Am, M, l, rj, st);
  if (e != hipSuccess || A.det == nullptr) return e;
  const int cc = train::C[l];
  return det_reduce(A, Am, M, train::det_rows_dgrad(A.B, l), det_dst(A.L[l - 1].bst, 2 * cc, 1), 2, l, st);
}

// The fused single-device step (Python: train_ops.FUSED_REDUCE): atomic mode with the parameter table and
// wgrad partials, backward BN rows from the table.
static bool fused_ok(const Args& A) {
  return A.tab != nullptr && A.det == nullptr && A.wpart != nullptr && A.groups == 1 && !A.bwd_self;
}

hipError_t train_launch_fwd(const Args& A, int l, hipStream_t st) { return op_fwd(A, nullptr, 1, l, st); }

hipError_t train_launch_tab(const Args& A, int mode, int l, hipStream_t st) {
  if (A.tab == nullptr) return hipSuccess;  // no table (multi-rank / deterministic / MC-Dropout ctx)
  if (l < 0 || l >= 6) return hipErrorInvalidValue;
  return train::tab_launch(A, nullptr, 1, mode, l, st);
}

hipError_t train_launch_head(const Args& A, int backward, hipStream_t st, bool with_tab) {
  const int tabx = (with_tab && A.tab != nullptr) ? 6 : 0;  // + the table's forward rows, one workgroup per block
  return op_head(A, nullptr, 1, backward, tabx, st);
}

// fused (l <= 4): the launch also reduces wgrad<l+1>'s partials, which the previous launch wrote
hipError_t train_launch_dgrad(const Args& A, int l, hipStream_t st, bool fused) {
  if (l < 1 || l > 5) return hipErrorInvalidValue;  // before red_job indexes A.L[l + 1]
  if (fused && (!fused_ok(A) || l > 4)) return hipErrorInvalidValue;
  return op_dgrad(A, nullptr, 1, l, fused ? train::red_job(A, l + 1, 1, A.wpart) : train::RedJob{}, st);
}

hipError_t train_launch_wgrad(const Args& A, int l, hipStream_t st, bool fused) {
  if (A.groups != 1) return hipErrorInvalidValue;  // training: one stats group (the staging's single affine)
  if (fused && !fused_ok(A)) return hipErrorInvalidValue;
  return train::wgrad_launch(A, nullptr, 1, l, fused, st);
}

// fused: BN finalize and the reductions of wgrad<1> / wgrad<0>'s partials in one launch
hipError_t train_launch_finalize(const Args& A, int update_moving, int grads, hipStream_t st, bool fused) {
  if (!fused) {
    hipLaunchKernelGGL(train::bn_finalize_kernel<false>, dim3(6), dim3(256), 0, st, A, nullptr, update_moving, grads);
    return hipGetLastError();
  }
  if (!fused_ok(A)) return hipErrorInvalidValue;
  const train::RedJob j1 = train::red_job(A, 1, 1, A.wpart),
                      j0 = train::red_job(A, 0, 1, A.wpart + train::wg_main_floats(A.B));
  hipLaunchKernelGGL(train::step_reduce_kernel, dim3(6 + j1.blocks + j0.blocks), dim3(256), 0, st, A, j1, j0,
                     update_moving, grads);
  return hipGetLastError();
}

// Member-batched training step ops (one launch for M ensemble members of identical batch size):
// A0 = member 0's Args (host copy: sizes and flags, identical for every member), Am = the device array of
// all M members' Args.  op: 0 fwd(layer) | 1 head(flag = backward) | 2 dgrad(layer) | 3 wgrad(layer)
// | 4 finalize(layer = update_moving, flag = grads) | 5 forward rows of the parameter table.
// Single-device training only (no shared block 1).  Deterministic mode (every member with partial
// tables, A0.det set): each reduction is followed by the two det passes over all members.
hipError_t train_launch_mb(const Args& A0, const Args* Am, int M, int op, int layer, int flag, hipStream_t st) {
  if (M < 1 || M > 65535 || Am == nullptr || A0.shared0 || A0.groups != 1) return hipErrorInvalidValue;
  if (A0.det != nullptr && A0.tab != nullptr) return hipErrorInvalidValue;
  switch (op) {
    case 0: return op_fwd(A0, Am, M, layer, st);
    case 1: return op_head(A0, Am, M, flag, 0, st);
    case 2: return op_dgrad(A0, Am, M, layer, train::RedJob{}, st);
    case 3: return train::wgrad_launch(A0, Am, M, layer, false, st);
    case 4:
      hipLaunchKernelGGL(train::bn_finalize_kernel<true>, dim3(6, 1, M), dim3(256), 0, st, A0, Am, layer, flag);
      return hipGetLastError();
    case 5:
      if (A0.tab == nullptr) return hipSuccess;
      return train::tab_launch(A0, Am, M, 0, 0, st);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace apneauq
