// torch.library registration of the recalibration kernels (uq_recal.hip), namespace torch.ops.apneauq.
#include "bind_util.h"
#include "uq_api.h"

namespace {
using namespace apneauq::bind;

void check_fold(const at::Tensor& fold, int64_t n, int64_t F, const char* what) {
  TORCH_CHECK(fold.is_cuda() && fold.scalar_type() == at::kInt && fold.dim() == 1 &&
                  (fold.size(0) == n || (fold.size(0) == 0 && F == 1)),
              what, ": fold must be (n,) int32 on the GPU (or empty with one fold)");
}

// recal_sums: (F, Q, 12) fp64 sums of probs (T, n) fp32, y (n) uint8 and fold (n) int32 (empty: one fold) at the
// candidates thetas (Q, 3) fp64; objective 0 = joint, 1 = member.  range_len (ops/recal.py:range_len) fixes the order
// of the fp64 additions; grid (0: one workgroup per range) does not change the result.  Limits: T <= 128, Q <= 64,
// F <= 16, n <= 2^27, the planes and the (F, Q, 12) accumulator fit 160 KiB of LDS, the range partials 64 MB.
at::Tensor recal_sums(const at::Tensor& probs, const at::Tensor& y, const at::Tensor& fold, const at::Tensor& thetas,
                      int64_t n_folds, int64_t objective, int64_t range_len, int64_t grid) {
  TORCH_CHECK(probs.is_cuda() && probs.scalar_type() == at::kFloat && probs.dim() == 2,
              "recal_sums: probs must be (T, n) fp32 on the GPU");
  const int64_t T = probs.size(0), n = probs.size(1);
  TORCH_CHECK(T >= 1 && T <= apneauq::recal_max_t(), "recal_sums: T must be in 1..128");
  TORCH_CHECK(n >= 1 && n <= (int64_t(1) << 27), "recal_sums: n must be in 1..2^27");
  TORCH_CHECK(n_folds >= 1 && n_folds <= apneauq::recal_max_f(), "recal_sums: n_folds must be in 1..16");
  TORCH_CHECK(thetas.is_cuda() && thetas.scalar_type() == at::kDouble && thetas.dim() == 2 && thetas.size(1) == 3,
              "recal_sums: thetas must be (Q, 3) fp64 on the GPU");
  const int64_t Q = thetas.size(0);
  TORCH_CHECK(Q >= 1 && Q <= apneauq::recal_max_q(), "recal_sums: Q must be in 1..64");
  TORCH_CHECK(y.is_cuda() && y.scalar_type() == at::kByte && y.dim() == 1 && y.size(0) == n,
              "recal_sums: y must be (n,) uint8 on the GPU");
  check_fold(fold, n, n_folds, "recal_sums");
  TORCH_CHECK(objective == 0 || objective == 1, "recal_sums: objective must be 0 (joint) or 1 (member)");
  TORCH_CHECK(range_len >= 1 && grid >= 0 && grid < (int64_t(1) << 20), "recal_sums: bad range_len / grid");
  const int64_t n_ranges = (n + range_len - 1) / range_len;
  const int64_t slot = n_folds * Q * 12;
  TORCH_CHECK(n_ranges <= (int64_t(1) << 20) && n_ranges * slot * 8 <= (int64_t(64) << 20),
              "recal_sums: the range partials must stay within 64 MB");
  TORCH_CHECK(apneauq::recal_lds_bytes((int)T, (int)n_folds, (int)Q) <= apneauq::recal_max_lds(),
              "recal_sums: T planes and the (F, Q, 12) accumulator must fit 160 KiB of LDS (fewer candidates per call)");
  auto pp = probs.contiguous(), tt = thetas.contiguous(), yy = y.contiguous(), ff = fold.contiguous();
  const at::DeviceGuard guard(pp.device());
  auto part = at::empty({n_ranges * slot}, tt.options());
  auto out = at::empty({n_folds, Q, 12}, tt.options());
  check(apneauq::launch_recal_sums(pp.data_ptr<float>(), yy.data_ptr<uint8_t>(),
                                   ff.size(0) ? ff.data_ptr<int>() : nullptr, tt.data_ptr<double>(), (long long)n,
                                   (int)T, (int)Q, (int)n_folds, (int)objective, (long long)range_len, (int)grid,
                                   part.data_ptr<double>(), out.data_ptr<double>(), cur_stream()),
        "recal_sums");
  return out;
}

// recal_apply: (T, n) fp32, every window mapped by thetas[fold] (F, 3) fp64; NaN for a non-finite input or a fold
// code outside [0, F).
at::Tensor recal_apply(const at::Tensor& probs, const at::Tensor& fold, const at::Tensor& thetas) {
  TORCH_CHECK(probs.is_cuda() && probs.scalar_type() == at::kFloat && probs.dim() == 2,
              "recal_apply: probs must be (T, n) fp32 on the GPU");
  const int64_t T = probs.size(0), n = probs.size(1);
  TORCH_CHECK(T >= 0 && T < (int64_t(1) << 24) && n >= 0 && n <= (int64_t(1) << 36), "recal_apply: bad shape");
  TORCH_CHECK(thetas.is_cuda() && thetas.scalar_type() == at::kDouble && thetas.dim() == 2 && thetas.size(1) == 3,
              "recal_apply: thetas must be (F, 3) fp64 on the GPU");
  const int64_t F = thetas.size(0);
  TORCH_CHECK(F >= 1 && F <= apneauq::recal_max_f(), "recal_apply: F must be in 1..16");
  check_fold(fold, n, F, "recal_apply");
  auto pp = probs.contiguous(), tt = thetas.contiguous(), ff = fold.contiguous();
  if (reinterpret_cast<uintptr_t>(pp.data_ptr()) % 16 != 0) pp = pp.clone();
  const at::DeviceGuard guard(pp.device());
  auto out = at::empty({T, n}, pp.options());
  if (T == 0 || n == 0) return out;
  check(apneauq::launch_recal_apply(pp.data_ptr<float>(), ff.size(0) ? ff.data_ptr<int>() : nullptr,
                                    tt.data_ptr<double>(), (long long)n, (int)T, (int)F, out.data_ptr<float>(),
                                    cur_stream()),
        "recal_apply");
  return out;
}

}  // namespace

TORCH_LIBRARY_FRAGMENT(apneauq, m) {
  m.def("recal_sums(Tensor probs, Tensor y, Tensor fold, Tensor thetas, int n_folds, int objective, int range_len, "
        "int grid) -> Tensor");
  m.def("recal_apply(Tensor probs, Tensor fold, Tensor thetas) -> Tensor");
}

TORCH_LIBRARY_IMPL(apneauq, CUDA, m) {
  m.impl("recal_sums", &recal_sums);
  m.impl("recal_apply", &recal_apply);
}
