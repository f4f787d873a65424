// Helpers shared by every *_bindings.cpp: the current stream, launch-error and tensor checks.
#pragma once
#include <ATen/ATen.h>
#include <c10/core/DeviceGuard.h>
#include <c10/hip/HIPStream.h>
#include <torch/library.h>

#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace apneauq {
namespace bind {

inline hipStream_t cur_stream() { return c10::hip::getCurrentHIPStream().stream(); }

inline void check(hipError_t e, const char* what) {
  TORCH_CHECK(e == hipSuccess, what, " failed: ", hipGetErrorString(e));
}

inline bool aligned(const at::Tensor& t, uintptr_t bytes) {
  return reinterpret_cast<uintptr_t>(t.data_ptr()) % bytes == 0;
}

// contiguous, 16-B aligned GPU tensor of one dtype with at least min_numel elements
inline void need(const at::Tensor& t, at::ScalarType dt, int64_t min_numel, const char* what) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == dt && t.is_contiguous(), what, ": contiguous GPU tensor of dtype ", dt,
              " required");
  TORCH_CHECK(t.numel() >= min_numel, what, ": ", t.numel(), " elements, need >= ", min_numel);
  TORCH_CHECK(aligned(t, 16), what, ": 16-B alignment required");
}
// the fp32 form of the generic training path (its own wording)
inline void need_f32(const at::Tensor& t, int64_t n, const char* what) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kFloat && t.is_contiguous() && t.numel() >= n, what,
              ": fp32 contiguous GPU tensor of >= ", n, " elements required");
  TORCH_CHECK(aligned(t, 16), what, ": 16-B alignment required");
}
// activation buffers of the generic training path: (rows, c) bf16, or fp32 (precision="fp32")
inline void need_rows(const at::Tensor& t, int64_t rows, int64_t c, const char* what) {
  TORCH_CHECK(t.is_cuda() && (t.scalar_type() == at::kBFloat16 || t.scalar_type() == at::kFloat) && t.is_contiguous(), what,
              ": bf16 or fp32 contiguous GPU tensor required");
  TORCH_CHECK(t.numel() >= rows * c, what, ": buffer too small (", t.numel(), " < ", rows * c, ")");
  TORCH_CHECK(aligned(t, 16), what, ": 16-B alignment required");
}

// optional device-resident dropout stream key (int32, one element): graph-replayed steps
inline const unsigned* skey_dev_ptr(const c10::optional<at::Tensor>& t) {
  if (!t.has_value() || !t->defined()) return nullptr;
  TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kInt && t->numel() >= 1, "skey_dev: int32 GPU tensor");
  return reinterpret_cast<const unsigned*>(t->data_ptr<int>());
}

// optional (B, n) resampling indices as int32 (holder keeps the converted tensor alive); nullptr: the device
// draws them (common.h boot_draw).  what: "<op>: idx must be (B, <n>)"
inline const int* opt_idx(const c10::optional<at::Tensor>& idx, int64_t B, int64_t n, const char* what,
                          at::Tensor& holder) {
  if (!idx.has_value()) return nullptr;
  holder = idx->to(at::kInt).contiguous();
  TORCH_CHECK(holder.is_cuda() && holder.dim() == 2 && holder.size(0) == B && holder.size(1) == n, what,
              " on the GPU");
  return holder.data_ptr<int>();
}

}  // namespace bind
}  // namespace apneauq
