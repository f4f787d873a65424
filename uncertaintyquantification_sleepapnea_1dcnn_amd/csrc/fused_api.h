// Host interface of the fused whole-network inference kernels (fused_forward.hip, fused_tiled.hip,
// fused_tiled_x3.hip), included by those files and by fused_bindings.cpp.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace apneauq {
hipError_t launch_fused_forward(const void* x, const uint8_t* blob, long long blob_stride, float* out, int n_win,
                                int n_pass, int n_member, unsigned window_offset, unsigned pass_offset,
                                unsigned long long seed, int dropout, int out_logits, const unsigned* thr,
                                const float* dscale, int grid, hipStream_t stream);
int fused_blob_bytes();
int fused_lds_bytes();
void fused_layout(int* woffs, int* eoffs, int* dense_off);
hipError_t launch_fused_tiled(int net, const void* x, const uint8_t* blob, long long blob_stride, float* out,
                              int n_win, int n_pass, int n_member, unsigned window_offset, unsigned pass_offset,
                              unsigned long long seed, int dropout, int out_logits, const unsigned* thr,
                              hipStream_t stream);
int fused_pooled_lds_bytes();
hipError_t launch_fused_tiled_x3(int net, const float* x, const uint8_t* blob, long long blob_stride, float* out,
                                 int n_win, int n_pass, int n_member, unsigned window_offset, unsigned pass_offset,
                                 unsigned long long seed, int dropout, int out_logits, const unsigned* thr,
                                 hipStream_t stream);
void fused_layout_x3(int* woffs, int* eoffs, int* dense_off, int* bytes, int* lds);
}  // namespace apneauq
