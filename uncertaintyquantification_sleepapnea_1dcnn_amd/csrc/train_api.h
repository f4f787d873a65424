// Host interface of the layer-wise training kernels (train_launch.hip), included by that file and by
// train_bindings.cpp.  The argument block is in train_ctx.h.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "train_ctx.h"

namespace apneauq {
long long train_wgrad_part_floats(int B);
int train_det_floats(int B);
hipError_t train_launch_fwd(const train::Args& A, int l, hipStream_t st);
hipError_t train_launch_tab(const train::Args& A, int mode, int l, hipStream_t st);
hipError_t train_launch_head(const train::Args& A, int backward, hipStream_t st, bool with_tab);
hipError_t train_launch_dgrad(const train::Args& A, int l, hipStream_t st, bool fused);
hipError_t train_launch_wgrad(const train::Args& A, int l, hipStream_t st, bool fused);
hipError_t train_launch_finalize(const train::Args& A, int update_moving, int grads, hipStream_t st, bool fused);
hipError_t train_launch_mb(const train::Args& A0, const train::Args* Am, int M, int op, int layer, int flag,
                           hipStream_t st);
}  // namespace apneauq
