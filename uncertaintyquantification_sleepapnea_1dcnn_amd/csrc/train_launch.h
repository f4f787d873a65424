// Host entries of the four training kernel families (train_fwd / train_head / train_dgrad / train_wgrad.hip),
// called by train_launch.hip.  One entry per family: Am == nullptr launches the single-model kernels (by-value
// Args, M ignored), otherwise the member-batched ones (gridDim.z = M members, Args from the device array Am).
// Every grid, LDS size and reduction shape comes from train_geo.h.
#pragma once
#include "train_args.h"

namespace apneauq {
namespace train {

hipError_t fwd_launch(const Args& A, const Args* Am, int M, int l, bool pf, hipStream_t st);
hipError_t tab_launch(const Args& A, const Args* Am, int M, int mode, int l, hipStream_t st);
hipError_t head_launch(const Args& A, const Args* Am, int M, int backward, int tabx, hipStream_t st);
hipError_t dgrad_launch(const Args& A, const Args* Am, int M, int l, const RedJob& rj, hipStream_t st);
hipError_t wgrad_launch(const Args& A, const Args* Am, int M, int l, bool fused, hipStream_t st);

// The reduction of wgrad<l>'s partials (row grouping of an M-member launch) at part.
inline RedJob red_job(const Args& A, int l, int M, const float* part) {
  const WgShape s = wg_shape(l, A.B, M, A.det != nullptr);
  return {part, A.L[l].gw, A.L[l].gb, s.rgs, s.kcc, s.cout, s.J, s.blocks};
}

}  // namespace train
}  // namespace apneauq
