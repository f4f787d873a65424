// Host interface of the optimizer / counter / step-edge kernels (adam.hip, the counter launchers of
// train_launch.hip), the streaming metrics (metrics.hip) and the preprocessing kernels (prep.hip), included by
// those files and by bindings.cpp.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace apneauq {
// adam.hip
int adam_max_sets();
hipError_t launch_adam_multi(int ns, float* const* p, const float* const* g, float* const* m, float* const* v,
                             const int* const* step, long long n, float b1, float b2, float alpha, float eps,
                             hipStream_t stream);
hipError_t launch_adam(float* p, const float* g, float* m, float* v, long long n, float b1, float b2, float alpha,
                       float eps, float gscale, const int* step_dev, hipStream_t stream);
int zero_max_buffers();
hipError_t launch_zero(int nb, void* const* ptrs, const long long* words, hipStream_t stream);
int train_tail_max();
hipError_t launch_train_tail(int* counters, int ncounters, int members, const float* const* logits,
                             float* const* probs, int n, hipStream_t stream);
hipError_t launch_train_inputs(int members, const float* const* x, void* const* xd, const float* const* y,
                               float* const* yd, int n, int L, int C, int SR, hipStream_t stream);
// train_launch.hip
hipError_t train_bump_counters(int* c, int n, hipStream_t st);
hipError_t train_stream_keys(unsigned* keys, const int* c, int n, unsigned long long seed, unsigned pass_base,
                             hipStream_t st);
// metrics.hip
hipError_t launch_metrics_update(const float* p, const float* y, long long n, const float* thr, int n_thr,
                                 unsigned long long* counts, hipStream_t stream);
// prep.hip
hipError_t launch_standardize(const double* x, double* out, long long n_win, int L, int C, double eps,
                              hipStream_t stream);
hipError_t launch_knn(const double* X, int n, int D, long long* out, int k, hipStream_t stream);
int knn_lds_bytes(int D, int K);
}  // namespace apneauq
