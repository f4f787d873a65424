// Host interface of the generic-spec kernels -- inference (generic_conv.hip), bf16 training (generic_train.hip,
// generic_wgrad.hip), fp32 (gf32_conv.hip) and fp16x3 (gx3_conv.hip) -- included by those files and by
// generic_bindings.cpp.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace apneauq {
// generic_conv.hip
hipError_t launch_generic_conv(const void* x, const void* wfrag, const float* epi, void* y, int n, int L, int cin,
                               int cout, int cout_pad, int ksize, int pool, int dropout, unsigned thr, int layer,
                               int n_win, unsigned pass_offset, unsigned window_offset, unsigned long long seed,
                               hipStream_t stream, int mode, int in_rs, int in_off, float* stats, long long x_rows,
                               int det_slots);
hipError_t launch_generic_head(const void* y, const float* w, float b, int n, int L, int C, int out_logits, float* out,
                               hipStream_t stream);
// generic_train.hip
hipError_t launch_gt_bn_finalize(const float* st, int nslots, int C, double inv_count, const float* gamma,
                                 const float* beta, float eps, float momentum, float* mmean, float* mvar, int update,
                                 float* bn, hipStream_t stream);
hipError_t launch_gt_apply(const void* z, const float* bn, void* out, int n, int L, int C, int pool, int out_rs,
                           int out_off, int dropout, unsigned thr, float inv_keep, unsigned skey,
                           unsigned window_offset, hipStream_t stream, const unsigned* skey_dev, int f32);
hipError_t launch_gt_bwd(int dz_mode, const void* z, const float* bn, const void* dh, const float* dlog,
                         const float* w, float invL, int n, int L, int C, int pool, int dropout, unsigned thr,
                         float inv_keep, unsigned skey, unsigned window_offset, float* bst, const float* coef,
                         const float* gamma, void* dz, int dz_rs, int dz_off, float* gbias, hipStream_t stream,
                         const unsigned* skey_dev, int det_slots, int f32);
hipError_t launch_gt_bwd_finalize(const float* bst, int nslots, int C, double inv_count, float* coef, float* ggamma,
                                  float* gbeta, const float* dbs, int bslots, int BC, float* gbias,
                                  hipStream_t stream);
// generic_wgrad.hip
hipError_t launch_ordered_sum(const float* part, int nrows, long long ncols, float* out, hipStream_t st);
hipError_t launch_gt_wgrad(const void* x, long long x_rows, const void* dz, long long R, int cin, int cout, int k,
                           float* gw, hipStream_t st, float* part, long long part_floats);
hipError_t launch_gt_head(const void* h, const float* w, const float* b, const float* y, float* prob, float* dlog,
                          float* loss, float* gw, float* gb, int n, int L, int C, float inv_gb, hipStream_t st,
                          float* part, long long part_floats, int f32);
int gt_pack_max_blocks();
int gt_pack_max_zero();
hipError_t launch_gt_pack(int nb, const float* const* w, void* const* fwd, void* const* dgr, const int* k,
                          const int* cin, const int* cout, hipStream_t st, int nz, void* const* zp,
                          const long long* zw);
// gf32_conv.hip
hipError_t launch_gf32_conv(const float* x, const float* w, const float* bias, float* y, float* stats, int n, int L,
                            int cin, int cout, int ksize, int mode, int in_rs, int in_off, int flip, int det_slots,
                            hipStream_t st);
hipError_t launch_gf32_wgrad(const float* x, const float* dz, long long R, int cin, int cout, int k, float* gw,
                             float* part, long long part_floats, hipStream_t st);
// gx3_conv.hip
int gx3_max_blocks();
hipError_t launch_gx3_pack(int nb, const float* const* w, void* const* fwd, void* const* dgr, float* const* wsc,
                           const int* k, const int* cin, const int* cout, float* wpart, hipStream_t st);
hipError_t launch_gx3_amax(const float* x, long long n, unsigned* out, hipStream_t st);
hipError_t launch_gx3_conv(const float* x, long long x_rows, const void* wfrag, const float* wsc, const float* bias,
                           float* y, float* stats, unsigned* amax_out, int n, int L, int cin, int cout, int ksize,
                           int mode, int in_rs, int in_off, int det_slots, hipStream_t st);
hipError_t launch_gx3_wgrad(const float* x, const float* dz, const unsigned* amax_x, const unsigned* amax_dz,
                            long long R, int cin, int cout, int k, float* gw, float* part, long long part_floats,
                            hipStream_t st);
}  // namespace apneauq
