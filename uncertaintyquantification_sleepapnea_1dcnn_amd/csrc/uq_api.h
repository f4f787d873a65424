// Host interface of the UQ reduction kernels (uq_reduce.hip, uq_calib.hip, uq_patient.hip, uq_rank.hip,
// uq_conformal.hip, uq_laplace.hip, uq_converge.hip, uq_recal.hip, uq_shift.hip, uq_members.hip), included by those files and by
// uq_bindings.cpp / recal_bindings.cpp.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace apneauq {
// uq_reduce.hip
hipError_t launch_uq_reduce(const float* probs, int t_count, int n, float* out, hipStream_t stream);
hipError_t launch_bootstrap(const float* metrics, const int* y, const int* idx, unsigned seed, int n, int n_boot,
                            double* out, hipStream_t stream);
hipError_t launch_bootstrap_partial(const float* metrics, const int* y, const int* idx, unsigned seed, int n, int lo,
                                    int n_loc, int n_boot, double* out, hipStream_t stream);
// uq_calib.hip
hipError_t launch_calib_prep(const float* p, const float* score, const int* y, const float* thr, int n, int n_bins,
                             int n_thr, int* rec, hipStream_t stream);
hipError_t launch_calib_bootstrap(const int* rec, const int* idx, unsigned seed, int n, int lo, int n_loc, int n_boot,
                                  int n_bins, int n_thr, int slices, long long* out, hipStream_t stream);
// uq_patient.hip
hipError_t launch_patient_reduce(const float* probs, const float* m, const int* y, const int* code, int t_count, int n,
                                 int n_pat, int* pass_pos, long long* rec, hipStream_t stream);
hipError_t launch_patient_bootstrap(const long long* prec, const int* idx, unsigned seed, int n_pat, int n_boot,
                                    long long* out, hipStream_t stream);
// uq_rank.hip
int rank_max_splits();
hipError_t launch_rank_count(const int* pos, const int* idx, unsigned seed, int n_draw, int n_sorted, int b0, int n_boot,
                             long long stride, int* w, hipStream_t stream);
hipError_t launch_rank_totals(const int* w, long long stride, const unsigned char* packed, const int* bounds, int n,
                              int n_boot, int splits, long long* tot, hipStream_t stream);
hipError_t launch_rank_scan(const int* w, long long stride, const unsigned char* packed, const int* bounds,
                            const long long* tot, int n, int n_boot, int splits, long long* part, hipStream_t stream);
// uq_conformal.hip
int conformal_tile();
int conformal_max_segments();
int conformal_max_alpha();
int conformal_max_cuts();
hipError_t launch_conformal_select(const int* unit, const unsigned char* packed, const int* within, const int* ucount,
                                   int n_units, int n, int span, unsigned seed, int r0, int n_splits,
                                   unsigned long long cal_thr, const int* alpha_ppm, int n_alpha, int strata, int* totals,
                                   int* member, hipStream_t stream);
hipError_t launch_conformal_count(const int* unit, const unsigned char* packed, const int* within, const int* ucount,
                                  int n_units, int n, int span, unsigned seed, int r0, int n_splits,
                                  unsigned long long cal_thr, const int* cuts, int n_cuts, int* out, hipStream_t stream);
// uq_laplace.hip
int laplace_max_dp();
long long laplace_part_doubles(int D);
hipError_t launch_laplace_gram(const float* phi, const double* theta, const unsigned char* y, long long n, int D,
                               long long range_len, int grid, double* part, double* out, hipStream_t stream);
hipError_t launch_laplace_predict(const float* phi, const double* mx, long long n, int D, int T, float* preds,
                                  double* mu, double* vv, double* probit, hipStream_t stream);
// uq_converge.hip
hipError_t launch_converge(const float* probs, const int* y, const int* orders, const int* counts, int t_count, int n,
                           int n_rep, int n_cnt, int rep_groups, long long* out, hipStream_t stream);
// uq_recal.hip
int recal_max_t();
int recal_max_q();
int recal_max_f();
int recal_max_lds();
long long recal_lds_bytes(int T, int F, int Q);
hipError_t launch_recal_sums(const float* probs, const unsigned char* y, const int* fold, const double* thetas,
                             long long n, int T, int Q, int F, int objective, long long range_len, int grid,
                             double* part, double* out, hipStream_t stream);
hipError_t launch_recal_apply(const float* probs, const int* fold, const double* thetas, long long n, int T, int F,
                              float* out, hipStream_t stream);
// uq_shift.hip: the K conditions of a launch travel by value (kind code, parameter p, channel bit mask)
constexpr int kShiftMaxK = 64, kShiftMaxL = 256, kShiftMaxC = 4, kShiftKinds = 8;
struct ShiftConds {
  double p[kShiftMaxK];
  unsigned char kind[kShiftMaxK];
  unsigned char mask[kShiftMaxK];
};
hipError_t launch_shift_corrupt(const void* x, bool x_is_double, long long n, int L, int C, const ShiftConds& conds,
                                int K, unsigned long long seed, unsigned long long window_offset, bool restandardize,
                                float* out, hipStream_t stream);
// uq_members.hip
int member_max_t();
int member_max_q();
int member_max_f();
hipError_t launch_member_pairs(const float* probs, const int* y, int t_count, int n, int grid, int slices,
                               long long* out, long long* head, hipStream_t stream);
hipError_t launch_member_mix(const float* probs, const int* y, const unsigned char* fold, const int* counts,
                             int t_count, int n, int n_rows, int n_folds, int grid, long long* out,
                             hipStream_t stream);
}  // namespace apneauq
