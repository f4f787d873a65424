// torch.library registration of the UQ reduction kernels (uq_reduce.hip, uq_calib.hip, uq_patient.hip, uq_rank.hip,
// uq_conformal.hip, uq_laplace.hip, uq_converge.hip, uq_shift.hip, uq_members.hip), namespace torch.ops.apneauq.
#include "bind_util.h"
#include "uq_api.h"

#include <cmath>
#include <tuple>

namespace {
using namespace apneauq::bind;

at::Tensor uq_reduce(const at::Tensor& probs) {
  TORCH_CHECK(probs.is_cuda() && probs.scalar_type() == at::kFloat && probs.dim() == 2,
              "uq_reduce: probs must be a (T, N) float32 GPU tensor");
  auto p = probs.contiguous();
  const at::DeviceGuard guard(p.device());
  auto out = at::empty({7, p.size(1)}, p.options());
  check(apneauq::launch_uq_reduce(p.data_ptr<float>(), (int)p.size(0), (int)p.size(1), out.data_ptr<float>(),
                                  cur_stream()),
        "uq_reduce");
  return out;
}

at::Tensor bootstrap(const at::Tensor& metrics, const at::Tensor& y, const c10::optional<at::Tensor>& idx,
                     int64_t seed, int64_t n_boot) {
  TORCH_CHECK(metrics.is_cuda() && metrics.scalar_type() == at::kFloat && metrics.dim() == 2 && metrics.size(0) == 7,
              "bootstrap: metrics must be the (7, N) output of uq_reduce");
  const int64_t n = metrics.size(1);
  auto m = metrics.contiguous();
  auto yy = y.to(at::kInt).contiguous();
  TORCH_CHECK(yy.is_cuda() && yy.numel() == n, "bootstrap: y must be (N,) on the GPU");
  at::Tensor ii;
  const int* ip = opt_idx(idx, n_boot, n, "bootstrap: idx must be (B, N)", ii);
  const at::DeviceGuard guard(m.device());
  auto out = at::empty({n_boot, 6}, m.options().dtype(at::kDouble));
  check(apneauq::launch_bootstrap(m.data_ptr<float>(), yy.data_ptr<int>(), ip, (unsigned)seed, (int)n, (int)n_boot,
                                  out.data_ptr<double>(), cur_stream()),
        "bootstrap");
  return out;
}

// Sharded bootstrap: raw (B, 8) sums over the draws landing in this rank's windows
// [lo, lo + n_loc) of n_global; summed over ranks by the caller, then turned into the 6 means.
at::Tensor bootstrap_partial(const at::Tensor& metrics, const at::Tensor& y, const c10::optional<at::Tensor>& idx,
                             int64_t seed, int64_t n_boot, int64_t n_global, int64_t lo) {
  TORCH_CHECK(metrics.is_cuda() && metrics.scalar_type() == at::kFloat && metrics.dim() == 2 && metrics.size(0) == 7,
              "bootstrap_partial: metrics must be the (7, n_loc) output of uq_reduce");
  const int64_t n_loc = metrics.size(1);
  TORCH_CHECK(lo >= 0 && lo + n_loc <= n_global && n_global < (int64_t(1) << 31), "bootstrap_partial: bad shard");
  auto m = metrics.contiguous();
  auto yy = y.to(at::kInt).contiguous();
  TORCH_CHECK(yy.is_cuda() && yy.numel() == n_loc, "bootstrap_partial: y must be (n_loc,) on the GPU");
  at::Tensor ii;
  const int* ip = opt_idx(idx, n_boot, n_global, "bootstrap_partial: idx must be (B, n_global)", ii);
  const at::DeviceGuard guard(m.device());
  auto out = at::empty({n_boot, 8}, m.options().dtype(at::kDouble));
  check(apneauq::launch_bootstrap_partial(m.data_ptr<float>(), yy.data_ptr<int>(), ip, (unsigned)seed, (int)n_global,
                                          (int)lo, (int)n_loc, (int)n_boot, out.data_ptr<double>(), cur_stream()),
        "bootstrap_partial");
  return out;
}

// Calibration / selective prediction (uq_calib.hip): per-window integer records, then the bootstrap
// histogram sums.  Limits: K <= 32 bins, J <= 64 thresholds, n <= 2^27 (sum nll_q stays below 2^63).
at::Tensor calib_prep(const at::Tensor& p, const at::Tensor& score, const at::Tensor& y, const at::Tensor& thr,
                      int64_t n_bins) {
  TORCH_CHECK(p.is_cuda() && p.scalar_type() == at::kFloat && p.dim() == 1, "calib_prep: p must be (N,) float32 on the GPU");
  const int64_t n = p.size(0), n_thr = thr.numel();
  TORCH_CHECK(score.is_cuda() && score.scalar_type() == at::kFloat && score.dim() == 1 && score.size(0) == n,
              "calib_prep: score must be (N,) float32 on the GPU");
  TORCH_CHECK(thr.is_cuda() && thr.scalar_type() == at::kFloat && thr.dim() == 1,
              "calib_prep: thr must be (J,) float32 on the GPU");
  TORCH_CHECK(n_bins >= 1 && n_bins <= 32, "calib_prep: n_bins must be in 1..32");
  TORCH_CHECK(n_thr <= 64, "calib_prep: at most 64 thresholds");
  TORCH_CHECK(n <= (int64_t(1) << 27), "calib_prep: at most 2^27 windows");
  auto pp = p.contiguous(), ss = score.contiguous(), tt = thr.contiguous();
  auto yy = y.to(at::kInt).contiguous();
  TORCH_CHECK(yy.is_cuda() && yy.dim() == 1 && yy.size(0) == n, "calib_prep: y must be (N,) on the GPU");
  const at::DeviceGuard guard(pp.device());
  auto rec = at::empty({n, 4}, pp.options().dtype(at::kInt));
  check(apneauq::launch_calib_prep(pp.data_ptr<float>(), ss.data_ptr<float>(), yy.data_ptr<int>(), tt.data_ptr<float>(),
                                   (int)n, (int)n_bins, (int)n_thr, rec.data_ptr<int>(), cur_stream()),
        "calib_prep");
  return rec;
}

at::Tensor calib_bootstrap(const at::Tensor& rec, const c10::optional<at::Tensor>& idx, int64_t seed, int64_t n_boot,
                           int64_t n_global, int64_t lo, int64_t n_bins, int64_t n_thr, int64_t slices) {
  TORCH_CHECK(rec.is_cuda() && rec.scalar_type() == at::kInt && rec.dim() == 2 && rec.size(1) == 4,
              "calib_bootstrap: rec must be the (n_loc, 4) int32 output of calib_prep");
  const int64_t n_loc = rec.size(0);
  TORCH_CHECK(n_bins >= 1 && n_bins <= 32, "calib_bootstrap: n_bins must be in 1..32");
  TORCH_CHECK(n_thr >= 0 && n_thr <= 64, "calib_bootstrap: n_thr must be in 0..64");
  TORCH_CHECK(n_global >= 1 && n_global <= (int64_t(1) << 27), "calib_bootstrap: n_global must be in 1..2^27");
  TORCH_CHECK(lo >= 0 && lo + n_loc <= n_global, "calib_bootstrap: bad shard");
  TORCH_CHECK(n_boot >= 0 && n_boot < (int64_t(1) << 31), "calib_bootstrap: bad n_boot");
  TORCH_CHECK(slices >= 1 && slices <= 1024, "calib_bootstrap: slices must be in 1..1024");
  auto rr = rec.contiguous();
  TORCH_CHECK(reinterpret_cast<uintptr_t>(rr.data_ptr()) % 16 == 0, "calib_bootstrap: 16-B alignment required");
  at::Tensor ii;
  const int* ip = opt_idx(idx, n_boot, n_global, "calib_bootstrap: idx must be (B, n_global)", ii);
  const int64_t n_col = 3 * n_bins + 4 * (n_thr + 1) + 2;
  const at::DeviceGuard guard(rr.device());
  auto slabs = at::empty({n_boot, slices, n_col}, rr.options().dtype(at::kLong));
  check(apneauq::launch_calib_bootstrap(rr.data_ptr<int>(), ip, (unsigned)seed, (int)n_global, (int)lo, (int)n_loc,
                                        (int)n_boot, (int)n_bins, (int)n_thr, (int)slices,
                                        reinterpret_cast<long long*>(slabs.data_ptr<int64_t>()), cur_stream()),
        "calib_bootstrap");
  return slices == 1 ? slabs.select(1, 0) : slabs.sum(1);
}

// Patient-level sums (uq_patient.hip).  Limits: n <= 2^27 windows (a fixed-point term is at most 2^32, so every
// rec sum stays below 2^59), T <= 65536, P <= 2^24 and T P < 2^31.  Windows with a code outside [0, P) are skipped.
std::tuple<at::Tensor, at::Tensor> patient_reduce(const at::Tensor& probs, const at::Tensor& m, const at::Tensor& y,
                                                  const at::Tensor& code, int64_t n_pat) {
  TORCH_CHECK(probs.is_cuda() && probs.scalar_type() == at::kFloat && probs.dim() == 2,
              "patient_reduce: probs must be a (T, n) float32 GPU tensor");
  const int64_t t_count = probs.size(0), n = probs.size(1);
  TORCH_CHECK(m.is_cuda() && m.scalar_type() == at::kFloat && m.dim() == 2 && m.size(0) == 7 && m.size(1) == n,
              "patient_reduce: m must be the (7, n) output of uq_reduce");
  TORCH_CHECK(t_count >= 1 && t_count <= 65536, "patient_reduce: T must be in 1..65536");
  TORCH_CHECK(n >= 1 && n <= (int64_t(1) << 27), "patient_reduce: n must be in 1..2^27");
  TORCH_CHECK(n_pat >= 1 && n_pat <= (int64_t(1) << 24) && t_count * n_pat < (int64_t(1) << 31),
              "patient_reduce: P must be in 1..2^24 with T P < 2^31");
  TORCH_CHECK(code.is_cuda() && code.scalar_type() == at::kInt && code.dim() == 1 && code.size(0) == n,
              "patient_reduce: code must be (n,) int32 on the GPU");
  auto pp = probs.contiguous(), mm = m.contiguous(), cc = code.contiguous();
  auto yy = y.to(at::kInt).contiguous();
  TORCH_CHECK(yy.is_cuda() && yy.dim() == 1 && yy.size(0) == n, "patient_reduce: y must be (n,) on the GPU");
  const at::DeviceGuard guard(pp.device());
  auto pass_pos = at::zeros({t_count, n_pat}, pp.options().dtype(at::kInt));
  auto rec = at::zeros({n_pat, 12}, pp.options().dtype(at::kLong));
  check(apneauq::launch_patient_reduce(pp.data_ptr<float>(), mm.data_ptr<float>(), yy.data_ptr<int>(),
                                       cc.data_ptr<int>(), (int)t_count, (int)n, (int)n_pat, pass_pos.data_ptr<int>(),
                                       reinterpret_cast<long long*>(rec.data_ptr<int64_t>()), cur_stream()),
        "patient_reduce");
  return {pass_pos, rec};
}

// Patient-cluster bootstrap: (B, 41) sums of the (P, 25) per-patient records over P draws per replicate.
// Limits: P <= 2^20 and P max|prec| < 2^63, so that no replicate (which may draw one patient P times) overflows.
at::Tensor patient_bootstrap(const at::Tensor& prec, const c10::optional<at::Tensor>& idx, int64_t seed,
                             int64_t n_boot) {
  TORCH_CHECK(prec.is_cuda() && prec.scalar_type() == at::kLong && prec.dim() == 2 && prec.size(1) == 25,
              "patient_bootstrap: prec must be a (P, 25) int64 GPU tensor");
  const int64_t n_pat = prec.size(0);
  TORCH_CHECK(n_pat >= 1 && n_pat <= (int64_t(1) << 20), "patient_bootstrap: P must be in 1..2^20");
  TORCH_CHECK(n_boot >= 0 && n_boot < (int64_t(1) << 31), "patient_bootstrap: bad n_boot");
  auto rr = prec.contiguous();
  const int64_t lo = rr.min().item<int64_t>(), hi = rr.max().item<int64_t>();
  const int64_t lim = INT64_MAX / n_pat;
  TORCH_CHECK(lo >= -lim && hi <= lim, "patient_bootstrap: P max|prec| must stay below 2^63");
  at::Tensor ii;
  const int* ip = opt_idx(idx, n_boot, n_pat, "patient_bootstrap: idx must be (B, P)", ii);
  const at::DeviceGuard guard(rr.device());
  auto out = at::empty({n_boot, 41}, rr.options());
  check(apneauq::launch_patient_bootstrap(reinterpret_cast<const long long*>(rr.data_ptr<int64_t>()), ip, (unsigned)seed,
                                          (int)n_pat, (int)n_boot, reinterpret_cast<long long*>(out.data_ptr<int64_t>()),
                                          cur_stream()),
        "patient_bootstrap");
  return out;
}

// Rank statistics (uq_rank.hip).  rank_count: (B, n_sorted) int32 multiplicities of the sorted windows in replicates
// b0 .. b0 + B - 1, rows 16-B aligned (the result is a view of a (B, n_sorted rounded up to 4) buffer).  Limits:
// at most 2^27 draws per replicate, so a replicate's total weight stays below 2^31.
at::Tensor rank_count(const at::Tensor& pos, const c10::optional<at::Tensor>& idx, int64_t seed, int64_t b0,
                      int64_t n_boot, int64_t n_sorted) {
  TORCH_CHECK(pos.is_cuda() && pos.scalar_type() == at::kInt && pos.dim() == 1,
              "rank_count: pos must be (n,) int32 on the GPU");
  const int64_t n_draw = pos.size(0);
  TORCH_CHECK(n_draw >= 1 && n_draw <= (int64_t(1) << 27), "rank_count: n must be in 1..2^27");
  TORCH_CHECK(n_sorted >= 1 && n_sorted <= n_draw, "rank_count: n_sorted must be in 1..n");
  TORCH_CHECK(n_boot >= 0 && b0 >= 0 && b0 + n_boot < (int64_t(1) << 31), "rank_count: bad replicate range");
  auto pp = pos.contiguous();
  at::Tensor ii;
  const int* ip = opt_idx(idx, n_boot, n_draw, "rank_count: idx must be (B, n)", ii);
  const int64_t stride = (n_sorted + 3) / 4 * 4;
  const at::DeviceGuard guard(pp.device());
  auto w = at::zeros({n_boot, stride}, pp.options());
  check(apneauq::launch_rank_count(pp.data_ptr<int>(), ip, (unsigned)seed, (int)n_draw, (int)n_sorted, (int)b0,
                                   (int)n_boot, (long long)stride, w.data_ptr<int>(), cur_stream()),
        "rank_count");
  return w.narrow(1, 0, n_sorted);
}

// rank_scan: (B, 6) int64 sums W, P, U2, groups, prauc_q, ap_q of weight rows over the sorted windows.  bounds
// (G + 1,) are the split points (tie-group starts, ops/rank.py:split_bounds); the result does not depend on G.
// Limits: n <= 2^27, G <= 64, weights non-negative with every row's total below 2^31 (checked on the totals).
at::Tensor rank_scan(const at::Tensor& w, const at::Tensor& packed, const at::Tensor& bounds) {
  TORCH_CHECK(w.is_cuda() && w.scalar_type() == at::kInt && w.dim() == 2, "rank_scan: w must be (B, n) int32 on the GPU");
  const int64_t n_boot = w.size(0), n = w.size(1);
  TORCH_CHECK(n >= 1 && n <= (int64_t(1) << 27), "rank_scan: n must be in 1..2^27");
  TORCH_CHECK(n_boot >= 0 && n_boot < (int64_t(1) << 31), "rank_scan: bad number of replicates");
  TORCH_CHECK(packed.is_cuda() && packed.scalar_type() == at::kByte && packed.dim() == 1 && packed.size(0) == n,
              "rank_scan: packed must be (n,) uint8 on the GPU");
  TORCH_CHECK(bounds.is_cuda() && bounds.scalar_type() == at::kInt && bounds.dim() == 1 && bounds.size(0) >= 2 &&
                  bounds.size(0) <= apneauq::rank_max_splits() + 1,
              "rank_scan: bounds must be (G + 1,) int32 on the GPU, G in 1..64");
  const int64_t splits = bounds.size(0) - 1;
  const at::DeviceGuard guard(w.device());
  // rows on 16-B boundaries for the vector loads: the view rank_count returns qualifies, anything else is copied
  at::Tensor ww = w;
  const int64_t stride = (n + 3) / 4 * 4;
  if (n_boot > 0 && (w.stride(1) != 1 || w.stride(0) % 4 != 0 || w.stride(0) < n ||
                     reinterpret_cast<uintptr_t>(w.data_ptr()) % 16 != 0)) {
    auto buf = at::zeros({n_boot, stride}, w.options());
    buf.narrow(1, 0, n).copy_(w);
    ww = buf.narrow(1, 0, n);
  }
  auto pk = packed.contiguous(), bb = bounds.contiguous();
  TORCH_CHECK(reinterpret_cast<uintptr_t>(pk.data_ptr()) % 4 == 0, "rank_scan: 4-B alignment of packed required");
  auto tot = at::empty({n_boot, splits, 3}, w.options().dtype(at::kLong));
  auto part = at::empty({n_boot, splits, 4}, w.options().dtype(at::kLong));
  auto out = at::empty({n_boot, 6}, w.options().dtype(at::kLong));
  if (n_boot == 0) return out;
  const long long row = n_boot > 1 ? ww.stride(0) : stride;
  check(apneauq::launch_rank_totals(ww.data_ptr<int>(), row, pk.data_ptr<uint8_t>(), bb.data_ptr<int>(), (int)n,
                                    (int)n_boot, (int)splits, reinterpret_cast<long long*>(tot.data_ptr<int64_t>()),
                                    cur_stream()),
        "rank_totals");
  auto t = tot.sum(1);  // (B, 3): positives, negatives, negative weights
  TORCH_CHECK(t.select(1, 2).max().item<int64_t>() == 0, "rank_scan: weights must be non-negative");
  auto total = t.select(1, 0) + t.select(1, 1);
  TORCH_CHECK(total.max().item<int64_t>() < (int64_t(1) << 31), "rank_scan: a replicate's total weight must stay below 2^31");
  check(apneauq::launch_rank_scan(ww.data_ptr<int>(), row, pk.data_ptr<uint8_t>(), bb.data_ptr<int>(),
                                  reinterpret_cast<const long long*>(tot.data_ptr<int64_t>()), (int)n, (int)n_boot,
                                  (int)splits, reinterpret_cast<long long*>(part.data_ptr<int64_t>()), cur_stream()),
        "rank_scan");
  out.select(1, 0).copy_(total);
  out.select(1, 1).copy_(t.select(1, 0));
  out.narrow(1, 2, 4).copy_(part.sum(1));
  return out;
}

// Split conformal prediction (uq_conformal.hip).  The role inputs of both ops: unit (n,) int32 and packed (n,) uint8
// over the sorted windows, and for cluster = "subsample" within (n,) int32 with ucount (P,) int32.  segments (0: the
// most the kernel holds) caps the segments a row is cut into; the results do not depend on it.
struct ConfInputs {
  at::Tensor unit, packed, within, ucount;
  const int* within_ptr = nullptr;
  const int* ucount_ptr = nullptr;
  int n = 0, n_units = 0, span = 1;
};

at::Tensor conf_aligned(const at::Tensor& t) {
  auto c = t.contiguous();
  return aligned(c, 16) ? c : c.clone();
}

ConfInputs conf_inputs(const char* op, const at::Tensor& unit, const at::Tensor& packed,
                       const c10::optional<at::Tensor>& within, const c10::optional<at::Tensor>& ucount, int64_t r0,
                       int64_t n_splits, int64_t cal_thr, int64_t segments) {
  ConfInputs in;
  TORCH_CHECK(unit.is_cuda() && unit.scalar_type() == at::kInt && unit.dim() == 1, op,
              ": unit must be (n,) int32 on the GPU");
  const int64_t n = unit.size(0);
  TORCH_CHECK(n >= 1 && n <= (int64_t(1) << 27), op, ": n must be in 1..2^27");
  TORCH_CHECK(packed.is_cuda() && packed.scalar_type() == at::kByte && packed.dim() == 1 && packed.size(0) == n, op,
              ": packed must be (n,) uint8 on the GPU");
  TORCH_CHECK(within.has_value() == ucount.has_value(), op, ": within and ucount go together");
  TORCH_CHECK(n_splits >= 0 && r0 >= 0 && r0 + n_splits < (int64_t(1) << 31), op, ": bad split range");
  TORCH_CHECK(cal_thr >= 0 && cal_thr <= (int64_t(1) << 32), op, ": cal_thr must be in 0..2^32");
  TORCH_CHECK(segments >= 0 && segments <= apneauq::conformal_max_segments(), op, ": segments must be in 0..",
              apneauq::conformal_max_segments());
  in.unit = conf_aligned(unit);
  in.packed = conf_aligned(packed);
  if (within.has_value()) {
    TORCH_CHECK(within->is_cuda() && within->scalar_type() == at::kInt && within->dim() == 1 && within->size(0) == n, op,
                ": within must be (n,) int32 on the GPU");
    TORCH_CHECK(ucount->is_cuda() && ucount->scalar_type() == at::kInt && ucount->dim() == 1 && ucount->size(0) >= 1 &&
                    ucount->size(0) < (int64_t(1) << 31),
                op, ": ucount must be (P,) int32 on the GPU");
    in.within = conf_aligned(*within);
    in.ucount = ucount->contiguous();
    in.within_ptr = in.within.data_ptr<int>();
    in.ucount_ptr = in.ucount.data_ptr<int>();
    in.n_units = (int)in.ucount.size(0);
  }
  const int64_t tiles = (n + apneauq::conformal_tile() - 1) / apneauq::conformal_tile();
  const int64_t cap = segments ? segments : apneauq::conformal_max_segments();
  in.n = (int)n;
  in.span = (int)((tiles + cap - 1) / cap);
  return in;
}

// conformal_select: totals (R, 4) int32 = cal0, cal1, test0, test1 and member (R, strata, A) int32, the sorted
// position of the calibration window of rank k(n_cal) per stratum and level (-1: k > n_cal).  Limits: A <= 32.
std::tuple<at::Tensor, at::Tensor> conformal_select(const at::Tensor& unit, const at::Tensor& packed,
                                                    const c10::optional<at::Tensor>& within,
                                                    const c10::optional<at::Tensor>& ucount, int64_t seed, int64_t r0,
                                                    int64_t n_splits, int64_t cal_thr, const at::Tensor& alpha_ppm,
                                                    int64_t strata, int64_t segments) {
  auto in = conf_inputs("conformal_select", unit, packed, within, ucount, r0, n_splits, cal_thr, segments);
  TORCH_CHECK(alpha_ppm.is_cuda() && alpha_ppm.scalar_type() == at::kInt && alpha_ppm.dim() == 1 &&
                  alpha_ppm.size(0) >= 1 && alpha_ppm.size(0) <= apneauq::conformal_max_alpha(),
              "conformal_select: alpha_ppm must be (A,) int32 on the GPU, A in 1..32");
  TORCH_CHECK(strata == 1 || strata == 2, "conformal_select: strata must be 1 or 2");
  auto aa = alpha_ppm.contiguous();
  const int64_t n_alpha = aa.size(0);
  const at::DeviceGuard guard(in.unit.device());
  auto totals = at::empty({n_splits, 4}, in.unit.options());
  auto member = at::empty({n_splits, strata, n_alpha}, in.unit.options());
  check(apneauq::launch_conformal_select(in.unit.data_ptr<int>(), in.packed.data_ptr<uint8_t>(), in.within_ptr,
                                         in.ucount_ptr, in.n_units, in.n, in.span, (unsigned)seed, (int)r0, (int)n_splits,
                                         (unsigned long long)cal_thr, aa.data_ptr<int>(), (int)n_alpha, (int)strata,
                                         totals.data_ptr<int>(), member.data_ptr<int>(), cur_stream()),
        "conformal_select");
  return std::make_tuple(totals, member);
}

// conformal_count: (R, Q, 2) int32, the test windows of class 0 / 1 among sorted positions [0, cuts[r, q]) (cuts are
// clamped to [0, n]).  Limits: Q <= 64.
at::Tensor conformal_count(const at::Tensor& unit, const at::Tensor& packed, const c10::optional<at::Tensor>& within,
                           const c10::optional<at::Tensor>& ucount, int64_t seed, int64_t r0, int64_t cal_thr,
                           const at::Tensor& cuts, int64_t segments) {
  TORCH_CHECK(cuts.is_cuda() && cuts.scalar_type() == at::kInt && cuts.dim() == 2 && cuts.size(1) >= 1 &&
                  cuts.size(1) <= apneauq::conformal_max_cuts(),
              "conformal_count: cuts must be (R, Q) int32 on the GPU, Q in 1..64");
  const int64_t n_splits = cuts.size(0), n_cuts = cuts.size(1);
  auto in = conf_inputs("conformal_count", unit, packed, within, ucount, r0, n_splits, cal_thr, segments);
  auto cc = cuts.contiguous();
  const at::DeviceGuard guard(in.unit.device());
  auto out = at::empty({n_splits, n_cuts, 2}, in.unit.options());
  check(apneauq::launch_conformal_count(in.unit.data_ptr<int>(), in.packed.data_ptr<uint8_t>(), in.within_ptr,
                                        in.ucount_ptr, in.n_units, in.n, in.span, (unsigned)seed, (int)r0, (int)n_splits,
                                        (unsigned long long)cal_thr, cc.data_ptr<int>(), (int)n_cuts, out.data_ptr<int>(),
                                        cur_stream()),
        "conformal_count");
  return out;
}

// Last-layer Laplace (uq_laplace.hip).  laplace_gram: flat fp64 [(D+1)^2 H | (D+1) g | loglik | n_valid] of phi (n, D)
// fp32, theta (D+1) fp64 and y (n) uint8.  range_len (windows per range, ops/laplace.py:range_len) fixes the order of
// the fp64 additions; grid (0: one workgroup per range) does not change the result.  Limits: D + 1 <= 128 and the
// range partials stay within 64 MB.
at::Tensor laplace_gram(const at::Tensor& phi, const at::Tensor& theta, const at::Tensor& y, int64_t range_len,
                        int64_t grid) {
  TORCH_CHECK(phi.is_cuda() && phi.scalar_type() == at::kFloat && phi.dim() == 2,
              "laplace_gram: phi must be (n, D) fp32 on the GPU");
  const int64_t n = phi.size(0), D = phi.size(1);
  TORCH_CHECK(D >= 1 && D + 1 <= apneauq::laplace_max_dp(), "laplace_gram: D + 1 must be in 2..128");
  TORCH_CHECK(theta.is_cuda() && theta.scalar_type() == at::kDouble && theta.dim() == 1 && theta.size(0) == D + 1,
              "laplace_gram: theta must be (D + 1,) fp64 on the GPU");
  TORCH_CHECK(y.is_cuda() && y.scalar_type() == at::kByte && y.dim() == 1 && y.size(0) == n,
              "laplace_gram: y must be (n,) uint8 on the GPU");
  TORCH_CHECK(range_len >= 1 && grid >= 0 && grid < (int64_t(1) << 20), "laplace_gram: bad range_len / grid");
  const int64_t n_ranges = (n + range_len - 1) / range_len;
  const int64_t pd = apneauq::laplace_part_doubles((int)D);
  TORCH_CHECK(n_ranges * pd * 8 <= (int64_t(64) << 20), "laplace_gram: the range partials must stay within 64 MB");
  auto pp = phi.contiguous(), tt = theta.contiguous(), yy = y.contiguous();
  const at::DeviceGuard guard(pp.device());
  auto part = at::empty({std::max<int64_t>(n_ranges, 1) * pd}, tt.options());
  auto out = at::empty({(D + 1) * (D + 1) + (D + 1) + 2}, tt.options());
  check(apneauq::launch_laplace_gram(pp.data_ptr<float>(), tt.data_ptr<double>(), yy.data_ptr<uint8_t>(), (long long)n,
                                     (int)D, (long long)range_len, (int)grid, part.data_ptr<double>(),
                                     out.data_ptr<double>(), cur_stream()),
        "laplace_gram");
  return out;
}

// laplace_predict: mx (D+1, 1 + T + D+1) fp64 = [theta | theta_1 .. theta_T | L] -> preds (T, n) fp32 and the moments
// (3, n) fp64: mean logit, logit variance, probit probability.  NaN for a window with a non-finite feature.
std::tuple<at::Tensor, at::Tensor> laplace_predict(const at::Tensor& phi, const at::Tensor& mx, int64_t T) {
  TORCH_CHECK(phi.is_cuda() && phi.scalar_type() == at::kFloat && phi.dim() == 2,
              "laplace_predict: phi must be (n, D) fp32 on the GPU");
  const int64_t n = phi.size(0), D = phi.size(1);
  TORCH_CHECK(D >= 1 && D + 1 <= apneauq::laplace_max_dp(), "laplace_predict: D + 1 must be in 2..128");
  TORCH_CHECK(T >= 0 && T < (int64_t(1) << 24), "laplace_predict: T must be in 0..2^24");
  TORCH_CHECK(mx.is_cuda() && mx.scalar_type() == at::kDouble && mx.dim() == 2 && mx.size(0) == D + 1 &&
                  mx.size(1) == T + D + 2,
              "laplace_predict: mx must be (D + 1, T + D + 2) fp64 on the GPU");
  auto pp = phi.contiguous(), mm = mx.contiguous();
  const at::DeviceGuard guard(pp.device());
  auto preds = at::empty({T, n}, pp.options());
  auto mom = at::empty({3, n}, mm.options());
  if (n == 0) return std::make_tuple(preds, mom);
  double* mp = mom.data_ptr<double>();
  check(apneauq::launch_laplace_predict(pp.data_ptr<float>(), mm.data_ptr<double>(), (long long)n, (int)D, (int)T,
                                        preds.data_ptr<float>(), mp, mp + n, mp + 2 * n, cur_stream()),
        "laplace_predict");
  return std::make_tuple(preds, mom);
}

// Pass / member-count convergence (uq_converge.hip): (R, K, 11) int64 sums over the windows of the metrics of
// the first counts[k] passes of orders[r].  Limits: T <= 128 (the tile's planes fit LDS), K <= 32, R <= 4096 and
// n <= 2^22 per launch (a fixed-point term is at most 2^40, so every sum stays below 2^62; the front end splits
// larger sets and adds).  The kernel clamps the pass indices to [0, T); ops/converge.py checks orders and counts.
at::Tensor converge(const at::Tensor& probs, const at::Tensor& y, const at::Tensor& orders, const at::Tensor& counts,
                    int64_t rep_groups) {
  TORCH_CHECK(probs.is_cuda() && probs.scalar_type() == at::kFloat && probs.dim() == 2,
              "converge: probs must be a (T, n) float32 GPU tensor");
  const int64_t t_count = probs.size(0), n = probs.size(1);
  TORCH_CHECK(t_count >= 1 && t_count <= 128, "converge: T must be in 1..128");
  TORCH_CHECK(n >= 1 && n <= (int64_t(1) << 22), "converge: n must be in 1..2^22");
  TORCH_CHECK(orders.is_cuda() && orders.scalar_type() == at::kInt && orders.dim() == 2 && orders.size(1) == t_count,
              "converge: orders must be (R, T) int32 on the GPU");
  const int64_t n_rep = orders.size(0);
  TORCH_CHECK(n_rep >= 1 && n_rep <= 4096, "converge: R must be in 1..4096");
  TORCH_CHECK(counts.is_cuda() && counts.scalar_type() == at::kInt && counts.dim() == 1,
              "converge: counts must be (K,) int32 on the GPU");
  const int64_t n_cnt = counts.size(0);
  TORCH_CHECK(n_cnt >= 1 && n_cnt <= 32, "converge: K must be in 1..32");
  TORCH_CHECK(rep_groups >= 1 && rep_groups <= 1024, "converge: rep_groups must be in 1..1024");
  auto pp = probs.contiguous(), oo = orders.contiguous(), cc = counts.contiguous();
  auto yy = y.to(at::kInt).contiguous();
  TORCH_CHECK(yy.is_cuda() && yy.dim() == 1 && yy.size(0) == n, "converge: y must be (n,) on the GPU");
  const at::DeviceGuard guard(pp.device());
  auto out = at::zeros({n_rep, n_cnt, 11}, pp.options().dtype(at::kLong));
  check(apneauq::launch_converge(pp.data_ptr<float>(), yy.data_ptr<int>(), oo.data_ptr<int>(), cc.data_ptr<int>(),
                                 (int)t_count, (int)n, (int)n_rep, (int)n_cnt, (int)rep_groups,
                                 reinterpret_cast<long long*>(out.data_ptr<int64_t>()), cur_stream()),
        "converge");
  return out;
}

// Signal corruptions of the shift sweep (uq_shift.hip): (K, n, L, C) fp32, condition k of the windows x (n, L, C)
// fp32 or fp64.  kinds (K,) int, params (K,) float64 and chmask (K,) int are host tensors (they travel by value
// with the launch; ops/shift.py builds them).  Limits: C <= 4, L <= 256, K <= 64, n <= 2^27 and
// window_offset + n <= 2^32.
at::Tensor shift_corrupt(const at::Tensor& x, const at::Tensor& kinds, const at::Tensor& params,
                         const at::Tensor& chmask, int64_t seed, int64_t window_offset, bool restandardize) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 3 && (x.scalar_type() == at::kFloat || x.scalar_type() == at::kDouble),
              "shift_corrupt: x must be (n, L, C) float32 or float64 on the GPU");
  const int64_t n = x.size(0), L = x.size(1), C = x.size(2), K = kinds.numel();
  TORCH_CHECK(L >= 1 && L <= apneauq::kShiftMaxL, "shift_corrupt: L must be in 1..", apneauq::kShiftMaxL);
  TORCH_CHECK(C >= 1 && C <= apneauq::kShiftMaxC, "shift_corrupt: C must be in 1..", apneauq::kShiftMaxC);
  TORCH_CHECK(K >= 1 && K <= apneauq::kShiftMaxK, "shift_corrupt: K must be in 1..", apneauq::kShiftMaxK);
  TORCH_CHECK(n <= (int64_t(1) << 27), "shift_corrupt: at most 2^27 windows");
  TORCH_CHECK(window_offset >= 0 && window_offset + n <= (int64_t(1) << 32),
              "shift_corrupt: window_offset + n must stay within 2^32");
  TORCH_CHECK(kinds.dim() == 1 && params.dim() == 1 && chmask.dim() == 1 && params.numel() == K && chmask.numel() == K,
              "shift_corrupt: kinds, params and chmask must be (K,)");
  auto kk = kinds.to(at::kCPU, at::kLong).contiguous();
  auto pp = params.to(at::kCPU, at::kDouble).contiguous();
  auto mm = chmask.to(at::kCPU, at::kLong).contiguous();
  apneauq::ShiftConds cd = {};
  for (int64_t k = 0; k < K; ++k) {
    const int64_t kind = kk.data_ptr<int64_t>()[k], mask = mm.data_ptr<int64_t>()[k];
    const double p = pp.data_ptr<double>()[k];
    TORCH_CHECK(kind >= 0 && kind < apneauq::kShiftKinds, "shift_corrupt: kind ", kind, " is not in 0..",
                apneauq::kShiftKinds - 1);
    TORCH_CHECK(mask >= 0 && mask < (int64_t(1) << C), "shift_corrupt: chmask must hold bits of channels 0..C-1");
    TORCH_CHECK(std::isfinite(p) && p >= 0.0, "shift_corrupt: params must be finite and non-negative");
    cd.kind[k] = (unsigned char)kind;
    cd.mask[k] = (unsigned char)mask;
    cd.p[k] = p;
  }
  auto xx = x.contiguous();
  if (!aligned(xx, 32)) xx = xx.clone();
  TORCH_CHECK(aligned(xx, 32), "shift_corrupt: 32-B alignment required");
  const at::DeviceGuard guard(xx.device());
  auto out = at::empty({K, n, L, C}, xx.options().dtype(at::kFloat));
  if (n == 0) return out;
  check(apneauq::launch_shift_corrupt(xx.data_ptr(), xx.scalar_type() == at::kDouble, (long long)n, (int)L, (int)C, cd,
                                      (int)K, (unsigned long long)seed, (unsigned long long)window_offset, restandardize,
                                      out.data_ptr<float>(), cur_stream()),
        "shift_corrupt");
  return out;
}

// Ensemble composition (uq_members.hip).  Both ops take exactly what the kernels read: contiguous GPU tensors,
// probs (T, n) float32 and y (n,) int32; nothing is converted here.  member_pairs: the symmetric (T, T, 3) int64
// table (both correct and y = 0, both correct and y = 1, the residual Gram quantised at 2^40 per window and
// pair) and the header (n_valid, n_y1).  Limits: T <= 128, n <= 2^22 per launch (a term is at most 2^40, so
// every sum stays below 2^62; the front end splits larger sets and adds).  grid and slices (0: auto) only change
// the speed.
std::tuple<at::Tensor, at::Tensor> member_pairs(const at::Tensor& probs, const at::Tensor& y, int64_t grid,
                                                int64_t slices) {
  TORCH_CHECK(probs.is_cuda() && probs.scalar_type() == at::kFloat && probs.dim() == 2 && probs.is_contiguous(),
              "member_pairs: probs must be a contiguous (T, n) float32 GPU tensor");
  const int64_t t_count = probs.size(0), n = probs.size(1);
  TORCH_CHECK(t_count >= 1 && t_count <= apneauq::member_max_t(), "member_pairs: T must be in 1..",
              apneauq::member_max_t());
  TORCH_CHECK(n >= 1 && n <= (int64_t(1) << 22), "member_pairs: n must be in 1..2^22");
  TORCH_CHECK(y.is_cuda() && y.scalar_type() == at::kInt && y.dim() == 1 && y.size(0) == n && y.is_contiguous() &&
                  y.device() == probs.device(),
              "member_pairs: y must be a contiguous (n,) int32 tensor on the GPU of probs");
  TORCH_CHECK(grid >= 0 && grid <= 65535, "member_pairs: grid must be in 0..65535");
  TORCH_CHECK(slices >= 0 && slices <= 64 && (slices & (slices - 1)) == 0,
              "member_pairs: slices must be 0 or a power of two up to 64");
  const at::DeviceGuard guard(probs.device());
  auto up = at::zeros({t_count, t_count, 3}, probs.options().dtype(at::kLong));
  auto head = at::zeros({2}, probs.options().dtype(at::kLong));
  check(apneauq::launch_member_pairs(probs.data_ptr<float>(), y.data_ptr<int>(), (int)t_count, (int)n, (int)grid,
                                     (int)slices, reinterpret_cast<long long*>(up.data_ptr<int64_t>()),
                                     reinterpret_cast<long long*>(head.data_ptr<int64_t>()), cur_stream()),
        "member_pairs");
  // the kernel writes a <= b and the strict lower triangle stays zero, so the mirror is one add
  auto planes = up.permute({2, 0, 1});   // (3, T, T)
  auto full = planes + at::triu(planes, 1).transpose(1, 2);
  return std::make_tuple(full.permute({1, 2, 0}).contiguous(), head);
}

// member_mix: (F, Q, 7) int64 sums per fold and per row of integer member counts: n_valid, n_y1, nll_q (2^36),
// brier_q (2^40), correct, true_pos, pred_pos of the mixture sum_t c_t p_t / k.  fold (n,) uint8 is optional
// (absent: one fold); a window with a code >= F contributes to nothing.  Limits: T <= 128, Q <= 64, F <= 16,
// n <= 2^21 per launch (an nll term stays below 2^41), counts (a host tensor) in 0..255 with a positive row sum.
at::Tensor member_mix(const at::Tensor& probs, const at::Tensor& y, const c10::optional<at::Tensor>& fold,
                      const at::Tensor& counts, int64_t n_folds, int64_t grid) {
  TORCH_CHECK(probs.is_cuda() && probs.scalar_type() == at::kFloat && probs.dim() == 2 && probs.is_contiguous(),
              "member_mix: probs must be a contiguous (T, n) float32 GPU tensor");
  const int64_t t_count = probs.size(0), n = probs.size(1);
  TORCH_CHECK(t_count >= 1 && t_count <= apneauq::member_max_t(), "member_mix: T must be in 1..",
              apneauq::member_max_t());
  TORCH_CHECK(n >= 1 && n <= (int64_t(1) << 21), "member_mix: n must be in 1..2^21");
  TORCH_CHECK(y.is_cuda() && y.scalar_type() == at::kInt && y.dim() == 1 && y.size(0) == n && y.is_contiguous() &&
                  y.device() == probs.device(),
              "member_mix: y must be a contiguous (n,) int32 tensor on the GPU of probs");
  TORCH_CHECK(n_folds >= 1 && n_folds <= apneauq::member_max_f(), "member_mix: F must be in 1..",
              apneauq::member_max_f());
  const unsigned char* fp = nullptr;
  if (fold.has_value()) {
    TORCH_CHECK(fold->is_cuda() && fold->scalar_type() == at::kByte && fold->dim() == 1 && fold->size(0) == n &&
                    fold->is_contiguous() && fold->device() == probs.device(),
                "member_mix: fold must be a contiguous (n,) uint8 tensor on the GPU of probs");
    fp = fold->data_ptr<uint8_t>();
  }
  TORCH_CHECK(counts.is_cpu() && counts.scalar_type() == at::kInt && counts.dim() == 2 && counts.size(1) == t_count &&
                  counts.is_contiguous(),
              "member_mix: counts must be a contiguous (Q, T) int32 host tensor");
  const int64_t n_rows = counts.size(0);
  TORCH_CHECK(n_rows >= 1 && n_rows <= apneauq::member_max_q(), "member_mix: Q must be in 1..",
              apneauq::member_max_q());
  TORCH_CHECK(grid >= 0 && grid <= 65535, "member_mix: grid must be in 0..65535");
  // the counts are a host tensor (as the conditions of shift_corrupt are): their values are checked here without a
  // device synchronise, and they are uploaded with the launch
  const int* cp = counts.data_ptr<int>();
  for (int64_t q = 0; q < n_rows; ++q) {
    int64_t k = 0;
    for (int64_t t = 0; t < t_count; ++t) {
      const int c = cp[q * t_count + t];
      TORCH_CHECK(c >= 0 && c <= 255, "member_mix: counts must lie in 0..255");
      k += c;
    }
    TORCH_CHECK(k >= 1, "member_mix: every row of counts needs a positive sum");
  }
  const at::DeviceGuard guard(probs.device());
  auto dev_counts = counts.to(probs.device(), /*non_blocking=*/true);
  auto out = at::zeros({n_folds, n_rows, 7}, probs.options().dtype(at::kLong));
  check(apneauq::launch_member_mix(probs.data_ptr<float>(), y.data_ptr<int>(), fp, dev_counts.data_ptr<int>(), (int)t_count,
                                   (int)n, (int)n_rows, (int)n_folds, (int)grid,
                                   reinterpret_cast<long long*>(out.data_ptr<int64_t>()), cur_stream()),
        "member_mix");
  return out;
}

}  // namespace

TORCH_LIBRARY_FRAGMENT(apneauq, m) {
  m.def("uq_reduce(Tensor probs) -> Tensor");
  m.def("bootstrap(Tensor metrics, Tensor y, Tensor? idx, int seed, int n_boot) -> Tensor");
  m.def("bootstrap_partial(Tensor metrics, Tensor y, Tensor? idx, int seed, int n_boot, int n_global, int lo) -> Tensor");
  m.def("calib_prep(Tensor p, Tensor score, Tensor y, Tensor thr, int n_bins) -> Tensor");
  m.def("calib_bootstrap(Tensor rec, Tensor? idx, int seed, int n_boot, int n_global, int lo, int n_bins, int n_thr, int slices) -> Tensor");
  m.def("patient_reduce(Tensor probs, Tensor m, Tensor y, Tensor code, int n_pat) -> (Tensor, Tensor)");
  m.def("patient_bootstrap(Tensor prec, Tensor? idx, int seed, int n_boot) -> Tensor");
  m.def("rank_count(Tensor pos, Tensor? idx, int seed, int b0, int n_boot, int n_sorted) -> Tensor");
  m.def("rank_scan(Tensor w, Tensor packed, Tensor bounds) -> Tensor");
  m.def("conformal_select(Tensor unit, Tensor packed, Tensor? within, Tensor? ucount, int seed, int r0, int n_splits, int cal_thr, Tensor alpha_ppm, int strata, int segments) -> (Tensor, Tensor)");
  m.def("conformal_count(Tensor unit, Tensor packed, Tensor? within, Tensor? ucount, int seed, int r0, int cal_thr, Tensor cuts, int segments) -> Tensor");
  m.def("laplace_gram(Tensor phi, Tensor theta, Tensor y, int range_len, int grid) -> Tensor");
  m.def("laplace_predict(Tensor phi, Tensor mx, int T) -> (Tensor, Tensor)");
  m.def("converge(Tensor probs, Tensor y, Tensor orders, Tensor counts, int rep_groups) -> Tensor");
  m.def("shift_corrupt(Tensor x, Tensor kinds, Tensor params, Tensor chmask, int seed, int window_offset, bool restandardize) -> Tensor");
  m.def("member_pairs(Tensor probs, Tensor y, int grid, int slices) -> (Tensor, Tensor)");
  m.def("member_mix(Tensor probs, Tensor y, Tensor? fold, Tensor counts, int n_folds, int grid) -> Tensor");
}

TORCH_LIBRARY_IMPL(apneauq, CUDA, m) {
  m.impl("uq_reduce", &uq_reduce);
  m.impl("bootstrap", &bootstrap);
  m.impl("bootstrap_partial", &bootstrap_partial);
  m.impl("calib_prep", &calib_prep);
  m.impl("calib_bootstrap", &calib_bootstrap);
  m.impl("patient_reduce", &patient_reduce);
  m.impl("patient_bootstrap", &patient_bootstrap);
  m.impl("rank_count", &rank_count);
  m.impl("rank_scan", &rank_scan);
  m.impl("conformal_select", &conformal_select);
  m.impl("conformal_count", &conformal_count);
  m.impl("laplace_gram", &laplace_gram);
  m.impl("laplace_predict", &laplace_predict);
  m.impl("converge", &converge);
  m.impl("shift_corrupt", &shift_corrupt);
  m.impl("member_pairs", &member_pairs);
  m.impl("member_mix", &member_mix);
}
