// torch.library registration of the generic-spec kernels: inference (generic_conv.hip), bf16 training
// (generic_train.hip, generic_wgrad.hip), fp32 (gf32_conv.hip) and fp16x3 (gx3_conv.hip); torch.ops.apneauq.
#include "bind_util.h"
#include "generic_api.h"

#include <vector>

namespace {
using namespace apneauq::bind;

// Generic-spec conv block (csrc/generic_conv.hip): x (N, L, Cin) bf16 -> (N, L or L/2, Cout) bf16.
at::Tensor generic_conv(const at::Tensor& x, const at::Tensor& wfrag, const at::Tensor& epi, int64_t cout,
                        int64_t ksize, bool pool, bool dropout, int64_t thr, int64_t layer, int64_t n_win,
                        int64_t pass_offset, int64_t window_offset, int64_t seed) {
  TORCH_CHECK(x.is_cuda() && wfrag.is_cuda() && epi.is_cuda(), "generic_conv: tensors must be on the GPU");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 && x.is_contiguous() && x.dim() == 3, "generic_conv: x must be contiguous bf16 (N, L, C)");
  TORCH_CHECK(wfrag.scalar_type() == at::kBFloat16 && wfrag.is_contiguous() && wfrag.dim() == 4 && wfrag.size(2) == 64 &&
              wfrag.size(3) == 8, "generic_conv: wfrag must be (nstep, Cout_pad/16, 64, 8) bf16");
  const int64_t n = x.size(0), L = x.size(1), cin = x.size(2), cout_pad = wfrag.size(1) * 16;
  TORCH_CHECK(wfrag.size(0) == (ksize * cin + 31) / 32, "generic_conv: wfrag k-steps do not match k*Cin");
  TORCH_CHECK(cout > 0 && cout % 4 == 0 && cout <= cout_pad && cout_pad - cout < 16, "generic_conv: Cout must be a multiple of 4");
  TORCH_CHECK(cout_pad <= 1024 && L < (1 << 22), "generic_conv: dropout hash needs C <= 1024, L < 2^22");
  TORCH_CHECK(epi.scalar_type() == at::kFloat && epi.is_contiguous() && epi.numel() == 8 * cout_pad, "generic_conv: epi must be (8, Cout_pad) fp32");
  TORCH_CHECK(ksize % 2 == 1, "generic_conv: odd kernel sizes only ('same' padding)");
  TORCH_CHECK(n_win >= 1 && n % n_win == 0, "generic_conv: N must be n_pass * n_win");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0, "generic_conv: 16-B alignment required");
  TORCH_CHECK(n * L < (int64_t(1) << 31), "generic_conv: too many rows");
  const at::DeviceGuard guard(x.device());
  const int64_t lout = pool ? L / 2 : L;
  auto y = at::empty({n, lout, cout}, x.options());
  check(apneauq::launch_generic_conv(x.data_ptr(), wfrag.data_ptr(), epi.data_ptr<float>(), y.data_ptr(), (int)n, (int)L,
                                     (int)cin, (int)cout, (int)cout_pad, (int)ksize, pool ? 1 : 0, dropout ? 1 : 0,
                                     (unsigned)thr, (int)layer, (int)n_win, (unsigned)pass_offset, (unsigned)window_offset,
                                     (unsigned long long)seed, cur_stream(), 0, (int)L, 0, nullptr, n * L, 0),
        "generic_conv");
  return y;
}

// ---- generic-spec training (csrc/generic_train.hip); every buffer is preallocated by ops/generic_train.py ----
// activation buffers of the generic training path: bf16, or fp32 (precision="fp32"); one launch's
// activation tensors must share the dtype (need_same)
constexpr int64_t kGtSlots = 16;
inline void need_same(const at::Tensor& a, const at::Tensor& b, const char* what) {
  TORCH_CHECK(a.scalar_type() == b.scalar_type(), what, ": activation buffers must share one dtype");
}

// mode 1: y = relu(conv(x) + bias) (N, L, Cout) + BN moment slots; mode 2: y = conv(x) (dgrad).
// x row (n, t) lives at n * in_rs + in_off + t (zero-padded layouts); the conv reads rows
// in_off - pad .. in_off + L - 1 + pad of each sample, all of which must exist.
void gt_conv(const at::Tensor& x, const at::Tensor& wfrag, const c10::optional<at::Tensor>& bias, at::Tensor& y,
             const c10::optional<at::Tensor>& stats, int64_t n, int64_t L, int64_t cin, int64_t cout, int64_t ksize,
             int64_t mode, int64_t in_rs, int64_t in_off, bool det) {
  TORCH_CHECK(mode == 1 || mode == 2, "gt_conv: mode must be 1 (train) or 2 (linear)");
  TORCH_CHECK(ksize % 2 == 1 && cout % 4 == 0 && cout <= 1024 && n >= 0 && L >= 1, "gt_conv: bad shape");
  TORCH_CHECK(wfrag.is_cuda() && wfrag.scalar_type() == at::kBFloat16 && wfrag.is_contiguous() && wfrag.dim() == 4 &&
              wfrag.size(0) == (ksize * cin + 31) / 32 && wfrag.size(2) == 64 && wfrag.size(3) == 8 &&
              wfrag.size(1) * 16 >= cout && wfrag.size(1) * 16 - cout < 16, "gt_conv: wfrag shape mismatch");
  const int64_t pad = (ksize - 1) / 2;
  TORCH_CHECK(in_rs >= L && in_off >= 0, "gt_conv: bad input row layout");
  if (n > 0) need_rows(x, (n - 1) * in_rs + in_off + L, cin, "gt_conv x");
  (void)pad;  // rows outside [0, L) of a sample are masked in the kernel, never read
  need_rows(y, n * L, cout, "gt_conv y");
  const float* bp = nullptr;
  float* sp = nullptr;
  if (mode == 1) {
    TORCH_CHECK(bias.has_value() && stats.has_value(), "gt_conv: mode 1 needs bias and stats");
    need_f32(*bias, cout, "gt_conv bias");
    need_f32(*stats, kGtSlots * 2 * cout, "gt_conv stats");
    bp = bias->data_ptr<float>();
    sp = stats->data_ptr<float>();
  }
  // deterministic mode: one plain-store slot per (workgroup, wave row); the launcher checks the count
  const int det_slots = (mode == 1 && det) ? (int)(stats->numel() / (2 * cout)) : 0;
  TORCH_CHECK(n * L < (int64_t(1) << 31), "gt_conv: too many rows");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 && y.scalar_type() == at::kBFloat16, "gt_conv: bf16 (fp32: gf_conv)");
  const at::DeviceGuard guard(y.device());
  check(apneauq::launch_generic_conv(x.data_ptr(), wfrag.data_ptr(), bp, y.data_ptr(), (int)n, (int)L, (int)cin,
                                     (int)cout, (int)(wfrag.size(1) * 16), (int)ksize, 0, 0, 0u, 0, 1, 0u, 0u, 0ull,
                                     cur_stream(), (int)mode, (int)in_rs, (int)in_off, sp, x.numel() / cin, det_slots),
        "gt_conv");
}

void gt_bn_finalize(const at::Tensor& st, int64_t C, double inv_count, const at::Tensor& gamma, const at::Tensor& beta,
                    double eps, double momentum, at::Tensor& mmean, at::Tensor& mvar, bool update, at::Tensor& bn) {
  need_f32(st, kGtSlots * 2 * C, "gt_bn_finalize st");
  TORCH_CHECK(gamma.is_cuda() && gamma.numel() == C && beta.numel() == C && mmean.numel() == C && mvar.numel() == C,
              "gt_bn_finalize: per-channel tensors must have C elements");
  need_f32(bn, 4 * C, "gt_bn_finalize bn");
  const at::DeviceGuard guard(bn.device());
  // every slot of the table is summed (in a fixed order): kGtSlots atomic copies or the deterministic slots
  // (large tables in 64-slot ranges whose sums overwrite the ranges' first slots: st is consumed)
  check(apneauq::launch_gt_bn_finalize(st.data_ptr<float>(), (int)(st.numel() / (2 * C)), (int)C, inv_count,
                                       gamma.data_ptr<float>(),
                                       beta.data_ptr<float>(), (float)eps, (float)momentum, mmean.data_ptr<float>(),
                                       mvar.data_ptr<float>(), update ? 1 : 0, bn.data_ptr<float>(), cur_stream()),
        "gt_bn_finalize");
}

void gt_apply(const at::Tensor& z, const at::Tensor& bn, at::Tensor& out, int64_t n, int64_t L, int64_t C, bool pool,
              int64_t out_rs, int64_t out_off, bool dropout, int64_t thr, double inv_keep, int64_t skey,
              int64_t window_offset, const c10::optional<at::Tensor>& skey_dev) {
  TORCH_CHECK(C % 4 == 0 && C <= 1024 && L >= 1, "gt_apply: bad shape");
  const unsigned* kd = skey_dev_ptr(skey_dev);
  const int64_t lout = pool ? L / 2 : L;
  need_rows(z, n * L, C, "gt_apply z");
  need_f32(bn, 4 * C, "gt_apply bn");
  TORCH_CHECK(out_rs >= lout && out_off >= 0, "gt_apply: bad output row layout");
  if (n > 0) need_rows(out, (n - 1) * out_rs + out_off + lout, C, "gt_apply out");
  need_same(z, out, "gt_apply");
  const at::DeviceGuard guard(out.device());
  check(apneauq::launch_gt_apply(z.data_ptr(), bn.data_ptr<float>(), out.data_ptr(), (int)n, (int)L, (int)C, pool ? 1 : 0,
                                 (int)out_rs, (int)out_off, dropout ? 1 : 0, (unsigned)thr, (float)inv_keep,
                                 (unsigned)skey, (unsigned)window_offset, cur_stream(), kd, z.scalar_type() == at::kFloat),
        "gt_apply");
}

// dz_mode 0: BN-backward sums into bst; 1: dz (zero-padded rows) + bias gradient.  The upstream
// gradient is dh (N, L/2 or L, C) bf16, or (head mode, dh undefined) dlog[n] * w[c] * invL.
void gt_bwd(bool dz_mode, const at::Tensor& z, const at::Tensor& bn, const c10::optional<at::Tensor>& dh,
            const c10::optional<at::Tensor>& dlog, const c10::optional<at::Tensor>& w, double invL, int64_t n, int64_t L,
            int64_t C, bool pool, bool dropout, int64_t thr, double inv_keep, int64_t skey, int64_t window_offset,
            const c10::optional<at::Tensor>& bst, const c10::optional<at::Tensor>& coef,
            const c10::optional<at::Tensor>& gamma, const c10::optional<at::Tensor>& dz, int64_t dz_rs, int64_t dz_off,
            const c10::optional<at::Tensor>& gbias, const c10::optional<at::Tensor>& skey_dev, bool det) {
  TORCH_CHECK(C % 4 == 0 && C <= 1024 && L >= 1, "gt_bwd: bad shape");
  const int64_t lout = pool ? L / 2 : L;
  need_rows(z, n * L, C, "gt_bwd z");
  need_f32(bn, 4 * C, "gt_bwd bn");
  const void* dhp = nullptr;
  const float *dlp = nullptr, *wp = nullptr;
  if (dh.has_value()) {
    need_rows(*dh, n * lout, C, "gt_bwd dh");
    need_same(z, *dh, "gt_bwd");
    dhp = dh->data_ptr();
  } else {
    TORCH_CHECK(dlog.has_value() && w.has_value(), "gt_bwd: need dh or (dlog, w)");
    need_f32(*dlog, n, "gt_bwd dlog");
    need_f32(*w, C, "gt_bwd w");
    dlp = dlog->data_ptr<float>();
    wp = w->data_ptr<float>();
  }
  float* bp = nullptr;
  const float *cp = nullptr, *gp = nullptr;
  void* dzp = nullptr;
  float* gbp = nullptr;
  if (!dz_mode) {
    TORCH_CHECK(bst.has_value(), "gt_bwd: stats mode needs bst");
    need_f32(*bst, kGtSlots * 2 * C, "gt_bwd bst");
    bp = bst->data_ptr<float>();
  } else {
    TORCH_CHECK(coef.has_value() && gamma.has_value() && dz.has_value() && gbias.has_value(), "gt_bwd: dz mode args");
    need_f32(*coef, 2 * C, "gt_bwd coef");
    TORCH_CHECK(gamma->is_cuda() && gamma->numel() == C, "gt_bwd gamma");
    TORCH_CHECK(dz_rs >= L && dz_off >= 0, "gt_bwd: bad dz row layout");
    if (n > 0) need_rows(*dz, (n - 1) * dz_rs + dz_off + L, C, "gt_bwd dz");
    need_same(z, *dz, "gt_bwd");
    need_f32(*gbias, kGtSlots * C, "gt_bwd gbias slots");
    cp = coef->data_ptr<float>();
    gp = gamma->data_ptr<float>();
    dzp = dz->data_ptr();
    gbp = gbias->data_ptr<float>();
  }
  // deterministic mode: workgroup b writes slot b (the grid is capped to the slot count)
  const int det_slots = !det ? 0 : (int)(dz_mode ? gbias->numel() / C : bst->numel() / (2 * C));
  const at::DeviceGuard guard(z.device());
  check(apneauq::launch_gt_bwd(dz_mode ? 1 : 0, z.data_ptr(), bn.data_ptr<float>(), dhp, dlp, wp, (float)invL, (int)n,
                               (int)L, (int)C, pool ? 1 : 0, dropout ? 1 : 0, (unsigned)thr, (float)inv_keep,
                               (unsigned)skey, (unsigned)window_offset, bp, cp, gp, dzp, (int)dz_rs, (int)dz_off, gbp,
                               cur_stream(), skey_dev_ptr(skey_dev), det_slots, z.scalar_type() == at::kFloat),
        "gt_bwd");
}

// BN-backward finalize of one block (C > 0; C == 0: none) plus, as extra workgroups of the same launch,
// the bias gradient gbias (BC) = column sums of a (slots, BC) table (the block above's, done by now).
void gt_bwd_finalize(const at::Tensor& bst, int64_t C, double inv_count, at::Tensor& coef, at::Tensor& ggamma,
                     at::Tensor& gbeta, const c10::optional<at::Tensor>& dbs, const c10::optional<at::Tensor>& gbias) {
  TORCH_CHECK(C >= 0, "gt_bwd_finalize: C >= 0");
  if (C > 0) {
    need_f32(bst, kGtSlots * 2 * C, "gt_bwd_finalize bst");
    need_f32(coef, 2 * C, "gt_bwd_finalize coef");
    TORCH_CHECK(ggamma.is_cuda() && ggamma.scalar_type() == at::kFloat && ggamma.numel() == C && gbeta.numel() == C,
                "gt_bwd_finalize: grads must have C elements");
  }
  TORCH_CHECK(dbs.has_value() == gbias.has_value(), "gt_bwd_finalize: dbs and gbias go together");
  int bslots = 0, BC = 0;
  float* gbp = nullptr;
  const float* dbp = nullptr;
  if (gbias.has_value()) {
    const at::Tensor& d = *dbs;
    const at::Tensor& gbt = *gbias;
    TORCH_CHECK(d.is_cuda() && d.scalar_type() == at::kFloat && d.is_contiguous() && d.dim() == 2,
                "gt_bwd_finalize: dbs must be a contiguous (slots, C) fp32 GPU tensor");
    TORCH_CHECK(gbt.is_cuda() && gbt.scalar_type() == at::kFloat && gbt.is_contiguous() && gbt.numel() == d.size(1),
                "gt_bwd_finalize: gbias must have dbs.size(1) fp32 elements");
    bslots = (int)d.size(0);
    BC = (int)d.size(1);
    dbp = d.data_ptr<float>();
    gbp = gbt.data_ptr<float>();
  }
  const at::DeviceGuard guard(C > 0 ? coef.device() : gbias->device());
  check(apneauq::launch_gt_bwd_finalize(C > 0 ? bst.data_ptr<float>() : nullptr, C > 0 ? (int)(bst.numel() / (2 * C)) : 0,
                                        (int)C, inv_count, C > 0 ? coef.data_ptr<float>() : nullptr,
                                        C > 0 ? ggamma.data_ptr<float>() : nullptr,
                                        C > 0 ? gbeta.data_ptr<float>() : nullptr, dbp, bslots, BC, gbp, cur_stream()),
        "gt_bwd_finalize");
}

// Generic wgrad (csrc/generic_wgrad.hip): gw (k, cin, cout) fp32 += sum_R x[R + tap] dz[R]; gw pre-zeroed.
// part (deterministic mode): fp32 scratch for the per-row-group partials, summed in order into gw.
void gt_wgrad(const at::Tensor& x, const at::Tensor& dz, int64_t R, int64_t cin, int64_t cout, int64_t k, at::Tensor& gw,
              const c10::optional<at::Tensor>& part) {
  need_rows(x, R + k - 1, cin, "gt_wgrad x");
  need_rows(dz, R, cout, "gt_wgrad dz");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 && dz.scalar_type() == at::kBFloat16, "gt_wgrad: bf16 (fp32: gf_wgrad)");
  need_f32(gw, k * cin * cout, "gt_wgrad gw");
  TORCH_CHECK(k >= 1 && k <= 15 && cin >= 1 && cout >= 1, "gt_wgrad: 1 <= k <= 15");
  const at::DeviceGuard guard(x.device());
  float* pp = nullptr;
  if (part.has_value() && part->defined()) {
    need_f32(*part, k * cin * cout, "gt_wgrad part");
    pp = part->data_ptr<float>();
  }
  check(apneauq::launch_gt_wgrad(x.data_ptr(), x.numel() / cin, dz.data_ptr(), R, (int)cin, (int)cout, (int)k,
                                 gw.data_ptr<float>(), cur_stream(), pp, pp ? part->numel() : 0),
        "gt_wgrad");
}

// Generic head (csrc/generic_wgrad.hip): GAP + Dense + BCE + dlogit + dense grads, n samples.
void gt_head(const at::Tensor& h, const at::Tensor& w, const at::Tensor& b, const at::Tensor& y, at::Tensor& prob,
             at::Tensor& dlog, at::Tensor& loss, at::Tensor& gw, at::Tensor& gb, int64_t n, int64_t L, int64_t C,
             double inv_gb, const c10::optional<at::Tensor>& part) {
  need_rows(h, n * L, C, "gt_head h");
  need_f32(w, C, "gt_head w");
  for (const at::Tensor* t : std::initializer_list<const at::Tensor*>{&b, &loss, &gb}) need_f32(*t, 1, "gt_head scalar");
  for (const at::Tensor* t : std::initializer_list<const at::Tensor*>{&y, &prob, &dlog}) need_f32(*t, n, "gt_head per-sample");
  need_f32(gw, C, "gt_head gw");
  TORCH_CHECK(C >= 1 && C <= 4096 && L >= 1, "gt_head: bad shape");
  float* pp = nullptr;  // deterministic mode: per-workgroup records, summed in order
  if (part.has_value() && part->defined()) {
    need_f32(*part, ((n + 3) / 4) * (C + 2), "gt_head part");
    pp = part->data_ptr<float>();
  }
  const at::DeviceGuard guard(h.device());
  check(apneauq::launch_gt_head(h.data_ptr(), w.data_ptr<float>(), b.data_ptr<float>(), y.data_ptr<float>(),
                                prob.data_ptr<float>(), dlog.data_ptr<float>(), loss.data_ptr<float>(),
                                gw.data_ptr<float>(), gb.data_ptr<float>(), (int)n, (int)L, (int)C, (float)inv_gb,
                                cur_stream(), pp, pp ? part->numel() : 0, h.scalar_type() == at::kFloat),
        "gt_head");
}

// fp32 conv (csrc/gf32_conv.hip): mode 1 y = relu(conv(x) + bias) + BN moment slots (det: one slot per
// (workgroup, wave row)); mode 2 y = conv(x) with the flipped kernel (flip, dgrad).  w is the Keras kernel
// (k, Cin_k, Cout_k) read in place: forward cin = Cin_k, cout = Cout_k; dgrad cin = Cout_k, cout = Cin_k.
void gf_conv(const at::Tensor& x, const at::Tensor& w, const c10::optional<at::Tensor>& bias, at::Tensor& y,
             const c10::optional<at::Tensor>& stats, int64_t n, int64_t L, int64_t cin, int64_t cout, int64_t ksize,
             int64_t mode, int64_t in_rs, int64_t in_off, bool det) {
  TORCH_CHECK(mode == 1 || mode == 2, "gf_conv: mode must be 1 (train) or 2 (dgrad)");
  TORCH_CHECK(ksize % 2 == 1 && ksize <= 15 && cout % 4 == 0 && cin >= 1 && n >= 0 && L >= 1, "gf_conv: bad shape");
  TORCH_CHECK(x.scalar_type() == at::kFloat && y.scalar_type() == at::kFloat, "gf_conv: fp32 activations");
  need_f32(w, ksize * cin * cout, "gf_conv w");
  TORCH_CHECK(w.dim() == 3 && w.size(0) == ksize &&
                  (mode == 1 ? (w.size(1) == cin && w.size(2) == cout) : (w.size(1) == cout && w.size(2) == cin)),
              "gf_conv: kernel shape must be (k, cin, cout) forward / (k, cout, cin) dgrad");
  TORCH_CHECK(in_rs >= L && in_off >= 0, "gf_conv: bad input row layout");
  if (n > 0) need_rows(x, (n - 1) * in_rs + in_off + L, cin, "gf_conv x");
  need_rows(y, n * L, cout, "gf_conv y");
  TORCH_CHECK(n * L < (int64_t(1) << 31), "gf_conv: too many rows");
  const float* bp = nullptr;
  float* sp = nullptr;
  int det_slots = 0;
  if (mode == 1) {
    TORCH_CHECK(bias.has_value() && stats.has_value(), "gf_conv: mode 1 needs bias and stats");
    need_f32(*bias, cout, "gf_conv bias");
    need_f32(*stats, kGtSlots * 2 * cout, "gf_conv stats");
    bp = bias->data_ptr<float>();
    sp = stats->data_ptr<float>();
    if (det) det_slots = (int)(stats->numel() / (2 * cout));
  }
  const at::DeviceGuard guard(y.device());
  check(apneauq::launch_gf32_conv(x.data_ptr<float>(), w.data_ptr<float>(), bp, y.data_ptr<float>(), sp, (int)n, (int)L,
                                  (int)cin, (int)cout, (int)ksize, (int)mode, (int)in_rs, (int)in_off, mode == 2 ? 1 : 0,
                                  det_slots, cur_stream()),
        "gf_conv");
}

// fp32 wgrad (csrc/gf32_conv.hip): gw (k, cin, cout) = sum_R x[R + tap] dz[R], row-group partials in part
// summed in a fixed order (deterministic).
void gf_wgrad(const at::Tensor& x, const at::Tensor& dz, int64_t R, int64_t cin, int64_t cout, int64_t k, at::Tensor& gw,
              at::Tensor& part) {
  TORCH_CHECK(x.scalar_type() == at::kFloat && dz.scalar_type() == at::kFloat, "gf_wgrad: fp32 activations");
  need_rows(x, R + k - 1, cin, "gf_wgrad x");
  need_rows(dz, R, cout, "gf_wgrad dz");
  need_f32(gw, k * cin * cout, "gf_wgrad gw");
  need_f32(part, k * cin * cout, "gf_wgrad part");
  TORCH_CHECK(k >= 1 && k <= 15 && cin >= 1 && cout >= 1, "gf_wgrad: 1 <= k <= 15");
  const at::DeviceGuard guard(x.device());
  check(apneauq::launch_gf32_wgrad(x.data_ptr<float>(), dz.data_ptr<float>(), R, (int)cin, (int)cout, (int)k,
                                   gw.data_ptr<float>(), part.data_ptr<float>(), part.numel(), cur_stream()),
        "gf_wgrad");
}

// All blocks' forward (+ dgrad) MFMA fragments in one launch (csrc/generic_wgrad.hip pack_kernel), and
// optionally (zero) a list of accumulators cleared by the same launch.
void gt_pack_impl(at::TensorList w, at::TensorList fwd, at::TensorList dgr, at::IntArrayRef k, at::IntArrayRef cin,
                  at::IntArrayRef cout, at::TensorList zero) {
  const int64_t nb = (int64_t)w.size();
  TORCH_CHECK(nb >= 1 && nb <= apneauq::gt_pack_max_blocks() && (int64_t)fwd.size() == nb && (int64_t)dgr.size() == nb &&
                  (int64_t)k.size() == nb && (int64_t)cin.size() == nb && (int64_t)cout.size() == nb,
              "gt_pack: inconsistent block lists");
  std::vector<const float*> wp(nb);
  std::vector<void*> fp(nb), dp(nb);
  std::vector<int> kk(nb), ci(nb), co(nb);
  for (int64_t i = 0; i < nb; ++i) {
    kk[i] = (int)k[i];
    ci[i] = (int)cin[i];
    co[i] = (int)cout[i];
    TORCH_CHECK(w[i].is_cuda() && w[i].scalar_type() == at::kFloat && w[i].is_contiguous() &&
                    w[i].numel() == k[i] * cin[i] * cout[i],
                "gt_pack: w must be contiguous fp32 (k, cin, cout)");
    const int64_t nf = ((k[i] * cin[i] + 31) / 32) * 512 * ((cout[i] + 15) / 16);
    const int64_t nd = ((k[i] * cout[i] + 31) / 32) * 512 * ((cin[i] + 15) / 16);
    TORCH_CHECK(fwd[i].scalar_type() == at::kBFloat16 && fwd[i].is_contiguous() && fwd[i].numel() == nf,
                "gt_pack: forward fragment buffer has the wrong size");
    TORCH_CHECK(dgr[i].numel() == 0 || (dgr[i].scalar_type() == at::kBFloat16 && dgr[i].is_contiguous() &&
                                        dgr[i].numel() == nd),
                "gt_pack: dgrad fragment buffer has the wrong size");
    wp[i] = w[i].data_ptr<float>();
    fp[i] = fwd[i].data_ptr();
    dp[i] = dgr[i].numel() ? dgr[i].data_ptr() : nullptr;
  }
  const int nz = (int)zero.size();
  TORCH_CHECK(nz <= apneauq::gt_pack_max_zero(), "gt_pack_zero: at most ", apneauq::gt_pack_max_zero(), " buffers");
  std::vector<void*> zp(nz);
  std::vector<long long> zw(nz);
  for (int i = 0; i < nz; ++i) {
    TORCH_CHECK(zero[i].is_cuda() && zero[i].is_contiguous() && zero[i].device() == w[0].device() &&
                    (zero[i].numel() * zero[i].element_size()) % 4 == 0 &&
                    reinterpret_cast<uintptr_t>(zero[i].data_ptr()) % 4 == 0,
                "gt_pack_zero: contiguous GPU buffers of whole 4-byte words on the weights' device required");
    zp[i] = zero[i].data_ptr();
    zw[i] = (long long)(zero[i].numel() * zero[i].element_size() / 4);
  }
  const at::DeviceGuard guard(w[0].device());
  check(apneauq::launch_gt_pack((int)nb, wp.data(), fp.data(), dp.data(), kk.data(), ci.data(), co.data(), cur_stream(),
                                nz, zp.data(), zw.data()),
        "gt_pack");
}

void gt_pack(at::TensorList w, at::TensorList fwd, at::TensorList dgr, at::IntArrayRef k, at::IntArrayRef cin,
             at::IntArrayRef cout) {
  gt_pack_impl(w, fwd, dgr, k, cin, cout, {});
}

void gt_pack_zero(at::TensorList w, at::TensorList fwd, at::TensorList dgr, at::IntArrayRef k, at::IntArrayRef cin,
                  at::IntArrayRef cout, at::TensorList zero) {
  gt_pack_impl(w, fwd, dgr, k, cin, cout, zero);
}

// ---- fp32-faithful (fp16x3) generic conv kernels (csrc/gx3_conv.hip): the precision="fp32" path ----
// packed hi/lo fragments of nb blocks' kernels (forward; + dgrad where dgr[i] is non-empty), per-tensor
// scales wsc[i] (one fp32 each), wpart: >= 16 nb floats of scratch
void gx3_pack(at::TensorList w, at::TensorList fwd, at::TensorList dgr, at::TensorList wsc, at::IntArrayRef k,
              at::IntArrayRef cin, at::IntArrayRef cout, at::Tensor& wpart) {
  const int64_t nb = (int64_t)w.size();
  TORCH_CHECK(nb >= 1 && nb <= apneauq::gx3_max_blocks() && (int64_t)fwd.size() == nb && (int64_t)dgr.size() == nb &&
                  (int64_t)wsc.size() == nb && (int64_t)k.size() == nb && (int64_t)cin.size() == nb &&
                  (int64_t)cout.size() == nb,
              "gx3_pack: inconsistent block lists");
  need_f32(wpart, 16 * nb, "gx3_pack wpart");
  std::vector<const float*> wp(nb);
  std::vector<void*> fp(nb), dp(nb);
  std::vector<float*> sp(nb);
  std::vector<int> kk(nb), ci(nb), co(nb);
  for (int64_t i = 0; i < nb; ++i) {
    kk[i] = (int)k[i];
    ci[i] = (int)cin[i];
    co[i] = (int)cout[i];
    TORCH_CHECK(k[i] >= 1 && cin[i] >= 1 && cout[i] % 4 == 0, "gx3_pack: cout must be a multiple of 4");
    TORCH_CHECK(w[i].is_cuda() && w[i].scalar_type() == at::kFloat && w[i].is_contiguous() &&
                    w[i].numel() == k[i] * cin[i] * cout[i] && reinterpret_cast<uintptr_t>(w[i].data_ptr()) % 16 == 0,
                "gx3_pack: w must be contiguous, 16-B aligned fp32 (k, cin, cout)");
    const int64_t nf = 2 * ((k[i] * cin[i] + 31) / 32) * 512 * ((cout[i] + 15) / 16);
    const int64_t nd = 2 * ((k[i] * cout[i] + 31) / 32) * 512 * ((cin[i] + 15) / 16);
    TORCH_CHECK(fwd[i].scalar_type() == at::kHalf && fwd[i].is_contiguous() && fwd[i].numel() == nf,
                "gx3_pack: forward fragment buffer must be fp16 of the packed size");
    TORCH_CHECK(dgr[i].numel() == 0 || (dgr[i].scalar_type() == at::kHalf && dgr[i].is_contiguous() && dgr[i].numel() == nd),
                "gx3_pack: dgrad fragment buffer must be fp16 of the packed size");
    need_f32(wsc[i], 1, "gx3_pack wsc");
    wp[i] = w[i].data_ptr<float>();
    fp[i] = fwd[i].data_ptr();
    dp[i] = dgr[i].numel() ? dgr[i].data_ptr() : nullptr;
    sp[i] = const_cast<float*>(wsc[i].data_ptr<float>());
  }
  const at::DeviceGuard guard(w[0].device());
  check(apneauq::launch_gx3_pack((int)nb, wp.data(), fp.data(), dp.data(), sp.data(), kk.data(), ci.data(), co.data(),
                                 wpart.data_ptr<float>(), cur_stream()),
        "gx3_pack");
}

// amax (int32, >= 1): atomicMax of max |x| (fp32 bits) over x's first n elements
void gx3_amax(const at::Tensor& x, int64_t n, at::Tensor& amax) {
  need_f32(x, n, "gx3_amax x");
  TORCH_CHECK(amax.is_cuda() && amax.scalar_type() == at::kInt && amax.numel() >= 1, "gx3_amax: amax must be int32");
  const at::DeviceGuard guard(x.device());
  check(apneauq::launch_gx3_amax(x.data_ptr<float>(), n, reinterpret_cast<unsigned*>(amax.data_ptr<int32_t>()),
                                 cur_stream()),
        "gx3_amax");
}

// mode 1: y = relu(conv(x) + bias) + BN moment slots (det: one per (workgroup, wave row)); mode 2:
// y = conv(x) with the flipped packed kernel (dgrad; cin = the forward Cout).  wfrag: gx3_pack output of
// that orientation, wsc its scale.  The input's row layout must keep >= pad zero rows around every
// sample's data (in_off >= pad, in_rs - L >= pad): taps never reach a neighbour's rows.
// amax (int32, nullable): atomicMax of the input's max |x| (the tensor maximum, for gx3_wgrad).
void gx3_conv(const at::Tensor& x, const at::Tensor& wfrag, const at::Tensor& wsc, const c10::optional<at::Tensor>& bias,
              at::Tensor& y, const c10::optional<at::Tensor>& stats, const c10::optional<at::Tensor>& amax, int64_t n,
              int64_t L, int64_t cin, int64_t cout, int64_t ksize, int64_t mode, int64_t in_rs, int64_t in_off, bool det) {
  TORCH_CHECK(mode == 1 || mode == 2, "gx3_conv: mode must be 1 (train) or 2 (dgrad)");
  TORCH_CHECK(ksize % 2 == 1 && cout % 4 == 0 && cin >= 1 && n >= 0 && L >= 1, "gx3_conv: bad shape");
  const int64_t pad = (ksize - 1) / 2;
  TORCH_CHECK(in_off >= pad && in_rs - L >= pad, "gx3_conv: input rows need >= pad zero rows around each sample");
  TORCH_CHECK(x.scalar_type() == at::kFloat && y.scalar_type() == at::kFloat, "gx3_conv: fp32 activations");
  need_rows(x, n > 0 ? (n - 1) * in_rs + in_off + L + pad : 0, cin, "gx3_conv x");
  need_rows(y, n * L, cout, "gx3_conv y");
  TORCH_CHECK(wfrag.is_cuda() && wfrag.scalar_type() == at::kHalf && wfrag.is_contiguous() &&
                  wfrag.numel() == 2 * ((ksize * cin + 31) / 32) * 512 * ((cout + 15) / 16),
              "gx3_conv: wfrag must be the fp16 hi/lo fragments of this orientation");
  need_f32(wsc, 1, "gx3_conv wsc");
  TORCH_CHECK(n * L < (int64_t(1) << 31), "gx3_conv: too many rows");
  const float* bp = nullptr;
  float* sp = nullptr;
  int det_slots = 0;
  if (mode == 1) {
    TORCH_CHECK(bias.has_value() && stats.has_value(), "gx3_conv: mode 1 needs bias and stats");
    need_f32(*bias, cout, "gx3_conv bias");
    need_f32(*stats, kGtSlots * 2 * cout, "gx3_conv stats");
    bp = bias->data_ptr<float>();
    sp = stats->data_ptr<float>();
    if (det) det_slots = (int)(stats->numel() / (2 * cout));
  }
  unsigned* ap = nullptr;
  if (amax.has_value()) {
    TORCH_CHECK(amax->is_cuda() && amax->scalar_type() == at::kInt && amax->numel() >= 1, "gx3_conv: amax must be int32");
    ap = reinterpret_cast<unsigned*>(amax->data_ptr<int32_t>());
  }
  const at::DeviceGuard guard(y.device());
  check(apneauq::launch_gx3_conv(x.data_ptr<float>(), x.numel() / cin, wfrag.data_ptr(), wsc.data_ptr<float>(), bp,
                                 y.data_ptr<float>(), sp, ap, (int)n, (int)L, (int)cin, (int)cout, (int)ksize, (int)mode,
                                 (int)in_rs, (int)in_off, det_slots, cur_stream()),
        "gx3_conv");
}

// gw (k, cin, cout) = sum_R x[R + tap] dz[R] on the fp16x3 MFMA, the operands prescaled by their tensor
// maxima amax_x / amax_dz (int32 fp32 bits, >= the true maxima); row-group partials in part summed in a
// fixed order (deterministic)
void gx3_wgrad(const at::Tensor& x, const at::Tensor& dz, const at::Tensor& amax_x, const at::Tensor& amax_dz, int64_t R,
               int64_t cin, int64_t cout, int64_t k, at::Tensor& gw, at::Tensor& part) {
  TORCH_CHECK(x.scalar_type() == at::kFloat && dz.scalar_type() == at::kFloat, "gx3_wgrad: fp32 activations");
  TORCH_CHECK(k >= 1 && k <= 15 && cin >= 1 && cout % 4 == 0, "gx3_wgrad: 1 <= k <= 15, cout % 4 == 0");
  need_rows(x, R + k - 1, cin, "gx3_wgrad x");
  need_rows(dz, R, cout, "gx3_wgrad dz");
  need_f32(gw, k * cin * cout, "gx3_wgrad gw");
  need_f32(part, k * cin * cout, "gx3_wgrad part");
  TORCH_CHECK(amax_x.is_cuda() && amax_x.scalar_type() == at::kInt && amax_dz.is_cuda() && amax_dz.scalar_type() == at::kInt,
              "gx3_wgrad: amax must be int32");
  const at::DeviceGuard guard(x.device());
  check(apneauq::launch_gx3_wgrad(x.data_ptr<float>(), dz.data_ptr<float>(),
                                  reinterpret_cast<const unsigned*>(amax_x.data_ptr<int32_t>()),
                                  reinterpret_cast<const unsigned*>(amax_dz.data_ptr<int32_t>()), R, (int)cin, (int)cout,
                                  (int)k, gw.data_ptr<float>(), part.data_ptr<float>(), part.numel(), cur_stream()),
        "gx3_wgrad");
}

at::Tensor generic_head(const at::Tensor& y, const at::Tensor& w, double b, bool out_logits) {
  TORCH_CHECK(y.is_cuda() && y.scalar_type() == at::kBFloat16 && y.is_contiguous() && y.dim() == 3, "generic_head: y must be (N, L, C) bf16");
  TORCH_CHECK(w.is_cuda() && w.scalar_type() == at::kFloat && w.is_contiguous() && w.numel() == y.size(2), "generic_head: w must be (C,) fp32");
  const at::DeviceGuard guard(y.device());
  auto out = at::empty({y.size(0)}, y.options().dtype(at::kFloat));
  check(apneauq::launch_generic_head(y.data_ptr(), w.data_ptr<float>(), (float)b, (int)y.size(0), (int)y.size(1), (int)y.size(2),
                                     out_logits ? 1 : 0, out.data_ptr<float>(), cur_stream()),
        "generic_head");
  return out;
}

}  // namespace

TORCH_LIBRARY_FRAGMENT(apneauq, m) {
  m.def("generic_conv(Tensor x, Tensor wfrag, Tensor epi, int cout, int ksize, bool pool, bool dropout, int thr, "
        "int layer, int n_win, int pass_offset, int window_offset, int seed) -> Tensor");
  m.def("generic_head(Tensor y, Tensor w, float b, bool logits) -> Tensor");
  m.def("gt_conv(Tensor x, Tensor wfrag, Tensor? bias, Tensor(a!) y, Tensor(b!)? stats, int n, int L, int cin, "
        "int cout, int ksize, int mode, int in_rs, int in_off, bool det=False) -> ()");
  m.def("gt_bn_finalize(Tensor st, int C, float inv_count, Tensor gamma, Tensor beta, float eps, float momentum, "
        "Tensor(a!) mmean, Tensor(b!) mvar, bool update, Tensor(c!) bn) -> ()");
  m.def("gt_apply(Tensor z, Tensor bn, Tensor(a!) out, int n, int L, int C, bool pool, int out_rs, int out_off, "
        "bool dropout, int thr, float inv_keep, int skey, int window_offset, Tensor? skey_dev=None) -> ()");
  m.def("gt_bwd(bool dz_mode, Tensor z, Tensor bn, Tensor? dh, Tensor? dlog, Tensor? w, float invL, int n, int L, "
        "int C, bool pool, bool dropout, int thr, float inv_keep, int skey, int window_offset, Tensor(a!)? bst, "
        "Tensor? coef, Tensor? gamma, Tensor(b!)? dz, int dz_rs, int dz_off, Tensor(c!)? gbias, Tensor? skey_dev=None, "
        "bool det=False) -> ()");
  m.def("gt_bwd_finalize(Tensor bst, int C, float inv_count, Tensor(a!) coef, Tensor(b!) ggamma, Tensor(c!) gbeta, Tensor? dbs=None, Tensor(d!)? gbias=None) -> ()");
  m.def("gt_wgrad(Tensor x, Tensor dz, int R, int cin, int cout, int k, Tensor(a!) gw, Tensor(b!)? part=None) -> ()");
  m.def("gt_head(Tensor h, Tensor w, Tensor b, Tensor y, Tensor(a!) prob, Tensor(b!) dlog, Tensor(c!) loss, "
        "Tensor(d!) gw, Tensor(e!) gb, int n, int L, int C, float inv_gb, Tensor(f!)? part=None) -> ()");
  m.def("gt_pack(Tensor[] w, Tensor(a!)[] fwd, Tensor(b!)[] dgr, int[] k, int[] cin, int[] cout) -> ()");
  m.def("gt_pack_zero(Tensor[] w, Tensor(a!)[] fwd, Tensor(b!)[] dgr, int[] k, int[] cin, int[] cout, "
        "Tensor(c!)[] zero) -> ()");
  m.def("gf_conv(Tensor x, Tensor w, Tensor? bias, Tensor(a!) y, Tensor(b!)? stats, int n, int L, int cin, int cout, "
        "int ksize, int mode, int in_rs, int in_off, bool det=False) -> ()");
  m.def("gf_wgrad(Tensor x, Tensor dz, int R, int cin, int cout, int k, Tensor(a!) gw, Tensor(b!) part) -> ()");
  m.def("gx3_pack(Tensor[] w, Tensor(a!)[] fwd, Tensor(b!)[] dgr, Tensor(c!)[] wsc, int[] k, int[] cin, int[] cout, "
        "Tensor(d!) wpart) -> ()");
  m.def("gx3_amax(Tensor x, int n, Tensor(a!) amax) -> ()");
  m.def("gx3_conv(Tensor x, Tensor wfrag, Tensor wsc, Tensor? bias, Tensor(a!) y, Tensor(b!)? stats, Tensor(c!)? amax, "
        "int n, int L, int cin, int cout, int ksize, int mode, int in_rs, int in_off, bool det=False) -> ()");
  m.def("gx3_wgrad(Tensor x, Tensor dz, Tensor amax_x, Tensor amax_dz, int R, int cin, int cout, int k, Tensor(a!) gw, "
        "Tensor(b!) part) -> ()");
}

TORCH_LIBRARY_IMPL(apneauq, CUDA, m) {
  m.impl("generic_conv", &generic_conv);
  m.impl("generic_head", &generic_head);
  m.impl("gt_conv", &gt_conv);
  m.impl("gt_bn_finalize", &gt_bn_finalize);
  m.impl("gt_apply", &gt_apply);
  m.impl("gt_bwd", &gt_bwd);
  m.impl("gt_bwd_finalize", &gt_bwd_finalize);
  m.impl("gt_wgrad", &gt_wgrad);
  m.impl("gt_head", &gt_head);
  m.impl("gt_pack", &gt_pack);
  m.impl("gt_pack_zero", &gt_pack_zero);
  m.impl("gf_conv", &gf_conv);
  m.impl("gf_wgrad", &gf_wgrad);
  m.impl("gx3_pack", &gx3_pack);
  m.impl("gx3_amax", &gx3_amax);
  m.impl("gx3_conv", &gx3_conv);
  m.impl("gx3_wgrad", &gx3_wgrad);
}
