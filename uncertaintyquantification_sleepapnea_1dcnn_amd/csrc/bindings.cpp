// torch.library registration of the apneauq HIP kernels (namespace torch.ops.apneauq): this file defines the
// library and the optimizer / counter / step-edge, metrics and preprocessing ops; every other family registers its
// operators from its own *_bindings.cpp.  Plain host C++; every kernel lives in a .hip file built for gfx950.
#include "bind_util.h"
#include "misc_api.h"

#include <vector>

namespace {
using namespace apneauq::bind;

void adam_step(at::Tensor& p, const at::Tensor& g, at::Tensor& m, at::Tensor& v, double b1, double b2, double alpha,
               double eps, double gscale, const c10::optional<at::Tensor>& counters) {
  TORCH_CHECK(p.is_cuda() && g.is_cuda() && m.is_cuda() && v.is_cuda(), "adam_step: GPU tensors required");
  for (const at::Tensor* t : std::initializer_list<const at::Tensor*>{&p, &g, &m, &v})
    TORCH_CHECK(t->scalar_type() == at::kFloat && t->is_contiguous() && t->numel() == p.numel() &&
                    reinterpret_cast<uintptr_t>(t->data_ptr()) % 16 == 0,
                "adam_step: contiguous, 16-B aligned fp32 tensors of equal size required");
  const at::DeviceGuard guard(p.device());
  const int* step_dev = nullptr;
  if (counters.has_value()) {  // [pass offset, iterations]: alpha = lr, corrected on the device
    TORCH_CHECK(counters->is_cuda() && counters->scalar_type() == at::kInt && counters->numel() >= 2,
                "adam_step: counters must be an int32 GPU tensor [pass, iterations]");
    step_dev = counters->data_ptr<int>() + 1;
  }
  check(apneauq::launch_adam(p.data_ptr<float>(), g.data_ptr<float>(), m.data_ptr<float>(), v.data_ptr<float>(),
                             p.numel(), (float)b1, (float)b2, (float)alpha, (float)eps, (float)gscale, step_dev,
                             cur_stream()),
        "adam_step");
}

// Adam over M members' flat buffers in one launch (same size and hyper-parameters; per-member device
// iteration counters [pass, iterations] as in adam_step).
void adam_step_multi(at::TensorList p, at::TensorList g, at::TensorList m, at::TensorList v, double b1, double b2,
                     double alpha, double eps, at::TensorList counters) {
  const int ns = (int)p.size();
  TORCH_CHECK(ns >= 1 && ns <= apneauq::adam_max_sets() && (int)g.size() == ns && (int)m.size() == ns &&
                  (int)v.size() == ns && (int)counters.size() == ns,
              "adam_step_multi: 1..", apneauq::adam_max_sets(), " equally long lists");
  std::vector<float*> pp(ns), mm(ns), vv(ns);
  std::vector<const float*> gg(ns);
  std::vector<const int*> st(ns);
  const int64_t n = p[0].numel();
  for (int i = 0; i < ns; ++i) {
    for (const at::Tensor* t : {&p[i], &g[i], &m[i], &v[i]})
      TORCH_CHECK(t->is_cuda() && t->device() == p[0].device() && t->scalar_type() == at::kFloat && t->is_contiguous() &&
                      t->numel() == n && reinterpret_cast<uintptr_t>(t->data_ptr()) % 16 == 0,
                  "adam_step_multi: contiguous, 16-B aligned fp32 GPU tensors of equal size on one device required");
    TORCH_CHECK(counters[i].is_cuda() && counters[i].scalar_type() == at::kInt && counters[i].numel() >= 2,
                "adam_step_multi: counters must be int32 GPU tensors [pass, iterations]");
    pp[i] = p[i].data_ptr<float>();
    gg[i] = g[i].data_ptr<float>();
    mm[i] = m[i].data_ptr<float>();
    vv[i] = v[i].data_ptr<float>();
    st[i] = counters[i].data_ptr<int>() + 1;
  }
  const at::DeviceGuard guard(p[0].device());
  check(apneauq::launch_adam_multi(ns, pp.data(), gg.data(), mm.data(), vv.data(), st.data(), n, (float)b1, (float)b2,
                                   (float)alpha, (float)eps, cur_stream()),
        "adam_step_multi");
}

// Zero several GPU buffers (4-byte multiples) in one launch.
void zero_buffers(at::TensorList ts) {
  const int nb = (int)ts.size();
  TORCH_CHECK(nb >= 1 && nb <= apneauq::zero_max_buffers(), "zero_buffers: 1..", apneauq::zero_max_buffers(), " tensors");
  std::vector<void*> p(nb);
  std::vector<long long> w(nb);
  for (int i = 0; i < nb; ++i) {
    TORCH_CHECK(ts[i].is_cuda() && ts[i].is_contiguous() && ts[i].device() == ts[0].device() &&
                    (ts[i].numel() * ts[i].element_size()) % 4 == 0 &&
                    reinterpret_cast<uintptr_t>(ts[i].data_ptr()) % 4 == 0,
                "zero_buffers: contiguous GPU tensors of whole 4-byte words on one device required");
    p[i] = ts[i].data_ptr();
    w[i] = (long long)(ts[i].numel() * ts[i].element_size() / 4);
  }
  const at::DeviceGuard guard(ts[0].device());
  check(apneauq::launch_zero(nb, p.data(), w.data(), cur_stream()), "zero_buffers");
}

void bump_counters(at::Tensor& counters) {
  TORCH_CHECK(counters.is_cuda() && counters.scalar_type() == at::kInt && counters.numel() <= 64,
              "bump_counters: int32 GPU tensor of <= 64 counters");
  const at::DeviceGuard guard(counters.device());
  check(apneauq::train_bump_counters(counters.data_ptr<int>(), (int)counters.numel(), cur_stream()), "bump_counters");
}

void stream_keys(at::Tensor& keys, const at::Tensor& counters, int64_t seed, int64_t pass_base) {
  TORCH_CHECK(keys.is_cuda() && keys.scalar_type() == at::kInt && keys.is_contiguous() && keys.numel() <= 64,
              "stream_keys: contiguous int32 GPU tensor of <= 64 keys");
  TORCH_CHECK(counters.is_cuda() && counters.scalar_type() == at::kInt && counters.numel() >= 1 &&
                  counters.device() == keys.device(), "stream_keys: int32 GPU counters on the keys' device");
  const at::DeviceGuard guard(keys.device());
  check(apneauq::train_stream_keys(reinterpret_cast<unsigned*>(keys.data_ptr<int>()), counters.data_ptr<int>(),
                                   (int)keys.numel(), static_cast<unsigned long long>(seed),
                                   static_cast<unsigned>(pass_base), cur_stream()),
        "stream_keys");
}

// The training step's tail: bump the device counters, probs = sigmoid(logits[:n]) of every member.
void train_tail(at::Tensor& counters, at::TensorList logits, at::TensorList probs) {
  const int M = (int)logits.size();
  TORCH_CHECK(M >= 1 && M <= apneauq::train_tail_max() && (int)probs.size() == M, "train_tail: 1..",
              apneauq::train_tail_max(), " members, one probs buffer each");
  TORCH_CHECK(counters.is_cuda() && counters.scalar_type() == at::kInt && counters.is_contiguous(),
              "train_tail: contiguous int32 GPU counters");
  const int64_t n = logits[0].numel();
  std::vector<const float*> lp(M);
  std::vector<float*> pp(M);
  for (int i = 0; i < M; ++i) {
    TORCH_CHECK(logits[i].is_cuda() && logits[i].scalar_type() == at::kFloat && logits[i].is_contiguous() &&
                    logits[i].numel() == n && probs[i].scalar_type() == at::kFloat && probs[i].is_contiguous() &&
                    probs[i].numel() == n && probs[i].device() == counters.device() &&
                    logits[i].device() == counters.device(),
                "train_tail: contiguous fp32 logits / probs of one length on the counters' device");
    lp[i] = logits[i].data_ptr<float>();
    pp[i] = probs[i].data_ptr<float>();
  }
  const at::DeviceGuard guard(counters.device());
  check(apneauq::launch_train_tail(counters.data_ptr<int>(), (int)counters.numel(), M, lp.data(), pp.data(), (int)n,
                                   cur_stream()),
        "train_tail");
}

// The step's inputs of every member in one launch: x (n, L, C) fp32 into the padded-row bf16 buffer
// (rows of SR, the first n * SR * C elements of xd), y (n) fp32 into yd.
void train_inputs(at::TensorList x, at::TensorList y, at::TensorList xd, at::TensorList yd, int64_t sr) {
  const int M = (int)x.size();
  TORCH_CHECK(M >= 1 && M <= apneauq::train_tail_max() && (int)y.size() == M && (int)xd.size() == M &&
                  (int)yd.size() == M,
              "train_inputs: 1..", apneauq::train_tail_max(), " members with x, y, xd, yd each");
  const int64_t n = x[0].size(0), L = x[0].size(1), C = x[0].size(2);
  std::vector<const float*> xp(M), yp(M);
  std::vector<void*> xdp(M);
  std::vector<float*> ydp(M);
  for (int i = 0; i < M; ++i) {
    TORCH_CHECK(x[i].is_cuda() && x[i].scalar_type() == at::kFloat && x[i].is_contiguous() && x[i].dim() == 3 &&
                    x[i].size(0) == n && x[i].size(1) == L && x[i].size(2) == C,
                "train_inputs: contiguous fp32 (n, L, C) inputs of one shape");
    TORCH_CHECK(y[i].is_cuda() && y[i].scalar_type() == at::kFloat && y[i].is_contiguous() && y[i].numel() == n,
                "train_inputs: contiguous fp32 labels (n)");
    TORCH_CHECK(xd[i].scalar_type() == at::kBFloat16 && xd[i].is_contiguous() && xd[i].numel() >= n * sr * C &&
                    yd[i].scalar_type() == at::kFloat && yd[i].is_contiguous() && yd[i].numel() >= n,
                "train_inputs: destination buffers too small");
    TORCH_CHECK(x[i].device() == xd[i].device() && y[i].device() == xd[i].device() && yd[i].device() == xd[i].device(),
                "train_inputs: one device per member");
    xp[i] = x[i].data_ptr<float>();
    yp[i] = y[i].data_ptr<float>();
    xdp[i] = xd[i].data_ptr();
    ydp[i] = yd[i].data_ptr<float>();
  }
  const at::DeviceGuard guard(xd[0].device());
  check(apneauq::launch_train_inputs(M, xp.data(), xdp.data(), yp.data(), ydp.data(), (int)n, (int)L, (int)C, (int)sr,
                                     cur_stream()),
        "train_inputs");
}

// K10 (csrc/metrics.hip): counts (int64, 1 + 2 (n_thr + 1)) += accuracy / AUC-bucket counts of a batch.
void metrics_update(const at::Tensor& p, const at::Tensor& y, const at::Tensor& thr, at::Tensor& counts) {
  TORCH_CHECK(p.is_cuda() && y.is_cuda() && thr.is_cuda() && counts.is_cuda(), "metrics_update: GPU tensors required");
  TORCH_CHECK(p.scalar_type() == at::kFloat && y.scalar_type() == at::kFloat && thr.scalar_type() == at::kFloat &&
              p.is_contiguous() && y.is_contiguous() && thr.is_contiguous() && p.numel() == y.numel(),
              "metrics_update: contiguous fp32 p, y of equal size and fp32 thresholds required");
  TORCH_CHECK(thr.numel() >= 1 && thr.numel() <= 1024, "metrics_update: 1..1024 thresholds");
  TORCH_CHECK(counts.scalar_type() == at::kLong && counts.is_contiguous() && counts.numel() == 1 + 2 * (thr.numel() + 1),
              "metrics_update: counts must be int64 (1 + 2 (n_thr + 1))");
  const at::DeviceGuard guard(p.device());
  check(apneauq::launch_metrics_update(p.data_ptr<float>(), y.data_ptr<float>(), p.numel(), thr.data_ptr<float>(),
                                       (int)thr.numel(), reinterpret_cast<unsigned long long*>(counts.data_ptr<int64_t>()),
                                       cur_stream()),
        "metrics_update");
}

// K14 (csrc/prep.hip): per-window z-score of an (N, L, C) float64 tensor; exact fp64 k-NN of SMOTE
at::Tensor prep_standardize(const at::Tensor& x, double eps) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kDouble && x.dim() == 3, "prep_standardize: (N, L, C) float64 GPU tensor");
  auto xc = x.contiguous();
  TORCH_CHECK(xc.size(1) * xc.size(2) * 8 <= 64 * 1024 && xc.size(2) <= 256, "prep_standardize: window too large");
  const at::DeviceGuard guard(xc.device());
  auto out = at::empty_like(xc);
  check(apneauq::launch_standardize(xc.data_ptr<double>(), out.data_ptr<double>(), xc.size(0), (int)xc.size(1),
                                    (int)xc.size(2), eps, cur_stream()),
        "prep_standardize");
  return out;
}

at::Tensor prep_knn(const at::Tensor& X, int64_t k) {
  TORCH_CHECK(X.is_cuda() && X.scalar_type() == at::kDouble && X.dim() == 2, "prep_knn: (n, D) float64 GPU tensor");
  TORCH_CHECK(k >= 1 && k <= 16, "prep_knn: 1 <= k <= 16");
  TORCH_CHECK(X.size(0) < (int64_t(1) << 31), "prep_knn: too many rows");
  auto xc = X.contiguous();
  TORCH_CHECK(apneauq::knn_lds_bytes((int)xc.size(1), k <= 8 ? 8 : 16) <= 160 * 1024, "prep_knn: rows too wide for LDS");
  const at::DeviceGuard guard(xc.device());
  auto out = at::empty({xc.size(0), k}, xc.options().dtype(at::kLong));
  check(apneauq::launch_knn(xc.data_ptr<double>(), (int)xc.size(0), (int)xc.size(1),
                            reinterpret_cast<long long*>(out.data_ptr<int64_t>()), (int)k, cur_stream()),
        "prep_knn");
  return out;
}

}  // namespace

TORCH_LIBRARY(apneauq, m) {
  m.def("prep_standardize(Tensor x, float eps) -> Tensor");
  m.def("prep_knn(Tensor X, int k) -> Tensor");
  m.def("adam_step(Tensor(a!) p, Tensor g, Tensor(b!) m, Tensor(c!) v, float b1, float b2, float alpha, float eps, "
        "float gscale, Tensor? counters=None) -> ()");
  m.def("adam_step_multi(Tensor(a!)[] p, Tensor[] g, Tensor(b!)[] m, Tensor(c!)[] v, float b1, float b2, float alpha, "
        "float eps, Tensor[] counters) -> ()");
  m.def("bump_counters(Tensor(a!) counters) -> ()");
  m.def("stream_keys(Tensor(a!) keys, Tensor counters, int seed, int pass_base) -> ()");
  m.def("zero_buffers(Tensor(a!)[] ts) -> ()");
  m.def("metrics_update(Tensor p, Tensor y, Tensor thr, Tensor(a!) counts) -> ()");
  m.def("train_tail(Tensor(a!) counters, Tensor[] logits, Tensor(b!)[] probs) -> ()");
  m.def("train_inputs(Tensor[] x, Tensor[] y, Tensor(a!)[] xd, Tensor(b!)[] yd, int sr) -> ()");
}

TORCH_LIBRARY_IMPL(apneauq, CUDA, m) {
  m.impl("adam_step", &adam_step);
  m.impl("adam_step_multi", &adam_step_multi);
  m.impl("bump_counters", &bump_counters);
  m.impl("stream_keys", &stream_keys);
  m.impl("zero_buffers", &zero_buffers);
  m.impl("metrics_update", &metrics_update);
  m.impl("train_tail", &train_tail);
  m.impl("train_inputs", &train_inputs);
  m.impl("prep_standardize", &prep_standardize);
  m.impl("prep_knn", &prep_knn);
}
