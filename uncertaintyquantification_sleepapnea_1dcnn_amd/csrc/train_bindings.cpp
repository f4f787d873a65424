// torch.library registration of the layer-wise training kernels (train_launch.hip), namespace torch.ops.apneauq.
#include "bind_util.h"
#include "train_api.h"

#include <cstring>
#include <string>
#include <vector>

namespace {
using namespace apneauq::bind;

// ctx: int64 CPU tensor of device pointers / scalars built once per workspace (ops/train_ops.py pack_ctx): one slot
// per field of the two lists in train_ctx.h, in list order -- the six layers' fields, then the launch-wide ones
#define CTX_ONE(...) +1
constexpr int kCtxLayer = 0 APNEAUQ_TRAIN_LAYER_FIELDS(CTX_ONE, CTX_ONE, CTX_ONE, CTX_ONE, CTX_ONE, CTX_ONE);
constexpr int kCtxLen = 6 * kCtxLayer APNEAUQ_TRAIN_ARGS_FIELDS(CTX_ONE, CTX_ONE, CTX_ONE, CTX_ONE, CTX_ONE, CTX_ONE);

float bits_to_float(int64_t v) {
  uint32_t u = static_cast<uint32_t>(v);
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}

double bits_to_double(int64_t v) {
  double d;
  std::memcpy(&d, &v, 8);
  return d;
}

#define CTX_NAME_P(T, n) v.push_back(pre + #n);
#define CTX_NAME(n) v.push_back(pre + #n);
std::vector<std::string> train_ctx_fields() {
  std::vector<std::string> v;
  for (int l = 0; l < 6; ++l) {
    const std::string pre = "L" + std::to_string(l) + ".";
    APNEAUQ_TRAIN_LAYER_FIELDS(CTX_NAME_P, CTX_NAME, CTX_NAME, CTX_NAME, CTX_NAME, CTX_NAME)
  }
  const std::string pre;
  APNEAUQ_TRAIN_ARGS_FIELDS(CTX_NAME_P, CTX_NAME, CTX_NAME, CTX_NAME, CTX_NAME, CTX_NAME)
  return v;
}

// S.<field> = the next ctx slot, by the field's kind
#define CTX_P(T, n) S.n = reinterpret_cast<decltype(S.n)>(*c++);
#define CTX_I(n) S.n = static_cast<int>(*c++);
#define CTX_U(n) S.n = static_cast<unsigned>(*c++);
#define CTX_Q(n) S.n = static_cast<unsigned long long>(*c++);
#define CTX_F(n) S.n = bits_to_float(*c++);
#define CTX_D(n) S.n = bits_to_double(*c++);
apneauq::train::Args args_from_ctx(const at::Tensor& ctx, int64_t pass_base) {
  TORCH_CHECK(ctx.device().is_cpu() && ctx.scalar_type() == at::kLong && ctx.numel() == kCtxLen,
              "train ctx must be an int64 CPU tensor of length ", kCtxLen);
  const int64_t* c = ctx.data_ptr<int64_t>();
  apneauq::train::Args A;
  for (auto& S : A.L) {
    APNEAUQ_TRAIN_LAYER_FIELDS(CTX_P, CTX_I, CTX_U, CTX_Q, CTX_F, CTX_D)
  }
  {
    auto& S = A;
    APNEAUQ_TRAIN_ARGS_FIELDS(CTX_P, CTX_I, CTX_U, CTX_Q, CTX_F, CTX_D)
  }
  if (pass_base >= 0) A.pass_base = static_cast<unsigned>(pass_base);
  A.bwd_self = 0;
  TORCH_CHECK(A.hpart == nullptr || A.det == nullptr, "train ctx: head slots are for the atomic mode");
  TORCH_CHECK(A.tab == nullptr || (A.det == nullptr && A.groups == 1 && A.wpart != nullptr),
              "train ctx: the parameter table needs one stats group, no deterministic partials and wgrad partials "
              "(wgrad_reduce writes its backward rows)");
  TORCH_CHECK(A.st_groups >= A.groups, "train ctx: moment buffers hold fewer groups than requested");
  return A;
}

// op: 0 fwd(layer; flag=1: the pass-shared block 1 of batch-BN MC Dropout, over the n_win windows)
//     | 1 head(flag bit 0 = backward, bit 1 = + the table's forward rows, replacing op 5) | 2 dgrad(layer) | 3 wgrad(layer) | 4 finalize(layer=update_moving, flag=grads)
//     (2 / 3: flag bit 0 = Args::bwd_self, the backward BN rows from the slots instead of the table; bit 1 =
//     the fused single-device step: wgrad launches no reduce, dgrad<l> reduces wgrad<l+1>'s partials, and
//     finalize (flag bit 1, bit 0 = grads) those of wgrad<1> / wgrad<0>)
//     | 5 parameter table (flag 0: forward rows of every block, 1: backward rows of block ``layer``)
void train_call(const at::Tensor& ctx, int64_t op, int64_t layer, int64_t flag, int64_t pass_base, int64_t device) {
  const at::DeviceGuard guard(at::Device(at::kCUDA, static_cast<c10::DeviceIndex>(device)));
  auto A = args_from_ctx(ctx, pass_base);
  TORCH_CHECK(A.B > 0 && A.n_win > 0 && A.groups > 0, "train_call: bad sizes");
  hipStream_t s = cur_stream();
  switch (op) {
    case 0:
      TORCH_CHECK(layer >= 0 && layer < 6);
      if (flag == 1) {
        TORCH_CHECK(layer == 0 && A.shared0, "train fwd: flag 1 = shared block 1 (layer 0, shared0 ctx)");
        A.B = A.n_win;  // one copy per window; stats group 0 (the buffers keep the ctx's group stride)
      }
      check(apneauq::train_launch_fwd(A, (int)layer, s), "train fwd");
      break;
    case 1: check(apneauq::train_launch_head(A, (int)(flag & 1), s, (flag & 2) != 0), "train head"); break;
    case 2:
      TORCH_CHECK(layer >= 1 && layer < 6);
      A.bwd_self = (int)(flag & 1);
      check(apneauq::train_launch_dgrad(A, (int)layer, s, (flag & 2) != 0), "train dgrad");
      break;
    case 3:
      TORCH_CHECK(layer >= 0 && layer < 6);
      A.bwd_self = (int)(flag & 1);
      check(apneauq::train_launch_wgrad(A, (int)layer, s, (flag & 2) != 0), "train wgrad");
      break;
    case 4: check(apneauq::train_launch_finalize(A, (int)layer, (int)(flag & 1), s, (flag & 2) != 0), "train finalize"); break;
    case 5: check(apneauq::train_launch_tab(A, (int)flag, (int)layer, s), "train param table"); break;
    default: TORCH_CHECK(false, "train_call: unknown op ", op);
  }
}

// Member-batched training (train_launch.hip train_launch_mb): the Args of M members' contexts in one device
// array, validated to share every size / mode the launch geometry depends on.
at::Tensor train_args_dev(const std::vector<at::Tensor>& ctxs, int64_t device) {
  const int64_t M = (int64_t)ctxs.size();
  TORCH_CHECK(M >= 1 && M <= 65535, "train_args_dev: 1..65535 member contexts");
  std::vector<apneauq::train::Args> v;
  v.reserve(M);
  for (const auto& c : ctxs) v.push_back(args_from_ctx(c, -1));
  const auto& a = v[0];
  for (const auto& x : v) {
    TORCH_CHECK(x.B == a.B && x.n_win == a.n_win && x.groups == 1 && x.st_groups == a.st_groups && (x.det == nullptr) == (a.det == nullptr) &&
                    !x.shared0 && (x.tab == nullptr) == (a.tab == nullptr) && x.wpart != nullptr &&
                    (x.hpart == nullptr) == (a.hpart == nullptr) && x.pass_dev != nullptr,
                "train_args_dev: member contexts must share batch size, stats groups and modes (atomic or "
                "deterministic, device counters, wgrad partials)");
  }
  auto cpu = at::empty({M * (int64_t)sizeof(apneauq::train::Args)}, at::TensorOptions().dtype(at::kByte));
  std::memcpy(cpu.data_ptr(), v.data(), M * sizeof(apneauq::train::Args));
  return cpu.to(at::Device(at::kCUDA, static_cast<c10::DeviceIndex>(device)));
}

void train_call_mb(const at::Tensor& args_dev, const at::Tensor& ctx0, int64_t M, int64_t op, int64_t layer, int64_t flag) {
  TORCH_CHECK(args_dev.is_cuda() && args_dev.scalar_type() == at::kByte && args_dev.is_contiguous() &&
                  args_dev.numel() == M * (int64_t)sizeof(apneauq::train::Args),
              "train_call_mb: args_dev must hold M device Args (train_args_dev)");
  const auto A0 = args_from_ctx(ctx0, -1);
  TORCH_CHECK(op >= 0 && op <= 5, "train_call_mb: unknown op ", op);
  TORCH_CHECK((op != 0 || (layer >= 0 && layer < 6)) && (op != 2 || (layer >= 1 && layer < 6)) &&
                  (op != 3 || (layer >= 0 && layer < 6)),
              "train_call_mb: bad layer");
  const at::DeviceGuard guard(args_dev.device());
  check(apneauq::train_launch_mb(A0, reinterpret_cast<const apneauq::train::Args*>(args_dev.data_ptr()), (int)M,
                                 (int)op, (int)layer, (int)flag, cur_stream()),
        "train_call_mb");
}

int64_t train_wgrad_part_size(int64_t B) { return apneauq::train_wgrad_part_floats((int)B); }
int64_t train_det_size(int64_t B) { return apneauq::train_det_floats((int)B); }

}  // namespace

TORCH_LIBRARY_FRAGMENT(apneauq, m) {
  m.def("train_ctx_fields() -> str[]", &train_ctx_fields);
  m.def("train_call(Tensor ctx, int op, int layer, int flag, int pass_base, int device) -> ()", &train_call);
  m.def("train_args_dev(Tensor[] ctxs, int device) -> Tensor", &train_args_dev);
  m.def("train_call_mb(Tensor args_dev, Tensor ctx0, int M, int op, int layer, int flag) -> ()", &train_call_mb);
  m.def("train_wgrad_part_size(int B) -> int", &train_wgrad_part_size);
  m.def("train_det_size(int B) -> int", &train_det_size);
}
