// The argument block of the layer-wise training kernels (train_fwd / train_head / train_dgrad / train_wgrad.hip, train_reduce.hip): train::Layer and
// train::Args, passed by value to every fwd / head / dgrad / wgrad / tab launch and copied raw into the device
// array of the member-batched step.  Seen by the kernels (through train_args.h) and by the host bindings.
//
// The structs, the decoder of the Python-built ctx (train_bindings.cpp args_from_ctx) and the ctx's name
// table (torch.ops.apneauq.train_ctx_fields) all expand the two field lists below, in list order: a field
// is added by adding one line here.  Kinds: P(type, name) device pointer, I int, U unsigned, Q unsigned
// 64-bit, F float and D double (both carried in the int64 ctx as their bit patterns).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#if defined(__HIPCC__)
#include "common.h"
#endif

namespace apneauq {
namespace train {

// Element types: the kernels see them, the host compiler sees void (a pointer's size does not depend on them).
#if defined(__HIPCC__)
typedef gbf16x8 frag_t;  // 16-B MFMA weight fragment in global memory
typedef __bf16 act_t;    // padded-row (PL) activation
#else
typedef void frag_t;
typedef void act_t;
#endif

#define APNEAUQ_TRAIN_LAYER_FIELDS(P, I, U, Q, F, D)                                                           \
  P(const frag_t, wf)  /* forward fragments  (ksteps, Cout/16, 64, 8) */                                      \
  P(const frag_t, wd)  /* dgrad fragments    (ksteps', Cin/16, 64, 8) */                                      \
  P(const float, bias)                                                                                         \
  P(const float, gamma)                                                                                        \
  P(const float, beta)                                                                                         \
  P(float, mmean)                                                                                              \
  P(float, mvar)                                                                                               \
  P(float, gw)         /* dW (k, Cin, Cout) fp32, in the flat gradient buffer */                               \
  P(float, gb)                                                                                                 \
  P(float, ggamma)                                                                                             \
  P(float, gbeta)                                                                                              \
  P(act_t, R)          /* PL (rows, C) post-ReLU, pre-BN */                                                    \
  P(act_t, dY)         /* PL (rows, C) gradient wrt BN output (blocks 1..5) */                                 \
  P(act_t, dZ)         /* PL (rows, C) gradient wrt the conv pre-activation, written by dgrad_l (l >= 1) */    \
  P(double, st)        /* [slots][groups][2][C] forward moment sums (sum r, sum r^2), fp64 */                  \
  P(double, bst)       /* [slots][2][C] backward sums (sum dY, sum dY * xhat), fp64: partial sums of data-    \
                          parallel ranks then add exactly (a 2-rank step computes the 1-rank BN-backward      \
                          coefficients bit for bit in deterministic mode) */                                   \
  U(thr)               /* dropout threshold (16-bit units) and 1/(1-p) */                                      \
  F(dsc)

// wpart  wgrad partials [row group][K*Cin*Cout + Cout] (nullptr: fp32 atomics)
// det    deterministic mode (training, one stats group): per-workgroup / per-sample partial sums of the BN
//        moments, head and dgrad statistics go here with plain stores and det_reduce_kernel adds them in a
//        fixed order (nullptr: atomics, whose summation order varies run to run)
// shared0  batch-BN MC Dropout: block 1 (no dropout before it) is computed once for the n_win windows (stats
//        group 0, R_0 unencoded, indexed by window) and shared by every pass; block 2's staging applies block
//        1's dropout from the hash
// tab    single-device training: per-layer BN parameter table [6][kTabRows][256] fp32 (mean, rstd, gamma*rstd,
//        beta - mean*gamma*rstd, mean dY, mean dY*xhat), written once per step by tab_kernel; the ~512
//        workgroups of each backward kernel read a few KB instead of each re-summing 16 fp64 slots per channel
//        from the device-coherent moment buffers (~100 MB per dgrad launch).  nullptr: slot sums
// hpart  training head: per-workgroup dense-weight / loss / dense-bias sums go to [kStatSlots][96 + 2] fp32
//        slots (workgroup % kStatSlots) that bn_finalize adds in slot order, instead of 256 workgroups'
//        atomics on the same 98 addresses (nullptr: direct atomics)
#define APNEAUQ_TRAIN_ARGS_FIELDS(P, I, U, Q, F, D)                                                            \
  P(const act_t, x)    /* PL (rows, 4) */                                                                      \
  P(const float, y)    /* labels (B) */                                                                        \
  P(const float, dense_w)                                                                                      \
  P(const float, dense_b)                                                                                      \
  P(float, g_dense_w)                                                                                          \
  P(float, g_dense_b)                                                                                          \
  P(float, logits)     /* (B) */                                                                               \
  P(float, dlogit)     /* (B) */                                                                               \
  P(float, loss_sum)   /* (1) */                                                                               \
  I(B)                 /* samples in this launch (T*N for batch-BN MC Dropout) */                              \
  I(n_win)             /* samples per stats group (B for training, N for MC Dropout) */                        \
  I(groups)            /* number of stats groups */                                                            \
  U(pass_base)         /* dropout pass id of group 0 */                                                        \
  U(window_offset)                                                                                             \
  Q(seed)                                                                                                      \
  D(inv_count)         /* 1 / (samples per group * 60) -- BN moment normaliser; a double (and next to the */   \
                       /* 64-bit seed, so the block keeps its size): a float 1/3840 is off by 2^-25 */        \
  I(dropout)                                                                                                   \
  F(inv_batch)         /* 1 / global batch size -- BCE mean */                                                 \
  F(eps)                                                                                                       \
  F(momentum)                                                                                                  \
  P(const unsigned, pass_dev) /* optional device step counter added to pass_base (HIP-graph replays) */        \
  I(st_groups)         /* groups the moment buffers are allocated for (>= groups) */                           \
  P(float, wpart)                                                                                              \
  P(float, det)                                                                                                \
  I(shared0)                                                                                                   \
  P(float, tab)                                                                                                \
  P(float, hpart)

#define APNEAUQ_DECL_P(T, n) T* n;
#define APNEAUQ_DECL_I(n) int n;
#define APNEAUQ_DECL_U(n) unsigned n;
#define APNEAUQ_DECL_Q(n) unsigned long long n;
#define APNEAUQ_DECL_F(n) float n;
#define APNEAUQ_DECL_D(n) double n;

struct Layer {
  APNEAUQ_TRAIN_LAYER_FIELDS(APNEAUQ_DECL_P, APNEAUQ_DECL_I, APNEAUQ_DECL_U, APNEAUQ_DECL_Q, APNEAUQ_DECL_F, APNEAUQ_DECL_D)
};

struct Args {
  Layer L[6];
  APNEAUQ_TRAIN_ARGS_FIELDS(APNEAUQ_DECL_P, APNEAUQ_DECL_I, APNEAUQ_DECL_U, APNEAUQ_DECL_Q, APNEAUQ_DECL_F, APNEAUQ_DECL_D)
  int bwd_self;  // dgrad / wgrad launch flag (not in the ctx): sum the backward BN rows of block l from bst[l]
                 // themselves instead of reading the table rows that wgrad_reduce's side job writes -- so a
                 // wgrad chain on a second stream (GraphedTrainStep overlap) carries no dependency back into
                 // the dgrad chain
};

#undef APNEAUQ_DECL_P
#undef APNEAUQ_DECL_I
#undef APNEAUQ_DECL_U
#undef APNEAUQ_DECL_Q
#undef APNEAUQ_DECL_F
#undef APNEAUQ_DECL_D

// The layout every compilation pass (device, hipcc host, the bindings' host compiler) must agree on.
static_assert(sizeof(Layer) == 136 && sizeof(Args) == 1008, "train::Layer / train::Args layout changed");
static_assert(__builtin_offsetof(Args, x) == 816 && __builtin_offsetof(Args, seed) == 912 &&
                  __builtin_offsetof(Args, inv_count) == 920 && __builtin_offsetof(Args, pass_dev) == 944 && __builtin_offsetof(Args, bwd_self) == 1000,
              "train::Args layout changed");

}  // namespace train
}  // namespace apneauq
