// The split-fp16 ("fp16x3") vocabulary of the fp32-precision kernels: x3_layers.hip (the headline
// engine), gx3_conv.hip (the layer-wise kernels) and fused_tiled_x3.hip (the fused short-sequence nets).
//
// An fp32 value v is scaled by an exact power of two 2^s and held as two fp16 halves, v 2^s = hi + lo
// (hi = fp16(v 2^s), lo = fp16(v 2^s - hi)); a product of two such values is formed by three
// v_mfma_f32_16x16x32_f16 (hi hi, lo hi, hi lo; fp32 accumulate).  The ORDER of the three MFMAs is each
// kernel's own (it fixes the rounding of the accumulator, so it is part of what a kernel computes) and
// is documented where the kernel issues them: gx3::mfma3, fused_tiled_x3.hip:step, x3_layers.hip.
#pragma once

#include "common.h"

namespace apneauq {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(1))) const f16x8 gf16x8;

__device__ __forceinline__ f32x4 mfma(const f16x8& a, const f16x8& b, const f32x4& c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}

// The exponent s that puts a bound b > 0 on the values to split into [2^13, 2^14): hi = fp16(v 2^s) is
// finite (< 65504) and lo normal.  b = 0 (nothing to scale), infinity and NaN give 14; callers that need
// another answer there wrap this (tiled3::sample_exp).
__device__ __forceinline__ int prescale_exp(float bound) {
  int e = 0;
  if (bound > 0.f && bound < INFINITY) frexpf(bound, &e);  // bound = f 2^e, f in [0.5, 1)
  return min(100, max(-100, 14 - e));
}

// Split a pair: hi = fp16(a) two at a time (v_cvt_pk_f16_f32); lo = fp16(a - hi) in one mixed-precision
// FMA per element, a - hi evaluated in fp32 from hi's f16 half (op_sel_hi on src0), written straight into
// the pair's lo / hi half: 3 VALU per pair instead of 8, bit-identical to the plain convert / convert
// back / subtract / convert (tools/probes/split/split_check.hip, 8.4 M pairs).
__device__ __forceinline__ void split2(float a0, float a1, unsigned& hi, unsigned& lo) {
  hi = __builtin_bit_cast(unsigned, (f16x2){(_Float16)a0, (_Float16)a1});
  unsigned l;
  asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(l) : "v"(hi), "v"(a0));
  asm("v_fma_mixhi_f16 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(l) : "v"(hi), "v"(a1));
  lo = l;
}

}  // namespace apneauq
