// The split-fp16 ("x3") operand rule, shared by the forward kernels (conv_f16.hip) and the training backward (train_half.hip).
#pragma once
#include "common.h"

// X3 ("split fp16") operands: a real value v is carried as the fp16 pair hi = f16(v·2^s), lo = f16(v·2^s − hi), i.e. 22
// significand bits, and a product as hi·hi + hi·lo + lo·hi on the fp16 matrix cores with fp32 accumulation (the dropped
// lo·lo term is 2^-22 relative): fp32-grade results at 16/3 of the fp32 MFMA rate. Tensors keep the NHWC fp16 machinery:
// 16 real channels are one 32-half record [hi 0..15 | lo 0..15], so a tensor with C real channels looks like an fp16
// tensor with 2C channels and the loaders run unchanged; one 32-wide K chunk is then 16 real channels of a tap.
struct X3Pair { _Float16 hi, lo; };
static __device__ __forceinline__ X3Pair x3_split(float x, float scale) {
  float v = x * scale;
  v = fminf(fmaxf(v, -60000.f), 60000.f);     // saturate instead of inf (fp16 max 65504)
  const _Float16 h = (_Float16)v;
  return {h, (_Float16)(v - (float)h)};
}
// the same, tracking the largest scaled magnitude in `amax` (one v_max per value): the caller reports a clamp once per thread
// through bit DI_STATUS_X3_SATURATED of the context's status word — saturation is never silent
static __device__ __forceinline__ X3Pair x3_split(float x, float scale, float& amax) {
  amax = fmaxf(amax, fabsf(x * scale));
  return x3_split(x, scale);
}
static __device__ __forceinline__ void x3_report(float amax, int* status) {
  if (amax > 60000.f) atomicOr(status, DI_STATUS_X3_SATURATED);
}
