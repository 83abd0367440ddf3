// bvq_act.h -- the activations a quantizer kernel can apply to x before the statistic / the quantizer
// (bvq_pre_op, include/bvq.h), beyond the ReLU the kernels take as a run-time flag (pre_relu).
//
// A kernel instantiated with ACT = BVQ_PRE_SIGMOID or BVQ_PRE_TANH computes a = act(x) exactly as torch's device kernels
// do -- in float opmath, rounded to x's dtype -- and, in backward, turns the quantizer's input gradient (rounded to x's
// dtype, as autograd hands it on) into dx with torch's sigmoid_backward / tanh_backward:
//   sigmoid           1 / (1 + exp(-x))                      (ATen UnarySigmoidKernels)
//   sigmoid_backward  g * (1 - y) * y                        (ATen BinaryMiscBackwardOpsKernels)
//   tanh              tanh(x)
//   tanh_backward     g * (1 - y * y)
// The backward's rounding is torch's as measured on the device: float32 contracts tanh_backward's 1 - y * y to one
// fma (written out here: the library is compiled with -ffp-contract=off), float16 / bfloat16 round after every
// operation.  16-bit tanh does not match torch on every input (bfloat16 tanh, float16 tanh_backward): the
// Python routing leaves it materialised.
// ACT = 0 is "no activation of this header": the existing instantiations, whose ReLU / none choice stays a run-time
// flag.  tests/test_gpu_act_fused.py compares bvq_selftest_pre_op with torch over every 16-bit input and a large
// float32 sample.
#pragma once

#include "bvq_quant_math.h"

namespace bvq {

template <int ACT>
__device__ __forceinline__ float act_f(float x) {
  if constexpr (ACT == BVQ_PRE_SIGMOID) {
    return 1.0f / (1.0f + expf(-x));
  } else if constexpr (ACT == BVQ_PRE_TANH) {
    return tanhf(x);
  } else {
    return x;
  }
}

// gradient w.r.t. x from the gradient g w.r.t. a = act(x) and a itself (both values of T).  float32 computes in float
// (tanh_backward's 1 - y * y contracted to an fma); the 16-bit types round after every operation, as ATen's device
// kernels for Half / BFloat16 do on this platform (measured: tests/test_gpu_act_fused.py)
template <typename T, int ACT>
__device__ __forceinline__ float act_bwd_f(float g, float a) {
  if constexpr (ACT == BVQ_PRE_SIGMOID) {
    return rnd<T>(rnd<T>(g * rnd<T>(1.0f - a)) * a);
  } else if constexpr (ACT == BVQ_PRE_TANH) {
    if constexpr (sizeof(T) == 4) {
      return g * __builtin_fmaf(-a, a, 1.0f);
    } else {
      return rnd<T>(g * rnd<T>(1.0f - rnd<T>(a * a)));
    }
  } else {
    return g;
  }
}

// a = act(x) rounded to T
template <typename T, int ACT>
__device__ __forceinline__ float act_rnd(float x) {
  return rnd<T>(act_f<ACT>(x));
}
template <typename T, int ACT>
__device__ __forceinline__ f2 act_rnd2(f2 x) {
  return f2{act_rnd<T, ACT>(x.x), act_rnd<T, ACT>(x.y)};
}

// dx from the quantizer's input gradient d (not yet rounded) and a: both rounding points of torch's route
template <typename T, int ACT>
__device__ __forceinline__ float act_bwd_rnd(float d, float a) {
  return rnd<T>(act_bwd_f<T, ACT>(rnd<T>(d), a));
}
template <typename T, int ACT>
__device__ __forceinline__ f2 act_bwd_rnd2(f2 d, f2 a) {
  return f2{act_bwd_rnd<T, ACT>(d.x, a.x), act_bwd_rnd<T, ACT>(d.y, a.y)};
}

}  // namespace bvq
