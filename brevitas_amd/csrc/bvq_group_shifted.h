// bvq_group_shifted.h -- the statistics -> scale and zero-point chain of the asymmetric group-wise quantizer, shared by
// its own kernels (bvq_group_shifted.hip) and the GPTQ column loop (bvq_gptq.hip): the ordered keys of a chunk's
// largest and smallest element, the two statistics behind them, and scale and integer zero-point with the rounding
// points of the torch ops.
#pragma once

#include "bvq_group_quant.h"

namespace bvq {

// Largest and smallest element of one 16-byte chunk as ORDERED keys: the sign-magnitude pattern b of a float mapped to
// an integer that compares like the value (negative: magnitude bits flipped), then biased into unsigned order so that
// seg_max_u32 / seg_min_u32 apply.  A NaN keeps its place at one of the two ends (positive above +inf, negative below
// -inf), so it always survives one of the two reductions: shifted_stats() hands it to both statistics.  The keys of -0
// and +0 differ by one; nothing reads that: the statistics are compared as VALUES from here on.
template <typename T>
__device__ __forceinline__ void chunk_minmax_keys(const vec_t<T, elem<T>::vec>& xv, uint32_t& kmax, uint32_t& kmin) {
  constexpr int VEC = elem<T>::vec;
  if constexpr (sizeof(T) == 2) {
    typedef short i16x2 __attribute__((ext_vector_type(2)));
    const vec_t<uint32_t, VEC / 2> w = __builtin_bit_cast(vec_t<uint32_t, VEC / 2>, xv);
    i16x2 hi = {-32768, -32768}, lo = {32767, 32767};
#pragma unroll
    for (int k = 0; k < VEC / 2; ++k) {
      const i16x2 b = __builtin_bit_cast(i16x2, w.v[k]);
      const i16x2 key = b ^ ((b >> 15) & (short)0x7fff);  // signed order, two elements per word
      hi = __builtin_elementwise_max(hi, key);
      lo = __builtin_elementwise_min(lo, key);
    }
    const short mx = hi.x > hi.y ? hi.x : hi.y, mn = lo.x < lo.y ? lo.x : lo.y;
    kmax = ((uint32_t)(uint16_t)mx) ^ 0x8000u;
    kmin = ((uint32_t)(uint16_t)mn) ^ 0x8000u;
  } else {
    kmax = 0u;
    kmin = ~0u;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      const int32_t b = __builtin_bit_cast(int32_t, xv.v[k]);
      const uint32_t key = (uint32_t)b ^ ((uint32_t)(b >> 31) | 0x80000000u);
      kmax = key > kmax ? key : kmax;
      kmin = key < kmin ? key : kmin;
    }
  }
}

// the value of T behind an ordered key
template <typename T>
__device__ __forceinline__ float ordered_key_value(uint32_t key) {
  if constexpr (sizeof(T) == 2) {
    const uint32_t k = key ^ 0x8000u;
    const uint32_t b = ((k & 0x8000u) ? (k ^ 0x7fffu) : k) & 0xffffu;
    if constexpr (elem<T>::id == BVQ_F16)
      return (float)__builtin_bit_cast(f16_t, (uint16_t)b);
    else
      return __builtin_bit_cast(float, b << 16);
  } else {
    return __builtin_bit_cast(float, (key & 0x80000000u) ? (key ^ 0x80000000u) : ~key);
  }
}

// the group's two statistics from the segment-wide keys; a NaN anywhere in the group is both, as torch.max / torch.min
// propagate it
template <typename T>
__device__ __forceinline__ void shifted_stats(uint32_t kmax, uint32_t kmin, float& mx, float& mn) {
  mx = ordered_key_value<T>(kmax);
  mn = ordered_key_value<T>(kmin);
  const bool nan = mx != mx || mn != mn;
  mx = nan ? __builtin_nanf("") : mx;
  mn = nan ? __builtin_nanf("") : mn;
}

// v + 0.0 of the torch ops that add a zero (the zero-point's "+ min_int", the dense zero gradients added to dx): only a
// -0 changes, to +0.  On the bit pattern: written as a float add of a constant zero, the compiler may fold it into a
// sign modifier of the next instruction, which keeps the -0.
__device__ __forceinline__ float plus_zero(float v) {
  return __builtin_bit_cast(uint32_t, v) == 0x80000000u ? 0.f : v;
}

// statistics -> scale and zero-point with the rounding points of the torch ops (scale: bvq_stat_epilogue.h through
// group_scale; zero-point: IntQuant.to_int of -m0 with min_int = 0, bvq_quant_math.h).  d, u and r are what the backward
// needs of the way there.
struct ShiftedGroup {
  float s, zp;
  float d;  // T(mx - mn)
  float u;  // T(-m0 / s)
  float r;  // round(u + 0), before the clamp
};
template <typename T>
__device__ __forceinline__ ShiftedGroup shifted_group(float mx, float mn, const GroupArgs& a, float qmin, float qmax) {
  ShiftedGroup p;
  p.d = rnd<T>(mx - mn);
  p.s = group_scale<T>(__builtin_fabsf(p.d), a.use_min != 0, a.min_val, a.thr_div);
  const float m0 = mn <= 0.f ? mn : 0.f;  // NegativeMinOrZero: a NaN minimum gives 0, the scale is NaN then anyway
  p.u = rnd<T>(-m0 / p.s);
  p.r = round_op<T, BVQ_ROUND>(plus_zero(p.u));  // "+ min_int": -0 becomes +0
  p.zp = clamp_where(p.r, qmin, qmax);      // a NaN passes
  return p;
}

}  // namespace bvq
