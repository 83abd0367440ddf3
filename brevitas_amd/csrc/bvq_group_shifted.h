// bvq_group_shifted.h -- the statistics -> scale and zero-point chain of the asymmetric group-wise quantizer, shared by
// its own kernels (bvq_group_shifted.hip), the per-row kernels of the dynamic activation quantizers
// (bvq_row_shifted.hip) and the GPTQ column loop (bvq_gptq.hip): the ordered keys of a chunk's largest and smallest
// element, the two statistics behind them, scale and integer zero-point with the rounding points of the torch ops, and
// the backward in the steps a kernel puts its own reductions between: the elements of a chunk, the first positions of
// the statistics, the chain from the two gradient sums to the statistics' gradients, the deposits.
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

// GroupArgs with `stat` holding [2 * groups] values, the maxima then the minima (as BVQ_STAT_MINMAX)
struct GroupShiftedArgs : GroupArgs {
  void* zp;         // fwd: [groups] out
  const void* gzp;  // bwd, nullable: gradient arriving through the returned zero-point, [groups]
};

// The backward, step 1: dx of one chunk and the rounded gradient terms of scale and zero-point per element exactly as
// the per-channel backward computes them (bwd_elem2, kBwdDsDzp), added onto ds2 / dz2.  Every element of dx has been
// through the "+ 0" of the dense zero gradients the per-channel route adds there, which turns a -0 into +0.
template <typename T, typename Div>
__device__ __forceinline__ vec_t<T, elem<T>::vec> shifted_bwd_elems(bool clamp_ste, const vec_t<T, elem<T>::vec>& xv,
                                                                    const vec_t<T, elem<T>::vec>& gv, const Div& div,
                                                                    const ShiftedGroup& p, float qmin, float qmax,
                                                                    f2& ds2, f2& dz2) {
  constexpr int VEC = elem<T>::vec;
  f2 unused = splat2(0.f);
  vec_t<T, VEC> dv;
#pragma unroll
  for (int k = 0; k < VEC; k += 2) {
    const f2 d = bwd_elem2<T, BVQ_ROUND, kBwdDsDzp, false, false, true>(
        widen2<T>(xv.v[k], xv.v[k + 1]), widen2<T>(gv.v[k], gv.v[k + 1]), div, p.s, p.zp, qmin, qmax, clamp_ste,
        BVQ_ROUND, ds2, dz2, unused);
    pack2<T>(f2{plus_zero(d.x), plus_zero(d.y)}, dv.v[k], dv.v[k + 1]);  // (d is rounded to T: the conversion is exact)
  }
  return dv;
}

// Step 2: the lowest position e0 + k of a chunk's elements equal to each statistic, folded into fmx / fmn (~0: none so
// far; a NaN statistic is equal to nothing).  e0: the position of the chunk's first element in its group.
template <typename T>
__device__ __forceinline__ void shifted_first(const vec_t<T, elem<T>::vec>& xv, uint32_t e0, float mx, float mn,
                                              uint32_t& fmx, uint32_t& fmn) {
  constexpr int VEC = elem<T>::vec;
  uint32_t cmx = ~0u, cmn = ~0u;
#pragma unroll
  for (int k = VEC - 1; k >= 0; --k) {
    const float xf = to_f<T>(xv.v[k]);
    cmx = xf == mx ? e0 + k : cmx;
    cmn = xf == mn ? e0 + k : cmn;
  }
  fmx = cmx < fmx ? cmx : fmx;
  fmn = cmn < fmn ? cmn : fmn;
}

// Step 3: the group's two float32 sums -> what its statistics receive.  The autograd of the scale-shaped torch ops of
// the graph, each rounding to T:
//   zero-point   dzp (+ gzp) -> its own clamp (masked where it clipped unless straight-through) -> round (STE) -> "+ 0"
//                -> u = n / s: dn = dzp / s to n = -m0, -dzp * ((n / s) / s) to the scale -> m0 -> mn where mn <= 0
//   scale        ds (+ gscale) + the zero-point's share -> / thr_div -> clamp_min (STE) -> |d|: * sgn(d) -> d = mx - mn
struct ShiftedDeposit {
  float dd;     // to the first element equal to mx, and negated to the first equal to mn
  float dmn_z;  // the zero-point statistic's, to the first element equal to mn
};
template <typename T>
__device__ __forceinline__ ShiftedDeposit shifted_bwd_chain(const GroupShiftedArgs& a, const ShiftedGroup& p, float mn,
                                                            float ds, float dzs, float gsc, float gzp, float qmin,
                                                            float qmax) {
  const bool clamp_ste = a.clamp_ste != 0;
  // the zero-point's gradient on its way back through to_int
  float dzp = rnd<T>(dzs);
  if (a.gzp) dzp = rnd<T>(dzp + gzp);
  const bool zhi = p.r > qmax;
  const bool zlo = (zhi ? qmax : p.r) < qmin;
  const float dzi = (clamp_ste || !(zhi || zlo)) ? dzp : 0.f;
  const float dn = rnd<T>(dzi / p.s);
  const float dsz = rnd<T>(-dzi * rnd<T>(p.u / p.s));
  // the scale's gradient: the quantizer's, the one arriving through `scale`, the zero-point's share, in that order
  float v = rnd<T>(ds);
  if (a.gscale) v = rnd<T>(v + gsc);
  v = rnd<T>(v + dsz);
  const float dthr = rnd<T>(v / a.thr_div);
  const float dd = rnd<T>(dthr * sgn_f(p.d));  // abs: zero at 0, a constant group deposits nothing through it
  return {dd, mn <= 0.f ? -dn : 0.f};
}

// Step 4: the deposits on a chunk of dx, in the order the per-channel route adds its dense gradients to dx: the
// zero-point statistic's first (on the first element equal to mn), then the scale statistic's (max and min, added to
// each other first where one element is both).  fmx / fmn: the group-wide first positions.
template <typename T>
__device__ __forceinline__ void shifted_deposit(vec_t<T, elem<T>::vec>& dv, uint32_t e0, uint32_t fmx, uint32_t fmn,
                                                const ShiftedDeposit& dep) {
  constexpr int VEC = elem<T>::vec;
#pragma unroll
  for (int k = 0; k < VEC; ++k) {
    const bool is_mx = fmx == e0 + k, is_mn = fmn == e0 + k;
    float val = to_f<T>(dv.v[k]);
    val = is_mn ? rnd<T>(val + dep.dmn_z) : val;
    float add = is_mx ? dep.dd : 0.f;
    add = is_mn ? rnd<T>(add - dep.dd) : add;
    dv.v[k] = (is_mx || is_mn) ? from_f<T>(val + add) : dv.v[k];
  }
}

}  // namespace bvq
