// bvq_group_quant.h -- what the quantizers on the sub-wave group walk that quantize to integers share: the group-wise
// quantizer with the abs-max scale (bvq_group_quant.hip), the one that searches a clipped threshold per group
// (bvq_group_mse.hip) and the asymmetric one (bvq_group_shifted.hip).  The argument struct, statistic -> scale, the
// choice of the division, the forward chain of a chunk, the backward of a chunk with its scale-gradient sum and arg-max
// deposit, and the host-side coverage check.
#pragma once

#include "bvq_fakequant_bwd.h"
#include "bvq_group_walk.h"  // the walk itself: segmented butterflies, chunk keys, the wave's window, the dispatch
#include "bvq_stat_epilogue.h"

namespace bvq {

struct GroupArgs : WalkArgs {
  void* scale;         // fwd: [groups] out
  void* stat;          // fwd: [groups] out, bwd: in
  const void* gscale;  // bwd, nullable: gradient arriving through the returned scale, [groups]
  float qmin, qmax, min_val, thr_div;
  int32_t use_min, clamp_ste;
};

// statistic -> scale with the rounding points of the scale epilogue (bvq_stat_epilogue.h): clamp_min, then the
// quotient rounded to the scale's dtype, which is x's here
template <typename T>
__device__ __forceinline__ float group_scale(float stat, bool use_min, float min_val, float thr_div) {
  const float thr = (use_min && stat < min_val) ? min_val : stat;  // NaN passes, like torch.clamp_min
  return rnd<T>(thr / thr_div);
}

// the forward chain of IntQuant on a pair (the rounding points of bvq_quant_math.h; the last rounding is the caller's
// pack2<T>).  16-bit types: the zero-point is +0, "+ zp" only turns -0 into +0 and "- zp" is the identity.
// kZp: the group has a zero-point of its own (bvq_group_shifted.hip), added and subtracted with their roundings.
template <typename T, bool kZp = false, typename Div>
__device__ __forceinline__ f2 group_fwd_pair(f2 xf, const Div& div, float s, float qmin, float qmax, float zp = 0.f) {
  f2 t = rnd2<T>(div(xf));
  if constexpr (kZp)
    t = rnd2<T>(t + zp);
  else
    t = t + 0.f;
  t = round_op2<T, BVQ_ROUND>(t);
  const f2 q = clamp_where2(t, qmin, qmax);
  if constexpr (kZp) return rnd2<T>(q - zp) * s;
  return sizeof(T) == 2 ? q * s : rnd2<T>(q - 0.f) * s;
}

template <typename T, bool kZp = false, typename Div>
__device__ __forceinline__ vec_t<T, elem<T>::vec> group_fwd_chunk(const vec_t<T, elem<T>::vec>& xv, const Div& div,
                                                                  float s, float qmin, float qmax, float zp = 0.f) {
  constexpr int VEC = elem<T>::vec;
  vec_t<T, VEC> yv;
#pragma unroll
  for (int k = 0; k < VEC; k += 2) {
    const f2 r = group_fwd_pair<T, kZp>(widen2<T>(xv.v[k], xv.v[k + 1]), div, s, qmin, qmax, zp);
    pack2<T>(r, yv.v[k], yv.v[k + 1]);
  }
  return yv;
}

// every lane's scale suits the reciprocal form of its dtype (bvq_fakequant.h): decided per wave load, and the two
// forms agree wherever the fast one is valid, so the choice cannot change a bit
template <typename T>
__device__ __forceinline__ bool wave_fast_div(float s) {
  if constexpr (elem<T>::id == BVQ_BF16)
    return __builtin_amdgcn_ballot_w64(!bf16_scale_ok(s)) == 0;
  else if constexpr (elem<T>::id == BVQ_F16)
    return __builtin_amdgcn_ballot_w64(!f16_scale_ok(s)) == 0;
  else
    return false;
}
template <typename T>
using FastDiv = std::conditional_t<elem<T>::id == BVQ_BF16, DivBf16, DivF16R>;
// r: 1.0f / s, for a caller that keeps it across several uses of one scale (bvq_gptq.hip)
template <typename T>
__device__ __forceinline__ FastDiv<T> fast_div(float s, float r) {
  if constexpr (elem<T>::id == BVQ_BF16)
    return DivBf16{r};
  else
    return DivF16R{s, r};
}
template <typename T>
__device__ __forceinline__ FastDiv<T> fast_div(float s) {
  return fast_div<T>(s, 1.0f / s);
}
// f(div) with the division by s that the wave takes for this load
template <typename T, typename F>
__device__ __forceinline__ auto with_group_div(float s, F&& f) {
  if constexpr (sizeof(T) == 2) {
    if (wave_fast_div<T>(s)) return f(fast_div<T>(s));
  }
  return f(DivExact{s});
}

// One chunk of the backward: dx and the two rounded scale-gradient terms per element exactly as the per-channel
// backward of the stats-scaled graph computes them (bwd_elem2, kBwdDs), the group's sum, the statistic's gradient
// with the rounding points of bwd_stats_finish_kernel, and its deposit on the first element attaining the statistic.
// kRatio: the scale came from the threshold stat * ratio rounded to T (bvq_group_mse.hip), so the threshold's gradient
// is multiplied by `ratio` and rounded once more on its way to the statistic; the element match still uses `stat`.
// sub: the lane within its segment (GroupPlace).
template <typename T, int L, bool kRatio = false, typename Div>
__device__ __forceinline__ vec_t<T, elem<T>::vec> group_bwd_chunk(const GroupArgs& a, const vec_t<T, elem<T>::vec>& xv,
                                                                  const vec_t<T, elem<T>::vec>& gv, uint32_t sub,
                                                                  const Div& div, float s, float stat, float gsc,
                                                                  float qmin, float qmax, float ratio = 1.f) {
  constexpr int VEC = elem<T>::vec;
  constexpr bool kZp0 = sizeof(T) == 2, kSame16 = sizeof(T) == 2;
  const bool clamp_ste = a.clamp_ste != 0;
  f2 ds2 = splat2(0.f), unused1 = splat2(0.f), unused2 = splat2(0.f);
  vec_t<T, VEC> dv;
#pragma unroll
  for (int k = 0; k < VEC; k += 2) {
    const f2 d = bwd_elem2<T, BVQ_ROUND, kBwdDs, kZp0, kSame16, true>(
        widen2<T>(xv.v[k], xv.v[k + 1]), widen2<T>(gv.v[k], gv.v[k + 1]), div, s, 0.f, qmin, qmax, clamp_ste,
        BVQ_ROUND, ds2, unused1, unused2);
    pack2<T>(d, dv.v[k], dv.v[k + 1]);
  }
  const float ds = seg_sum<L>(ds2.x + ds2.y);
  // dscale (+ the gradient arriving through `scale`) -> the statistic's gradient: scale = clamp_min_ste(stat) / thr_div,
  // every torch op rounding to the scale's dtype (T); the straight-through clamp passes it on
  float v = rnd<T>(ds);
  if (a.gscale) v = rnd<T>(v + gsc);
  float dstat = rnd<T>(v / a.thr_div);
  if constexpr (kRatio) dstat = rnd<T>(dstat * ratio);
  // first element of the group whose |x| is the statistic: segment-wide minimum over lane * VEC + index
  const uint32_t skey = abs_bits<T>(from_f<T>(stat));
  const uint32_t e0 = sub * VEC;
  uint32_t first = ~0u;
#pragma unroll
  for (int k = VEC - 1; k >= 0; --k) first = abs_bits<T>(xv.v[k]) == skey ? e0 + k : first;
  first = seg_min_u32<L>(first);  // ~0: no element equals the statistic (a NaN of another pattern)
#pragma unroll
  for (int k = 0; k < VEC; ++k) {
    // the owning lane adds sign(x) * dstat to its already rounded dx element: the deposit's two roundings
    const float dep = to_f<T>(dv.v[k]) + deposit<T, BVQ_MATCH_ABS>(dstat, xv.v[k]);
    dv.v[k] = first == e0 + k ? from_f<T>(dep) : dv.v[k];
  }
  return dv;
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
// what the kernels cover, apart from the pointers: BVQ_OK, or the error with its text
// shifted: the asymmetric quantizer (bvq_group_shifted.hip), one zero-point per group in x's dtype
// any_size: every `inner` passes here (the per-row kernels of bvq_row_shifted.hip, which hold their own bound to it)
static int group_check(const bvq_quant_desc* d, const char* what, bool shifted = false, bool any_size = false) {
  int rc = validate(d);
  if (rc) return rc;
  if (shifted && (d->outer != 1 || d->channels < 1 || !d->scale_per_channel || !d->zp_per_channel)) {
    set_error("%s: the descriptor of a grouped tensor with zero-points is outer 1, channels = groups, inner = group size, "
              "one scale and one zero-point per channel", what);
    return BVQ_ERR_UNSUPPORTED;
  }
  if (!shifted && (d->outer != 1 || d->channels < 1 || !d->scale_per_channel || d->zp_per_channel)) {
    set_error("%s: the descriptor of a grouped tensor is outer 1, channels = groups, inner = group size, one scale per "
              "channel and one zero-point", what);
    return BVQ_ERR_UNSUPPORTED;
  }
  if (shifted && d->zp_dtype != d->x_dtype) {
    set_error("%s: x and zero-point dtype must agree (x=%d zp=%d)", what, d->x_dtype, d->zp_dtype);
    return BVQ_ERR_UNSUPPORTED;
  }
  if (!any_size && d->inner != 16 && d->inner != 32 && d->inner != 64 && d->inner != 128 && d->inner != 256) {
    set_error("%s: group size %lld (16, 32, 64, 128 or 256)", what, (long long)d->inner);
    return BVQ_ERR_UNSUPPORTED;
  }
  if (d->round_mode != BVQ_ROUND) {
    set_error("%s: round_mode %d (half-even rounding only)", what, d->round_mode);
    return BVQ_ERR_UNSUPPORTED;
  }
  if (d->x_dtype != d->ct_dtype || d->scale_dtype != d->x_dtype) {
    set_error("%s: x, compute and scale dtype must agree (x=%d ct=%d scale=%d)", what, d->x_dtype, d->ct_dtype,
              d->scale_dtype);
    return BVQ_ERR_UNSUPPORTED;
  }
  if (d->pre_op != BVQ_PRE_NONE) {
    set_error("%s: pre_op %d is not covered", what, d->pre_op);
    return BVQ_ERR_UNSUPPORTED;
  }
  if (d->out_kind != BVQ_OUT_DEQUANT) {
    set_error("%s: integer output is not covered", what);
    return BVQ_ERR_UNSUPPORTED;
  }
  return BVQ_OK;
}

// Args: GroupArgs or what a quantizer extends it to; everything the descriptor and the scalars do not give is zero
template <typename Args = GroupArgs>
static Args group_args(const bvq_quant_desc* d, double min_val, int use_min, double thr_div) {
  Args a = {};
  a.chunks = d->channels * (d->inner * dtype_size(d->x_dtype) / 16);
  a.qmin = d->qmin;
  a.qmax = d->qmax;
  a.min_val = round_host((float)min_val, d->x_dtype);  // python scalar -> the statistic's dtype
  a.thr_div = (float)thr_div;
  a.use_min = use_min;
  a.clamp_ste = d->clamp_ste;
  return a;
}

}  // namespace bvq
