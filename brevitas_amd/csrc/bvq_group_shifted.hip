// bvq_group_shifted.hip -- asymmetric group-wise weight quantizer: unsigned codes, one scale and one integer zero-point
// per `group_size` consecutive elements (the 4-bit weight-only format of AWQ / GPTQ style checkpoints), one launch each
// way on the sub-wave group walk of bvq_group_walk.h.
//
// The result is the per-channel asymmetric graph (AbsMinMax scale, NegativeMinOrZero zero-point quantized through the
// quantizer's own to_int) on the tensor regrouped as [groups, g], every torch op rounding to x's dtype T:
//   mx = max x, mn = min x
//   scale = T(clamp_min(|T(mx - mn)|, min_val) / thr_div)
//   m0 = mn <= 0 ? mn : 0;  zp = clamp(round(T(T(-m0 / scale) + 0)), qmin, qmax)
//   q = clamp(round(T(T(x / scale) + zp)), qmin, qmax);  y = T(T(q - zp) * scale)
// A group's two statistics are segmented butterflies over ordered integer keys of the signed values, the two gradient
// sums of the backward (scale, zero-point) segmented float32 sums; the statistics' gradients land on the first element
// equal to each (-0 equals +0).  No LDS, no atomics, no workspace, no second launch.
//   forward   reads x, writes y                (+ 5 * bytes(x) / g for scale, zp and the two statistics)
//   backward  reads g and x, writes dx once    (+ 2 * bytes(x) / g for the statistics, + gscale / gzp when given)
// Only the ORDER in which a group's float32 gradient terms are added differs from the per-channel kernels, which can
// move the two deposited elements by a rounding.
#include "bvq_group_shifted.h"  // the argument struct, statistics -> scale and zero-point, the steps of the backward

namespace bvq {

// One chunk of the backward in the steps of bvq_group_shifted.h, a group's reductions being segmented butterflies
// between them.  sub: the lane within its segment (GroupPlace).
template <typename T, int L, typename Div>
__device__ __forceinline__ vec_t<T, elem<T>::vec> group_shifted_bwd_chunk(
    const GroupShiftedArgs& a, const vec_t<T, elem<T>::vec>& xv, const vec_t<T, elem<T>::vec>& gv, uint32_t sub,
    const Div& div, const ShiftedGroup& p, float mx, float mn, float gsc, float gzp, float qmin, float qmax) {
  constexpr int VEC = elem<T>::vec;
  f2 ds2 = splat2(0.f), dz2 = splat2(0.f);
  vec_t<T, VEC> dv = shifted_bwd_elems<T>(a.clamp_ste != 0, xv, gv, div, p, qmin, qmax, ds2, dz2);
  const float ds = seg_sum<L>(ds2.x + ds2.y);
  const float dzs = seg_sum<L>(dz2.x + dz2.y);
  const ShiftedDeposit dep = shifted_bwd_chain<T>(a, p, mn, ds, dzs, gsc, gzp, qmin, qmax);
  // first element of the group equal to each statistic: segment-wide minimum over lane * VEC + index
  const uint32_t e0 = sub * VEC;
  uint32_t fmx = ~0u, fmn = ~0u;
  shifted_first<T>(xv, e0, mx, mn, fmx, fmn);
  shifted_deposit<T>(dv, e0, seg_min_u32<L>(fmx), seg_min_u32<L>(fmn), dep);
  return dv;
}

// the asymmetric quantizer on the frame of bvq_group_walk.h
template <typename T, int L>
struct ShiftedQuant {
  using Args = GroupShiftedArgs;
  using Vec = vec_t<T, elem<T>::vec>;
  struct Side {
    T mx, mn, gscale, gzp;
  };
  const Args& a;
  const buf_t bs, bz, btx, btn, bgs, bgz;
  const float qmin, qmax;
  template <typename W>
  __device__ __forceinline__ ShiftedQuant(const Args& a, const W& w)
      : a(a), bs(w.groups(a.scale)), bz(w.groups(a.zp)), btx(w.groups(a.stat)),
        btn(w.groups(reinterpret_cast<const T*>(a.stat) + a.chunks / L)), bgs(w.groups_or_zeros(a.gscale, a.x)),
        bgz(w.groups_or_zeros(a.gzp, a.x)), qmin(rnd<T>(a.qmin)), qmax(rnd<T>(a.qmax)) {}

  __device__ __forceinline__ Vec fwd(const Vec& xv, const GroupPlace& p) const {
    uint32_t kmax, kmin;
    chunk_minmax_keys<T>(xv, kmax, kmin);
    float mx, mn;
    shifted_stats<T>(seg_max_u32<L>(kmax), seg_min_u32<L>(kmin), mx, mn);
    const ShiftedGroup sg = shifted_group<T>(mx, mn, a, qmin, qmax);
    store_group(bs, p, from_f<T>(sg.s));
    store_group(bz, p, from_f<T>(sg.zp));  // exact: an integer of the code range
    store_group(btx, p, from_f<T>(mx));    // exact: values of T
    store_group(btn, p, from_f<T>(mn));
    return with_group_div<T>(sg.s, [&](const auto& div) {
      return group_fwd_chunk<T, true>(xv, div, sg.s, qmin, qmax, sg.zp);
    });
  }

  __device__ __forceinline__ Side side(const GroupPlace& p) const {
    return {load_group<T>(btx, p), load_group<T>(btn, p), load_group<T>(bgs, p), load_group<T>(bgz, p)};
  }
  __device__ __forceinline__ Vec bwd(const Vec& xv, const Vec& gv, const Side& sd, const GroupPlace& p) const {
    const float mx = to_f<T>(sd.mx), mn = to_f<T>(sd.mn), gsc = to_f<T>(sd.gscale), gzp = to_f<T>(sd.gzp);
    // the forward's scale and zero-point from the saved statistics: the same arithmetic, the saved bits
    const ShiftedGroup sg = shifted_group<T>(mx, mn, a, qmin, qmax);
    return with_group_div<T>(sg.s, [&](const auto& div) {
      return group_shifted_bwd_chunk<T, L>(a, xv, gv, p.sub, div, sg, mx, mn, gsc, gzp, qmin, qmax);
    });
  }
};

}  // namespace bvq

using namespace bvq;

extern "C" int bvq_group_shifted_supported(const bvq_quant_desc* d, const void* x) {
  if (group_check(d, "bvq_group_shifted_supported", true)) return 0;
  return x && aligned16(x) ? 1 : 0;
}

extern "C" int bvq_group_shifted_fwd(const bvq_quant_desc* d, const void* x, double min_val, int use_min,
                                     double thr_div, void* y, void* scale, void* zp, void* stat, bvq_stream_t stream) {
  const char* what = "bvq_group_shifted_fwd";
  int rc = group_required(what, group_check(d, what, true), {x, y, scale, zp, stat});
  if ((rc = group_aligned(what, rc, {x, y}, "x and y"))) return rc;
  GroupShiftedArgs a = group_args<GroupShiftedArgs>(d, min_val, use_min, thr_div);
  a.x = x;
  a.y = y;
  a.scale = scale;
  a.zp = zp;
  a.stat = stat;
  // x read + y written
  return group_launch(what, d->x_dtype, d->inner, a.chunks, 32, kGroupFwdDepth, [&](auto t, auto l, auto nt, unsigned grid) {
    group_fwd_kernel<ShiftedQuant, typename decltype(t)::type, l, nt><<<grid, kBlock, 0, (hipStream_t)stream>>>(a);
  });
}

extern "C" int bvq_group_shifted_bwd(const bvq_quant_desc* d, const void* g, const void* x, const void* stat,
                                     const void* gscale, const void* gzp, double min_val, int use_min, double thr_div,
                                     void* dx, bvq_stream_t stream) {
  const char* what = "bvq_group_shifted_bwd";
  int rc = group_required(what, group_check(d, what, true), {g, x, stat, dx});
  if ((rc = group_aligned(what, rc, {g, x, dx}, "g, x and dx"))) return rc;
  GroupShiftedArgs a = group_args<GroupShiftedArgs>(d, min_val, use_min, thr_div);
  a.x = x;
  a.g = g;
  a.y = dx;
  a.stat = const_cast<void*>(stat);
  a.gscale = gscale;
  a.gzp = gzp;
  // g and x read, dx written
  return group_launch(what, d->x_dtype, d->inner, a.chunks, 48, kGroupBwdDepth, [&](auto t, auto l, auto nt, unsigned grid) {
    group_bwd_kernel<ShiftedQuant, typename decltype(t)::type, l, nt><<<grid, kBlock, 0, (hipStream_t)stream>>>(a);
  });
}
