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
#include "bvq_group_shifted.h"  // the argument struct, the forward chain of a chunk, statistics -> scale and zero-point

namespace bvq {

// GroupArgs with `stat` holding [2 * groups] values, the maxima then the minima (as BVQ_STAT_MINMAX)
struct GroupShiftedArgs : GroupArgs {
  void* zp;         // fwd: [groups] out
  const void* gzp;  // bwd, nullable: gradient arriving through the returned zero-point, [groups]
};

// One chunk of the backward: dx and the rounded gradient terms of scale and zero-point per element exactly as the
// per-channel backward computes them (bwd_elem2, kBwdDsDzp), the group's two sums, then the autograd of the scale-shaped
// torch ops of the graph, each rounding to T:
//   zero-point   dzp (+ gzp) -> its own clamp (masked where it clipped unless straight-through) -> round (STE) -> "+ 0"
//                -> u = n / s: dn = dzp / s to n = -m0, -dzp * ((n / s) / s) to the scale -> m0 -> mn where mn <= 0
//   scale        ds (+ gscale) + the zero-point's share -> / thr_div -> clamp_min (STE) -> |d|: * sgn(d) -> d = mx - mn
// and the deposits in the order the per-channel route adds its dense gradients to dx: the zero-point statistic's first
// (on the first element equal to mn), then the scale statistic's (max and min, added to each other first where one
// element is both).  Every element of dx has been through "+ 0" there, which turns a -0 into +0.
// sub: the lane within its segment (GroupPlace).
template <typename T, int L, typename Div>
__device__ __forceinline__ vec_t<T, elem<T>::vec> group_shifted_bwd_chunk(
    const GroupShiftedArgs& a, const vec_t<T, elem<T>::vec>& xv, const vec_t<T, elem<T>::vec>& gv, uint32_t sub,
    const Div& div, const ShiftedGroup& p, float mx, float mn, float gsc, float gzp, float qmin, float qmax) {
  constexpr int VEC = elem<T>::vec;
  const bool clamp_ste = a.clamp_ste != 0;
  f2 ds2 = splat2(0.f), dz2 = splat2(0.f), unused = splat2(0.f);
  vec_t<T, VEC> dv;
#pragma unroll
  for (int k = 0; k < VEC; k += 2) {
    const f2 d = bwd_elem2<T, BVQ_ROUND, kBwdDsDzp, false, false, true>(
        widen2<T>(xv.v[k], xv.v[k + 1]), widen2<T>(gv.v[k], gv.v[k + 1]), div, p.s, p.zp, qmin, qmax, clamp_ste,
        BVQ_ROUND, ds2, dz2, unused);
    pack2<T>(f2{plus_zero(d.x), plus_zero(d.y)}, dv.v[k], dv.v[k + 1]);  // (d is rounded to T: the conversion is exact)
  }
  const float ds = seg_sum<L>(ds2.x + ds2.y);
  const float dzs = seg_sum<L>(dz2.x + dz2.y);
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
  const float dmn_z = mn <= 0.f ? -dn : 0.f;
  // first element of the group equal to each statistic: segment-wide minimum over lane * VEC + index (a NaN statistic
  // is equal to nothing)
  const uint32_t e0 = sub * VEC;
  uint32_t fmx = ~0u, fmn = ~0u;
#pragma unroll
  for (int k = VEC - 1; k >= 0; --k) {
    const float xf = to_f<T>(xv.v[k]);
    fmx = xf == mx ? e0 + k : fmx;
    fmn = xf == mn ? e0 + k : fmn;
  }
  fmx = seg_min_u32<L>(fmx);
  fmn = seg_min_u32<L>(fmn);
#pragma unroll
  for (int k = 0; k < VEC; ++k) {
    const bool is_mx = fmx == e0 + k, is_mn = fmn == e0 + k;
    float val = to_f<T>(dv.v[k]);
    val = is_mn ? rnd<T>(val + dmn_z) : val;
    float dep = is_mx ? dd : 0.f;
    dep = is_mn ? rnd<T>(dep - dd) : dep;
    dv.v[k] = (is_mx || is_mn) ? from_f<T>(val + dep) : dv.v[k];
  }
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
