// bvq_group_quant.hip -- group-wise weight quantizer: one scale per `group_size` consecutive elements, statistic,
// scale, quantization, scale gradient and arg-max deposit inside registers, one launch each way.
//
// The tensor is walked as a flat stream of 16-byte lane accesses.  A group of g elements occupies
// L = g * sizeof(T) / 16 ADJACENT lanes of one wave load (2..32 lanes for 16-bit types, 4..64 for float32), and 64 / L
// groups share a load; L divides 64, so a group never straddles two loads.  Everything a group needs from its other
// elements -- the abs-max, the two sums of the scale gradient, the first element attaining the abs-max -- is a
// SEGMENTED butterfly over those L lanes (__shfl_xor with offsets L/2 .. 1: every lane of the segment ends with the
// same bits, in a fixed order).  No LDS, no atomics, no partials, no workspace, no second launch.
//   forward   reads x, writes y                (+ 2 * bytes(x) / g for scale and stat)
//   backward  reads g and x, writes dx once    (+ bytes(x) / g for stat)
// Results are the bits of the per-channel kernels on the tensor regrouped as [groups, g] (bvq_stats_fakequant_fwd,
// bvq_fakequant_bwd_stats); only the ORDER in which a group's float32 scale-gradient terms are added differs, which
// can move the deposited element by a rounding.
#include "bvq_group_quant.h"  // the argument struct, the chunk bodies and the coverage check

namespace bvq {

// the plain quantizer on the frame of bvq_group_walk.h: abs-max statistic, one scale per group
template <typename T, int L>
struct PlainQuant {
  using Args = GroupArgs;
  using Vec = vec_t<T, elem<T>::vec>;
  struct Side {
    T stat, gscale;
  };
  const Args& a;
  const buf_t bs, bt, bgs;
  const float qmin, qmax;
  template <typename W>
  __device__ __forceinline__ PlainQuant(const Args& a, const W& w)
      : a(a), bs(w.groups(a.scale)), bt(w.groups(a.stat)), bgs(w.groups_or_zeros(a.gscale, a.x)),
        qmin(rnd<T>(a.qmin)), qmax(rnd<T>(a.qmax)) {}

  __device__ __forceinline__ Vec fwd(const Vec& xv, const GroupPlace& p) const {
    const float stat = key_value<T>(seg_max_u32<L>(chunk_key<T>(xv)));
    const float s = group_scale<T>(stat, a.use_min != 0, a.min_val, a.thr_div);
    store_group(bs, p, from_f<T>(s));
    store_group(bt, p, from_f<T>(stat));  // exact: stat is a value of T
    return with_group_div<T>(s, [&](const auto& div) { return group_fwd_chunk<T>(xv, div, s, qmin, qmax); });
  }

  __device__ __forceinline__ Side side(const GroupPlace& p) const {
    return {load_group<T>(bt, p), load_group<T>(bgs, p)};
  }
  __device__ __forceinline__ Vec bwd(const Vec& xv, const Vec& gv, const Side& sd, const GroupPlace& p) const {
    const float stat = to_f<T>(sd.stat), gsc = to_f<T>(sd.gscale);
    // the forward's scale from the saved statistic: the same arithmetic, the saved bits
    const float s = group_scale<T>(stat, a.use_min != 0, a.min_val, a.thr_div);
    return with_group_div<T>(s, [&](const auto& div) {
      return group_bwd_chunk<T, L>(a, xv, gv, p.sub, div, s, stat, gsc, qmin, qmax);
    });
  }
};

}  // namespace bvq

using namespace bvq;

extern "C" int bvq_group_quant_supported(const bvq_quant_desc* d, const void* x) {
  if (group_check(d, "bvq_group_quant_supported")) return 0;
  return x && aligned16(x) ? 1 : 0;
}

extern "C" int bvq_group_quant_fwd(const bvq_quant_desc* d, const void* x, double min_val, int use_min, double thr_div,
                                   void* y, void* scale, void* stat, bvq_stream_t stream) {
  const char* what = "bvq_group_quant_fwd";
  int rc = group_required(what, group_check(d, what), {x, y, scale, stat});
  if ((rc = group_aligned(what, rc, {x, y}, "x and y"))) return rc;
  GroupArgs a = group_args(d, min_val, use_min, thr_div);
  a.x = x;
  a.y = y;
  a.scale = scale;
  a.stat = stat;
  // x read + y written
  return group_launch(what, d->x_dtype, d->inner, a.chunks, 32, kGroupFwdDepth, [&](auto t, auto l, auto nt, unsigned grid) {
    group_fwd_kernel<PlainQuant, typename decltype(t)::type, l, nt><<<grid, kBlock, 0, (hipStream_t)stream>>>(a);
  });
}

extern "C" int bvq_group_quant_bwd(const bvq_quant_desc* d, const void* g, const void* x, const void* scale,
                                   const void* stat, const void* gscale, double min_val, int use_min, double thr_div,
                                   void* dx, bvq_stream_t stream) {
  const char* what = "bvq_group_quant_bwd";
  int rc = group_required(what, group_check(d, what), {g, x, scale, stat, dx});
  if ((rc = group_aligned(what, rc, {g, x, dx}, "g, x and dx"))) return rc;
  GroupArgs a = group_args(d, min_val, use_min, thr_div);
  a.x = x;
  a.g = g;
  a.y = dx;
  a.stat = const_cast<void*>(stat);
  a.gscale = gscale;
  // g and x read, dx written
  return group_launch(what, d->x_dtype, d->inner, a.chunks, 48, kGroupBwdDepth, [&](auto t, auto l, auto nt, unsigned grid) {
    group_bwd_kernel<PlainQuant, typename decltype(t)::type, l, nt><<<grid, kBlock, 0, (hipStream_t)stream>>>(a);
  });
}
