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

#ifndef BVQ_GROUP_FWD_DEPTH
#define BVQ_GROUP_FWD_DEPTH 4  // wave loads of x in flight per wave
#endif
#ifndef BVQ_GROUP_BWD_DEPTH
#define BVQ_GROUP_BWD_DEPTH 2  // wave loads of x and of g in flight per wave
#endif
constexpr int kGroupFwdDepth = BVQ_GROUP_FWD_DEPTH;
constexpr int kGroupBwdDepth = BVQ_GROUP_BWD_DEPTH;

template <typename T, int L, bool NT>
__global__ __launch_bounds__(kBlock) void group_quant_fwd_kernel(GroupArgs a) {
  constexpr int VEC = elem<T>::vec, kD = kGroupFwdDepth;
  GroupWindow<T, L, kD> w;
  if (!w.init(a)) return;
  const int lane = threadIdx.x & 63;
  const buf_t bx = w.elems(a.x), by = w.elems(a.y), bs = w.groups(a.scale), bt = w.groups(a.stat);
  const float qmin = rnd<T>(a.qmin), qmax = rnd<T>(a.qmax);
  vec_t<T, VEC> xv[kD];
#pragma unroll
  for (int j = 0; j < kD; ++j) xv[j] = buf_load<T, VEC, NT>(bx, (uint32_t)(j * kWave + lane) * 16u);
#pragma unroll
  for (int j = 0; j < kD; ++j) {
    if ((uint32_t)(j * kWave) >= w.nch) break;  // wave-uniform: a load no lane has is not worked on
    const float stat = key_value<T>(seg_max_u32<L>(chunk_key<T>(xv[j])));
    const float s = group_scale<T>(stat, a.use_min != 0, a.min_val, a.thr_div);
    // one lane per segment writes the two small outputs (vector stores; dropped for the groups past the end)
    const uint32_t goff = (lane & (L - 1)) == 0 ? (uint32_t)(j * (kWave / L) + lane / L) * (uint32_t)sizeof(T) : kBufSkip;
    vec_t<T, 1> sv, tv;
    sv.v[0] = from_f<T>(s);
    tv.v[0] = from_f<T>(stat);  // exact: stat is a value of T
    buf_store<T, 1>(bs, goff, sv);
    buf_store<T, 1>(bt, goff, tv);
    const uint32_t off = (uint32_t)(j * kWave + lane) * 16u;
    if constexpr (sizeof(T) == 2) {
      if (wave_fast_div<T>(s)) {
        group_fwd_chunk<T, NT>(xv[j], by, off, fast_div<T>(s), s, qmin, qmax);
        continue;
      }
    }
    group_fwd_chunk<T, NT>(xv[j], by, off, DivExact{s}, s, qmin, qmax);
  }
}

template <typename T, int L, bool NT>
__global__ __launch_bounds__(kBlock) void group_quant_bwd_kernel(GroupArgs a) {
  constexpr int VEC = elem<T>::vec, kD = kGroupBwdDepth;
  GroupWindow<T, L, kD> w;
  if (!w.init(a)) return;
  const int lane = threadIdx.x & 63;
  const buf_t bx = w.elems(a.x), bg = w.elems(a.g), bd = w.elems(a.y), bt = w.groups(a.stat);
  const buf_t bgs = w.groups(a.gscale ? a.gscale : a.stat);
  const float qmin = rnd<T>(a.qmin), qmax = rnd<T>(a.qmax);
  vec_t<T, VEC> xv[kD], gv[kD];
  vec_t<T, 1> tv[kD], gsv[kD];
#pragma unroll
  for (int j = 0; j < kD; ++j) {
    const uint32_t off = (uint32_t)(j * kWave + lane) * 16u;
    const uint32_t goff = (uint32_t)(j * (kWave / L) + lane / L) * (uint32_t)sizeof(T);  // one address per segment
    xv[j] = buf_load<T, VEC, NT>(bx, off);
    gv[j] = buf_load<T, VEC, NT>(bg, off);
    tv[j] = buf_load<T, 1>(bt, goff);
    gsv[j] = buf_load<T, 1>(bgs, goff);
  }
#pragma unroll
  for (int j = 0; j < kD; ++j) {
    if ((uint32_t)(j * kWave) >= w.nch) break;  // wave-uniform
    const uint32_t off = (uint32_t)(j * kWave + lane) * 16u;
    const float stat = to_f<T>(tv[j].v[0]);
    // the forward's scale from the saved statistic: the same arithmetic, the saved bits
    const float s = group_scale<T>(stat, a.use_min != 0, a.min_val, a.thr_div);
    const float gsc = to_f<T>(gsv[j].v[0]);
    if constexpr (sizeof(T) == 2) {
      if (wave_fast_div<T>(s)) {
        group_bwd_chunk<T, L, NT>(a, xv[j], gv[j], bd, off, lane, fast_div<T>(s), s, stat, gsc, qmin, qmax);
        continue;
      }
    }
    group_bwd_chunk<T, L, NT>(a, xv[j], gv[j], bd, off, lane, DivExact{s}, s, stat, gsc, qmin, qmax);
  }
}

}  // namespace bvq

using namespace bvq;

extern "C" int bvq_group_quant_supported(const bvq_quant_desc* d, const void* x) {
  if (group_check(d, "bvq_group_quant_supported")) return 0;
  return x && aligned16(x) ? 1 : 0;
}

extern "C" int bvq_group_quant_fwd(const bvq_quant_desc* d, const void* x, double min_val, int use_min, double thr_div,
                                   void* y, void* scale, void* stat, bvq_stream_t stream) {
  int rc = group_check(d, "bvq_group_quant_fwd");
  if (rc) return rc;
  if (!x || !y || !scale || !stat) {
    set_error("bvq_group_quant_fwd: null pointer");
    return BVQ_ERR_INVALID;
  }
  if (!aligned16(x) || !aligned16(y)) {
    set_error("bvq_group_quant_fwd: x and y must lie on 16-byte boundaries");
    return BVQ_ERR_UNSUPPORTED;
  }
  GroupArgs a = group_args(d, min_val, use_min, thr_div);
  a.x = x;
  a.y = y;
  a.scale = scale;
  a.stat = stat;
  const bool nt = a.chunks * 32 >= nt_threshold_bytes();  // x read + y written
  rc = with_group_variant(d, nt, [&](auto t, auto l, auto ntc) {
    group_quant_fwd_kernel<typename decltype(t)::type, l, ntc>
        <<<group_grid(a.chunks, kGroupFwdDepth), kBlock, 0, (hipStream_t)stream>>>(a);
  });
  return rc ? rc : check_launch("bvq_group_quant_fwd");
}

extern "C" int bvq_group_quant_bwd(const bvq_quant_desc* d, const void* g, const void* x, const void* scale,
                                   const void* stat, const void* gscale, double min_val, int use_min, double thr_div,
                                   void* dx, bvq_stream_t stream) {
  int rc = group_check(d, "bvq_group_quant_bwd");
  if (rc) return rc;
  if (!g || !x || !scale || !stat || !dx) {
    set_error("bvq_group_quant_bwd: null pointer");
    return BVQ_ERR_INVALID;
  }
  if (!aligned16(g) || !aligned16(x) || !aligned16(dx)) {
    set_error("bvq_group_quant_bwd: g, x and dx must lie on 16-byte boundaries");
    return BVQ_ERR_UNSUPPORTED;
  }
  GroupArgs a = group_args(d, min_val, use_min, thr_div);
  a.x = x;
  a.g = g;
  a.y = dx;
  a.stat = const_cast<void*>(stat);
  a.gscale = gscale;
  const bool nt = a.chunks * 48 >= nt_threshold_bytes();  // g and x read, dx written
  rc = with_group_variant(d, nt, [&](auto t, auto l, auto ntc) {
    group_quant_bwd_kernel<typename decltype(t)::type, l, ntc>
        <<<group_grid(a.chunks, kGroupBwdDepth), kBlock, 0, (hipStream_t)stream>>>(a);
  });
  return rc ? rc : check_launch("bvq_group_quant_bwd");
}
