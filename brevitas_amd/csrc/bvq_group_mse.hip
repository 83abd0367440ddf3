// bvq_group_mse.hip -- group-wise weight quantizer with a per-group search of the clipping threshold: of n candidate
// thresholds t_i = abs-max * ratio_i (ratio_0 = 1) the group takes the first one with the smallest squared
// quantization error, one launch each way.
//
// The walk is that of bvq_group_quant.hip (bvq_group_walk.h): a group of g elements lives in L adjacent lanes of one
// wave load, so the whole search runs on the registers that hold the chunk.  x is read once; per candidate every lane
// quantizes its 16 bytes with the forward chain of the plain quantizer (group_fwd_pair, rounded to T as the stored y
// would be), squares the float32 difference from x and the group's error is a segmented butterfly; the best
// (error, index, scale) so far stays in three registers; y is written once, with the winning scale.  No LDS, no
// workspace, no atomics, no second launch.
//   forward   reads x, writes y                (+ 2 * bytes(x) / g for scale and stat, + one index byte per group)
//   backward  reads g and x, writes dx once    (+ bytes(x) / g for stat, + the index byte; gscale when given)
// The candidate loop runs n times for the whole wave (n is a kernel argument) and ratio[i] is a scalar read of the
// argument struct.  The backward's ratio belongs to a per-lane index: it is selected by the same uniform loop with
// one conditional move per candidate, never by indexing the table with the lane's value.
// With ratios = {1} both kernels compute the bits of bvq_group_quant_fwd / bvq_group_quant_bwd.
#include "bvq_group_quant.h"

namespace bvq {

constexpr int kMseMaxRatios = 64;

struct GroupMseArgs : GroupArgs {
  void* idx;  // [groups] uint8: fwd out, bwd in
  int32_t n;  // candidates, 1..kMseMaxRatios
  float ratio[kMseMaxRatios];
};

// a candidate's threshold: the statistic (a value of T) times the float32 ratio, formed in float32, rounded once to T
template <typename T>
__device__ __forceinline__ float mse_threshold(float stat, float ratio) {
  return rnd<T>(stat * ratio);
}

// this lane's part of a candidate's error: sum over its chunk of (float32(y) - float32(x))^2, y the value of T that the
// forward would store for the scale s
template <typename T, typename Div>
__device__ __forceinline__ float group_err_chunk(const vec_t<T, elem<T>::vec>& xv, const Div& div, float s, float qmin,
                                                 float qmax) {
  constexpr int VEC = elem<T>::vec;
  f2 acc = splat2(0.f);
#pragma unroll
  for (int k = 0; k < VEC; k += 2) {
    const f2 xf = widen2<T>(xv.v[k], xv.v[k + 1]);
    const f2 d = rnd2<T>(group_fwd_pair<T>(xf, div, s, qmin, qmax)) - xf;
    acc += d * d;
  }
  return acc.x + acc.y;
}

// the clip-search quantizer on the frame of bvq_group_walk.h
template <typename T, int L>
struct MseQuant {
  using Args = GroupMseArgs;
  using Vec = vec_t<T, elem<T>::vec>;
  struct Side {
    T stat, gscale;
    uint32_t k;
  };
  const Args& a;
  const buf_t bs, bt, bgs, bi;
  const float qmin, qmax;
  template <typename W>
  __device__ __forceinline__ MseQuant(const Args& a, const W& w)
      : a(a), bs(w.groups(a.scale)), bt(w.groups(a.stat)), bgs(w.groups_or_zeros(a.gscale, a.x)),
        bi(w.template groups<uint8_t>(a.idx)), qmin(rnd<T>(a.qmin)), qmax(rnd<T>(a.qmax)) {}

  __device__ __forceinline__ Vec fwd(const Vec& xv, const GroupPlace& p) const {
    const bool use_min = a.use_min != 0;
    const int n = a.n;
    const float stat = key_value<T>(seg_max_u32<L>(chunk_key<T>(xv)));
    // the search: first candidate with an error strictly below every earlier one.  A NaN error (a NaN or Inf group)
    // is below nothing and nothing is below it: such a group keeps candidate 0.
    float e_best = 0.f, s_best = 0.f;
    uint32_t k_best = 0;
    for (int i = 0; i < n; ++i) {  // wave-uniform count; a.ratio[i] is a scalar read
      const float s = group_scale<T>(mse_threshold<T>(stat, a.ratio[i]), use_min, a.min_val, a.thr_div);
      const float e = seg_sum<L>(
          with_group_div<T>(s, [&](const auto& div) { return group_err_chunk<T>(xv, div, s, qmin, qmax); }));
      const bool better = i == 0 || e < e_best;
      e_best = better ? e : e_best;
      s_best = better ? s : s_best;
      k_best = better ? (uint32_t)i : k_best;
    }
    store_group(bs, p, from_f<T>(s_best));
    store_group(bt, p, from_f<T>(stat));  // exact: stat is a value of T
    buf_store_u8(bi, p.head_at(1), k_best);
    return with_group_div<T>(s_best, [&](const auto& div) { return group_fwd_chunk<T>(xv, div, s_best, qmin, qmax); });
  }

  __device__ __forceinline__ Side side(const GroupPlace& p) const {
    return {load_group<T>(bt, p), load_group<T>(bgs, p), buf_load_u8(bi, p.at(1))};
  }
  // PlainQuant::bwd with the scale derived from the chosen candidate's threshold and the statistic's gradient scaled
  // by its ratio (group_bwd_chunk<.., kRatio = true>)
  __device__ __forceinline__ Vec bwd(const Vec& xv, const Vec& gv, const Side& sd, const GroupPlace& p) const {
    const int n = a.n;
    const float stat = to_f<T>(sd.stat), gsc = to_f<T>(sd.gscale);
    // the lane's ratio: a uniform walk over the table, one conditional move per candidate (an index the forward did
    // not write selects nothing and leaves ratio 0, which is 1)
    float ratio = a.ratio[0];
    for (int i = 1; i < n; ++i) ratio = sd.k == (uint32_t)i ? a.ratio[i] : ratio;
    // the forward's scale from the saved statistic and index: the same arithmetic, the saved bits
    const float s = group_scale<T>(mse_threshold<T>(stat, ratio), a.use_min != 0, a.min_val, a.thr_div);
    return with_group_div<T>(s, [&](const auto& div) {
      return group_bwd_chunk<T, L, true>(a, xv, gv, p.sub, div, s, stat, gsc, qmin, qmax, ratio);
    });
  }
};

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
static int mse_count_check(int n_ratios, const char* what) {
  if (n_ratios < 1 || n_ratios > kMseMaxRatios) {
    set_error("%s: %d candidate ratios (1 to %d)", what, n_ratios, kMseMaxRatios);
    return BVQ_ERR_UNSUPPORTED;
  }
  return BVQ_OK;
}

// the candidate table into the argument struct: ratios[0] is 1, every ratio finite and in (0, 1]
static int mse_fill(GroupMseArgs& m, const float* ratios, int n_ratios, const char* what) {
  for (int i = 0; i < n_ratios; ++i) {
    const float r = ratios[i];
    if (!(r > 0.f && r <= 1.f)) {  // a NaN fails both comparisons
      set_error("%s: ratio %d is %g (finite, in (0, 1])", what, i, (double)r);
      return BVQ_ERR_UNSUPPORTED;
    }
    m.ratio[i] = r;
  }
  if (ratios[0] != 1.f) {
    set_error("%s: ratio 0 is %g (the abs-max itself is always the first candidate: 1)", what, (double)ratios[0]);
    return BVQ_ERR_UNSUPPORTED;
  }
  m.n = n_ratios;
  return BVQ_OK;
}

}  // namespace bvq

using namespace bvq;

extern "C" int bvq_group_mse_supported(const bvq_quant_desc* d, const void* x, int n_ratios) {
  if (group_check(d, "bvq_group_mse_supported")) return 0;
  if (mse_count_check(n_ratios, "bvq_group_mse_supported")) return 0;
  return x && aligned16(x) ? 1 : 0;
}

extern "C" int bvq_group_mse_fwd(const bvq_quant_desc* d, const void* x, const float* ratios, int n_ratios,
                                 double min_val, int use_min, double thr_div, void* y, void* scale, void* stat,
                                 void* idx, bvq_stream_t stream) {
  const char* what = "bvq_group_mse_fwd";
  int rc = group_required(what, group_check(d, what), {x, ratios, y, scale, stat, idx});
  if (!rc) rc = mse_count_check(n_ratios, what);
  if ((rc = group_aligned(what, rc, {x, y}, "x and y"))) return rc;
  GroupMseArgs m = group_args<GroupMseArgs>(d, min_val, use_min, thr_div);
  if ((rc = mse_fill(m, ratios, n_ratios, what))) return rc;
  m.x = x;
  m.y = y;
  m.scale = scale;
  m.stat = stat;
  m.idx = idx;
  // x read + y written
  return group_launch(what, d->x_dtype, d->inner, m.chunks, 32, kGroupFwdDepth, [&](auto t, auto l, auto nt, unsigned grid) {
    group_fwd_kernel<MseQuant, typename decltype(t)::type, l, nt><<<grid, kBlock, 0, (hipStream_t)stream>>>(m);
  });
}

extern "C" int bvq_group_mse_bwd(const bvq_quant_desc* d, const void* g, const void* x, const void* stat,
                                 const void* idx, const void* gscale, const float* ratios, int n_ratios,
                                 double min_val, int use_min, double thr_div, void* dx, bvq_stream_t stream) {
  const char* what = "bvq_group_mse_bwd";
  int rc = group_required(what, group_check(d, what), {g, x, stat, idx, ratios, dx});
  if (!rc) rc = mse_count_check(n_ratios, what);
  if ((rc = group_aligned(what, rc, {g, x, dx}, "g, x and dx"))) return rc;
  GroupMseArgs m = group_args<GroupMseArgs>(d, min_val, use_min, thr_div);
  if ((rc = mse_fill(m, ratios, n_ratios, what))) return rc;
  m.x = x;
  m.g = g;
  m.y = dx;
  m.stat = const_cast<void*>(stat);
  m.gscale = gscale;
  m.idx = const_cast<void*>(idx);
  // g and x read, dx written
  return group_launch(what, d->x_dtype, d->inner, m.chunks, 48, kGroupBwdDepth, [&](auto t, auto l, auto nt, unsigned grid) {
    group_bwd_kernel<MseQuant, typename decltype(t)::type, l, nt><<<grid, kBlock, 0, (hipStream_t)stream>>>(m);
  });
}
