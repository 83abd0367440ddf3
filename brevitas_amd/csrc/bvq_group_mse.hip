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

#ifndef BVQ_GROUP_MSE_FWD_DEPTH
#define BVQ_GROUP_MSE_FWD_DEPTH 4  // wave loads of x in flight per wave
#endif
#ifndef BVQ_GROUP_MSE_BWD_DEPTH
#define BVQ_GROUP_MSE_BWD_DEPTH 2  // wave loads of x and of g in flight per wave
#endif
constexpr int kGroupMseFwdDepth = BVQ_GROUP_MSE_FWD_DEPTH;
constexpr int kGroupMseBwdDepth = BVQ_GROUP_MSE_BWD_DEPTH;
constexpr int kMseMaxRatios = 64;

struct GroupMseArgs {
  GroupArgs g;
  void* idx;  // [groups] uint8: fwd out, bwd in
  int32_t n;  // candidates, 1..kMseMaxRatios
  float ratio[kMseMaxRatios];
  int64_t chunks;  // = g.chunks (GroupWindow reads it here)
};

// one byte per group through the buffer descriptor (a vector store; dropped at kBufSkip and past the extent)
__device__ __forceinline__ void buf_store_u8(buf_t b, uint32_t byte_off, uint32_t v) {
  __builtin_amdgcn_raw_buffer_store_b8((unsigned char)v, b, byte_off, 0, 0);
}
__device__ __forceinline__ uint32_t buf_load_u8(buf_t b, uint32_t byte_off) {
  return __builtin_amdgcn_raw_buffer_load_b8(b, byte_off, 0, 0);
}

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

template <typename T, int L, bool NT>
__global__ __launch_bounds__(kBlock) void group_mse_fwd_kernel(GroupMseArgs m) {
  constexpr int VEC = elem<T>::vec, kD = kGroupMseFwdDepth;
  const GroupArgs& a = m.g;
  GroupWindow<T, L, kD> w;
  if (!w.init(m)) return;
  const int lane = threadIdx.x & 63;
  const buf_t bx = w.elems(a.x), by = w.elems(a.y), bs = w.groups(a.scale), bt = w.groups(a.stat);
  const buf_t bi = w.template groups<uint8_t>(m.idx);
  const float qmin = rnd<T>(a.qmin), qmax = rnd<T>(a.qmax);
  const bool use_min = a.use_min != 0;
  const int n = m.n;
  vec_t<T, VEC> xv[kD];
#pragma unroll
  for (int j = 0; j < kD; ++j) xv[j] = buf_load<T, VEC, NT>(bx, (uint32_t)(j * kWave + lane) * 16u);
#pragma unroll
  for (int j = 0; j < kD; ++j) {
    if ((uint32_t)(j * kWave) >= w.nch) break;  // wave-uniform: a load no lane has is not worked on
    const float stat = key_value<T>(seg_max_u32<L>(chunk_key<T>(xv[j])));
    // the search: first candidate with an error strictly below every earlier one.  A NaN error (a NaN or Inf group)
    // is below nothing and nothing is below it: such a group keeps candidate 0.
    float e_best = 0.f, s_best = 0.f;
    uint32_t k_best = 0;
    for (int i = 0; i < n; ++i) {  // wave-uniform count; m.ratio[i] is a scalar read
      const float s = group_scale<T>(mse_threshold<T>(stat, m.ratio[i]), use_min, a.min_val, a.thr_div);
      float e;
      if constexpr (sizeof(T) == 2) {
        if (wave_fast_div<T>(s))  // either division gives the same bits where both apply
          e = group_err_chunk<T>(xv[j], fast_div<T>(s), s, qmin, qmax);
        else
          e = group_err_chunk<T>(xv[j], DivExact{s}, s, qmin, qmax);
      } else {
        e = group_err_chunk<T>(xv[j], DivExact{s}, s, qmin, qmax);
      }
      e = seg_sum<L>(e);
      const bool better = i == 0 || e < e_best;
      e_best = better ? e : e_best;
      s_best = better ? s : s_best;
      k_best = better ? (uint32_t)i : k_best;
    }
    // one lane per segment writes the three small outputs (vector stores; dropped for the groups past the end)
    const bool head = (lane & (L - 1)) == 0;
    const uint32_t gi = (uint32_t)(j * (kWave / L) + lane / L);
    const uint32_t goff = head ? gi * (uint32_t)sizeof(T) : kBufSkip;
    vec_t<T, 1> sv, tv;
    sv.v[0] = from_f<T>(s_best);
    tv.v[0] = from_f<T>(stat);  // exact: stat is a value of T
    buf_store<T, 1>(bs, goff, sv);
    buf_store<T, 1>(bt, goff, tv);
    buf_store_u8(bi, head ? gi : kBufSkip, k_best);
    const uint32_t off = (uint32_t)(j * kWave + lane) * 16u;
    if constexpr (sizeof(T) == 2) {
      if (wave_fast_div<T>(s_best)) {
        group_fwd_chunk<T, NT>(xv[j], by, off, fast_div<T>(s_best), s_best, qmin, qmax);
        continue;
      }
    }
    group_fwd_chunk<T, NT>(xv[j], by, off, DivExact{s_best}, s_best, qmin, qmax);
  }
}

// group_quant_bwd_kernel with the scale derived from the chosen candidate's threshold and the statistic's gradient
// scaled by its ratio (group_bwd_chunk<.., kRatio = true>)
template <typename T, int L, bool NT>
__global__ __launch_bounds__(kBlock) void group_mse_bwd_kernel(GroupMseArgs m) {
  constexpr int VEC = elem<T>::vec, kD = kGroupMseBwdDepth;
  const GroupArgs& a = m.g;
  GroupWindow<T, L, kD> w;
  if (!w.init(m)) return;
  const int lane = threadIdx.x & 63;
  const buf_t bx = w.elems(a.x), bg = w.elems(a.g), bd = w.elems(a.y), bt = w.groups(a.stat);
  const buf_t bgs = w.groups(a.gscale ? a.gscale : a.stat);
  const buf_t bi = w.template groups<uint8_t>(m.idx);
  const float qmin = rnd<T>(a.qmin), qmax = rnd<T>(a.qmax);
  const int n = m.n;
  vec_t<T, VEC> xv[kD], gv[kD];
  vec_t<T, 1> tv[kD], gsv[kD];
  uint32_t kv[kD];
#pragma unroll
  for (int j = 0; j < kD; ++j) {
    const uint32_t off = (uint32_t)(j * kWave + lane) * 16u;
    const uint32_t gi = (uint32_t)(j * (kWave / L) + lane / L);  // one address per segment
    xv[j] = buf_load<T, VEC, NT>(bx, off);
    gv[j] = buf_load<T, VEC, NT>(bg, off);
    tv[j] = buf_load<T, 1>(bt, gi * (uint32_t)sizeof(T));
    gsv[j] = buf_load<T, 1>(bgs, gi * (uint32_t)sizeof(T));
    kv[j] = buf_load_u8(bi, gi);
  }
#pragma unroll
  for (int j = 0; j < kD; ++j) {
    if ((uint32_t)(j * kWave) >= w.nch) break;  // wave-uniform
    const uint32_t off = (uint32_t)(j * kWave + lane) * 16u;
    const float stat = to_f<T>(tv[j].v[0]);
    // the lane's ratio: a uniform walk over the table, one conditional move per candidate (an index the forward did
    // not write selects nothing and leaves ratio 0, which is 1)
    float ratio = m.ratio[0];
    for (int i = 1; i < n; ++i) ratio = kv[j] == (uint32_t)i ? m.ratio[i] : ratio;
    // the forward's scale from the saved statistic and index: the same arithmetic, the saved bits
    const float s = group_scale<T>(mse_threshold<T>(stat, ratio), a.use_min != 0, a.min_val, a.thr_div);
    const float gsc = to_f<T>(gsv[j].v[0]);
    if constexpr (sizeof(T) == 2) {
      if (wave_fast_div<T>(s)) {
        group_bwd_chunk<T, L, NT, true>(a, xv[j], gv[j], bd, off, lane, fast_div<T>(s), s, stat, gsc, qmin, qmax,
                                        ratio);
        continue;
      }
    }
    group_bwd_chunk<T, L, NT, true>(a, xv[j], gv[j], bd, off, lane, DivExact{s}, s, stat, gsc, qmin, qmax, ratio);
  }
}

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
  m.chunks = m.g.chunks;
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
  int rc = group_check(d, "bvq_group_mse_fwd");
  if (rc) return rc;
  if (!x || !ratios || !y || !scale || !stat || !idx) {
    set_error("bvq_group_mse_fwd: null pointer");
    return BVQ_ERR_INVALID;
  }
  if ((rc = mse_count_check(n_ratios, "bvq_group_mse_fwd"))) return rc;
  if (!aligned16(x) || !aligned16(y)) {
    set_error("bvq_group_mse_fwd: x and y must lie on 16-byte boundaries");
    return BVQ_ERR_UNSUPPORTED;
  }
  GroupMseArgs m = {};
  m.g = group_args(d, min_val, use_min, thr_div);
  if ((rc = mse_fill(m, ratios, n_ratios, "bvq_group_mse_fwd"))) return rc;
  m.g.x = x;
  m.g.y = y;
  m.g.scale = scale;
  m.g.stat = stat;
  m.idx = idx;
  const bool nt = m.chunks * 32 >= nt_threshold_bytes();  // x read + y written
  rc = with_group_variant(d, nt, [&](auto t, auto l, auto ntc) {
    group_mse_fwd_kernel<typename decltype(t)::type, l, ntc>
        <<<group_grid(m.chunks, kGroupMseFwdDepth), kBlock, 0, (hipStream_t)stream>>>(m);
  });
  return rc ? rc : check_launch("bvq_group_mse_fwd");
}

extern "C" int bvq_group_mse_bwd(const bvq_quant_desc* d, const void* g, const void* x, const void* stat,
                                 const void* idx, const void* gscale, const float* ratios, int n_ratios,
                                 double min_val, int use_min, double thr_div, void* dx, bvq_stream_t stream) {
  int rc = group_check(d, "bvq_group_mse_bwd");
  if (rc) return rc;
  if (!g || !x || !stat || !idx || !ratios || !dx) {
    set_error("bvq_group_mse_bwd: null pointer");
    return BVQ_ERR_INVALID;
  }
  if ((rc = mse_count_check(n_ratios, "bvq_group_mse_bwd"))) return rc;
  if (!aligned16(g) || !aligned16(x) || !aligned16(dx)) {
    set_error("bvq_group_mse_bwd: g, x and dx must lie on 16-byte boundaries");
    return BVQ_ERR_UNSUPPORTED;
  }
  GroupMseArgs m = {};
  m.g = group_args(d, min_val, use_min, thr_div);
  if ((rc = mse_fill(m, ratios, n_ratios, "bvq_group_mse_bwd"))) return rc;
  m.g.x = x;
  m.g.g = g;
  m.g.y = dx;
  m.g.stat = const_cast<void*>(stat);
  m.g.gscale = gscale;
  m.idx = const_cast<void*>(idx);
  const bool nt = m.chunks * 48 >= nt_threshold_bytes();  // g and x read, dx written
  rc = with_group_variant(d, nt, [&](auto t, auto l, auto ntc) {
    group_mse_bwd_kernel<typename decltype(t)::type, l, ntc>
        <<<group_grid(m.chunks, kGroupMseBwdDepth), kBlock, 0, (hipStream_t)stream>>>(m);
  });
  return rc ? rc : check_launch("bvq_group_mse_bwd");
}
