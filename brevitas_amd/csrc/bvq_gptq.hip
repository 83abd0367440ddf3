// bvq_gptq.hip -- the column loop of GPTQ weight quantization for one block of up to 128 input columns, one launch.
//
// GPTQ quantizes a weight [R, K] one input column at a time and pushes each column's error onto the columns not yet
// quantized, through the upper Cholesky factor U of the damped inverse Hessian (include/bvq.h, "GPTQ").  Rows are
// independent in that loop and a block of a row fits in registers: ONE WAVE PER ROW, lane l holding columns l and
// l + 64 of the block's float32 working copy.  In step i the owner's value is broadcast with a read-lane, every lane
// computes the same code and error, loads its two values of U[i, .] (coalesced) and updates the columns it holds that
// lie right of i.  Where scale and zero-point are computed in the loop, a group start is a segmented butterfly over the
// group's lanes (bvq_group_walk.h), with the statistic -> scale and zero-point chains of the group-wise quantizers
// (bvq_group_quant.h, bvq_group_shifted.h) and their forward chain for the code.  No LDS, no atomics, no workspace.
//   reads   the block's columns of Wf, the [B, B] triangle of U (+ scale / zero-point where they are given)
//   writes  the block's columns of Q, E [R, B] float32 (+ the block's scale / zero-point where they are computed)
#include "bvq_column_loop.h"  // the block width, read_lane and the host-side check, shared with bvq_gpfq.hip

namespace bvq {

// GroupArgs: x = Wf (float32 [rows, cols]), y = Q (T [rows, cols]), scale = [rows, cols / gsize] of T
struct GptqArgs : GroupArgs {
  const float* u;  // [cols, cols]
  float* err;      // [rows, bc]
  void* zp;        // [rows, cols / gsize] of T, asymmetric only
  int64_t rows, cols, col0;
  int32_t bc, gsize;
};

// one element as a whole chunk of itself: the chunk statistics of the group walk then give the element's own key
template <typename T>
__device__ __forceinline__ vec_t<T, elem<T>::vec> chunk_of(float w) {
  vec_t<T, elem<T>::vec> c;
#pragma unroll
  for (int k = 0; k < elem<T>::vec; ++k) c.v[k] = from_f<T>(w);
  return c;
}

// scale and zero-point of the group that the lane's element of the selected register half belongs to, from the values
// as they stand: every lane of the group's segment ends with the same bits.  G = 128: both halves are one group.
template <typename T, bool kZp, int G>
__device__ __forceinline__ void gptq_group_params(const GptqArgs& a, float w0, float w1, bool hi, float qmin,
                                                  float qmax, float& s, float& zp) {
  constexpr int L = G == 128 ? 64 : G;
  const float wsel = hi ? w1 : w0;
  if constexpr (kZp) {
    uint32_t kmax, kmin;
    if constexpr (G == 128) {
      uint32_t kmax1, kmin1;
      chunk_minmax_keys<T>(chunk_of<T>(w0), kmax, kmin);
      chunk_minmax_keys<T>(chunk_of<T>(w1), kmax1, kmin1);
      kmax = kmax1 > kmax ? kmax1 : kmax;
      kmin = kmin1 < kmin ? kmin1 : kmin;
    } else {
      chunk_minmax_keys<T>(chunk_of<T>(wsel), kmax, kmin);
    }
    float mx, mn;
    shifted_stats<T>(seg_max_u32<L>(kmax), seg_min_u32<L>(kmin), mx, mn);
    const ShiftedGroup sg = shifted_group<T>(mx, mn, a, qmin, qmax);
    s = sg.s;
    zp = sg.zp;
  } else {
    uint32_t key;
    if constexpr (G == 128) {
      const uint32_t k0 = chunk_key<T>(chunk_of<T>(w0)), k1 = chunk_key<T>(chunk_of<T>(w1));
      key = k1 > k0 ? k1 : k0;
    } else {
      key = chunk_key<T>(chunk_of<T>(wsel));
    }
    const float stat = key_value<T>(seg_max_u32<L>(key));
    s = group_scale<T>(stat, a.use_min != 0, a.min_val, a.thr_div);
    zp = 0.f;
  }
}

// G: the group size whose scale (and zero-point) the loop computes at each group start, or 0: they are given
template <typename T, bool kZp, int G>
__global__ __launch_bounds__(kBlock) void gptq_block_kernel(GptqArgs a) {
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t r = (int64_t)blockIdx.x * kWavesPerBlock + wave;
  if (r >= a.rows) return;  // wave-uniform
  const int lane = threadIdx.x & 63;
  const int bc = a.bc;
  const bool in0 = lane < bc, in1 = lane + 64 < bc;
  const float* wrow = reinterpret_cast<const float*>(a.x) + r * a.cols + a.col0;
  const float* ub = a.u + a.col0 * a.cols + a.col0;  // U[col0, col0]
  float w0 = in0 ? wrow[lane] : 0.f, w1 = in1 ? wrow[lane + 64] : 0.f;
  const float qmin = rnd<T>(a.qmin), qmax = rnd<T>(a.qmax);
  const int64_t gpr = a.cols / a.gsize;  // groups per row
  T* const srow = reinterpret_cast<T*>(a.scale) + r * gpr;
  T* const zrow = kZp ? reinterpret_cast<T*>(a.zp) + r * gpr : nullptr;

  float s0 = 0.f, s1 = 0.f, z0 = 0.f, z1 = 0.f;  // given: the lane's own columns'
  if constexpr (G == 0) {
    const int64_t g0 = (a.col0 + lane) / a.gsize, g1 = (a.col0 + lane + 64) / a.gsize;
    s0 = in0 ? to_f<T>(srow[g0]) : 0.f;
    s1 = in1 ? to_f<T>(srow[g1]) : 0.f;
    if constexpr (kZp) {
      z0 = in0 ? to_f<T>(zrow[g0]) : 0.f;
      z1 = in1 ? to_f<T>(zrow[g1]) : 0.f;
    }
  }

  float s = 0.f, zp = 0.f, q0 = 0.f, q1 = 0.f, e0 = 0.f, e1 = 0.f;
  // the division by s that the wave takes (bvq_group_quant.h) and its reciprocal, kept from one change of s to the next
  bool fast = false;
  float rs = 0.f;
  int64_t togo = 0;  // given: steps until the next group's scale and zero-point apply
  // row i of the triangle, one step ahead of its use
  float u0 = in0 ? ub[lane] : 0.f, u1 = in1 ? ub[lane + 64] : 0.f, d = ub[0];
  for (int i = 0; i < bc; ++i) {
    const float cu0 = u0, cu1 = u1, cd = d;
    if (i + 1 < bc) {  // wave-uniform
      const float* un = ub + (int64_t)(i + 1) * a.cols;
      u0 = in0 ? un[lane] : 0.f;
      u1 = in1 ? un[lane + 64] : 0.f;
      d = un[i + 1];
    }
    const int src = i & 63;
    const bool hi = i >= 64;
    bool fresh = false;
    if constexpr (G != 0) {
      if ((i & (G - 1)) == 0) {  // group start, wave-uniform
        fresh = true;
        float sg, zg;
        gptq_group_params<T, kZp, G>(a, w0, w1, hi, qmin, qmax, sg, zg);
        s = read_lane(sg, src);
        zp = read_lane(zg, src);
        if (lane == 0) {
          const int64_t grp = (a.col0 + i) / G;
          srow[grp] = from_f<T>(s);
          if constexpr (kZp) zrow[grp] = from_f<T>(zp);  // exact: an integer of the code range
        }
      }
    } else {
      if (togo == 0) {  // wave-uniform
        fresh = true;
        togo = a.gsize - (a.col0 + i) % a.gsize;
        s = read_lane(hi ? s1 : s0, src);
        if constexpr (kZp) zp = read_lane(hi ? z1 : z0, src);
      }
      --togo;
    }
    if constexpr (sizeof(T) == 2) {
      if (fresh) {
        fast = wave_fast_div<T>(s);
        rs = 1.0f / s;
      }
    }
    const float wi = read_lane(hi ? w1 : w0, src);
    const f2 xt = splat2(rnd<T>(wi));
    f2 y;
    if (sizeof(T) == 2 && fast)
      y = group_fwd_pair<T, kZp>(xt, fast_div<T>(s, rs), s, qmin, qmax, zp);
    else
      y = group_fwd_pair<T, kZp>(xt, DivExact{s}, s, qmin, qmax, zp);
    T qa, qb;
    pack2<T>(y, qa, qb);
    const float q = to_f<T>(qa);
    const float e = (wi - q) / cd;  // IEEE division
    const bool own = lane == src;
    q0 = (own && !hi) ? q : q0;
    e0 = (own && !hi) ? e : e0;
    q1 = (own && hi) ? q : q1;
    e1 = (own && hi) ? e : e1;
    // the columns right of i: product rounded, then the difference rounded (no fused multiply-add)
    const float n0 = __fsub_rn(w0, __fmul_rn(e, cu0)), n1 = __fsub_rn(w1, __fmul_rn(e, cu1));
    w0 = (!hi && lane > src) ? n0 : w0;
    w1 = (!hi || lane > src) ? n1 : w1;
  }

  T* qrow = reinterpret_cast<T*>(a.y) + r * a.cols + a.col0;
  float* erow = a.err + r * bc;
  if (in0) {
    qrow[lane] = from_f<T>(q0);
    erow[lane] = e0;
  }
  if (in1) {
    qrow[lane + 64] = from_f<T>(q1);
    erow[lane + 64] = e1;
  }
}

}  // namespace bvq

using namespace bvq;

extern "C" int bvq_gptq_block_supported(const bvq_quant_desc* d, int64_t rows, int64_t cols, int64_t col0,
                                        int block_cols, int computed, const void* wf, const void* u, const void* q) {
  if (column_block_check(d, "bvq_gptq_block_supported", rows, cols, col0, block_cols, computed)) return 0;
  return wf && u && q && aligned16(wf) && aligned16(u) && aligned16(q) ? 1 : 0;
}

extern "C" int bvq_gptq_block(const bvq_quant_desc* d, const float* wf, const float* u, int64_t rows, int64_t cols,
                              int64_t col0, int block_cols, int computed, double min_val, int use_min, double thr_div,
                              void* q, float* err, void* scale, void* zp, bvq_stream_t stream) {
  const char* what = "bvq_gptq_block";
  int rc = column_block_check(d, what, rows, cols, col0, block_cols, computed);
  const bool shifted = !rc && d->zp_per_channel;
  rc = group_required(what, rc, {wf, u, q, err, scale});
  if (!rc && shifted && !zp) {
    set_error("%s: null pointer (zp of an asymmetric quantizer)", what);
    return BVQ_ERR_INVALID;
  }
  if ((rc = group_aligned(what, rc, {wf, u, q, err}, "wf, u, q and err"))) return rc;
  GptqArgs a = group_args<GptqArgs>(d, min_val, use_min, thr_div);
  a.x = wf;
  a.y = q;
  a.scale = scale;
  a.u = u;
  a.err = err;
  a.zp = zp;
  a.rows = rows;
  a.cols = cols;
  a.col0 = col0;
  a.bc = block_cols;
  a.gsize = (int32_t)d->inner;
  const unsigned grid = (unsigned)((rows + kWavesPerBlock - 1) / kWavesPerBlock);
  const int g = computed ? (int)d->inner : 0;
  rc = with_dtype(d->x_dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    return with_bool(shifted, [&](auto z) {
      return with_value<0, 16, 32, 64, 128>(g, [&](auto gc) {
        gptq_block_kernel<T, decltype(z)::value, decltype(gc)::value><<<grid, kBlock, 0, (hipStream_t)stream>>>(a);
      });
    });
  });
  return rc ? rc : check_launch(what);
}
