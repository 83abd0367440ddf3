// bvq_column_loop.h -- the column loop of one block of up to 128 input columns, the frame of bvq_gptq.hip and
// bvq_gpfq.hip: ONE WAVE PER ROW, the block of the row in registers, lane l holding columns l and l + 64.  In step i the
// owner's values are broadcast with a read-lane, every lane computes the same code and error, loads its two values of
// row i of a [K, K] matrix (coalesced, one step ahead) and updates the running state of the columns it holds that lie
// right of i.  Scale and zero-point are given, for groups of any size, or computed at each group start by a segmented
// butterfly over the group's lanes (bvq_group_walk.h) with the statistic -> scale and zero-point chains of the
// group-wise quantizers (bvq_group_quant.h, bvq_group_shifted.h).  No LDS, no atomics, no workspace.
//
// An algorithm is a Rule, a struct of compile-time statements and nothing else:
//   kCorrection           what the running state r of a lane is: the working weight itself (false), or a correction
//                         beside the weight, which is then held read-only in two more registers (true)
//   value(wi, ri, cd)     what is quantized in step i, from the owner's weight, its running state and the diagonal
//   error(wi, q, cd)      the error of step i
//   update(r, p)          the running state right of i, from the rounded product p = e * M[i, .]
// The host side: the coverage check of descriptor, shape and block, and the one launcher of both entries.
#pragma once

#include "bvq_group_shifted.h"

namespace bvq {

constexpr int kColumnBlock = 128;  // columns of a block: two per lane

// GroupArgs: x = Wf (float32 [rows, cols]), y = Q (T [rows, cols]), scale = [rows, cols / gsize] of T
struct ColumnArgs : GroupArgs {
  const float* u;  // [cols, cols]: the matrix whose row i spreads the error of step i (GPTQ: U, GPFQ: H)
  const float* c;  // [rows, cols]: the running correction where the rule has one, else null
  float* err;      // [rows, bc]
  void* zp;        // [rows, cols / gsize] of T, asymmetric only; written where it is computed in the loop
  int64_t rows, cols, col0;
  int32_t bc, gsize;
};

__device__ __forceinline__ float read_lane(float v, int lane) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}

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
__device__ __forceinline__ void column_group_params(const ColumnArgs& a, float w0, float w1, bool hi, float qmin,
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

// G: the group size whose scale (and zero-point) the loop computes at each group start, from the running state, and
// writes; or 0: they are given and read only
template <typename T, bool kZp, int G, typename Rule>
__global__ __launch_bounds__(kBlock) void column_loop_kernel(ColumnArgs a) {
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t r = (int64_t)blockIdx.x * kWavesPerBlock + wave;
  if (r >= a.rows) return;  // wave-uniform
  const int lane = threadIdx.x & 63;
  const int bc = a.bc;
  const bool in0 = lane < bc, in1 = lane + 64 < bc;
  const float* wrow = reinterpret_cast<const float*>(a.x) + r * a.cols + a.col0;
  const float* ub = a.u + a.col0 * a.cols + a.col0;  // the matrix at [col0, col0]
  float r0 = in0 ? wrow[lane] : 0.f, r1 = in1 ? wrow[lane + 64] : 0.f;  // the running state
  float w0 = 0.f, w1 = 0.f;                                              // the weight beside a correction
  if constexpr (Rule::kCorrection) {
    const float* crow = a.c + r * a.cols + a.col0;
    w0 = r0;
    w1 = r1;
    r0 = in0 ? crow[lane] : 0.f;
    r1 = in1 ? crow[lane + 64] : 0.f;
  }
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
  const auto new_scale = [&] {  // called where s changes, inside that branch: the steps between pay no test for it
    if constexpr (sizeof(T) == 2) {
      fast = wave_fast_div<T>(s);
      rs = 1.0f / s;
    }
  };
  int64_t togo = 0;  // given: steps until the next group's scale and zero-point apply, a group of any size, also one
                     // that began before the block
  // row i of the matrix and its diagonal, one step ahead of their use
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
    if constexpr (G != 0) {
      if ((i & (G - 1)) == 0) {  // group start, wave-uniform
        float sg, zg;
        column_group_params<T, kZp, G>(a, r0, r1, hi, qmin, qmax, sg, zg);
        s = read_lane(sg, src);
        zp = read_lane(zg, src);
        if (lane == 0) {
          const int64_t grp = (a.col0 + i) / G;
          srow[grp] = from_f<T>(s);
          if constexpr (kZp) zrow[grp] = from_f<T>(zp);  // exact: an integer of the code range
        }
        new_scale();
      }
    } else {
      if (togo == 0) {  // wave-uniform
        togo = a.gsize - (a.col0 + i) % a.gsize;
        s = read_lane(hi ? s1 : s0, src);
        if constexpr (kZp) zp = read_lane(hi ? z1 : z0, src);
        new_scale();
      }
      --togo;
    }
    // the owner's weight, then its running state where that is not the weight: one read-lane, or two in this order
    float wi, ri;
    if constexpr (Rule::kCorrection) {
      wi = read_lane(hi ? w1 : w0, src);
      ri = read_lane(hi ? r1 : r0, src);
    } else {
      wi = ri = read_lane(hi ? r1 : r0, src);
    }
    const f2 xt = splat2(rnd<T>(Rule::value(wi, ri, cd)));
    f2 y;
    if (sizeof(T) == 2 && fast)
      y = group_fwd_pair<T, kZp>(xt, fast_div<T>(s, rs), s, qmin, qmax, zp);
    else
      y = group_fwd_pair<T, kZp>(xt, DivExact{s}, s, qmin, qmax, zp);
    T qa, qb;
    pack2<T>(y, qa, qb);
    const float q = to_f<T>(qa);
    const float e = Rule::error(wi, q, cd);
    const bool own = lane == src;
    q0 = (own && !hi) ? q : q0;
    e0 = (own && !hi) ? e : e0;
    q1 = (own && hi) ? q : q1;
    e1 = (own && hi) ? e : e1;
    // the columns right of i: the product rounded, then the rule's sum or difference rounded (no fused multiply-add)
    const float n0 = Rule::update(r0, __fmul_rn(e, cu0)), n1 = Rule::update(r1, __fmul_rn(e, cu1));
    r0 = (!hi && lane > src) ? n0 : r0;
    r1 = (!hi || lane > src) ? n1 : r1;
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

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
// what a column-loop kernel covers apart from the pointers: BVQ_OK, or the error with its text
// computed: scale and zero-point are computed in the loop, at each group start (GPTQ only)
static int column_block_check(const bvq_quant_desc* d, const char* what, int64_t rows, int64_t cols, int64_t col0,
                              int block_cols, int computed) {
  int rc = validate(d);
  if (rc) return rc;
  if (d->outer != 1 || d->channels < 1 || d->inner < 1 || !d->scale_per_channel) {
    set_error("%s: the descriptor of a grouped tensor is outer 1, channels = groups, inner = group size, one scale per "
              "channel", what);
    return BVQ_ERR_UNSUPPORTED;
  }
  if (d->round_mode != BVQ_ROUND || d->pre_op != BVQ_PRE_NONE || d->out_kind != BVQ_OUT_DEQUANT) {
    set_error("%s: half-even rounding, no pre_op and dequantized output only (round_mode=%d pre_op=%d out_kind=%d)", what,
              d->round_mode, d->pre_op, d->out_kind);
    return BVQ_ERR_UNSUPPORTED;
  }
  if (d->x_dtype != d->ct_dtype || d->scale_dtype != d->x_dtype || (d->zp_per_channel && d->zp_dtype != d->x_dtype)) {
    set_error("%s: x, compute, scale and zero-point dtype must agree (x=%d ct=%d scale=%d zp=%d)", what, d->x_dtype,
              d->ct_dtype, d->scale_dtype, d->zp_dtype);
    return BVQ_ERR_UNSUPPORTED;
  }
  if (rows < 1 || cols < 1 || cols % d->inner != 0 || rows * (cols / d->inner) != d->channels) {
    set_error("%s: rows %lld x cols %lld is not %lld groups of %lld", what, (long long)rows, (long long)cols,
              (long long)d->channels, (long long)d->inner);
    return BVQ_ERR_INVALID;
  }
  if (block_cols < 1 || block_cols > kColumnBlock) {
    set_error("%s: block_cols %d (1 .. %d)", what, block_cols, kColumnBlock);
    return BVQ_ERR_INVALID;
  }
  if (col0 < 0 || col0 + block_cols > cols) {
    set_error("%s: columns %lld .. %lld of %lld", what, (long long)col0, (long long)(col0 + block_cols), (long long)cols);
    return BVQ_ERR_INVALID;
  }
  if (computed) {
    if (d->inner != 16 && d->inner != 32 && d->inner != 64 && d->inner != 128) {
      set_error("%s: group size %lld (16, 32, 64 or 128 where scale and zero-point are computed in the loop)", what,
                (long long)d->inner);
      return BVQ_ERR_UNSUPPORTED;
    }
    if (col0 % d->inner != 0 || block_cols % d->inner != 0) {
      set_error("%s: col0 %lld and block_cols %d must be multiples of the group size %lld", what, (long long)col0,
                block_cols, (long long)d->inner);
      return BVQ_ERR_INVALID;
    }
  }
  return BVQ_OK;
}

// The launching entry `what` of the rule's kernel: the checks, the arguments, one wave per row.  c: the correction where
// the rule has one, else null; Gs: the group sizes instantiated (0: given parameters), of which `computed` selects the
// descriptor's or 0; names: the pointers that must lie on 16-byte boundaries, for the text
template <typename Rule, int... Gs>
static int column_block_launch(const char* what, const bvq_quant_desc* d, const float* wf, const float* c,
                               const float* u, int64_t rows, int64_t cols, int64_t col0, int block_cols, int computed,
                               double min_val, int use_min, double thr_div, void* q, float* err, void* scale, void* zp,
                               const char* names, bvq_stream_t stream) {
  int rc = column_block_check(d, what, rows, cols, col0, block_cols, computed);
  const bool shifted = !rc && d->zp_per_channel;
  rc = group_required(what, rc, {wf, Rule::kCorrection ? c : wf, u, q, err, scale});
  if (!rc && shifted && !zp) {
    set_error("%s: null pointer (zp of an asymmetric quantizer)", what);
    return BVQ_ERR_INVALID;
  }
  if ((rc = group_aligned(what, rc, {wf, c, u, q, err}, names))) return rc;
  ColumnArgs a = group_args<ColumnArgs>(d, min_val, use_min, thr_div);
  a.x = wf;
  a.y = q;
  a.scale = scale;
  a.u = u;
  a.c = c;
  a.err = err;
  a.zp = zp;
  a.rows = rows;
  a.cols = cols;
  a.col0 = col0;
  a.bc = block_cols;
  a.gsize = (int32_t)d->inner;
  const unsigned grid = (unsigned)((rows + kWavesPerBlock - 1) / kWavesPerBlock);
  rc = with_dtype(d->x_dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    return with_bool(shifted, [&](auto z) {
      return with_value<Gs...>(computed ? (int)d->inner : 0, [&](auto g) {
        column_loop_kernel<T, decltype(z)::value, decltype(g)::value, Rule><<<grid, kBlock, 0, (hipStream_t)stream>>>(a);
      });
    });
  });
  return rc ? rc : check_launch(what);
}

}  // namespace bvq
