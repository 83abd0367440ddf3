// bvq_weight_norm.hip -- weight-normalised weight quantizers, one launch each way: per output channel (a ROW of the
// weight viewed [rows, K]) the weight is divided by its norm, rescaled by a learned g and quantized with a learned
// scale s.  BVQ_NORM_L2 with half-even rounding is the weight-norm quantizer; BVQ_NORM_L1 with round-to-zero and g
// capped at T * s is the accumulator-aware quantizer A2Q, whose integer codes satisfy sum |q| <= T per row.
//
// All arithmetic is float32 whatever the weight's dtype T (v is widened exactly, y and dv are rounded to T once):
//
//   n  = norm(v) > norm_min ? norm(v) : norm_min     norm = sum |v_i|  or  sqrt(sum v_i^2)
//   g' = g <= T * s ? g : T * s                       (a tie goes to g; T = +inf never caps)
//   p  = (s * n) / g'                                 two operations, in this order
//   t_i = v_i / p  (IEEE division);  r_i = R(t_i);  q_i = clamp(r_i, -qmax, qmax);  y_i = T(q_i * s)
//
//   backward, m_i = clamp_ste or not (r_i > qmax or r_i < -qmax):
//   A = sum gy_i * m_i * t_i      B = sum gy_i * q_i
//   c1 = g' / n;  sA = s * A;  c2 = n > norm_min ? sA / n : 0
//   dv_i = T(gy_i * m_i * c1 - c2 * sign(v_i))            L1, sign(0) = 0
//   dv_i = T(gy_i * m_i * c1 - (c2 / n) * v_i)            L2
//   dg' = sA / g';  g <= T * s: ds = B - A, dg = dg';  else: ds = (B - A) + T * dg', dg = 0
//
// A row lives in the registers of one wave or one workgroup from its only load to its only store (bvq_row_walk.h has
// the three geometries).  Forward: all loads issued, the norm's partial sums formed in registers, butterfly inside the
// wave, one LDS exchange with one barrier across the waves of a row, the row's chain (g', p) once on wave-uniform values,
// quantization from the registers.  Backward: p rebuilt from the saved n with the forward's operations, so t, r, q and m
// are the forward's bits; A and B cross the row's waves together with one barrier; gy * m (gy or 0: exact in T) replaces
// gy in its registers, so no element is divided twice.
//   forward   reads v, writes y               (+ s, g read and n written per row)
//   backward  reads gy and v, writes dv once  (+ s, g, n read and ds, dg written per row)
// No workspace, no atomics, nothing between workgroups.
//
// Sum order (the norm's sum, A and B alike; fixed by K, the dtype and the geometry, hence the same bits on every run):
// a lane adds the terms of its chunks in ascending j, inside a chunk in ascending element pairs, element 2k to the first
// and element 2k + 1 to the second half of one pair accumulator; the halves are added; the 64 lanes by the xor butterfly
// 32, 16, 8, 4, 2, 1; the kW waves as ((w0 + w1) + w2) + w3.  A lane past the row's end adds +0 (forward) or nothing
// (backward).  The square root of the L2 norm is taken of the folded sum.
#include "bvq_fakequant.h"
#include "bvq_row_walk.h"

namespace bvq {

struct WeightNormArgs : WalkArgs {  // x: v, g: gy, y: y (forward) / dv (backward)
  int64_t rows;
  uint32_t cpr;        // 16-byte chunks per row
  const float* scale;  // [rows]
  const float* gpar;   // [rows]
  float* norm;         // [rows]: forward out, backward in
  float* dscale;       // [rows], backward out
  float* dgpar;        // [rows], backward out
  float qmax, t_bound, norm_min;
  int32_t clamp_ste;
};

template <int kNorm>
constexpr int kNormRound = kNorm == BVQ_NORM_L1 ? BVQ_ROUND_TO_ZERO : BVQ_ROUND;

// the row's chain from n: g' and p, and whether g was capped
struct NormRow {
  float s, gp, p;
  bool capped;
};
__device__ __forceinline__ NormRow norm_row(const WeightNormArgs& a, int64_t row, float n) {
  NormRow r;
  r.s = a.scale[row];
  const float g = a.gpar[row], ts = a.t_bound * r.s;
  r.capped = !(g <= ts);
  r.gp = r.capped ? ts : g;
  r.p = (r.s * n) / r.gp;
  return r;
}

// the sum of one value per lane over the row: butterfly, then the row's waves in wave order
template <int kW, int N>
__device__ __forceinline__ void row_sums(uint32_t (&ex)[kW][4], uint32_t wave, float (&v)[N]) {
  uint32_t mine[N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    v[i] = seg_sum<kWave>(v[i]);
    mine[i] = __builtin_bit_cast(uint32_t, v[i]);
  }
  if constexpr (kW > 1) {
    uint32_t all[kW][N];
    row_exchange<kW, N>(ex, wave, mine, all);
#pragma unroll
    for (int i = 0; i < N; ++i) {
      v[i] = __builtin_bit_cast(float, all[0][i]);
#pragma unroll
      for (int w = 1; w < kW; ++w) v[i] += __builtin_bit_cast(float, all[w][i]);
    }
  }
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = uniform_f(v[i]);
}

template <typename T, int kNorm, int kW, int kD, bool NT>
__global__ __launch_bounds__(kBlock) void weight_norm_fwd_kernel(WeightNormArgs a) {
  constexpr int VEC = elem<T>::vec;
  __shared__ uint32_t ex[kW][4];
  RowSlot<kW> slot;
  if (!slot.init(a)) return;
  const buf_t bx = slot.template elems<T>(a.x, a), by = slot.template elems<T>(a.y, a);
  vec_t<T, VEC> xv[kD];
#pragma unroll
  for (int j = 0; j < kD; ++j) xv[j] = buf_load<T, VEC, NT>(bx, slot.chunk(j) * 16u);
  f2 acc = splat2(0.f);
#pragma unroll
  for (int j = 0; j < kD; ++j) {
    if (slot.first(j) >= a.cpr) break;  // wave-uniform; a lane past the row's end holds zeros, which add +0
#pragma unroll
    for (int k = 0; k < VEC; k += 2) {
      const f2 xf = widen2<T>(xv[j].v[k], xv[j].v[k + 1]);
      if constexpr (kNorm == BVQ_NORM_L1)
        acc = acc + __builtin_elementwise_abs(xf);
      else
        acc = acc + xf * xf;
    }
  }
  float sum[1] = {acc.x + acc.y};
  row_sums<kW, 1>(ex, slot.wave, sum);
  // the row's chain, once, on wave-uniform values
  const float raw = kNorm == BVQ_NORM_L1 ? sum[0] : __builtin_sqrtf(sum[0]);
  const float n = raw > a.norm_min ? raw : a.norm_min;
  const NormRow r = norm_row(a, slot.row, n);
  if (slot.wave == 0 && (threadIdx.x & 63) == 0) a.norm[slot.row] = n;
  const f2 p2 = splat2(r.p);
#pragma unroll
  for (int j = 0; j < kD; ++j) {
    if (slot.first(j) >= a.cpr) break;
    vec_t<T, VEC> yv;
#pragma unroll
    for (int k = 0; k < VEC; k += 2) {
      const f2 t = widen2<T>(xv[j].v[k], xv[j].v[k + 1]) / p2;
      const f2 q = clamp_where2(round_op2<float, kNormRound<kNorm>>(t), -a.qmax, a.qmax);
      pack2<T>(q * r.s, yv.v[k], yv.v[k + 1]);
    }
    buf_store<T, VEC, NT>(by, slot.chunk(j) * 16u, yv);
  }
}

template <typename T, int kNorm, int kW, int kD, bool NT>
__global__ __launch_bounds__(kBlock) void weight_norm_bwd_kernel(WeightNormArgs a) {
  constexpr int VEC = elem<T>::vec;
  __shared__ uint32_t ex[kW][4];
  RowSlot<kW> slot;
  if (!slot.init(a)) return;
  const buf_t bx = slot.template elems<T>(a.x, a), bg = slot.template elems<T>(a.g, a),
              bd = slot.template elems<T>(a.y, a);
  vec_t<T, VEC> xv[kD], gv[kD];
#pragma unroll
  for (int j = 0; j < kD; ++j) xv[j] = buf_load<T, VEC, NT>(bx, slot.chunk(j) * 16u);
#pragma unroll
  for (int j = 0; j < kD; ++j) gv[j] = buf_load<T, VEC, NT>(bg, slot.chunk(j) * 16u);
  // the forward's p from the saved n: the same operations, the saved bits
  const float n = a.norm[slot.row];
  const NormRow r = norm_row(a, slot.row, n);
  const bool clamp_ste = a.clamp_ste != 0;
  const f2 p2 = splat2(r.p);
  f2 a2 = splat2(0.f), b2 = splat2(0.f);
#pragma unroll
  for (int j = 0; j < kD; ++j) {
    if (slot.first(j) >= a.cpr) break;  // wave-uniform
    if (slot.chunk(j) < a.cpr) {        // a lane past the row's end adds no term
#pragma unroll
      for (int k = 0; k < VEC; k += 2) {
        const f2 gf = widen2<T>(gv[j].v[k], gv[j].v[k + 1]);
        const f2 t = widen2<T>(xv[j].v[k], xv[j].v[k + 1]) / p2;
        const f2 rr = round_op2<float, kNormRound<kNorm>>(t);
        const f2 q = clamp_where2(rr, -a.qmax, a.qmax);
        f2 gm = gf;  // gy * m: gy or 0
        if (!clamp_ste) {
          gm.x = (rr.x > a.qmax || rr.x < -a.qmax) ? 0.f : gf.x;
          gm.y = (rr.y > a.qmax || rr.y < -a.qmax) ? 0.f : gf.y;
        }
        a2 = a2 + gm * t;
        b2 = b2 + gf * q;
        pack2<T>(gm, gv[j].v[k], gv[j].v[k + 1]);  // exact
      }
    }
  }
  float sums[2] = {a2.x + a2.y, b2.x + b2.y};
  row_sums<kW, 2>(ex, slot.wave, sums);
  // the row's chain, once, on wave-uniform values
  const float c1 = r.gp / n, sA = r.s * sums[0];
  const float c2 = n > a.norm_min ? sA / n : 0.f;
  const float dgp = sA / r.gp;
  if (slot.wave == 0 && (threadIdx.x & 63) == 0) {
    const float ds = sums[1] - sums[0];
    a.dscale[slot.row] = r.capped ? ds + a.t_bound * dgp : ds;
    a.dgpar[slot.row] = r.capped ? 0.f : dgp;
  }
  const float c3 = kNorm == BVQ_NORM_L1 ? c2 : c2 / n;
#pragma unroll
  for (int j = 0; j < kD; ++j) {
    if (slot.first(j) >= a.cpr) break;
    vec_t<T, VEC> dv;
#pragma unroll
    for (int k = 0; k < VEC; k += 2) {
      const f2 xf = widen2<T>(xv[j].v[k], xv[j].v[k + 1]);
      const f2 gm = widen2<T>(gv[j].v[k], gv[j].v[k + 1]);
      f2 dn = xf;  // dn / dv_i (L2: up to the factor 1 / n, which c3 carries)
      if constexpr (kNorm == BVQ_NORM_L1) {
        dn.x = (float)(xf.x > 0.f) - (float)(xf.x < 0.f);
        dn.y = (float)(xf.y > 0.f) - (float)(xf.y < 0.f);
      }
      pack2<T>(gm * c1 - dn * c3, dv.v[k], dv.v[k + 1]);
    }
    buf_store<T, VEC, NT>(bd, slot.chunk(j) * 16u, dv);
  }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
// what the kernels cover, apart from the pointers: BVQ_OK, or the error with its text
static int weight_norm_check(const bvq_quant_desc* d, int norm_kind, double t_bound, double norm_min, const char* what) {
  const int rc = validate(d);
  if (rc) return rc;
  if (norm_kind != BVQ_NORM_L1 && norm_kind != BVQ_NORM_L2) {
    set_error("%s: bad norm kind %d", what, norm_kind);
    return BVQ_ERR_INVALID;
  }
  if (!(t_bound > 0.0) || !(norm_min > 0.0)) {  // (a NaN is refused too)
    set_error("%s: t_bound %g and norm_min %g must be positive", what, t_bound, norm_min);
    return BVQ_ERR_INVALID;
  }
  if (d->outer != 1 || !d->scale_per_channel || d->zp_per_channel) {
    set_error("%s: the descriptor of a weight [rows, K] is outer 1, channels = rows, inner = K, one scale per channel and "
              "one zero-point", what);
    return BVQ_ERR_UNSUPPORTED;
  }
  if (d->ct_dtype != BVQ_F32 || d->scale_dtype != BVQ_F32) {
    set_error("%s: compute and scale dtype must be float32 (ct=%d scale=%d)", what, d->ct_dtype, d->scale_dtype);
    return BVQ_ERR_UNSUPPORTED;
  }
  if (d->round_mode != (norm_kind == BVQ_NORM_L1 ? BVQ_ROUND_TO_ZERO : BVQ_ROUND)) {
    set_error("%s: round_mode %d (round-to-zero with the L1 norm, half-even with the L2 norm)", what, d->round_mode);
    return BVQ_ERR_UNSUPPORTED;
  }
  if (!(d->qmax >= 1.f) || d->qmin != -d->qmax) {
    set_error("%s: a narrow signed range, qmin = -qmax <= -1 (qmin=%g qmax=%g)", what, d->qmin, d->qmax);
    return BVQ_ERR_UNSUPPORTED;
  }
  if (d->pre_op != BVQ_PRE_NONE || d->out_kind != BVQ_OUT_DEQUANT) {
    set_error("%s: pre_op %d / out_kind %d are not covered", what, d->pre_op, d->out_kind);
    return BVQ_ERR_UNSUPPORTED;
  }
  const int64_t bytes = d->inner * dtype_size(d->x_dtype);
  if (d->inner < 1 || bytes % 16 != 0 || bytes > kRowMaxBytes) {
    set_error("%s: a row of %lld bytes (a multiple of 16, at most %lld)", what, (long long)bytes,
              (long long)kRowMaxBytes);
    return BVQ_ERR_UNSUPPORTED;
  }
  return BVQ_OK;
}

static WeightNormArgs weight_norm_args(const bvq_quant_desc* d, double t_bound, double norm_min) {
  WeightNormArgs a = {};
  a.rows = d->channels;
  a.cpr = (uint32_t)(d->inner * dtype_size(d->x_dtype) / 16);
  a.chunks = a.rows * a.cpr;
  a.qmax = d->qmax;
  a.t_bound = (float)t_bound;
  a.norm_min = (float)norm_min;
  a.clamp_ste = d->clamp_ste;
  return a;
}

// f(type_tag<T>, int_c<kNorm>, int_c<kW>, int_c<kD>, std::bool_constant<NT>, grid)
template <typename F>
static int weight_norm_launch(const char* what, const bvq_quant_desc* d, int norm_kind, const WeightNormArgs& a,
                              int chunk_bytes, F&& f) {
  return row_launch(what, d->x_dtype, a, chunk_bytes, [&](auto t, auto w, auto depth, auto nt, unsigned grid) {
    if (norm_kind == BVQ_NORM_L1) return call_rc(f, t, int_c<BVQ_NORM_L1>{}, w, depth, nt, grid);
    return call_rc(f, t, int_c<BVQ_NORM_L2>{}, w, depth, nt, grid);
  });
}

}  // namespace bvq

using namespace bvq;

extern "C" int bvq_weight_norm_supported(const bvq_quant_desc* d, int norm_kind, double t_bound, double norm_min,
                                         const void* x) {
  if (weight_norm_check(d, norm_kind, t_bound, norm_min, "bvq_weight_norm_supported")) return 0;
  return x && aligned16(x) ? 1 : 0;
}

extern "C" int bvq_weight_norm_fwd(const bvq_quant_desc* d, int norm_kind, double t_bound, double norm_min,
                                   const void* x, const float* scale, const float* g, void* y, float* norm,
                                   bvq_stream_t stream) {
  const char* what = "bvq_weight_norm_fwd";
  int rc = group_required(what, weight_norm_check(d, norm_kind, t_bound, norm_min, what), {x, scale, g, y, norm});
  if ((rc = group_aligned(what, rc, {x, y}, "x and y"))) return rc;
  WeightNormArgs a = weight_norm_args(d, t_bound, norm_min);
  a.x = x;
  a.y = y;
  a.scale = scale;
  a.gpar = g;
  a.norm = norm;
  // x read + y written
  return weight_norm_launch(what, d, norm_kind, a, 32, [&](auto t, auto k, auto w, auto depth, auto nt, unsigned grid) {
    weight_norm_fwd_kernel<typename decltype(t)::type, k, w, depth, nt><<<grid, kBlock, 0, (hipStream_t)stream>>>(a);
  });
}

extern "C" int bvq_weight_norm_bwd(const bvq_quant_desc* d, int norm_kind, double t_bound, double norm_min,
                                   const void* gy, const void* x, const float* scale, const float* g,
                                   const float* norm, void* dx, float* dscale, float* dg, bvq_stream_t stream) {
  const char* what = "bvq_weight_norm_bwd";
  int rc = group_required(what, weight_norm_check(d, norm_kind, t_bound, norm_min, what),
                          {gy, x, scale, g, norm, dx, dscale, dg});
  if ((rc = group_aligned(what, rc, {gy, x, dx}, "gy, x and dx"))) return rc;
  WeightNormArgs a = weight_norm_args(d, t_bound, norm_min);
  a.x = x;
  a.g = gy;
  a.y = dx;
  a.scale = scale;
  a.gpar = g;
  a.norm = const_cast<float*>(norm);
  a.dscale = dscale;
  a.dgpar = dg;
  // gy and x read, dx written
  return weight_norm_launch(what, d, norm_kind, a, 48, [&](auto t, auto k, auto w, auto depth, auto nt, unsigned grid) {
    weight_norm_bwd_kernel<typename decltype(t)::type, k, w, depth, nt><<<grid, kBlock, 0, (hipStream_t)stream>>>(a);
  });
}
