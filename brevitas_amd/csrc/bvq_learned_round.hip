// bvq_learned_round.hip -- learned rounding (AdaRound; LearnedRoundSte of later Brevitas releases): IntQuant whose
// float_to_int_impl is floor(t) + h(value), with one trainable offset `value` per element, as one kernel each way.
//
// Composed from the modules, one optimisation step is about a dozen elementwise launches forward and more backward;
// here the forward is one read of x, one of value and one write of y, the backward reads g, x and value and writes
// dvalue (and dx when it is asked for).  Nothing needs a reduction: no LDS, no atomics, no workspace.
//
// The tensor is walked as a flat stream of 16-byte lane accesses through buffer descriptors that end with the tensor
// (GroupWindow of bvq_group_walk.h with one lane per "group"): lanes past the end read zeros and drop their stores, so
// there is no tail branch, and all loads of a wave's window are in flight before the arithmetic.  Rows are whole
// chunks (the host checks it), so a lane's chunk lies inside one channel: its scale and zero-point are one cached load
// each, at the channel index  chunk / (chunks per row)  -- a multiply-high and a shift with constants from the host.
//
// Every line of the chain (include/bvq.h, "Learned rounding") is one torch op on the composed route and is rounded to
// the dtype T where torch's device kernel rounds it (rnd / rnd2 of bvq_quant_math.h; sigmoid and sigmoid_backward of
// bvq_act.h), so y, dvalue and dx are the composed route's bits.
#include "bvq_act.h"
#include "bvq_group_quant.h"  // the window, the choice of the division, validate()

namespace bvq {

struct LrArgs : WalkArgs {  // x; g (bwd); y (fwd: y, bwd: dvalue); chunks
  const void* value;
  void* dx;           // bwd, nullable
  const void* scale;  // 1 or `channels` elements, scale_dtype
  const void* zp;     // 1 or `channels` elements, zp_dtype
  uint32_t cpr, magic, shift, channels;  // chunks per row and its multiply-high / shift form (lr_divider)
  float qmin, qmax, c0, c1;
  int32_t scale_dtype, zp_dtype, scale_pc, zp_pc, scalar_cast, clamp_ste, hard;
};

// one element of a scale-like array of runtime dtype, as loaded (the conversion waits until the value is used)
__device__ __forceinline__ uint32_t lr_side_load(buf_t b, int dt, uint32_t idx) {
  if (dt == BVQ_F32) return buf_load<uint32_t, 1>(b, idx * 4u).v[0];
  return buf_load<uint16_t, 1>(b, idx * 2u).v[0];
}
__device__ __forceinline__ float lr_side_value(uint32_t raw, int dt) {
  if (dt == BVQ_F32) return __builtin_bit_cast(float, raw);
  if (dt == BVQ_BF16) return __builtin_bit_cast(float, raw << 16);
  return (float)__builtin_bit_cast(f16_t, (uint16_t)raw);
}

// scale and zero-point of a lane's chunk: wave constants for a one-element operand, else one load per wave load at the
// chunk's channel.  A chunk past the end has a channel past the array: its load returns zeros without a memory access.
template <typename T>
struct LrSide {
  const LrArgs& a;
  buf_t bs, bz;
  uint32_t c0;  // first chunk of the wave's window (chunks < 2^31: lr_check)
  float s1, z1;
  __device__ __forceinline__ LrSide(const LrArgs& a, int64_t c0) : a(a), c0((uint32_t)c0) {
    bs = make_buf(reinterpret_cast<const char*>(a.scale), a.scale_pc ? a.channels * (a.scale_dtype == BVQ_F32 ? 4u : 2u) : 0u);
    bz = make_buf(reinterpret_cast<const char*>(a.zp), a.zp_pc ? a.channels * (a.zp_dtype == BVQ_F32 ? 4u : 2u) : 0u);
    s1 = z1 = 0.f;
    if (!a.scale_pc) {
      s1 = load_scalar_as_f(a.scale, a.scale_dtype, 0);
      if (a.scalar_cast) s1 = rnd<T>(s1);  // device-torch semantics for a 0-dim operand wider than T (bvq.h)
    }
    if (!a.zp_pc) {
      z1 = load_scalar_as_f(a.zp, a.zp_dtype, 0);
      if (a.scalar_cast) z1 = rnd<T>(z1);
    }
  }
  __device__ __forceinline__ uint32_t channel(int j) const {
    const uint32_t c = c0 + (uint32_t)(j * kWave) + (threadIdx.x & 63);
    return (__umulhi(c, a.magic) + c) >> a.shift;  // c / cpr for c < 2^31
  }
  __device__ __forceinline__ void load(int j, uint32_t& sr, uint32_t& zr) const {
    sr = zr = 0u;
    if (a.scale_pc | a.zp_pc) {  // wave-uniform
      const uint32_t ch = channel(j);
      if (a.scale_pc) sr = lr_side_load(bs, a.scale_dtype, ch);
      if (a.zp_pc) zr = lr_side_load(bz, a.zp_dtype, ch);
    }
  }
  __device__ __forceinline__ void get(uint32_t sr, uint32_t zr, float& s, float& z) const {
    s = a.scale_pc ? lr_side_value(sr, a.scale_dtype) : s1;
    z = a.zp_pc ? lr_side_value(zr, a.zp_dtype) : z1;
  }
};

__device__ __forceinline__ float lr_clamp01(float v) {  // torch.clamp(v, 0.0, 1.0): a NaN stays
  return v != v ? v : __builtin_fminf(__builtin_fmaxf(v, 0.f), 1.f);
}

// A tensor of T times a host scalar: the product of float(a) and the float32 scalar, rounded to T -- two roundings, which
// is what torch's device kernels do for bfloat16.  For float16 torch's own kernel is not one function of its inputs: its
// vectorised body rounds twice like this, its tail path compiles to the mixed-precision fma, which rounds the exact
// product once (and, with its +0 addend, turns a -0 product into +0).  The two differ where the float32 product lands
// on a float16 tie -- every tenth element for float(1.4), never for float(1.2) or a power of two.  The Python routing
// sends float16 here only for scalars with which they cannot differ (learned_round.f16_products_agree).
template <typename T>
__device__ __forceinline__ f2 mul_scalar2(f2 a, float b) {
  return rnd2<T>(a * splat2(b));
}

// h(value) with torch's rounding points, on pairs.
//   BVQ_LR_HARD_SIGMOID  sg = sigmoid(v); pre = sg * c0 + c1 (two ops; c0 = float(zeta - gamma), c1 = float(gamma): a
//                        Python-float operand enters in float32 opmath); p = clamp(pre, 0, 1); hard: p > 0.5
//   BVQ_LR_SIGMOID       sg = sigmoid(v * inv), inv = 1.0f / float(temperature) (a division by a host scalar is a
//                        multiplication by its reciprocal on the device); p = sg; hard: v > 0
template <typename T, int IMPL>
struct LrMath {
  float c0, c1, inv;
  __device__ __forceinline__ LrMath(const LrArgs& a) : c0(a.c0), c1(a.c1), inv(1.0f / a.c0) {}
  __device__ __forceinline__ f2 soft(f2 v, f2& sg, f2& pre) const {
    if constexpr (IMPL == BVQ_LR_HARD_SIGMOID) {
      sg = act_rnd2<T, BVQ_PRE_SIGMOID>(v);
      const f2 m = mul_scalar2<T>(sg, c0);
      pre = rnd2<T>(m + splat2(c1));
      return f2{lr_clamp01(pre.x), lr_clamp01(pre.y)};
    } else {
      const f2 u = mul_scalar2<T>(v, inv);
      sg = act_rnd2<T, BVQ_PRE_SIGMOID>(u);
      pre = sg;
      return sg;
    }
  }
  __device__ __forceinline__ f2 hard(f2 v) const {
    if constexpr (IMPL == BVQ_LR_HARD_SIGMOID) {
      f2 sg, pre;
      const f2 p = soft(v, sg, pre);
      return f2{p.x > 0.5f ? 1.f : 0.f, p.y > 0.5f ? 1.f : 0.f};
    } else {
      return f2{v.x > 0.f ? 1.f : 0.f, v.y > 0.f ? 1.f : 0.f};
    }
  }
  // dvalue from dr (the gradient of r = floor(t) + p, a value of T), and what soft() left
  __device__ __forceinline__ f2 grad(f2 dr, f2 sg, f2 pre) const {
    if constexpr (IMPL == BVQ_LR_HARD_SIGMOID) {
      // torch.clamp's backward: where((pre >= 0) & (pre <= 1), grad, 0)
      f2 dp = {(pre.x >= 0.f && pre.x <= 1.f) ? dr.x : 0.f, (pre.y >= 0.f && pre.y <= 1.f) ? dr.y : 0.f};
      dp = mul_scalar2<T>(dp, c0);
      return f2{act_bwd_f<T, BVQ_PRE_SIGMOID>(dp.x, sg.x), act_bwd_f<T, BVQ_PRE_SIGMOID>(dp.y, sg.y)};
    } else {
      const f2 d = {act_bwd_f<T, BVQ_PRE_SIGMOID>(dr.x, sg.x), act_bwd_f<T, BVQ_PRE_SIGMOID>(dr.y, sg.y)};
      return mul_scalar2<T>(d, inv);
    }
  }
};

template <typename T>
struct LrPairs {
  f2 v[elem<T>::vec / 2];
};

// t = x / s + zp of a chunk, both roundings, with the division the wave takes for this load
template <typename T>
__device__ __forceinline__ LrPairs<T> lr_t_chunk(const vec_t<T, elem<T>::vec>& xv, float s, float z) {
  return with_group_div<T>(s, [&](const auto& div) {
    LrPairs<T> r;
#pragma unroll
    for (int k = 0; k < elem<T>::vec / 2; ++k) {
      const f2 t = rnd2<T>(div(widen2<T>(xv.v[2 * k], xv.v[2 * k + 1])));
      r.v[k] = rnd2<T>(t + splat2(z));
    }
    return r;
  });
}

template <typename T, int IMPL, bool NT>
__global__ __launch_bounds__(kBlock) void lr_fwd_kernel(LrArgs a) {
  constexpr int VEC = elem<T>::vec, kD = kGroupFwdDepth;
  GroupWindow<T, 1, kD> w;
  if (!w.init(a)) return;
  const buf_t bx = w.elems(a.x), bv = w.elems(a.value), by = w.elems(a.y);
  const LrSide<T> side(a, w.c0);
  const LrMath<T, IMPL> m(a);
  const float qmin = rnd<T>(a.qmin), qmax = rnd<T>(a.qmax);
  const bool hard = a.hard != 0;
  vec_t<T, VEC> xv[kD], vv[kD];
  uint32_t sr[kD], zr[kD];
#pragma unroll
  for (int j = 0; j < kD; ++j) {
    const uint32_t off = group_place<1>(j).off;
    xv[j] = buf_load<T, VEC, NT>(bx, off);
    vv[j] = buf_load<T, VEC, NT>(bv, off);
    side.load(j, sr[j], zr[j]);
  }
#pragma unroll
  for (int j = 0; j < kD; ++j) {
    if ((uint32_t)(j * kWave) >= w.nch) break;  // wave-uniform
    float s, z;
    side.get(sr[j], zr[j], s, z);
    const LrPairs<T> t = lr_t_chunk<T>(xv[j], s, z);
    vec_t<T, VEC> yv;
#pragma unroll
    for (int k = 0; k < VEC / 2; ++k) {
      const f2 v = widen2<T>(vv[j].v[2 * k], vv[j].v[2 * k + 1]);
      f2 sg, pre;
      const f2 p = hard ? m.hard(v) : m.soft(v, sg, pre);
      const f2 r = rnd2<T>(__builtin_elementwise_floor(t.v[k]) + p);
      const f2 c = clamp_where2(r, qmin, qmax);
      pack2<T>(rnd2<T>(c - splat2(z)) * splat2(s), yv.v[2 * k], yv.v[2 * k + 1]);
    }
    buf_store<T, VEC, NT>(by, group_place<1>(j).off, yv);
  }
}

template <typename T, int IMPL, bool NT>
__global__ __launch_bounds__(kBlock) void lr_bwd_kernel(LrArgs a) {
  constexpr int VEC = elem<T>::vec, kD = kGroupBwdDepth;
  GroupWindow<T, 1, kD> w;
  if (!w.init(a)) return;
  const buf_t bx = w.elems(a.x), bv = w.elems(a.value), bg = w.elems(a.g), bd = w.elems(a.y);
  const bool want_dx = a.dx != nullptr;  // wave-uniform
  const buf_t bdx = want_dx ? w.elems(a.dx) : make_buf(reinterpret_cast<const T*>(a.x), 0u);
  const LrSide<T> side(a, w.c0);
  const LrMath<T, IMPL> m(a);
  const float qmin = rnd<T>(a.qmin), qmax = rnd<T>(a.qmax);
  const bool ste = a.clamp_ste != 0;
  vec_t<T, VEC> xv[kD], vv[kD], gv[kD];
  uint32_t sr[kD], zr[kD];
#pragma unroll
  for (int j = 0; j < kD; ++j) {
    const uint32_t off = group_place<1>(j).off;
    xv[j] = buf_load<T, VEC, NT>(bx, off);
    vv[j] = buf_load<T, VEC, NT>(bv, off);
    gv[j] = buf_load<T, VEC, NT>(bg, off);
    side.load(j, sr[j], zr[j]);
  }
#pragma unroll
  for (int j = 0; j < kD; ++j) {
    if ((uint32_t)(j * kWave) >= w.nch) break;  // wave-uniform
    float s, z;
    side.get(sr[j], zr[j], s, z);
    const LrPairs<T> t = lr_t_chunk<T>(xv[j], s, z);
    LrPairs<T> dr;
    vec_t<T, VEC> dv;
#pragma unroll
    for (int k = 0; k < VEC / 2; ++k) {
      const f2 v = widen2<T>(vv[j].v[2 * k], vv[j].v[2 * k + 1]);
      const f2 g = widen2<T>(gv[j].v[2 * k], gv[j].v[2 * k + 1]);
      f2 sg, pre;
      const f2 p = m.soft(v, sg, pre);
      const f2 r = rnd2<T>(__builtin_elementwise_floor(t.v[k]) + p);
      const f2 dc = rnd2<T>(g * splat2(s));
      // tensor_clamp's backward: the gradient passes where r was not replaced (a NaN was not); straight through: all
      const f2 d = {(ste || !(r.x > qmax || r.x < qmin)) ? dc.x : 0.f, (ste || !(r.y > qmax || r.y < qmin)) ? dc.y : 0.f};
      dr.v[k] = d;
      pack2<T>(m.grad(d, sg, pre), dv.v[2 * k], dv.v[2 * k + 1]);
    }
    const uint32_t off = group_place<1>(j).off;
    buf_store<T, VEC, NT>(bd, off, dv);
    if (want_dx) {  // floor_ste and the add of the zero-point are identities: dx = dr / s
      const vec_t<T, VEC> xg = with_group_div<T>(s, [&](const auto& div) {
        vec_t<T, VEC> o;
#pragma unroll
        for (int k = 0; k < VEC / 2; ++k) pack2<T>(div(dr.v[k]), o.v[2 * k], o.v[2 * k + 1]);
        return o;
      });
      buf_store<T, VEC, NT>(bdx, off, xg);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
// n / d for n < 2^31 as (umulhi(n, magic) + n) >> shift (the round-up method; the sum stays below 2^32)
static void lr_divider(uint32_t d, uint32_t& magic, uint32_t& shift) {
  for (shift = 0; shift < 32; ++shift)
    if ((1u << shift) >= d) break;
  const uint64_t one = 1;
  magic = (uint32_t)(((one << 32) * ((one << shift) - d)) / d + 1);
}

static bool lr_per_channel(const bvq_quant_desc* d) {
  return (d->scale_per_channel || d->zp_per_channel) && d->channels > 1;
}

// what the kernels cover, apart from the pointers: BVQ_OK, or the error with its text
static int lr_check(const bvq_quant_desc* d, int impl, const char* what) {
  int rc = validate(d);
  if (rc) return rc;
  if (impl != BVQ_LR_HARD_SIGMOID && impl != BVQ_LR_SIGMOID) {
    set_error("%s: bad impl %d", what, impl);
    return BVQ_ERR_INVALID;
  }
  if (bad_dtype(d->x_dtype) || bad_dtype(d->scale_dtype) || bad_dtype(d->zp_dtype)) {
    set_error("%s: bad dtype", what);
    return BVQ_ERR_INVALID;
  }
  if (d->x_dtype != d->ct_dtype) {
    set_error("%s: x and compute dtype must agree (x=%d ct=%d)", what, d->x_dtype, d->ct_dtype);
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
  const int64_t es = dtype_size(d->x_dtype);
  const int64_t n = d->outer * d->channels * d->inner;
  if (lr_per_channel(d) && (d->outer != 1 || (d->inner * es) % 16 != 0)) {
    set_error("%s: a per-channel tensor is [1, channels, inner] with rows of whole 16-byte chunks, got [%lld, %lld, %lld]",
              what, (long long)d->outer, (long long)d->channels, (long long)d->inner);
    return BVQ_ERR_UNSUPPORTED;
  }
  if (lr_per_channel(d) && d->channels >= ((int64_t)1 << 30)) {  // 32-bit byte offsets into a float32 side array
    set_error("%s: %lld channels (fewer than 2^30)", what, (long long)d->channels);
    return BVQ_ERR_UNSUPPORTED;
  }
  if ((n * es) % 16 != 0 || n * es / 16 >= ((int64_t)1 << 31)) {
    set_error("%s: %lld elements are not whole 16-byte chunks, or more than 2^31 of them", what, (long long)n);
    return BVQ_ERR_UNSUPPORTED;
  }
  return BVQ_OK;
}

static LrArgs lr_args(const bvq_quant_desc* d, double c0, double c1, int hard) {
  LrArgs a = {};
  const bool pc = lr_per_channel(d);
  const int64_t es = dtype_size(d->x_dtype);
  a.chunks = d->outer * d->channels * d->inner * es / 16;
  a.channels = pc ? (uint32_t)d->channels : 1u;
  a.cpr = pc ? (uint32_t)(d->inner * es / 16) : 1u;
  lr_divider(a.cpr, a.magic, a.shift);
  a.qmin = d->qmin;
  a.qmax = d->qmax;
  a.c0 = (float)c0;
  a.c1 = (float)c1;
  a.scale_dtype = d->scale_dtype;
  a.zp_dtype = d->zp_dtype;
  a.scale_pc = (pc && d->scale_per_channel) ? 1 : 0;
  a.zp_pc = (pc && d->zp_per_channel) ? 1 : 0;
  a.scalar_cast = d->scalar_mode == BVQ_SCALAR_CAST;
  a.clamp_ste = d->clamp_ste;
  a.hard = hard;
  return a;
}

// f(type_tag<T>, int_c<IMPL>, std::bool_constant<NT>, grid) launches <<<grid, kBlock>>> the kernel whose waves own
// `depth` loads; streams: the tensors the kernel reads and writes, for the NT decision
template <typename F>
static int lr_launch(const char* what, const bvq_quant_desc* d, int impl, int64_t chunks, int streams, int depth, F&& f) {
  const bool nt = chunks * 16 * streams >= nt_threshold_bytes();
  const int64_t per_block = (int64_t)kWavesPerBlock * depth * kWave;
  const unsigned grid = (unsigned)((chunks + per_block - 1) / per_block);
  const int rc = with_dtype(d->x_dtype, [&](auto t) {
    return with_value<BVQ_LR_HARD_SIGMOID, BVQ_LR_SIGMOID>(
        impl, [&](auto i) { return with_bool(nt, [&](auto ntc) { return call_rc(f, t, i, ntc, grid); }); });
  });
  return rc ? rc : check_launch(what);
}

}  // namespace bvq

using namespace bvq;

extern "C" int bvq_learned_round_supported(const bvq_quant_desc* d, const void* x, const void* value, const void* y) {
  if (lr_check(d, BVQ_LR_HARD_SIGMOID, "bvq_learned_round_supported")) return 0;
  if (d->outer * d->channels * d->inner == 0) return 0;
  return x && value && aligned16(x) && aligned16(value) && aligned16(y) ? 1 : 0;
}

extern "C" int bvq_learned_round_fwd(const bvq_quant_desc* d, const void* x, const void* value, const void* scale,
                                     const void* zp, int impl, double c0, double c1, int hard, void* y,
                                     bvq_stream_t stream) {
  const char* what = "bvq_learned_round_fwd";
  int rc = lr_check(d, impl, what);
  if (rc) return rc;
  if (d->outer * d->channels * d->inner == 0) return BVQ_OK;
  rc = group_required(what, rc, {x, value, scale, zp, y});
  if ((rc = group_aligned(what, rc, {x, value, y}, "x, value and y"))) return rc;
  LrArgs a = lr_args(d, c0, c1, hard != 0);
  a.x = x;
  a.value = value;
  a.scale = scale;
  a.zp = zp;
  a.y = y;
  return lr_launch(what, d, impl, a.chunks, 3, kGroupFwdDepth, [&](auto t, auto i, auto nt, unsigned grid) {
    lr_fwd_kernel<typename decltype(t)::type, i, nt><<<grid, kBlock, 0, (hipStream_t)stream>>>(a);
  });
}

extern "C" int bvq_learned_round_bwd(const bvq_quant_desc* d, const void* g, const void* x, const void* value,
                                     const void* scale, const void* zp, int impl, double c0, double c1, void* dvalue,
                                     void* dx, bvq_stream_t stream) {
  const char* what = "bvq_learned_round_bwd";
  int rc = lr_check(d, impl, what);
  if (rc) return rc;
  if (d->outer * d->channels * d->inner == 0) return BVQ_OK;
  rc = group_required(what, rc, {g, x, value, scale, zp, dvalue});
  if ((rc = group_aligned(what, rc, {g, x, value, dvalue, dx}, "g, x, value, dvalue and dx"))) return rc;
  LrArgs a = lr_args(d, c0, c1, 0);
  a.g = g;
  a.x = x;
  a.value = value;
  a.scale = scale;
  a.zp = zp;
  a.y = dvalue;
  a.dx = dx;
  return lr_launch(what, d, impl, a.chunks, dx ? 5 : 4, kGroupBwdDepth, [&](auto t, auto i, auto nt, unsigned grid) {
    lr_bwd_kernel<typename decltype(t)::type, i, nt><<<grid, kBlock, 0, (hipStream_t)stream>>>(a);
  });
}
