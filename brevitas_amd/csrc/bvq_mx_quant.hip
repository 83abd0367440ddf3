// bvq_mx_quant.hip -- OCP Microscaling (MX) block-scaled quantizers: groups of `group_size` consecutive elements share
// one power-of-two scale, the elements are minifloats (E4M3, E5M2, E3M2, E2M3, E2M1) or MXINT8.  The definition is in
// include/bvq.h ("MX block-scaled quantizers"); every step below is exact float32 arithmetic except the final rounding
// to T.
//
// The walk is that of bvq_group_quant.hip (bvq_group_walk.h): 16-byte lane accesses, a group in L adjacent lanes, the
// abs-max key, the scale-gradient sum and the first arg-max as segmented butterflies, buffer descriptors that end with
// the tensor.  One launch each way, no LDS, no atomics, no workspace:
//   forward   reads x, writes y                   (+ 4 * groups bytes for the float32 scale)
//   backward  reads g and x, writes dx once       (+ 4 * groups bytes when a gradient arrives through the scale)
// The backward recomputes the group's abs-max and exponent from x in registers: no saved statistic is read.
// The element format is a few wave-uniform scalars (MxFormat), not a template argument: the format's arithmetic is
// the same instruction sequence for all six, so one instantiation per (T, L, NT) serves them.
#include "bvq_group_walk.h"

namespace bvq {

#ifndef BVQ_MX_FWD_DEPTH
#define BVQ_MX_FWD_DEPTH 4  // wave loads of x in flight per wave
#endif
#ifndef BVQ_MX_BWD_DEPTH
#define BVQ_MX_BWD_DEPTH 2  // wave loads of x and of g in flight per wave
#endif
constexpr int kMxFwdDepth = BVQ_MX_FWD_DEPTH;
constexpr int kMxBwdDepth = BVQ_MX_BWD_DEPTH;
constexpr int kMxEMin = -126, kMxEMax = 127;  // the scale stays a normal float32

// r = p rounded to a multiple of 2^max(floor(log2 |p|) - mbits, qe_min); MXINT8 has mbits so large that the quantum
// is always 2^qe_min
struct MxFormat {
  float max_val;
  int32_t emax, mbits, qe_min;
};

struct MxArgs {
  const void* x;
  const void* g;       // bwd
  void* y;             // fwd: y, bwd: dx
  float* scale;        // fwd: [groups] out
  const float* gscale; // bwd, nullable: gradient arriving through the returned scale, [groups]
  int64_t chunks;      // 16-byte chunks of the tensor = groups * L
  MxFormat f;
  int32_t ceil_rule, clamp_ste;
};

// the group's scale exponent from its abs-max
struct MxGroup {
  int e;        // clamped to [kMxEMin, kMxEMax]
  bool finite;  // a is neither NaN nor Inf
  bool no_da;   // a == 0, the exponent was clamped or a is not finite: nothing flows back through a
};

__device__ __forceinline__ MxGroup mx_group(float a, const MxFormat& f, bool ceil_rule) {
  const uint32_t bits = __builtin_bit_cast(uint32_t, a);
  MxGroup r;
  r.finite = bits < 0x7f800000u;
  // floor(log2 a) is a's exponent field.  A subnormal or zero a reads as -127: its true value is no larger, and both
  // land below the clamp.
  int e = (int)(bits >> 23) - 127 - f.emax;
  if (ceil_rule && ldexpf(a, -e) > f.max_val) e += 1;  // a * 2^-e is exact (scaled into [2^emax, 2^(emax + 1)))
  r.e = e < kMxEMin ? kMxEMin : (e > kMxEMax ? kMxEMax : e);
  r.no_da = r.e != e || !r.finite;
  return r;
}

// steps 3-5 on one element: p, q and inside
struct MxElem {
  float p, q;
  bool inside;
};
__device__ __forceinline__ MxElem mx_elem(float x, const MxGroup& gr, const MxFormat& f) {
  MxElem r;
  r.p = gr.finite ? ldexpf(x, -gr.e) : __builtin_nanf("");
  const int ep = (int)((__builtin_bit_cast(uint32_t, r.p) >> 23) & 0xffu) - 127;
  const int qe = ep - f.mbits > f.qe_min ? ep - f.mbits : f.qe_min;
  const float v = ldexpf(rintf(ldexpf(r.p, -qe)), qe);  // half-even on the unbounded grid; the sign survives on a zero
  r.q = v > f.max_val ? f.max_val : (v < -f.max_val ? -f.max_val : v);  // a NaN passes
  r.inside = fabsf(v) <= f.max_val;
  return r;
}

template <typename T, int L, bool NT>
__global__ __launch_bounds__(kBlock) void mx_quant_fwd_kernel(MxArgs a) {
  constexpr int VEC = elem<T>::vec, kD = kMxFwdDepth;
  GroupWindow<T, L, kD> w;
  if (!w.init(a)) return;
  const int lane = threadIdx.x & 63;
  const buf_t bx = w.elems(a.x), by = w.elems(a.y), bs = w.template groups<float>(a.scale);
  const MxFormat f = a.f;
  const bool ceil_rule = a.ceil_rule != 0;
  vec_t<T, VEC> xv[kD];
#pragma unroll
  for (int j = 0; j < kD; ++j) xv[j] = buf_load<T, VEC, NT>(bx, (uint32_t)(j * kWave + lane) * 16u);
#pragma unroll
  for (int j = 0; j < kD; ++j) {
    if ((uint32_t)(j * kWave) >= w.nch) break;  // wave-uniform: a load no lane has is not worked on
    const MxGroup gr = mx_group(key_value<T>(seg_max_u32<L>(chunk_key<T>(xv[j]))), f, ceil_rule);
    // one lane per segment writes the scale (a vector store; dropped for the groups past the end)
    const uint32_t goff = (lane & (L - 1)) == 0 ? (uint32_t)(j * (kWave / L) + lane / L) * 4u : kBufSkip;
    vec_t<float, 1> sv;
    sv.v[0] = gr.finite ? ldexpf(1.0f, gr.e) : __builtin_nanf("");
    buf_store<float, 1>(bs, goff, sv);
    vec_t<T, VEC> yv;
#pragma unroll
    for (int k = 0; k < VEC; ++k) yv.v[k] = from_f<T>(ldexpf(mx_elem(to_f<T>(xv[j].v[k]), gr, f).q, gr.e));
    buf_store<T, VEC, NT>(by, (uint32_t)(j * kWave + lane) * 16u, yv);  // dropped past the tensor's end
  }
}

template <typename T, int L, bool NT>
__global__ __launch_bounds__(kBlock) void mx_quant_bwd_kernel(MxArgs a) {
  constexpr int VEC = elem<T>::vec, kD = kMxBwdDepth;
  GroupWindow<T, L, kD> w;
  if (!w.init(a)) return;
  const int lane = threadIdx.x & 63;
  const buf_t bx = w.elems(a.x), bg = w.elems(a.g), bd = w.elems(a.y);
  // no gradient through the scale: a descriptor of no bytes, whose loads return zeros without a memory access
  const buf_t bgs = a.gscale ? w.template groups<float>(a.gscale) : make_buf(reinterpret_cast<const float*>(a.x), 0u);
  const MxFormat f = a.f;
  const bool ceil_rule = a.ceil_rule != 0, clamp_ste = a.clamp_ste != 0;
  vec_t<T, VEC> xv[kD], gv[kD];
  vec_t<float, 1> gsv[kD];
#pragma unroll
  for (int j = 0; j < kD; ++j) {
    const uint32_t off = (uint32_t)(j * kWave + lane) * 16u;
    xv[j] = buf_load<T, VEC, NT>(bx, off);
    gv[j] = buf_load<T, VEC, NT>(bg, off);
    gsv[j] = buf_load<float, 1>(bgs, (uint32_t)(j * (kWave / L) + lane / L) * 4u);  // one address per segment
  }
#pragma unroll
  for (int j = 0; j < kD; ++j) {
    if ((uint32_t)(j * kWave) >= w.nch) break;  // wave-uniform
    const uint32_t key = seg_max_u32<L>(chunk_key<T>(xv[j]));
    const float amax = key_value<T>(key);
    const MxGroup gr = mx_group(amax, f, ceil_rule);
    float acc = 0.f;
    vec_t<T, VEC> dv;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      const MxElem e = mx_elem(to_f<T>(xv[j].v[k]), gr, f);
      const bool pass = e.inside || clamp_ste;
      acc += to_f<T>(gv[j].v[k]) * (e.q - (pass ? e.p : 0.f));  // q - p is exact; the product is rounded once
      dv.v[k] = pass ? gv[j].v[k] : from_f<T>(0.f);
    }
    const float s = seg_sum<L>(acc);
    // d scale / d a = scale / a: the floor (or ceil) of the exponent is straight-through
    const float da = gr.no_da ? 0.f : (gsv[j].v[0] + s) * (ldexpf(1.0f, gr.e) / amax);
    // first element of the group whose |x| is the abs-max: segment-wide minimum over lane * VEC + index
    const uint32_t e0 = (uint32_t)(lane & (L - 1)) * VEC;
    uint32_t first = ~0u;
#pragma unroll
    for (int k = VEC - 1; k >= 0; --k) first = abs_bits<T>(xv[j].v[k]) == key ? e0 + k : first;
    first = gr.no_da ? ~0u : seg_min_u32<L>(first);
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      const float dep = to_f<T>(dv.v[k]) + (to_f<T>(xv[j].v[k]) < 0.f ? -da : da);
      dv.v[k] = first == e0 + k ? from_f<T>(dep) : dv.v[k];
    }
    buf_store<T, VEC, NT>(bd, (uint32_t)(j * kWave + lane) * 16u, dv);
  }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
// {max_val, emax, mbits, qe_min = emin - mbits} in the order of bvq_mx_format.  MXINT8: k / 64, so a fixed quantum of
// 2^-6 (mbits above every exponent difference) and emax 0.
static const MxFormat kMxFormats[] = {
    {448.0f, 8, 3, -6 - 3}, {57344.0f, 15, 2, -14 - 2}, {28.0f, 4, 2, -2 - 2},
    {7.5f, 2, 3, 0 - 3},    {6.0f, 2, 1, 0 - 1},        {127.0f / 64.0f, 0, 512, -6}};

// what the kernels cover, apart from the pointers: BVQ_OK, or the error with its text
static int mx_check(int dtype, int64_t groups, int group_size, int format, int scale_rule, const char* what) {
  if (dtype != BVQ_F32 && dtype != BVQ_BF16 && dtype != BVQ_F16) {
    set_error("%s: dtype %d (float32, bfloat16 or float16)", what, dtype);
    return BVQ_ERR_UNSUPPORTED;
  }
  if (group_size != 16 && group_size != 32 && group_size != 64 && group_size != 128 && group_size != 256) {
    set_error("%s: group size %d (16, 32, 64, 128 or 256)", what, group_size);
    return BVQ_ERR_UNSUPPORTED;
  }
  if (format < BVQ_MX_E4M3 || format > BVQ_MX_INT8) {
    set_error("%s: element format %d (bvq_mx_format)", what, format);
    return BVQ_ERR_UNSUPPORTED;
  }
  if (scale_rule != BVQ_MX_FLOOR && scale_rule != BVQ_MX_CEIL) {
    set_error("%s: scale rule %d (bvq_mx_scale_rule)", what, scale_rule);
    return BVQ_ERR_UNSUPPORTED;
  }
  if (groups < 1) {
    set_error("%s: %lld groups", what, (long long)groups);
    return BVQ_ERR_INVALID;
  }
  return BVQ_OK;
}

static MxArgs mx_args(int dtype, int64_t groups, int group_size, int format, int scale_rule) {
  MxArgs a = {};
  a.chunks = groups * (group_size * dtype_size(dtype) / 16);
  a.f = kMxFormats[format];
  a.ceil_rule = scale_rule == BVQ_MX_CEIL;
  return a;
}

}  // namespace bvq

using namespace bvq;

extern "C" int bvq_mx_quant_supported(int dtype, int64_t groups, int group_size, int format, const void* x) {
  if (mx_check(dtype, groups, group_size, format, BVQ_MX_FLOOR, "bvq_mx_quant_supported")) return 0;
  return x && aligned16(x) ? 1 : 0;
}

extern "C" int bvq_mx_quant_fwd(int dtype, int64_t groups, int group_size, int format, int scale_rule, const void* x,
                                void* y, void* scale, bvq_stream_t stream) {
  int rc = mx_check(dtype, groups, group_size, format, scale_rule, "bvq_mx_quant_fwd");
  if (rc) return rc;
  if (!x || !y || !scale) {
    set_error("bvq_mx_quant_fwd: null pointer");
    return BVQ_ERR_INVALID;
  }
  if (!aligned16(x) || !aligned16(y) || !aligned16(scale)) {
    set_error("bvq_mx_quant_fwd: x, y and scale must lie on 16-byte boundaries");
    return BVQ_ERR_UNSUPPORTED;
  }
  MxArgs a = mx_args(dtype, groups, group_size, format, scale_rule);
  a.x = x;
  a.y = y;
  a.scale = static_cast<float*>(scale);
  const bool nt = a.chunks * 32 >= nt_threshold_bytes();  // x read + y written
  rc = with_group_variant(dtype, group_size, nt, [&](auto t, auto l, auto ntc) {
    mx_quant_fwd_kernel<typename decltype(t)::type, l, ntc>
        <<<group_grid(a.chunks, kMxFwdDepth), kBlock, 0, (hipStream_t)stream>>>(a);
  });
  return rc ? rc : check_launch("bvq_mx_quant_fwd");
}

extern "C" int bvq_mx_quant_bwd(int dtype, int64_t groups, int group_size, int format, int scale_rule, int clamp_ste,
                                const void* g, const void* x, const void* gscale, void* dx, bvq_stream_t stream) {
  int rc = mx_check(dtype, groups, group_size, format, scale_rule, "bvq_mx_quant_bwd");
  if (rc) return rc;
  if (!g || !x || !dx) {
    set_error("bvq_mx_quant_bwd: null pointer");
    return BVQ_ERR_INVALID;
  }
  if (!aligned16(g) || !aligned16(x) || !aligned16(dx) || !aligned16(gscale)) {
    set_error("bvq_mx_quant_bwd: g, x, gscale and dx must lie on 16-byte boundaries");
    return BVQ_ERR_UNSUPPORTED;
  }
  MxArgs a = mx_args(dtype, groups, group_size, format, scale_rule);
  a.x = x;
  a.g = g;
  a.y = dx;
  a.gscale = static_cast<const float*>(gscale);
  a.clamp_ste = clamp_ste != 0;
  const bool nt = a.chunks * 48 >= nt_threshold_bytes();  // g and x read, dx written
  rc = with_group_variant(dtype, group_size, nt, [&](auto t, auto l, auto ntc) {
    mx_quant_bwd_kernel<typename decltype(t)::type, l, ntc>
        <<<group_grid(a.chunks, kMxBwdDepth), kBlock, 0, (hipStream_t)stream>>>(a);
  });
  return rc ? rc : check_launch("bvq_mx_quant_bwd");
}
