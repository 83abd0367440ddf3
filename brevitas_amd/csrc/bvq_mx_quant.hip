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
//   encode    reads x, writes bits / 8 bytes per element of packed codes and one E8M0 byte per group
//   decode    reads those, writes y once
// The backward recomputes the group's abs-max and exponent from x in registers: no saved statistic is read.
// The element format is a few wave-uniform scalars (MxFormat), not a template argument: the format's arithmetic is
// the same instruction sequence for all six, so one instantiation per (T, L, NT) serves them.
#include "bvq_group_walk.h"

namespace bvq {

constexpr int kMxEMin = -126, kMxEMax = 127;  // the scale stays a normal float32

// r = p rounded to a multiple of 2^max(floor(log2 |p|) - mbits, qe_min); MXINT8 has mbits so large that the quantum
// is always 2^qe_min
struct MxFormat {
  float max_val;
  int32_t emax, mbits, qe_min;
};

struct MxArgs : WalkArgs {
  float* scale;         // fwd: [groups] out
  const float* gscale;  // bwd, nullable: gradient arriving through the returned scale, [groups]
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

// steps 3 and 4 on one element: p, and r as the integer n = r / 2^qe on the quantum 2^qe
struct MxRound {
  float p, n;
  int qe;
};
__device__ __forceinline__ MxRound mx_round(float x, const MxGroup& gr, const MxFormat& f) {
  MxRound r;
  r.p = gr.finite ? ldexpf(x, -gr.e) : __builtin_nanf("");
  const int ep = (int)((__builtin_bit_cast(uint32_t, r.p) >> 23) & 0xffu) - 127;
  r.qe = ep - f.mbits > f.qe_min ? ep - f.mbits : f.qe_min;
  r.n = rintf(ldexpf(r.p, -r.qe));  // half-even on the unbounded grid; the sign survives on a zero
  return r;
}

// steps 3-5 on one element: p, q and inside
struct MxElem {
  float p, q;
  bool inside;
};
__device__ __forceinline__ MxElem mx_elem(float x, const MxGroup& gr, const MxFormat& f) {
  const MxRound t = mx_round(x, gr, f);
  MxElem r;
  r.p = t.p;
  const float v = ldexpf(t.n, t.qe);
  r.q = v > f.max_val ? f.max_val : (v < -f.max_val ? -f.max_val : v);  // a NaN passes
  r.inside = fabsf(v) <= f.max_val;
  return r;
}

// the MX quantizer on the frame of bvq_group_walk.h
template <typename T, int L>
struct MxQuant {
  using Args = MxArgs;
  using Vec = vec_t<T, elem<T>::vec>;
  static constexpr int VEC = elem<T>::vec;
  struct Side {
    float gscale;
  };
  const buf_t bs, bgs;
  const MxFormat f;
  const bool ceil_rule, clamp_ste;
  template <typename W>
  __device__ __forceinline__ MxQuant(const Args& a, const W& w)
      : bs(w.template groups<float>(a.scale)), bgs(w.template groups_or_zeros<float>(a.gscale, a.x)), f(a.f),
        ceil_rule(a.ceil_rule != 0), clamp_ste(a.clamp_ste != 0) {}

  __device__ __forceinline__ Vec fwd(const Vec& xv, const GroupPlace& p) const {
    const MxGroup gr = mx_group(key_value<T>(seg_max_u32<L>(chunk_key<T>(xv))), f, ceil_rule);
    store_group(bs, p, gr.finite ? ldexpf(1.0f, gr.e) : __builtin_nanf(""));
    Vec yv;
#pragma unroll
    for (int k = 0; k < VEC; ++k) yv.v[k] = from_f<T>(ldexpf(mx_elem(to_f<T>(xv.v[k]), gr, f).q, gr.e));
    return yv;
  }

  __device__ __forceinline__ Side side(const GroupPlace& p) const { return {load_group<float>(bgs, p)}; }
  __device__ __forceinline__ Vec bwd(const Vec& xv, const Vec& gv, const Side& sd, const GroupPlace& p) const {
    const uint32_t key = seg_max_u32<L>(chunk_key<T>(xv));
    const float amax = key_value<T>(key);
    const MxGroup gr = mx_group(amax, f, ceil_rule);
    float acc = 0.f;
    Vec dv;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      const MxElem e = mx_elem(to_f<T>(xv.v[k]), gr, f);
      const bool pass = e.inside || clamp_ste;
      acc += to_f<T>(gv.v[k]) * (e.q - (pass ? e.p : 0.f));  // q - p is exact; the product is rounded once
      dv.v[k] = pass ? gv.v[k] : from_f<T>(0.f);
    }
    const float s = seg_sum<L>(acc);
    // d scale / d a = scale / a: the floor (or ceil) of the exponent is straight-through
    const float da = gr.no_da ? 0.f : (sd.gscale + s) * (ldexpf(1.0f, gr.e) / amax);
    // first element of the group whose |x| is the abs-max: segment-wide minimum over lane * VEC + index
    const uint32_t e0 = p.sub * VEC;
    uint32_t first = ~0u;
#pragma unroll
    for (int k = VEC - 1; k >= 0; --k) first = abs_bits<T>(xv.v[k]) == key ? e0 + k : first;
    first = gr.no_da ? ~0u : seg_min_u32<L>(first);
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      const float dep = to_f<T>(dv.v[k]) + (to_f<T>(xv.v[k]) < 0.f ? -da : da);
      dv.v[k] = first == e0 + k ? from_f<T>(dep) : dv.v[k];
    }
    return dv;
  }
};

// ------------------------------------------------------------------------------------------------
// the wire format (include/bvq.h, "MX wire format"): packed element codes and E8M0 scale bytes
// ------------------------------------------------------------------------------------------------
// A lane's 16-byte chunk of x becomes W = VEC * bits code bits (16 .. 64), so a wave load of x becomes a dense stream
// of 64 * W bits = 2 * W dwords.  The lanes below W / 2 each receive four consecutive dwords of that stream from the
// lanes that hold them (stream_dwords) and store 16 bytes; the scale bytes of a load are gathered into dwords too.
//   encode  reads x once, writes bits / 8 bytes per element and one byte per group
//   decode  reads those, writes y once
// No LDS, no atomics, no workspace; the descriptors of the outputs end with the outputs.

// the code's fields: sign on top, then exponent (bias), then mbits of mantissa; emin = 1 - bias
struct MxCode {
  int32_t width, mbits, bias;
  int32_t max_code;  // the magnitude code of max_val
  int32_t special;   // 0 none, 1 E4M3 (S.1111.111 is NaN), 2 E5M2 (exponent field 31 is Inf / NaN), 3 MXINT8
};

struct MxPackArgs : WalkArgs {  // x: encode, y: decode
  void* codes;
  void* scale;  // E8M0 bytes, [groups]
  MxFormat f;
  MxCode c;
  int32_t ceil_rule, lanes_log2;
};

// The element code of q = clamp(n * 2^qe) from the rounding's own n and qe (mx_round), without forming q: a normal
// value has n in [2^mbits, 2^(mbits + 1)] and the exponent field qe - qe_min + 1, a subnormal one has qe = qe_min and
// n below 2^mbits, so the magnitude code is ((qe - qe_min) << mbits) + |n| for both (n = 2^(mbits + 1), a rounding that
// carried, lands on the next exponent with a zero mantissa); codes are ordered like magnitudes, so the clamp to max_val
// is a min with its code.  MXINT8: qe is always -6 and n is k before the clamp.  A group that is not finite gives
// some code here; the caller writes zeros for it.
__device__ __forceinline__ uint32_t mx_code(const MxRound& t, const MxFormat& f, const MxCode& c) {
  if (c.special == 3) {
    const float k = t.n > 127.0f ? 127.0f : (t.n < -127.0f ? -127.0f : t.n);
    return (uint32_t)(int)k & 0xffu;  // a negative zero becomes 0
  }
  const uint32_t mag = ((uint32_t)(t.qe - f.qe_min) << c.mbits) + (uint32_t)fabsf(t.n);
  const uint32_t top = (uint32_t)c.max_code;
  return (mag < top ? mag : top) | ((__builtin_bit_cast(uint32_t, t.n) >> 31) << (c.width - 1));
}

// the value of any code of the format
__device__ __forceinline__ float mx_code_value(uint32_t code, const MxCode& c) {
  if (c.special == 3) return (float)(int)(int8_t)(code & 0xffu) * (1.0f / 64.0f);
  const uint32_t mag = code & ((1u << (c.width - 1)) - 1u), ef = mag >> c.mbits, m = mag & ((1u << c.mbits) - 1u);
  uint32_t bits = (mag << (23 - c.mbits)) + ((uint32_t)(127 - c.bias) << 23);
  if (ef == 0) bits = __builtin_bit_cast(uint32_t, ldexpf((float)m, 1 - c.bias - c.mbits));
  if (c.special == 1 && mag == 0x7fu) bits = 0x7fc00000u;
  if (c.special == 2 && ef == 31u) bits = m ? 0x7fc00000u : 0x7f800000u;
  return __builtin_bit_cast(float, bits | (((code >> (c.width - 1)) & 1u) << 31));
}

__device__ __forceinline__ uint32_t lane_get(uint32_t v, int src) { return (uint32_t)__shfl((int)v, src & 63, kWave); }

// The wave load's code stream, in which lane i's W bits `c` sit at bit i * W, as the four dwords 4 s .. 4 s + 3 in every
// lane s below W / 2.  One DPP move from the next lane first makes every dword of the stream whole in one lane (A:
// dword DA, B: dword DA + 1, where the lane has them); then one forward permute per slot k: every lane sends the
// dword whose index is k mod 4 to lane index / 4, or nothing (to lane 63, which stores nothing).
template <int W>
__device__ __forceinline__ vec_t<uint32_t, 4> stream_dwords(uint64_t c, int lane) {
  const uint32_t lo = (uint32_t)c, hi = (uint32_t)(c >> 32);
  // quad_perm [1, 2, 3, 3]: the low dword of the next lane of the quad
  const uint32_t next = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)lo, 0xF9, 0xf, 0xf, false);
  uint32_t A, B = 0;
  int DA;
  bool hasA = true, hasB = false;
  if constexpr (W == 64) {
    A = lo, B = hi, DA = 2 * lane, hasB = true;
  } else if constexpr (W == 32) {
    A = lo, DA = lane;
  } else if constexpr (W == 48) {  // two lanes are three dwords
    const bool odd = lane & 1;
    A = odd ? (uint32_t)(c >> 16) : lo;
    B = hi | (next << 16);
    DA = 3 * (lane >> 1) + (odd ? 2 : 0);
    hasB = !odd;
  } else if constexpr (W == 16) {  // two lanes are one dword
    A = lo | (next << 16);
    DA = lane >> 1;
    hasA = !(lane & 1);
  } else {  // 24: four lanes are three dwords
    static_assert(W == 24, "16, 24, 32, 48 or 64 code bits per lane");
    const int r = lane & 3;
    A = (lo >> (8 * r)) | (next << (24 - 8 * r));
    DA = 3 * (lane >> 2) + r;
    hasA = r != 3;
  }
  vec_t<uint32_t, 4> out;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const bool a = hasA && (DA & 3) == k, b = hasB && ((DA + 1) & 3) == k;
    const int dst = a ? DA >> 2 : (b ? (DA + 1) >> 2 : 63);
    out.v[k] = (uint32_t)__builtin_amdgcn_ds_permute(dst << 2, (int)(b ? B : A));
  }
  return out;
}

// a dword of scale bytes at byte `off` of a window of `ngr` scale bytes: whole when it fits, else its leading bytes
__device__ __forceinline__ void store_scale_dword(buf_t bs, uint32_t off, uint32_t v, uint32_t ngr) {
  if (off != kBufSkip && off + 4u > ngr) {  // at most one lane of the launch: the tensor's last, ragged dword
#pragma unroll
    for (int k = 0; k < 3; ++k)
      if (off + k < ngr) __builtin_amdgcn_raw_buffer_store_b8((unsigned char)(v >> (8 * k)), bs, off + k, 0, 0);
  } else {
    vec_t<uint32_t, 1> sv;
    sv.v[0] = v;
    buf_store<uint32_t, 1>(bs, off, sv);
  }
}

template <typename T, int L, bool NT, int BITS>
__global__ __launch_bounds__(kBlock) void mx_encode_kernel(MxPackArgs a) {
  constexpr int VEC = elem<T>::vec, kD = kGroupFwdDepth, W = VEC * BITS, GL = kWave / L;  // GL groups per load
  GroupWindow<T, L, kD> w;
  if (!w.init(a)) return;
  const int lane = threadIdx.x & 63;
  const buf_t bx = w.elems(a.x);
  const buf_t bc = make_buf(reinterpret_cast<const uint8_t*>(a.codes) + w.c0 * (W / 8), w.nch * (uint32_t)(W / 8));
  const buf_t bs = w.template groups<uint8_t>(a.scale);
  const MxFormat f = a.f;
  const MxCode cf = a.c;
  const bool ceil_rule = a.ceil_rule != 0;
  vec_t<T, VEC> xv[kD];
#pragma unroll
  for (int j = 0; j < kD; ++j) xv[j] = buf_load<T, VEC, NT>(bx, (uint32_t)(j * kWave + lane) * 16u);
  uint32_t held[2] = {0u, 0u};  // GL < 4: the window's kD * GL scale bytes, collected over its loads (lane 0 stores)
#pragma unroll
  for (int j = 0; j < kD; ++j) {
    if ((uint32_t)(j * kWave) >= w.nch) break;  // wave-uniform
    const MxGroup gr = mx_group(key_value<T>(seg_max_u32<L>(chunk_key<T>(xv[j]))), f, ceil_rule);
    // ---- scale bytes: GL adjacent bytes per load
    uint32_t sb = gr.finite ? (uint32_t)(gr.e + 127) : 0xffu;
    if constexpr (GL >= 4) {
      sb |= lane_get(sb, lane + L) << 8;
      sb |= lane_get(sb, lane + 2 * L) << 16;
      store_scale_dword(bs, (lane & (4 * L - 1)) == 0 ? (uint32_t)(j * GL + lane / L) : kBufSkip, sb, w.ngr);
    } else {
      if constexpr (GL == 2) sb |= lane_get(sb, lane + L) << 8;
      held[j * GL / 4] |= sb << (8 * (j * GL % 4));
    }
    // ---- element codes: this lane's W bits, then four dwords of the load's stream
    uint64_t c = 0;
#pragma unroll
    for (int k = 0; k < VEC; ++k) c |= (uint64_t)mx_code(mx_round(to_f<T>(xv[j].v[k]), gr, f), f, cf) << (k * BITS);
    const vec_t<uint32_t, 4> cv = stream_dwords<W>(gr.finite ? c : 0ull, lane);
    const uint32_t left = w.nch - (uint32_t)(j * kWave);
    const uint32_t bytes = (left < (uint32_t)kWave ? left : (uint32_t)kWave) * (uint32_t)(W / 8);  // of this load
    const uint32_t off = (uint32_t)j * (kWave * W / 8) + (uint32_t)lane * 16u;
    if ((bytes & 15u) == 0) {  // wave-uniform: every 16 bytes are inside or outside as a whole
      buf_store<uint32_t, 4, NT>(bc, lane < W / 2 ? off : kBufSkip, cv);
    } else {  // the tensor's last load ends inside 16 bytes: dwords, each inside or outside as a whole
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        vec_t<uint32_t, 1> one;
        one.v[0] = cv.v[d];
        buf_store<uint32_t, 1>(bc, lane < W / 2 ? off + 4u * d : kBufSkip, one);
      }
    }
  }
  if constexpr (GL < 4) {
    static_assert(kD * GL <= 8 && kD * GL % 4 == 0, "the window's scale bytes are one or two dwords");
#pragma unroll
    for (int k = 0; k < kD * GL / 4; ++k) store_scale_dword(bs, lane == 0 ? 4u * k : kBufSkip, held[k], w.ngr);
  }
}

// W bits at bit lane * W of the load's code stream, whose dwords 4 s .. 4 s + 3 lane s holds in r
template <int W>
__device__ __forceinline__ uint64_t stream_bits(const vec_t<uint32_t, 4>& r, int lane) {
  const int D0 = lane * W >> 5, o = lane * W & 31;
  auto dword = [&](int D) {  // every lane reads one lane's four dwords and keeps its own
    const uint32_t t0 = lane_get(r.v[0], D >> 2), t1 = lane_get(r.v[1], D >> 2);
    const uint32_t t2 = lane_get(r.v[2], D >> 2), t3 = lane_get(r.v[3], D >> 2);
    return D & 2 ? (D & 1 ? t3 : t2) : (D & 1 ? t1 : t0);
  };
  uint64_t v = dword(D0);
  if constexpr (W != 16 && W != 32) v |= (uint64_t)dword(D0 + 1) << 32;
  v >>= o;
  return W == 64 ? v : v & ((1ull << (W & 63)) - 1ull);
}

// T and the lanes per group are all the kernel needs of the walk; the lanes per group are a shift, not a template
// argument: there is no segmented reduction here
template <typename T, bool NT, int BITS>
__global__ __launch_bounds__(kBlock) void mx_decode_kernel(MxPackArgs a) {
  constexpr int VEC = elem<T>::vec, kD = kGroupFwdDepth, W = VEC * BITS;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t c0 = ((int64_t)blockIdx.x * kWavesPerBlock + wave) * (kD * kWave);
  if (c0 >= a.chunks) return;
  const int64_t rest = a.chunks - c0;
  const uint32_t nch = (uint32_t)(rest < kD * kWave ? rest : kD * kWave), ngr = nch >> a.lanes_log2;
  const int lane = threadIdx.x & 63;
  const buf_t by = make_buf(reinterpret_cast<const T*>(a.y) + c0 * VEC, nch * 16u);
  const buf_t bc = make_buf(reinterpret_cast<const uint8_t*>(a.codes) + c0 * (W / 8), nch * (uint32_t)(W / 8));
  const buf_t bs = make_buf(reinterpret_cast<const uint8_t*>(a.scale) + (c0 >> a.lanes_log2), ngr);
  const MxCode cf = a.c;
  vec_t<uint32_t, 4> cv[kD];
  uint32_t sb[kD];
#pragma unroll
  for (int j = 0; j < kD; ++j) {
    const uint32_t left = nch > (uint32_t)(j * kWave) ? nch - (uint32_t)(j * kWave) : 0u;
    const uint32_t bytes = (left < (uint32_t)kWave ? left : (uint32_t)kWave) * (uint32_t)(W / 8);
    const uint32_t off = (uint32_t)j * (kWave * W / 8) + (uint32_t)lane * 16u;
    if ((bytes & 15u) == 0) {  // wave-uniform, as in the encoder
      cv[j] = buf_load<uint32_t, 4, NT>(bc, lane < W / 2 ? off : kBufSkip);
    } else {
#pragma unroll
      for (int d = 0; d < 4; ++d) cv[j].v[d] = buf_load<uint32_t, 1>(bc, lane < W / 2 ? off + 4u * d : kBufSkip).v[0];
    }
    // one address per group; past the end a zero
    sb[j] = __builtin_amdgcn_raw_buffer_load_b8(bs, ((uint32_t)(j * kWave + lane)) >> a.lanes_log2, 0, 0);
  }
#pragma unroll
  for (int j = 0; j < kD; ++j) {
    if ((uint32_t)(j * kWave) >= nch) break;  // wave-uniform
    const uint64_t c = stream_bits<W>(cv[j], lane);
    const int e = (int)sb[j] - 127;
    vec_t<T, VEC> yv;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      const float v = mx_code_value((uint32_t)(c >> (k * BITS)) & ((1u << BITS) - 1u), cf);
      yv.v[k] = from_f<T>(sb[j] == 0xffu ? __builtin_nanf("") : ldexpf(v, e));  // v * 2^e, exact
    }
    buf_store<T, VEC, NT>(by, (uint32_t)(j * kWave + lane) * 16u, yv);  // dropped past the tensor's end
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

// {width, mbits, bias, max_code, special} in the order of bvq_mx_format
static const MxCode kMxCodes[] = {{8, 3, 7, 0x7e, 1}, {8, 2, 15, 0x7b, 2}, {6, 2, 3, 0x1f, 0},
                                  {6, 3, 1, 0x1f, 0}, {4, 1, 1, 0x7, 0},    {8, 6, 0, 127, 3}};

static MxPackArgs mx_pack_args(int dtype, int64_t groups, int group_size, int format, int scale_rule) {
  MxPackArgs a = {};
  const int lanes = group_size * dtype_size(dtype) / 16;
  a.chunks = groups * lanes;
  a.f = kMxFormats[format];
  a.c = kMxCodes[format];
  a.ceil_rule = scale_rule == BVQ_MX_CEIL;
  a.lanes_log2 = __builtin_ctz((unsigned)lanes);
  return a;
}

// f(int_c<bits>) for the code width of a format
template <typename F>
static int with_code_bits(int format, F&& f) {
  return with_value<4, 6, 8>(kMxCodes[format].width, f);
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
  const char* what = "bvq_mx_quant_fwd";
  int rc = group_required(what, mx_check(dtype, groups, group_size, format, scale_rule, what), {x, y, scale});
  if ((rc = group_aligned(what, rc, {x, y, scale}, "x, y and scale"))) return rc;
  MxArgs a = mx_args(dtype, groups, group_size, format, scale_rule);
  a.x = x;
  a.y = y;
  a.scale = static_cast<float*>(scale);
  // x read + y written
  return group_launch(what, dtype, group_size, a.chunks, 32, kGroupFwdDepth, [&](auto t, auto l, auto nt, unsigned grid) {
    group_fwd_kernel<MxQuant, typename decltype(t)::type, l, nt><<<grid, kBlock, 0, (hipStream_t)stream>>>(a);
  });
}

extern "C" int bvq_mx_quant_bwd(int dtype, int64_t groups, int group_size, int format, int scale_rule, int clamp_ste,
                                const void* g, const void* x, const void* gscale, void* dx, bvq_stream_t stream) {
  const char* what = "bvq_mx_quant_bwd";
  int rc = group_required(what, mx_check(dtype, groups, group_size, format, scale_rule, what), {g, x, dx});
  if ((rc = group_aligned(what, rc, {g, x, dx, gscale}, "g, x, gscale and dx"))) return rc;
  MxArgs a = mx_args(dtype, groups, group_size, format, scale_rule);
  a.x = x;
  a.g = g;
  a.y = dx;
  a.gscale = static_cast<const float*>(gscale);
  a.clamp_ste = clamp_ste != 0;
  // g and x read, dx written
  return group_launch(what, dtype, group_size, a.chunks, 48, kGroupBwdDepth, [&](auto t, auto l, auto nt, unsigned grid) {
    group_bwd_kernel<MxQuant, typename decltype(t)::type, l, nt><<<grid, kBlock, 0, (hipStream_t)stream>>>(a);
  });
}

extern "C" int bvq_mx_encode_supported(int dtype, int64_t groups, int group_size, int format, const void* x) {
  if (mx_check(dtype, groups, group_size, format, BVQ_MX_FLOOR, "bvq_mx_encode_supported")) return 0;
  return x && aligned16(x) ? 1 : 0;
}

extern "C" int bvq_mx_encode(int dtype, int64_t groups, int group_size, int format, int scale_rule, const void* x,
                             void* codes, void* scale_e8m0, bvq_stream_t stream) {
  const char* what = "bvq_mx_encode";
  int rc = group_required(what, mx_check(dtype, groups, group_size, format, scale_rule, what), {x, codes, scale_e8m0});
  if ((rc = group_aligned(what, rc, {x, codes, scale_e8m0}, "x, codes and scale_e8m0"))) return rc;
  MxPackArgs a = mx_pack_args(dtype, groups, group_size, format, scale_rule);
  a.x = x;
  a.codes = codes;
  a.scale = scale_e8m0;
  // the policy of the forward, on the same x
  return group_launch(what, dtype, group_size, a.chunks, 32, kGroupFwdDepth, [&](auto t, auto l, auto nt, unsigned grid) {
    return with_code_bits(format, [&](auto b) {
      mx_encode_kernel<typename decltype(t)::type, l, nt, b><<<grid, kBlock, 0, (hipStream_t)stream>>>(a);
    });
  });
}

extern "C" int bvq_mx_decode(int dtype, int64_t groups, int group_size, int format, const void* codes,
                             const void* scale_e8m0, void* y, bvq_stream_t stream) {
  const char* what = "bvq_mx_decode";
  int rc = group_required(what, mx_check(dtype, groups, group_size, format, BVQ_MX_FLOOR, what), {codes, scale_e8m0, y});
  if ((rc = group_aligned(what, rc, {codes, scale_e8m0, y}, "codes, scale_e8m0 and y"))) return rc;
  MxPackArgs a = mx_pack_args(dtype, groups, group_size, format, BVQ_MX_FLOOR);
  a.y = y;
  a.codes = const_cast<void*>(codes);
  a.scale = const_cast<void*>(scale_e8m0);
  // the kernel takes the lanes per group from its arguments: one instantiation serves every L
  return group_launch(what, dtype, group_size, a.chunks, 32, kGroupFwdDepth, [&](auto t, auto, auto nt, unsigned grid) {
    return with_code_bits(format, [&](auto b) {
      mx_decode_kernel<typename decltype(t)::type, nt, b><<<grid, kBlock, 0, (hipStream_t)stream>>>(a);
    });
  });
}
