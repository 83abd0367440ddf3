// bvq_fakequant_fwd.hip -- fused affine quantize/dequantize: the forward kernels and their entry points.
//
// Replaces the ~9 full-tensor ATen passes of IntQuant.forward (B/core/quant/int_base.py:63-97)
// with one read of x and one write of y, and the ~8 passes autograd runs for its backward with one
// read of g, one read of x and one write of dx (the per-channel scale / zero-point gradient sums,
// and the search for the elements that attain the abs-max statistic, ride on the same reads).
// HBM-bound: algorithmic bytes per element are
//   forward  sizeof(x) + sizeof(y)          backward  sizeof(g) + sizeof(x) + sizeof(dx).

#include "bvq_act.h"
#include "bvq_fakequant.h"
#include "bvq_stat_epilogue.h"

namespace bvq {

// ------------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------------
// ZP0: the zero-point is +0.0: "+ zp" only turns -0 into +0 and "- zp" is the identity, so their
// re-roundings are skipped (the values are already representable).
template <typename CT, int RM, bool ZP0, typename Div>
__device__ __forceinline__ float fwd_elem(float xf, const Div& div, float s, float z, float qmin,
                                          float qmax, bool out_int, int mode, float& q_out) {
  float t = rnd<CT>(div(xf));                  // y = x / scale            int_base.py:69
  t = ZP0 ? t + 0.f : rnd<CT>(t + z);          // y = y + zero_point       :70
  t = do_round<CT, RM>(t, mode);               // y = float_to_int_impl(y) :73
  const float q = clamp_where(t, qmin, qmax);  // y = tensor_clamp_impl(.) :74
  q_out = q;
  if (out_int) return q;
  return ZP0 ? rnd<CT>(q * s) : rnd<CT>(rnd<CT>(q - z) * s);  // (y_int - zero_point) * scale :93-94
}

// fwd_elem on a pair of elements (bvq_quant_math.h: packed fp32 / packed bf16 conversion)
template <typename CT, int RM, bool ZP0, typename Div, typename S>
__device__ __forceinline__ f2 fwd_elem2(f2 xf, const Div& div, S s, S z, float qmin, float qmax,
                                        bool out_int, int mode, f2& q_out) {
  f2 t = rnd2<CT>(div(xf));
  t = ZP0 ? t + 0.f : rnd2<CT>(t + z);
  t = do_round2<CT, RM>(t, mode);
  const f2 q = clamp_where2(t, qmin, qmax);
  q_out = q;
  if (out_int) return q;
  // the last rounding to CT is the caller's pack2<CT> (one v_cvt_pk_bf16_f32 for the pair)
  return ZP0 ? q * s : rnd2<CT>(q - z) * s;  // (y_int - zero_point) * scale :93-94
}

// store VEC integer codes (parity / export mode): int32, int8 or uint8
template <int VEC>
__device__ __forceinline__ void store_codes(void* base, int codes_dtype, int64_t off, const float* q) {
  if (codes_dtype == BVQ_CODES_I32) {
    vec_t<int32_t, VEC> cv;
#pragma unroll
    for (int k = 0; k < VEC; ++k) cv.v[k] = (int32_t)q[k];
    store_vec<int32_t, VEC>(reinterpret_cast<int32_t*>(base) + off, cv);
  } else if (codes_dtype == BVQ_CODES_I8) {
    vec_t<int8_t, VEC> cv;
#pragma unroll
    for (int k = 0; k < VEC; ++k) cv.v[k] = (int8_t)(int32_t)q[k];
    store_vec<int8_t, VEC>(reinterpret_cast<int8_t*>(base) + off, cv);
  } else {
    vec_t<uint8_t, VEC> cv;
#pragma unroll
    for (int k = 0; k < VEC; ++k) cv.v[k] = (uint8_t)(int32_t)q[k];
    store_vec<uint8_t, VEC>(reinterpret_cast<uint8_t*>(base) + off, cv);
  }
}

// NT: cache policy of the stores of y; NTL: of the loads of x (the same unless stated); ACT: the activation of
// bvq_act.h applied to x first (0: none; PRE is the ReLU)
template <typename XT, typename CT, int VEC, int RM, bool NT, bool ZP0, bool PRE, bool NTL = NT, int ACT = 0,
          typename Div>
__device__ __forceinline__ void fwd_unit(const QuantArgs& a, const Unit& u, const Div& div, float s,
                                         float z, float qmin, float qmax) {
  const int lane = threadIdx.x & 63;
  const XT* __restrict__ xp = reinterpret_cast<const XT*>(a.x) + u.base;
  CT* __restrict__ yp = a.y ? reinterpret_cast<CT*>(a.y) + u.base : nullptr;
  void* const cp = a.codes;  // indexed from the tensor start: u.base + offset
  const bool out_int = a.out_int != 0;
  const int mode = a.round_mode;

  ChunkCursor cur;
  cur.init(u, VEC, lane);
  const int64_t total = (int64_t)u.nrows * cur.cpr;
  for (int64_t done = 0; done < total; done += (int64_t)kWave * kUnroll) {
    vec_t<XT, VEC> xv[kUnroll];
    int64_t off[kUnroll];
    bool ok[kUnroll];
#pragma unroll
    for (int j = 0; j < kUnroll; ++j) {
      ok[j] = cur.valid();
      off[j] = cur.offset(u.row_stride, VEC);
      xv[j] = load_vec<XT, VEC, NTL>(xp + (ok[j] ? off[j] : 0));  // past the end: re-read the unit's first chunk
      cur.next();
    }
#pragma unroll
    for (int j = 0; j < kUnroll; ++j) {
      if (ok[j]) {
        vec_t<CT, VEC> yv;
        float qv[VEC];
        if constexpr (VEC % 2 == 0) {
#pragma unroll
          for (int k = 0; k < VEC; k += 2) {
            f2 xf = widen2<XT>(xv[j].v[k], xv[j].v[k + 1]);
            if constexpr (PRE) xf = relu2(xf);
            if constexpr (ACT != 0) xf = act_rnd2<XT, ACT>(xf);
            f2 q2;
            const f2 r = fwd_elem2<CT, RM, ZP0>(xf, div, s, z, qmin, qmax, out_int, mode, q2);
            pack2<CT>(r, yv.v[k], yv.v[k + 1]);
            qv[k] = q2.x;
            qv[k + 1] = q2.y;
          }
        } else {
#pragma unroll
          for (int k = 0; k < VEC; ++k) {
            float xf = PRE ? relu_f(to_f<XT>(xv[j].v[k])) : to_f<XT>(xv[j].v[k]);
            if constexpr (ACT != 0) xf = act_rnd<XT, ACT>(xf);
            const float r = fwd_elem<CT, RM, ZP0>(xf, div, s, z, qmin, qmax, out_int, mode, qv[k]);
            yv.v[k] = from_f<CT>(r);
          }
        }
        if (yp) store_vec<CT, VEC, NT>(yp + off[j], yv);
        if (cp) store_codes<VEC>(cp, a.codes_dtype, u.base + off[j], qv);  // parity / export mode only
      }
    }
  }
  // ragged ends: the (< VEC) elements after the last full chunk of every row of the unit
  const int32_t tail = (int32_t)(u.len - (int64_t)cur.cpr * VEC);
  for (int32_t e = lane; e < u.nrows * tail; e += kWave) {
    const int32_t tr = e / tail, tk = e - tr * tail;
    const int64_t i = (int64_t)tr * u.row_stride + (int64_t)cur.cpr * VEC + tk;
    float q;
    float xf = PRE ? relu_f(to_f<XT>(xp[i])) : to_f<XT>(xp[i]);
    if constexpr (ACT != 0) xf = act_rnd<XT, ACT>(xf);
    const float r = fwd_elem<CT, RM, ZP0>(xf, div, s, z, qmin, qmax, out_int, mode, q);
    if (yp) yp[i] = from_f<CT>(r);
    if (cp) store_codes<1>(cp, a.codes_dtype, u.base + i, &q);
  }
}

template <typename XT, typename CT, int VEC, int RM, bool NT, bool NTL = NT, int ACT = 0>
__global__ __launch_bounds__(kBlock) void fakequant_fwd_kernel(QuantArgs a) {
  const Unit u = locate_unit(a.t);
  if (!u.valid) return;
  float s, z;
  load_scale_zp<CT>(a, u.channel, s, z);
  // the reference clamps against min_int/max_int converted to the tensor dtype (max_val.type_as(x))
  const float qmin = rnd<CT>(a.bounds ? a.bounds[0] : a.qmin), qmax = rnd<CT>(a.bounds ? a.bounds[1] : a.qmax);
  // wave-uniform choices: fused pre-activation, zero zero-point (16-bit compute types: saves two
  // re-roundings per element), and (bf16) the reciprocal fast path
  const bool zp0 = sizeof(CT) == 2 && zp_is_pos_zero(z);
#define BVQ_FWD_UNIT(ZP0, PRE, DIV) fwd_unit<XT, CT, VEC, RM, NT, ZP0, PRE, NTL, ACT>(a, u, DIV, s, z, qmin, qmax)
#define BVQ_FWD_PRE(ZP0, DIV)      \
  do {                             \
    if constexpr (ACT != 0)        \
      BVQ_FWD_UNIT(ZP0, false, DIV); \
    else if (a.pre_relu)           \
      BVQ_FWD_UNIT(ZP0, true, DIV); \
    else                           \
      BVQ_FWD_UNIT(ZP0, false, DIV); \
  } while (0)
  if constexpr (elem<CT>::id == BVQ_BF16) {
    if (bf16_scale_ok(s)) {
      const DivBf16 div{1.0f / s};
      if (zp0)
        BVQ_FWD_PRE(true, div);
      else
        BVQ_FWD_PRE(false, div);
      return;
    }
  }
  // float16: the refined reciprocal product (DivF16R: the exact float32 quotient in 4 instructions, no branch; the
  // guarded reciprocal's wave-wide check cost 15 % here: profiles/r01_f16_fastdiv.txt)
#ifndef BVQ_F16_FWD_EXACT
  if constexpr (elem<CT>::id == BVQ_F16) {
    if (f16_scale_ok(s)) {
      const DivF16R div{s, 1.0f / s};
      if (zp0)
        BVQ_FWD_PRE(true, div);
      else
        BVQ_FWD_PRE(false, div);
      return;
    }
  }
#endif
  const DivExact div{s};
  if constexpr (sizeof(CT) == 2) {
    if (zp0) {
      BVQ_FWD_PRE(true, div);
      return;
    }
  }
  BVQ_FWD_PRE(false, div);
#undef BVQ_FWD_PRE
#undef BVQ_FWD_UNIT
}


template <typename T>
constexpr int kColsFwdVec = sizeof(T) == 2 ? kColsFwdVec16 : elem<T>::vec;

// One wave's unit of the column-mapped forward: a block of rows of its strip of 64 column chunks, addressed through buffer
// descriptors like the backward's (bvq_fakequant_bwd.h, cols_bwd_rows): rows past the block's end read zeros without a
// memory access and drop their stores, so the walk has no execution mask and no 64-bit address arithmetic; the fused ReLU
// is a template parameter; a lane holds 4 columns of a 16-bit type (8-byte loads: half the per-column scales /
// reciprocals / zero-points to fetch and divide at the start of every unit, half the registers).
template <typename T, int RM, bool NT, bool ZP0, bool FAST, bool PRE>
__device__ __forceinline__ void cols_fwd_rows(const ColsQuantArgs& a, const ColsLane<T, kColsFwdVec<T>>& ln, float qmin,
                                              float qmax) {
  constexpr int VEC = kColsFwdVec<T>;
#ifndef BVQ_COLS_FWD_UNROLL
#define BVQ_COLS_FWD_UNROLL 4  // rows in flight per lane
#endif
  constexpr int kU = BVQ_COLS_FWD_UNROLL;
  const int64_t nrows = ln.row_end - ln.blk0;  // wave-uniform, > 0
  const uint32_t bytes = (uint32_t)(nrows * a.p.L * (int64_t)sizeof(T));
  const buf_t bx = make_buf(reinterpret_cast<const T*>(a.x) + ln.blk0 * a.p.L, bytes);
  const buf_t by = make_buf(reinterpret_cast<T*>(a.y) + ln.blk0 * a.p.L, bytes);
  const uint32_t step = (uint32_t)((int64_t)a.p.rpp * a.p.L * (int64_t)sizeof(T));  // between a lane's consecutive rows
  uint32_t off = (uint32_t)(((int64_t)ln.sub * a.p.L + (int64_t)ln.chunk * VEC) * (int64_t)sizeof(T));
  const int32_t steps = (int32_t)((nrows + a.p.rpp - 1) / a.p.rpp);  // rows per lane, the last possibly past the end
  f2 r2[VEC / 2];
#pragma unroll
  for (int k = 0; k < VEC / 2; ++k) r2[k] = f2{1.0f / ln.s2[k].x, 1.0f / ln.s2[k].y};
  const int mode = a.round_mode;
  for (int32_t i = 0; i < steps; i += kU) {
    vec_t<T, VEC> xv[kU];
#pragma unroll
    for (int j = 0; j < kU; ++j) xv[j] = buf_load<T, VEC, NT>(bx, off + (uint32_t)j * step);
#pragma unroll
    for (int j = 0; j < kU; ++j) {
      if (i + j < steps) {  // wave-uniform
        vec_t<T, VEC> yv;
#pragma unroll
        for (int k = 0; k < VEC; k += 2) {
          f2 xf = widen2<T>(xv[j].v[k], xv[j].v[k + 1]);
          if constexpr (PRE) xf = relu2(xf);
          f2 q2, res;
          if constexpr (FAST && elem<T>::id == BVQ_F16)
            res = fwd_elem2<T, RM, ZP0>(xf, BVQ_DIVF16V{ln.s2[k / 2], r2[k / 2]}, ln.s2[k / 2], ln.z2[k / 2], qmin, qmax, false,
                                        mode, q2);
          else if constexpr (FAST)
            res = fwd_elem2<T, RM, ZP0>(xf, DivBf16V{r2[k / 2]}, ln.s2[k / 2], ln.z2[k / 2], qmin, qmax, false, mode, q2);
          else
            res = fwd_elem2<T, RM, ZP0>(xf, DivExactV{ln.s2[k / 2]}, ln.s2[k / 2], ln.z2[k / 2], qmin, qmax, false, mode, q2);
          pack2<T>(res, yv.v[k], yv.v[k + 1]);
        }
        buf_store<T, VEC, NT>(by, off + (uint32_t)j * step, yv);  // dropped past the block's end
      }
    }
    off += (uint32_t)kU * step;
  }
}

template <typename T, int RM, bool NT>
__global__ __launch_bounds__(kBlock) void fakequant_fwd_cols_kernel(ColsQuantArgs a) {
  ColsLane<T, kColsFwdVec<T>> ln;
  if (!ln.init(a) || !ln.active) return;
  const float qmin = rnd<T>(a.qmin), qmax = rnd<T>(a.qmax);
#define BVQ_COLS_FWD(ZP0, FAST)                                \
  do {                                                         \
    if (a.pre_relu)                                            \
      cols_fwd_rows<T, RM, NT, ZP0, FAST, true>(a, ln, qmin, qmax);  \
    else                                                       \
      cols_fwd_rows<T, RM, NT, ZP0, FAST, false>(a, ln, qmin, qmax); \
  } while (0)
  if constexpr (sizeof(T) == 2) {
    if (ln.fast) {
      if (ln.zp0)
        BVQ_COLS_FWD(true, true);
      else
        BVQ_COLS_FWD(false, true);
      return;
    }
    if (ln.zp0) {
      BVQ_COLS_FWD(true, false);
      return;
    }
  }
  BVQ_COLS_FWD(false, false);
#undef BVQ_COLS_FWD
}

// ------------------------------------------------------------------------------------------------
// statistic + quantizer in ONE kernel, small channels: the channel stays in registers between the two
// ------------------------------------------------------------------------------------------------
// AbsMax -> clamp_min -> / int_threshold -> IntQuant (zero zero-point): the stats-scaled graphs of
// SURVEY 8a.  The two-kernel form reads x twice (statistic, then quantize).  Here ONE workgroup owns a
// channel at a time: every wave loads one slice of the channel (<= 8 chunks of 16 bytes per lane: 8 KiB
// per wave) into registers, the workgroup agrees on the channel's maximum through LDS, and every wave
// quantizes what it still holds.  x is read ONCE, one launch instead of three.  Channels that do not fit
// one workgroup's registers: the cluster form below (several workgroups hold one channel and exchange one key word
// each).  Pipelining slabs of channels through the Infinity Cache instead (round 2,
// profiles/r02_slab_pipeline_experiment.txt) lost to the two-kernel route.
constexpr int kFusedSlots = 8;          // 16-byte chunks per lane held in registers
constexpr int kFusedSliceChunks = 512;  // kWave * kFusedSlots
constexpr int kFusedMaxWaves = 8;       // waves per workgroup

struct FusedArgs {
  const void* x;
  void* y;
  void* stat_out;   // [channels], dtype of x
  void* scale_out;  // [channels], scale_dtype
  int64_t outer, inner;
  int32_t channels;
  int32_t cpr;      // chunks per row
  int32_t spr;      // slices per row
  int32_t slices;   // slices per channel = outer * spr
  float qmin, qmax, min_val, int_threshold;
  int32_t use_min, scale_dtype, scale_pc, scalar_cast, round_mode, pre_relu;
};

// statistic (an |x| key) -> the statistic as a float and the scale, with the rounding points of
// clamp_min_ste(stat, min_val) / int_threshold (ScaleEpilogue of bvq_stats.hip)
template <typename T>
__device__ __forceinline__ float scale_from_key(uint32_t key, bool use_min, float min_val, float int_threshold,
                                                int scale_dtype, float& stat) {
  if constexpr (elem<T>::id == BVQ_F16)
    stat = (float)__builtin_bit_cast(f16_t, (uint16_t)key);
  else
    stat = __builtin_bit_cast(float, key);
  const float thr = (use_min && stat < min_val) ? min_val : stat;  // NaN passes, like torch.clamp_min
  float s = thr / int_threshold;
  // rounded to the scale's dtype as a tensor op would
  if (scale_dtype == BVQ_BF16)
    s = rnd<bf16_t>(s);
  else if (scale_dtype == BVQ_F16)
    s = rnd<f16_t>(s);
  return s;
}
template <typename T>
__device__ __forceinline__ void store_stat_scale(void* stat_out, void* scale_out, int scale_dtype, int32_t c,
                                                 float stat, float s) {
  if constexpr (elem<T>::id == BVQ_F32)
    reinterpret_cast<float*>(stat_out)[c] = stat;
  else
    reinterpret_cast<T*>(stat_out)[c] = (T)stat;  // exact: stat is a value of T
  if (scale_dtype == BVQ_F32)
    reinterpret_cast<float*>(scale_out)[c] = s;
  else if (scale_dtype == BVQ_BF16)
    reinterpret_cast<bf16_t*>(scale_out)[c] = (bf16_t)s;
  else
    reinterpret_cast<f16_t*>(scale_out)[c] = (f16_t)s;
}

template <typename T, int RM, bool PRE, typename Div, typename Ok>
__device__ __forceinline__ void fused_quantize(const vec_t<T, elem<T>::vec> (&xv)[kFusedSlots], const Ok& ok,
                                               T* __restrict__ yp, int lane, const Div& div, float s,
                                               float qmin, float qmax, int mode) {
  constexpr int VEC = elem<T>::vec;
  constexpr bool ZP0 = sizeof(T) == 2;
#pragma unroll
  for (int j = 0; j < kFusedSlots; ++j) {
    if (ok[j]) {
      vec_t<T, VEC> yv;
#pragma unroll
      for (int k = 0; k < VEC; k += 2) {
        f2 xf = widen2<T>(xv[j].v[k], xv[j].v[k + 1]);
        if constexpr (PRE) xf = relu2(xf);
        f2 q2;
        const f2 r = fwd_elem2<T, RM, ZP0>(xf, div, s, 0.f, qmin, qmax, false, mode, q2);
        pack2<T>(r, yv.v[k], yv.v[k + 1]);
      }
      store_vec<T, VEC, true>(yp + (int64_t)(lane + kWave * j) * VEC, yv);
    }
  }
}

__global__ void fused_zero_kernel(uint32_t* p, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = 0u;
}

// the slice of a channel wave `q` of a workgroup holds (q < slices), and which of its 16-byte slots are in the row
__device__ __forceinline__ void fused_slice(const FusedArgs& a, int q, int lane, int& r, int& sl, bool (&ok)[kFusedSlots]) {
  const bool active = q < a.slices;
  r = active ? q / a.spr : 0;
  sl = active ? q - r * a.spr : 0;
  const int nch = active ? (a.cpr - sl * kFusedSliceChunks < kFusedSliceChunks ? a.cpr - sl * kFusedSliceChunks
                                                                              : kFusedSliceChunks)
                         : 0;
#pragma unroll
  for (int j = 0; j < kFusedSlots; ++j) ok[j] = lane + kWave * j < nch;
}

// phase 1 of a channel: the slice (r, sl) of channel c into registers (slots that are not in the row read the tensor's
// first chunk and are never used)
template <typename T>
__device__ __forceinline__ void fused_load(const FusedArgs& a, int32_t c, int r, int sl, const bool (&ok)[kFusedSlots],
                                           int lane, vec_t<T, elem<T>::vec> (&xv)[kFusedSlots]) {
  constexpr int VEC = elem<T>::vec;
  const int64_t base = ((int64_t)r * a.channels + c) * a.inner + (int64_t)sl * kFusedSliceChunks * VEC;
  const T* __restrict__ xp = reinterpret_cast<const T*>(a.x) + base;
#pragma unroll
  for (int j = 0; j < kFusedSlots; ++j)
    xv[j] = load_vec<T, VEC, true>(ok[j] ? xp + (int64_t)(lane + kWave * j) * VEC : reinterpret_cast<const T*>(a.x));
}

// The same two for a kernel short of registers (the cluster forward below): the slots of a wave's slice as ONE count of
// chunks, every ok[j] a compare where it is used instead of eight lane masks held in registers; and a load whose
// address is the slice's (wave-uniform) start plus a 32-bit lane offset (slots that are not in the row read the slice's
// first chunk and are never used)
struct SlotCount {
  int lane, nch;
  __device__ __forceinline__ bool operator[](int j) const { return lane + kWave * j < nch; }
};
__device__ __forceinline__ void fused_slice(const FusedArgs& a, int q, int lane, int& r, int& sl, SlotCount& ok) {
  const bool active = q < a.slices;
  r = active ? q / a.spr : 0;
  sl = active ? q - r * a.spr : 0;
  const int left = a.cpr - sl * kFusedSliceChunks;
  ok.lane = lane;
  ok.nch = active ? (left < kFusedSliceChunks ? left : kFusedSliceChunks) : 0;
}
template <typename T>
__device__ __forceinline__ void fused_load(const FusedArgs& a, int32_t c, int r, int sl, const SlotCount& ok, int lane,
                                           vec_t<T, elem<T>::vec> (&xv)[kFusedSlots]) {
  constexpr int VEC = elem<T>::vec;
  const int64_t base = ((int64_t)r * a.channels + c) * a.inner + (int64_t)sl * kFusedSliceChunks * VEC;
  const T* __restrict__ xp = reinterpret_cast<const T*>(a.x) + base;
  // opaque to the optimizer: the eight lane offsets are recomputed at every call (a few VALU instructions) instead of
  // being hoisted out of the caller's channel loop into eight more registers
  asm volatile("" : "+v"(lane));
#pragma unroll
  for (int j = 0; j < kFusedSlots; ++j)
    xv[j] = load_vec<T, VEC, true>(xp + (lane + kWave * j < ok.nch ? (uint32_t)(lane + kWave * j) * VEC : 0u));
}

// ... and its maximum |x| key (this lane's)
template <typename T, typename Ok>
__device__ __forceinline__ uint32_t fused_key(const FusedArgs& a, const vec_t<T, elem<T>::vec> (&xv)[kFusedSlots],
                                              const Ok& ok) {
  uint32_t m = 0;
#pragma unroll
  for (int j = 0; j < kFusedSlots; ++j) {
    if (ok[j]) {
#pragma unroll
      for (int k = 0; k < elem<T>::vec; ++k) {
        const uint32_t b = a.pre_relu ? pre_abs_bits<T, true>(xv[j].v[k]) : pre_abs_bits<T, false>(xv[j].v[k]);
        m = b > m ? b : m;
      }
    }
  }
  return m;
}
// (SlotCount, float32: a select per slot instead of a branch -- what keeps the cluster kernel within 64 registers;
// the 16-bit types are within them with the branches above and far beyond with the selects)
template <typename T, std::enable_if_t<sizeof(T) == 4, int> = 0>
__device__ __forceinline__ uint32_t fused_key(const FusedArgs& a, const vec_t<T, elem<T>::vec> (&xv)[kFusedSlots],
                                              const SlotCount& ok) {
  uint32_t m = 0;
#pragma unroll
  for (int j = 0; j < kFusedSlots; ++j) {
    uint32_t mj = 0;
#pragma unroll
    for (int k = 0; k < elem<T>::vec; ++k) {
      const uint32_t b = a.pre_relu ? pre_abs_bits<T, true>(xv[j].v[k]) : pre_abs_bits<T, false>(xv[j].v[k]);
      mj = b > mj ? b : mj;
    }
    mj = ok[j] ? mj : 0u;
    m = mj > m ? mj : m;
  }
  return m;
}

// phase 2 of a channel: quantize what the registers still hold with the scale s
template <typename T, int RM, typename Ok>
__device__ __forceinline__ void fused_apply(const FusedArgs& a, int32_t c, int r, int sl,
                                            const vec_t<T, elem<T>::vec> (&xv)[kFusedSlots], const Ok& ok,
                                            float s, float qmin, float qmax, int lane) {
  constexpr int VEC = elem<T>::vec;
  const int64_t base = ((int64_t)r * a.channels + c) * a.inner + (int64_t)sl * kFusedSliceChunks * VEC;
  T* __restrict__ yp = reinterpret_cast<T*>(a.y) + base;
  const int mode = a.round_mode;
  if constexpr (elem<T>::id == BVQ_BF16) {
    if (bf16_scale_ok(s)) {
      const DivBf16 div{1.0f / s};
      if (a.pre_relu)
        fused_quantize<T, RM, true>(xv, ok, yp, lane, div, s, qmin, qmax, mode);
      else
        fused_quantize<T, RM, false>(xv, ok, yp, lane, div, s, qmin, qmax, mode);
      return;
    }
  }
  if constexpr (elem<T>::id == BVQ_F16) {
    if (f16_scale_ok(s)) {
      const DivF16R div{s, 1.0f / s};
      if (a.pre_relu)
        fused_quantize<T, RM, true>(xv, ok, yp, lane, div, s, qmin, qmax, mode);
      else
        fused_quantize<T, RM, false>(xv, ok, yp, lane, div, s, qmin, qmax, mode);
      return;
    }
  }
  const DivExact div{s};
  if (a.pre_relu)
    fused_quantize<T, RM, true>(xv, ok, yp, lane, div, s, qmin, qmax, mode);
  else
    fused_quantize<T, RM, false>(xv, ok, yp, lane, div, s, qmin, qmax, mode);
}

// one channel c of the tensor `a` by the whole workgroup: every wave loads its slice into registers, the workgroup
// agrees on the maximum through LDS, every wave quantizes what it holds.  Waves without a slice (ok all false) take
// part in the barriers only.
template <typename T, int RM>
__device__ __forceinline__ void fused_channel(const FusedArgs& a, int32_t c, int r, int sl, const bool (&ok)[kFusedSlots],
                                              float qmin, float qmax, int wave, int lane, int nwaves,
                                              uint32_t* sh_max, uint32_t& sh_stat) {
  vec_t<T, elem<T>::vec> xv[kFusedSlots];
  fused_load<T>(a, c, r, sl, ok, lane, xv);
  const uint32_t m = wave_max_u32(fused_key<T>(a, xv, ok));
  if (lane == 0) sh_max[wave] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t bm = 0;
    for (int w = 0; w < nwaves; ++w) bm = sh_max[w] > bm ? sh_max[w] : bm;
    sh_stat = bm;
  }
  __syncthreads();
  float stat;
  float s = scale_from_key<T>(sh_stat, a.use_min, a.min_val, a.int_threshold, a.scale_dtype, stat);
  if (threadIdx.x == 0) store_stat_scale<T>(a.stat_out, a.scale_out, a.scale_dtype, c, stat, s);
  // a 0-dim float32 scale next to a 16-bit tensor is rounded again by the device's scalar semantics
  if (a.scalar_cast && !a.scale_pc) s = rnd<T>(s);
  fused_apply<T, RM>(a, c, r, sl, xv, ok, s, qmin, qmax, lane);
}

template <typename T, int RM>
__global__ __launch_bounds__(kFusedMaxWaves * kWave) void fused_absmax_fakequant_kernel(FusedArgs a) {
  __shared__ uint32_t sh_max[kFusedMaxWaves];
  __shared__ uint32_t sh_stat;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int nwaves = (int)(blockDim.x >> 6);
  int r, sl;  // this wave's slice of every channel the workgroup visits
  bool ok[kFusedSlots];
  fused_slice(a, wave, lane, r, sl, ok);
  const float qmin = rnd<T>(a.qmin), qmax = rnd<T>(a.qmax);
  for (int32_t c = blockIdx.x; c < a.channels; c += gridDim.x)
    fused_channel<T, RM>(a, c, r, sl, ok, qmin, qmax, wave, lane, nwaves, sh_max, sh_stat);
}

// The same over a LIST of tensors (bvq_weight_quant_list_fwd): the workgroups are dealt over the (tensor, channel) pairs
// of the whole list; the workgroup has the list's largest number of slices per channel in waves, and a tensor with
// fewer leaves the rest idle.  Every channel is done exactly as fused_absmax_fakequant_kernel does it.
struct FusedListArgs {
  FusedArgs a[BVQ_WEIGHT_LIST_MAX];
  int32_t start[BVQ_WEIGHT_LIST_MAX + 1];  // first pair of tensor i; start[n] = all pairs
  int32_t n;
};
static_assert(sizeof(FusedListArgs) <= 4096, "kernel arguments are limited to 4 KiB");

template <typename T, int RM>
__global__ __launch_bounds__(kFusedMaxWaves * kWave) void fused_list_fakequant_kernel(FusedListArgs la) {
  __shared__ uint32_t sh_max[kFusedMaxWaves];
  __shared__ uint32_t sh_stat;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int nwaves = (int)(blockDim.x >> 6);
  int p = -1, r = 0, sl = 0;
  bool ok[kFusedSlots];
  float qmin = 0.f, qmax = 0.f;
  for (int32_t pair = blockIdx.x; pair < la.start[la.n]; pair += gridDim.x) {
    if (p < 0 || pair >= la.start[p + 1]) {  // (workgroup-uniform) the pairs only grow: the tensor index follows them
      if (p < 0) p = 0;
      while (p + 1 < la.n && pair >= la.start[p + 1]) ++p;
      fused_slice(la.a[p], wave, lane, r, sl, ok);
      qmin = rnd<T>(la.a[p].qmin);
      qmax = rnd<T>(la.a[p].qmax);
    }
    fused_channel<T, RM>(la.a[p], pair - la.start[p], r, sl, ok, qmin, qmax, wave, lane, nwaves, sh_max, sh_stat);
  }
}


// ------------------------------------------------------------------------------------------------
// statistic + quantizer in ONE kernel, channels held by a CLUSTER of workgroups
// ------------------------------------------------------------------------------------------------
// A channel that does not fit one workgroup's registers ([256,512,56,56] bf16: 1.53 MiB) is held by `members`
// workgroups of 16 waves at once, one slice (fused_slice) per wave, so x is still read once.  The members agree on the
// channel's maximum through one 32-bit word each: every member folds its key in LDS, its wave 0 publishes the key
// (tagged, one agent-scope store: the word is the data and its own flag, so no release fence; cdna_hip_programming §6
// Guideline 16 R2) and then sweeps the cluster's words with one relaxed agent-scope load per lane (one member per lane,
// s_sleep between passes) while the other waves wait at the barrier.
//
// The kernel needs at most 64 VGPRs, so TWO 1024-thread workgroups are resident per CU: while one sweeps and quantizes,
// the other one loads, which is where the overlap of loads, exchange and stores comes from (an earlier form kept a second
// register set with the next channel's loads in flight in ONE workgroup per CU: 109 VGPRs, slower on every measured
// shape, removed; profiles/cluster_fwd.md).  Two walks over the channels, chosen by cluster_plan through nclusters:
//   walking   a persistent grid of (resident workgroups / members) clusters; cluster k takes channels k, k + nclusters, ...
//   one-shot  nclusters = channels: a grid of channels x members workgroups, each handles one channel and exits, and a
//             slot refills the moment a workgroup retires.
// One-shot placement: members of a cluster have consecutive block ids, and the dispatcher starts the blocks of an XCD
// in order, so every member of the lowest unfinished cluster is resident or next in its XCD's queue, and every
// workgroup resident ahead of it belongs to a lower cluster and finishes without it.  HIP does not promise that order:
// it is relied on for speed only.  If it fails, the budget below ends the wait, the fallback gives the same bits, and
// every workgroup still terminates.  No cooperative launch (+15-19 us per call), no wait without a bound.
//
// Never an unbounded wait: the sweep has a budget on the constant-rate clock (s_memrealtime, 100 MHz); when it runs
// out (partners not resident, or the test bit BVQ_CLUSTER_FORCE_FALLBACK) the workgroup reads every row of the channel
// itself (cluster_fallback_key).  A max is exact and order-independent, so that gives the same bits; the workgroup has
// already published, so its partners still finish.
//
// Arrival words (zero on entry, handed back as zeros): key[c * members + i] for member i of channel c, then dep[c]:
// every member adds one to dep[c] once it has its maximum (after its sweep's loads returned, or, on the fallback, after
// its own key store has been written through: s_waitcnt vmcnt(0)); the member whose add completes the count knows no
// partner still reads channel c's words and zeroes them.  Member 0 writes the statistic, scale and running statistic
// (absmax_epilogue: the bits of bvq_absmax_scale_onepass).
constexpr int kClusterWaves = 16;                   // waves per workgroup: one member is 16 slices and one key word
constexpr int kClusterMaxMembers = kWave;           // one sweeping lane per member
constexpr uint32_t kClusterTag = 0x80000000u;       // abs keys never have the top bit set
constexpr uint64_t kClusterBudgetTicks = 200000;    // 2 ms of s_memrealtime (100 MHz) before the fallback
enum { kClusterAuto = 0, kClusterWalk = 1, kClusterOneShot = 2 };  // the `form` of bvq_absmax_fakequant_cluster_form

struct ClusterArgs {
  FusedArgs f;        // the tensor (f.stat_out / f.scale_out unused: the epilogue writes the outputs)
  ScaleEpilogue ep;
  void* stat_out;     // [channels], dtype of x
  int32_t in_dtype;
  uint32_t* key;      // [channels][members]
  uint32_t* dep;      // [channels]
  uint32_t* fallbacks;  // nullable: fallbacks taken
  int32_t members, nclusters, force_fallback;
#ifdef BVQ_CLUSTER_STAMPS
  uint64_t* stamps;   // nullable: [channels][members][kClusterStamps] s_memrealtime ticks (developer builds only)
#endif
};

// BVQ_CLUSTER_STAMPS (developer builds, never the product library): wave 0 of every workgroup reads the constant-rate
// clock at the start of a round and at five points of it, and writes the six values with ordinary vector stores at the
// round's end (tools/cluster_phases.py turns them into per-phase medians)
constexpr int kClusterStamps = 6;  // round start | loads landed | key published | sweep done | quantizer done, stores issued | words handed back
#ifdef BVQ_CLUSTER_STAMPS
#define BVQ_CLUSTER_STAMP(k) \
  do {                       \
    if (wave == 0) tk[k] = __builtin_amdgcn_s_memrealtime(); \
  } while (0)
#else
#define BVQ_CLUSTER_STAMP(k) \
  do {                       \
  } while (0)
#endif

// wave_max_u32 of a whole wave without the six lane-index registers of its ds_bpermute form (the kernel has none
// to spare): four DPP steps leave every row of 16 lanes with its maximum, four lane reads fold the rows
__device__ __forceinline__ uint32_t cluster_wave_max(uint32_t v) {
#define BVQ_DPP_MAX(ctrl)                                                                       \
  do {                                                                                          \
    const uint32_t o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, ctrl, 0xf, 0xf, false); \
    v = o > v ? o : v;                                                                          \
  } while (0)
  BVQ_DPP_MAX(0xB1);   // quad_perm:[1,0,3,2]
  BVQ_DPP_MAX(0x4E);   // quad_perm:[2,3,0,1]
  BVQ_DPP_MAX(0x141);  // row_half_mirror
  BVQ_DPP_MAX(0x140);  // row_mirror
#undef BVQ_DPP_MAX
  const uint32_t a = (uint32_t)__builtin_amdgcn_readlane((int)v, 0), b = (uint32_t)__builtin_amdgcn_readlane((int)v, 16);
  const uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)v, 32), d = (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
  const uint32_t ab = a > b ? a : b, cd = c > d ? c : d;
  return ab > cd ? ab : cd;
}

// The fallback: the maximum |x| key of every row of channel c, read by this workgroup alone, one chunk per lane at a
// time.  Cold, and written so that it needs a handful of registers next to the channel slice the caller still holds.
template <typename T>
__device__ __forceinline__ uint32_t cluster_fallback_key(const FusedArgs& a, int32_t c, int wave, int lane) {
  constexpr int VEC = elem<T>::vec;
  uint32_t fm = 0;
  for (int q = wave; q < a.slices; q += kClusterWaves) {  // (wave-uniform)
    const int fr = q / a.spr, fsl = q - fr * a.spr;
    const int left = a.cpr - fsl * kFusedSliceChunks;
    const int nch = left < kFusedSliceChunks ? left : kFusedSliceChunks;
    const T* xp = reinterpret_cast<const T*>(a.x) + ((int64_t)fr * a.channels + c) * a.inner +
                  (int64_t)fsl * kFusedSliceChunks * VEC;
#pragma clang loop unroll(disable)
    for (int i = lane; i < nch; i += kWave) {
      const vec_t<T, VEC> u = load_vec<T, VEC, false>(xp + (int64_t)i * VEC);
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        const uint32_t b = a.pre_relu ? pre_abs_bits<T, true>(u.v[k]) : pre_abs_bits<T, false>(u.v[k]);
        fm = b > fm ? b : fm;
      }
    }
  }
  return cluster_wave_max(fm);
}

// (the second launch bound is waves per SIMD: 8 = two workgroups of 16 waves per CU, at most 64 VGPRs)
template <typename T, int RM>
__global__ __launch_bounds__(kClusterWaves * kWave, 8) void cluster_absmax_fakequant_kernel(ClusterArgs ca) {
  constexpr int VEC = elem<T>::vec;
  __shared__ uint32_t sh_max[kClusterWaves];
  __shared__ uint32_t sh_stat, sh_ok;
  const FusedArgs& a = ca.f;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int32_t members = ca.members;
  const int32_t member = (int32_t)blockIdx.x % members, cluster = (int32_t)blockIdx.x / members;
  int r, sl;
  SlotCount ok;
  fused_slice(a, member * kClusterWaves + wave, lane, r, sl, ok);
  const float qmin = rnd<T>(a.qmin), qmax = rnd<T>(a.qmax);
  int32_t c = cluster;
  if (c >= a.channels) return;  // (workgroup-uniform)
#ifdef BVQ_CLUSTER_STAMPS
  uint64_t tk[kClusterStamps] = {};
#endif
  BVQ_CLUSTER_STAMP(0);
  vec_t<T, VEC> xv[kFusedSlots];
  fused_load<T>(a, c, r, sl, ok, lane, xv);
  for (; c < a.channels; c += ca.nclusters) {
    const uint32_t m = cluster_wave_max(fused_key<T>(a, xv, ok));
    if (lane == 0) sh_max[wave] = m;
    BVQ_CLUSTER_STAMP(1);
    __syncthreads();
    uint32_t* const keys = ca.key + (int64_t)c * members;
    if (wave == 0) {
      uint32_t bm = 0;
      for (int w = 0; w < kClusterWaves; ++w) bm = sh_max[w] > bm ? sh_max[w] : bm;
      if (lane == 0) __hip_atomic_store(keys + member, bm | kClusterTag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    BVQ_CLUSTER_STAMP(2);
    const int32_t cn = c + ca.nclusters;
    if (wave == 0) {
      bool done = false;
      uint32_t v = 0;
      if (!ca.force_fallback) {
        const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
        for (;;) {
          v = lane < members ? __hip_atomic_load(keys + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : kClusterTag;
          if (__all((v & kClusterTag) != 0)) {
            done = true;
            break;
          }
          if (__builtin_amdgcn_s_memrealtime() - t0 > kClusterBudgetTicks) break;
          __builtin_amdgcn_s_sleep(2);
        }
      }
      v = cluster_wave_max(v) & ~kClusterTag;
      if (lane == 0) {
        sh_stat = v;
        sh_ok = done ? 1u : 0u;
      }
    }
    __syncthreads();
    if (!sh_ok) {  // (workgroup-uniform) the fallback
      const uint32_t fm = cluster_fallback_key<T>(a, c, wave, lane);
      if (lane == 0) sh_max[wave] = fm;
      __syncthreads();
      if (threadIdx.x == 0) {
        uint32_t bm = 0;
        for (int w = 0; w < kClusterWaves; ++w) bm = sh_max[w] > bm ? sh_max[w] : bm;
        sh_stat = bm;
        if (ca.fallbacks) __hip_atomic_fetch_add(ca.fallbacks, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      __syncthreads();
    }
    BVQ_CLUSTER_STAMP(3);
    const uint32_t key = sh_stat;
    // departure: this member no longer reads channel c's words (on the fallback its key store is drained first, so
    // that the zeroing below cannot overtake it)
    uint32_t before = 0;
    if (wave == 0) {
      if (lane == 0) {
        if (!sh_ok) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        before = __hip_atomic_fetch_add(ca.dep + c, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    float stat;
    const float s = scale_from_key<T>(key, a.use_min, a.min_val, a.int_threshold, a.scale_dtype, stat);
    if (member == 0 && threadIdx.x == 0) absmax_epilogue(ca.stat_out, ca.in_dtype, ca.in_dtype, ca.ep, c, key);
    if constexpr (RM == kAnyRM && elem<T>::id == BVQ_BF16) {
      // bfloat16: the rounding mode chosen once per round, not inside every pair of elements.  Straight-line
      // quantizers are what keeps this instance within 64 registers (float16 and float32 are within them with the
      // switch inside, and float16 is not with it here: tools/kernel_resources.py)
      switch (a.round_mode) {
#define BVQ_CLUSTER_APPLY(M)                                              \
  case M:                                                                 \
    fused_apply<T, M>(a, c, r, sl, xv, ok, s, qmin, qmax, lane); \
    break
        BVQ_CLUSTER_APPLY(BVQ_ROUND);
        BVQ_CLUSTER_APPLY(BVQ_FLOOR);
        BVQ_CLUSTER_APPLY(BVQ_CEIL);
        BVQ_CLUSTER_APPLY(BVQ_ROUND_TO_ZERO);
        default:
          fused_apply<T, BVQ_DPU_ROUND>(a, c, r, sl, xv, ok, s, qmin, qmax, lane);
#undef BVQ_CLUSTER_APPLY
      }
    } else {
      fused_apply<T, RM>(a, c, r, sl, xv, ok, s, qmin, qmax, lane);
    }
    BVQ_CLUSTER_STAMP(4);
    if (wave == 0) {
      before = __builtin_amdgcn_readfirstlane(before);
      if (before + 1 == (uint32_t)members) {  // the last departure hands the channel's words back as zeros
        if (lane < members) __hip_atomic_store(keys + lane, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (lane == 0) __hip_atomic_store(ca.dep + c, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
#ifdef BVQ_CLUSTER_STAMPS
    BVQ_CLUSTER_STAMP(5);
    if (ca.stamps && wave == 0 && lane < kClusterStamps) {
      uint64_t t = tk[0];
#pragma unroll
      for (int k = 1; k < kClusterStamps; ++k) t = lane == k ? tk[k] : t;
      ca.stamps[((int64_t)c * members + member) * kClusterStamps + lane] = t;
    }
    if (wave == 0) tk[0] = tk[5];  // the next round starts where this one ended
#endif
    if (cn < a.channels) fused_load<T>(a, cn, r, sl, ok, lane, xv);
  }
}
#undef BVQ_CLUSTER_STAMP

}  // namespace bvq

using namespace bvq;

static int fakequant_fwd_impl(const bvq_quant_desc* d, const void* x, const void* scale, const void* zp, void* y,
                             void* codes, const float* bounds, bvq_stream_t stream) {
  int rc = validate(d, true);
  if (rc) return rc;
  const bool act = d->pre_op >= BVQ_PRE_SIGMOID;  // bvq_act.h: the row-mapped kernel, dequantized output only
  if (act && (codes || bounds || !y || d->out_kind != BVQ_OUT_DEQUANT || d->x_dtype != d->ct_dtype)) {
    set_error("bvq_fakequant_fwd: pre_op %d needs the dequantized output in x's dtype, no codes, no device bounds",
              d->pre_op);
    return BVQ_ERR_UNSUPPORTED;
  }
  const int64_t n = d->outer * d->channels * d->inner;
  if (n == 0) return BVQ_OK;
  if (!x || !scale || !zp || (!y && !codes)) {
    set_error("bvq_fakequant_fwd: null pointer");
    return BVQ_ERR_INVALID;
  }
  if (y && !codes && !bounds && !act) {
    const ColsPlan cp = cols_quant_plan(d, x, y, nullptr, true, false, kColsFwdVec16);
    if (cp.ok) {
      ColsQuantArgs ca = {};
      fill_cols_args(ca, cp, d);
      ca.x = x;
      ca.y = y;
      ca.scale = scale;
      ca.zp = zp;
      hipStream_t cst = (hipStream_t)stream;
      const bool cnt = n * (int64_t)(2 * dtype_size(d->x_dtype)) >= nt_threshold_bytes();
      rc = with_cols_variant(d, cnt, [&](auto t, auto rm, auto ntc) {
        fakequant_fwd_cols_kernel<typename decltype(t)::type, rm, ntc><<<grid_for_units(cp.units), kBlock, 0, cst>>>(ca);
      });
      return rc ? rc : check_launch("bvq_fakequant_fwd/cols");
    }
  }
  int64_t outer, row_len;
  int32_t channels;
  rows_of(d, outer, row_len, channels);
  const void* ptrs[3] = {x, y, codes};
  const int els[3] = {dtype_size(d->x_dtype), dtype_size(d->ct_dtype), d->codes_dtype == BVQ_CODES_I32 ? 4 : 1};
  const int full = 16 / dtype_size(d->x_dtype);
  const int vec = snap_vec(pick_vec(full, outer * channels, row_len, ptrs, els, 3, true), full);
  QuantArgs a = {};
  a.t = make_tiling(outer, channels, row_len, vec, 0, true);
  a.x = x;
  a.scale = scale;
  a.zp = zp;
  a.y = y;
  a.codes = codes;
  a.bounds = bounds;
  fill_args(a, d);
  hipStream_t st = (hipStream_t)stream;
  const bool nt = n * (int64_t)(dtype_size(d->x_dtype) + dtype_size(d->ct_dtype)) >= nt_threshold_bytes();
  if (act) {
    rc = with_dtype(d->x_dtype, [&](auto xt) {
      using XT = typename decltype(xt)::type;
      return with_value<BVQ_PRE_SIGMOID, BVQ_PRE_TANH>(d->pre_op, [&](auto ac) {
        return with_stream_variant<elem<XT>::vec>("bvq_fakequant_fwd", vec, a.round_mode, nt, [&](auto v, auto rm, auto ntc) {
          fakequant_fwd_kernel<XT, XT, v, rm, ntc, ntc, ac><<<grid_for_units(a.t.units), kBlock, 0, st>>>(a);
        });
      });
    });
    return rc ? rc : check_launch("bvq_fakequant_fwd");
  }
  rc = with_pair(d->x_dtype, d->ct_dtype, [&](auto xt, auto ct) {
    using XT = typename decltype(xt)::type;
    return with_stream_variant<elem<XT>::vec>("bvq_fakequant_fwd", vec, a.round_mode, nt, [&](auto v, auto rm, auto ntc) {
      fakequant_fwd_kernel<XT, typename decltype(ct)::type, v, rm, ntc><<<grid_for_units(a.t.units), kBlock, 0, st>>>(a);
    });
  });
  return rc ? rc : check_launch("bvq_fakequant_fwd");
}

extern "C" int bvq_fakequant_fwd(const bvq_quant_desc* d, const void* x, const void* scale,
                                 const void* zp, void* y, void* codes, bvq_stream_t stream) {
  return fakequant_fwd_impl(d, x, scale, zp, y, codes, nullptr, stream);
}

extern "C" int bvq_fakequant_fwd_bounds(const bvq_quant_desc* d, const void* x, const void* scale, const void* zp,
                                        const float* bounds, void* y, bvq_stream_t stream) {
  if (!bounds) {
    set_error("bvq_fakequant_fwd_bounds: null bounds");
    return BVQ_ERR_INVALID;
  }
  return fakequant_fwd_impl(d, x, scale, zp, y, nullptr, bounds, stream);
}


// ---- statistic + quantizer in one launch ------------------------------------------------------------
struct FusedPlan {
  int32_t cpr, spr, slices, waves, nblocks;
};

static int num_cus() {
  static int n = [] {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0)
      v = 256;
    return v;
  }();
  return n;
}

struct FusedShape {
  bool ok;
  int64_t outer, channels, inner;
  int vec;
};

// 0: no one-launch statistic + quantizer (bvq_stats_fakequant_fwd_workspace_bytes reports it as not covered)
#ifndef BVQ_FUSED_FWD
#define BVQ_FUSED_FWD 1
#endif
constexpr bool kFusedFwd = BVQ_FUSED_FWD != 0;

// what both one-launch forms need: x and y of one dtype, dequantized output, whole 16-byte chunks
static FusedShape fused_shape(const bvq_quant_desc* d, const void* x, const void* y) {
  FusedShape f = {};
  if (!kFusedFwd) return f;
  if (d->x_dtype != d->ct_dtype || d->out_kind != BVQ_OUT_DEQUANT) return f;
  if (d->zp_per_channel) return f;
  const bool pc = d->scale_per_channel && d->channels > 1;
  f.outer = pc ? d->outer : 1;
  f.channels = pc ? d->channels : 1;
  f.inner = pc ? d->inner : d->outer * d->channels * d->inner;
  f.vec = 16 / dtype_size(d->x_dtype);
  if (f.inner <= 0 || f.outer <= 0 || f.inner % f.vec != 0) return f;
  if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15) return f;
  f.ok = true;
  return f;
}

// the register-resident form applies when a channel fits the registers of ONE workgroup
static bool fused_plan(const bvq_quant_desc* d, const void* x, const void* y, FusedPlan& p) {
  const FusedShape f = fused_shape(d, x, y);
  if (!f.ok) return false;
  const int64_t cpr = f.inner / f.vec;
  const int64_t spr = (cpr + kFusedSliceChunks - 1) / kFusedSliceChunks;
  const int64_t slices = f.outer * spr;
  if (cpr > (1 << 30) || slices > kFusedMaxWaves) return false;
  p.cpr = (int32_t)cpr;
  p.spr = (int32_t)spr;
  p.slices = (int32_t)slices;
  p.waves = (int)slices;
  // residency budget: 2 workgroups of 512 threads per CU (or the same number of waves in smaller ones)
  const int64_t budget = (int64_t)num_cus() * 2 * kFusedMaxWaves / p.waves;
  p.nblocks = (int32_t)(budget < f.channels ? budget : f.channels);
  return true;
}

extern "C" int64_t bvq_stats_fakequant_fwd_workspace_bytes(const bvq_quant_desc* d, const void* x, const void* y) {
  if (validate(d)) return -1;
  FusedPlan p;
  if (fused_plan(d, x, y, p)) return 16;  // no workspace needed; non-zero says "covered"
  return 0;  // not applicable: use bvq_absmax_scale + bvq_fakequant_fwd
}

// the kernel arguments of one tensor of the one-launch statistic + quantizer
static FusedArgs fused_args(const bvq_quant_desc* d, const FusedPlan& p, const void* x, void* y, void* stat_out,
                            void* scale_out, double min_val, int use_min, double int_threshold) {
  const bool pc = d->scale_per_channel && d->channels > 1;
  FusedArgs a = {};
  a.x = x;
  a.y = y;
  a.stat_out = stat_out;
  a.scale_out = scale_out;
  a.outer = pc ? d->outer : 1;
  a.inner = pc ? d->inner : d->outer * d->channels * d->inner;
  a.channels = (int32_t)(pc ? d->channels : 1);
  a.cpr = p.cpr;
  a.spr = p.spr;
  a.slices = p.slices;
  a.qmin = d->qmin;
  a.qmax = d->qmax;
  a.min_val = round_host((float)min_val, d->x_dtype);  // python scalar -> the statistic's dtype
  a.use_min = use_min;
  a.int_threshold = (float)int_threshold;
  a.scale_dtype = d->scale_dtype;
  a.scale_pc = pc ? 1 : 0;
  a.scalar_cast = d->scalar_mode == BVQ_SCALAR_CAST;
  a.round_mode = d->round_mode;
  a.pre_relu = d->pre_op == BVQ_PRE_RELU;
  return a;
}

extern "C" int bvq_stats_fakequant_fwd(const bvq_quant_desc* d, const void* x, double min_val, int use_min,
                                       double int_threshold, void* stat_out, void* scale_out, void* y,
                                       void* workspace, int64_t workspace_bytes, bvq_stream_t stream) {
  int rc = validate(d);
  if (rc) return rc;
  if (!x || !y || !stat_out || !scale_out || !workspace) {
    set_error("bvq_stats_fakequant_fwd: null pointer");
    return BVQ_ERR_INVALID;
  }
  hipStream_t st = (hipStream_t)stream;
  FusedPlan p;
  if (fused_plan(d, x, y, p)) {
    const FusedArgs a = fused_args(d, p, x, y, stat_out, scale_out, min_val, use_min, int_threshold);
    const dim3 grid((unsigned)p.nblocks), block((unsigned)(p.waves * kWave));
    // (one cache policy: the kernel streams non-temporally whatever the size)
    rc = with_cols_variant(d, false, [&](auto t, auto rm, auto) {
      fused_absmax_fakequant_kernel<typename decltype(t)::type, rm><<<grid, block, 0, st>>>(a);
    });
    return rc ? rc : check_launch("bvq_stats_fakequant_fwd");
  }
  set_error("bvq_stats_fakequant_fwd: shape / layout not covered by the one-launch form");
  return BVQ_ERR_UNSUPPORTED;
}

// ---- statistic + quantizer in one launch, channels held by a cluster of workgroups ---------------------------------
struct ClusterPlan {
  FusedPlan p;
  int32_t members, nclusters;
  int64_t words;  // arrival words
};

// form: kClusterAuto, or the form a developer / test asks for (bvq_absmax_fakequant_cluster_form)
static bool cluster_plan(const bvq_quant_desc* d, const void* x, const void* y, ClusterPlan& cp, int form = kClusterAuto) {
  if (!(d->scale_per_channel && d->channels > 1) || d->channels >= ((int64_t)1 << 31)) return false;
  const FusedShape f = fused_shape(d, x, y);
  if (!f.ok) return false;
  // y must not overlap x: a fallback re-reads x while partners write y
  const uintptr_t bytes = (uintptr_t)(f.outer * f.channels * f.inner * dtype_size(d->x_dtype));
  const uintptr_t xa = reinterpret_cast<uintptr_t>(x), ya = reinterpret_cast<uintptr_t>(y);
  if (xa < ya + bytes && ya < xa + bytes) return false;
  const int64_t cpr = f.inner / f.vec;
  const int64_t spr = (cpr + kFusedSliceChunks - 1) / kFusedSliceChunks;
  const int64_t slices = f.outer * spr;
  const int64_t members = (slices + kClusterWaves - 1) / kClusterWaves;
  if (cpr > (1 << 30) || members > kClusterMaxMembers) return false;
  cp.p.cpr = (int32_t)cpr;
  cp.p.spr = (int32_t)spr;
  cp.p.slices = (int32_t)slices;
  cp.p.waves = kClusterWaves;
  cp.members = (int32_t)members;
  // persistent grid: whole clusters within the resident workgroups (two per CU)
  int64_t nc = (int64_t)num_cus() * 2 / members;
  nc = nc < 1 ? 1 : (nc > f.channels ? f.channels : nc);
  // The rule, from tools/cluster_ab.py --forms walk,oneshot (profiles/cluster_fwd.md, rows of 392 chunks): up to 4
  // rounds per walking cluster the walk is level or ahead (2 rounds: 6 %), from 8 rounds on the one-shot grid is level
  // or ahead (8 rounds: 0-5 %, 16 rounds, the headline: 8 %).  Rows of 98 chunks, which leave four fifths of a slice
  // empty, keep the walk (6-9 % ahead at 16 rounds: a workgroup's start is not paid back by 25 KB of work); the
  // boundary between the two measured row lengths is put at half a slice.
  if (form == kClusterAuto) {
    const int64_t row_chunks = cpr < kFusedSliceChunks ? cpr : kFusedSliceChunks;
    const bool oneshot = f.channels > 4 * nc && 2 * row_chunks >= kFusedSliceChunks;
    form = oneshot ? kClusterOneShot : kClusterWalk;
  }
  if (form == kClusterOneShot && f.channels * members > ((int64_t)1 << 30)) form = kClusterWalk;  // grid size
  if (form == kClusterOneShot) nc = f.channels;  // a cluster per channel
  cp.nclusters = (int32_t)nc;
  cp.p.nblocks = (int32_t)(nc * members);
  cp.words = f.channels * (members + 1);
  return true;
}

extern "C" int64_t bvq_absmax_fakequant_cluster_supported(const bvq_quant_desc* d, const void* x, const void* y) {
  if (validate(d)) return 0;
  ClusterPlan cp;
  return cluster_plan(d, x, y, cp) ? cp.words : 0;
}

static int cluster_impl(const bvq_quant_desc* d, const void* x, double min_val, int use_min, double int_threshold,
                        void* stat_out, void* scale_out, int run_dtype, void* running, double momentum, int first_batch,
                        void* y, uint32_t* arrive, int64_t arrive_words, int flags, uint32_t* fallbacks, int form,
                        uint64_t* stamps, bvq_stream_t stream) {
  int rc = validate(d);
  if (rc) return rc;
  if (!x || !y || !stat_out || !scale_out || !arrive) {
    set_error("bvq_absmax_fakequant_cluster: null pointer");
    return BVQ_ERR_INVALID;
  }
  if ((running && bad_dtype(run_dtype)) || bad_dtype(d->scale_dtype) || !(int_threshold == int_threshold) ||
      (flags & ~BVQ_CLUSTER_FORCE_FALLBACK)) {
    set_error("bvq_absmax_fakequant_cluster: bad argument");
    return BVQ_ERR_INVALID;
  }
  if (form < kClusterAuto || form > kClusterOneShot) {
    set_error("bvq_absmax_fakequant_cluster: form %d", form);
    return BVQ_ERR_INVALID;
  }
#ifndef BVQ_CLUSTER_STAMPS
  if (stamps) {
    set_error("bvq_absmax_fakequant_cluster: this library was built without BVQ_CLUSTER_STAMPS");
    return BVQ_ERR_UNSUPPORTED;
  }
#endif
  ClusterPlan cp;
  if (!cluster_plan(d, x, y, cp, form)) {
    set_error("bvq_absmax_fakequant_cluster: shape / layout not covered (bvq_absmax_fakequant_cluster_supported)");
    return BVQ_ERR_UNSUPPORTED;
  }
  if (arrive_words < cp.words) {
    set_error("bvq_absmax_fakequant_cluster: arrival buffer of %lld words, %lld needed", (long long)arrive_words,
              (long long)cp.words);
    return BVQ_ERR_WORKSPACE;
  }
  ClusterArgs ca = {};
  ca.f = fused_args(d, cp.p, x, y, stat_out, scale_out, min_val, use_min, int_threshold);
  // (the same min_val and int_threshold as ca.f's: both round them for the statistic's dtype, x's)
  ca.ep = with_running(scale_epilogue(scale_out, d->scale_dtype, use_min, min_val, d->x_dtype, int_threshold),
                       run_dtype, running, momentum, first_batch);
  ca.stat_out = stat_out;
  ca.in_dtype = d->x_dtype;
  ca.key = arrive;
  ca.dep = arrive + (int64_t)ca.f.channels * cp.members;
  ca.fallbacks = fallbacks;
  ca.members = cp.members;
  ca.nclusters = cp.nclusters;
  ca.force_fallback = (flags & BVQ_CLUSTER_FORCE_FALLBACK) ? 1 : 0;
#ifdef BVQ_CLUSTER_STAMPS
  ca.stamps = stamps;
#endif
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)cp.p.nblocks), block(kClusterWaves * kWave);
  rc = with_cols_variant(d, false, [&](auto t, auto rm, auto) {
    cluster_absmax_fakequant_kernel<typename decltype(t)::type, rm><<<grid, block, 0, st>>>(ca);
  });
  return rc ? rc : check_launch("bvq_absmax_fakequant_cluster");
}

extern "C" int bvq_absmax_fakequant_cluster(const bvq_quant_desc* d, const void* x, double min_val, int use_min,
                                            double int_threshold, void* stat_out, void* scale_out, int run_dtype,
                                            void* running, double momentum, int first_batch, void* y, uint32_t* arrive,
                                            int64_t arrive_words, int flags, uint32_t* fallbacks,
                                            bvq_stream_t stream) {
  return cluster_impl(d, x, min_val, use_min, int_threshold, stat_out, scale_out, run_dtype, running, momentum,
                      first_batch, y, arrive, arrive_words, flags, fallbacks, kClusterAuto, nullptr, stream);
}

extern "C" int bvq_absmax_fakequant_cluster_form(const bvq_quant_desc* d, const void* x, double min_val, int use_min,
                                                 double int_threshold, void* stat_out, void* scale_out, int run_dtype,
                                                 void* running, double momentum, int first_batch, void* y,
                                                 uint32_t* arrive, int64_t arrive_words, int flags, uint32_t* fallbacks,
                                                 int form, uint64_t* stamps, bvq_stream_t stream) {
  return cluster_impl(d, x, min_val, use_min, int_threshold, stat_out, scale_out, run_dtype, running, momentum,
                      first_batch, y, arrive, arrive_words, flags, fallbacks, form, stamps, stream);
}

namespace bvq {
int fused_list_fwd(int n, const bvq_quant_desc* descs, const bvq_weight_item* items, hipStream_t st) {
  FusedListArgs la = {};
  la.n = n;
  int64_t pairs = 0;
  int waves = 1;
  for (int i = 0; i < n; ++i) {
    const bvq_weight_item& it = items[i];
    FusedPlan p;
    if (!fused_plan(&descs[i], it.x, it.y, p)) {
      set_error("bvq_weight_quant_list_fwd: item %d not covered by the one-launch form", i);
      return BVQ_ERR_UNSUPPORTED;
    }
    la.a[i] = fused_args(&descs[i], p, it.x, it.y, it.stat, it.scale, it.min_val, it.use_min, it.int_threshold);
    la.start[i] = (int32_t)pairs;
    pairs += la.a[i].channels;
    waves = p.waves > waves ? p.waves : waves;
  }
  if (pairs >= ((int64_t)1 << 31)) {
    set_error("bvq_weight_quant_list_fwd: too many channels");
    return BVQ_ERR_UNSUPPORTED;
  }
  la.start[n] = (int32_t)pairs;
  // residency budget of the single-tensor launch: 2 workgroups of 512 threads per CU (or as many waves in smaller ones)
  const int64_t budget = (int64_t)num_cus() * 2 * kFusedMaxWaves / waves;
  const dim3 grid((unsigned)(budget < pairs ? budget : pairs)), block((unsigned)(waves * kWave));
  const int rc = with_cols_variant(&descs[0], false, [&](auto t, auto rm, auto) {
    fused_list_fakequant_kernel<typename decltype(t)::type, rm><<<grid, block, 0, st>>>(la);
  });
  return rc ? rc : check_launch("bvq_weight_quant_list_fwd");
}
}  // namespace bvq

// self-test of the float16 division (DivF16R): out[j * n_a + i] = the quotient the kernels compute for numerator
// a[i] and scale s[j], so that a test can compare EVERY pair with a / s on the device itself
__global__ __launch_bounds__(256) void selftest_div_f16r_kernel(const float* __restrict__ a, const float* __restrict__ sc,
                                                                float* __restrict__ out, int32_t n_a) {
  const float s = sc[blockIdx.y];
  const float r = 1.0f / s;
  for (int32_t i = blockIdx.x * 256 + threadIdx.x; i < n_a; i += gridDim.x * 256)
    out[(int64_t)blockIdx.y * n_a + i] = div_refined(a[i], s, r);
}

extern "C" int bvq_selftest_div_f16r(const float* a, int32_t n_a, const float* scales, int32_t n_s, float* out,
                                     bvq_stream_t stream) {
  if (!a || !scales || !out || n_a < 1 || n_s < 1 || n_s > 65535) {
    set_error("bvq_selftest_div_f16r: bad argument");
    return BVQ_ERR_INVALID;
  }
  int nb = (n_a + 255) / 256;
  if (nb > 1024) nb = 1024;
  selftest_div_f16r_kernel<<<dim3((unsigned)nb, (unsigned)n_s), dim3(256), 0, (hipStream_t)stream>>>(a, scales, out, n_a);
  return check_launch("bvq_selftest_div_f16r");
}


// self-test of the fused activations (bvq_act.h): act(x) and its backward, element by element, as the quantizer kernels
// compute them
template <typename T, int ACT>
__global__ __launch_bounds__(256) void selftest_pre_op_kernel(const T* __restrict__ x, const T* __restrict__ g,
                                                              T* __restrict__ act_out, T* __restrict__ dact_out, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float a = act_rnd<T, ACT>(to_f<T>(x[i]));
    act_out[i] = from_f<T>(a);
    dact_out[i] = from_f<T>(act_bwd_rnd<T, ACT>(to_f<T>(g[i]), a));
  }
}

extern "C" int bvq_selftest_pre_op(int pre_op, int dtype, const void* x, const void* g, void* act_out, void* dact_out,
                                   int64_t n, bvq_stream_t stream) {
  if (!x || !g || !act_out || !dact_out || n < 0) {
    set_error("bvq_selftest_pre_op: bad argument");
    return BVQ_ERR_INVALID;
  }
  if (pre_op != BVQ_PRE_SIGMOID && pre_op != BVQ_PRE_TANH) {
    set_error("bvq_selftest_pre_op: pre_op %d has no bvq_act.h form", pre_op);
    return BVQ_ERR_UNSUPPORTED;
  }
  if (n == 0) return BVQ_OK;
  int64_t nb = (n + 255) / 256;
  if (nb > 4096) nb = 4096;
  hipStream_t st = (hipStream_t)stream;
  const int rc = with_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    return with_value<BVQ_PRE_SIGMOID, BVQ_PRE_TANH>(pre_op, [&](auto ac) {
      selftest_pre_op_kernel<T, ac><<<dim3((unsigned)nb), dim3(256), 0, st>>>(
          reinterpret_cast<const T*>(x), reinterpret_cast<const T*>(g), reinterpret_cast<T*>(act_out),
          reinterpret_cast<T*>(dact_out), n);
    });
  });
  return rc ? rc : check_launch("bvq_selftest_pre_op");
}
