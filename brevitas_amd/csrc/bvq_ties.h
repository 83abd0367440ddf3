// bvq_ties.h -- bookkeeping of the elements that attain a max/min statistic ("ties"), shared by the
// statistics backward (bvq_stats.hip) and the fused quantizer backward (bvq_fakequant_bwd.h).
//
// tie_info layout (unsigned 64-bit words, device memory, bvq_tie_info_bytes(channels) bytes):
//   channels > 1 : first[c]  = smallest (outer*inner + i) position matching stat[c]   (init: ~0)
//   channels == 1: [0] = number of ties (also the list cursor), [1] = unused,
//                  [2 .. 2+kTieCap) = flat element indices of the first kTieCap ties found
#pragma once

#include "bvq_common.h"

namespace bvq {

constexpr int kTieCap = 1024;
// batch-sharded tensors: a shard's claim on a channel's deposit is its rank, or this when it holds no arg-max
constexpr double kShardNoOwner = 1073741824.0;  // 2^30, above any rank

static inline int64_t tie_info_words(int64_t channels) { return channels > 1 ? channels : 2 + kTieCap; }

__device__ __forceinline__ void record_tie(unsigned long long* info, bool per_channel, int32_t channel,
                                           unsigned long long pos) {
  if (per_channel) {
    atomicMin(&info[channel], pos);
  } else {
    const unsigned long long slot = atomicAdd(&info[0], 1ull);
    if (slot < (unsigned long long)kTieCap) info[2 + slot] = pos;
  }
}

// |v| as an order-preserving integer key (float32 pattern for f32/bf16, 16-bit pattern for f16)
template <typename T>
__device__ __forceinline__ uint32_t abs_bits(T v);
template <>
__device__ __forceinline__ uint32_t abs_bits<float>(float v) {
  return __builtin_bit_cast(uint32_t, v) & 0x7fffffffu;
}
template <>
__device__ __forceinline__ uint32_t abs_bits<bf16_t>(bf16_t v) {
  return ((uint32_t)(__builtin_bit_cast(uint16_t, v) & 0x7fffu)) << 16;
}
template <>
__device__ __forceinline__ uint32_t abs_bits<f16_t>(f16_t v) {
  return (uint32_t)(__builtin_bit_cast(uint16_t, v) & 0x7fffu);
}

// the key a tie search compares the |x| keys with: the statistic's own, or -- a NaN statistic -- ~0, which is no key:
// like torch's ==, a NaN is attained by nothing, not even by the NaN of the same bit pattern it was taken from
template <typename T>
__device__ __forceinline__ uint32_t stat_key(T stat) {
  const uint32_t b = abs_bits<T>(stat);
  return b > abs_bits<T>((T)__builtin_inff()) ? ~0u : b;
}

// torch.relu: x < 0 ? 0 : x  (NaN and -0.0 pass through unchanged)
__device__ __forceinline__ float relu_f(float v) { return v < 0.f ? 0.f : v; }

// |pre_op(v)| as the same key: negative (non-NaN) values become 0 under RELU
template <typename T, bool RELU>
__device__ __forceinline__ uint32_t pre_abs_bits(T v) {
  if constexpr (RELU) {
    return to_f<T>(v) < 0.f ? 0u : abs_bits<T>(v);
  } else {
    return abs_bits<T>(v);
  }
}

#ifdef __HIPCC__
// torch.sign
__device__ __forceinline__ float sgn_f(float v) { return (float)(0.f < v) - (float)(v < 0.f); }

// Where the statistic's gradient comes from: an array of the statistic's dtype, or the float32
// scale-gradient sums of the fused quantizer backward, taken through
//   dscale.to(scale dtype)  ->  / int_threshold (in the dtype torch computes that quotient in)  ->  .to(T)
// i.e. the backward of  scale = clamp_min_ste(stat) / int_threshold  (B/core/quant/int.py:160).
struct GstatSrc {
  const void* p;
  int32_t from_dscale;  // 0: p holds T values; 1: p holds float32 dscale sums
  int32_t scale_dtype;
  int32_t quot_dtype;
  float int_threshold;
  int32_t pre_relu;  // the statistic was taken of relu(x): the deposit's sign is sgn(relu(x))
};

// the source of the fused quantizer backward's finishing steps (p: the sums, where the kernel reads them from there)
static inline GstatSrc dscale_src(int scale_dtype, int quot_dtype, double int_threshold, int pre_op,
                                  const float* dscale = nullptr) {
  return GstatSrc{dscale, 1, scale_dtype, quot_dtype, (float)int_threshold, pre_op == BVQ_PRE_RELU};
}

__device__ __forceinline__ float round_rt(float v, int dt) {
  return dt == BVQ_F32 ? v : (dt == BVQ_BF16 ? rnd<bf16_t>(v) : rnd<f16_t>(v));
}

// a float32 scale-gradient sum -> the statistic's gradient in T: the three rounding points of the chain above
template <typename T>
__device__ __forceinline__ float dscale_to_gstat(float ds, int scale_dtype, int quot_dtype, float int_threshold) {
  return rnd<T>(round_rt(round_rt(ds, scale_dtype) / int_threshold, quot_dtype));
}

template <typename T>
__device__ __forceinline__ float gstat_value(const GstatSrc& g, int64_t c) {
  if (!g.from_dscale) return to_f<T>(reinterpret_cast<const T*>(g.p)[c]);
  return dscale_to_gstat<T>(reinterpret_cast<const float*>(g.p)[c], g.scale_dtype, g.quot_dtype, g.int_threshold);
}

template <typename T, int MATCH>
__device__ __forceinline__ float deposit(float g, T xv, bool pre_relu = false) {
  if constexpr (MATCH == BVQ_MATCH_ABS) {
    return rnd<T>(g * sgn_f(pre_relu ? relu_f(to_f<T>(xv)) : to_f<T>(xv)));
  } else {
    return g;
  }
}

// a store / load that is performed at agent scope (global_store / global_load ... sc1): written through to, read from
// the memory every XCD sees (MI355X_MICROARCH.md, inter-workgroup visibility: sc1 stores and sc1 loads on both sides
// of a hand-off, the storing wave's vmcnt(0) wait before its arrival add)
template <typename T>
__device__ __forceinline__ void store_through(T* p, T v) {
  if constexpr (sizeof(T) == 2) {
    __hip_atomic_store(reinterpret_cast<uint16_t*>(p), __builtin_bit_cast(uint16_t, v), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
  } else {
    __hip_atomic_store(reinterpret_cast<uint32_t*>(p), __builtin_bit_cast(uint32_t, v), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
  }
}
template <typename T>
__device__ __forceinline__ T load_through(const T* p) {
  if constexpr (sizeof(T) == 2) {
    return __builtin_bit_cast(T, __hip_atomic_load(reinterpret_cast<const uint16_t*>(p), __ATOMIC_RELAXED,
                                                   __HIP_MEMORY_SCOPE_AGENT));
  } else {
    return __builtin_bit_cast(T, __hip_atomic_load(reinterpret_cast<const uint32_t*>(p), __ATOMIC_RELAXED,
                                                   __HIP_MEMORY_SCOPE_AGENT));
  }
}

// flat element index of channel c's position pos = o * inner + i in x[outer, channels, inner]
__device__ __forceinline__ int64_t pos_to_flat(unsigned long long pos, int32_t c, int32_t channels, int64_t inner) {
  const int64_t o = (int64_t)(pos / (unsigned long long)inner);
  const int64_t i = (int64_t)(pos - (unsigned long long)o * (unsigned long long)inner);
  return (o * channels + c) * inner + i;
}

// dx[channel c's position pos] += the abs-max statistic's gradient g with the element's sign
template <typename T>
__device__ __forceinline__ void deposit_abs_at(float g, unsigned long long pos, int32_t c, int32_t channels,
                                               int64_t inner, const void* x, void* dx, bool pre_relu) {
  const int64_t flat = pos_to_flat(pos, c, channels, inner);
  T* dp = reinterpret_cast<T*>(dx) + flat;
  *dp = from_f<T>(to_f<T>(*dp) + deposit<T, BVQ_MATCH_ABS>(g, reinterpret_cast<const T*>(x)[flat], pre_relu));
}

// the unit that holds partial k (of nob * ppr) of channel c: units are (outer block, channel, piece)
__device__ __forceinline__ int64_t partial_unit(int32_t c, int64_t k, int64_t nob, int64_t ppr, int32_t channels) {
  if (nob == 1) return (int64_t)c * ppr + k;
  const int64_t o = k / ppr, p = k - o * ppr;
  return (o * channels + c) * ppr + p;
}

#endif

void launch_tie_init(unsigned long long* info, int64_t channels, hipStream_t st, int first_only = 0);

}  // namespace bvq
