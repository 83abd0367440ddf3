// bvq_group_walk.h -- the sub-wave group walk shared by the group-wise integer quantizer (bvq_group_quant.hip) and the
// MX block-scaled quantizers (bvq_mx_quant.hip).
//
// The tensor is walked as a flat stream of 16-byte lane accesses.  A group of g elements occupies
// L = g * sizeof(T) / 16 ADJACENT lanes of one wave load (2..32 lanes for 16-bit types, 4..64 for float32), and 64 / L
// groups share a load; L divides 64, so a group never straddles two loads.  Everything a group needs from its other
// elements is a SEGMENTED butterfly over those L lanes (__shfl_xor with offsets L/2 .. 1: every lane of the segment
// ends with the same bits, in a fixed order).  No LDS, no atomics, no partials, no workspace, no second launch.
#pragma once

#include "bvq_ties.h"

namespace bvq {

template <int L>
__device__ __forceinline__ uint32_t seg_max_u32(uint32_t v) {
#pragma unroll
  for (int off = L / 2; off > 0; off >>= 1) {
    const uint32_t o = (uint32_t)__shfl_xor((int)v, off, kWave);
    v = o > v ? o : v;
  }
  return v;
}
template <int L>
__device__ __forceinline__ uint32_t seg_min_u32(uint32_t v) {
#pragma unroll
  for (int off = L / 2; off > 0; off >>= 1) {
    const uint32_t o = (uint32_t)__shfl_xor((int)v, off, kWave);
    v = o < v ? o : v;
  }
  return v;
}
// a + b is commutative, so both partners of every exchange compute the same bits: the sum is the same in every lane
// of the segment, and from run to run
template <int L>
__device__ __forceinline__ float seg_sum(float v) {
#pragma unroll
  for (int off = L / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
  return v;
}

// largest |x| key (abs_bits<T>) of one 16-byte chunk: sign-cleared bit patterns, so a NaN wins and propagates
template <typename T>
__device__ __forceinline__ uint32_t chunk_key(const vec_t<T, elem<T>::vec>& xv) {
  constexpr int VEC = elem<T>::vec;
  if constexpr (sizeof(T) == 2) {
    typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
    const vec_t<uint32_t, VEC / 2> w = __builtin_bit_cast(vec_t<uint32_t, VEC / 2>, xv);
    u16x2 m2 = {0, 0};
#pragma unroll
    for (int k = 0; k < VEC / 2; ++k)
      m2 = __builtin_elementwise_max(m2, __builtin_bit_cast(u16x2, w.v[k] & 0x7fff7fffu));
    const uint32_t m16 = m2.x > m2.y ? m2.x : m2.y;
    return elem<T>::id == BVQ_BF16 ? (m16 << 16) : m16;
  } else {
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      const uint32_t b = abs_bits<T>(xv.v[k]);
      m = b > m ? b : m;
    }
    return m;
  }
}

template <typename T>
__device__ __forceinline__ float key_value(uint32_t key) {
  if constexpr (elem<T>::id == BVQ_F16)
    return (float)__builtin_bit_cast(f16_t, (uint16_t)key);
  else
    return __builtin_bit_cast(float, key);
}

// the wave's window of the tensor: kD wave loads from chunk c0 on, seen through buffer descriptors whose extents end
// with the tensor -- lanes past the end read zeros without a memory access and their stores are dropped, so the walk
// has no tail branch.  The tensor is whole groups, so a group is either inside or outside as a whole.
// Args: the kernel's argument struct; `chunks` is the number of 16-byte chunks of the tensor = groups * L.
template <typename T, int L, int kD>
struct GroupWindow {
  int64_t c0;
  uint32_t nch, ngr;
  template <typename Args>
  __device__ __forceinline__ bool init(const Args& a) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    c0 = ((int64_t)blockIdx.x * kWavesPerBlock + wave) * (kD * kWave);
    if (c0 >= a.chunks) return false;
    const int64_t left = a.chunks - c0;
    nch = (uint32_t)(left < kD * kWave ? left : kD * kWave);
    ngr = nch / L;
    return true;
  }
  __device__ __forceinline__ buf_t elems(const void* p) const {
    return make_buf(reinterpret_cast<const T*>(p) + c0 * elem<T>::vec, nch * 16u);
  }
  // one value of type S per group (S = T unless named)
  template <typename S = T>
  __device__ __forceinline__ buf_t groups(const void* p) const {
    return make_buf(reinterpret_cast<const S*>(p) + c0 / L, ngr * (uint32_t)sizeof(S));
  }
};

static unsigned group_grid(int64_t chunks, int depth) {
  const int64_t per_block = (int64_t)kWavesPerBlock * depth * kWave;
  return (unsigned)((chunks + per_block - 1) / per_block);
}

// f(type_tag<T>, int_c<L>, std::bool_constant<NT>) for the lanes per group of a dtype and a group size
template <typename F>
static int with_group_variant(int dtype, int64_t group_size, bool nt, F&& f) {
  const int lanes = (int)(group_size * dtype_size(dtype) / 16);
  return with_dtype(dtype, [&](auto t) {
    return with_bool(nt, [&](auto ntc) {
      if constexpr (sizeof(typename decltype(t)::type) == 2)
        return with_value<2, 4, 8, 16, 32>(lanes, [&](auto l) { return call_rc(f, t, l, ntc); });
      else
        return with_value<4, 8, 16, 32, 64>(lanes, [&](auto l) { return call_rc(f, t, l, ntc); });
    });
  });
}

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace bvq
