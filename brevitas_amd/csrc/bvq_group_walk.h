// bvq_group_walk.h -- the sub-wave group walk of the group-wise integer quantizers (bvq_group_quant.hip,
// bvq_group_mse.hip, bvq_group_shifted.hip) and the MX block-scaled quantizers (bvq_mx_quant.hip): the butterflies, the
// wave's window, the kernel frame that every quantizer on the walk plugs into, and the host side of a launch.
//
// The tensor is walked as a flat stream of 16-byte lane accesses.  A group of g elements occupies
// L = g * sizeof(T) / 16 ADJACENT lanes of one wave load (2..32 lanes for 16-bit types, 4..64 for float32), and 64 / L
// groups share a load; L divides 64, so a group never straddles two loads.  Everything a group needs from its other
// elements is a SEGMENTED butterfly over those L lanes (__shfl_xor with offsets L/2 .. 1: every lane of the segment
// ends with the same bits, in a fixed order).  No LDS, no atomics, no partials, no workspace, no second launch.
#pragma once

#include "bvq_ties.h"

namespace bvq {

// the geometry of every kernel on the walk: wave loads a wave owns (its window), all in flight before the arithmetic
#ifndef BVQ_GROUP_FWD_DEPTH
#define BVQ_GROUP_FWD_DEPTH 4  // forward, encoder, decoder: loads of x (of the codes)
#endif
#ifndef BVQ_GROUP_BWD_DEPTH
#define BVQ_GROUP_BWD_DEPTH 2  // backward: loads of x and of g
#endif
constexpr int kGroupFwdDepth = BVQ_GROUP_FWD_DEPTH;
constexpr int kGroupBwdDepth = BVQ_GROUP_BWD_DEPTH;

// what every kernel of the walk is given; a quantizer's Args extend it
struct WalkArgs {
  const void* x;
  const void* g;   // bwd
  void* y;         // fwd: y, bwd: dx
  int64_t chunks;  // 16-byte chunks of the tensor = groups * L
};

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
template <typename T, int L, int kD>
struct GroupWindow {
  int64_t c0;
  uint32_t nch, ngr;
  __device__ __forceinline__ bool init(const WalkArgs& a) {
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
  // a per-group input that may be absent (p null): then a descriptor of no bytes, whose loads return zeros without a
  // memory access
  template <typename S = T>
  __device__ __forceinline__ buf_t groups_or_zeros(const void* p, const void* any) const {
    return p ? groups<S>(p) : make_buf(reinterpret_cast<const S*>(any), 0u);
  }
};

// where a lane stands in wave load j of its window
struct GroupPlace {
  uint32_t off;    // byte offset of the lane's 16 bytes, for the descriptors of GroupWindow::elems
  uint32_t group;  // the lane's group, for the descriptors of GroupWindow::groups: one address per segment
  uint32_t sub;    // the lane within its segment, 0 .. L - 1
  // byte offset of the group's value of `size` bytes: for every lane of the segment (loads), and for its head lane
  // alone, the others skipping (a store: one lane per segment writes a per-group output)
  __device__ __forceinline__ uint32_t at(uint32_t size) const { return group * size; }
  __device__ __forceinline__ uint32_t head_at(uint32_t size) const { return sub == 0 ? group * size : kBufSkip; }
};
template <int L>
__device__ __forceinline__ GroupPlace group_place(int j) {
  const uint32_t lane = threadIdx.x & 63;
  return {(uint32_t)(j * kWave + lane) * 16u, (uint32_t)(j * (kWave / L)) + lane / L, lane & (L - 1)};
}
template <typename S>
__device__ __forceinline__ S load_group(buf_t b, const GroupPlace& p) {
  return buf_load<S, 1>(b, p.at(sizeof(S))).v[0];
}
template <typename S>
__device__ __forceinline__ void store_group(buf_t b, const GroupPlace& p, S v) {
  vec_t<S, 1> o;
  o.v[0] = v;
  buf_store<S, 1>(b, p.head_at(sizeof(S)), o);  // dropped for the groups past the end
}

// one byte per group (the index of a searched candidate: bvq_group_mse.hip, bvq_group_hqo.hip) through the buffer descriptor (a vector store; dropped at kBufSkip and past the extent)
__device__ __forceinline__ void buf_store_u8(buf_t b, uint32_t byte_off, uint32_t v) {
  __builtin_amdgcn_raw_buffer_store_b8((unsigned char)v, b, byte_off, 0, 0);
}
__device__ __forceinline__ uint32_t buf_load_u8(buf_t b, uint32_t byte_off) {
  return __builtin_amdgcn_raw_buffer_load_b8(b, byte_off, 0, 0);
}

// The kernel frame.  A quantizer Q<T, L> plugs in with
//   Args                       its argument struct, a WalkArgs
//   Q(args, window)            its descriptors (GroupWindow::groups) and wave constants, built once
//   fwd(x, place) -> y         one load of the forward: the lane's 16 bytes of y; per-group outputs by store_group
//   Side, side(place)          the backward's per-group inputs of one load, as loaded (load_group): no arithmetic
//   bwd(x, g, side, place) -> dx
// The frame keeps what every kernel on the walk relies on: all kD loads of a wave are issued before the first use (x,
// then g and the side values of the same load), no load or store has a tail branch (the descriptors end with the
// tensor), and a load that no lane has is not worked on.
template <template <typename, int> class Q, typename T, int L, bool NT>
__global__ __launch_bounds__(kBlock) void group_fwd_kernel(typename Q<T, L>::Args a) {
  constexpr int VEC = elem<T>::vec, kD = kGroupFwdDepth;
  GroupWindow<T, L, kD> w;
  if (!w.init(a)) return;
  const buf_t bx = w.elems(a.x), by = w.elems(a.y);
  const Q<T, L> q(a, w);
  vec_t<T, VEC> xv[kD];
#pragma unroll
  for (int j = 0; j < kD; ++j) xv[j] = buf_load<T, VEC, NT>(bx, group_place<L>(j).off);
#pragma unroll
  for (int j = 0; j < kD; ++j) {
    if ((uint32_t)(j * kWave) >= w.nch) break;  // wave-uniform
    const GroupPlace p = group_place<L>(j);
    buf_store<T, VEC, NT>(by, p.off, q.fwd(xv[j], p));
  }
}

template <template <typename, int> class Q, typename T, int L, bool NT>
__global__ __launch_bounds__(kBlock) void group_bwd_kernel(typename Q<T, L>::Args a) {
  constexpr int VEC = elem<T>::vec, kD = kGroupBwdDepth;
  GroupWindow<T, L, kD> w;
  if (!w.init(a)) return;
  const buf_t bx = w.elems(a.x), bg = w.elems(a.g), bd = w.elems(a.y);
  const Q<T, L> q(a, w);
  vec_t<T, VEC> xv[kD], gv[kD];
  typename Q<T, L>::Side sv[kD];
#pragma unroll
  for (int j = 0; j < kD; ++j) {
    const GroupPlace p = group_place<L>(j);
    xv[j] = buf_load<T, VEC, NT>(bx, p.off);
    gv[j] = buf_load<T, VEC, NT>(bg, p.off);
    sv[j] = q.side(p);
  }
#pragma unroll
  for (int j = 0; j < kD; ++j) {
    if ((uint32_t)(j * kWave) >= w.nch) break;  // wave-uniform
    const GroupPlace p = group_place<L>(j);
    buf_store<T, VEC, NT>(bd, p.off, q.bwd(xv[j], gv[j], sv[j], p));
  }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
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

// A launching entry `what` in three steps, each handing on the first refusal (rc, with its text): the family's coverage
// check, then
//   the pointers that must be given
static int group_required(const char* what, int rc, std::initializer_list<const void*> ptrs) {
  if (rc) return rc;
  for (const void* p : ptrs)
    if (!p) {
      set_error("%s: null pointer", what);
      return BVQ_ERR_INVALID;
    }
  return BVQ_OK;
}
//   the pointers that must lie on 16-byte boundaries (a null one does), `names` for the text
static int group_aligned(const char* what, int rc, std::initializer_list<const void*> ptrs, const char* names) {
  if (rc) return rc;
  for (const void* p : ptrs)
    if (!aligned16(p)) {
      set_error("%s: %s must lie on 16-byte boundaries", what, names);
      return BVQ_ERR_UNSUPPORTED;
    }
  return BVQ_OK;
}
//   the launch: f(type_tag<T>, int_c<L>, std::bool_constant<NT>, grid) launches <<<grid, kBlock>>> the kernel whose
//   waves own `depth` loads; chunk_bytes: what the kernel moves per 16-byte chunk of the tensor, for the NT decision
template <typename F>
static int group_launch(const char* what, int dtype, int64_t group_size, int64_t chunks, int chunk_bytes, int depth,
                        F&& f) {
  const bool nt = chunks * chunk_bytes >= nt_threshold_bytes();
  const int64_t per_block = (int64_t)kWavesPerBlock * depth * kWave;
  const unsigned grid = (unsigned)((chunks + per_block - 1) / per_block);
  const int rc =
      with_group_variant(dtype, group_size, nt, [&](auto t, auto l, auto ntc) { return call_rc(f, t, l, ntc, grid); });
  return rc ? rc : check_launch(what);
}

}  // namespace bvq
