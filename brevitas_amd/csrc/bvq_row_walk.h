// bvq_row_walk.h -- what the kernels that keep a whole ROW of x[rows, H] in registers share (bvq_row_shifted.hip: a token
// of the dynamic activation quantizers; bvq_weight_norm.hip: an output channel of a weight): where a wave stands, the
// exchange across the waves of a row, and the host side of a launch.
//
// A row of C = H * sizeof(T) / 16 chunks fits the registers of one workgroup:
//
//   C <=  128   kW = 1, kD = 2   one wave per row, four rows per workgroup, no LDS, no barrier
//   C <=  512   kW = 4, kD = 2   one workgroup per row
//   C <= 2048   kW = 4, kD = 8   one workgroup per row (2048 chunks = kRowMaxBytes)
//
// Lane l of wave w of the row holds chunks j * 64 kW + 64 w + l, j = 0 .. kD - 1, from its only load to its only
// store, through buffer descriptors whose extent ends with the row: a lane past the row's end reads zeros without a
// memory access and its store is dropped.  Row bases are 64-bit.  Within a wave values cross by butterflies
// (bvq_group_walk.h, seg_* with L = 64); across the kW waves of a row by row_exchange: one LDS write per wave, ONE
// barrier, every wave reads all kW and folds them in wave order.
// Args: a WalkArgs with `rows` and `cpr` (16-byte chunks per row).
#pragma once

#include "bvq_group_walk.h"

namespace bvq {

constexpr int64_t kRowMaxBytes = 32768;

// where a wave stands: its row, its place among the row's kW waves, its lanes' first chunk
template <int kW>
struct RowSlot {
  int64_t row;
  uint32_t wave;  // within the row
  uint32_t c0;    // the lane's chunk of load 0
  template <typename Args>
  __device__ __forceinline__ bool init(const Args& a) {
    const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if constexpr (kW == 1) {
      row = (int64_t)blockIdx.x * kWavesPerBlock + w;
      wave = 0;
    } else {
      static_assert(kW == kWavesPerBlock, "a row is held by one wave or by the whole workgroup");
      row = blockIdx.x;
      wave = w;
    }
    c0 = wave * kWave + (threadIdx.x & 63);
    return row < a.rows;  // (kW > 1: always, the grid is the rows -- every wave reaches the barrier)
  }
  // first chunk of the wave in load j (wave-uniform), and the lane's
  __device__ __forceinline__ uint32_t first(int j) const { return (uint32_t)j * (kW * kWave) + wave * kWave; }
  __device__ __forceinline__ uint32_t chunk(int j) const { return (uint32_t)j * (kW * kWave) + c0; }
  template <typename T, typename Args>
  __device__ __forceinline__ buf_t elems(const void* p, const Args& a) const {
    return make_buf(reinterpret_cast<const T*>(p) + row * ((int64_t)a.cpr * elem<T>::vec), a.cpr * 16u);
  }
};

// n values per wave across the kW waves of the row: ex[w][i] written by lane 0 of wave w, one barrier, all read by all
template <int kW, int N>
__device__ __forceinline__ void row_exchange(uint32_t (&ex)[kW][4], uint32_t wave, const uint32_t (&mine)[N],
                                             uint32_t (&all)[kW][N]) {
  static_assert(N <= 4, "row_exchange: up to four words per wave");
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int i = 0; i < N; ++i) ex[wave][i] = mine[i];
  }
  __syncthreads();
#pragma unroll
  for (int w = 0; w < kW; ++w)
#pragma unroll
    for (int i = 0; i < N; ++i) all[w][i] = ex[w][i];
}

__device__ __forceinline__ uint32_t uniform_u32(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}
__device__ __forceinline__ float uniform_f(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
// the launch: f(type_tag<T>, int_c<kW>, int_c<kD>, std::bool_constant<NT>, grid) for the geometry of the row length;
// chunk_bytes: what the kernel moves per 16-byte chunk of the tensor, for the NT decision
template <typename Args, typename F>
static int row_launch(const char* what, int dtype, const Args& a, int chunk_bytes, F&& f) {
  const bool nt = a.chunks * chunk_bytes >= nt_threshold_bytes();
  const unsigned one_wave = (unsigned)((a.rows + kWavesPerBlock - 1) / kWavesPerBlock), whole = (unsigned)a.rows;
  const int rc = with_dtype(dtype, [&](auto t) {
    return with_bool(nt, [&](auto ntc) {
      if (a.cpr <= 2 * kWave) return call_rc(f, t, int_c<1>{}, int_c<2>{}, ntc, one_wave);
      if (a.cpr <= 2 * kBlock) return call_rc(f, t, int_c<kWavesPerBlock>{}, int_c<2>{}, ntc, whole);
      return call_rc(f, t, int_c<kWavesPerBlock>{}, int_c<8>{}, ntc, whole);
    });
  });
  return rc ? rc : check_launch(what);
}
static_assert(8 * kBlock * 16 == kRowMaxBytes, "the deepest geometry holds the longest row");

}  // namespace bvq
