// bvq_hadamard.h -- what the two Hadamard kernels share (bvq_hadamard.hip: the Sylvester transform; bvq_hadamard_kron.hip:
// a Paley matrix of order 12, 20, 28, 36 times a Sylvester one): the arguments, the Sylvester stages inside a chunk and
// across the lanes of a wave for a row held on the row walk (the layout and the order of the stages: bvq_hadamard.hip),
// and the host checks of a row.
#pragma once

#include "bvq_row_walk.h"

namespace bvq {

struct HadamardArgs : WalkArgs {
  int64_t rows;
  uint32_t cpr;  // 16-byte chunks per row
  int32_t lb;    // log2 of the power-of-two block
  float scale;
};

typedef float f4_t __attribute__((ext_vector_type(4)));

// own + partner in the lower element of a pair, partner - own in the upper (sgn = +1 / -1): one fused multiply-add
// whose product is exact, hence the correctly rounded sum or difference
__device__ __forceinline__ float pair_fold(float sgn, float own, float partner) {
  return __builtin_fmaf(sgn, own, partner);
}

// the partner's value at lane stride D = 1, 2, 4, 8 as DPP moves (no LDS crossbar): quad permutes, a rotation of the
// 16-lane row by 8, and for 4 a shift either way, each written to the banks (groups of four lanes) that need it
template <int D>
__device__ __forceinline__ float dpp_xor(float x) {
  const int i = __builtin_bit_cast(int, x);
  int r;
  if constexpr (D == 1) {
    r = __builtin_amdgcn_update_dpp(i, i, 0xB1, 0xF, 0xF, false);  // quad_perm [1, 0, 3, 2]
  } else if constexpr (D == 2) {
    r = __builtin_amdgcn_update_dpp(i, i, 0x4E, 0xF, 0xF, false);  // quad_perm [2, 3, 0, 1]
  } else if constexpr (D == 4) {
    r = __builtin_amdgcn_update_dpp(i, i, 0x104, 0xF, 0x5, false);  // row_shl:4 -> banks 0, 2: from lane + 4
    r = __builtin_amdgcn_update_dpp(r, i, 0x114, 0xF, 0xA, false);  // row_shr:4 -> banks 1, 3: from lane - 4
  } else {
    static_assert(D == 8, "dpp_xor: 1, 2, 4 or 8");
    r = __builtin_amdgcn_update_dpp(i, i, 0x128, 0xF, 0xF, false);  // row_ror:8
  }
  return __builtin_bit_cast(float, r);
}

// One lane stage of stride 16 or 32 on TWO registers by the half-swaps of gfx950: after swap(a, b) the lower lane of
// a pair holds both values of a (its own and the upper lane's) and the upper lane both values of b; every lane adds
// and subtracts; the second swap hands the results back.  No sign, no select.
template <int D>
__device__ __forceinline__ void swap_stage(float& a, float& b) {
  typedef unsigned u2 __attribute__((ext_vector_type(2)));
  const unsigned ua = __builtin_bit_cast(unsigned, a), ub = __builtin_bit_cast(unsigned, b);
  u2 r;
  if constexpr (D == 16)
    r = __builtin_amdgcn_permlane16_swap(ua, ub, false, false);
  else
    r = __builtin_amdgcn_permlane32_swap(ua, ub, false, false);
  const float lo = __builtin_bit_cast(float, (unsigned)r[0]), hi = __builtin_bit_cast(float, (unsigned)r[1]);
  const unsigned us = __builtin_bit_cast(unsigned, lo + hi), ud = __builtin_bit_cast(unsigned, lo - hi);
  if constexpr (D == 16)
    r = __builtin_amdgcn_permlane16_swap(us, ud, false, false);
  else
    r = __builtin_amdgcn_permlane32_swap(us, ud, false, false);
  a = __builtin_bit_cast(float, (unsigned)r[0]);
  b = __builtin_bit_cast(float, (unsigned)r[1]);
}

template <int VEC, int LV>
__device__ __forceinline__ void lane_stages(float (&v)[VEC], uint32_t lane, int lb) {
  if (LV + 0 >= lb) return;
  {
    const float sgn = (lane & 1) ? -1.f : 1.f;
#pragma unroll
    for (int k = 0; k < VEC; ++k) v[k] = pair_fold(sgn, v[k], dpp_xor<1>(v[k]));
  }
  if (LV + 1 >= lb) return;
  {
    const float sgn = (lane & 2) ? -1.f : 1.f;
#pragma unroll
    for (int k = 0; k < VEC; ++k) v[k] = pair_fold(sgn, v[k], dpp_xor<2>(v[k]));
  }
  if (LV + 2 >= lb) return;
  {
    const float sgn = (lane & 4) ? -1.f : 1.f;
#pragma unroll
    for (int k = 0; k < VEC; ++k) v[k] = pair_fold(sgn, v[k], dpp_xor<4>(v[k]));
  }
  if (LV + 3 >= lb) return;
  {
    const float sgn = (lane & 8) ? -1.f : 1.f;
#pragma unroll
    for (int k = 0; k < VEC; ++k) v[k] = pair_fold(sgn, v[k], dpp_xor<8>(v[k]));
  }
  if (LV + 4 >= lb) return;
#pragma unroll
  for (int k = 0; k < VEC; k += 2) swap_stage<16>(v[k], v[k + 1]);
  if (LV + 5 >= lb) return;
#pragma unroll
  for (int k = 0; k < VEC; k += 2) swap_stage<32>(v[k], v[k + 1]);
}

// the stages h < VEC on the registers of one chunk (bvq_hadamard.hip spells the same loop out in its kernel: as a call
// it changes the register allocation of that file's deepest 16-bit instantiations, 104 -> 134 VGPRs)
template <int VEC, int LV>
__device__ __forceinline__ void chunk_stages(float (&v)[VEC], int lb) {
#pragma unroll
  for (int s = 0; s < LV; ++s) {
    if (s >= lb) break;
    const int h = 1 << s;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      if (k & h) continue;
      const float u = v[k], w = v[k + h];
      v[k] = u + w;
      v[k + h] = u - w;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// host side: the checks of an entry, around its own check of the block
// ------------------------------------------------------------------------------------------------
static int hadamard_shape_check(const char* what, int dtype, int64_t rows, int64_t cols) {
  if (bad_dtype(dtype)) {
    set_error("%s: bad dtype %d", what, dtype);
    return BVQ_ERR_INVALID;
  }
  if (rows < 1 || cols < 1) {
    set_error("%s: rows %lld, cols %lld (at least 1 each)", what, (long long)rows, (long long)cols);
    return BVQ_ERR_INVALID;
  }
  return BVQ_OK;
}

static int hadamard_row_check(const char* what, int dtype, int64_t rows, int64_t cols, int64_t block) {
  if (block > cols || cols % block != 0) {
    set_error("%s: block %lld does not divide cols %lld", what, (long long)block, (long long)cols);
    return BVQ_ERR_INVALID;
  }
  const int64_t bytes = cols * dtype_size(dtype);
  if (bytes % 16 != 0 || bytes > kRowMaxBytes) {
    set_error("%s: a row of %lld bytes (a multiple of 16, at most %lld)", what, (long long)bytes,
              (long long)kRowMaxBytes);
    return BVQ_ERR_UNSUPPORTED;
  }
  if (rows > (int64_t)0xffffffffll) {
    set_error("%s: %lld rows (at most 2^32 - 1)", what, (long long)rows);
    return BVQ_ERR_UNSUPPORTED;
  }
  return BVQ_OK;
}

}  // namespace bvq
