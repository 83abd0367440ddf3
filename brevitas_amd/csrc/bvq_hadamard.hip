// bvq_hadamard.hip -- the fast Walsh-Hadamard transform along the last dimension of x[rows, H], in blocks of b:
//   y = scale * (I_{H/b} (x) H_b) x,   H_b the Sylvester (natural-order) +-1 matrix, b a power of two dividing H.
//
// Definition (include/bvq.h, "Hadamard transform"): every element is widened to float32; stages h = 1, 2, 4 .. b/2 in
// this ascending order, in each of which every pair (i, i + h) with (i & h) == 0 becomes (u + v, u - v), one float32
// addition or subtraction each; one float32 multiply by float32(scale); one rounding to T.  Intermediates are float32
// from the load to the multiply, through LDS too.  The stage order fixes the roundings, hence the bits.
//
// A row is held as in the other row kernels (the row walk, bvq_row_walk.h):
//
//   C <=  128   kW = 1, kD = 2   one wave per row, four rows per workgroup, no LDS, no barrier
//   C <=  512   kW = 4, kD = 2   one workgroup per row
//   C <= 2048   kW = 4, kD = 8   one workgroup per row
//
// Lane l of wave w holds chunks j * 64 kW + 64 w + l, j = 0 .. kD - 1, from its only load to its only store (so y may
// be x).  An element's index in the row is, from the low bits up, [k: its place in the chunk][l: 6 bits][w: 0 or 2
// bits][j: 1 or 3 bits], and a stage h pairs the elements that differ in ONE of these bits, so ascending h is:
//   chunk stages        h < VEC            plain arithmetic on the registers of one chunk
//   lane stages         the six lane bits  cross-lane exchanges on the VALU, none through the LDS crossbar: d = 1, 2, 4,
//                                          8 a DPP move of the partner's value, then the lane with (l & d) == 0 keeps
//                                          own + partner, the other one partner - own; d = 16, 32 the half-swaps of
//                                          gfx950 (v_permlane16_swap, v_permlane32_swap) on two registers at a time
//   wave stages         the two wave bits  LDS, both stages from ONE exchange per load j: every wave writes the float32
//                                          values of its chunk, one barrier, every wave reads the other three waves'
//                                          values of its own (lane, k) positions and applies wave bit 0, then wave bit 1
//   chunk-index stages  the bits of j      plain arithmetic across the registers of the kD loads
// A block smaller than the row stops that sequence early: log2 b is a kernel argument and every test on it is scalar.
// b | H, so both elements of a pair lie in one block, which is inside the row or past its end as a whole: a lane past
// the row's end holds zeros (the descriptor's answer), pairs only with zeros, and its store is dropped.
//
// LDS.  One load's float32 image is 64 lanes x VEC floats per wave: 8 KiB per workgroup for the 16-bit types, 4 KiB
// for float32.  Two such slices alternate (load j uses slice j & 1), so ONE barrier per load suffices: a wave that
// writes slice j & 1 again for load j + 2 has passed the barrier of load j + 1, which every wave reaches only after
// its reads of load j.  16 KiB (8 KiB) per workgroup; every wave of a workgroup reaches every barrier (the grid is the
// rows, and what is skipped is skipped on values the whole workgroup shares).
//   reads x once, writes y once.  No workspace, no atomics, nothing between workgroups.
#include "bvq_row_walk.h"

namespace bvq {

struct HadamardArgs : WalkArgs {
  int64_t rows;
  uint32_t cpr;  // 16-byte chunks per row
  int32_t lb;    // log2 of the block
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

template <typename T, int kW, int kD, bool NT>
__global__ __launch_bounds__(kBlock) void hadamard_kernel(HadamardArgs a) {
  constexpr int VEC = elem<T>::vec, LV = VEC == 8 ? 3 : 2, LW = kW == 4 ? 2 : 0, LD = kD == 8 ? 3 : 1;
  static_assert((1 << LV) == VEC && (1 << LW) == kW && (1 << LD) == kD, "powers of two");
  RowSlot<kW> slot;
  if (!slot.init(a)) return;
  const buf_t bx = slot.template elems<T>(a.x, a), by = slot.template elems<T>(a.y, a);
  vec_t<T, VEC> xv[kD];
#pragma unroll
  for (int j = 0; j < kD; ++j) xv[j] = buf_load<T, VEC, NT>(bx, slot.chunk(j) * 16u);
  const int lb = a.lb;
  const uint32_t lane = threadIdx.x & 63;
  float v[kD][VEC];
#pragma unroll
  for (int j = 0; j < kD; ++j)
#pragma unroll
    for (int k = 0; k < VEC; ++k) v[j][k] = to_f<T>(xv[j].v[k]);

  // chunk stages and lane stages, load by load (a load that this wave has no chunk of is zeros and stays zeros)
#pragma unroll
  for (int j = 0; j < kD; ++j) {
    if (slot.first(j) >= a.cpr) break;  // wave-uniform
#pragma unroll
    for (int s = 0; s < LV; ++s) {
      if (s >= lb) break;
      const int h = 1 << s;
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        if (k & h) continue;
        const float u = v[j][k], w = v[j][k + h];
        v[j][k] = u + w;
        v[j][k + h] = u - w;
      }
    }
    lane_stages<VEC, LV>(v[j], lane, lb);
  }

  // wave stages: both from one exchange per load
  if constexpr (kW > 1) {
    if (lb > LV + 6) {
      __shared__ f4_t ex[2][kW][VEC / 4][kWave];
      const uint32_t w = slot.wave;
      const float s0 = (w & 1) ? -1.f : 1.f, s1 = (w & 2) ? -1.f : 1.f;
      const bool both = lb > LV + 7;
#pragma unroll
      for (int j = 0; j < kD; ++j) {
        if ((uint32_t)j * (kW * kWave) >= a.cpr) break;  // the same for every wave of the workgroup
#pragma unroll
        for (int q = 0; q < VEC / 4; ++q)
          ex[j & 1][w][q][lane] = f4_t{v[j][4 * q], v[j][4 * q + 1], v[j][4 * q + 2], v[j][4 * q + 3]};
        __syncthreads();
#pragma unroll
        for (int q = 0; q < VEC / 4; ++q) {
          const f4_t p1 = ex[j & 1][w ^ 1][q][lane];
          if (both) {
            const f4_t p2 = ex[j & 1][w ^ 2][q][lane], p3 = ex[j & 1][w ^ 3][q][lane];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              const float mine = pair_fold(s0, v[j][4 * q + k], p1[k]);  // wave bit 0: this wave's, and its partner's
              const float other = pair_fold(s0, p2[k], p3[k]);           // of wave bit 1
              v[j][4 * q + k] = pair_fold(s1, mine, other);
            }
          } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) v[j][4 * q + k] = pair_fold(s0, v[j][4 * q + k], p1[k]);
          }
        }
      }
    }
  }

  // chunk-index stages
#pragma unroll
  for (int s = 0; s < LD; ++s) {
    if (LV + 6 + LW + s >= lb) break;
    const int h = 1 << s;
#pragma unroll
    for (int j = 0; j < kD; ++j) {
      if (j & h) continue;
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        const float u = v[j][k], w = v[j + h][k];
        v[j][k] = u + w;
        v[j + h][k] = u - w;
      }
    }
  }

#pragma unroll
  for (int j = 0; j < kD; ++j) {
    if (slot.first(j) >= a.cpr) break;
    vec_t<T, VEC> o;
#pragma unroll
    for (int k = 0; k < VEC; ++k) o.v[k] = from_f<T>(v[j][k] * a.scale);
    buf_store<T, VEC, NT>(by, slot.chunk(j) * 16u, o);
  }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
// what the kernel covers, apart from the pointers: BVQ_OK and log2(block), or the error with its text
static int hadamard_check(const char* what, int dtype, int64_t rows, int64_t cols, int64_t block, int* lb) {
  if (bad_dtype(dtype)) {
    set_error("%s: bad dtype %d", what, dtype);
    return BVQ_ERR_INVALID;
  }
  if (rows < 1 || cols < 1) {
    set_error("%s: rows %lld, cols %lld (at least 1 each)", what, (long long)rows, (long long)cols);
    return BVQ_ERR_INVALID;
  }
  if (block < 2 || (block & (block - 1)) != 0) {
    set_error("%s: block %lld is no power of two >= 2", what, (long long)block);
    return BVQ_ERR_INVALID;
  }
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
  int l = 0;
  while (((int64_t)1 << l) < block) ++l;
  *lb = l;
  return BVQ_OK;
}

}  // namespace bvq

using namespace bvq;

extern "C" int bvq_hadamard_supported(int dtype, int64_t rows, int64_t cols, int64_t block, const void* x,
                                      const void* y) {
  int lb;
  if (hadamard_check("bvq_hadamard_supported", dtype, rows, cols, block, &lb)) return 0;
  return x && y && aligned16(x) && aligned16(y) ? 1 : 0;
}

extern "C" int bvq_hadamard(int dtype, const void* x, int64_t rows, int64_t cols, int64_t block, double scale, void* y,
                            bvq_stream_t stream) {
  const char* what = "bvq_hadamard";
  HadamardArgs a{};
  int rc = group_required(what, hadamard_check(what, dtype, rows, cols, block, &a.lb), {x, y});
  if ((rc = group_aligned(what, rc, {x, y}, "x and y"))) return rc;
  a.x = x;
  a.y = y;
  a.rows = rows;
  a.cpr = (uint32_t)(cols * dtype_size(dtype) / 16);
  a.chunks = rows * a.cpr;
  a.scale = (float)scale;
  // x read + y written
  return row_launch(what, dtype, a, 32, [&](auto t, auto w, auto depth, auto nt, unsigned grid) {
    hadamard_kernel<typename decltype(t)::type, w, depth, nt><<<grid, kBlock, 0, (hipStream_t)stream>>>(a);
  });
}
