// gptq_lane_per_row.hip -- the REJECTED shape of the GPTQ column-loop kernel, kept as a developer experiment
// (tools/gptq_alt_bench.py builds and times it; profiles/gptq.md has the numbers).  One LANE per row on a TRANSPOSED
// float32 working copy [K, R]: a lane keeps the 128 columns of its row's block in registers, U is read wave-uniformly
// (scalar loads), nothing is computed twice -- but a layer of R rows gives only R / 64 waves, and the triangle of
// updates is 128 x 127 / 2 multiply-subtract pairs of straight-line code per division form.
// Covered: bfloat16, symmetric, group size 128 computed in the loop, whole blocks of 128 columns.  It uses the
// library's own statistic -> scale and forward chain (bvq_group_quant.h), so its codes are those of bvq_gptq_block.
#include "../brevitas_amd/csrc/bvq_group_quant.h"

using namespace bvq;

template <typename T>
__global__ __launch_bounds__(64) void gptq_lane_per_row_kernel(const float* __restrict__ wft, const float* __restrict__ u,
                                                               T* __restrict__ qt, float* __restrict__ et, int64_t rows,
                                                               int64_t cols, int64_t col0, float qmin_, float qmax_,
                                                               float min_val, float thr_div) {
  constexpr int B = 128;
  const int64_t r0 = (int64_t)blockIdx.x * 64 + threadIdx.x;
  const bool live = r0 < rows;
  const int64_t r = live ? r0 : rows - 1;  // a lane past the end works on the last row and stores nothing
  const float qmin = rnd<T>(qmin_), qmax = rnd<T>(qmax_);
  float w[B];
#pragma unroll
  for (int j = 0; j < B; ++j) w[j] = wft[(col0 + j) * rows + r];
  const float* ub = u + col0 * cols + col0;
  // the group is the block: its abs-max before any update
  uint32_t key = 0;
#pragma unroll
  for (int j = 0; j < B; ++j) {
    const uint32_t k = abs_bits<T>(from_f<T>(w[j]));
    key = k > key ? k : key;
  }
  const float s = group_scale<T>(key_value<T>(key), true, min_val, thr_div);
  auto body = [&](const auto& div) {
#pragma unroll
    for (int i = 0; i < B; ++i) {
      const f2 y = group_fwd_pair<T, false>(splat2(rnd<T>(w[i])), div, s, qmin, qmax);
      T qa, qb;
      pack2<T>(y, qa, qb);
      const float q = to_f<T>(qa);
      const float e = (w[i] - q) / ub[(int64_t)i * cols + i];
      if (live) {
        qt[(col0 + i) * rows + r] = qa;
        et[(int64_t)i * rows + r] = e;
      }
#pragma unroll
      for (int j = i + 1; j < B; ++j) w[j] = __fsub_rn(w[j], __fmul_rn(e, ub[(int64_t)i * cols + j]));
    }
  };
  if constexpr (sizeof(T) == 2) {
    if (wave_fast_div<T>(s)) {
      body(fast_div<T>(s));
      return;
    }
  }
  body(DivExact{s});
}

extern "C" int gptq_lane_per_row_block(const float* wft, const float* u, void* qt, float* et, int64_t rows,
                                       int64_t cols, int64_t col0, float qmin, float qmax, float min_val,
                                       float thr_div, void* stream) {
  if (!wft || !u || !qt || !et || rows < 1 || col0 < 0 || col0 + 128 > cols) return -1;
  const unsigned grid = (unsigned)((rows + 63) / 64);
  gptq_lane_per_row_kernel<bf16_t><<<grid, 64, 0, (hipStream_t)stream>>>(wft, u, reinterpret_cast<bf16_t*>(qt), et, rows,
                                                                           cols, col0, qmin, qmax, min_val, thr_div);
  return hipGetLastError() == hipSuccess ? 0 : -4;
}
