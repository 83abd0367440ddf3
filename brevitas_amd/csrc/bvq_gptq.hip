// bvq_gptq.hip -- the column loop of GPTQ weight quantization for one block of up to 128 input columns, one launch.
//
// GPTQ quantizes a weight [R, K] one input column at a time and pushes each column's error onto the columns not yet
// quantized, through the upper Cholesky factor U of the damped inverse Hessian (include/bvq.h, "GPTQ").  Rows are
// independent in that loop and a block of a row fits in registers: the frame of bvq_column_loop.h, a lane's running
// state being its two columns of the block's float32 working copy.  Step i quantizes the owner's value as it stands, and
// every lane takes e * U[i, .] off the columns it holds right of i.  Scale and zero-point are given, or computed in the
// loop at each group start from the working copy as it stands.
//   reads   the block's columns of Wf, the [B, B] triangle of U (+ scale / zero-point where they are given)
//   writes  the block's columns of Q, E [R, B] float32 (+ the block's scale / zero-point where they are computed)
#include "bvq_column_loop.h"

namespace bvq {

struct GptqRule {
  static constexpr bool kCorrection = false;  // the running state is the working weight
  static __device__ __forceinline__ float value(float wi, float, float) { return wi; }
  static __device__ __forceinline__ float error(float wi, float q, float cd) { return (wi - q) / cd; }  // IEEE division
  static __device__ __forceinline__ float update(float w, float p) { return __fsub_rn(w, p); }
};

}  // namespace bvq

using namespace bvq;

extern "C" int bvq_gptq_block_supported(const bvq_quant_desc* d, int64_t rows, int64_t cols, int64_t col0,
                                        int block_cols, int computed, const void* wf, const void* u, const void* q) {
  if (column_block_check(d, "bvq_gptq_block_supported", rows, cols, col0, block_cols, computed)) return 0;
  return wf && u && q && aligned16(wf) && aligned16(u) && aligned16(q) ? 1 : 0;
}

extern "C" int bvq_gptq_block(const bvq_quant_desc* d, const float* wf, const float* u, int64_t rows, int64_t cols,
                              int64_t col0, int block_cols, int computed, double min_val, int use_min, double thr_div,
                              void* q, float* err, void* scale, void* zp, bvq_stream_t stream) {
  return column_block_launch<GptqRule, 0, 16, 32, 64, 128>("bvq_gptq_block", d, wf, nullptr, u, rows, cols, col0,
                                                           block_cols, computed, min_val, use_min, thr_div, q, err,
                                                           scale, zp, "wf, u, q and err", stream);
}
