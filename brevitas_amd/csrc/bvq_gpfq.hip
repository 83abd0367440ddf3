// bvq_gpfq.hip -- the column loop of GPFQ weight quantization for one block of up to 128 input columns, one launch.
//
// GPFQ (greedy path-following quantization) picks each input column's code so that the quantized layer on the quantized
// path's input follows the float layer on the float input (include/bvq.h, "GPFQ").  Column i of a row is quantized at
// v = w_i + c_i / H[i, i], where the running correction c collects, for the columns left of i, the float weight times
// the drift of the input (the caller's Wf @ triu(D)) and the rounding errors e_j = w_j - q_j times H[j, i].  Rows are
// independent and a block of a row fits in registers: the frame of bvq_column_loop.h, a lane's running state being its
// two columns of c, beside its two columns of Wf (read only).  Every lane adds e * H[i, .] to the c of the columns it
// holds right of i.  Scale and zero-point are always given, for groups of any size that divides K.
//   reads   the block's columns of Wf and C, the [B, B] triangle of H, scale / zero-point
//   writes  the block's columns of Q, E [R, B] float32
#include "bvq_column_loop.h"

namespace bvq {

struct GpfqRule {
  static constexpr bool kCorrection = true;  // the running state is c, beside the weight
  // IEEE division, then the sum; a column whose input never fired is rounded to nearest
  static __device__ __forceinline__ float value(float wi, float ci, float cd) {
    return cd > 0.f ? __fadd_rn(wi, ci / cd) : wi;
  }
  // against the original weight, not v
  static __device__ __forceinline__ float error(float wi, float q, float) { return __fsub_rn(wi, q); }
  static __device__ __forceinline__ float update(float c, float p) { return __fadd_rn(c, p); }
};

}  // namespace bvq

using namespace bvq;

extern "C" int bvq_gpfq_block_supported(const bvq_quant_desc* d, int64_t rows, int64_t cols, int64_t col0,
                                        int block_cols, const void* wf, const void* c, const void* h, const void* q) {
  if (column_block_check(d, "bvq_gpfq_block_supported", rows, cols, col0, block_cols, 0)) return 0;
  return wf && c && h && q && aligned16(wf) && aligned16(c) && aligned16(h) && aligned16(q) ? 1 : 0;
}

extern "C" int bvq_gpfq_block(const bvq_quant_desc* d, const float* wf, const float* c, const float* h, int64_t rows,
                              int64_t cols, int64_t col0, int block_cols, void* q, float* err, const void* scale,
                              const void* zp, bvq_stream_t stream) {
  // scale and zp are read only here: the one instantiated group size is 0, given parameters
  return column_block_launch<GpfqRule, 0>("bvq_gpfq_block", d, wf, c, h, rows, cols, col0, block_cols, 0, 0.0, 0, 1.0, q,
                                          err, const_cast<void*>(scale), const_cast<void*>(zp),
                                          "wf, c, h, q and err", stream);
}
