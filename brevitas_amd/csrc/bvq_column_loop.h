// bvq_column_loop.h -- what the column-loop kernels share (bvq_gptq.hip, bvq_gpfq.hip): one wave per row, a block of up
// to 128 input columns in registers, lane l holding columns l and l + 64.  The block width, the read-lane broadcast of
// the owner's value and the host-side coverage check of descriptor, shape and block.
#pragma once

#include "bvq_group_shifted.h"

namespace bvq {

constexpr int kColumnBlock = 128;  // columns of a block: two per lane

__device__ __forceinline__ float read_lane(float v, int lane) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
// what a column-loop kernel covers apart from the pointers: BVQ_OK, or the error with its text
// computed: scale and zero-point are computed in the loop, at each group start (GPTQ only)
static int column_block_check(const bvq_quant_desc* d, const char* what, int64_t rows, int64_t cols, int64_t col0,
                              int block_cols, int computed) {
  int rc = validate(d);
  if (rc) return rc;
  if (d->outer != 1 || d->channels < 1 || d->inner < 1 || !d->scale_per_channel) {
    set_error("%s: the descriptor of a grouped tensor is outer 1, channels = groups, inner = group size, one scale per "
              "channel", what);
    return BVQ_ERR_UNSUPPORTED;
  }
  if (d->round_mode != BVQ_ROUND || d->pre_op != BVQ_PRE_NONE || d->out_kind != BVQ_OUT_DEQUANT) {
    set_error("%s: half-even rounding, no pre_op and dequantized output only (round_mode=%d pre_op=%d out_kind=%d)", what,
              d->round_mode, d->pre_op, d->out_kind);
    return BVQ_ERR_UNSUPPORTED;
  }
  if (d->x_dtype != d->ct_dtype || d->scale_dtype != d->x_dtype || (d->zp_per_channel && d->zp_dtype != d->x_dtype)) {
    set_error("%s: x, compute, scale and zero-point dtype must agree (x=%d ct=%d scale=%d zp=%d)", what, d->x_dtype,
              d->ct_dtype, d->scale_dtype, d->zp_dtype);
    return BVQ_ERR_UNSUPPORTED;
  }
  if (rows < 1 || cols < 1 || cols % d->inner != 0 || rows * (cols / d->inner) != d->channels) {
    set_error("%s: rows %lld x cols %lld is not %lld groups of %lld", what, (long long)rows, (long long)cols,
              (long long)d->channels, (long long)d->inner);
    return BVQ_ERR_INVALID;
  }
  if (block_cols < 1 || block_cols > kColumnBlock) {
    set_error("%s: block_cols %d (1 .. %d)", what, block_cols, kColumnBlock);
    return BVQ_ERR_INVALID;
  }
  if (col0 < 0 || col0 + block_cols > cols) {
    set_error("%s: columns %lld .. %lld of %lld", what, (long long)col0, (long long)(col0 + block_cols), (long long)cols);
    return BVQ_ERR_INVALID;
  }
  if (computed) {
    if (d->inner != 16 && d->inner != 32 && d->inner != 64 && d->inner != 128) {
      set_error("%s: group size %lld (16, 32, 64 or 128 where scale and zero-point are computed in the loop)", what,
                (long long)d->inner);
      return BVQ_ERR_UNSUPPORTED;
    }
    if (col0 % d->inner != 0 || block_cols % d->inner != 0) {
      set_error("%s: col0 %lld and block_cols %d must be multiples of the group size %lld", what, (long long)col0,
                block_cols, (long long)d->inner);
      return BVQ_ERR_INVALID;
    }
  }
  return BVQ_OK;
}

}  // namespace bvq
