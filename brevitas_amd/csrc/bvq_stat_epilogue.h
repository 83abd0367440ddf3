// bvq_stat_epilogue.h -- what follows a per-channel abs-max statistic, on the device: the statistic's store, the
// scale epilogue (clamp_min -> / int_threshold) and _RuntimeStats' running average.  Shared by the statistic's
// finishing code (bvq_stats.hip) and the one-pass statistic + quantizer of channels held by a cluster of workgroups
// (bvq_fakequant_fwd.hip), so that both write the same bits.
#pragma once

#include "bvq_common.h"

namespace bvq {

__device__ __forceinline__ void store_stat(void* out, int out_dtype, int64_t idx, float v) {
  if (out_dtype == BVQ_F32)
    reinterpret_cast<float*>(out)[idx] = v;
  else if (out_dtype == BVQ_BF16)
    reinterpret_cast<bf16_t*>(out)[idx] = (bf16_t)v;  // exact: v is a bf16 value
  else
    reinterpret_cast<f16_t*>(out)[idx] = (f16_t)v;
}

// optional epilogue of the abs-max finisher: statistic -> scale in the same launch
//   thr   = scalar_clamp_min_ste(stat, min_val)      (B/core/restrict_val.py:22-42)
//   scale = thr / int_threshold                       (B/core/quant/int.py:160)
// min_val is already rounded to the statistic's dtype and int_threshold to the dtype the division
// runs in, so the kernel only has to round the quotient to scale_dtype.
struct ScaleEpilogue {
  void* scale_out;  // null: no epilogue
  int32_t scale_dtype;
  int32_t use_min;
  float min_val;
  float int_threshold;
  // optionally, in the same launch: _RuntimeStats' running average of the statistic (B/core/stats/stats_wrapper.py:61-66)
  void* running;    // null: none
  int32_t run_dtype, first_batch;
  float momentum, one_minus_m;
};

// The epilogue from the arguments of the C ABI (host side).  scale_epilogue: the scale part; min_val is a python scalar
// that torch converts to the statistic's dtype.  A null scale_out gives the empty epilogue.
inline ScaleEpilogue scale_epilogue(void* scale_out, int scale_dtype, int use_min, double min_val, int stat_dtype,
                                    double int_threshold) {
  ScaleEpilogue ep = {};
  if (!scale_out) return ep;
  ep.scale_out = scale_out;
  ep.scale_dtype = scale_dtype;
  ep.use_min = use_min;
  ep.min_val = round_host((float)min_val, stat_dtype);
  ep.int_threshold = (float)int_threshold;
  return ep;
}

// with_running: `ep` and the running average; torch turns the python scalars (1 - momentum) and momentum into float32
// for these dtypes (bvq_running_stats_update).  A null running adds nothing.
inline ScaleEpilogue with_running(ScaleEpilogue ep, int run_dtype, void* running, double momentum, int first_batch) {
  if (!running) return ep;
  ep.running = running;
  ep.run_dtype = run_dtype;
  ep.first_batch = first_batch;
  ep.one_minus_m = (float)(1.0 - momentum);
  ep.momentum = (float)momentum;
  return ep;
}

// running *= out (first batch)  |  running *= (1 - momentum); running += momentum * out -- every torch op rounds to
// its result dtype: running's for the in-place ops, out's for momentum * out
__device__ __forceinline__ float running_update(float r, float o, int run_dtype, int stat_dtype, float one_minus_m,
                                                float m, int first) {
  auto round_to = [](float v, int dt) {
    return dt == BVQ_F32 ? v : (dt == BVQ_BF16 ? rnd<bf16_t>(v) : rnd<f16_t>(v));
  };
  if (first) return round_to(r * o, run_dtype);
  r = round_to(r * one_minus_m, run_dtype);
  const float u = round_to(o * m, stat_dtype);
  return round_to(r + u, run_dtype);
}

// statistic, scale epilogue, running statistic of channel c from the abs-max key `bits` (an abs_bits<> key of in_dtype)
__device__ __forceinline__ void absmax_epilogue(void* stat_out, int stat_dtype, int in_dtype, const ScaleEpilogue& ep,
                                                int32_t c, uint32_t bits) {
  const float v = in_dtype == BVQ_F16 ? (float)__builtin_bit_cast(f16_t, (uint16_t)bits) : __builtin_bit_cast(float, bits);
  store_stat(stat_out, stat_dtype, c, v);
  if (ep.scale_out) {
    const float thr = (ep.use_min && v < ep.min_val) ? ep.min_val : v;  // NaN passes, like torch.clamp_min
    store_stat(ep.scale_out, ep.scale_dtype, c, thr / ep.int_threshold);
  }
  if (ep.running) {
    const float run = load_scalar_as_f(ep.running, ep.run_dtype, c);
    store_stat(ep.running, ep.run_dtype, c,
               running_update(run, v, ep.run_dtype, stat_dtype, ep.one_minus_m, ep.momentum, ep.first_batch));
  }
}

}  // namespace bvq
