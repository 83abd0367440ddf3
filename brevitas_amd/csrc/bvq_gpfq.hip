// bvq_gpfq.hip -- the column loop of GPFQ weight quantization for one block of up to 128 input columns, one launch.
//
// GPFQ (greedy path-following quantization) picks each input column's code so that the quantized layer on the quantized
// path's input follows the float layer on the float input (include/bvq.h, "GPFQ").  Column i of a row is quantized at
// v = w_i + c_i / H[i, i], where the running correction c collects, for the columns left of i, the float weight times
// the drift of the input (the caller's Wf @ triu(D)) and the rounding errors e_j = w_j - q_j times H[j, i].  Rows are
// independent and a block of a row fits in registers: the frame of bvq_gptq.hip, ONE WAVE PER ROW, lane l holding columns
// l and l + 64 of Wf (read only) and of c.  In step i the owner's w and c are broadcast with a read-lane, every lane
// computes the same v, code and error, and updates the c of the columns it holds that lie right of i with its two
// values of H[i, .] (coalesced, loaded one step ahead).  Scale and zero-point are always given, for groups of any size
// that divides K, also groups that began before the block.  No LDS, no atomics, no workspace.
//   reads   the block's columns of Wf and C, the [B, B] triangle of H, scale / zero-point
//   writes  the block's columns of Q, E [R, B] float32
#include "bvq_column_loop.h"

namespace bvq {

// GroupArgs: x = Wf (float32 [rows, cols]), y = Q (T [rows, cols]), scale = [rows, cols / gsize] of T
struct GpfqArgs : GroupArgs {
  const float* c;   // [rows, cols]
  const float* h;   // [cols, cols]
  float* err;       // [rows, bc]
  const void* zp;   // [rows, cols / gsize] of T, asymmetric only
  int64_t rows, cols, col0;
  int32_t bc, gsize;
};

template <typename T, bool kZp>
__global__ __launch_bounds__(kBlock) void gpfq_block_kernel(GpfqArgs a) {
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t r = (int64_t)blockIdx.x * kWavesPerBlock + wave;
  if (r >= a.rows) return;  // wave-uniform
  const int lane = threadIdx.x & 63;
  const int bc = a.bc;
  const bool in0 = lane < bc, in1 = lane + 64 < bc;
  const float* wrow = reinterpret_cast<const float*>(a.x) + r * a.cols + a.col0;
  const float* crow = a.c + r * a.cols + a.col0;
  const float* hb = a.h + a.col0 * a.cols + a.col0;  // H[col0, col0]
  const float w0 = in0 ? wrow[lane] : 0.f, w1 = in1 ? wrow[lane + 64] : 0.f;
  float c0 = in0 ? crow[lane] : 0.f, c1 = in1 ? crow[lane + 64] : 0.f;
  const float qmin = rnd<T>(a.qmin), qmax = rnd<T>(a.qmax);
  const int64_t gpr = a.cols / a.gsize;  // groups per row
  const T* const srow = reinterpret_cast<const T*>(a.scale) + r * gpr;
  const T* const zrow = kZp ? reinterpret_cast<const T*>(a.zp) + r * gpr : nullptr;

  // the lane's own columns' scale and zero-point
  const int64_t g0 = (a.col0 + lane) / a.gsize, g1 = (a.col0 + lane + 64) / a.gsize;
  const float s0 = in0 ? to_f<T>(srow[g0]) : 0.f, s1 = in1 ? to_f<T>(srow[g1]) : 0.f;
  float z0 = 0.f, z1 = 0.f;
  if constexpr (kZp) {
    z0 = in0 ? to_f<T>(zrow[g0]) : 0.f;
    z1 = in1 ? to_f<T>(zrow[g1]) : 0.f;
  }

  float s = 0.f, zp = 0.f, q0 = 0.f, q1 = 0.f, e0 = 0.f, e1 = 0.f;
  // the division by s that the wave takes (bvq_group_quant.h) and its reciprocal, kept from one change of s to the next
  bool fast = false;
  float rs = 0.f;
  int64_t togo = 0;  // steps until the next group's scale and zero-point apply
  // row i of the triangle, one step ahead of its use
  float h0 = in0 ? hb[lane] : 0.f, h1 = in1 ? hb[lane + 64] : 0.f, d = hb[0];
  for (int i = 0; i < bc; ++i) {
    const float ch0 = h0, ch1 = h1, cd = d;
    if (i + 1 < bc) {  // wave-uniform
      const float* hn = hb + (int64_t)(i + 1) * a.cols;
      h0 = in0 ? hn[lane] : 0.f;
      h1 = in1 ? hn[lane + 64] : 0.f;
      d = hn[i + 1];
    }
    const int src = i & 63;
    const bool hi = i >= 64;
    if (togo == 0) {  // wave-uniform
      togo = a.gsize - (a.col0 + i) % a.gsize;
      s = read_lane(hi ? s1 : s0, src);
      if constexpr (kZp) zp = read_lane(hi ? z1 : z0, src);
      if constexpr (sizeof(T) == 2) {
        fast = wave_fast_div<T>(s);
        rs = 1.0f / s;
      }
    }
    --togo;
    const float wi = read_lane(hi ? w1 : w0, src);
    const float ci = read_lane(hi ? c1 : c0, src);
    // IEEE division, then the sum; a column whose input never fired is rounded to nearest
    const float v = cd > 0.f ? __fadd_rn(wi, ci / cd) : wi;
    const f2 xt = splat2(rnd<T>(v));
    f2 y;
    if (sizeof(T) == 2 && fast)
      y = group_fwd_pair<T, kZp>(xt, fast_div<T>(s, rs), s, qmin, qmax, zp);
    else
      y = group_fwd_pair<T, kZp>(xt, DivExact{s}, s, qmin, qmax, zp);
    T qa, qb;
    pack2<T>(y, qa, qb);
    const float q = to_f<T>(qa);
    const float e = __fsub_rn(wi, q);  // against the original weight, not v
    const bool own = lane == src;
    q0 = (own && !hi) ? q : q0;
    e0 = (own && !hi) ? e : e0;
    q1 = (own && hi) ? q : q1;
    e1 = (own && hi) ? e : e1;
    // the columns right of i: product rounded, then the sum rounded (no fused multiply-add)
    const float n0 = __fadd_rn(c0, __fmul_rn(e, ch0)), n1 = __fadd_rn(c1, __fmul_rn(e, ch1));
    c0 = (!hi && lane > src) ? n0 : c0;
    c1 = (!hi || lane > src) ? n1 : c1;
  }

  T* qrow = reinterpret_cast<T*>(a.y) + r * a.cols + a.col0;
  float* erow = a.err + r * bc;
  if (in0) {
    qrow[lane] = from_f<T>(q0);
    erow[lane] = e0;
  }
  if (in1) {
    qrow[lane + 64] = from_f<T>(q1);
    erow[lane + 64] = e1;
  }
}

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
  const char* what = "bvq_gpfq_block";
  int rc = column_block_check(d, what, rows, cols, col0, block_cols, 0);
  const bool shifted = !rc && d->zp_per_channel;
  rc = group_required(what, rc, {wf, c, h, q, err, scale});
  if (!rc && shifted && !zp) {
    set_error("%s: null pointer (zp of an asymmetric quantizer)", what);
    return BVQ_ERR_INVALID;
  }
  if ((rc = group_aligned(what, rc, {wf, c, h, q, err}, "wf, c, h, q and err"))) return rc;
  GpfqArgs a = group_args<GpfqArgs>(d, 0.0, 0, 1.0);
  a.x = wf;
  a.y = q;
  a.scale = const_cast<void*>(scale);  // read only here
  a.c = c;
  a.h = h;
  a.err = err;
  a.zp = zp;
  a.rows = rows;
  a.cols = cols;
  a.col0 = col0;
  a.bc = block_cols;
  a.gsize = (int32_t)d->inner;
  const unsigned grid = (unsigned)((rows + kWavesPerBlock - 1) / kWavesPerBlock);
  rc = with_dtype(d->x_dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    return with_bool(shifted, [&](auto z) {
      gpfq_block_kernel<T, decltype(z)::value><<<grid, kBlock, 0, (hipStream_t)stream>>>(a);
    });
  });
  return rc ? rc : check_launch(what);
}
