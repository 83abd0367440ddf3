// bvq_group_clip.hip -- AWQ's activation-aware clip search over one group-wise quantized weight, one launch: of n <= 16
// candidate thresholds t_i = abs-max * ratio_i (ratio_0 = 1, the candidates of bvq_group_mse.hip) a group of g input
// columns takes the first one with the smallest OUTPUT error d^T H_jj d, d = y_i - x and H_jj the g x g diagonal block of
// the layer's input Hessian that belongs to the group's columns.
//
// The error costs g^2 multiply-adds per (row, group, candidate), so this kernel does not use the sub-wave group walk:
// it is a small dense product per group on the matrix cores, float32 in and out (the argmin compares losses that
// differ by rounding-sized amounts).
//
// Work split.  A workgroup of 4 waves takes one group column j and kClipRows rows.  It copies hb[j] (g * g floats:
// 64 KiB at g = 128) into LDS once; its waves then loop over the rows, one (row, group) per wave iteration, the next
// row's x asked for before the current one is worked on.  hb is read R / kClipRows times in all: at most half the
// weight's own bytes (g = 128, 16-bit weights), and from L2.
//
// Matrix product.  v_mfma_f32_16x16x4_f32 with M = the candidates: P[16 cand, 16 cols] += D[16 cand, 4 k] * hb[4 k,
// 16 cols], rows of D past n zero.  Which column of the group a (step, k) pair or a (tile, n) pair stands for is free as
// long as D and hb agree, and it is chosen so that every lane's share of x is one contiguous run:
//   A operand  lane l, step s  : candidate l % 16, column (l / 16) * (g / 4) + s          -> g / 4 consecutive elements
//   C tile t   lane l, reg i   : candidate 4 * (l / 16) + i, column (l % 16) * (g / 16) + t -> g / 16 consecutive elements
// A candidate's scale depends on the group's abs-max and ratio_i alone, so after one 16-lane butterfly for the abs-max
// a lane computes d of its candidate directly in the A layout, and again in the C layout for sum(P o D): no
// transposition of D, nothing of D in LDS.  hb lies in LDS in the order the B operand reads it: row a, column b at
// a * g + (((b % (g/16)) * 16 + b / (g/16)) ^ swizzle(a)), swizzle(a) = 16 * (a / (g/4)) mod g, so that the four rows a
// B read touches fall into different banks (g >= 64; two-way at g = 32, where a row is half the banks).
//
// The sum over a tile's 16 columns is a DPP row reduction, the sum over the g / 16 tiles a register add.  The pick is
// a wave-uniform walk over the n losses by v_readlane (first strict minimum; a NaN loss is below nothing, so a NaN or
// Inf group keeps candidate 0).  Then the first 16 lanes quantize the group with the winning scale and store y once;
// scale, stat and the index byte go out per group, the n losses from the lanes that hold them.
//   reads x once and hb R / kClipRows times, writes y  (+ 2 * bytes(x) / g + (1 + 4 n) bytes per group)
// Nothing of size [n, R, K] exists; no workspace, no atomics.  For a given index y, scale and stat have the bits of
// bvq_group_mse_fwd's.
#include "bvq_group_quant.h"

namespace bvq {

constexpr int kClipMaxCandidates = 16;  // the M dimension of the matrix instruction
constexpr int kClipRows = 512;          // rows of one workgroup: hb[j] is loaded once for them

struct GroupClipArgs {
  const void* x;
  const float* hb;  // [K / g, g, g]
  void* y;
  void* scale;      // [R, K / g] in x's dtype
  void* stat;       // likewise
  uint8_t* idx;     // [R, K / g]
  float* losses;    // [R, K / g, n]
  int64_t rows, k;
  int32_t n, use_min;
  float qmin, qmax, min_val, thr_div;
  float ratio[kClipMaxCandidates];
};

typedef float f4 __attribute__((ext_vector_type(4)));

template <typename T, int N>
struct run_t {
  T v[N];
};

// N consecutive elements from p, which lies on a boundary of min(16, N * sizeof(T)) bytes
template <typename T, int N>
__device__ __forceinline__ run_t<T, N> load_run(const T* p) {
  constexpr int kPer = N * (int)sizeof(T) >= 16 ? 16 / (int)sizeof(T) : N;
  run_t<T, N> out;
#pragma unroll
  for (int k = 0; k < N; k += kPer) {
    const vec_t<T, kPer> v = load_vec<T, kPer>(p + k);
#pragma unroll
    for (int e = 0; e < kPer; ++e) out.v[k + e] = v.v[e];
  }
  return out;
}
template <typename T, int N>
__device__ __forceinline__ void store_run(T* p, const run_t<T, N>& r) {
  constexpr int kPer = N * (int)sizeof(T) >= 16 ? 16 / (int)sizeof(T) : N;
#pragma unroll
  for (int k = 0; k < N; k += kPer) {
    vec_t<T, kPer> v;
#pragma unroll
    for (int e = 0; e < kPer; ++e) v.v[e] = r.v[k + e];
    store_vec<T, kPer>(p + k, v);
  }
}

// a run quantized at the scale s: the values of T the forward would store (group_fwd_chunk on a run)
template <typename T, int N, typename Div>
__device__ __forceinline__ run_t<T, N> clip_quant(const run_t<T, N>& x, const Div& div, float s, float qmin,
                                                  float qmax) {
  run_t<T, N> y;
  if constexpr (N == 1) {
    T unused;
    pack2<T>(group_fwd_pair<T>(widen2<T>(x.v[0], x.v[0]), div, s, qmin, qmax), y.v[0], unused);
  } else {
#pragma unroll
    for (int k = 0; k < N; k += 2)
      pack2<T>(group_fwd_pair<T>(widen2<T>(x.v[k], x.v[k + 1]), div, s, qmin, qmax), y.v[k], y.v[k + 1]);
  }
  return y;
}

// d = float32(y) - float32(x) of a run at the scale s, y as clip_quant stores it (group_err_chunk's difference); zeros
// where !live: a row of D past the last candidate
template <typename T, int N>
__device__ __forceinline__ run_t<float, N> clip_diff(const run_t<T, N>& x, float s, float qmin, float qmax, bool live) {
  return with_group_div<T>(s, [&](const auto& div) {
    const run_t<T, N> y = clip_quant<T, N>(x, div, s, qmin, qmax);
    run_t<float, N> d;
#pragma unroll
    for (int k = 0; k < N; ++k) d.v[k] = live ? to_f<T>(y.v[k]) - to_f<T>(x.v[k]) : 0.f;
    return d;
  });
}

// the sum over the 16 lanes of a DPP row, the same bits in each of them (every exchange adds the same two values)
__device__ __forceinline__ float row16_sum(float v) {
#define BVQ_ROW_ADD(ctrl) \
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), ctrl, 0xF, 0xF, false))
  BVQ_ROW_ADD(0xB1);   // quad_perm [1, 0, 3, 2]
  BVQ_ROW_ADD(0x4E);   // quad_perm [2, 3, 0, 1]
  BVQ_ROW_ADD(0x141);  // row_half_mirror: the other quad pair's sum
  BVQ_ROW_ADD(0x140);  // row_mirror: the other half's
#undef BVQ_ROW_ADD
  return v;
}

template <typename T, int G>
__global__ __launch_bounds__(kBlock, 2) void group_clip_kernel(GroupClipArgs a) {
  constexpr int NA = G / 4, NC = G / 16;
  __shared__ float hs[G * G];
  const int tid = threadIdx.x, lane = tid & 63, q = lane >> 4, n16 = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t j = blockIdx.x, gpr = a.k / G;

  // hb[j] into LDS, in the B operand's order
  const float* hb = a.hb + j * (G * G);
  for (int e = tid * 4; e < G * G; e += kBlock * 4) {
    const vec_t<float, 4> v = load_vec<float, 4>(hb + e);
    const int r = e / G, b = e % G;
    float* row = hs + r * G;
    const int sw = ((r / NA) << 4) & (G - 1);
#pragma unroll
    for (int c = 0; c < 4; ++c) row[((((b + c) % NC) << 4) + (b + c) / NC) ^ sw] = v.v[c];
  }
  __syncthreads();

  // the lane's ratios: candidate n16 in the A layout, candidates 4 q + i in the C layout.  A uniform walk over the table
  // with conditional moves, never an index by the lane's value; a candidate past n keeps ratio 1 and is not live.
  const int n = a.n;
  float ra = 1.f, rc[4] = {1.f, 1.f, 1.f, 1.f};
  for (int c = 0; c < n; ++c) {
    const float r = a.ratio[c];
    ra = n16 == c ? r : ra;
#pragma unroll
    for (int i = 0; i < 4; ++i) rc[i] = 4 * q + i == c ? r : rc[i];
  }
  const bool use_min = a.use_min != 0;
  const float qmin = rnd<T>(a.qmin), qmax = rnd<T>(a.qmax);
  const float* bq = hs + q * NA * G;  // the lane's rows of hb: q * NA + step
  const int swq = (q << 4) & (G - 1);

  const int64_t row0 = (int64_t)blockIdx.y * kClipRows;
  const int64_t row_end = row0 + kClipRows < a.rows ? row0 + kClipRows : a.rows;
  int64_t row = row0 + wave;
  if (row >= row_end) return;
  const T* xg = reinterpret_cast<const T*>(a.x) + row * a.k + j * G;
  run_t<T, NA> xa = load_run<T, NA>(xg + q * NA);
  run_t<T, NC> xc = load_run<T, NC>(xg + n16 * NC);
  for (; row < row_end; row += kWavesPerBlock) {
    const run_t<T, NA> xa0 = xa;
    const run_t<T, NC> xc0 = xc;
    if (row + kWavesPerBlock < row_end) {  // wave-uniform
      const T* xn = reinterpret_cast<const T*>(a.x) + (row + kWavesPerBlock) * a.k + j * G;
      xa = load_run<T, NA>(xn + q * NA);
      xc = load_run<T, NC>(xn + n16 * NC);
    }
    // the group's abs-max: every DPP row holds the whole group
    uint32_t key = 0;
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      const uint32_t b = abs_bits<T>(xc0.v[k]);
      key = b > key ? b : key;
    }
    const float stat = key_value<T>(seg_max_u32<16>(key));

    // D in the A layout and the product
    const float sa = group_scale<T>(mse_threshold<T>(stat, ra), use_min, a.min_val, a.thr_div);
    const run_t<float, NA> da = clip_diff<T, NA>(xa0, sa, qmin, qmax, n16 < n);
    f4 acc[NC];
#pragma unroll
    for (int t = 0; t < NC; ++t) acc[t] = f4{0.f, 0.f, 0.f, 0.f};
    // the B fragments of step s + 1 are asked for before the products of step s; the scheduling barrier keeps the
    // compiler from hoisting every LDS read of the loop to its top (g * g / 64 registers)
    float b[NC], bn[NC];
#pragma unroll
    for (int t = 0; t < NC; ++t) b[t] = bq[((t << 4) + n16) ^ swq];
#pragma unroll
    for (int s = 0; s < NA; ++s) {
      if (s + 1 < NA) {
#pragma unroll
        for (int t = 0; t < NC; ++t) bn[t] = bq[(s + 1) * G + (((t << 4) + n16) ^ swq)];
      }
#pragma unroll
      for (int t = 0; t < NC; ++t) {
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(da.v[s], b[t], acc[t], 0, 0, 0);
        b[t] = bn[t];
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    // D again in the C layout: sum(P o D) over the lane's columns, then over the row's 16 lanes
    float loss[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float sc = group_scale<T>(mse_threshold<T>(stat, rc[i]), use_min, a.min_val, a.thr_div);
      const run_t<float, NC> dc = clip_diff<T, NC>(xc0, sc, qmin, qmax, 4 * q + i < n);
      float part = 0.f;
#pragma unroll
      for (int t = 0; t < NC; ++t) part += acc[t][i] * dc.v[t];
      loss[i] = row16_sum(part);
    }
    // the pick: candidate c's loss is register c % 4 of row c / 4
    float e_best = 0.f, r_best = 1.f;
    uint32_t k_best = 0;
#pragma unroll
    for (int c = 0; c < kClipMaxCandidates; ++c) {
      const float e =
          __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, loss[c & 3]), 16 * (c >> 2)));
      const bool better = c < n && (c == 0 || e < e_best);  // wave-uniform
      e_best = better ? e : e_best;
      r_best = better ? a.ratio[c] : r_best;
      k_best = better ? (uint32_t)c : k_best;
    }
    const float s_best = group_scale<T>(mse_threshold<T>(stat, r_best), use_min, a.min_val, a.thr_div);
    const run_t<T, NC> yc = with_group_div<T>(
        s_best, [&](const auto& div) { return clip_quant<T, NC>(xc0, div, s_best, qmin, qmax); });
    const int64_t group = row * gpr + j;
    if (q == 0) store_run<T, NC>(reinterpret_cast<T*>(a.y) + row * a.k + j * G + n16 * NC, yc);
    if (lane == 0) {
      reinterpret_cast<T*>(a.scale)[group] = from_f<T>(s_best);
      reinterpret_cast<T*>(a.stat)[group] = from_f<T>(stat);  // exact: stat is a value of T
      a.idx[group] = (uint8_t)k_best;
    }
    if (n16 == 0) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (4 * q + i < n) a.losses[group * n + 4 * q + i] = loss[i];
    }
  }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
// what the entries cover next to group_check: the group sizes of the kernel, the weight's geometry, the candidate count
static int clip_check(const bvq_quant_desc* d, int64_t k, int n_ratios, const char* what) {
  if (!d) {
    set_error("%s: null descriptor", what);
    return BVQ_ERR_INVALID;
  }
  int rc = group_check(d, what);
  if (rc) return rc;
  if (d->inner > 128) {
    set_error("%s: group size %lld (16, 32, 64 or 128: a block of the Hessian stays in LDS)", what, (long long)d->inner);
    return BVQ_ERR_UNSUPPORTED;
  }
  if (n_ratios < 1 || n_ratios > kClipMaxCandidates) {
    set_error("%s: %d candidate ratios (1 to %d)", what, n_ratios, kClipMaxCandidates);
    return BVQ_ERR_UNSUPPORTED;
  }
  if (k < d->inner || k % d->inner != 0 || d->channels % (k / d->inner) != 0) {
    set_error("%s: rows of %lld elements are no whole groups of %lld, or %lld groups no whole rows", what, (long long)k,
              (long long)d->inner, (long long)d->channels);
    return BVQ_ERR_UNSUPPORTED;
  }
  const int64_t rows = d->channels / (k / d->inner);
  if (k / d->inner > 0x7fffffff || (rows + kClipRows - 1) / kClipRows > 65535) {
    set_error("%s: %lld rows of %lld groups are beyond the launch grid", what, (long long)rows,
              (long long)(k / d->inner));
    return BVQ_ERR_UNSUPPORTED;
  }
  return BVQ_OK;
}

// the candidate table into the argument struct: ratios[0] is 1, every ratio finite and in (0, 1]
static int clip_fill(GroupClipArgs& a, const float* ratios, int n_ratios, const char* what) {
  for (int i = 0; i < n_ratios; ++i) {
    const float r = ratios[i];
    if (!(r > 0.f && r <= 1.f)) {  // a NaN fails both comparisons
      set_error("%s: ratio %d is %g (finite, in (0, 1])", what, i, (double)r);
      return BVQ_ERR_UNSUPPORTED;
    }
    a.ratio[i] = r;
  }
  if (ratios[0] != 1.f) {
    set_error("%s: ratio 0 is %g (the abs-max itself is always the first candidate: 1)", what, (double)ratios[0]);
    return BVQ_ERR_UNSUPPORTED;
  }
  a.n = n_ratios;
  return BVQ_OK;
}

}  // namespace bvq

using namespace bvq;

extern "C" int bvq_group_clip_supported(const bvq_quant_desc* d, const void* x, const void* hb, int64_t k,
                                        int n_ratios) {
  if (clip_check(d, k, n_ratios, "bvq_group_clip_supported")) return 0;
  return x && hb && aligned16(x) && aligned16(hb) ? 1 : 0;
}

extern "C" int bvq_group_clip_fwd(const bvq_quant_desc* d, const void* x, const void* hb, int64_t k,
                                  const float* ratios, int n_ratios, double min_val, int use_min, double thr_div,
                                  void* y, void* scale, void* stat, void* idx, void* losses, bvq_stream_t stream) {
  const char* what = "bvq_group_clip_fwd";
  int rc = clip_check(d, k, n_ratios, what);
  if (rc) return rc;
  rc = group_required(what, rc, {x, hb, ratios, y, scale, stat, idx, losses});
  if ((rc = group_aligned(what, rc, {x, hb, y}, "x, hb and y"))) return rc;
  const GroupArgs g = group_args(d, min_val, use_min, thr_div);  // the scalars as every group-wise entry forms them
  GroupClipArgs a = {};
  if ((rc = clip_fill(a, ratios, n_ratios, what))) return rc;
  a.x = x;
  a.hb = reinterpret_cast<const float*>(hb);
  a.y = y;
  a.scale = scale;
  a.stat = stat;
  a.idx = reinterpret_cast<uint8_t*>(idx);
  a.losses = reinterpret_cast<float*>(losses);
  a.k = k;
  a.rows = d->channels / (k / d->inner);
  a.use_min = g.use_min;
  a.qmin = g.qmin;
  a.qmax = g.qmax;
  a.min_val = g.min_val;
  a.thr_div = g.thr_div;
  const dim3 grid((unsigned)(k / d->inner), (unsigned)((a.rows + kClipRows - 1) / kClipRows));
  rc = with_dtype(d->x_dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    return with_value<16, 32, 64, 128>((int)d->inner, [&](auto gs) {
      group_clip_kernel<T, gs><<<grid, kBlock, 0, (hipStream_t)stream>>>(a);
    });
  });
  return rc ? rc : check_launch(what);
}
