// bvq_group_awq.hip -- the candidates of an AWQ search (activation-aware weight quantization, Lin et al. 2023) over one
// group-wise quantized weight, all of them in one launch on the sub-wave group walk of bvq_group_walk.h.
//
// A candidate scales the input columns of the weight w [R, K] by a factor s [K], quantizes the scaled weight with the
// group-wise quantizer (bvq_group_quant.hip, or the asymmetric bvq_group_shifted.hip) and divides the factor out again,
// every torch op rounding to w's dtype T:
//   xs = T(w * s[col])                                       col = flat index mod K
//   scale (, zp) = the quantizer's statistics -> scale (-> zero-point) chain on each group of xs
//   yq = the quantizer's forward chain of xs at (scale, zp)
//   y  = T(yq / s[col])                                      the IEEE float32 quotient, then rounded to T
// The walk is that of the two quantizers: a group of g elements lives in L adjacent lanes of one wave load, so a wave
// keeps its window of w in registers and computes candidate after candidate from them.  w is read once, one y is
// written per candidate; per candidate and load a lane reads the 16 bytes of its eight (four) consecutive column
// factors, which never cross a row: K is whole groups and a group whole chunks.  No LDS, no atomics, no workspace.
//   reads x and n * K factors (from cache), writes n * (y + (1 or 2) * bytes(x) / g for scale, zp)
// The candidate loop runs n times for the whole wave (n is a kernel argument).  The factors of candidate i + 1 are
// asked for before candidate i is worked on, so that no wave waits for them behind its own stores.
// With n = 1 and factors of one the outputs have the bits of bvq_group_quant_fwd / bvq_group_shifted_fwd.
#include "bvq_group_shifted.h"

namespace bvq {

constexpr int kAwqMaxCandidates = 64;

// x: the weight; y, scale, zp: candidate i at i * (elements of x) and i * groups
struct GroupAwqArgs : GroupShiftedArgs {
  const void* table;     // [n, K] column factors in x's dtype
  int64_t k;             // elements per row of x
  uint32_t row_chunks;   // 16-byte chunks per row
  int32_t n;             // candidates, 1..kAwqMaxCandidates
};

// The byte offsets of a lane's column factors in a row of the table, one per wave load: chunk c of the tensor holds the
// columns of chunk c mod row_chunks of a row.  The window's first chunk is reduced once per wave (in 32 bits unless the
// tensor has 2^31 chunks or more), the lane's once, and a wave load further on is 64 chunks further round the row.
template <int kD>
__device__ __forceinline__ void awq_columns(int64_t c0, uint32_t row_chunks, uint32_t (&off)[kD]) {
  const uint32_t first = c0 < ((int64_t)1 << 31) ? (uint32_t)c0 % row_chunks : (uint32_t)(c0 % (int64_t)row_chunks);
  const uint32_t step = (uint32_t)kWave % row_chunks;
  uint32_t col = (first + (threadIdx.x & 63)) % row_chunks;  // first + 63 < 2^32: row_chunks < 2^27
#pragma unroll
  for (int j = 0; j < kD; ++j) {
    off[j] = col * 16u;
    col += step;  // < 2 * row_chunks
    col -= col >= row_chunks ? row_chunks : 0u;
  }
}

// one wave load of one candidate: the lane's 16 bytes of y; scale and zero-point by the segment's head lane
template <typename T, int L, bool kShifted>
__device__ __forceinline__ vec_t<T, elem<T>::vec> awq_chunk(const GroupAwqArgs& a, const vec_t<T, elem<T>::vec>& xv,
                                                            const vec_t<T, elem<T>::vec>& sv, const GroupPlace& p,
                                                            buf_t bs, buf_t bz, float qmin, float qmax) {
  constexpr int VEC = elem<T>::vec;
  vec_t<T, VEC> xs, yq, yv;
#pragma unroll
  for (int k = 0; k < VEC; k += 2)
    pack2<T>(widen2<T>(xv.v[k], xv.v[k + 1]) * widen2<T>(sv.v[k], sv.v[k + 1]), xs.v[k], xs.v[k + 1]);
  if constexpr (kShifted) {
    uint32_t kmax, kmin;
    chunk_minmax_keys<T>(xs, kmax, kmin);
    float mx, mn;
    shifted_stats<T>(seg_max_u32<L>(kmax), seg_min_u32<L>(kmin), mx, mn);
    const ShiftedGroup sg = shifted_group<T>(mx, mn, a, qmin, qmax);
    store_group(bs, p, from_f<T>(sg.s));
    store_group(bz, p, from_f<T>(sg.zp));  // exact: an integer of the code range
    yq = with_group_div<T>(sg.s, [&](const auto& div) {
      return group_fwd_chunk<T, true>(xs, div, sg.s, qmin, qmax, sg.zp);
    });
  } else {
    const float stat = key_value<T>(seg_max_u32<L>(chunk_key<T>(xs)));
    const float s = group_scale<T>(stat, a.use_min != 0, a.min_val, a.thr_div);
    store_group(bs, p, from_f<T>(s));
    yq = with_group_div<T>(s, [&](const auto& div) { return group_fwd_chunk<T>(xs, div, s, qmin, qmax); });
  }
#pragma unroll
  for (int k = 0; k < VEC; k += 2) {
    const f2 q = widen2<T>(yq.v[k], yq.v[k + 1]), s = widen2<T>(sv.v[k], sv.v[k + 1]);
    pack2<T>(f2{q.x / s.x, q.y / s.y}, yv.v[k], yv.v[k + 1]);
  }
  return yv;
}

// The frame of bvq_group_walk.h (group_fwd_kernel) with a candidate loop between the loads and the stores: the same
// window, the same descriptors ending with the tensor (no tail branch, stores past the end dropped), every candidate's
// outputs behind a 64-bit base of their own.
template <typename T, int L, bool kShifted, bool NT>
__global__ __launch_bounds__(kBlock) void group_awq_kernel(GroupAwqArgs a) {
  constexpr int VEC = elem<T>::vec, kD = kGroupFwdDepth;
  using Vec = vec_t<T, VEC>;
  GroupWindow<T, L, kD> w;
  if (!w.init(a)) return;
  const buf_t bx = w.elems(a.x);
  Vec xv[kD], sv[kD], sn[kD];
#pragma unroll
  for (int j = 0; j < kD; ++j) xv[j] = buf_load<T, VEC, NT>(bx, group_place<L>(j).off);
  uint32_t col[kD];
  awq_columns<kD>(w.c0, a.row_chunks, col);
  const T* table = reinterpret_cast<const T*>(a.table);
  const uint32_t row_bytes = a.row_chunks * 16u;
  const int64_t elems = a.chunks * VEC, groups = a.chunks / L;
  const float qmin = rnd<T>(a.qmin), qmax = rnd<T>(a.qmax);
  // the factors stay in cache for every wave: default policy, whatever NT
  const buf_t bt0 = make_buf(table, row_bytes);
#pragma unroll
  for (int j = 0; j < kD; ++j) sv[j] = buf_load<T, VEC>(bt0, col[j]);
  for (int i = 0; i < a.n; ++i) {  // wave-uniform
    const int next = i + 1 < a.n ? i + 1 : i;  // the last candidate asks for its own row again
    const buf_t bt = make_buf(table + next * a.k, row_bytes);
#pragma unroll
    for (int j = 0; j < kD; ++j) sn[j] = buf_load<T, VEC>(bt, col[j]);
    const buf_t by = w.elems(reinterpret_cast<const T*>(a.y) + i * elems);
    const buf_t bs = w.groups(reinterpret_cast<const T*>(a.scale) + i * groups);
    const buf_t bz = kShifted ? w.groups(reinterpret_cast<const T*>(a.zp) + i * groups) : bs;
#pragma unroll
    for (int j = 0; j < kD; ++j) {
      if ((uint32_t)(j * kWave) >= w.nch) break;  // wave-uniform
      const GroupPlace p = group_place<L>(j);
      buf_store<T, VEC, NT>(by, p.off, awq_chunk<T, L, kShifted>(a, xv[j], sv[j], p, bs, bz, qmin, qmax));
    }
#pragma unroll
    for (int j = 0; j < kD; ++j) sv[j] = sn[j];
  }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
// what the entries cover next to group_check: the table's geometry and the candidate count
static int awq_check(const bvq_quant_desc* d, int64_t k, int n, const char* what) {
  if (!d) {
    set_error("%s: null descriptor", what);
    return BVQ_ERR_INVALID;
  }
  int rc = group_check(d, what, d->zp_per_channel != 0);
  if (rc) return rc;
  if (n < 1 || n > kAwqMaxCandidates) {
    set_error("%s: %d candidates (1 to %d)", what, n, kAwqMaxCandidates);
    return BVQ_ERR_UNSUPPORTED;
  }
  if (k < d->inner || k % d->inner != 0 || d->channels % (k / d->inner) != 0) {
    set_error("%s: rows of %lld elements are no whole groups of %lld, or %lld groups no whole rows", what, (long long)k,
              (long long)d->inner, (long long)d->channels);
    return BVQ_ERR_UNSUPPORTED;
  }
  if (k * dtype_size(d->x_dtype) > kMaxUnitBytes) {
    set_error("%s: a row of %lld elements is beyond a buffer descriptor's 2^31 bytes", what, (long long)k);
    return BVQ_ERR_UNSUPPORTED;
  }
  return BVQ_OK;
}

}  // namespace bvq

using namespace bvq;

extern "C" int bvq_group_awq_supported(const bvq_quant_desc* d, const void* x, const void* table, const void* y,
                                       int64_t k, int n) {
  if (awq_check(d, k, n, "bvq_group_awq_supported")) return 0;
  return x && table && aligned16(x) && aligned16(table) && aligned16(y) ? 1 : 0;
}

extern "C" int bvq_group_awq_fwd(const bvq_quant_desc* d, const void* x, const void* table, int64_t k, int n,
                                 double min_val, int use_min, double thr_div, void* y, void* scale, void* zp,
                                 bvq_stream_t stream) {
  const char* what = "bvq_group_awq_fwd";
  int rc = awq_check(d, k, n, what);
  if (rc) return rc;
  const bool shifted = d->zp_per_channel != 0;
  rc = group_required(what, rc, {x, table, y, scale, shifted ? zp : x});  // zp: where the descriptor has one per group
  if ((rc = group_aligned(what, rc, {x, table, y}, "x, table and y"))) return rc;
  GroupAwqArgs a = group_args<GroupAwqArgs>(d, min_val, use_min, thr_div);
  a.x = x;
  a.y = y;
  a.scale = scale;
  a.zp = zp;
  a.table = table;
  a.k = k;
  a.row_chunks = (uint32_t)(k * dtype_size(d->x_dtype) / 16);
  a.n = n;
  // x read + n candidates written
  return group_launch(what, d->x_dtype, d->inner, a.chunks, 16 * (1 + n), kGroupFwdDepth,
                      [&](auto t, auto l, auto nt, unsigned grid) {
    using T = typename decltype(t)::type;
    if (shifted)
      group_awq_kernel<T, l, true, nt><<<grid, kBlock, 0, (hipStream_t)stream>>>(a);
    else
      group_awq_kernel<T, l, false, nt><<<grid, kBlock, 0, (hipStream_t)stream>>>(a);
  });
}
