// bvq_row_shifted.hip -- asymmetric per-row quantizer of the dynamic activation quantizers: unsigned codes, one scale
// and one integer zero-point per ROW of x[rows, H] (per token), taken from the row itself, one launch each way.
//
// The arithmetic is that of bvq_group_shifted.hip with "group" read as "row": the statistics -> scale -> zero-point
// chain and the steps of the backward are those of bvq_group_shifted.h, the forward chain of a chunk that of
// bvq_group_quant.h.  What differs is who holds a row.  A row of C = H * sizeof(T) / 16 chunks does not fit a fraction
// of one wave load; it fits the registers of one workgroup (the row walk, bvq_row_walk.h):
//
//   C <=  128   kW = 1, kD = 2   one wave per row, four rows per workgroup, no LDS, no barrier
//   C <=  512   kW = 4, kD = 2   one workgroup per row
//   C <= 2048   kW = 4, kD = 8   one workgroup per row (2048 chunks = bvq_row_shifted_max_row_bytes())
//
// Lane l of wave w of the row holds chunks j * 64 kW + 64 w + l, j = 0 .. kD - 1, from its only load to its only
// store.  All kD loads (backward: of x, then of g) are issued before the arithmetic, through buffer descriptors whose
// extent ends with the row: a lane past the row's end reads zeros without a memory access, its store is dropped, and it
// is kept out of the statistics, the sums and the positions by its chunk index.  Row bases are 64-bit.
//
// Exchanges.  Within a wave: butterflies (xor 32 .. 1), after which every lane holds the same bits.  Across the kW
// waves of a row: each wave writes its values to LDS, ONE barrier, every wave reads all kW and folds them in wave order.
// The forward exchanges the two ordered keys (one barrier), the backward the two float32 sums and the two first
// positions together (one barrier).  The row's chain -- the divisions from the statistics to scale and zero-point, and
// from the sums to the deposits -- is computed once per row on wave-uniform values, not per chunk.
//
// Sum order (backward, both sums alike; fixed by H, the dtype and the table above, hence the same bits on every run):
// a lane adds the terms of its chunks in ascending j, inside a chunk in ascending element pairs, the two terms of every
// element to the two halves of a pair accumulator as bwd_elem2 does; the halves are added; the 64 lanes by the xor
// butterfly 32, 16, 8, 4, 2, 1; the kW waves as ((w0 + w1) + w2) + w3.
//
// The statistics' gradients land on the first element equal to each BY POSITION in the row (the lowest flat index,
// whichever lane or wave holds it), in registers, before dx is stored.
//   forward   reads x, writes y              (+ 4 values per row)
//   backward  reads g and x, writes dx once  (+ 2 values per row, + gscale / gzp when given)
// No workspace, no atomics, no arrival words, no second kernel, nothing between workgroups.
#include "bvq_group_shifted.h"
#include "bvq_row_walk.h"

namespace bvq {

struct RowShiftedArgs : GroupShiftedArgs {
  int64_t rows;
  uint32_t cpr;  // 16-byte chunks per row
};

template <typename T, int kW, int kD, bool NT>
__global__ __launch_bounds__(kBlock) void row_shifted_fwd_kernel(RowShiftedArgs a) {
  constexpr int VEC = elem<T>::vec;
  __shared__ uint32_t ex[kW][4];
  RowSlot<kW> slot;
  if (!slot.init(a)) return;
  const buf_t bx = slot.template elems<T>(a.x, a), by = slot.template elems<T>(a.y, a);
  vec_t<T, VEC> xv[kD];
#pragma unroll
  for (int j = 0; j < kD; ++j) xv[j] = buf_load<T, VEC, NT>(bx, slot.chunk(j) * 16u);
  uint32_t kmax = 0u, kmin = ~0u;
#pragma unroll
  for (int j = 0; j < kD; ++j) {
    if (slot.first(j) >= a.cpr) break;  // wave-uniform
    uint32_t hi, lo;
    chunk_minmax_keys<T>(xv[j], hi, lo);
    const bool in = slot.chunk(j) < a.cpr;
    hi = in ? hi : 0u;
    lo = in ? lo : ~0u;
    kmax = hi > kmax ? hi : kmax;
    kmin = lo < kmin ? lo : kmin;
  }
  kmax = seg_max_u32<kWave>(kmax);
  kmin = seg_min_u32<kWave>(kmin);
  if constexpr (kW > 1) {
    const uint32_t mine[2] = {kmax, kmin};
    uint32_t all[kW][2];
    row_exchange<kW, 2>(ex, slot.wave, mine, all);
#pragma unroll
    for (int w = 0; w < kW; ++w) {
      kmax = all[w][0] > kmax ? all[w][0] : kmax;
      kmin = all[w][1] < kmin ? all[w][1] : kmin;
    }
  }
  // the row's chain, once, on wave-uniform values
  const float qmin = rnd<T>(a.qmin), qmax = rnd<T>(a.qmax);
  float mx, mn;
  shifted_stats<T>(uniform_u32(kmax), uniform_u32(kmin), mx, mn);
  const ShiftedGroup sg = shifted_group<T>(mx, mn, a, qmin, qmax);
  if (slot.wave == 0 && (threadIdx.x & 63) == 0) {
    T* const stat = reinterpret_cast<T*>(a.stat);
    reinterpret_cast<T*>(a.scale)[slot.row] = from_f<T>(sg.s);
    reinterpret_cast<T*>(a.zp)[slot.row] = from_f<T>(sg.zp);  // exact: an integer of the code range
    stat[slot.row] = from_f<T>(mx);                           // exact: values of T
    stat[a.rows + slot.row] = from_f<T>(mn);
  }
  with_group_div<T>(sg.s, [&](const auto& div) {
#pragma unroll
    for (int j = 0; j < kD; ++j) {
      if (slot.first(j) >= a.cpr) break;
      buf_store<T, VEC, NT>(by, slot.chunk(j) * 16u, group_fwd_chunk<T, true>(xv[j], div, sg.s, qmin, qmax, sg.zp));
    }
    return 0;
  });
}

template <typename T, int kW, int kD, bool NT>
__global__ __launch_bounds__(kBlock) void row_shifted_bwd_kernel(RowShiftedArgs a) {
  constexpr int VEC = elem<T>::vec;
  __shared__ uint32_t ex[kW][4];
  RowSlot<kW> slot;
  if (!slot.init(a)) return;
  const buf_t bx = slot.template elems<T>(a.x, a), bg = slot.template elems<T>(a.g, a),
              bd = slot.template elems<T>(a.y, a);
  vec_t<T, VEC> xv[kD], gv[kD];
#pragma unroll
  for (int j = 0; j < kD; ++j) xv[j] = buf_load<T, VEC, NT>(bx, slot.chunk(j) * 16u);
#pragma unroll
  for (int j = 0; j < kD; ++j) gv[j] = buf_load<T, VEC, NT>(bg, slot.chunk(j) * 16u);
  const T* const stat = reinterpret_cast<const T*>(a.stat);
  const float mx = to_f<T>(stat[slot.row]), mn = to_f<T>(stat[a.rows + slot.row]);
  const float gsc = a.gscale ? to_f<T>(reinterpret_cast<const T*>(a.gscale)[slot.row]) : 0.f;
  const float gzp = a.gzp ? to_f<T>(reinterpret_cast<const T*>(a.gzp)[slot.row]) : 0.f;
  // the forward's scale and zero-point from the saved statistics: the same arithmetic, the saved bits
  const float qmin = rnd<T>(a.qmin), qmax = rnd<T>(a.qmax);
  const ShiftedGroup sg = shifted_group<T>(mx, mn, a, qmin, qmax);
  const bool clamp_ste = a.clamp_ste != 0;
  f2 ds2 = splat2(0.f), dz2 = splat2(0.f);
  uint32_t fmx = ~0u, fmn = ~0u;
  vec_t<T, VEC> dv[kD];
  with_group_div<T>(sg.s, [&](const auto& div) {
#pragma unroll
    for (int j = 0; j < kD; ++j) {
      if (slot.first(j) >= a.cpr) break;  // wave-uniform
      if (slot.chunk(j) < a.cpr) {        // a lane past the row's end adds no term and owns no position
        dv[j] = shifted_bwd_elems<T>(clamp_ste, xv[j], gv[j], div, sg, qmin, qmax, ds2, dz2);
        shifted_first<T>(xv[j], slot.chunk(j) * VEC, mx, mn, fmx, fmn);
      }
    }
    return 0;
  });
  float ds = seg_sum<kWave>(ds2.x + ds2.y);
  float dzs = seg_sum<kWave>(dz2.x + dz2.y);
  fmx = seg_min_u32<kWave>(fmx);
  fmn = seg_min_u32<kWave>(fmn);
  if constexpr (kW > 1) {
    const uint32_t mine[4] = {__builtin_bit_cast(uint32_t, ds), __builtin_bit_cast(uint32_t, dzs), fmx, fmn};
    uint32_t all[kW][4];
    row_exchange<kW, 4>(ex, slot.wave, mine, all);
    ds = __builtin_bit_cast(float, all[0][0]);
    dzs = __builtin_bit_cast(float, all[0][1]);
    fmx = all[0][2];
    fmn = all[0][3];
#pragma unroll
    for (int w = 1; w < kW; ++w) {
      ds += __builtin_bit_cast(float, all[w][0]);
      dzs += __builtin_bit_cast(float, all[w][1]);
      fmx = all[w][2] < fmx ? all[w][2] : fmx;
      fmn = all[w][3] < fmn ? all[w][3] : fmn;
    }
  }
  fmx = uniform_u32(fmx);
  fmn = uniform_u32(fmn);
  const ShiftedDeposit dep =
      shifted_bwd_chain<T>(a, sg, mn, uniform_f(ds), uniform_f(dzs), gsc, gzp, qmin, qmax);
#pragma unroll
  for (int j = 0; j < kD; ++j) {
    if (slot.first(j) >= a.cpr) break;
    const uint32_t e0 = slot.chunk(j) * VEC;
    if (fmx - e0 < (uint32_t)VEC || fmn - e0 < (uint32_t)VEC) shifted_deposit<T>(dv[j], e0, fmx, fmn, dep);
    buf_store<T, VEC, NT>(bd, slot.chunk(j) * 16u, dv[j]);
  }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
// what the kernels cover, apart from the pointers: BVQ_OK, or the error with its text
static int row_check(const bvq_quant_desc* d, const char* what) {
  const int rc = group_check(d, what, true, true);
  if (rc) return rc;
  const int64_t bytes = d->inner * dtype_size(d->x_dtype);
  if (d->inner < 1 || bytes % 16 != 0 || bytes > kRowMaxBytes) {
    set_error("%s: a row of %lld bytes (a multiple of 16, at most %lld)", what, (long long)bytes,
              (long long)kRowMaxBytes);
    return BVQ_ERR_UNSUPPORTED;
  }
  return BVQ_OK;
}

static RowShiftedArgs row_args(const bvq_quant_desc* d, double min_val, int use_min, double thr_div) {
  RowShiftedArgs a = group_args<RowShiftedArgs>(d, min_val, use_min, thr_div);
  a.rows = d->channels;
  a.cpr = (uint32_t)(d->inner * dtype_size(d->x_dtype) / 16);
  return a;
}

}  // namespace bvq

using namespace bvq;

extern "C" int64_t bvq_row_shifted_max_row_bytes(void) { return kRowMaxBytes; }

extern "C" int bvq_row_shifted_supported(const bvq_quant_desc* d, const void* x) {
  if (row_check(d, "bvq_row_shifted_supported")) return 0;
  return x && aligned16(x) ? 1 : 0;
}

extern "C" int bvq_row_shifted_fwd(const bvq_quant_desc* d, const void* x, double min_val, int use_min, double thr_div,
                                   void* y, void* scale, void* zp, void* stat, bvq_stream_t stream) {
  const char* what = "bvq_row_shifted_fwd";
  int rc = group_required(what, row_check(d, what), {x, y, scale, zp, stat});
  if ((rc = group_aligned(what, rc, {x, y, scale, zp, stat}, "x, y, scale, zp and stat"))) return rc;
  RowShiftedArgs a = row_args(d, min_val, use_min, thr_div);
  a.x = x;
  a.y = y;
  a.scale = scale;
  a.zp = zp;
  a.stat = stat;
  // x read + y written
  return row_launch(what, d->x_dtype, a, 32, [&](auto t, auto w, auto depth, auto nt, unsigned grid) {
    row_shifted_fwd_kernel<typename decltype(t)::type, w, depth, nt><<<grid, kBlock, 0, (hipStream_t)stream>>>(a);
  });
}

extern "C" int bvq_row_shifted_bwd(const bvq_quant_desc* d, const void* g, const void* x, const void* stat,
                                   const void* gscale, const void* gzp, double min_val, int use_min, double thr_div,
                                   void* dx, bvq_stream_t stream) {
  const char* what = "bvq_row_shifted_bwd";
  int rc = group_required(what, row_check(d, what), {g, x, stat, dx});
  if ((rc = group_aligned(what, rc, {g, x, stat, gscale, gzp, dx}, "g, x, stat, gscale, gzp and dx"))) return rc;
  RowShiftedArgs a = row_args(d, min_val, use_min, thr_div);
  a.x = x;
  a.g = g;
  a.y = dx;
  a.stat = const_cast<void*>(stat);
  a.gscale = gscale;
  a.gzp = gzp;
  // g and x read, dx written
  return row_launch(what, d->x_dtype, a, 48, [&](auto t, auto w, auto depth, auto nt, unsigned grid) {
    row_shifted_bwd_kernel<typename decltype(t)::type, w, depth, nt><<<grid, kBlock, 0, (hipStream_t)stream>>>(a);
  });
}
