// bvq_unit_walk.h -- the three walks of the read-mostly kernels (statistics, select, tie scan, abs-affine backward):
// how a wave gets from its unit, or a workgroup from its place in the grid, to the vectors and elements it owns.  A
// kernel on a walk is its state, a body per vector or element, and its write-out; nothing here knows a statistic.
//
//   row-mapped    (Tiling / Unit, bvq_common.h): walk_unit -- ChunkWalker over the full chunks of the unit's rows, kU
//                 predicated loads in flight before the first use, then walk_unit_tail over the ragged ends.
//   column-mapped (ColsPlan, bvq_common.h): cols_locate places a lane (ColsPlace), walk_cols takes it down its rows
//                 with kU loads in flight.
//   flat          (a pointer and a count): walk_flat -- the grid's workgroups stride over the 16-byte chunks of a
//                 buffer with kU predicated loads in flight; workgroup 0 takes the elements around the chunks.
#pragma once

#include "bvq_common.h"

namespace bvq {

// ---- row-mapped -----------------------------------------------------------------------------------------------------
// The ragged ends of a unit: the (< VEC) elements after the last full chunk of EVERY row.  Lane e takes element
// e % tail of row e / tail; f(offset from the unit's base, position from u.pos0) -- the two numbers walk_unit hands on.
//
// Which units have a tail is decided on the host (pick_vec, bvq_common.hip).  With ragged_ok, rows that are not whole
// chunks keep the full vector width and every row of a unit has a tail.  Without it, pick_vec gives the full width to
// such rows only when there is a SINGLE row (rows == 1: per-tensor layouts, a long row cut into pieces), so only
// single-row units have a tail; there lane k takes tail element k, one element per lane at most.
//
// Beside the every-row form stands a wave-uniform shortcut for nrows == 1.  It is the same assignment (e / tail = 0,
// e % tail = e), written without the division: with the division alone absmoments_kernel<16-bit, 8, NT> needs 66 VGPRs
// instead of 62 and runs 7 waves per SIMD instead of 8 (profiles/stat_walk.md).
template <int VEC, typename F>
__device__ __forceinline__ void walk_unit_tail(const Unit& u, int64_t row_len, int lane, F&& f) {
  if constexpr (VEC > 1) {
    const int64_t full = (u.len / VEC) * VEC;  // elements of a row in full chunks
    const int32_t tail = (int32_t)(u.len - full);
    if (u.nrows == 1) {  // (wave-uniform) lane k, element k
      if (lane < tail) f(full + lane, full + lane);
    } else {
      for (int32_t e = lane; e < u.nrows * tail; e += kWave) {
        const int32_t r = e / tail, k = e - r * tail;
        f((int64_t)r * u.row_stride + full + k, (int64_t)r * row_len + full + k);
      }
    }
  }
}

// One wave over its unit (xp: the unit's first element).  Full chunks: kU predicated loads (16 bytes per lane at full
// width, cache policy NT) are issued before the first is used, then chunk(xv, offset, position) per loaded vector;
// ragged ends: each(x, offset, position) per element.  offset counts from the unit's base, position from u.pos0 (the
// reference's reduction order, row_len apart from row to row); a body that ignores them leaves no instruction behind.
// (Two bodies even where both apply one function: a single per-element body, handed the elements of a vector one by
// one, costs the bf16 min/max kernels 5 VGPRs and one instantiation an occupancy step, profiles/stat_walk.md.)
// The walker is advanced between a load and its body -- that is what puts kU loads in flight -- so with kU = 1 a
// storing body holds the vector, its place and the advanced walker together: more registers than a load-use-advance
// loop (abs_affine_bwd_kernel, tie_scan_kernel: 8 waves per SIMD either way).
// ChunkWalker, not ChunkCursor: see bvq_common.h.
template <typename T, int VEC, bool NT, int kU, typename C, typename E>
__device__ __forceinline__ void walk_unit(const Unit& u, const T* __restrict__ xp, int64_t row_len, int lane,
                                          C&& chunk, E&& each) {
  ChunkWalker cur;
  cur.init(u, VEC, lane);
  const int64_t total = (int64_t)u.nrows * cur.cpr;
  for (int64_t done = 0; done < total; done += (int64_t)kWave * kU) {
    vec_t<T, VEC> xv[kU];
    ChunkWalker at[kU];  // where each vector lies: offset and position are worked out only for a body that asks
    bool ok[kU];
#pragma unroll
    for (int j = 0; j < kU; ++j) {
      ok[j] = cur.valid();
      at[j] = cur;
      if (ok[j]) xv[j] = load_vec<T, VEC, NT>(xp + cur.offset(u.row_stride, VEC));
      cur.next();
    }
#pragma unroll
    for (int j = 0; j < kU; ++j) {
      if (ok[j]) chunk(xv[j], at[j].offset(u.row_stride, VEC), at[j].pos(row_len, VEC));
    }
  }
  walk_unit_tail<VEC>(u, row_len, lane, [&](int64_t o, int64_t p) { each(xp[o], o, p); });
}

// ---- column-mapped --------------------------------------------------------------------------------------------------
// Where a lane stands in a ColsPlan: its unit is row block `rblk` x column strip `strip`; the lane owns column chunk
// `chunk` (VEC columns) and, of every pass of rpp rows, row `sub`.
struct ColsPlace {
  int64_t rblk;
  int32_t strip, sub, chunk;
  bool active;    // the lane has a chunk and a row (lanes past the plan's last chunk, or past rpp rows, idle)
  int64_t blk0;   // first row of the unit's row block (wave-uniform)
  int64_t row0;   // the lane's first row
  int64_t row_end;
};

// false: the wave has no unit.  team: the unit is the WORKGROUP's -- its waves take the block's rows in turn (wave w:
// rows w, w + 4, ... of each lane group), so that the workgroup walks one contiguous window of memory
__device__ __forceinline__ bool cols_locate(const ColsPlan& p, bool team, ColsPlace& c) {
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = threadIdx.x & 63;
  const int64_t unit = team ? (int64_t)blockIdx.x : (int64_t)blockIdx.x * kWavesPerBlock + wave;
  if (unit >= p.units) return false;
  c.rblk = unit / p.strips;
  c.strip = (int32_t)(unit - c.rblk * p.strips);
  c.sub = lane / p.lpr;                              // which of the rpp rows of a pass
  c.chunk = c.strip * kWave + (lane - c.sub * p.lpr);  // column chunk of this lane
  c.active = c.sub < p.rpp && c.chunk < p.cps;
  c.blk0 = c.rblk * p.rb;
  c.row0 = c.blk0 + (team ? (int64_t)wave * p.rpp : 0) + c.sub;
  c.row_end = (c.rblk + 1) * p.rb < p.rows ? (c.rblk + 1) * p.rb : p.rows;
  return true;
}

// An ACTIVE lane down its rows (x: the tensor's first element): kU loads in flight -- a row past the end reads row0
// again and is dropped -- then body(xv, row) per loaded vector.
template <typename T, int VEC, bool NT, int kU, typename F>
__device__ __forceinline__ void walk_cols(const ColsPlan& p, const ColsPlace& c, const T* __restrict__ x, F&& body) {
  const T* __restrict__ xp = x + (int64_t)c.chunk * VEC;
  for (int64_t r = c.row0; r < c.row_end; r += (int64_t)kU * p.rpp) {
    vec_t<T, VEC> xv[kU];
    bool ok[kU];
#pragma unroll
    for (int j = 0; j < kU; ++j) {
      const int64_t rr = r + (int64_t)j * p.rpp;
      ok[j] = rr < c.row_end;
      xv[j] = load_vec<T, VEC, NT>(xp + (ok[j] ? rr : c.row0) * p.L);
    }
#pragma unroll
    for (int j = 0; j < kU; ++j) {
      if (ok[j]) body(xv[j], r + (int64_t)j * p.rpp);
    }
  }
}

// ---- flat -----------------------------------------------------------------------------------------------------------
// The whole grid over [x - head, x + n), x on a 16-byte boundary, workgroups of kB threads: a workgroup-strided run
// over the full 16-byte chunks of [x, x + n) with kU predicated loads (cache policy NT) issued before the first is
// used, then workgroup 0 alone over the (< VEC) elements after the last chunk and the `head` (< VEC) elements in front
// of x -- what lies before the first 16-byte boundary of a caller's buffer.  each(v) per element; it sees every element
// exactly once, in no particular order (the kernels on this walk count).
// Chunks, tail and head are three separate branches: a body that votes across its wave (low_count, bvq_select.hip)
// must meet, in one ballot, only lanes that came through the same branch.
template <typename T, int kB, bool NT, int kU, typename E>
__device__ __forceinline__ void walk_flat(const T* __restrict__ x, int64_t n, int32_t head, E&& each) {
  constexpr int VEC = elem<T>::vec;
  const int64_t chunks = n / VEC;
  const int64_t stride = (int64_t)gridDim.x * kB;
  for (int64_t c = (int64_t)blockIdx.x * kB + threadIdx.x; c < chunks; c += stride * kU) {
    vec_t<T, VEC> xv[kU];
    bool ok[kU];
#pragma unroll
    for (int j = 0; j < kU; ++j) {
      const int64_t cj = c + (int64_t)j * stride;
      ok[j] = cj < chunks;
      if (ok[j]) xv[j] = load_vec<T, VEC, NT>(x + cj * VEC);
    }
#pragma unroll
    for (int j = 0; j < kU; ++j) {
      if (ok[j]) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) each(xv[j].v[k]);
      }
    }
  }
  if (blockIdx.x == 0 && chunks * VEC + threadIdx.x < n) each(x[chunks * VEC + threadIdx.x]);
  if (blockIdx.x == 0 && (int32_t)threadIdx.x < head) each(x[(int64_t)threadIdx.x - head]);
}

}  // namespace bvq
