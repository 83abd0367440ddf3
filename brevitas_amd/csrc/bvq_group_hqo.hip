// bvq_group_hqo.hip -- asymmetric group-wise weight quantizer whose zero-point is searched per group by half-quadratic
// optimisation (HQQ; HalfQuadraticOptimizerZeroPoint of later Brevitas releases): from the integer zero-point of
// bvq_group_shifted.hip on, up to n proximal steps move a real-valued zero-point towards a lower robust (l_p, p <= 1)
// error, and the group keeps the first candidate with the smallest summed |error| reached before the error stops
// falling.  One launch each way.
//
// The walk is that of bvq_group_shifted.hip (bvq_group_walk.h): a group of g elements lives in L adjacent lanes of one
// wave load, so the whole search runs on the registers that hold the chunk.  x is read once; per candidate every lane
// quantizes its 16 bytes at the candidate zero-point with the forward chain of the plain quantizer (rounded to T as
// the stored y would be), the group's error and the next zero-point are segmented butterflies, the best
// (error, zero-point, index) so far and the group's `live` flag stay in registers; y is written once, at the kept
// zero-point.  No LDS, no workspace, no atomics, no second launch.
//   forward   reads x, writes y                (+ 4 * bytes(x) / g for scale, zp and the two statistics, + one index byte)
//   backward  reads g and x, writes dx once    (+ 3 * bytes(x) / g for the statistics and zp; gscale when given)
// The candidate loop runs at most n + 1 times for the whole wave (n is a kernel argument, ib[i] a scalar read of the
// argument struct) and ends early once no group of the wave is live, which changes no bit.  The shrinkage of p = 1 and
// of p = 0.5 are two instantiations of the kernel, never a per-lane branch.
// With n = 0 the forward computes the bits of bvq_group_shifted_fwd.
#include "bvq_group_shifted.h"

namespace bvq {

constexpr int kHqoMaxIters = 63;
constexpr int kHqoLp1 = 0, kHqoLpHalf = 1;  // the `lp` codes of include/bvq.h: p = 1, p = 0.5

struct GroupHqoArgs : GroupShiftedArgs {
  void* idx;  // [groups] uint8: fwd out
  int32_t n;  // proximal steps, 0..kHqoMaxIters: candidates 0..n
  float ib[kHqoMaxIters + 1];  // ib[i] = 1 / (beta * kappa^i)
};

// the shrinkage of one residual: sign(r) * max(|r| - thr, 0), thr = ib (p = 1) or ib / sqrt(|r|) (p = 0.5), in the
// spelling of the torch ops (sign(0) = +0, so a residual of zero shrinks to +0 and a negative one to -0 at most)
template <int kLp>
__device__ __forceinline__ float hqo_shrink(float r, float ib) {
  const float ar = __builtin_fabsf(r);
  float thr = ib;
  if constexpr (kLp == kHqoLpHalf) thr = ib / __builtin_sqrtf(ar);  // |r| = 0: inf
  float m = ar - thr;
  m = m < 0.f ? 0.f : m;  // clamp_min: a NaN passes
  const float sg = (float)(0.f < r) - (float)(r < 0.f);
  return sg * m;
}

// One candidate on this lane's chunk: the forward chain at the zero-point zp (a value of T), the lane's part of the
// error sum |x - y| and of the next zero-point's sum q - (x - w_e) * inv_s.  Within the chunk the even-indexed
// elements are added in order into .x and the odd-indexed into .y, the first pair starting the accumulators.
// kUpdate: false for the last candidate, which no zero-point follows: its shrinkage is not computed (one wave-uniform
// branch per candidate in the caller, two straight-line bodies).
template <typename T, int kLp, bool kUpdate, typename Div>
__device__ __forceinline__ void hqo_candidate_chunk(const vec_t<T, elem<T>::vec>& xv, const Div& div, float s,
                                                    float inv_s, float zp, float qmin, float qmax, float ib, float& e,
                                                    float& z) {
  constexpr int VEC = elem<T>::vec;
  f2 eacc = splat2(0.f), zacc = splat2(0.f);
#pragma unroll
  for (int k = 0; k < VEC; k += 2) {
    const f2 xf = widen2<T>(xv.v[k], xv.v[k + 1]);
    f2 t = rnd2<T>(div(xf));
    t = rnd2<T>(t + zp);
    t = round_op2<T, BVQ_ROUND>(t);
    const f2 q = clamp_where2(t, qmin, qmax);
    const f2 y = rnd2<T>(rnd2<T>(q - zp) * s);
    const f2 r = xf - y;
    const f2 ar = {__builtin_fabsf(r.x), __builtin_fabsf(r.y)};
    eacc = k == 0 ? ar : eacc + ar;  // (not 0 + |r|, 0 + term: a sum of -0 terms stays -0, as in the torch spelling)
    if constexpr (kUpdate) {
      const f2 we = {hqo_shrink<kLp>(r.x, ib), hqo_shrink<kLp>(r.y, ib)};
      const f2 term = q - (xf - we) * inv_s;
      zacc = k == 0 ? term : zacc + term;
    }
  }
  e = eacc.x + eacc.y;
  z = zacc.x + zacc.y;
}

// the search of one wave load: -> the kept zero-point (a value of T) and its index.  Every lane of a segment ends
// with the same bits.  searched: the group is live after candidate 0.
template <typename T, int L, int kLp, typename Div>
__device__ __forceinline__ void hqo_search(const GroupHqoArgs& a, const vec_t<T, elem<T>::vec>& xv, const Div& div,
                                           float s, float zp0, bool searched, float qmin, float qmax,
                                           float& zp_best, uint32_t& k_best) {
  constexpr float inv_g = 1.0f / (float)(L * elem<T>::vec);  // exact: g is a power of two
  const int n = a.n;
  const float inv_s = 1.0f / s;
  float z = zp0, e_best = 0.f;
  bool live = true;  // (set at candidate 0)
  zp_best = zp0;
  k_best = 0;
  for (int i = 0; i <= n; ++i) {  // wave-uniform count; a.ib[i] is a scalar read
    const float zp = rnd<T>(z);
    float e, zn;
    if (i < n)
      hqo_candidate_chunk<T, kLp, true>(xv, div, s, inv_s, zp, qmin, qmax, a.ib[i], e, zn);
    else
      hqo_candidate_chunk<T, kLp, false>(xv, div, s, inv_s, zp, qmin, qmax, 0.f, e, zn);
    e = seg_sum<L>(e);
    // strict: ties keep the earlier candidate; a NaN error is below nothing.  A group whose error did not fall is
    // finished for good.
    const bool better = i == 0 || (live && e < e_best);
    e_best = better ? e : e_best;
    zp_best = better ? zp : zp_best;
    k_best = better ? (uint32_t)i : k_best;
    live = i == 0 ? searched : better;
    if (__builtin_amdgcn_ballot_w64(live) == 0) break;  // wave-uniform: nothing of this load can change any more
    z = seg_sum<L>(zn) * inv_g;  // (read by live groups alone)
  }
}

// the HQO quantizer on the frame of bvq_group_walk.h
template <typename T, int L, int kLp>
struct HqoQuantLp {
  using Args = GroupHqoArgs;
  using Vec = vec_t<T, elem<T>::vec>;
  struct Side {
    T mx, mn, zp, gscale;
  };
  const Args& a;
  const buf_t bs, bz, btx, btn, bgs, bi;
  const float qmin, qmax;
  template <typename W>
  __device__ __forceinline__ HqoQuantLp(const Args& a, const W& w)
      : a(a), bs(w.groups(a.scale)), bz(w.groups(a.zp)), btx(w.groups(a.stat)),
        btn(w.groups(reinterpret_cast<const T*>(a.stat) + a.chunks / L)), bgs(w.groups_or_zeros(a.gscale, a.x)),
        bi(w.template groups<uint8_t>(a.idx)), qmin(rnd<T>(a.qmin)), qmax(rnd<T>(a.qmax)) {}

  __device__ __forceinline__ Vec fwd(const Vec& xv, const GroupPlace& p) const {
    uint32_t kmax, kmin;
    chunk_minmax_keys<T>(xv, kmax, kmin);
    float mx, mn;
    shifted_stats<T>(seg_max_u32<L>(kmax), seg_min_u32<L>(kmin), mx, mn);
    const ShiftedGroup sg = shifted_group<T>(mx, mn, a, qmin, qmax);
    store_group(bs, p, from_f<T>(sg.s));
    store_group(btx, p, from_f<T>(mx));  // exact: values of T
    store_group(btn, p, from_f<T>(mn));
    return with_group_div<T>(sg.s, [&](const auto& div) {
      float zp;
      uint32_t k;
      // a constant group (the scale is its lower bound, the grid has collapsed) is not searched; a NaN one is, in vain
      hqo_search<T, L, kLp>(a, xv, div, sg.s, sg.zp, !(mx == mn), qmin, qmax, zp, k);
      store_group(bz, p, from_f<T>(zp));  // exact: a value of T
      buf_store_u8(bi, p.head_at(1), k);
      return group_fwd_chunk<T, true>(xv, div, sg.s, qmin, qmax, zp);
    });
  }

  __device__ __forceinline__ Side side(const GroupPlace& p) const {
    return {load_group<T>(btx, p), load_group<T>(btn, p), load_group<T>(bz, p), load_group<T>(bgs, p)};
  }
  // ShiftedQuant::bwd at the kept zero-point, which is a constant: its own gradient path does not exist, the scale's
  // gradient is the quantizer's alone (+ gscale) and goes to the two statistics
  __device__ __forceinline__ Vec bwd(const Vec& xv, const Vec& gv, const Side& sd, const GroupPlace& p) const {
    constexpr int VEC = elem<T>::vec;
    const float mx = to_f<T>(sd.mx), mn = to_f<T>(sd.mn), gsc = to_f<T>(sd.gscale);
    // the forward's scale from the saved statistics: the same arithmetic, the saved bits
    ShiftedGroup sg = shifted_group<T>(mx, mn, a, qmin, qmax);
    sg.zp = to_f<T>(sd.zp);
    return with_group_div<T>(sg.s, [&](const auto& div) {
      f2 ds2 = splat2(0.f), dz2 = splat2(0.f);
      Vec dv = shifted_bwd_elems<T>(a.clamp_ste != 0, xv, gv, div, sg, qmin, qmax, ds2, dz2);
      float v = rnd<T>(seg_sum<L>(ds2.x + ds2.y));
      if (a.gscale) v = rnd<T>(v + gsc);
      const float dthr = rnd<T>(v / a.thr_div);
      const ShiftedDeposit dep = {rnd<T>(dthr * sgn_f(sg.d)), 0.f};  // abs: zero at 0
      const uint32_t e0 = p.sub * VEC;
      uint32_t fmx = ~0u, fmn = ~0u;
      shifted_first<T>(xv, e0, mx, mn, fmx, fmn);
      shifted_deposit<T>(dv, e0, seg_min_u32<L>(fmx), seg_min_u32<L>(fmn), dep);
      return dv;
    });
  }
};
template <typename T, int L>
using HqoQuant = HqoQuantLp<T, L, kHqoLp1>;
template <typename T, int L>
using HqoQuantHalf = HqoQuantLp<T, L, kHqoLpHalf>;

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
static int hqo_check(int n_iters, int lp, const char* what) {
  if (n_iters < 0 || n_iters > kHqoMaxIters) {
    set_error("%s: %d iterations (0 to %d)", what, n_iters, kHqoMaxIters);
    return BVQ_ERR_UNSUPPORTED;
  }
  if (lp != kHqoLp1 && lp != kHqoLpHalf) {
    set_error("%s: lp code %d (0: p = 1, 1: p = 0.5)", what, lp);
    return BVQ_ERR_UNSUPPORTED;
  }
  return BVQ_OK;
}

// the table 1 / (beta * kappa^i), i = 0..n_iters, into the argument struct: every entry finite and positive
static int hqo_fill(GroupHqoArgs& h, const float* inv_beta, int n_iters, const char* what) {
  for (int i = 0; i <= n_iters; ++i) {
    const float v = inv_beta[i];
    if (!(v > 0.f && v <= 3.4028234663852886e38f)) {  // a NaN fails both comparisons
      set_error("%s: inv_beta %d is %g (finite and positive)", what, i, (double)v);
      return BVQ_ERR_UNSUPPORTED;
    }
    h.ib[i] = v;
  }
  h.n = n_iters;
  return BVQ_OK;
}

}  // namespace bvq

using namespace bvq;

extern "C" int bvq_group_hqo_supported(const bvq_quant_desc* d, const void* x, int n_iters, int lp) {
  if (group_check(d, "bvq_group_hqo_supported", true)) return 0;
  if (hqo_check(n_iters, lp, "bvq_group_hqo_supported")) return 0;
  return x && aligned16(x) ? 1 : 0;
}

extern "C" int bvq_group_hqo_fwd(const bvq_quant_desc* d, const void* x, const float* inv_beta, int n_iters, int lp,
                                 double min_val, int use_min, double thr_div, void* y, void* scale, void* zp,
                                 void* stat, void* idx, bvq_stream_t stream) {
  const char* what = "bvq_group_hqo_fwd";
  int rc = group_required(what, group_check(d, what, true), {x, inv_beta, y, scale, zp, stat, idx});
  if (!rc) rc = hqo_check(n_iters, lp, what);
  if ((rc = group_aligned(what, rc, {x, y}, "x and y"))) return rc;
  GroupHqoArgs h = group_args<GroupHqoArgs>(d, min_val, use_min, thr_div);
  if ((rc = hqo_fill(h, inv_beta, n_iters, what))) return rc;
  h.x = x;
  h.y = y;
  h.scale = scale;
  h.zp = zp;
  h.stat = stat;
  h.idx = idx;
  // x read + y written
  return group_launch(what, d->x_dtype, d->inner, h.chunks, 32, kGroupFwdDepth, [&](auto t, auto l, auto nt, unsigned grid) {
    using T = typename decltype(t)::type;
    if (lp == kHqoLp1)
      group_fwd_kernel<HqoQuant, T, l, nt><<<grid, kBlock, 0, (hipStream_t)stream>>>(h);
    else
      group_fwd_kernel<HqoQuantHalf, T, l, nt><<<grid, kBlock, 0, (hipStream_t)stream>>>(h);
  });
}

extern "C" int bvq_group_hqo_bwd(const bvq_quant_desc* d, const void* g, const void* x, const void* stat,
                                 const void* zp, const void* gscale, double min_val, int use_min, double thr_div,
                                 void* dx, bvq_stream_t stream) {
  const char* what = "bvq_group_hqo_bwd";
  int rc = group_required(what, group_check(d, what, true), {g, x, stat, zp, dx});
  if ((rc = group_aligned(what, rc, {g, x, dx}, "g, x and dx"))) return rc;
  GroupHqoArgs h = group_args<GroupHqoArgs>(d, min_val, use_min, thr_div);
  h.x = x;
  h.g = g;
  h.y = dx;
  h.stat = const_cast<void*>(stat);
  h.zp = const_cast<void*>(zp);
  h.gscale = gscale;
  // g and x read, dx written
  return group_launch(what, d->x_dtype, d->inner, h.chunks, 48, kGroupBwdDepth, [&](auto t, auto l, auto nt, unsigned grid) {
    group_bwd_kernel<HqoQuant, typename decltype(t)::type, l, nt><<<grid, kBlock, 0, (hipStream_t)stream>>>(h);
  });
}
