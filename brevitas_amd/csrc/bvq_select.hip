// bvq_select.hip -- exact k-th value per channel (percentile statistics) by MSD radix select.
//
// Replaces torch.kthvalue on |x| or x (AbsPercentile / NegativePercentileOrZero / PercentileInterval,
// B/core/stats/stats_op.py:41-126), which the default activation quantizer
// (Int8ActPerTensorFloat: AbsPercentile(99.999), B/quant/base.py:68-75) runs on every one of its
// first 300 training steps -- a sort-class kernel over the whole activation in the reference.
//
// Values are mapped to order-preserving unsigned keys (16 bits for bf16/f16, 32 for f32; every NaN
// sorts last, as torch.kthvalue orders them) and the k-th key is found digit by digit from the top:
// each pass streams x once, histograms one 11-bit digit of the keys that match the prefix found so
// far (the row-mapped walk of bvq_unit_walk.h; LDS, one private 2048-bin histogram per wave, flushed
// with global atomics), and a tiny kernel picks the bin that holds the k-th element.  16-bit types need
// 2 passes (11 + 5 bits), f32 3 (11 + 11 + 10); after the first pass almost no key matches the prefix,
// so later passes are pure streaming reads.  Algorithmic bytes per element: passes * sizeof(x).  The result is exact.
// One-channel (per-tensor) calls of bvq_kth_value take a wider first digit instead -- 15 bits, all 32768 bins in
// the LDS of one 1024-thread workgroup per CU -- and need one read (|x| of a 16-bit type) or two: see below.
#include "bvq_common.h"
#include "bvq_unit_walk.h"
#include "bvq_ties.h"

namespace bvq {

// Bin counters are uint32 end to end (per-wave LDS bins, the global histograms, the all-reduced shard sums): a bin
// may hold every element of a channel (a constant tensor, post-ReLU zeros), so a channel -- over ALL shards of a
// batch-sharded tensor -- must have fewer than 2^32 elements.  Enforced here per call and, for the shard count,
// by brevitas_amd.distributed.sharded_kth_value.
constexpr int64_t kSelMaxCount = 0xFFFFFFFFll;


constexpr int kDigitBits = 11;
constexpr int kBins = 1 << kDigitBits;
constexpr int kSelUnroll = 4;
constexpr int64_t kSelUnitCap = 4096;  // units per channel

// order-preserving key of a value
template <typename T, bool ABS>
__device__ __forceinline__ uint32_t sel_key(T v);

template <>
__device__ __forceinline__ uint32_t sel_key<float, true>(float v) {
  return __builtin_bit_cast(uint32_t, v) & 0x7fffffffu;  // NaN patterns exceed +inf
}
template <>
__device__ __forceinline__ uint32_t sel_key<float, false>(float v) {
  const uint32_t b = __builtin_bit_cast(uint32_t, v);
  if (v != v) return 0xffffffffu;
  return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}
template <typename T, bool ABS>
__device__ __forceinline__ uint32_t sel_key16(T v) {
  const uint32_t b = __builtin_bit_cast(uint16_t, v);
  if (ABS) return b & 0x7fffu;
  if (to_f<T>(v) != to_f<T>(v)) return 0xffffu;
  return b ^ ((b & 0x8000u) ? 0xffffu : 0x8000u);
}
template <>
__device__ __forceinline__ uint32_t sel_key<bf16_t, true>(bf16_t v) {
  return sel_key16<bf16_t, true>(v);
}
template <>
__device__ __forceinline__ uint32_t sel_key<bf16_t, false>(bf16_t v) {
  return sel_key16<bf16_t, false>(v);
}
template <>
__device__ __forceinline__ uint32_t sel_key<f16_t, true>(f16_t v) {
  return sel_key16<f16_t, true>(v);
}
template <>
__device__ __forceinline__ uint32_t sel_key<f16_t, false>(f16_t v) {
  return sel_key16<f16_t, false>(v);
}

struct SelArgs {
  Tiling t;
  const void* x;
  const uint32_t* prefix;  // [channels] key bits fixed by earlier passes (already shifted down)
  uint32_t* hist;          // [channels][kBins] of this pass
  int32_t shift;           // this pass looks at (key >> shift) & (kBins - 1) ...
  int32_t bits;            // ... of which `bits` low bits are significant (last pass may be narrower)
  int32_t first_pass;      // no prefix to match yet
};

template <typename T, int VEC, bool ABS, bool NT>
__global__ __launch_bounds__(kBlock) void kth_hist_kernel(SelArgs a) {
  __shared__ uint32_t lds[kWavesPerBlock][kBins];
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = threadIdx.x & 63;
  uint32_t* h = lds[wave];
  for (int b = lane; b < kBins; b += kWave) h[b] = 0;
  __syncthreads();  // every wave reaches this (the unit check comes after)
  const Unit u = locate_unit(a.t);
  if (!u.valid) return;
  const uint32_t want = a.first_pass ? 0u : a.prefix[u.channel];
  const int hi_shift = a.shift + a.bits;  // bits above this pass's digit
  const uint32_t mask = (1u << a.bits) - 1u;
  auto count = [&](T v) {
    const uint32_t key = sel_key<T, ABS>(v);
    const bool match = a.first_pass || (hi_shift >= 32 ? true : (key >> hi_shift) == want);
    if (match) atomicAdd(&h[(key >> a.shift) & mask], 1u);
  };
  walk_unit<T, VEC, NT, kSelUnroll>(
      u, reinterpret_cast<const T*>(a.x) + u.base, a.t.row_len, lane,
      [&](const vec_t<T, VEC>& xv, int64_t, int64_t) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) count(xv.v[k]);
      },
      [&](T v, int64_t, int64_t) { count(v); });
  // flush the non-empty bins of this wave's histogram
  uint32_t* gh = a.hist + (int64_t)u.channel * kBins;
  for (int b = lane; b < kBins; b += kWave) {
    const uint32_t c = h[b];
    if (c) atomicAdd(&gh[b], c);
  }
}

// rank rule of the percentile statistics (B/core/stats/stats_op.py:56,84,114-116), evaluated on the
// device from the number of elements the first histogram counted -- for a tensor sharded over several
// devices that is the GLOBAL count once the histograms have been summed, with no host round trip.
// python evaluates `.01 * q * n` left to right in double; IEEE doubles give the same bits here.
__device__ __forceinline__ int64_t rank_from_rule(int rule, double q, int64_t n) {
  double v = 0.01 * q;
  v = v * (double)n;
  int64_t k = rule == BVQ_KTH_HIGH ? (int64_t)floor(v + 0.5) : (int64_t)ceil(v);
  if (k < 1) k = 1;  // torch.kthvalue raises for k = 0; a device kernel cannot -- documented in bvq.h
  if (k > n) k = n;
  return k;
}

// One workgroup of kB threads per channel c = blockIdx.x: the bin of the channel's histogram hist[c][0, nbins) that
// holds the k-th (1-indexed) counted key; sel[c] <- sel[c] << bits | bin (first: sel[c] counts as 0, whatever it
// holds), krem[c] <- rank inside that bin.  kNBins: the bin count where it is fixed (the digit passes), 0: nbins.
// The rank k: from the rule and the histogram's total -- the GLOBAL element count once the shards' histograms have
// been summed -- when a rule is given (a first pick), else k_arg when that is > 0, else krem[c] (a later pick, or a
// first one whose rank bvq_kth_begin stored).
template <int kB, int kNBins>
__global__ __launch_bounds__(kB) void kth_pick_kernel(const uint32_t* __restrict__ hist, int32_t nbins, int32_t bits,
                                                      int32_t first, int64_t k_arg, uint32_t* __restrict__ sel,
                                                      int64_t* __restrict__ krem, int32_t rule, double q) {
  __shared__ int64_t part[kB];
  __shared__ int64_t before_me[kB];
  __shared__ int64_t k_sh;
  __shared__ uint32_t prev_sh;
  const int c = blockIdx.x;
  const int nb = kNBins ? kNBins : nbins;
  const uint32_t* h = hist + (int64_t)c * nb;
  static_assert(kNBins % kB == 0, "a fixed bin count is a whole number of bins per thread");
  const int per = (nb + kB - 1) / kB;  // consecutive bins per thread (a constant trip count where kNBins is given)
  const int lo = threadIdx.x * per, hi = kNBins || lo + per < nb ? lo + per : nb;
  int64_t mine = 0;
  for (int b = lo; b < hi; ++b) mine += h[b];
  part[threadIdx.x] = mine;
  __syncthreads();
  // exclusive prefix over the partial sums (serial on one thread: kB adds)
  if (threadIdx.x == 0) {
    int64_t run = 0;
    for (int t = 0; t < kB; ++t) {
      before_me[t] = run;
      run += part[t];
    }
    k_sh = rule != BVQ_KTH_EXPLICIT ? rank_from_rule(rule, q, run) : (k_arg > 0 ? k_arg : krem[c]);
    prev_sh = first ? 0u : sel[c];
  }
  __syncthreads();  // krem / sel have been read before the owner overwrites them
  const int64_t k = k_sh;
  int64_t run = before_me[threadIdx.x];
  if (k > run && k <= run + mine) {  // exactly one thread owns the k-th element
    for (int b = lo; b < hi; ++b) {
      const int64_t cnt = h[b];
      if (k <= run + cnt) {
        sel[c] = (prev_sh << bits) | (uint32_t)b;
        krem[c] = k - run;
        break;
      }
      run += cnt;
    }
  }
}

template <typename T, bool ABS>
__global__ void kth_store_kernel(const uint32_t* __restrict__ prefix, void* out, int32_t channels) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= channels) return;
  const uint32_t key = prefix[c];
  T* o = reinterpret_cast<T*>(out);
  if constexpr (sizeof(T) == 4) {
    const uint32_t b = ABS ? key : ((key >> 31) ? (key ^ 0x80000000u) : ~key);
    o[c] = __builtin_bit_cast(float, b);
  } else {
    const uint16_t b = (uint16_t)(ABS ? key : ((key & 0x8000u) ? (key ^ 0x8000u) : (~key & 0xffffu)));
    o[c] = __builtin_bit_cast(T, b);
  }
}

__global__ void kth_init_kernel(uint32_t* prefix, int64_t* krem, int64_t k, int32_t channels) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < channels) {
    prefix[c] = 0;
    krem[c] = k;
  }
}

// ---- per-tensor route of bvq_kth_value: 15-bit first digit in LDS, the rest through global counters ----------
// A workgroup of 1024 threads keeps ALL 32768 bins of the key's top 15 bits in LDS (128 of gfx950's 160 KB).
//  * |x| of a 16-bit type: that IS the whole key -- one streaming read decides the k-th value, where the digit
//    passes above read twice; and the keys spread over 16x more bins than an 11-bit digit, which is what the
//    LDS atomics of that first pass choke on (a bf16 activation puts ~5 % of its elements into the hottest
//    11-bit bin, 0.3 % into the hottest 15-bit one).
//  * every other key (16 signed bits, 31 or 32 bits of float32): a second read histograms the remaining
//    1 / 16 / 17 low bits of the few elements that fell into the chosen bin, straight into global counters
//    (a wave whose matching lanes all hold the same key adds their count once: constant tensors stay cheap).
// Two reads instead of three for float32, exact like the digit passes.
constexpr int kBins15 = 1 << 15;
constexpr int kBlock15 = 1024;
constexpr int kLowBitsMax = 17;
constexpr int64_t kLowStride = (int64_t)1 << kLowBitsMax;  // counters of one rank's second read

__global__ void kth_zero_kernel(uint32_t* p, int32_t n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = 0;
}

// first read, on walk_flat (x, n, head: see there): each workgroup counts in LDS and flushes its non-empty bins
template <typename T, bool ABS, bool NT>
__global__ __launch_bounds__(kBlock15) void kth_hist15_kernel(const T* __restrict__ x, int64_t n, int32_t shift,
                                                             uint32_t* __restrict__ hist, int32_t head) {
  __shared__ uint32_t h[kBins15];
  for (int b = threadIdx.x; b < kBins15; b += kBlock15) h[b] = 0;
  __syncthreads();
  walk_flat<T, kBlock15, NT, kSelUnroll>(x, n, head, [&](T v) { atomicAdd(&h[sel_key<T, ABS>(v) >> shift], 1u); });
  __syncthreads();
  for (int b = threadIdx.x; b < kBins15; b += kBlock15) {
    const uint32_t c = h[b];
    if (c) atomicAdd(&hist[b], c);
  }
}

// second read: low `shift` bits of the keys whose top 15 bits equal sel[0]
__device__ __forceinline__ void low_count(uint32_t key, uint32_t want, int32_t shift, uint32_t lowmask,
                                          uint32_t* __restrict__ ghist) {
  if ((key >> shift) == want) {
    const uint32_t low = key & lowmask;
    const uint32_t first = __builtin_amdgcn_readfirstlane(low);
    const uint64_t active = __builtin_amdgcn_ballot_w64(true);
    if (__builtin_amdgcn_ballot_w64(low != first) == 0) {
      if ((threadIdx.x & 63) == (uint32_t)__builtin_ctzll(active)) atomicAdd(&ghist[first], (uint32_t)__builtin_popcountll(active));
    } else {
      atomicAdd(&ghist[low], 1u);
    }
  }
}

// SMALL: at most 11 low bits (the last bit of a signed 16-bit key): the matching elements of a workgroup meet in
// an LDS histogram first -- with 2 bins, one global atomic per element would be ~10^4 serialized updates of
// the same two addresses
template <typename T, bool ABS, bool NT, bool SMALL>
__global__ __launch_bounds__(kBlock) void kth_low_kernel(const T* __restrict__ x, int64_t n, int32_t shift,
                                                        const uint32_t* __restrict__ sel, uint32_t* __restrict__ gh,
                                                        int32_t nk, int32_t head) {
  // nk (1 or 2) ranks are served by the same read: rank i has its own chosen bin sel[i] and its own counters
  __shared__ uint32_t lh[SMALL ? 2 * kBins : 1];
  if constexpr (SMALL) {
    for (int b = threadIdx.x; b < 2 * kBins; b += kBlock) lh[b] = 0;
    __syncthreads();
  }
  uint32_t* ghist = SMALL ? lh : gh;
  const int64_t hstride = SMALL ? kBins : kLowStride;
  const uint32_t want = sel[0], want2 = nk > 1 ? sel[1] : 0u;
  const uint32_t lowmask = (1u << shift) - 1u;
  // (head, chunks and tail reach low_count from separate branches of the walk: its ballots see whole waves)
  walk_flat<T, kBlock, NT, kSelUnroll>(x, n, head, [&](T v) {
    const uint32_t key = sel_key<T, ABS>(v);
    low_count(key, want, shift, lowmask, ghist);
    if (nk > 1) low_count(key, want2, shift, lowmask, ghist + hstride);
  });
  if constexpr (SMALL) {
    __syncthreads();
    for (int i = 0; i < nk; ++i)
      for (int b = threadIdx.x; b < (1 << shift); b += kBlock) {
        const uint32_t c = lh[i * kBins + b];
        if (c) atomicAdd(&gh[i * kLowStride + b], c);
      }
  }
}

}  // namespace bvq

using namespace bvq;

// ---- channel-last layouts (short `inner`): select on a transposed copy -----------------------------------------
// A per-channel radix select needs a channel's elements together: one private 2048-bin LDS histogram per wave is what
// makes the first digit pass cheap, and `channels x 2048` counters do not fit on chip for a wave that sees every
// channel in each row (channel-last [tokens, hidden], NHWC).  Round 2 sent such layouts down the row-mapped route with
// one-element rows (27 ms for AbsPercentile on [802816,512] bf16).  Round 3: the tensor, seen as a [rows][L = channels *
// inner] matrix, is transposed once into the caller's workspace -- [L][rows]: a channel's inner * rows elements are
// contiguous, in another order, which a k-th VALUE does not care about -- and every digit pass reads the copy as
// (outer = 1, channels, inner * rows).  64 x 64 tiles through LDS, 16-byte loads and stores: one read + one write.
constexpr int kTile = 64;

template <typename T>
__global__ __launch_bounds__(kBlock) void transpose_kernel(const T* __restrict__ x, T* __restrict__ out, int64_t R,
                                                           int64_t L) {
  constexpr int VEC = 16 / sizeof(T);              // elements per 16-byte access
  constexpr int kTPR = kTile / VEC;                // threads per tile row
  constexpr int kRPI = kBlock / kTPR;              // tile rows per load iteration
  __shared__ T tile[kTile][kTile + 16 / sizeof(T) / 4 * 2 + 2];  // padded pitch: the column reads below spread over the banks
  const int64_t r0 = (int64_t)blockIdx.x * kTile, c0 = (int64_t)blockIdx.y * kTile;
  const int tr = threadIdx.x / kTPR, tc = (threadIdx.x % kTPR) * VEC;
#pragma unroll
  for (int i = 0; i < kTile / kRPI; ++i) {
    const int r = tr + i * kRPI;
    if (r0 + r < R && c0 + tc < L) {  // (L is a multiple of VEC: a chunk is whole or absent)
      const vec_t<T, VEC> v = load_vec<T, VEC>(x + (r0 + r) * L + c0 + tc);
#pragma unroll
      for (int k = 0; k < VEC; ++k) tile[r][tc + k] = v.v[k];
    }
  }
  __syncthreads();
  // output row (c0 + oc) = tile column oc; a thread writes VEC consecutive original rows of it
  const bool aligned = (R * (int64_t)sizeof(T)) % 16 == 0;
#pragma unroll
  for (int i = 0; i < kTile / kRPI; ++i) {
    const int oc = tr + i * kRPI, orow = tc;
    if (c0 + oc >= L || r0 + orow >= R) continue;
    T* dst = out + (c0 + oc) * R + r0 + orow;
    if (aligned && r0 + orow + VEC <= R) {
      vec_t<T, VEC> v;
#pragma unroll
      for (int k = 0; k < VEC; ++k) v.v[k] = tile[orow + k][oc];
      store_vec<T, VEC>(dst, v);
    } else {
      for (int k = 0; k < VEC && r0 + orow + k < R; ++k) dst[k] = tile[orow + k][oc];
    }
  }
}

// the layouts that take the transposed copy, and where it lives in the workspace
static bool cols_select_applies(int dtype, const void* x, int64_t outer, int64_t channels, int64_t inner) {
  return x && (reinterpret_cast<uintptr_t>(x) & 15) == 0 && cols_plan(dtype, outer, channels, inner).ok;
}

// ---- workspace of the select entries (Carve, bvq_common.h; DESIGN.md, Workspaces) ------------------------------
// The entries publish byte offsets into the workspace (bvq_kth_hist_offset, bvq_kthw_plan) that the caller slices it at,
// so the layout must not depend on where the buffer starts: the base is on a 16-byte boundary (sel_carve refuses any
// other), the widest alignment a take() below asks for.  One buffer serves whichever route a call comes out with:
//   the step state | one channel: the wide state | a channel-last tensor: its transposed copy
// and a query is the layout measured, with no slack.
constexpr int kMaxPasses = 3;
static int passes_for(int dtype) { return dtype == BVQ_F32 ? kMaxPasses : 2; }

// the per-tensor ("wide") route's state, behind the step state of one channel
struct WideWs {
  uint32_t* counters;  // [counter_words] hist, then low: what a begin zeroes from its start
  uint32_t* hist;      // [hist_words] first digit
  uint32_t* low;       // [2][kLowStride] the second read's counters of each rank
  int64_t hist_words, counter_words;
  int64_t* krem;       // [2]
  uint32_t* sel;       // [2]
};
struct SelWs {
  uint32_t* counters;         // [passes][channels][kBins], what bvq_kth_begin zeroes
  uint32_t* hist[kMaxPasses];  // the counters of each pass
  int64_t pass_words, counter_words;
  int64_t* krem;     // [channels] remaining rank
  uint32_t* prefix;  // [channels]
  WideWs wide;       // channels == 1
};

// What lies behind the step state starts on the second multiple of 256 bytes past its end: there bvq_kthw_plan has
// published the wide counters since the route exists, and a sharded caller's slices stay where they were.
static void sel_skip_line(Carve& c) { c.take<char>((c.used + 255) / 256 * 256 + 256 - c.used); }

static WideWs sel_wide_layout(Carve& c) {
  WideWs w;
  sel_skip_line(c);
  w.hist_words = kBins15;
  w.counter_words = w.hist_words + 2 * kLowStride;
  w.counters = c.take<uint32_t>(w.counter_words);
  w.hist = w.counters;
  w.low = w.counters + w.hist_words;
  w.krem = c.take<int64_t>(2);
  w.sel = c.take<uint32_t>(2);
  return w;
}

static SelWs sel_layout(Carve& c, int dtype, int64_t channels) {
  SelWs s = {};
  s.pass_words = channels * kBins;
  s.counter_words = passes_for(dtype) * s.pass_words;
  s.counters = c.take<uint32_t>(s.counter_words);
  for (int p = 0; p < passes_for(dtype); ++p) s.hist[p] = s.counters + p * s.pass_words;
  s.krem = c.take<int64_t>(channels);
  s.prefix = c.take<uint32_t>(channels);
  if (channels == 1) s.wide = sel_wide_layout(c);
  return s;
}

// the transposed copy of a channel-last tensor, behind the state; moved in 16-byte accesses
struct alignas(16) Chunk16 { char b[16]; };
static void* sel_copy_layout(Carve& c, int64_t bytes) {
  sel_skip_line(c);
  return c.take<Chunk16>((bytes + 15) / 16);
}

// the layout from a stand-in base, never dereferenced: what the offset queries measure from
alignas(16) static char sel_origin[16];
static int64_t sel_offset_of(const void* p) {
  return (int64_t)(reinterpret_cast<uintptr_t>(p) - reinterpret_cast<uintptr_t>(sel_origin));
}

static void pass_bits(int dtype, int pass, int& bits, int& shift) {
  const int key_bits = dtype == BVQ_F32 ? 32 : 16;
  int done = 0;
  for (int p = 0;; ++p) {
    bits = (key_bits - done) < kDigitBits ? (key_bits - done) : kDigitBits;
    shift = key_bits - done - bits;
    if (p == pass) return;
    done += bits;
  }
}

// the state of every step, per channel or wide (channels = 1), carved from the caller's workspace
// (rest: the Carve, for what the caller takes behind the state)
static int sel_carve(const char* who, int dtype, int64_t channels, void* workspace, int64_t workspace_bytes, SelWs& s,
                     Carve* rest = nullptr) {
  if (bad_dtype(dtype) || channels < 1) {
    set_error("%s: bad argument", who);
    return BVQ_ERR_INVALID;
  }
  Carve ws(workspace);
  if (reinterpret_cast<uintptr_t>(workspace) & 15) {
    set_error("%s: the workspace must start on a 16-byte boundary (its published offsets are those of an aligned base)",
              who);
    return BVQ_ERR_INVALID;
  }
  s = sel_layout(ws, dtype, channels);
  if (!ws.fits(workspace_bytes)) {
    set_error("%s: workspace %lld < %lld bytes", who, (long long)workspace_bytes, (long long)ws.used);
    return BVQ_ERR_WORKSPACE;
  }
  if (rest) *rest = ws;
  return BVQ_OK;
}

static bool bad_rule(int rule) { return rule < BVQ_KTH_EXPLICIT || rule > BVQ_KTH_LOW; }
// a first pick's rank: an explicit k >= 1, or a percentile for the rule
static bool bad_rank(int rule, int64_t k, double q) {
  return bad_rule(rule) || (rule == BVQ_KTH_EXPLICIT ? k < 1 : !(q >= 0.0 && q <= 100.0));
}

// (a kernel, not hipMemsetAsync: every step of the select is then an ordinary launch under graph capture)
static void launch_zero(uint32_t* p, int64_t words, hipStream_t st) {
  kth_zero_kernel<<<dim3((unsigned)((words + 255) / 256)), dim3(256), 0, st>>>(p, (int32_t)words);
}

static int launch_store(int abs_key, int dtype, const uint32_t* keys, void* out, int64_t n, unsigned grid, unsigned block,
                        hipStream_t st) {
  return with_dtype(dtype, [&](auto t) {
    return with_bool(abs_key, [&](auto abs) {
      kth_store_kernel<typename decltype(t)::type, abs><<<grid, block, 0, st>>>(keys, out, (int32_t)n);
    });
  });
}

extern "C" int64_t bvq_kth_workspace_bytes(int dtype, int64_t outer, int64_t channels, int64_t inner) {
  if (bad_dtype(dtype) || outer < 0 || channels < 1 || inner < 0) {
    set_error("bvq_kth_workspace_bytes: bad argument");
    return -1;
  }
  return measured([&](Carve& c) {
    sel_layout(c, dtype, channels);
    // (the copy is sized whether or not x will turn out 16-byte aligned)
    if (cols_plan(dtype, outer, channels, inner).ok) sel_copy_layout(c, outer * channels * inner * (int64_t)dtype_size(dtype));
  });
}

extern "C" int bvq_kth_passes(int dtype) { return bad_dtype(dtype) ? -1 : passes_for(dtype); }

extern "C" int64_t bvq_kth_hist_offset(int dtype, int64_t channels, int pass) {
  if (bad_dtype(dtype) || channels < 1 || pass < 0 || pass >= passes_for(dtype)) return -1;
  Carve c(sel_origin);
  return sel_offset_of(sel_layout(c, dtype, channels).hist[pass]);
}

extern "C" int bvq_kth_begin(int dtype, int64_t channels, int rule, int64_t k, double q, void* workspace,
                             int64_t workspace_bytes, bvq_stream_t stream) {
  SelWs w;
  int rc = sel_carve("bvq_kth_begin", dtype, channels, workspace, workspace_bytes, w);
  if (rc) return rc;
  if (bad_rank(rule, k, q)) {
    set_error("bvq_kth_begin: bad rank (rule %d, k %lld, q %g)", rule, (long long)k, q);
    return BVQ_ERR_INVALID;
  }
  hipStream_t st = (hipStream_t)stream;
  launch_zero(w.counters, w.counter_words, st);
  kth_init_kernel<<<dim3((unsigned)((channels + 255) / 256)), dim3(256), 0, st>>>(
      w.prefix, w.krem, rule == BVQ_KTH_EXPLICIT ? k : 0, (int32_t)channels);
  return check_launch("bvq_kth_begin");
}

extern "C" int bvq_kth_hist(int abs_key, int dtype, const void* x, int64_t outer, int64_t channels,
                            int64_t inner, int pass, void* workspace, int64_t workspace_bytes,
                            bvq_stream_t stream) {
  Carve ws(nullptr);
  SelWs w;
  int rc = sel_carve("bvq_kth_hist", dtype, channels, workspace, workspace_bytes, w, &ws);
  if (rc) return rc;
  if (outer < 0 || inner < 0 || pass < 0 || pass >= passes_for(dtype)) {
    set_error("bvq_kth_hist: bad argument");
    return BVQ_ERR_INVALID;
  }
  if (outer * inner == 0) return BVQ_OK;  // an empty shard adds nothing to the histogram
  if (outer * inner > kSelMaxCount) {
    set_error("bvq_kth_hist: %lld elements per channel; the digit counters are 32-bit (limit 2^32 - 1 over all shards)",
              (long long)(outer * inner));
    return BVQ_ERR_UNSUPPORTED;
  }
  if (!x) {
    set_error("bvq_kth_hist: null pointer");
    return BVQ_ERR_INVALID;
  }
  hipStream_t st = (hipStream_t)stream;
  if (cols_select_applies(dtype, x, outer, channels, inner)) {
    // channel-last: pass 0 transposes x into the workspace, every pass reads the copy (outer = 1, inner * outer per channel)
    void* copy = sel_copy_layout(ws, outer * channels * inner * (int64_t)dtype_size(dtype));
    if (!ws.fits(workspace_bytes)) {
      set_error("bvq_kth_hist: workspace %lld < %lld bytes (channel-last layout: bvq_kth_workspace_bytes with the shape)",
                (long long)workspace_bytes, (long long)ws.used);
      return BVQ_ERR_WORKSPACE;
    }
    if (pass == 0) {
      const int64_t L = channels * inner;
      const dim3 tg((unsigned)((outer + kTile - 1) / kTile), (unsigned)((L + kTile - 1) / kTile));
      if (tg.y > 65535) {
        set_error("bvq_kth_hist: %lld columns exceed the transpose grid", (long long)L);
        return BVQ_ERR_UNSUPPORTED;
      }
      if (dtype == BVQ_F32)
        transpose_kernel<float><<<tg, dim3(kBlock), 0, st>>>(reinterpret_cast<const float*>(x),
                                                            reinterpret_cast<float*>(copy), outer, L);
      else  // bf16 / f16: 2-byte elements move as bit patterns
        transpose_kernel<uint16_t><<<tg, dim3(kBlock), 0, st>>>(reinterpret_cast<const uint16_t*>(x),
                                                               reinterpret_cast<uint16_t*>(copy), outer, L);
      rc = check_launch("bvq_kth_hist/transpose");
      if (rc) return rc;
    }
    x = copy;
    inner = outer * inner;
    outer = 1;
  }
  const void* ptrs[1] = {x};
  const RowView r = row_view(dtype, outer, channels, inner, ptrs, 1);
  const int vec = r.vec;
  SelArgs a;
  // every wave flushes a 2048-bin histogram: keep the waves few and their pieces long
  a.t = make_tiling(r.outer, (int32_t)channels, r.row_len, vec, kSelUnitCap);
  a.x = x;
  a.prefix = w.prefix;
  a.hist = w.hist[pass];
  int bits, shift;
  pass_bits(dtype, pass, bits, shift);
  a.bits = bits;
  a.shift = shift;
  a.first_pass = pass == 0;
  const bool nt = outer * channels * inner * (int64_t)dtype_size(dtype) >= nt_threshold_bytes();
  rc = with_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    return with_bool(abs_key, [&](auto abs) {
      return with_read_variant<elem<T>::vec>(vec, nt, [&](auto v, auto ntc) {
        kth_hist_kernel<T, v, abs, ntc><<<grid_for_units(a.t.units), kBlock, 0, st>>>(a);
      });
    });
  });
  return rc ? rc : check_launch("bvq_kth_hist");
}

extern "C" int bvq_kth_pick(int dtype, int64_t channels, int pass, int rule, double q, void* workspace,
                            int64_t workspace_bytes, bvq_stream_t stream) {
  SelWs w;
  int rc = sel_carve("bvq_kth_pick", dtype, channels, workspace, workspace_bytes, w);
  if (rc) return rc;
  if (pass < 0 || pass >= passes_for(dtype) || bad_rule(rule)) {
    set_error("bvq_kth_pick: bad argument");
    return BVQ_ERR_INVALID;
  }
  int bits, shift;
  pass_bits(dtype, pass, bits, shift);
  // the rank rule applies once, to the count of the first pass; otherwise the rank is the one bvq_kth_begin stored or
  // the last pick left
  kth_pick_kernel<kBlock, kBins><<<dim3((unsigned)channels), dim3(kBlock), 0, (hipStream_t)stream>>>(
      w.hist[pass], kBins, bits, pass == 0, 0, w.prefix, w.krem,
      pass == 0 ? rule : BVQ_KTH_EXPLICIT, q);
  return check_launch("bvq_kth_pick");
}

extern "C" int bvq_kth_finish(int abs_key, int dtype, int64_t channels, void* out, void* workspace,
                              int64_t workspace_bytes, bvq_stream_t stream) {
  SelWs w;
  int rc = sel_carve("bvq_kth_finish", dtype, channels, workspace, workspace_bytes, w);
  if (rc) return rc;
  if (!out) {
    set_error("bvq_kth_finish: null pointer");
    return BVQ_ERR_INVALID;
  }
  rc = launch_store(abs_key, dtype, w.prefix, out, channels, (unsigned)((channels + 255) / 256), 256, (hipStream_t)stream);
  return rc ? rc : check_launch("bvq_kth_finish");
}

// ---- the per-tensor route (see kth_hist15_kernel), as steps -----------------------------------------------------
// zero, histogram of pass p, pick of pass p for rank i, store: bvq_kth_value / bvq_kth_pair run them in order for nk = 1
// or 2 ranks (ONE histogram read, + one read for the low bits of both); each bvq_kthw_* entry (include/bvq.h: the same
// route for a batch-sharded tensor) is one of them.  The steps launch; their callers check the launch and choose the grid.
#ifndef BVQ_KTH_WIDE
#define BVQ_KTH_WIDE 1  // 0: the digit passes for every layout
#endif
constexpr bool kKthWide = BVQ_KTH_WIDE != 0;
static bool wide_select_applies(int64_t channels, int64_t n, const void* x) {
  return kKthWide && channels == 1 && n >= ((int64_t)1 << 22) && (reinterpret_cast<uintptr_t>(x) & 15) == 0;
}

// low bits left for the second read: 0 (|x| of a 16-bit type: one pass), 1, 16 or 17
static int wide_shift(int abs_key, int dtype) { return (dtype == BVQ_F32 ? 32 : 16) - (abs_key ? 1 : 0) - 15; }
static int wide_passes(int abs_key, int dtype) { return wide_shift(abs_key, dtype) ? 2 : 1; }
// the second read's SMALL form (kth_low_kernel)
static bool wide_low_small(int shift) { return shift <= kDigitBits; }
static int wide_block(int pass) { return pass == 0 ? kBlock15 : kBlock; }
// The grid of pass p that covers the chip.  First read: one workgroup per CU is all the LDS allows, 256 of them.
static unsigned wide_full_grid(int pass, int shift) { return pass == 0 ? 256 : wide_low_small(shift) ? 1024 : 2048; }

// x: 16-byte aligned, n elements behind it and `head` in front of it
static int wide_hist(int abs_key, int dtype, const void* x, int64_t n, int32_t head, int pass, int nk, unsigned grid,
                     const WideWs& w, hipStream_t st) {
  const int shift = wide_shift(abs_key, dtype);
  const bool nt = (n + head) * (int64_t)dtype_size(dtype) >= nt_threshold_bytes();
  return with_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    return with_bool(abs_key, [&](auto abs) {
      const T* xp = reinterpret_cast<const T*>(x);
      if (pass == 0)
        with_bool(nt, [&](auto ntc) { kth_hist15_kernel<T, abs, ntc><<<grid, kBlock15, 0, st>>>(xp, n, shift, w.hist, head); });
      else if (wide_low_small(shift))
        kth_low_kernel<T, abs, false, true><<<grid, kBlock, 0, st>>>(xp, n, shift, w.sel, w.low, nk, head);
      else
        with_bool(nt, [&](auto ntc) {
          kth_low_kernel<T, abs, ntc, false><<<grid, kBlock, 0, st>>>(xp, n, shift, w.sel, w.low, nk, head);
        });
    });
  });
}

// rank i of pass p; rule / k / q: the first pick's rank (bad_rank), ignored by the second
static void wide_pick(int abs_key, int dtype, int pass, int i, int rule, int64_t k, double q, const WideWs& w,
                      hipStream_t st) {
  const int shift = wide_shift(abs_key, dtype);
  if (pass == 0)
    kth_pick_kernel<kBlock15, 0><<<1, kBlock15, 0, st>>>(w.hist, kBins15, 15, 1, k, w.sel + i, w.krem + i, rule, q);
  else
    kth_pick_kernel<kBlock15, 0><<<1, kBlock15, 0, st>>>(w.low + i * kLowStride, 1 << shift, shift, 0, 0, w.sel + i,
                                                         w.krem + i, BVQ_KTH_EXPLICIT, 0.0);
}

static int wide_store(int abs_key, int dtype, void* out, int nk, const WideWs& w, hipStream_t st) {
  return launch_store(abs_key, dtype, w.sel, out, nk, 1, 64, st);
}

// the steps in order, for a tensor in one piece; out[nk]
static int wide_select(int abs_key, int dtype, const void* x, int64_t n, const int64_t* ks, int nk, void* out,
                       const WideWs& w, hipStream_t st) {
  const int shift = wide_shift(abs_key, dtype);
  launch_zero(w.counters, shift ? w.counter_words : w.hist_words, st);
  int rc = BVQ_OK;
  for (int p = 0; !rc && p < wide_passes(abs_key, dtype); ++p) {
    rc = wide_hist(abs_key, dtype, x, n, 0, p, nk, wide_full_grid(p, shift), w, st);
    for (int i = 0; !rc && i < nk; ++i) wide_pick(abs_key, dtype, p, i, BVQ_KTH_EXPLICIT, ks[i], 0.0, w, st);
  }
  if (!rc) rc = wide_store(abs_key, dtype, out, nk, w, st);
  return rc ? rc : check_launch("bvq_kth_value/wide");
}

extern "C" int bvq_kthw_plan(int abs_key, int dtype, int pass, int64_t* hist_offset_bytes, int64_t* hist_words) {
  if (bad_dtype(dtype)) return -1;
  const int passes = wide_passes(abs_key, dtype);
  if (pass < 0 || pass >= passes) return passes;  // (a query for the pass count alone)
  Carve c(sel_origin);
  const WideWs w = sel_layout(c, dtype, 1).wide;
  if (hist_offset_bytes) *hist_offset_bytes = sel_offset_of(pass ? w.low : w.hist);
  if (hist_words) *hist_words = pass ? (int64_t)1 << wide_shift(abs_key, dtype) : w.hist_words;
  return passes;
}

extern "C" int bvq_kthw_begin(int abs_key, int dtype, void* workspace, int64_t workspace_bytes, bvq_stream_t stream) {
  SelWs w;
  int rc = sel_carve("bvq_kthw_begin", dtype, 1, workspace, workspace_bytes, w);
  if (rc) return rc;
  const int shift = wide_shift(abs_key, dtype);  // (one rank: the first rank's low counters)
  launch_zero(w.wide.counters, w.wide.hist_words + (shift ? (int64_t)1 << shift : 0), (hipStream_t)stream);
  return check_launch("bvq_kthw_begin");
}

extern "C" int bvq_kthw_hist(int abs_key, int dtype, const void* x, int64_t n, int pass, void* workspace,
                             int64_t workspace_bytes, bvq_stream_t stream) {
  SelWs w;
  int rc = sel_carve("bvq_kthw_hist", dtype, 1, workspace, workspace_bytes, w);
  if (rc) return rc;
  if (n < 0 || pass < 0 || pass >= wide_passes(abs_key, dtype)) {
    set_error("bvq_kthw_hist: bad argument");
    return BVQ_ERR_INVALID;
  }
  if (n == 0) return BVQ_OK;  // an empty shard adds nothing
  if (n > kSelMaxCount) {
    set_error("bvq_kthw_hist: %lld elements; the counters are 32-bit (limit 2^32 - 1 over all shards)", (long long)n);
    return BVQ_ERR_UNSUPPORTED;
  }
  if (!x) {
    set_error("bvq_kthw_hist: null pointer");
    return BVQ_ERR_INVALID;
  }
  // the kernels take 16-byte chunks from an aligned address: the elements in front of it are counted one by one
  const int es = dtype_size(dtype);
  int64_t head = (int64_t)(((16 - (reinterpret_cast<uintptr_t>(x) & 15)) & 15) / (uintptr_t)es);
  if (head > n) head = n;
  // few elements: few workgroups (each one flushes its own histogram), at most the grid that covers the chip
  const int64_t chunks = (n - head) / (16 / es), per_group = (int64_t)wide_block(pass) * kSelUnroll;
  const int64_t full = wide_full_grid(pass, wide_shift(abs_key, dtype));
  int64_t grid = (chunks + per_group - 1) / per_group;
  grid = grid < 1 ? 1 : (grid > full ? full : grid);
  rc = wide_hist(abs_key, dtype, reinterpret_cast<const char*>(x) + head * es, n - head, (int32_t)head, pass, 1,
                 (unsigned)grid, w.wide, (hipStream_t)stream);
  return rc ? rc : check_launch("bvq_kthw_hist");
}

extern "C" int bvq_kthw_pick(int abs_key, int dtype, int pass, int rule, int64_t k, double q, void* workspace,
                             int64_t workspace_bytes, bvq_stream_t stream) {
  SelWs w;
  int rc = sel_carve("bvq_kthw_pick", dtype, 1, workspace, workspace_bytes, w);
  if (rc) return rc;
  if (pass < 0 || pass >= wide_passes(abs_key, dtype) || (pass == 0 ? bad_rank(rule, k, q) : bad_rule(rule))) {
    set_error("bvq_kthw_pick: bad argument");
    return BVQ_ERR_INVALID;
  }
  wide_pick(abs_key, dtype, pass, 0, rule, k, q, w.wide, (hipStream_t)stream);
  return check_launch("bvq_kthw_pick");
}

extern "C" int bvq_kthw_finish(int abs_key, int dtype, void* out, void* workspace, int64_t workspace_bytes,
                               bvq_stream_t stream) {
  SelWs w;
  int rc = sel_carve("bvq_kthw_finish", dtype, 1, workspace, workspace_bytes, w);
  if (rc) return rc;
  if (!out) {
    set_error("bvq_kthw_finish: null pointer");
    return BVQ_ERR_INVALID;
  }
  rc = wide_store(abs_key, dtype, out, 1, w.wide, (hipStream_t)stream);
  return rc ? rc : check_launch("bvq_kthw_finish");
}

// bvq_kth_value (nk = 1) and bvq_kth_pair (nk = 2): ranks ks[nk] -> out[nk][channels]; who: the entry the error text names
static int kth_select(const char* who, int abs_key, int dtype, const void* x, int64_t outer, int64_t channels,
                      int64_t inner, const int64_t* ks, int nk, void* out, void* workspace, int64_t workspace_bytes,
                      bvq_stream_t stream) {
  if (bad_dtype(dtype) || outer < 0 || channels < 1 || inner < 0) {
    set_error("%s: bad argument", who);
    return BVQ_ERR_INVALID;
  }
  const int64_t per_channel = outer * inner;
  if (per_channel > kSelMaxCount) {
    set_error("%s: %lld elements per channel; the digit counters are 32-bit (limit 2^32 - 1)", who,
              (long long)per_channel);
    return BVQ_ERR_UNSUPPORTED;
  }
  for (int i = 0; i < nk; ++i)
    if (ks[i] < 1 || ks[i] > per_channel) {  // torch.kthvalue: "selected index k out of range"
      set_error("%s: k = %lld out of range [1, %lld]", who, (long long)ks[i], (long long)per_channel);
      return BVQ_ERR_INVALID;
    }
  if (!x || !out || !workspace) {
    set_error("%s: null pointer", who);
    return BVQ_ERR_INVALID;
  }
  if (wide_select_applies(channels, per_channel, x)) {
    SelWs w;
    const int rc = sel_carve(who, dtype, 1, workspace, workspace_bytes, w);
    return rc ? rc : wide_select(abs_key, dtype, x, per_channel, ks, nk, out, w.wide, (hipStream_t)stream);
  }
  int rc = BVQ_OK;
  for (int i = 0; !rc && i < nk; ++i) {  // the digit passes, once per rank
    rc = bvq_kth_begin(dtype, channels, BVQ_KTH_EXPLICIT, ks[i], 0.0, workspace, workspace_bytes, stream);
    for (int p = 0; !rc && p < passes_for(dtype); ++p) {
      rc = bvq_kth_hist(abs_key, dtype, x, outer, channels, inner, p, workspace, workspace_bytes, stream);
      if (!rc) rc = bvq_kth_pick(dtype, channels, p, BVQ_KTH_EXPLICIT, 0.0, workspace, workspace_bytes, stream);
    }
    if (!rc)
      rc = bvq_kth_finish(abs_key, dtype, channels, reinterpret_cast<char*>(out) + i * channels * (int64_t)dtype_size(dtype),
                          workspace, workspace_bytes, stream);
  }
  return rc;
}

extern "C" int bvq_kth_value(int abs_key, int dtype, const void* x, int64_t outer, int64_t channels,
                             int64_t inner, int64_t k, void* out, void* workspace,
                             int64_t workspace_bytes, bvq_stream_t stream) {
  return kth_select("bvq_kth_value", abs_key, dtype, x, outer, channels, inner, &k, 1, out, workspace, workspace_bytes,
                    stream);
}

extern "C" int bvq_kth_pair(int abs_key, int dtype, const void* x, int64_t outer, int64_t channels, int64_t inner,
                            int64_t k_first, int64_t k_second, void* out, void* workspace, int64_t workspace_bytes,
                            bvq_stream_t stream) {
  const int64_t ks[2] = {k_first, k_second};
  return kth_select("bvq_kth_pair", abs_key, dtype, x, outer, channels, inner, ks, 2, out, workspace, workspace_bytes,
                    stream);
}
