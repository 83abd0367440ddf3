// bvq_hadamard_kron.hip -- the Hadamard transform of order b = K * P along the last dimension of x[rows, H], K one of 12,
// 20, 28, 36 and P a power of two:
//   y = scale * (I_{H/b} (x) (H_K (x) H_P)) x,   H_K the Paley matrix (or its transpose), H_P the Sylvester one.
// The widths of QuaRot / SpinQuant rotations that are no power of two: 3072 .. 12288 = 12 * 2^n, 5120 = 20 * 256,
// 14336 = 28 * 512, 4608 = 36 * 128.
//
// Definition (include/bvq.h, "Hadamard transform of order K * 2^n"): a block is [K][P], K the high digit.  Every element
// is widened to float32; every sub-row of P elements takes the Sylvester stages h = 1 .. P / 2 in ascending order; then
// the K stage: for every column m and every output i, acc = s_i0 * v_0, then acc = acc + s_ij * v_j for j = 1 .. K - 1 in
// ascending order, one float32 addition each; one multiply by float32(scale); one rounding to T.
//
// One workgroup of four waves per row, on the row walk (bvq_row_walk.h: C <= 512 chunks two loads per lane, C <= 2048
// eight; lane l of wave w holds chunks j * 256 + 64 w + l), in three phases:
//   1. load the row, widen, and the Sylvester stages of a sub-row that stay inside a wave load: inside a chunk and
//      across the lanes (bvq_hadamard.h).  Every lane writes the float32 image of its chunks to LDS (16-byte writes, row
//      order); one barrier.  A row of at most 32 KiB leaves ONE stage above those, and for K = 12 only (P = 128 VEC,
//      h = 64 VEC: chunk c with chunk c ^ 64, waves w and w ^ 1): each lane reads its partner's chunk from the image,
//      folds it into its registers, and after a barrier writes its chunk again, then a barrier.
//   2. K * P rarely puts the K values of a column into one lane (5120 = 20 * 256 puts two sub-rows into one wave load),
//      hence the image: thread t takes the column pairs t, t + 256 .. of the H / 2K pairs of adjacent columns of the
//      row.  It reads the K pairs of its two columns at stride P (8 bytes a lane, consecutive lanes at consecutive
//      addresses: no bank conflict), forms the K outputs in registers -- K input pairs live, every step ONE packed
//      float32 add for the two columns, half the VALU issue of a column at a time -- and writes them back over the K
//      inputs, which no other thread touches.  The signs are constexpr masks per K (and per transpose for the Paley I
//      orders, whose matrix is not symmetric), so every step of the unrolled stage is a plain add or subtract.
//   3. one barrier, every lane reads its own chunks back (16-byte reads), multiplies, rounds and stores them where it
//      loaded them: coalesced, through the descriptor that drops the stores past the row's end.
// LDS: the image, 4 bytes per element of the row (at most 64 KiB), dynamic.  Every wave of a workgroup reaches every
// barrier: the grid is the rows, and what is skipped is skipped on values the whole workgroup shares (phase 2's loop
// bound differs by thread, and holds no barrier).  The row is whole in registers before the first barrier and stored
// after the last one, so y may be x.
//   reads x once, writes y once, ONE launch.  No workspace, no atomics, nothing between workgroups.
#include "bvq_hadamard.h"

namespace bvq {

struct HadamardKronArgs : HadamardArgs {  // lb: log2 P
  uint32_t columns;                       // cols / K: the columns of the K stage in a row
};

// The Paley matrices by formula, as sign masks: bit j of row[i] set <=> H[i][j] = -1; col[] the same of the transpose.
// chi the Legendre symbol mod q, Q[i][j] = chi(i - j).
//   Paley I  (q = K - 1 = 3 mod 4: 12, 20)      S = [[0, 1'], [-1, Q]], H = I + S
//   Paley II (q = K / 2 - 1 = 1 mod 4: 28, 36)  S = [[0, 1'], [1, Q]],  H = S (x) [[1, 1], [1, -1]] + I (x) [[1, -1], [-1, -1]]
template <int K>
struct PaleySigns {
  uint64_t row[K] = {}, col[K] = {};
  static constexpr bool kSymmetric = K == 28 || K == 36;  // Paley II
  static constexpr int q = kSymmetric ? K / 2 - 1 : K - 1;
  static constexpr int chi(int a) {
    a = ((a % q) + q) % q;
    if (a == 0) return 0;
    for (int x = 1; x < q; ++x)
      if (x * x % q == a) return 1;
    return -1;
  }
  static constexpr int border(int i, int j, int first_column) {  // S
    if (i == 0) return j == 0 ? 0 : 1;
    return j == 0 ? first_column : chi(i - j);
  }
  static constexpr int entry(int i, int j) {
    if constexpr (!kSymmetric) {
      return i == j ? 1 : border(i, j, -1);
    } else {
      const int s = border(i / 2, j / 2, 1), r = i & 1, c = j & 1;
      if (s != 0) return r && c ? -s : s;
      return r || c ? -1 : 1;
    }
  }
  constexpr PaleySigns() {
    for (int i = 0; i < K; ++i)
      for (int j = 0; j < K; ++j)
        if (entry(i, j) < 0) {
          row[i] |= (uint64_t)1 << j;
          col[j] |= (uint64_t)1 << i;
        }
  }
};
static_assert(PaleySigns<12>::q == 11 && PaleySigns<20>::q == 19 && PaleySigns<28>::q == 13 && PaleySigns<36>::q == 17,
              "the primes of the four orders");

// the K stage of two adjacent columns, one in each half of an f2_t: out_i = (..((s_i0 in_0 + s_i1 in_1) + s_i2 in_2) ..
// + s_i,K-1 in_K-1), every step one packed float32 add (v_pk_add_f32, the subtraction as its negate modifier), which
// rounds each half as the plain add does
typedef float f2_t __attribute__((ext_vector_type(2)));
template <int K, bool TR>
__device__ __forceinline__ void paley_mix(const f2_t (&in)[K], f2_t (&out)[K]) {
  constexpr PaleySigns<K> signs{};
#pragma unroll
  for (int i = 0; i < K; ++i) {
    const uint64_t minus = TR ? signs.col[i] : signs.row[i];
    f2_t acc = (minus & 1) ? -in[0] : in[0];
#pragma unroll
    for (int j = 1; j < K; ++j) acc = ((minus >> j) & 1) ? acc - in[j] : acc + in[j];
    out[i] = acc;
  }
}

extern __shared__ f4_t kron_lds[];
static_assert(kRowMaxBytes / 12 < 256 * 16, "a sub-row is at most 128 chunks: one stage above the lanes");

template <typename T, int K, int kD, bool TR, bool NT>
__global__ __launch_bounds__(kBlock) void hadamard_kron_kernel(HadamardKronArgs a) {
  constexpr int VEC = elem<T>::vec, LV = VEC == 8 ? 3 : 2, kW = kWavesPerBlock;
  RowSlot<kW> slot;
  slot.init(a);  // the grid is the rows
  const buf_t bx = slot.template elems<T>(a.x, a), by = slot.template elems<T>(a.y, a);
  vec_t<T, VEC> xv[kD];
#pragma unroll
  for (int j = 0; j < kD; ++j) xv[j] = buf_load<T, VEC, NT>(bx, slot.chunk(j) * 16u);
  const int lb = a.lb;
  const uint32_t lane = threadIdx.x & 63;
  float v[kD][VEC];
#pragma unroll
  for (int j = 0; j < kD; ++j)
#pragma unroll
    for (int k = 0; k < VEC; ++k) v[j][k] = to_f<T>(xv[j].v[k]);

  // the image ends with the row: a lane holds chunk j of it or, past the end, zeros that go nowhere
  const auto image_write = [&](int j) {
    if (slot.chunk(j) >= a.cpr) return;
#pragma unroll
    for (int q = 0; q < VEC / 4; ++q)
      kron_lds[slot.chunk(j) * (VEC / 4) + q] = f4_t{v[j][4 * q], v[j][4 * q + 1], v[j][4 * q + 2], v[j][4 * q + 3]};
  };

#pragma unroll
  for (int j = 0; j < kD; ++j) {
    if (slot.first(j) >= a.cpr) break;  // wave-uniform
    chunk_stages<VEC, LV>(v[j], lb);
    lane_stages<VEC, LV>(v[j], lane, lb);
    image_write(j);
  }
  __syncthreads();
  if (lb > LV + 6) {  // the stage h = 64 VEC; a sub-row is whole chunks of the row, so the partner's chunk is in the image
    const float sgn = (slot.wave & 1) ? -1.f : 1.f;
#pragma unroll
    for (int j = 0; j < kD; ++j) {
      if (slot.chunk(j) >= a.cpr) break;
#pragma unroll
      for (int q = 0; q < VEC / 4; ++q) {
        const f4_t partner = kron_lds[(slot.chunk(j) ^ kWave) * (VEC / 4) + q];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[j][4 * q + k] = pair_fold(sgn, v[j][4 * q + k], partner[k]);
      }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kD; ++j) image_write(j);
    __syncthreads();
  }

  // (P is at least four elements: a pair of columns lies in one sub-row, on an 8-byte boundary of the image)
  f2_t* image = reinterpret_cast<f2_t*>(kron_lds);
  const int lp = lb - 1;  // log2 of the pairs in a sub-row
  const uint32_t in_sub_row = (1u << lp) - 1;
  for (uint32_t c = threadIdx.x; c < a.columns / 2; c += kBlock) {
    f2_t* column = image + (((c >> lp) * K) << lp) + (c & in_sub_row);  // block c / (P / 2), sub-row 0, pair c % (P / 2)
    f2_t in[K], out[K];
#pragma unroll
    for (int j = 0; j < K; ++j) in[j] = column[(uint32_t)j << lp];
    paley_mix<K, TR>(in, out);
#pragma unroll
    for (int i = 0; i < K; ++i) column[(uint32_t)i << lp] = out[i];
  }
  __syncthreads();

#pragma unroll
  for (int j = 0; j < kD; ++j) {
    if (slot.chunk(j) >= a.cpr) break;  // (a lane's chunks ascend with j)
    vec_t<T, VEC> o;
#pragma unroll
    for (int q = 0; q < VEC / 4; ++q) {
      const f4_t r = kron_lds[slot.chunk(j) * (VEC / 4) + q];
#pragma unroll
      for (int k = 0; k < 4; ++k) o.v[4 * q + k] = from_f<T>(r[k] * a.scale);
    }
    buf_store<T, VEC, NT>(by, slot.chunk(j) * 16u, o);
  }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
// what the kernel covers, apart from the pointers: BVQ_OK and log2(block / base), or the error with its text
static int hadamard_kron_check(const char* what, int dtype, int64_t rows, int64_t cols, int64_t base, int64_t block,
                               int* lp) {
  if (const int rc = hadamard_shape_check(what, dtype, rows, cols)) return rc;
  if (base != 12 && base != 20 && base != 28 && base != 36) {
    set_error("%s: base %lld (12, 20, 28 or 36)", what, (long long)base);
    return BVQ_ERR_INVALID;
  }
  const int64_t p = block / base;
  if (block < base || block % base != 0 || (p & (p - 1)) != 0) {
    set_error("%s: block %lld is not %lld times a power of two", what, (long long)block, (long long)base);
    return BVQ_ERR_INVALID;
  }
  if (const int rc = hadamard_row_check(what, dtype, rows, cols, block)) return rc;
  if (p * dtype_size(dtype) % 16 != 0) {
    set_error("%s: a sub-row of %lld bytes (block / base elements: a multiple of 16 bytes)", what,
              (long long)(p * dtype_size(dtype)));
    return BVQ_ERR_UNSUPPORTED;
  }
  int l = 0;
  while (((int64_t)1 << l) < p) ++l;
  *lp = l;
  return BVQ_OK;
}

}  // namespace bvq

using namespace bvq;

extern "C" int bvq_hadamard_kron_supported(int dtype, int64_t rows, int64_t cols, int64_t base, int64_t block,
                                           const void* x, const void* y) {
  int lp;
  if (hadamard_kron_check("bvq_hadamard_kron_supported", dtype, rows, cols, base, block, &lp)) return 0;
  return x && y && aligned16(x) && aligned16(y) ? 1 : 0;
}

extern "C" int bvq_hadamard_kron(int dtype, const void* x, int64_t rows, int64_t cols, int64_t base, int64_t block,
                                 int transpose, double scale, void* y, bvq_stream_t stream) {
  const char* what = "bvq_hadamard_kron";
  HadamardKronArgs a{};
  int rc = group_required(what, hadamard_kron_check(what, dtype, rows, cols, base, block, &a.lb), {x, y});
  if ((rc = group_aligned(what, rc, {x, y}, "x and y"))) return rc;
  a.x = x;
  a.y = y;
  a.rows = rows;
  a.cpr = (uint32_t)(cols * dtype_size(dtype) / 16);
  a.chunks = rows * a.cpr;
  a.scale = (float)scale;
  a.columns = (uint32_t)(cols / base);
  const bool nt = a.chunks * 32 >= nt_threshold_bytes();  // x read + y written
  const bool deep = a.cpr > 2 * kBlock;
  rc = with_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    const size_t lds = (size_t)cols * 4;  // the image
    return with_value<12, 20, 28, 36>((int)base, [&](auto k) {
      const auto launch = [&](auto tr) {
        return with_bool(nt, [&](auto ntc) {
          if (deep)
            hadamard_kron_kernel<T, k, 8, tr, ntc><<<(unsigned)rows, kBlock, lds, (hipStream_t)stream>>>(a);
          else
            hadamard_kron_kernel<T, k, 2, tr, ntc><<<(unsigned)rows, kBlock, lds, (hipStream_t)stream>>>(a);
        });
      };
      // a symmetric matrix is its own transpose: one instantiation
      if constexpr (PaleySigns<k>::kSymmetric)
        return launch(std::false_type{});
      else
        return with_bool(transpose != 0, launch);
    });
  });
  return rc ? rc : check_launch(what);
}
