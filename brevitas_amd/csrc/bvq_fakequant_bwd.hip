// bvq_fakequant_bwd.hip -- entry points of the quantizer backward (include/bvq.h) and the launches of its column-mapped
// and finishing kernels; the row-mapped kernel is instantiated per dtype family in bvq_fakequant_bwd_{bf16,f16,f32}.hip.
#include "bvq_fakequant_bwd.h"

namespace bvq {
extern template BVQ_LAUNCH_BWD(float, float);
extern template BVQ_LAUNCH_BWD(bf16_t, bf16_t);
extern template BVQ_LAUNCH_BWD(bf16_t, float);
extern template BVQ_LAUNCH_BWD(f16_t, f16_t);
extern template BVQ_LAUNCH_BWD(f16_t, float);
}  // namespace bvq

using namespace bvq;

static int launch_bwd_pair(const bvq_quant_desc* d, const QuantArgs& a, int vec, int mode, bool nt, hipStream_t st) {
  return with_pair(d->x_dtype, d->ct_dtype, [&](auto xt, auto ct) {
    return launch_bwd<typename decltype(xt)::type, typename decltype(ct)::type>(a, vec, mode, nt, st);
  });
}

static int64_t bwd_units(const bvq_quant_desc* d) {
  int64_t outer, row_len;
  int32_t channels;
  rows_of(d, outer, row_len, channels);
  // upper bound over the vector widths the launcher may pick
  const int full = 16 / dtype_size(d->x_dtype);
  const int64_t a = bwd_tiling(outer, channels, row_len, full).units;
  const int64_t b = bwd_tiling(outer, channels, row_len, 1).units;
  return a > b ? a : b;
}

// the column-mapped backward's scale-gradient workspace: the partial rows and their fold (floats), then, 8-byte aligned,
// the double-precision middle stage of the per-channel sums (rows of more than kSumSlice columns per channel)
static int64_t cols_bwd_mid_off(const ColsPlan& cp) {
  return (((cp.prows + cols_fold_scratch_rows(cp.prows)) * cp.L * (int64_t)sizeof(float) + 7) / 8) * 8;
}
static int64_t cols_bwd_sum_bytes(const ColsPlan& cp, int64_t inner, int64_t channels) {
  return cols_bwd_mid_off(cp) + channel_sums_mid_bytes(inner, channels);
}

extern "C" int64_t bvq_fakequant_bwd_workspace_bytes(const bvq_quant_desc* d) {
  if (validate(d, true)) return -1;
  int64_t outer, row_len;
  int32_t channels;
  rows_of(d, outer, row_len, channels);
  const int64_t units = bwd_units(d);
  const int64_t mid = channel_sums_mid_bytes(units / channels + 1, channels) + 16;
  int64_t bytes = 3 * units * (int64_t)sizeof(float) + mid + 256;  // (a third partial array: bvq_fakequant_bwd_bounds)
  const ColsPlan cp = cols_quant_plan(d, nullptr, nullptr, nullptr, false, true);
  if (cp.ok && cols_bwd_sum_bytes(cp, d->inner, channels) + 256 > bytes)
    bytes = cols_bwd_sum_bytes(cp, d->inner, channels) + 256;
  return bytes;
}

static int fakequant_bwd_impl(const bvq_quant_desc* d, const void* g, const void* x, const void* scale,
                             const void* zp, void* dx, float* dscale, float* dzp, const void* tie_stat,
                             int64_t* tie_info, void* workspace, int64_t workspace_bytes, bvq_stream_t stream,
                             const LearnedScaleEpilogue* epilogue, const float* bounds = nullptr,
                             float* dbounds = nullptr) {
  int rc = validate(d, true);
  if (rc) return rc;
  const bool act = d->pre_op >= BVQ_PRE_SIGMOID;  // bvq_act.h: the row-mapped kernel, dx and dscale only
  if (act && (tie_stat || dzp || bounds || dbounds || d->x_dtype != d->ct_dtype)) {
    set_error("bvq_fakequant_bwd: pre_op %d covers dx and dscale in x's dtype only (no ties, dzp or bounds)",
              d->pre_op);
    return BVQ_ERR_UNSUPPORTED;
  }
  const int64_t n = d->outer * d->channels * d->inner;
  hipStream_t st = (hipStream_t)stream;
  int64_t outer, row_len;
  int32_t channels;
  rows_of(d, outer, row_len, channels);
  const bool need_sums = dscale != nullptr || dzp != nullptr;
  if ((tie_stat != nullptr) != (tie_info != nullptr)) {
    set_error("bvq_fakequant_bwd: tie_stat and tie_info go together");
    return BVQ_ERR_INVALID;
  }
  if (tie_stat && (!dscale || dzp)) {
    set_error("bvq_fakequant_bwd: the tie search rides on the dscale variant (dscale set, dzp null)");
    return BVQ_ERR_UNSUPPORTED;
  }
  if (tie_stat && channels != d->channels) {
    set_error("bvq_fakequant_bwd: tie search needs the statistic's layout (per-channel scale iff "
              "channels > 1)");
    return BVQ_ERR_UNSUPPORTED;
  }
  if (tie_info) launch_tie_init(reinterpret_cast<unsigned long long*>(tie_info), channels, st);
  if (n == 0) {
    if (dscale) (void)hipMemsetAsync(dscale, 0, sizeof(float) * channels, st);
    if (dzp) (void)hipMemsetAsync(dzp, 0, sizeof(float) * channels, st);
    return BVQ_OK;
  }
  if (!g || !x || !scale || !zp || !dx) {
    set_error("bvq_fakequant_bwd: null pointer");
    return BVQ_ERR_INVALID;
  }
  if (dbounds && (dzp || tie_stat || !dscale)) {
    set_error("bvq_fakequant_bwd: the bound gradients ride on the dscale variant (dscale set, dzp / tie_stat null)");
    return BVQ_ERR_UNSUPPORTED;
  }
  if (!dzp && !bounds && !act) {
    const ColsPlan cp = cols_quant_plan(d, x, g, dx, !dscale && !tie_stat, true);
    if (cp.ok) {
      const int64_t need = dscale ? cols_bwd_sum_bytes(cp, d->inner, channels) : 0;
      if (dscale && (!workspace || workspace_bytes < need)) {
        set_error("bvq_fakequant_bwd: workspace %lld < %lld bytes", (long long)workspace_bytes, (long long)need);
        return BVQ_ERR_WORKSPACE;
      }
      ColsQuantArgs ca = {};
      fill_cols_args(ca, cp, d);
      ca.x = x;
      ca.g = g;
      ca.y = dx;
      ca.scale = scale;
      ca.zp = zp;
      ca.ds_part = dscale ? reinterpret_cast<float*>(workspace) : nullptr;
      ca.tie_stat = tie_stat;
      ca.tie_info = reinterpret_cast<unsigned long long*>(tie_info);
      const bool cnt = n * (int64_t)(3 * dtype_size(d->x_dtype)) >= nt_threshold_bytes();
      rc = with_cols_variant(d, cnt, [&](auto t, auto rm, auto ntc) {
        fakequant_bwd_cols_kernel<typename decltype(t)::type, rm, ntc><<<(unsigned)cp.units, kBlock, 0, st>>>(ca);
      });
      if (!rc) rc = check_launch("bvq_fakequant_bwd/cols");
      if (rc) return rc;
      if (dscale) {
        float* folded = nullptr;
        launch_cols_fold_sum_min(ca.ds_part, nullptr, cp.prows, cp.L, ca.ds_part + cp.prows * cp.L, nullptr, &folded,
                                 nullptr, st);
        launch_channel_sums(folded, nullptr, dscale, nullptr, 1, channels, d->inner,
                            reinterpret_cast<char*>(workspace) + cols_bwd_mid_off(cp), st, epilogue);
        rc = check_launch("bvq_fakequant_bwd/cols_sum");
      }
      return rc;
    }
  }
  const void* ptrs[3] = {x, g, dx};
  const int els[3] = {dtype_size(d->x_dtype), dtype_size(d->ct_dtype), dtype_size(d->x_dtype)};
  const int full = 16 / dtype_size(d->x_dtype);
  const int vec = snap_vec(pick_vec(full, outer * channels, row_len, ptrs, els, 3, true), full);
  QuantArgs a = {};
  a.t = bwd_tiling(outer, channels, row_len, vec);
  int64_t mid_off = 0;
  if (need_sums) {
    // float partials (8-byte aligned end), then the doubles of a split reduction
    mid_off = (((dbounds ? 3 : 2) * a.t.units * (int64_t)sizeof(float) + 7) / 8) * 8;
    const int64_t need = mid_off + channel_sums_mid_bytes(a.t.nob * a.t.ppr, channels);
    if (!workspace || workspace_bytes < need) {
      set_error("bvq_fakequant_bwd: workspace %lld < %lld bytes", (long long)workspace_bytes,
                (long long)need);
      return BVQ_ERR_WORKSPACE;
    }
    a.ds_part = reinterpret_cast<float*>(workspace);
    a.dzp_part = a.ds_part + a.t.units;
    a.dq_part = a.dzp_part + a.t.units;
  }
  a.x = x;
  a.g = g;
  a.scale = scale;
  a.zp = zp;
  a.y = dx;
  a.bounds = bounds;
  a.tie_stat = tie_stat;
  a.tie_info = reinterpret_cast<unsigned long long*>(tie_info);
  fill_args(a, d);
  const int mode = dbounds ? kBwdDsBounds : (tie_stat ? kBwdDsTies : (dzp ? kBwdDsDzp : (dscale ? kBwdDs : kBwdDx)));
  const bool nt =
      n * (int64_t)(2 * dtype_size(d->x_dtype) + dtype_size(d->ct_dtype)) >= nt_threshold_bytes();
  rc = launch_bwd_pair(d, a, vec, mode, nt, st);
  if (!rc) rc = check_launch("bvq_fakequant_bwd");
  if (rc) return rc;
  if (need_sums) {
    // dbounds: [d(qmin) per channel | d(qmax) per channel] (the bounds themselves are scalars: the caller adds the
    // channels up)
    launch_channel_sums(dscale ? a.ds_part : nullptr, (dzp || dbounds) ? a.dzp_part : nullptr, dscale,
                        dbounds ? dbounds : dzp, a.t.nob, channels, a.t.ppr,
                        reinterpret_cast<char*>(workspace) + mid_off, st, epilogue);
    if (dbounds)
      launch_channel_sums(a.dq_part, nullptr, dbounds + channels, nullptr, a.t.nob, channels, a.t.ppr,
                          reinterpret_cast<char*>(workspace) + mid_off, st, nullptr);
    rc = check_launch("bvq_fakequant_bwd/channel_sum");
  }
  return rc;
}

extern "C" int bvq_fakequant_bwd(const bvq_quant_desc* d, const void* g, const void* x,
                                 const void* scale, const void* zp, void* dx, float* dscale,
                                 float* dzp, const void* tie_stat, int64_t* tie_info, void* workspace,
                                 int64_t workspace_bytes, bvq_stream_t stream) {
  return fakequant_bwd_impl(d, g, x, scale, zp, dx, dscale, dzp, tie_stat, tie_info, workspace, workspace_bytes,
                            stream, nullptr);
}

extern "C" int bvq_fakequant_bwd_bounds(const bvq_quant_desc* d, const void* g, const void* x, const void* scale,
                                        const void* zp, const float* bounds, void* dx, float* dscale, float* dbounds,
                                        void* workspace, int64_t workspace_bytes, bvq_stream_t stream) {
  if (!bounds || !dscale) {
    set_error("bvq_fakequant_bwd_bounds: null pointer");
    return BVQ_ERR_INVALID;
  }
  return fakequant_bwd_impl(d, g, x, scale, zp, dx, dscale, nullptr, nullptr, nullptr, workspace, workspace_bytes,
                            stream, nullptr, bounds, dbounds);
}

extern "C" int bvq_fakequant_bwd_learned(const bvq_quant_desc* d, const void* g, const void* x, const void* scale,
                                         const void* zp, void* dx, float* dscale, const void* value, int value_dtype,
                                         double min_val, int use_min, double int_threshold, const void* gscale,
                                         void* dvalue, void* workspace, int64_t workspace_bytes,
                                         bvq_stream_t stream) {
  if (!value || !dvalue || !dscale || value_dtype < BVQ_F32 || value_dtype > BVQ_F16) {
    set_error("bvq_fakequant_bwd_learned: bad argument");
    return BVQ_ERR_INVALID;
  }
  if (d && d->zp_per_channel) {
    set_error("bvq_fakequant_bwd_learned: per-channel zero-points are not covered");
    return BVQ_ERR_UNSUPPORTED;
  }
  LearnedScaleEpilogue ep = {};
  ep.value = value;
  ep.dvalue = dvalue;
  ep.gscale = gscale;
  ep.value_dtype = value_dtype;
  ep.scale_dtype = d ? d->scale_dtype : BVQ_F32;
  ep.use_min = use_min;
  ep.min_val = round_host((float)min_val, value_dtype);    // python scalar -> the parameter's dtype
  ep.int_threshold = (float)int_threshold;                  // the caller rounds it to the division's dtype
  return fakequant_bwd_impl(d, g, x, scale, zp, dx, dscale, nullptr, nullptr, nullptr, workspace, workspace_bytes,
                            stream, &ep);
}

static bool bwd_stats_supported(const bvq_quant_desc* d, int64_t& units, int64_t& per_channel) {
  if (!(d->scale_per_channel && d->channels > 1) || d->zp_per_channel) return false;
  const ColsPlan cp = cols_quant_plan(d, nullptr, nullptr, nullptr, false, true);
  if (cp.ok) {  // column-mapped partials: [prows][L] plus their fold [L]; first positions [L]
    units = (cp.prows + cols_fold_scratch_rows(cp.prows)) * cp.L;
    per_channel = d->inner;
    return true;
  }
  units = bwd_units(d);
  per_channel = units / d->channels;
  return per_channel <= 4096;  // one workgroup of bwd_stats_finish_kernel per channel walks them
}

extern "C" int64_t bvq_fakequant_bwd_stats_workspace_bytes(const bvq_quant_desc* d) {
  if (validate(d)) return -1;
  int64_t units, per_channel;
  if (!bwd_stats_supported(d, units, per_channel)) return 0;  // use bvq_fakequant_bwd + bvq_stat_tie_apply_dscale
  const ColsPlan cp = cols_quant_plan(d, nullptr, nullptr, nullptr, false, true);
  if (cp.ok)  // float partial rows and their fold, then one first position per column
    return units * (int64_t)sizeof(float) + cp.L * (int64_t)sizeof(unsigned long long) + 256;
  return units * (int64_t)(sizeof(float) + sizeof(unsigned long long)) + 256;
}

struct ShardOut {  // batch-sharded tensors: the all-gather message instead of the deposit (null: unsharded)
  double* msg;
  long long* pos;
  int32_t rank;
};
static int bwd_stats_impl(const bvq_quant_desc* d, const void* g, const void* x, const void* scale, const void* zp,
                          const void* stat, void* dx, float* dscale, int scale_dtype, double int_threshold,
                          int quot_dtype, void* workspace, int64_t workspace_bytes, uint32_t* arrive,
                          int64_t arrive_words, bvq_stream_t stream, const ShardOut* shard = nullptr);

extern "C" int bvq_fakequant_bwd_stats(const bvq_quant_desc* d, const void* g, const void* x, const void* scale,
                                       const void* zp, const void* stat, void* dx, float* dscale,
                                       int scale_dtype, double int_threshold, int quot_dtype, void* workspace,
                                       int64_t workspace_bytes, bvq_stream_t stream) {
  return bwd_stats_impl(d, g, x, scale, zp, stat, dx, dscale, scale_dtype, int_threshold, quot_dtype, workspace,
                        workspace_bytes, nullptr, 0, stream);
}

extern "C" int bvq_fakequant_bwd_stats_onepass_supported(const bvq_quant_desc* d) {
  int64_t units, per_channel;
  if (validate(d) || !bwd_stats_supported(d, units, per_channel)) return 0;
  if (cols_quant_plan(d, nullptr, nullptr, nullptr).ok) return 0;  // column-mapped layouts: two launches
  // the one-launch kernel's instantiations (x's alignment, which may still narrow the vector width, is checked at launch)
  const int full = 16 / dtype_size(d->x_dtype);
  return stream_full_rne(full, full, d->round_mode) ? 1 : 0;
}

extern "C" int bvq_fakequant_bwd_stats_onepass(const bvq_quant_desc* d, const void* g, const void* x,
                                               const void* scale, const void* zp, const void* stat, void* dx,
                                               float* dscale, int scale_dtype, double int_threshold, int quot_dtype,
                                               void* workspace, int64_t workspace_bytes, uint32_t* arrive,
                                               int64_t arrive_words, bvq_stream_t stream) {
  if (!arrive) {
    set_error("bvq_fakequant_bwd_stats_onepass: null arrival buffer");
    return BVQ_ERR_INVALID;
  }
  if (!bvq_fakequant_bwd_stats_onepass_supported(d)) {
    set_error("bvq_fakequant_bwd_stats_onepass: layout not covered: use bvq_fakequant_bwd_stats");
    return BVQ_ERR_UNSUPPORTED;
  }
  if (arrive_words < d->channels) {
    set_error("bvq_fakequant_bwd_stats_onepass: arrival buffer of %lld words, %lld needed", (long long)arrive_words,
              (long long)d->channels);
    return BVQ_ERR_WORKSPACE;
  }
  return bwd_stats_impl(d, g, x, scale, zp, stat, dx, dscale, scale_dtype, int_threshold, quot_dtype, workspace,
                        workspace_bytes, arrive, arrive_words, stream);
}

extern "C" int bvq_fakequant_bwd_shard(const bvq_quant_desc* d, const void* g, const void* x, const void* scale,
                                       const void* zp, const void* stat, void* dx, double* message, int64_t* first_pos,
                                       int rank, void* workspace, int64_t workspace_bytes, uint32_t* arrive,
                                       int64_t arrive_words, bvq_stream_t stream) {
  if (!message || !first_pos || rank < 0) {
    set_error("bvq_fakequant_bwd_shard: bad argument");
    return BVQ_ERR_INVALID;
  }
  if (arrive && (!bvq_fakequant_bwd_stats_onepass_supported(d) || arrive_words < d->channels)) arrive = nullptr;
  ShardOut so = {message, reinterpret_cast<long long*>(first_pos), rank};
  float unused = 0.f;
  return bwd_stats_impl(d, g, x, scale, zp, stat, dx, &unused, BVQ_F32, 1.0, BVQ_F32, workspace, workspace_bytes, arrive,
                        arrive_words, stream, &so);
}

extern "C" int bvq_shard_unpack_deposit(int dtype, const void* x, void* dx, const double* gathered, int world,
                                        int64_t channels, int rank, const int64_t* first_pos, int64_t inner,
                                        int scale_dtype, double int_threshold, int quot_dtype, int pre_op,
                                        float* dscale_total, bvq_stream_t stream) {
  // (x and dx both null: an empty shard, which owns no deposit)
  if (dtype < BVQ_F32 || dtype > BVQ_F16 || scale_dtype < BVQ_F32 || scale_dtype > BVQ_F16 || quot_dtype < BVQ_F32 ||
      quot_dtype > BVQ_F16 || channels < 1 || world < 1 || rank < 0 || rank >= world || inner < 1 ||
      (x == nullptr) != (dx == nullptr) || !gathered || !first_pos || !(int_threshold == int_threshold)) {
    set_error("bvq_shard_unpack_deposit: bad argument");
    return BVQ_ERR_INVALID;
  }
  GstatSrc gs = {};
  gs.from_dscale = 1;
  gs.scale_dtype = scale_dtype;
  gs.quot_dtype = quot_dtype;
  gs.int_threshold = (float)int_threshold;
  if (const int prc = check_pre_op(pre_op, "bvq_shard_unpack_deposit")) return prc;
  gs.pre_relu = pre_op == BVQ_PRE_RELU;
  const dim3 grid((unsigned)((channels + 255) / 256)), block(256);
  hipStream_t st = (hipStream_t)stream;
  const long long* fp = reinterpret_cast<const long long*>(first_pos);
  const int rc = with_dtype(dtype, [&](auto t) {
    shard_unpack_deposit_kernel<typename decltype(t)::type><<<grid, block, 0, st>>>(gathered, world, (int32_t)channels,
                                                                                    rank, fp, x, dx, inner, gs, dscale_total);
  });
  return rc ? rc : check_launch("bvq_shard_unpack_deposit");
}

static int bwd_stats_impl(const bvq_quant_desc* d, const void* g, const void* x, const void* scale, const void* zp,
                          const void* stat, void* dx, float* dscale, int scale_dtype, double int_threshold,
                          int quot_dtype, void* workspace, int64_t workspace_bytes, uint32_t* arrive,
                          int64_t arrive_words, bvq_stream_t stream, const ShardOut* shard) {
  int rc = validate(d);
  if (rc) return rc;
  int64_t units, per_channel;
  if (!bwd_stats_supported(d, units, per_channel)) {
    set_error("bvq_fakequant_bwd_stats: layout not covered (per-tensor scale or too many units per channel)");
    return BVQ_ERR_UNSUPPORTED;
  }
  if (scale_dtype < BVQ_F32 || scale_dtype > BVQ_F16 || quot_dtype < BVQ_F32 || quot_dtype > BVQ_F16) {
    set_error("bvq_fakequant_bwd_stats: bad dtype");
    return BVQ_ERR_INVALID;
  }
  const int64_t n = d->outer * d->channels * d->inner;
  hipStream_t st = (hipStream_t)stream;
  const int32_t channels = (int32_t)d->channels;
  if (n == 0) {
    if (shard) {  // an empty shard claims nothing: zero sums, no owner, no position (dscale is the entry's dummy)
      QuantArgs fa = {};
      fa.t.nob = 1;
      fa.t.channels = channels;
      fa.arrive_per_channel = 0;  // no partials: channel_finish reads none and writes acc = 0, pmin = ~0
      fa.shard_msg = shard->msg;
      fa.shard_pos = shard->pos;
      fa.shard_rank = shard->rank;
      const dim3 cgrid((unsigned)((channels + kWavesPerBlock - 1) / kWavesPerBlock));
      channel_finish_kernel<float><<<cgrid, dim3(kBlock), 0, st>>>(fa);
      return check_launch("bvq_fakequant_bwd_shard/empty");
    }
    if (dscale) (void)hipMemsetAsync(dscale, 0, sizeof(float) * channels, st);
    return BVQ_OK;
  }
  if (!g || !x || !scale || !zp || !stat || !dx || !dscale || !workspace) {
    set_error("bvq_fakequant_bwd_stats: null pointer");
    return BVQ_ERR_INVALID;
  }
  GstatSrc gs = {};
  gs.from_dscale = 1;
  gs.scale_dtype = scale_dtype;
  gs.quot_dtype = quot_dtype;
  gs.int_threshold = (float)int_threshold;
  gs.pre_relu = d->pre_op == BVQ_PRE_RELU;
  const bool nt =
      n * (int64_t)(2 * dtype_size(d->x_dtype) + dtype_size(d->ct_dtype)) >= nt_threshold_bytes();
  {
    const ColsPlan cp = cols_quant_plan(d, x, g, dx, false, true);
    const ColsPlan sized = cols_quant_plan(d, nullptr, nullptr, nullptr, false, true);
    if (sized.ok && !cp.ok) {
      set_error("bvq_fakequant_bwd_stats: the column-mapped route needs 16-byte aligned x, g and dx");
      return BVQ_ERR_UNSUPPORTED;
    }
    if (cp.ok) {
      const int64_t words = (cp.prows + cols_fold_scratch_rows(cp.prows)) * cp.L;
      const int64_t pos_off_c = ((words * (int64_t)sizeof(float) + 7) / 8) * 8;
      if (workspace_bytes < pos_off_c + cp.L * (int64_t)sizeof(unsigned long long)) {
        set_error("bvq_fakequant_bwd_stats: workspace too small");
        return BVQ_ERR_WORKSPACE;
      }
      ColsQuantArgs ca = {};
      fill_cols_args(ca, cp, d);
      ca.x = x;
      ca.g = g;
      ca.y = dx;
      ca.scale = scale;
      ca.zp = zp;
      ca.ds_part = reinterpret_cast<float*>(workspace);
      // first positions attaining the statistic: one entry per column, taken by atomic min from the few lanes that see it
      ca.pos_part = reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(workspace) + pos_off_c);
      ca.tie_stat = stat;
      launch_tie_init(ca.pos_part, cp.L, st);
      rc = with_cols_variant(d, nt, [&](auto t, auto rm, auto ntc) {
        fakequant_bwd_cols_kernel<typename decltype(t)::type, rm, ntc><<<(unsigned)cp.units, kBlock, 0, st>>>(ca);
      });
      if (!rc) rc = check_launch("bvq_fakequant_bwd_stats/cols");
      if (rc) return rc;
      float* ds_fold = nullptr;
      unsigned long long* pos_fold = ca.pos_part;
      launch_cols_fold_sum_min(ca.ds_part, nullptr, cp.prows, cp.L, ca.ds_part + cp.prows * cp.L, nullptr, &ds_fold,
                               nullptr, st);
      if (shard) {  // this shard's all-gather message from the folded partials: one wave per channel
        QuantArgs fa = {};
        fa.t.nob = 1;
        fa.t.channels = channels;
        fa.t.ppr = d->inner;
        fa.arrive_per_channel = (uint32_t)d->inner;
        fa.ds_part = ds_fold;
        fa.pos_part = pos_fold;
        fa.shard_msg = shard->msg;
        fa.shard_pos = shard->pos;
        fa.shard_rank = shard->rank;
        const dim3 cgrid((unsigned)((channels + kWavesPerBlock - 1) / kWavesPerBlock));
        channel_finish_kernel<float><<<cgrid, dim3(kBlock), 0, st>>>(fa);  // (the message path touches no tensor element)
        return check_launch("bvq_fakequant_bwd_shard/cols_finish");
      }
      rc = with_dtype(d->x_dtype, [&](auto t) {
        bwd_stats_finish_kernel<typename decltype(t)::type><<<(unsigned)channels, kBlock, 0, st>>>(
            ds_fold, pos_fold, dscale, gs, x, dx, 1, channels, d->inner, d->inner);
      });
      return rc ? rc : check_launch("bvq_fakequant_bwd_stats/cols_finish");
    }
  }
  const void* ptrs[3] = {x, g, dx};
  const int els[3] = {dtype_size(d->x_dtype), dtype_size(d->ct_dtype), dtype_size(d->x_dtype)};
  const int full = 16 / dtype_size(d->x_dtype);
  const int vec = snap_vec(pick_vec(full, d->outer * channels, d->inner, ptrs, els, 3, true), full);
  QuantArgs a = {};
  a.t = bwd_tiling(d->outer, channels, d->inner, vec);
  const int64_t pos_off = ((a.t.units * (int64_t)sizeof(float) + 7) / 8) * 8;
  if (workspace_bytes < pos_off + a.t.units * (int64_t)sizeof(unsigned long long)) {
    set_error("bvq_fakequant_bwd_stats: workspace too small");
    return BVQ_ERR_WORKSPACE;
  }
  a.ds_part = reinterpret_cast<float*>(workspace);
  a.pos_part = reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(workspace) + pos_off);
  a.x = x;
  a.g = g;
  a.scale = scale;
  a.zp = zp;
  a.y = dx;
  a.tie_stat = stat;
  fill_args(a, d);
  a.arrive_per_channel = (uint32_t)(a.t.nob * a.t.ppr);
  if (shard) {
    a.shard_msg = shard->msg;
    a.shard_pos = shard->pos;
    a.shard_rank = shard->rank;
  }
  if (arrive && !stream_full_rne(vec, full, d->round_mode)) arrive = nullptr;  // two launches for the rare forms
  if (arrive) {  // one launch: the wave that completes a channel finishes it
    a.arrive = arrive;
    a.dscale_out = dscale;
    a.gs_scale_dtype = scale_dtype;
    a.gs_quot_dtype = quot_dtype;
    a.gs_int_threshold = (float)int_threshold;
    rc = launch_bwd_pair(d, a, vec, kBwdDsArrive, nt, st);
    return rc ? rc : check_launch("bvq_fakequant_bwd_stats_onepass");
  }
  rc = launch_bwd_pair(d, a, vec, kBwdDsTies, nt, st);
  if (!rc) rc = check_launch("bvq_fakequant_bwd_stats");
  if (rc) return rc;
  if (shard) {
    const dim3 cgrid((unsigned)((channels + kWavesPerBlock - 1) / kWavesPerBlock));
    channel_finish_kernel<float><<<cgrid, dim3(kBlock), 0, st>>>(a);  // (the message path touches no tensor element)
    return check_launch("bvq_fakequant_bwd_shard/finish");
  }
  rc = with_dtype(d->x_dtype, [&](auto t) {
    bwd_stats_finish_kernel<typename decltype(t)::type><<<(unsigned)channels, kBlock, 0, st>>>(
        a.ds_part, a.pos_part, dscale, gs, x, dx, a.t.nob, channels, a.t.ppr, d->inner);
  });
  return rc ? rc : check_launch("bvq_fakequant_bwd_stats/finish");
}

