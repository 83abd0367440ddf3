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

// the tensors every backward entry takes
struct BwdTensors { const void *g, *x, *scale, *zp; void* dx; };
struct ShardOut {  // batch-sharded tensors: the all-gather message instead of the deposit (null: unsharded)
  double* msg;
  long long* pos;
  int32_t rank;
};

// the row-mapped kernel of `mode` on a's units
static int launch_bwd_rows(const bvq_quant_desc* d, const QuantArgs& a, const BwdRowPlan& p, int mode, hipStream_t st,
                           const char* what) {
  const int rc = with_pair(d->x_dtype, d->ct_dtype, [&](auto xt, auto ct) {
    return launch_bwd<typename decltype(xt)::type, typename decltype(ct)::type>(a, p.vec, mode, p.nt, st);
  });
  return rc ? rc : check_launch(what);
}

// the arguments of the row-mapped backward: partials from the layout w, the message of a shard
static QuantArgs rows_bwd_args(const bvq_quant_desc* d, const Tiling& t, const BwdTensors& T, const void* tie_stat,
                               int64_t* tie_info, const BwdWs& w, const ShardOut* shard = nullptr) {
  QuantArgs a = {};
  a.t = t;
  a.x = T.x;
  a.g = T.g;
  a.scale = T.scale;
  a.zp = T.zp;
  a.y = T.dx;
  a.tie_stat = tie_stat;
  a.tie_info = reinterpret_cast<unsigned long long*>(tie_info);
  fill_args(a, d);
  a.ds_part = w.ds;
  a.dzp_part = w.dzp;
  a.dq_part = w.dq;
  a.pos_part = w.pos;
  a.arrive_per_channel = (uint32_t)(t.nob * t.ppr);
  if (shard) {
    a.shard_msg = shard->msg;
    a.shard_pos = shard->pos;
    a.shard_rank = shard->rank;
  }
  return a;
}

// the column-mapped backward on cp's units, its partials from the layout w
static int launch_bwd_cols(const bvq_quant_desc* d, const ColsPlan& cp, const BwdTensors& T, const void* tie_stat,
                           int64_t* tie_info, const BwdWs& w, hipStream_t st, const char* what) {
  ColsQuantArgs ca = {};
  fill_cols_args(ca, cp, d);
  ca.x = T.x;
  ca.g = T.g;
  ca.y = T.dx;
  ca.scale = T.scale;
  ca.zp = T.zp;
  ca.ds_part = w.ds;
  ca.pos_part = w.pos;
  ca.tie_stat = tie_stat;
  ca.tie_info = reinterpret_cast<unsigned long long*>(tie_info);
  const int rc = with_cols_variant(d, bwd_nt(d), [&](auto t, auto rm, auto ntc) {
    fakequant_bwd_cols_kernel<typename decltype(t)::type, rm, ntc><<<(unsigned)cp.units, kBlock, 0, st>>>(ca);
  });
  return rc ? rc : check_launch(what);
}
static float* fold_cols_sums(const ColsPlan& cp, const BwdWs& w, hipStream_t st) {
  float* folded = nullptr;
  launch_cols_fold_sum_min(w.ds, nullptr, cp.prows, cp.L, w.fold, nullptr, &folded, nullptr, st);
  return folded;
}

// a shard's all-gather message from a's partials: one wave per channel (the message path touches no tensor element)
static int launch_channel_finish(const QuantArgs& a, hipStream_t st, const char* what) {
  const dim3 cgrid((unsigned)((a.t.channels + kWavesPerBlock - 1) / kWavesPerBlock));
  channel_finish_kernel<float><<<cgrid, dim3(kBlock), 0, st>>>(a);
  return check_launch(what);
}
// ... where no row-mapped launch wrote them: the folded columns, or none (an empty shard: zero sums, no owner)
static QuantArgs shard_finish_args(const ShardOut& so, int32_t channels, int64_t per_channel, float* ds,
                                   unsigned long long* pos) {
  QuantArgs fa = {};
  fa.t.nob = 1;
  fa.t.channels = channels;
  fa.t.ppr = per_channel;
  fa.arrive_per_channel = (uint32_t)per_channel;
  fa.ds_part = ds;
  fa.pos_part = pos;
  fa.shard_msg = so.msg;
  fa.shard_pos = so.pos;
  fa.shard_rank = so.rank;
  return fa;
}

extern "C" int64_t bvq_fakequant_bwd_workspace_bytes(const bvq_quant_desc* d) {
  if (validate(d, true)) return -1;
  // (with the third partial array of bvq_fakequant_bwd_bounds)
  int64_t bytes = measured_widths(d->x_dtype, [&](Carve& c, int vec) {
    bwd_sums_layout(c, bwd_row_plan(d, nullptr, nullptr, nullptr, vec).t, true);
  });
  const ColsPlan cp = cols_quant_plan(d, nullptr, nullptr, nullptr, false, true);
  if (cp.ok) bytes = std::max(bytes, measured([&](Carve& c) { bwd_cols_layout(c, cp, false, d->inner, d->channels); }));
  return bytes + kWorkspaceSlack;
}

static int fakequant_bwd_impl(const bvq_quant_desc* d, const BwdTensors& T, float* dscale, float* dzp,
                              const void* tie_stat, int64_t* tie_info, void* workspace, int64_t workspace_bytes,
                              bvq_stream_t stream, const LearnedScaleEpilogue* epilogue, const float* bounds = nullptr,
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
  if (!T.g || !T.x || !T.scale || !T.zp || !T.dx) {
    set_error("bvq_fakequant_bwd: null pointer");
    return BVQ_ERR_INVALID;
  }
  if (dbounds && (dzp || tie_stat || !dscale)) {
    set_error("bvq_fakequant_bwd: the bound gradients ride on the dscale variant (dscale set, dzp / tie_stat null)");
    return BVQ_ERR_UNSUPPORTED;
  }
  Carve ws(workspace);
  BwdWs w = {};
  const auto short_of = [&](bool carved) {
    if (!carved || ws.fits(workspace_bytes)) return false;
    set_error("bvq_fakequant_bwd: workspace %lld < %lld bytes", (long long)workspace_bytes, (long long)ws.used);
    return true;
  };
  if (!dzp && !bounds && !act) {
    const ColsPlan cp = cols_quant_plan(d, T.x, T.g, T.dx, !dscale && !tie_stat, true);
    if (cp.ok) {
      if (dscale) w = bwd_cols_layout(ws, cp, false, d->inner, channels);
      if (short_of(dscale != nullptr)) return BVQ_ERR_WORKSPACE;
      rc = launch_bwd_cols(d, cp, T, tie_stat, tie_info, w, st, "bvq_fakequant_bwd/cols");
      if (rc || !dscale) return rc;
      launch_channel_sums(fold_cols_sums(cp, w, st), nullptr, dscale, nullptr, 1, channels, d->inner, w.mid, st, epilogue);
      return check_launch("bvq_fakequant_bwd/cols_sum");
    }
  }
  const BwdRowPlan p = bwd_row_plan(d, T.x, T.g, T.dx);
  if (need_sums) w = bwd_sums_layout(ws, p.t, dbounds != nullptr);
  if (short_of(need_sums)) return BVQ_ERR_WORKSPACE;
  QuantArgs a = rows_bwd_args(d, p.t, T, tie_stat, tie_info, w);
  a.bounds = bounds;
  const int mode = dbounds ? kBwdDsBounds : (tie_stat ? kBwdDsTies : (dzp ? kBwdDsDzp : (dscale ? kBwdDs : kBwdDx)));
  rc = launch_bwd_rows(d, a, p, mode, st, "bvq_fakequant_bwd");
  if (rc || !need_sums) return rc;
  // dbounds: [d(qmin) per channel | d(qmax) per channel] (the bounds themselves are scalars: the caller adds the
  // channels up)
  launch_channel_sums(dscale ? w.ds : nullptr, (dzp || dbounds) ? w.dzp : nullptr, dscale, dbounds ? dbounds : dzp,
                      p.t.nob, channels, p.t.ppr, w.mid, st, epilogue);
  if (dbounds)
    launch_channel_sums(w.dq, nullptr, dbounds + channels, nullptr, p.t.nob, channels, p.t.ppr, w.mid, st, nullptr);
  return check_launch("bvq_fakequant_bwd/channel_sum");
}

extern "C" int bvq_fakequant_bwd(const bvq_quant_desc* d, const void* g, const void* x,
                                 const void* scale, const void* zp, void* dx, float* dscale,
                                 float* dzp, const void* tie_stat, int64_t* tie_info, void* workspace,
                                 int64_t workspace_bytes, bvq_stream_t stream) {
  return fakequant_bwd_impl(d, {g, x, scale, zp, dx}, dscale, dzp, tie_stat, tie_info, workspace, workspace_bytes,
                            stream, nullptr);
}

extern "C" int bvq_fakequant_bwd_bounds(const bvq_quant_desc* d, const void* g, const void* x, const void* scale,
                                        const void* zp, const float* bounds, void* dx, float* dscale, float* dbounds,
                                        void* workspace, int64_t workspace_bytes, bvq_stream_t stream) {
  if (!bounds || !dscale) {
    set_error("bvq_fakequant_bwd_bounds: null pointer");
    return BVQ_ERR_INVALID;
  }
  return fakequant_bwd_impl(d, {g, x, scale, zp, dx}, dscale, nullptr, nullptr, nullptr, workspace, workspace_bytes,
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
  return fakequant_bwd_impl(d, {g, x, scale, zp, dx}, dscale, nullptr, nullptr, nullptr, workspace, workspace_bytes,
                            stream, &ep);
}

// The stats-scaled backward covers per-channel scales with a scalar zero-point.  cp: the column-mapped plan where the
// layout goes that way; row-mapped, one workgroup of bwd_stats_finish_kernel per channel walks the channel's units.
static bool bwd_stats_supported(const bvq_quant_desc* d, ColsPlan& cp) {
  if (!(d->scale_per_channel && d->channels > 1) || d->zp_per_channel) return false;
  cp = cols_quant_plan(d, nullptr, nullptr, nullptr, false, true);
  const int full = 16 / dtype_size(d->x_dtype);
  return cp.ok || std::max(bwd_row_plan(d, nullptr, nullptr, nullptr, full).t.units,
                           bwd_row_plan(d, nullptr, nullptr, nullptr, 1).t.units) / d->channels <= 4096;
}

extern "C" int64_t bvq_fakequant_bwd_stats_workspace_bytes(const bvq_quant_desc* d) {
  if (validate(d)) return -1;
  ColsPlan cp;
  if (!bwd_stats_supported(d, cp)) return 0;  // use bvq_fakequant_bwd + bvq_stat_tie_apply_dscale
  if (cp.ok) return measured([&](Carve& c) { bwd_cols_layout(c, cp, true, d->inner, d->channels); }) + kWorkspaceSlack;
  return kWorkspaceSlack + measured_widths(d->x_dtype, [&](Carve& c, int vec) {
           bwd_stats_row_layout(c, bwd_row_plan(d, nullptr, nullptr, nullptr, vec).t);
         });
}

extern "C" int bvq_fakequant_bwd_stats_onepass_supported(const bvq_quant_desc* d) {
  ColsPlan cp;
  if (validate(d) || !bwd_stats_supported(d, cp)) return 0;
  if (cols_quant_plan(d, nullptr, nullptr, nullptr).ok) return 0;  // column-mapped layouts: two launches
  // the one-launch kernel's instantiations (x's alignment, which may still narrow the vector width, is checked at launch)
  const int full = 16 / dtype_size(d->x_dtype);
  return stream_full_rne(full, full, d->round_mode) ? 1 : 0;
}

// dscale and the deposit from finished partials: one workgroup per channel
static int launch_bwd_stats_finish(const bvq_quant_desc* d, const float* ds, const unsigned long long* pos,
                                   float* dscale, const GstatSrc& gs, const BwdTensors& T, int64_t nob, int64_t ppr,
                                   hipStream_t st, const char* what) {
  const int rc = with_dtype(d->x_dtype, [&](auto t) {
    bwd_stats_finish_kernel<typename decltype(t)::type><<<(unsigned)d->channels, kBlock, 0, st>>>(
        ds, pos, dscale, gs, T.x, T.dx, nob, (int32_t)d->channels, ppr, d->inner);
  });
  return rc ? rc : check_launch(what);
}

static int bwd_stats_impl(const bvq_quant_desc* d, const BwdTensors& T, const void* stat, float* dscale,
                          int scale_dtype, double int_threshold, int quot_dtype, void* workspace,
                          int64_t workspace_bytes, uint32_t* arrive, bvq_stream_t stream,
                          const ShardOut* shard = nullptr) {
  int rc = validate(d);
  if (rc) return rc;
  ColsPlan cp;
  if (!bwd_stats_supported(d, cp)) {
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
    if (shard)
      return launch_channel_finish(shard_finish_args(*shard, channels, 0, nullptr, nullptr), st,
                                   "bvq_fakequant_bwd_shard/empty");
    if (dscale) (void)hipMemsetAsync(dscale, 0, sizeof(float) * channels, st);
    return BVQ_OK;
  }
  if (!T.g || !T.x || !T.scale || !T.zp || !stat || !T.dx || !dscale || !workspace) {
    set_error("bvq_fakequant_bwd_stats: null pointer");
    return BVQ_ERR_INVALID;
  }
  const GstatSrc gs = dscale_src(scale_dtype, quot_dtype, int_threshold, d->pre_op);
  Carve ws(workspace);
  if (cp.ok) {
    if (!cols_quant_plan(d, T.x, T.g, T.dx, false, true).ok) {
      set_error("bvq_fakequant_bwd_stats: the column-mapped route needs 16-byte aligned x, g and dx");
      return BVQ_ERR_UNSUPPORTED;
    }
    const BwdWs w = bwd_cols_layout(ws, cp, true, d->inner, channels);
    if (!ws.fits(workspace_bytes)) {
      set_error("bvq_fakequant_bwd_stats: workspace too small");
      return BVQ_ERR_WORKSPACE;
    }
    launch_tie_init(w.pos, cp.L, st);
    rc = launch_bwd_cols(d, cp, T, stat, nullptr, w, st, "bvq_fakequant_bwd_stats/cols");
    if (rc) return rc;
    float* ds_fold = fold_cols_sums(cp, w, st);
    if (shard)  // this shard's message from the folded partials
      return launch_channel_finish(shard_finish_args(*shard, channels, d->inner, ds_fold, w.pos), st,
                                   "bvq_fakequant_bwd_shard/cols_finish");
    return launch_bwd_stats_finish(d, ds_fold, w.pos, dscale, gs, T, 1, d->inner, st,
                                   "bvq_fakequant_bwd_stats/cols_finish");
  }
  const BwdRowPlan p = bwd_row_plan(d, T.x, T.g, T.dx);
  const BwdWs w = bwd_stats_row_layout(ws, p.t);
  if (!ws.fits(workspace_bytes)) {
    set_error("bvq_fakequant_bwd_stats: workspace too small");
    return BVQ_ERR_WORKSPACE;
  }
  QuantArgs a = rows_bwd_args(d, p.t, T, stat, nullptr, w, shard);
  // two launches for the rare forms
  if (arrive && !stream_full_rne(p.vec, 16 / dtype_size(d->x_dtype), d->round_mode)) arrive = nullptr;
  if (arrive) {  // one launch: the wave that completes a channel finishes it
    a.arrive = arrive;
    a.dscale_out = dscale;
    a.gs_scale_dtype = scale_dtype;
    a.gs_quot_dtype = quot_dtype;
    a.gs_int_threshold = (float)int_threshold;
    return launch_bwd_rows(d, a, p, kBwdDsArrive, st, "bvq_fakequant_bwd_stats_onepass");
  }
  rc = launch_bwd_rows(d, a, p, kBwdDsTies, st, "bvq_fakequant_bwd_stats");
  if (rc) return rc;
  if (shard) return launch_channel_finish(a, st, "bvq_fakequant_bwd_shard/finish");
  return launch_bwd_stats_finish(d, w.ds, w.pos, dscale, gs, T, p.t.nob, p.t.ppr, st,
                                 "bvq_fakequant_bwd_stats/finish");
}

extern "C" int bvq_fakequant_bwd_stats(const bvq_quant_desc* d, const void* g, const void* x, const void* scale,
                                       const void* zp, const void* stat, void* dx, float* dscale,
                                       int scale_dtype, double int_threshold, int quot_dtype, void* workspace,
                                       int64_t workspace_bytes, bvq_stream_t stream) {
  return bwd_stats_impl(d, {g, x, scale, zp, dx}, stat, dscale, scale_dtype, int_threshold, quot_dtype, workspace,
                        workspace_bytes, nullptr, stream);
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
  return bwd_stats_impl(d, {g, x, scale, zp, dx}, stat, dscale, scale_dtype, int_threshold, quot_dtype, workspace,
                        workspace_bytes, arrive, stream);
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
  const ShardOut so = {message, reinterpret_cast<long long*>(first_pos), rank};
  float unused = 0.f;
  return bwd_stats_impl(d, {g, x, scale, zp, dx}, stat, &unused, BVQ_F32, 1.0, BVQ_F32, workspace, workspace_bytes,
                        arrive, stream, &so);
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
  if (const int prc = check_pre_op(pre_op, "bvq_shard_unpack_deposit")) return prc;
  const GstatSrc gs = dscale_src(scale_dtype, quot_dtype, int_threshold, pre_op);
  const dim3 grid((unsigned)((channels + 255) / 256)), block(256);
  hipStream_t st = (hipStream_t)stream;
  const long long* fp = reinterpret_cast<const long long*>(first_pos);
  const int rc = with_dtype(dtype, [&](auto t) {
    shard_unpack_deposit_kernel<typename decltype(t)::type><<<grid, block, 0, st>>>(gathered, world, (int32_t)channels,
                                                                                    rank, fp, x, dx, inner, gs, dscale_total);
  });
  return rc ? rc : check_launch("bvq_shard_unpack_deposit");
}
