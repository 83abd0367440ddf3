// bvq_weight_list.hip -- many per-output-channel weights, each with its own statistic, scale and integer range, in one
// launch each way (include/bvq.h, bvq_weight_quant_list_fwd / _bwd).  The forward is the register-resident statistic +
// quantizer of bvq_fakequant_fwd.hip dealt over the (tensor, channel) pairs of the list (fused_list_fwd).  The backward
// below is the one-launch stats-scaled backward (kBwdDsArrive, bvq_fakequant_bwd.h) dealt over the units of all tensors:
// every tensor keeps the tiling, the vector width, the partials and the combine order of its own
// bvq_fakequant_bwd_stats_onepass call, so dx and dscale are the same bits.
#include "bvq_fakequant_bwd.h"

namespace bvq {

// what one tensor's waves need besides the per-call fields
struct WeightBwdItem {
  Tiling t;
  const void* x;
  const void* g;
  const void* scale;
  const void* stat;
  void* dx;
  float* ds_part;                // [units] of this tensor (workspace)
  unsigned long long* pos_part;  // [units] of this tensor (workspace)
  uint32_t* arrive;              // this tensor's segment of the arrival buffer
  float* dscale;                 // [channels]
  float qmin, qmax, int_threshold;
  int32_t clamp_ste;
};

struct WeightBwdListArgs {
  WeightBwdItem it[BVQ_WEIGHT_LIST_MAX];
  int64_t start[BVQ_WEIGHT_LIST_MAX + 1];  // first dispatch slot of tensor i; start[n] = all slots
  int32_t n, scale_dtype, quot_dtype;
};
static_assert(sizeof(WeightBwdListArgs) <= 4096, "kernel arguments are limited to 4 KiB");

template <typename T, bool NT>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(BVQ_BWD_WAVES, 8))) void weight_list_bwd_kernel(
    WeightBwdListArgs la) {
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t slot = (int64_t)blockIdx.x * kWavesPerBlock + wave;
  if (slot >= la.start[la.n]) return;
  int p = 0;
  while (p + 1 < la.n && slot >= la.start[p + 1]) ++p;  // (wave-uniform)
  const WeightBwdItem& it = la.it[p];
  // the arguments of this tensor's own one-launch call (bwd_stats_impl)
  QuantArgs a = {};
  a.t = it.t;
  a.x = it.x;
  a.g = it.g;
  a.y = it.dx;
  a.scale = it.scale;
  a.tie_stat = it.stat;
  a.ds_part = it.ds_part;
  a.pos_part = it.pos_part;
  a.qmin = it.qmin;
  a.qmax = it.qmax;
  a.scale_dtype = la.scale_dtype;
  a.scale_pc = 1;
  a.clamp_ste = it.clamp_ste;
  a.round_mode = BVQ_ROUND;
  a.arrive = it.arrive;
  a.arrive_per_channel = (uint32_t)(it.t.nob * it.t.ppr);
  a.dscale_out = it.dscale;
  a.gs_scale_dtype = la.scale_dtype;
  a.gs_quot_dtype = la.quot_dtype;
  a.gs_int_threshold = it.int_threshold;
  const Unit u = locate_unit_slot(a.t, slot - la.start[p]);  // valid: start[] holds the tilings' own unit counts
  const float s = load_scalar_as_f(a.scale, a.scale_dtype, u.channel);
  bwd_unit_scaled<T, T, elem<T>::vec, BVQ_ROUND, kBwdDsArrive, NT>(a, u, s, 0.f);  // zero zero-point: +0
}

}  // namespace bvq

using namespace bvq;

// the descriptor of item `it`'s own single-tensor calls
static bvq_quant_desc item_desc(int dtype, int scale_dtype, int round_mode, const bvq_weight_item& it) {
  bvq_quant_desc d = {};
  d.outer = 1;
  d.channels = it.channels;
  d.inner = it.inner;
  d.x_dtype = d.ct_dtype = dtype;
  d.scale_dtype = scale_dtype;
  d.zp_dtype = BVQ_F32;
  d.scale_per_channel = 1;
  d.qmin = it.qmin;
  d.qmax = it.qmax;
  d.round_mode = round_mode;
  d.scalar_mode = BVQ_SCALAR_OPMATH;
  d.clamp_ste = it.clamp_ste;
  d.out_kind = BVQ_OUT_DEQUANT;
  d.pre_op = BVQ_PRE_NONE;
  return d;
}

// the checks that need no device; what: the entry's name.  fwd / bwd: the pointers that entry reads or writes.
static int check_list(const char* what, int dtype, int n, const bvq_weight_item* items, bool fwd, bool bwd) {
  if (!items || n < 1 || n > BVQ_WEIGHT_LIST_MAX) {
    set_error("%s: need 1..%d items, got %d%s", what, BVQ_WEIGHT_LIST_MAX, n, items ? "" : " (null)");
    return BVQ_ERR_INVALID;
  }
  if (bad_dtype(dtype)) {
    set_error("%s: bad dtype %d", what, dtype);
    return BVQ_ERR_INVALID;
  }
  for (int i = 0; i < n; ++i) {
    const bvq_weight_item& it = items[i];
    if (it.channels < 1 || it.inner < 1) {
      set_error("%s: item %d has shape [%lld, %lld]", what, i, (long long)it.channels, (long long)it.inner);
      return BVQ_ERR_INVALID;
    }
    const bool null_fwd = fwd && (!it.y || !it.stat || !it.scale);
    const bool null_bwd = bwd && (!it.g || !it.dx || !it.dscale || !it.stat || !it.scale);
    if (!it.x || null_fwd || null_bwd) {
      set_error("%s: item %d: null pointer", what, i);
      return BVQ_ERR_INVALID;
    }
  }
  return BVQ_OK;
}

// item covered by both one-launch forms (the pointers that are set are checked for alignment)
static bool item_covered(const bvq_quant_desc& d, const bvq_weight_item& it) {
  if (d.channels < 2 || bvq_stats_fakequant_fwd_workspace_bytes(&d, it.x, it.y) <= 0) return false;
  if (!bvq_fakequant_bwd_stats_onepass_supported(&d)) return false;
  return ((reinterpret_cast<uintptr_t>(it.g) | reinterpret_cast<uintptr_t>(it.dx)) & 15) == 0;
}

static int64_t list_channels(int n, const bvq_weight_item* items) {
  int64_t c = 0;
  for (int i = 0; i < n; ++i) c += items[i].channels;
  return c;
}

extern "C" int bvq_weight_list_supported(int dtype, int round_mode, int n, const bvq_weight_item* items,
                                         int64_t arrive_words) {
  if (check_list("bvq_weight_list_supported", dtype, n, items, false, false)) return 0;
  for (int i = 0; i < n; ++i) {
    const bvq_quant_desc d = item_desc(dtype, dtype, round_mode, items[i]);
    if (!item_covered(d, items[i])) return 0;
  }
  return arrive_words == 0 || list_channels(n, items) <= arrive_words ? 1 : 0;
}

extern "C" int bvq_weight_quant_list_fwd(int dtype, int scale_dtype, int round_mode, int n, const bvq_weight_item* items,
                                         bvq_stream_t stream) {
  int rc = check_list("bvq_weight_quant_list_fwd", dtype, n, items, true, false);
  if (rc) return rc;
  if (bad_dtype(scale_dtype)) {
    set_error("bvq_weight_quant_list_fwd: bad scale dtype %d", scale_dtype);
    return BVQ_ERR_INVALID;
  }
  bvq_quant_desc descs[BVQ_WEIGHT_LIST_MAX];
  for (int i = 0; i < n; ++i) {
    descs[i] = item_desc(dtype, scale_dtype, round_mode, items[i]);
    if (!item_covered(descs[i], items[i])) {
      set_error("bvq_weight_quant_list_fwd: item %d not covered", i);
      return BVQ_ERR_UNSUPPORTED;
    }
  }
  return fused_list_fwd(n, descs, items, (hipStream_t)stream);
}

extern "C" int64_t bvq_weight_quant_list_bwd_workspace_bytes(int dtype, int n, const bvq_weight_item* items) {
  if (check_list("bvq_weight_quant_list_bwd_workspace_bytes", dtype, n, items, false, false)) return -1;
  // every item's partials as its own stats-scaled backward lays them out (full width: the list takes no other item)
  return kWorkspaceSlack + measured([&](Carve& c) {
           for (int i = 0; i < n; ++i) {
             const bvq_quant_desc d = item_desc(dtype, dtype, BVQ_ROUND, items[i]);
             bwd_stats_row_layout(c, bwd_row_plan(&d, nullptr, nullptr, nullptr, 16 / dtype_size(dtype)).t);
           }
         });
}

extern "C" int bvq_weight_quant_list_bwd(int dtype, int scale_dtype, int quot_dtype, int round_mode, int n,
                                         const bvq_weight_item* items, void* workspace, int64_t workspace_bytes,
                                         uint32_t* arrive, int64_t arrive_words, bvq_stream_t stream) {
  int rc = check_list("bvq_weight_quant_list_bwd", dtype, n, items, false, true);
  if (rc) return rc;
  if (bad_dtype(scale_dtype) || bad_dtype(quot_dtype) || !workspace || !arrive) {
    set_error("bvq_weight_quant_list_bwd: bad argument");
    return BVQ_ERR_INVALID;
  }
  if (list_channels(n, items) > arrive_words) {
    set_error("bvq_weight_quant_list_bwd: arrival buffer of %lld words, %lld needed", (long long)arrive_words,
              (long long)list_channels(n, items));
    return BVQ_ERR_WORKSPACE;
  }
  const int full = 16 / dtype_size(dtype);
  WeightBwdListArgs la = {};
  Carve ws(workspace);
  la.n = n;
  la.scale_dtype = scale_dtype;
  la.quot_dtype = quot_dtype;
  int64_t slots = 0, chan = 0, bytes = 0;
  for (int i = 0; i < n; ++i) {
    const bvq_weight_item& src = items[i];
    const bvq_quant_desc d = item_desc(dtype, scale_dtype, round_mode, src);
    if (!item_covered(d, src)) {
      set_error("bvq_weight_quant_list_bwd: item %d not covered", i);
      return BVQ_ERR_UNSUPPORTED;
    }
    // the plan of the single-tensor call (full width: covered rows are whole, aligned 16-byte chunks)
    const BwdRowPlan p = bwd_row_plan(&d, src.x, src.g, src.dx);
    if (!stream_full_rne(p.vec, full, round_mode)) {
      set_error("bvq_weight_quant_list_bwd: item %d has no one-launch kernel", i);
      return BVQ_ERR_UNSUPPORTED;
    }
    WeightBwdItem& it = la.it[i];
    it.t = p.t;
    const BwdWs w = bwd_stats_row_layout(ws, it.t);
    it.ds_part = w.ds;
    it.pos_part = w.pos;
    it.x = src.x;
    it.g = src.g;
    it.scale = src.scale;
    it.stat = src.stat;
    it.dx = src.dx;
    it.arrive = arrive + chan;
    it.dscale = src.dscale;
    it.qmin = src.qmin;
    it.qmax = src.qmax;
    it.int_threshold = (float)src.int_threshold;
    it.clamp_ste = src.clamp_ste;
    la.start[i] = slots;
    slots += it.t.units;
    chan += d.channels;
    bytes += d.channels * d.inner * (int64_t)(3 * dtype_size(dtype));
  }
  la.start[n] = slots;
  if (!ws.fits(workspace_bytes)) {
    set_error("bvq_weight_quant_list_bwd: workspace %lld < %lld bytes", (long long)workspace_bytes, (long long)ws.used);
    return BVQ_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  const bool nt = bytes >= nt_threshold_bytes();  // (the cache policy changes no value)
  rc = with_dtype(dtype, [&](auto t) {
    return with_bool(nt, [&](auto ntc) {
      weight_list_bwd_kernel<typename decltype(t)::type, ntc><<<grid_for_units(slots), kBlock, 0, st>>>(la);
    });
  });
  return rc ? rc : check_launch("bvq_weight_quant_list_bwd");
}
