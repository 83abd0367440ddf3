/*
 * bvq.h -- C ABI of libbvq.so, the MI355X (gfx950) fake-quantization engine.
 *
 * This is the drop-in boundary for Brevitas' per-tensor / per-channel integer
 * quant-dequant hot path.  Nothing like it exists in the reference (it has no
 * native kernels besides 12 ATen-forwarding STE ops); every entry point below
 * names the reference interface whose tensor math it replaces.  Paths are
 * relative to the reference checkout, `B/` = `src/brevitas/`.
 *
 * Conventions
 *   - plain C, no torch types: raw device pointers, int64 sizes, a hipStream_t
 *     passed as void*.  The library owns no memory across calls: every output
 *     and every workspace is allocated by the caller (B/ ownership model: each
 *     op returns a fresh tensor from the host framework's allocator).
 *   - all pointers are DEVICE pointers unless the name says `host`.
 *   - every function is re-entrant, never synchronises the device, never
 *     allocates, and only enqueues work on `stream` (autograd runs backward on
 *     its own thread: B/ has no threads of its own, SURVEY 8b "Threading").
 *   - return 0 on success, a negative bvq_status otherwise; the message for the
 *     calling thread's last failure is bvq_last_error().  Never throws.
 *   - a tensor is described as [outer, channels, inner] (row-major,
 *     contiguous).  channels == 1 means per-tensor.  A weight [Cout,Cin,kh,kw]
 *     quantized per output channel is (1, Cout, Cin*kh*kw); an NCHW activation
 *     quantized per channel is (N, C, H*W) -- no permute copy is ever made
 *     (the reference does permute().contiguous(), B/core/function_wrapper/shape.py:19-27).
 */
#ifndef BVQ_H_
#define BVQ_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BVQ_ABI_VERSION 12

typedef void* bvq_stream_t; /* hipStream_t */

typedef enum bvq_status {
  BVQ_OK = 0,
  BVQ_ERR_INVALID = -1,     /* bad argument (null pointer, negative size, bad enum) */
  BVQ_ERR_UNSUPPORTED = -2, /* dtype / layout combination not built */
  BVQ_ERR_WORKSPACE = -3,   /* workspace too small */
  BVQ_ERR_LAUNCH = -4       /* HIP reported a launch error */
} bvq_status;

/* element types of tensors ("dtype" is the storage/arithmetic type, not a precision claim) */
typedef enum bvq_dtype { BVQ_F32 = 0, BVQ_BF16 = 1, BVQ_F16 = 2 } bvq_dtype;

/* float_to_int_impl variants: B/core/function_wrapper/ops_ste.py:14-76 */
typedef enum bvq_round_mode {
  BVQ_ROUND = 0,         /* torch.round, half to even  (round_ste,  B/function/ops_ste.py:46-67)  */
  BVQ_FLOOR = 1,         /* torch.floor                (floor_ste,  :94-115)                      */
  BVQ_CEIL = 2,          /* torch.ceil                 (ceil_ste,   :70-91)                       */
  BVQ_ROUND_TO_ZERO = 3, /* sign(x)*floor(|x|)         (B/function/ops.py:37-53)                  */
  BVQ_DPU_ROUND = 4      /* DPU rounding               (B/function/ops.py:56-72)                  */
} bvq_round_mode;

/* elementwise ops of the STE namespace, forward math only
 * (B/ops/autograd_ste_ops.py:37-382, B/csrc/autograd_ste_ops.cpp:14-194) */
typedef enum bvq_unary_op {
  BVQ_OP_ROUND = 0,
  BVQ_OP_FLOOR = 1,
  BVQ_OP_CEIL = 2,
  BVQ_OP_ROUND_TO_ZERO = 3,
  BVQ_OP_DPU_ROUND = 4,
  BVQ_OP_BINARY_SIGN = 5,  /* (x>=0) - (x<0), +1 at 0   (B/function/ops.py:16-34) */
  BVQ_OP_TERNARY_SIGN = 6, /* torch.sign                                          */
  BVQ_OP_ABS = 7           /* torch.abs (forward of abs_binary_sign_grad)         */
} bvq_unary_op;

typedef enum bvq_stat_kind {
  BVQ_STAT_ABSMAX = 0, /* out[c]      = max |x|              (AbsMax,    B/core/stats/stats_op.py:129-141) */
  BVQ_STAT_MINMAX = 1  /* out[c]=max, out[channels+c]=min    (AbsMinMax, B/core/stats/stats_op.py:144-158) */
} bvq_stat_kind;

/* How a 0-dim (one element) scale / zero-point whose dtype is WIDER than the
 * compute dtype enters the arithmetic.  torch's own kernels differ here:
 *   OPMATH: the scalar keeps its float32 value (ATen CPU reduced-float scalar path);
 *   CAST  : the scalar is first rounded to the compute dtype (ATen device kernels).
 * Same-dtype operands and per-channel operands are unaffected. */
typedef enum bvq_scalar_mode { BVQ_SCALAR_OPMATH = 0, BVQ_SCALAR_CAST = 1 } bvq_scalar_mode;

/* Elementwise activation applied to x BEFORE the statistic / the quantizer, fused into the same
 * kernels: FusedActivationQuantProxy.forward = tensor_quant(activation_impl(x))
 * (B/proxy/runtime_quant.py:73-84).  RELU: torch.relu forward (NaN and -0.0 pass), backward
 * grad * (x > 0) (threshold_backward).  SIGMOID / TANH: torch.sigmoid / torch.tanh in float opmath, rounded to
 * x's dtype; backward sigmoid_backward / tanh_backward with torch's rounding (brevitas_amd/csrc/bvq_act.h).
 * SIGMOID and TANH are covered, with x and the compute dtype alike, by bvq_fakequant_fwd (dequantized output),
 * bvq_fakequant_bwd (dx and dscale), bvq_fakequant_bwd_learned, and the row-mapped abs-max / min-max statistic of
 * bvq_stats_pre, bvq_absmax_scale and bvq_absmax_scale_running; every other entry fails with BVQ_ERR_UNSUPPORTED on
 * them. */
typedef enum bvq_pre_op { BVQ_PRE_NONE = 0, BVQ_PRE_RELU = 1, BVQ_PRE_SIGMOID = 2, BVQ_PRE_TANH = 3 } bvq_pre_op;

/* element type of the integer codes bvq_fakequant_fwd can emit: what QuantTensor.int() returns
 * (B/quant_tensor/__init__.py:174-187: int8 / uint8 up to 8 bits, int32 above) and what the QCDQ export
 * handlers quantize to (B/export/common/handler/qcdq.py:71-84) */
typedef enum bvq_codes_dtype { BVQ_CODES_I32 = 0, BVQ_CODES_I8 = 1, BVQ_CODES_U8 = 2 } bvq_codes_dtype;

/* output selection for bvq_fakequant_fwd */
#define BVQ_OUT_DEQUANT 0 /* y = (clamp(round(x/s+zp)) - zp) * s   IntQuant.forward, B/core/quant/int_base.py:86-97 */
#define BVQ_OUT_INT 1     /* y =  clamp(round(x/s+zp))             IntQuant.to_int,  B/core/quant/int_base.py:63-76 */

/*
 * Descriptor of one affine integer quantizer application.
 * Replaces the argument set of IntQuant.forward(scale, zero_point, bit_width, x)
 * (B/core/quant/int_base.py:86-97): bit_width only enters through
 * qmin = min_int(signed, narrow_range, bit_width), qmax = max_int(...)
 * (B/function/ops.py:132-191), computed on the host.
 */
typedef struct bvq_quant_desc {
  int64_t outer;    /* x viewed as [outer, channels, inner], contiguous */
  int64_t channels; /* 1 = per-tensor */
  int64_t inner;
  int32_t x_dtype;     /* dtype of x and of dx */
  int32_t ct_dtype;    /* torch.result_type(x, scale): dtype of every intermediate, of y and of g */
  int32_t scale_dtype; /* dtype of the scale buffer */
  int32_t zp_dtype;    /* dtype of the zero-point buffer */
  int32_t scale_per_channel; /* 0: one element, 1: `channels` elements */
  int32_t zp_per_channel;    /* 0: one element, 1: `channels` elements */
  float qmin;          /* integer clamp bounds, as floats (the reference keeps them as 0-dim float tensors) */
  float qmax;
  int32_t round_mode;  /* bvq_round_mode */
  int32_t scalar_mode; /* bvq_scalar_mode */
  int32_t clamp_ste;   /* backward only. 1: TensorClampSte (grad passes clipped elements, weights);
                          0: TensorClamp (grad masked where clipped, activations). B/core/quant/int_base.py:53-54 */
  int32_t out_kind;    /* forward only. BVQ_OUT_DEQUANT or BVQ_OUT_INT */
  int32_t pre_op;      /* bvq_pre_op applied to x first (forward and backward) */
  int32_t codes_dtype; /* forward only: element type of the optional integer-code output (bvq_codes_dtype) */
} bvq_quant_desc;

/* ---- library ------------------------------------------------------------------------------ */

int bvq_abi_version(void);
/* message of the calling thread's last failing call ("" if none) */
const char* bvq_last_error(void);
/* bytes of traffic from which an entry point launches the non-temporal variant of its kernels (the cache policy changes
 * no value): 256 MiB in the shipped library, 0 in the forced-NT build the tests load (csrc/build.py, build_nt0) */
int64_t bvq_nt_threshold_bytes(void);

/* ---- elementwise STE namespace (seam 1) ----------------------------------------------------
 * Forward math of torch.ops.autograd_ste_ops.<name>_impl / brevitas.ops.autograd_ste_ops.<name>_impl
 * (registration B/csrc/autograd_ste_ops.cpp:258-271, aliases B/ops/autograd_ste_ops.py:385-431).
 * The straight-through backward of these ops is the identity and needs no kernel. */

/* y[i] = op(x[i]).  x may alias y (tensor_clamp_ste_-style in-place use). */
int bvq_unary(int op, int dtype, const void* x, void* y, int64_t n, bvq_stream_t stream);

/* torch.clamp(x, lo, hi) / torch.clamp_min(x, lo): scalar_clamp_ste_impl, scalar_clamp_min_ste_impl
 * (B/ops/autograd_ste_ops.py:37-97).  Bounds are host doubles rounded to `dtype` like torch does.
 * use_lo / use_hi select which bounds apply.  NaN propagates. */
int bvq_scalar_clamp(int dtype, const void* x, void* y, int64_t n, double lo, int use_lo, double hi,
                     int use_hi, bvq_stream_t stream);

/* tensor_clamp(x, min_val, max_val) = where(x>max,max,x) then where(out<min,min,out)
 * (B/function/ops.py:75-100; tensor_clamp_ste_impl forward, B/ops/autograd_ste_ops.py:100-128).
 * lo / hi are device buffers of dtype `dtype`: one element each when bounds_full == 0
 * (the hot path: 0-dim min_int/max_int), n elements each when bounds_full == 1. */
int bvq_tensor_clamp(int dtype, const void* x, const void* lo, const void* hi, int bounds_full, void* y,
                     int64_t n, bvq_stream_t stream);

/* backward of the non-STE tensor_clamp w.r.t. x (autograd of the two torch.where):
 * dx = (!(x>hi) && !(x<lo)) ? g : 0 */
int bvq_tensor_clamp_bwd(int dtype, const void* g, const void* x, const void* lo, const void* hi,
                         int bounds_full, void* dx, int64_t n, bvq_stream_t stream);

/* backward of abs_binary_sign_grad (B/ops/autograd_ste_ops.py:356-382): dx = binary_sign(x) * g */
int bvq_abs_binary_sign_grad_bwd(int dtype, const void* g, const void* x, void* dx, int64_t n,
                                 bvq_stream_t stream);

/* ---- statistics (seam 2: AbsMax / AbsMinMax) ------------------------------------------------ */

/* Bytes of workspace that bvq_stats, bvq_stats_pre, bvq_absmax_scale[_running] (kind BVQ_STAT_ABSMAX) and bvq_stat_bwd
 * need for this problem: the largest of their routes' layouts, measured, plus a few bytes for a buffer that starts on
 * no boundary.  BVQ_STAT_ABSMAX needs about half of BVQ_STAT_MINMAX (one key per partial, not two).  -1: bad argument. */
int64_t bvq_stats_workspace_bytes(int kind, int dtype, int64_t outer, int64_t channels, int64_t inner);

/* Per-channel (or whole-tensor, channels == 1) statistic over the `outer` and `inner` axes of
 * x[outer, channels, inner].  One streaming read of x, no permuted copy.
 *   ABSMAX: out[c] = max |x|, NaN if any NaN (torch.max semantics)       -> `channels` elements
 *   MINMAX: out[c] = max x ; out[channels + c] = min x, NaN-propagating  -> 2*`channels` elements
 * out has dtype out_dtype: BVQ_F32 or the dtype of x (the values are exact in either). */
int bvq_stats(int kind, int dtype, const void* x, int64_t outer, int64_t channels, int64_t inner,
              int out_dtype, void* out, void* workspace, int64_t workspace_bytes, bvq_stream_t stream);

/* the same statistic of pre_op(x) (bvq_pre_op), without materialising the activation */
int bvq_stats_pre(int kind, int pre_op, int dtype, const void* x, int64_t outer, int64_t channels,
                  int64_t inner, int out_dtype, void* out, void* workspace, int64_t workspace_bytes,
                  bvq_stream_t stream);

/* bvq_stats(ABSMAX) with the scale derivation of a stats-scaled quantizer in the same launches:
 *   stat_out[c]  = max |x|                                        (dtype of x)
 *   thr          = use_min ? clamp_min(stat, min_val) : stat      (scalar_clamp_min_ste, B/core/restrict_val.py:22-42;
 *                                                                  min_val is rounded to the dtype of x like torch does)
 *   scale_out[c] = thr / int_threshold, rounded to scale_dtype    (RescalingIntQuant.forward, B/core/quant/int.py:160)
 * int_threshold is the value the division sees (the caller applies torch's promotion of the 0-dim
 * int_threshold tensor); scale_dtype is the dtype torch gives the quotient.  pre_op: the statistic is
 * taken of pre_op(x) (bvq_pre_op). */
int bvq_absmax_scale(int pre_op, int dtype, const void* x, int64_t outer, int64_t channels, int64_t inner,
                     void* stat_out, double min_val, int use_min, double int_threshold, int scale_dtype,
                     void* scale_out, void* workspace, int64_t workspace_bytes, bvq_stream_t stream);
/* bvq_absmax_scale whose finishing launch ALSO folds the statistic into _RuntimeStats' running average
 * (B/core/stats/stats_wrapper.py:61-66): first_batch: running *= stat; else running *= (1 - momentum);
 * running += momentum * stat -- the rounding points of bvq_running_stats_update, one launch fewer per step.
 * running: [channels] in run_dtype, updated in place. */
int bvq_absmax_scale_running(int pre_op, int dtype, const void* x, int64_t outer, int64_t channels, int64_t inner,
                             void* stat_out, double min_val, int use_min, double int_threshold, int scale_dtype,
                             void* scale_out, int run_dtype, void* running, double momentum, int first_batch,
                             void* workspace, int64_t workspace_bytes, bvq_stream_t stream);

/* The same statistic (+ optional scale epilogue, + optional running average) in ONE launch, for per-channel
 * layouts whose rows the row-mapped kernels walk (bvq_absmax_onepass_supported: 1 / 0).  Persistent waves fold their
 * maxima into a per-channel key word with an atomic max and count the units they covered in a per-channel counter;
 * the wave whose count completes a channel finishes it (B/core/stats/stats_op.py:129-141 -> stat_out;
 * B/core/restrict_val.py:22-42 and B/core/quant/int.py:160 -> scale_out; B/core/stats/stats_wrapper.py:61-66 ->
 * running).  No wave waits for another.  Results are the bits of bvq_absmax_scale[_running] (a max is exact).
 * stat_dtype: BVQ_F32 (the batch-sharded route all-reduces it) or the dtype of x.  scale_out / running: nullable.
 * Not covered (bvq_absmax_onepass_supported: 0): a whole-tensor statistic and per-channel layouts with more than 32
 * units per channel -- arrivals at one word serialise (~0.25 us each) and soon cost more than the finishing launch
 * they would save.
 * arrive: `arrive_words` >= 2 * channels uint32 words in device memory that are ALL ZERO when the launch starts;
 *   the finishing waves hand them back as zeros, so a caller keeps ONE such buffer per stream, cleared once when
 *   it is allocated, and never clears it again (launches on one stream are ordered; do not share it between streams).
 * BVQ_ERR_UNSUPPORTED: layout not covered (per-tensor, column-mapped): call bvq_absmax_scale[_running]. */
int bvq_absmax_onepass_supported(int dtype, const void* x, int64_t outer, int64_t channels, int64_t inner);
int bvq_absmax_scale_onepass(int pre_op, int dtype, const void* x, int64_t outer, int64_t channels, int64_t inner,
                             int stat_dtype, void* stat_out, double min_val, int use_min, double int_threshold,
                             int scale_dtype, void* scale_out, int run_dtype, void* running, double momentum,
                             int first_batch, uint32_t* arrive, int64_t arrive_words, bvq_stream_t stream);

/* AbsMax of a LIST of tensors that share the channel axis, + the scale epilogue, in ONE launch: the statistic of
 * _ParameterListStats with several tracked parameters (B/core/stats/stats_wrapper.py:83-114 -- a weight quantizer shared
 * by several layers reduces torch.cat of their weights' views; B/core/scaling/standalone.py StatsFromParameterScaling).
 * Tensor i is contiguous [outers[i], channels, inners[i]] of `dtype` (per output channel: outers = 1, inners = the
 * row of channel c; whole tensor: channels = 1, inners = numel).  No concatenation is materialised: the launch's waves
 * are dealt to the tensors, and the last wave to arrive at a channel's words finishes that channel (contract of the
 * arrival buffer: bvq_absmax_scale_onepass).  stat_out [channels] in `dtype`; scale_out nullable.  The bits are those
 * of the reference's reduction over the concatenation (a max is exact).
 * A whole-tensor statistic (channels = 1) leaves one partial per unit in `workspace` (>= 16 KiB) and takes a second,
 * finishing launch instead of the arrivals: every unit of every tensor would arrive at ONE pair of words, and
 * agent-scope atomics on one address serialise.  `arrive` may be null then; `workspace` may be null for channels > 1.
 * bvq_absmax_list_supported: 1 / 0 -- 1..8 tensors, at most 32 units per channel over the whole list.
 * BVQ_ERR_UNSUPPORTED otherwise: reduce the tensors one by one. */
int bvq_absmax_list_supported(int dtype, int n, const void* const* xs, const int64_t* outers, int64_t channels,
                              const int64_t* inners);
int bvq_absmax_scale_list(int dtype, int n, const void* const* xs, const int64_t* outers, int64_t channels,
                          const int64_t* inners, void* stat_out, double min_val, int use_min, double int_threshold,
                          int scale_dtype, void* scale_out, uint32_t* arrive, int64_t arrive_words,
                          void* workspace, int64_t workspace_bytes, bvq_stream_t stream);

/* Running average kept by _RuntimeStats (B/core/stats/stats_wrapper.py:61-66), one launch:
 *   first_batch: running *= stat ; otherwise running *= (1 - momentum); running += momentum * stat
 * with torch's rounding points (in-place results in run_dtype, momentum * stat in stat_dtype). */
int bvq_running_stats_update(int run_dtype, void* running, int stat_dtype, const void* stat, int64_t n,
                             double momentum, int first_batch, bvq_stream_t stream);

/* ---- batch-sharded tensors (one process per GPU, the activation split along the batch) ----------------
 * The two collectives of brevitas_amd/distributed.py carry small messages; these entry points build and consume
 * them in one launch each instead of a dozen scale-shaped torch ops.
 * bvq_scale_from_stat: the all-reduced (MAX) float32 statistic -> statistic in `stat_dtype` and
 *   scale = clamp_min(stat, min_val) / int_threshold in `scale_dtype` (rounding points of bvq_absmax_scale).
 * bvq_shard_pack: this shard's float64 [2][channels] message for the backward all-gather: its dscale sums and,
 *   per channel, `rank` if it holds an element attaining the statistic (tie_info[c] >= 0) else 2^30
 *   (per_channel = 0: the number of ties it holds, tie_info[0]).
 * bvq_shard_unpack: from the gathered [world][2][channels] messages: dscale_total (double sum in rank order:
 *   the same bits on every rank) and, per_channel, tie_info[c] = -1 for every channel whose lowest claiming rank
 *   is another shard; per_channel = 0: total_ties[0] = ties over all shards. */
int bvq_scale_from_stat(const float* stat32, int64_t channels, int stat_dtype, void* stat_out, double min_val,
                        int use_min, double int_threshold, int scale_dtype, void* scale_out, bvq_stream_t stream);
/* bvq_scale_from_stat with _RuntimeStats' running average folded in (the rounding points of bvq_absmax_scale_running);
 * running: nullable. */
int bvq_scale_from_stat_running(const float* stat32, int64_t channels, int stat_dtype, void* stat_out, double min_val,
                                int use_min, double int_threshold, int scale_dtype, void* scale_out, int run_dtype,
                                void* running, double momentum, int first_batch, bvq_stream_t stream);
/* The stats-scaled backward of ONE BATCH SHARD (per-channel layouts of bvq_fakequant_bwd_stats): dx WITHOUT the deposit,
 * and this shard's message for the backward all-gather, float64 [2][channels]: row 0 = the channel's dscale sum kept
 * in double (the shards' sums are added in double and rounded to float32 once: bvq_shard_unpack_deposit), row 1 = its
 * claim on the channel's deposit (`rank`, or 2^30 when no element of the shard attains the statistic); first_pos[c] =
 * the shard's first arg-max position (outer * inner + i; -1: none).  arrive (nullable): the arrival buffer of
 * bvq_fakequant_bwd_stats_onepass -- the streaming kernel's last-arriving wave per channel then writes the message
 * (one launch); without it, or on column-mapped layouts, a one-wave-per-channel launch follows the streaming kernel.
 * workspace: bvq_fakequant_bwd_stats_workspace_bytes.
 * An EMPTY shard (outer = 0) is legal and claims nothing: message[c] = 0.0, message[channels + c] = 2^30 and
 * first_pos[c] = -1 for every channel, written by one small launch; g, x, dx and the workspace are not touched and may
 * be null.  bvq_shard_unpack_deposit takes such a shard's x and dx as two null pointers: it owns no deposit.  (Two null
 * pointers skip the deposit on ANY rank, the owning one included, and still return BVQ_OK: pass them for an empty shard
 * only.  One null pointer of the two is refused.)
 * A NaN statistic is attained by nothing -- torch's ==, whatever the NaN's bit pattern -- so a NaN channel has no
 * claim, no position and no deposit.  The same rule holds for every tie search of this library: tie_stat of
 * bvq_fakequant_bwd, bvq_fakequant_bwd_stats, the weight lists, bvq_stat_tie_scan / bvq_stat_tie_apply and bvq_stat_bwd.
 * bvq_shard_unpack_deposit: from the gathered [world][2][channels] messages, per channel: dscale_total (nullable out)
 * = the double sum over the shards in rank order, rounded once (the same bits on every rank); on the shard that owns
 * the deposit (lowest claiming rank) dscale -> statistic's gradient (B/core/quant/int.py:160 backward, rounding points
 * of bvq_fakequant_bwd_stats) deposited on dx at first_pos[c].  One launch instead of unpack + cast + divide + deposit. */
int bvq_fakequant_bwd_shard(const bvq_quant_desc* d, const void* g, const void* x, const void* scale, const void* zp,
                            const void* stat, void* dx, double* message, int64_t* first_pos, int rank, void* workspace,
                            int64_t workspace_bytes, uint32_t* arrive, int64_t arrive_words, bvq_stream_t stream);
int bvq_shard_unpack_deposit(int dtype, const void* x, void* dx, const double* gathered, int world, int64_t channels,
                             int rank, const int64_t* first_pos, int64_t inner, int scale_dtype, double int_threshold,
                             int quot_dtype, int pre_op, float* dscale_total, bvq_stream_t stream);
int bvq_shard_pack(const float* dscale, const int64_t* tie_info, int64_t channels, int rank, int per_channel,
                   double* message, bvq_stream_t stream);
int bvq_shard_unpack(const double* gathered, int world, int64_t channels, int rank, int per_channel,
                     float* dscale_total, int64_t* tie_info, int64_t* total_ties, bvq_stream_t stream);

/* ---- histogram (KLMinimizerThreshold, B/core/stats/stats_op.py:280-350) -----------------------------------
 * counts[b] = number of elements of x in bin b of torch.histc(x, bins, min=-absmax, max=absmax) -- equal-width
 * bins, values outside the range ignored, bin = (int)((v + absmax) * bins / (2 absmax)) in float32, the value
 * +absmax in the last bin.  absmax: ONE element on the device in x's dtype (the AbsMax statistic: no host
 * sync); counts: int32 [bins], overwritten; 1 <= bins <= 8192.  One streaming read of x. */
int bvq_histc(int dtype, const void* x, int64_t n, const void* absmax, int bins, int32_t* counts,
              bvq_stream_t stream);

/* ---- moment statistics ---------------------------------------------------------------------------
 * sums is float32 [3 * channels]: sums[c] = SUM d, sums[channels + c] = SUM d^2 over the `outer` and `inner`
 * axes with d = |x| - p[c], and sums[2 * channels + c] = p[c], the channel's pivot (|x| of its first element,
 * 0 if that is not finite); per-unit float32 partials, double accumulation across units, fixed order.  The
 * host finishes on `channels` values:  mean |x| = p + SUM d / n,  var |x| = (SUM d^2 - (SUM d)^2 / n) / (n - 1)
 * -- shifted sums, so the variance does not cancel when the mean is far larger than the spread.  That is
 * what AbsAve (mean |x|) and MeanSigmaStd / MeanLearnedSigmaStd (mean |x| + sigma * sqrt(var |x| + eps))
 * need, in ONE read of x instead of abs (read + write) + mean (read) + var (read) --
 * B/core/stats/stats_op.py:186-262.  Sums are order-dependent: equal to torch's within float32 rounding. */
int64_t bvq_abs_moments_workspace_bytes(int dtype, int64_t outer, int64_t channels, int64_t inner);
int bvq_abs_moments(int dtype, const void* x, int64_t outer, int64_t channels, int64_t inner, float* sums,
                    void* workspace, int64_t workspace_bytes, bvq_stream_t stream);
/* dx = sgn(x) * (a[c] + b[c] * |x|), rounded once to x's dtype: the backward of any function of those two
 * moments (a = dL/dmean / n - 2 mean dL/dvar / (n-1), b = 2 dL/dvar / (n-1)); sgn(0) = 0 */
int bvq_abs_affine_bwd(int dtype, const void* x, const float* a, const float* b, void* dx, int64_t outer,
                       int64_t channels, int64_t inner, bvq_stream_t stream);

/* ---- percentile statistics ---------------------------------------------------------------------
 * k-th smallest value (k is 1-indexed, the same for every channel) of |x| (abs_key = 1) or of x
 * (abs_key = 0) over the `outer` and `inner` axes of x[outer, channels, inner]: torch.kthvalue on the
 * flat tensor / along dim 1 of the [C, -1] view, as used by AbsPercentile, NegativePercentileOrZero and
 * PercentileInterval (B/core/stats/stats_op.py:41-126).  Exact selection (MSD radix select); NaNs order last.
 * Streaming reads of x: channels == 1 (>= 4M elements, 16-byte aligned): 1 for |x| of a 16-bit type, else 2;
 * otherwise 2 for 16-bit types, 3 for float32.  out: dtype of x, `channels` elements.
 * bvq_kth_workspace_bytes: the workspace of every select entry below for this problem, to the byte (-1: bad argument).
 * The workspace starts on a 16-byte boundary: the byte offsets these entries publish are those of an aligned base, and
 * any other is refused with BVQ_ERR_INVALID before anything is launched. */
int64_t bvq_kth_workspace_bytes(int dtype, int64_t outer, int64_t channels, int64_t inner);
int bvq_kth_value(int abs_key, int dtype, const void* x, int64_t outer, int64_t channels, int64_t inner,
                  int64_t k, void* out, void* workspace, int64_t workspace_bytes, bvq_stream_t stream);
/* Two ranks of the same tensor in one call -- PercentileInterval's low and high percentile
 * (B/core/stats/stats_op.py:97-126): out[0][channels] = the k_first-th value, out[1][channels] = the k_second-th.
 * For channels == 1 (>= 4M elements, 16-byte aligned) both come from ONE histogram read (+ one read for the low
 * key bits of both); otherwise the same as two bvq_kth_value calls.  Workspace: bvq_kth_workspace_bytes. */
int bvq_kth_pair(int abs_key, int dtype, const void* x, int64_t outer, int64_t channels, int64_t inner,
                 int64_t k_first, int64_t k_second, void* out, void* workspace, int64_t workspace_bytes,
                 bvq_stream_t stream);

/* The same selection in steps, for a tensor whose batch is sharded over several devices (one process
 * per GPU): every shard histograms its own elements, the caller sums the histogram of the pass over the
 * shards (one RCCL all-reduce of channels * 2048 uint32 counters, at byte offset bvq_kth_hist_offset()
 * of the workspace) and every shard then picks the same digit -- the result is the k-th value of the
 * CONCATENATED tensor, on every shard, with no other exchange:
 *
 *   bvq_kth_begin(...);
 *   for (pass = 0; pass < bvq_kth_passes(dtype); ++pass) {
 *     bvq_kth_hist(..., pass, ...);   all-reduce(SUM) workspace[offset(pass) .. + channels*2048*4);
 *     bvq_kth_pick(..., pass, ...);
 *   }
 *   bvq_kth_finish(...);
 *
 * The rank is either explicit (BVQ_KTH_EXPLICIT, k >= 1) or derived ON THE DEVICE from the number of
 * elements the first (summed) histogram counted, by the rule the percentile statistics use -- so the
 * global element count never has to travel to the host:
 *   BVQ_KTH_HIGH: k = floor(.01 * q * n + 0.5)   AbsPercentile, PercentileInterval's upper end
 *   BVQ_KTH_LOW : k = ceil (.01 * q * n)         NegativePercentileOrZero, PercentileInterval's lower end
 * (B/core/stats/stats_op.py:56,84,114-116), clamped to [1, n] (torch.kthvalue raises for k = 0; callers
 * that need that error check q * n on the host).  Pass the same rule and q to bvq_kth_begin and to every
 * bvq_kth_pick.  The workspace (bvq_kth_workspace_bytes, with the shard's shape: a channel-last layout keeps a
 * transposed copy there) starts on a 16-byte boundary; the counter offsets depend on dtype and channels only.  Counters
 * are 32-bit: fewer than 2^32 elements per channel over all shards -- bvq_kth_value / bvq_kth_pair /
 * bvq_kth_hist return BVQ_ERR_UNSUPPORTED for a call that alone exceeds it; the caller of the sharded
 * protocol checks (elements per channel on a shard) x (shards) before starting. */
typedef enum bvq_kth_rule { BVQ_KTH_EXPLICIT = 0, BVQ_KTH_HIGH = 1, BVQ_KTH_LOW = 2 } bvq_kth_rule;
int bvq_kth_passes(int dtype);
int64_t bvq_kth_hist_offset(int dtype, int64_t channels, int pass);
int bvq_kth_begin(int dtype, int64_t channels, int rule, int64_t k, double q, void* workspace,
                  int64_t workspace_bytes, bvq_stream_t stream);
int bvq_kth_hist(int abs_key, int dtype, const void* x, int64_t outer, int64_t channels, int64_t inner,
                 int pass, void* workspace, int64_t workspace_bytes, bvq_stream_t stream);
int bvq_kth_pick(int dtype, int64_t channels, int pass, int rule, double q, void* workspace,
                 int64_t workspace_bytes, bvq_stream_t stream);
int bvq_kth_finish(int abs_key, int dtype, int64_t channels, void* out, void* workspace,
                   int64_t workspace_bytes, bvq_stream_t stream);

/* The sharded selection of a WHOLE-TENSOR statistic (one channel; the default Int8ActPerTensorFloat's
 * AbsPercentile, B/quant/base.py:68-75) with the 15-bit first digit of bvq_kth_value's per-tensor route: the first
 * pass histograms the top 15 key bits (32768 counters held in LDS) -- for |x| of a 16-bit type that is the whole key
 * and the only pass; otherwise a second pass counts the remaining 1 / 16 / 17 bits of the elements in the chosen
 * bin.  One read and one all-reduce for bf16 / f16 |x| (two of each with the 11-bit passes above), two for
 * float32 (three).  Same calling pattern, same rank rules, same 32-bit counter limit:
 *
 *   passes = bvq_kthw_plan(abs_key, dtype, -1, NULL, NULL);
 *   bvq_kthw_begin(...);
 *   for (pass = 0; pass < passes; ++pass) {
 *     bvq_kthw_hist(..., pass, ...);   bvq_kthw_plan(abs_key, dtype, pass, &offset, &words);
 *     all-reduce(SUM) the `words` uint32 counters at workspace + offset;
 *     bvq_kthw_pick(..., pass, ...);
 *   }
 *   bvq_kthw_finish(...);   -> out[1]
 *
 * x: n contiguous elements of this shard (any alignment, n may be 0).  Workspace: bvq_kth_workspace_bytes(dtype,
 * 1, 1, n).  rule / k / q are read by the pick of pass 0 only. */
int bvq_kthw_plan(int abs_key, int dtype, int pass, int64_t* hist_offset_bytes, int64_t* hist_words);
int bvq_kthw_begin(int abs_key, int dtype, void* workspace, int64_t workspace_bytes, bvq_stream_t stream);
int bvq_kthw_hist(int abs_key, int dtype, const void* x, int64_t n, int pass, void* workspace,
                  int64_t workspace_bytes, bvq_stream_t stream);
int bvq_kthw_pick(int abs_key, int dtype, int pass, int rule, int64_t k, double q, void* workspace,
                  int64_t workspace_bytes, bvq_stream_t stream);
int bvq_kthw_finish(int abs_key, int dtype, void* out, void* workspace, int64_t workspace_bytes,
                    bvq_stream_t stream);

/* which elements attain the statistic */
typedef enum bvq_match_kind {
  BVQ_MATCH_ABS = 0,   /* |x| == stat, deposit scaled by sgn(x): torch.max(torch.abs(x)) (AbsMax)   */
  BVQ_MATCH_VALUE = 1, /*  x  == stat: torch.max(x) / torch.min(x) (the two halves of AbsMinMax)    */
  /* OR-ed flag: even with channels == 1 only the FIRST attaining element receives the gradient (an
   * index-returning reduction such as torch.kthvalue / torch.max(dim) over a flattened tensor) */
  BVQ_MATCH_FIRST = 16
} bvq_match_kind;

/* Backward of a max / min statistic w.r.t. x, as autograd derives it from torch.max / torch.min
 * (and torch.abs) in B/core/stats/stats_op.py:137-158:
 *   channels == 1 (full reduction): every element attaining stat receives gstat / #ties;
 *   channels  > 1 (reduction along a dim): the FIRST such element of each channel, in
 *                                    (outer, inner) order, receives gstat[c];
 *   MATCH_ABS additionally multiplies by sgn(x) (0 at 0), so zeros carry the sign of x.
 * mode_add == 0: dx is fully written (zeros elsewhere); mode_add == 1: the terms are added in place
 * to an existing dx (used by the fused quantizer backward: one streaming read of x, no write pass).
 * stat, gstat and dx have dtype `dtype`.  workspace: bvq_stats_workspace_bytes(ABSMAX,...) bytes. */
int bvq_stat_bwd(int match, int dtype, const void* x, const void* stat, const void* gstat, void* dx,
                 int64_t outer, int64_t channels, int64_t inner, int mode_add, void* workspace,
                 int64_t workspace_bytes, bvq_stream_t stream);

/* The two halves of bvq_stat_bwd, for callers that put work between them (batch-sharded tensors:
 * the ranks agree on which shard owns each channel's first maximum before anything is deposited).
 * tie_info: device buffer of bvq_tie_info_bytes(channels) bytes (the words below, measured; -1 for channels < 1),
 * int64 words:
 *   channels > 1 : word c = smallest (outer*inner + i) position attaining stat[c], or -1 if none;
 *                  setting a word to -1 suppresses that channel's deposit;
 *   channels == 1: word 0 = number of ties found, words 2.. = flat indices of (up to 1024 of) them.
 * bvq_stat_tie_scan: one streaming read of x; if dx_zero_fill is non-null it is also written with
 *   the zeros non-attaining elements receive (signed by sgn(x) for MATCH_ABS).
 * bvq_stat_tie_apply: deposits gstat at the recorded positions.  total_ties (nullable, device, one
 *   int64) replaces the local tie count when the ties of a whole-tensor maximum are spread over
 *   several shards.  pre_op (MATCH_ABS only): the statistic was taken of pre_op(x), so the deposit's
 *   sign is sgn(pre_op(x)). */
int64_t bvq_tie_info_bytes(int64_t channels);
int bvq_stat_tie_scan(int match, int dtype, const void* x, const void* stat, int64_t outer,
                      int64_t channels, int64_t inner, void* dx_zero_fill, int64_t* tie_info,
                      bvq_stream_t stream);
int bvq_stat_tie_apply(int match, int pre_op, int dtype, const void* x, const void* stat,
                       const void* gstat, const int64_t* tie_info, const int64_t* total_ties, void* dx,
                       int64_t outer, int64_t channels, int64_t inner, int mode_add, bvq_stream_t stream);

/* bvq_stat_tie_apply(MATCH_ABS, mode_add = 1) for the fused stats-scaled quantizer, taking the
 * float32 scale-gradient sums of bvq_fakequant_bwd directly: per channel the deposited gradient is
 *   ((dscale.to(scale_dtype)) / int_threshold -> quot_dtype).to(dtype of x)
 * i.e. the backward of  scale = clamp_min_ste(stat) / int_threshold  (B/core/quant/int.py:160,
 * B/core/restrict_val.py:22-42) with torch's rounding points, without the three tiny launches.
 * pre_op: the statistic was taken of pre_op(x); the deposit's sign is sgn(pre_op(x)). */
int bvq_stat_tie_apply_dscale(int pre_op, int dtype, const void* x, const void* stat, const float* dscale,
                              int scale_dtype, double int_threshold, int quot_dtype,
                              const int64_t* tie_info, const int64_t* total_ties, void* dx, int64_t outer,
                              int64_t channels, int64_t inner, bvq_stream_t stream);

/* ---- fused affine quantize / dequantize (seam 2: IntQuant) ---------------------------------- */

/* Forward: one read of x, one write of y.
 *   t = x / scale ; t = t + zp ; t = round_mode(t) ; t = clamp(t, qmin, qmax) ;
 *   y = (t - zp) * scale          (BVQ_OUT_DEQUANT)   or   y = t   (BVQ_OUT_INT)
 * with every operation rounded to ct_dtype exactly where the reference's op chain rounds
 * (B/core/quant/int_base.py:63-97).  codes (nullable, desc->codes_dtype, same element count) receives
 * the clamped integer codes; y may be null when only the codes are wanted (1 read of x, 1-4 bytes
 * written per element: the layout downstream integer kernels and the QCDQ exporters consume). */
int bvq_fakequant_fwd(const bvq_quant_desc* desc, const void* x, const void* scale, const void* zp,
                      void* y, void* codes, bvq_stream_t stream);

/* Statistic AND quantizer in ONE launch: AbsMax over (outer, inner) -> clamp_min(min_val) -> / int_threshold
 * -> quantize-dequantize with that scale and a zero zero-point -- bvq_absmax_scale followed by
 * bvq_fakequant_fwd, i.e. RescalingIntQuant.forward on the stats-scaled graphs (B/core/quant/int.py:155-163,
 * B/core/scaling/runtime.py:50-72), in ONE launch, reading x ONCE: a channel that fits the registers of one
 * workgroup (weights, small activations) is held there between the reduction and the quantization (2 tensor
 * passes instead of 3, one launch instead of three).  Uses desc's shape, dtypes (x_dtype == ct_dtype), qmin/qmax,
 * round_mode, scalar_mode, pre_op, scale_dtype / scale_per_channel; zero-point is +0.  stat_out: [channels] in
 * x's dtype, scale_out: [channels] in scale_dtype.  bvq_stats_fakequant_fwd_workspace_bytes returns 0 when the
 * shape is not covered (a channel larger than one workgroup's registers, ragged rows, misaligned pointers):
 * the caller then takes the two-call route. */
int64_t bvq_stats_fakequant_fwd_workspace_bytes(const bvq_quant_desc* desc, const void* x, const void* y);
int bvq_stats_fakequant_fwd(const bvq_quant_desc* desc, const void* x, double min_val, int use_min,
                            double int_threshold, void* stat_out, void* scale_out, void* y, void* workspace,
                            int64_t workspace_bytes, bvq_stream_t stream);

/* The same AbsMax -> scale -> IntQuant in ONE launch (x read once) for channels that do NOT fit one workgroup: each
 * channel is held in registers by a CLUSTER of workgroups, which agree on its maximum through one arrival word each;
 * a persistent grid of clusters walks the channels, or (many channels per cluster) every channel has its own.  stat_out [channels] in x's dtype, scale_out [channels] in
 * desc->scale_dtype, running (nullable, [channels] of run_dtype: the running average of bvq_absmax_scale_onepass) and
 * y are the bits of bvq_absmax_scale_onepass + bvq_fakequant_fwd on the same descriptor.  A workgroup never waits
 * without a bound: past a time budget it reads the whole channel itself (same bits; `fallbacks`, nullable, counts
 * those).  flags: BVQ_CLUSTER_FORCE_FALLBACK (tests) takes that path every time.
 * bvq_absmax_fakequant_cluster_supported -> the arrival words the call needs, or 0 when not covered.  Covered: a
 * per-channel scale with channels > 1, x and y of one dtype, not overlapping, dequantized output, zero zero-point,
 * 16-byte aligned, rows of whole 16-byte chunks, a channel of at most 64 workgroups' registers.  Host-side only.
 * arrive: `arrive_words` uint32 words, all zero on entry, handed back as zeros (the contract of
 * bvq_absmax_scale_onepass). */
#define BVQ_CLUSTER_FORCE_FALLBACK 1
int64_t bvq_absmax_fakequant_cluster_supported(const bvq_quant_desc* desc, const void* x, const void* y);
int bvq_absmax_fakequant_cluster(const bvq_quant_desc* desc, const void* x, double min_val, int use_min,
                                 double int_threshold, void* stat_out, void* scale_out, int run_dtype, void* running,
                                 double momentum, int first_batch, void* y, uint32_t* arrive, int64_t arrive_words,
                                 int flags, uint32_t* fallbacks, bvq_stream_t stream);
/* Developer / test entry: the same call with the form of the kernel named instead of chosen per shape.
 * form: 0 the library's choice for the shape (= bvq_absmax_fakequant_cluster), 1 a persistent grid of clusters
 * walking the channels, 2 one-shot: one workgroup per (channel, member).  Both forms give the same bits and use the
 * same arrival words.  stamps: null, except with a library built with
 * -DBVQ_CLUSTER_STAMPS (tools/cluster_phases.py): [channels][members][6] clock ticks of every round. */
int bvq_absmax_fakequant_cluster_form(const bvq_quant_desc* desc, const void* x, double min_val, int use_min,
                                      double int_threshold, void* stat_out, void* scale_out, int run_dtype,
                                      void* running, double momentum, int first_batch, void* y, uint32_t* arrive,
                                      int64_t arrive_words, int flags, uint32_t* fallbacks, int form, uint64_t* stamps,
                                      bvq_stream_t stream);

/* bytes of scratch bvq_fakequant_bwd needs */
int64_t bvq_fakequant_bwd_workspace_bytes(const bvq_quant_desc* desc);

/* Backward of the chain above, as autograd derives it:
 *   dt = pass ? g*scale : 0      pass = clamp_ste || !(t_rounded > qmax || t_rounded < qmin)
 *   dx = dt / scale                                              (dtype x_dtype)
 *   dscale[c] = sum g*(t_clamped - zp)  -  sum dt * ((x/scale)/scale)     (float32, nullable)
 *   dzp[c]    = sum dt - sum g*scale                                      (float32, nullable)
 * dscale / dzp have `channels` elements when scale OR zero-point is per-channel, else one.
 * One read of g, one read of x, one write of dx; the per-channel sums ride on the same reads and
 * are combined in a fixed order (bit-reproducible run to run).
 * tie_stat / tie_info (both null or both set; requires dscale set and dzp null): while streaming x
 * the kernel also records which elements attain the abs-max statistic tie_stat (dtype of x,
 * `channels` elements) into tie_info (see bvq_stat_tie_scan), so that the statistic's gradient can
 * be deposited with bvq_stat_tie_apply without another pass over x. */
int bvq_fakequant_bwd(const bvq_quant_desc* desc, const void* g, const void* x, const void* scale,
                      const void* zp, void* dx, float* dscale, float* dzp, const void* tie_stat,
                      int64_t* tie_info, void* workspace, int64_t workspace_bytes, bvq_stream_t stream);

/* Learned bit widths (BitWidthParameter, B/core/bit_width/parameter.py:23-100): the integer range is then a pair of
 * 0-dim tensors in the autograd graph (min_int / max_int of the bit-width tensor, B/function/ops.py:132-191), not
 * host numbers.  `bounds` = [qmin, qmax] as float32 ON THE DEVICE replaces desc->qmin / qmax (no host sync):
 * bvq_fakequant_fwd_bounds is bvq_fakequant_fwd reading them; bvq_fakequant_bwd_bounds is bvq_fakequant_bwd(dscale)
 * that also returns, when dbounds is non-null (a plain TensorClamp: tensor_clamp's two torch.where send the gradient
 * of a replaced value to the bound that replaced it), dbounds[0 .. n) = per-channel sums of the gradient reaching
 * qmin and dbounds[n .. 2n) of that reaching qmax (n = channels for per-channel scales, else 1; the caller adds the
 * channels up).  With a straight-through clamp pass dbounds = null.  Workspace: bvq_fakequant_bwd_workspace_bytes. */
int bvq_fakequant_fwd_bounds(const bvq_quant_desc* desc, const void* x, const void* scale, const void* zp,
                             const float* bounds, void* y, bvq_stream_t stream);
int bvq_fakequant_bwd_bounds(const bvq_quant_desc* desc, const void* g, const void* x, const void* scale,
                             const void* zp, const float* bounds, void* dx, float* dscale, float* dbounds,
                             void* workspace, int64_t workspace_bytes, bvq_stream_t stream);

/* Learned scales (ParameterScaling, and ParameterFromRuntimeStatsScaling once its collection phase is over:
 * the steady state of the default Int8ActPerTensorFloat; B/core/scaling/standalone.py:75-152, 155-298), float
 * restriction:   scale = abs_binary_sign_grad(clamp_min_ste(value, min_val)) / int_threshold.
 * bvq_learned_scale: that forward in ONE launch over the n (1 or `channels`) elements of `value`, the quotient
 *   rounded to scale_dtype -- instead of clamp, |.|, division (3 launches).  min_val: python scalar (rounded to
 *   value_dtype here); int_threshold: already rounded to the dtype the division runs in.
 * bvq_fakequant_bwd_learned: bvq_fakequant_bwd(dscale) whose LAST reduction launch also carries the scale
 *   gradient through that chain's backward with torch's rounding points --
 *     dvalue = binary_sign(clamp_min(value)) * ((dscale.to(scale_dtype) [+ gscale]) / int_threshold)
 *   (gscale, nullable, scale_dtype: gradient reaching `scale` from its other users) -- instead of a cast, a
 *   division, a sign-multiply and their launches.  dscale (float32, 1 or `channels`) is still written.
 *   Workspace: bvq_fakequant_bwd_workspace_bytes. */
int bvq_learned_scale(int value_dtype, const void* value, int64_t n, double min_val, int use_min,
                      double int_threshold, int scale_dtype, void* scale_out, bvq_stream_t stream);
int bvq_fakequant_bwd_learned(const bvq_quant_desc* desc, const void* g, const void* x, const void* scale,
                              const void* zp, void* dx, float* dscale, const void* value, int value_dtype,
                              double min_val, int use_min, double int_threshold, const void* gscale,
                              void* dvalue, void* workspace, int64_t workspace_bytes, bvq_stream_t stream);

/* Backward of the stats-scaled per-channel graphs (scale = clamp_min(AbsMax(x)) / int_threshold) in
 * TWO launches: the backward kernel (dx, per-unit dscale sums, per-unit first position attaining `stat`) and one
 * finishing kernel per call that sums dscale (-> dscale[channels], float32), turns it into the statistic's
 * gradient -- dscale.to(scale_dtype) / int_threshold (in quot_dtype) -> x's dtype -- and adds it, times sgn(x),
 * to the first arg-max element of every channel in dx: bvq_fakequant_bwd(tie_stat) + bvq_stat_tie_apply_dscale
 * without their three helper launches.  bvq_fakequant_bwd_stats_workspace_bytes returns 0 for layouts it does
 * not cover (one scale for the whole tensor: its gradient is shared evenly by all ties; channels with more
 * than 4096 work units): the caller then takes the two-call route. */
int64_t bvq_fakequant_bwd_stats_workspace_bytes(const bvq_quant_desc* desc);
int bvq_fakequant_bwd_stats(const bvq_quant_desc* desc, const void* g, const void* x, const void* scale,
                            const void* zp, const void* stat, void* dx, float* dscale, int scale_dtype,
                            double int_threshold, int quot_dtype, void* workspace, int64_t workspace_bytes,
                            bvq_stream_t stream);

/* bvq_fakequant_bwd_stats in ONE launch (row-mapped per-channel layouts; bvq_fakequant_bwd_stats_onepass_supported:
 * 1 / 0): the backward kernel writes dx and its per-unit partials through to memory (agent scope), every wave counts
 * its unit in on its channel's arrival counter, and the wave whose count completes the channel sums the channel's
 * dscale partials (double, fixed order), takes the first arg-max position, converts dscale into the statistic's
 * gradient and deposits it on that element of dx -- the finishing launch of bvq_fakequant_bwd_stats, done by whoever
 * arrives last; no wave waits.  Same results, bit for bit (the sums are taken in a fixed order of their own).
 * arrive: `arrive_words` >= channels uint32 words, ALL ZERO when the launch starts, handed back as zeros (the
 * contract of bvq_absmax_scale_onepass; the two may share one buffer on one stream).  workspace: as
 * bvq_fakequant_bwd_stats_workspace_bytes. */
int bvq_fakequant_bwd_stats_onepass_supported(const bvq_quant_desc* d);
int bvq_fakequant_bwd_stats_onepass(const bvq_quant_desc* d, const void* g, const void* x, const void* scale,
                                    const void* zp, const void* stat, void* dx, float* dscale, int scale_dtype,
                                    double int_threshold, int quot_dtype, void* workspace, int64_t workspace_bytes,
                                    uint32_t* arrive, int64_t arrive_words, bvq_stream_t stream);

/* ---- the other quantizers of the family -------------------------------------------
 * BinaryQuant / ClampedBinaryQuant (B/core/quant/binary.py:19-101), TernaryQuant (B/core/quant/ternary.py:18-66),
 * DecoupledIntQuant (B/core/quant/int_base.py:100-182) and TruncIntQuant (B/core/quant/int.py:199-229) as ONE
 * forward kernel (read x, write y) and ONE backward kernel (read g, read x, write dx; the scale gradients as
 * float32 sums over the tensor or per channel) instead of the reference's 4..10 torch ops each, with the
 * reference's rounding points in the compute dtype ct_dtype = torch.result_type of its op chain.
 *   x viewed as [outer, channels, inner]; scale / pre_scale: 1 element (whole tensor) or `channels` elements in
 *   scale_dtype; zero-points: ONE element in zp_dtype, or null for +0.  kind-specific fields:
 *     BINARY          y = binary_sign(x) * scale
 *     CLAMPED_BINARY  x clamped to [-scale, scale] first; clamp_ste = 0: the clamp masks dx and feeds d(scale)
 *     TERNARY         y = [|x| > threshold * scale] * sign(x) * scale   (ct_dtype must be float32: the reference's
 *                     mask.float() promotes)
 *     DECOUPLED       round_mode / qmin / qmax / clamp_ste as bvq_quant_desc; rounding grid from (pre_scale, pre_zp),
 *                     de-quantization with (scale, zp); dpre_scale receives the pre-scale's gradient
 *     TRUNC           y = (round_mode(round((x / scale + zp)) / trunc_scale) - zp) * scale
 * dscale / dpre_scale: float32 [1 or channels], nullable.  Workspace: bvq_variant_bwd_workspace_bytes. */
typedef enum bvq_variant_kind {
  BVQ_VAR_BINARY = 0, BVQ_VAR_CLAMPED_BINARY = 1, BVQ_VAR_TERNARY = 2, BVQ_VAR_DECOUPLED = 3, BVQ_VAR_TRUNC = 4
} bvq_variant_kind;
typedef struct bvq_variant_desc {
  int64_t outer, channels, inner;
  int32_t kind;               /* bvq_variant_kind */
  int32_t x_dtype, ct_dtype, scale_dtype, zp_dtype;
  int32_t scale_per_channel;
  int32_t round_mode;         /* bvq_round_mode */
  int32_t clamp_ste;
  int32_t scalar_mode;        /* bvq_scalar_mode */
  float qmin, qmax;           /* DECOUPLED */
  float threshold;            /* TERNARY */
  float trunc_scale;          /* TRUNC: 2^(input_bit_width - output_bit_width) */
} bvq_variant_desc;
int bvq_variant_fwd(const bvq_variant_desc* desc, const void* x, const void* scale, const void* pre_scale,
                    const void* zp, const void* pre_zp, void* y, bvq_stream_t stream);
int64_t bvq_variant_bwd_workspace_bytes(const bvq_variant_desc* desc);
int bvq_variant_bwd(const bvq_variant_desc* desc, const void* g, const void* x, const void* scale,
                    const void* pre_scale, const void* zp, const void* pre_zp, void* dx, float* dscale,
                    float* dpre_scale, void* workspace, int64_t workspace_bytes, bvq_stream_t stream);

/* ---- many weights, each with its own statistic, in one launch each way --------------------------------------------
 * QAT re-quantizes every layer's weight on every forward (RescalingIntQuant.forward through proxy.tensor_quant,
 * B/proxy/parameter_quant.py:83-89, B/core/quant/int.py:155-163).  These entries do that for a LIST of independent
 * per-output-channel weights: each item has its own shape, statistic, scale and integer range; the call has one dtype
 * and one rounding mode.
 *   bvq_weight_quant_list_fwd: for every item, exactly bvq_stats_fakequant_fwd on the descriptor
 *     (outer 1, channels, inner, x_dtype = ct_dtype = dtype, scale_dtype, scale per channel, zero zero-point, qmin, qmax,
 *     round_mode) with (min_val, use_min, int_threshold): stat [channels] in dtype, scale [channels] in scale_dtype, y.
 *     ONE launch: the workgroups are dealt over the (item, channel) pairs of the whole list.
 *   bvq_weight_quant_list_bwd: for every item, exactly bvq_fakequant_bwd_stats_onepass on that descriptor (clamp_ste of
 *     the item) with g, stat, scale, (scale_dtype, int_threshold, quot_dtype): dx with the statistic's gradient deposited,
 *     dscale [channels] float32.  ONE launch: the waves are dealt over the units of all items, each item keeping the
 *     decomposition, the partials and their combine order of its own call -- dx and dscale are the same bits.
 *     Item i's channels take words [sum of the channels before it, + channels) of `arrive` (the contract of
 *     bvq_absmax_scale_onepass: all zero on entry, handed back as zeros).  workspace: bvq_weight_quant_list_bwd_workspace_bytes.
 * An item is covered when its channel fits one workgroup's registers (bvq_stats_fakequant_fwd_workspace_bytes > 0), its
 * layout has the one-launch backward (bvq_fakequant_bwd_stats_onepass_supported: per-channel, row-mapped, half-even
 * rounding), its rows are whole 16-byte chunks and x, y, g and dx (those that are not null) are 16-byte aligned; the
 * list is covered when every item is and its channels fit arrive_words (0: not checked).
 * bvq_weight_list_supported: 1 / 0.  The two calls return BVQ_ERR_UNSUPPORTED for a list not covered: quantize the items
 * one by one.  Null items, n < 1, n > BVQ_WEIGHT_LIST_MAX, a null pointer an item needs or a bad dtype: BVQ_ERR_INVALID,
 * found before anything touches the device.
 * Argument passing: the items travel BY VALUE in the kernel arguments (one struct of at most BVQ_WEIGHT_LIST_MAX
 * per-tensor blocks, <= 4 KiB): no table to upload, nothing to keep alive between calls, and graph capture records
 * them with the launch.  Longer lists take ceil(n / BVQ_WEIGHT_LIST_MAX) calls. */
#define BVQ_WEIGHT_LIST_MAX 16
typedef struct bvq_weight_item {
  const void* x;      /* the weight, [channels, inner] contiguous, the call's dtype */
  void* y;            /* forward: fake-quantized weight, like x */
  void* stat;         /* [channels] in dtype: written by the forward, read by the backward */
  void* scale;        /* [channels] in scale_dtype: written by the forward, read by the backward */
  const void* g;      /* backward: gradient of y, like x */
  void* dx;           /* backward: gradient of x, like x */
  float* dscale;      /* backward: [channels] float32 */
  int64_t channels;   /* output channels (>= 2) */
  int64_t inner;      /* elements per channel */
  double min_val;     /* clamp_min of the statistic (use_min); rounded to dtype like bvq_stats_fakequant_fwd */
  double int_threshold; /* the value the division sees, forward and backward (dimensioned scale: rounded to scale_dtype) */
  float qmin;         /* integer range */
  float qmax;
  int32_t use_min;
  int32_t clamp_ste;  /* backward: 1 TensorClampSte, 0 TensorClamp */
} bvq_weight_item;
int bvq_weight_list_supported(int dtype, int round_mode, int n, const bvq_weight_item* items, int64_t arrive_words);
int bvq_weight_quant_list_fwd(int dtype, int scale_dtype, int round_mode, int n, const bvq_weight_item* items,
                              bvq_stream_t stream);
int64_t bvq_weight_quant_list_bwd_workspace_bytes(int dtype, int n, const bvq_weight_item* items);
int bvq_weight_quant_list_bwd(int dtype, int scale_dtype, int quot_dtype, int round_mode, int n,
                              const bvq_weight_item* items, void* workspace, int64_t workspace_bytes, uint32_t* arrive,
                              int64_t arrive_words, bvq_stream_t stream);

/* ---- group-wise weights: one scale per group of consecutive elements ------------------------------------------------
 * A weight [out, K] with one scale per `group_size` consecutive elements of each row is, in memory, [groups, group_size]
 * with one scale per row.  The descriptor says so: outer = 1, channels = groups, inner = group_size, scale_per_channel,
 * x_dtype = ct_dtype = scale_dtype, zero zero-point.  The results are those of bvq_stats_fakequant_fwd and
 * bvq_fakequant_bwd_stats on that descriptor; what differs is the kernel: a group lives in a fraction of one wave, so
 * statistic, scale, quantization, scale gradient and arg-max deposit stay in registers -- ONE launch each way, no
 * workspace, no atomics.  Only the order in which a group's float32 scale-gradient terms are added differs from the
 * per-channel kernels (the deposited element can move by a rounding).
 *   bvq_group_quant_fwd: AbsMax per group -> clamp_min(min_val) (use_min) -> / thr_div (the value the division sees,
 *     rounded to the scale's dtype by the caller) -> quantize-dequantize.  y like x; scale, stat: [groups] in x's dtype.
 *   bvq_group_quant_bwd: dx = the quantizer's input gradient + the statistic's gradient of each group on the first
 *     element attaining it.  stat: the forward's output (the scale is derived from it again, same bits; `scale` is not
 *     read).  gscale (nullable, [groups] in x's dtype): a gradient arriving through the returned scale, added to the
 *     group's scale gradient before it becomes the statistic's.  The clamp_min is straight-through, as in the
 *     per-channel route.
 * Covered: group_size 16, 32, 64, 128 or 256; BVQ_ROUND; BVQ_PRE_NONE; BVQ_OUT_DEQUANT; every tensor pointer on a
 * 16-byte boundary.  Anything else returns BVQ_ERR_UNSUPPORTED with a bvq_last_error() text, found before anything
 * touches the device; bvq_group_quant_supported answers 1 / 0 for a descriptor and x. */
int bvq_group_quant_supported(const bvq_quant_desc* desc, const void* x);
int bvq_group_quant_fwd(const bvq_quant_desc* desc, const void* x, double min_val, int use_min, double thr_div, void* y,
                        void* scale, void* stat, bvq_stream_t stream);
int bvq_group_quant_bwd(const bvq_quant_desc* desc, const void* g, const void* x, const void* scale, const void* stat,
                        const void* gscale, double min_val, int use_min, double thr_div, void* dx, bvq_stream_t stream);

/* ---- group-wise weights with a searched clipping threshold (MSE) -------------------------------------------------------
 * The group-wise quantizer above with n candidate thresholds per group instead of the abs-max alone (the clip search
 * of low-bit weight-only recipes; `MSE` statistic of later Brevitas releases, no reference counterpart).  Descriptor,
 * min_val / use_min / thr_div, y, scale and stat as in bvq_group_quant_fwd.  ratios: a HOST array of n_ratios floats,
 * copied into the kernel's arguments (nothing of it is read after the call returns); ratios[0] == 1, every ratio finite
 * and in (0, 1], 1 <= n_ratios <= 64.  T is x's dtype.
 * Forward, per group:
 *     a   = max |x|                                      (stat, a value of T)
 *     t_i = T(a * ratios[i])                             (product in float32, rounded once)
 *     s_i = T(clamp_min(t_i, min_val) / thr_div)         (the scale of bvq_group_quant_fwd for the statistic t_i)
 *     y_i = quantize-dequantize of the group at s_i      (the values of T that bvq_group_quant_fwd would store)
 *     e_i = sum (float32(y_i) - float32(x))^2            (float32; added in the kernel's fixed butterfly order)
 *     k   = the first i with e_i < e_j for every j < i   (strict: ties keep the earlier candidate; a group with a NaN or
 *           Inf has NaN errors and keeps k = 0, a group of zeros keeps k = 0)
 *   y = y_k, scale = s_k, stat = a, idx = k as uint8 [groups].
 * Backward: k is a constant.  dx and the group's scale gradient v (+ gscale) as in bvq_group_quant_bwd at the scale
 * s_k, derived again from stat and idx; dt = T(v / thr_div), da = T(dt * ratios[k]); sign(x) * da is added to the first
 * element of the group with |x| == a.
 * With ratios = {1} both entries compute the bits of bvq_group_quant_fwd / bvq_group_quant_bwd.
 * One launch each way, no workspace, no atomics.  Covered: what the group-wise entries cover, and the ratios as above;
 * anything else returns BVQ_ERR_UNSUPPORTED with a bvq_last_error() text, found before anything touches the device;
 * bvq_group_mse_supported answers 1 / 0 for a descriptor, x and a candidate count. */
int bvq_group_mse_supported(const bvq_quant_desc* desc, const void* x, int n_ratios);
int bvq_group_mse_fwd(const bvq_quant_desc* desc, const void* x, const float* ratios, int n_ratios, double min_val,
                      int use_min, double thr_div, void* y, void* scale, void* stat, void* idx, bvq_stream_t stream);
int bvq_group_mse_bwd(const bvq_quant_desc* desc, const void* g, const void* x, const void* stat, const void* idx,
                      const void* gscale, const float* ratios, int n_ratios, double min_val, int use_min,
                      double thr_div, void* dx, bvq_stream_t stream);

/* ---- asymmetric group-wise weights: one scale and one integer zero-point per group ------------------------------------
 * The unsigned weight-only format of AWQ / GPTQ style checkpoints (ShiftedUint8WeightPerGroupFloat of later Brevitas
 * releases).  The descriptor is that of the group-wise section with zp_per_channel = 1 and zp_dtype = x_dtype; T is x's
 * dtype.  The results are those of the per-channel asymmetric graph (AbsMinMax scale, NegativeMinOrZero zero-point
 * quantized through IntQuant.to_int) on the tensor regrouped as [groups, group_size], every operation rounding to T:
 *     mx = max x, mn = min x                          (a NaN anywhere in the group is both)
 *     scale = T(clamp_min(|T(mx - mn)|, min_val) / thr_div)
 *     m0 = mn <= 0 ? mn : 0;  zp = clamp(round_half_even(T(T(-m0 / scale) + 0)), qmin, qmax)
 *     q = clamp(round_half_even(T(T(x / scale) + zp)), qmin, qmax);  y = T(T(q - zp) * scale)
 *   bvq_group_shifted_fwd: y like x; scale, zp: [groups] in T; stat: [2 * groups] in T, the maxima then the minima (the
 *     layout of BVQ_STAT_MINMAX).
 *   bvq_group_shifted_bwd: the autograd of that graph.  dx = the quantizer's input gradient; the group's scale and
 *     zero-point gradients are float32 sums rounded to T, joined by gscale / gzp (nullable, [groups] in T: gradients
 *     arriving through the returned scale / zero-point); the zero-point's travels through its own clamp (masked where it
 *     clipped unless clamp_ste), the rounding (straight-through) and -m0 / scale to the scale and, where mn <= 0, to mn;
 *     the scale's through / thr_div, the straight-through clamp_min and |mx - mn| (zero gradient at 0) to mx and mn.  The
 *     gradient of mx is added to the first element of the group equal to mx, that of mn to the first equal to mn (-0
 *     equals +0; a NaN statistic is equal to nothing).  stat: the forward's output; scale and zero-point are derived from
 *     it again, same bits.
 * One launch each way, no workspace, no atomics.  Only the order in which a group's float32 gradient terms are added
 * differs from the per-channel kernels (the two deposited elements can move by a rounding).  Covered: what the
 * group-wise entries cover; anything else returns BVQ_ERR_UNSUPPORTED with a bvq_last_error() text, found before
 * anything touches the device; bvq_group_shifted_supported answers 1 / 0 for a descriptor and x. */
int bvq_group_shifted_supported(const bvq_quant_desc* desc, const void* x);
int bvq_group_shifted_fwd(const bvq_quant_desc* desc, const void* x, double min_val, int use_min, double thr_div,
                          void* y, void* scale, void* zp, void* stat, bvq_stream_t stream);
int bvq_group_shifted_bwd(const bvq_quant_desc* desc, const void* g, const void* x, const void* stat,
                          const void* gscale, const void* gzp, double min_val, int use_min, double thr_div, void* dx,
                          bvq_stream_t stream);

/* ---- asymmetric group-wise weights with a searched zero-point (HQO) ----------------------------------------------------
 * The asymmetric group-wise quantizer above with the zero-point of each group moved by half-quadratic optimisation (HQQ;
 * HalfQuadraticOptimizerZeroPoint of later Brevitas releases, no reference counterpart).  Descriptor, min_val / use_min /
 * thr_div, y, scale and stat as in bvq_group_shifted_fwd; T is x's dtype.  inv_beta: a HOST array of n_iters + 1 floats,
 * inv_beta[i] = 1 / (beta * kappa^i), every one finite and positive, copied into the kernel's arguments; 0 <= n_iters
 * <= 63; lp: 0 for the norm p = 1, 1 for p = 0.5.
 * Forward, per group, with mx, mn, s and the integer zero-point zp_0 of bvq_group_shifted_fwd, xf = float32(x),
 * inv_s = 1 / float32(s) and z_0 = zp_0, for i = 0 .. n_iters:
 *     zp_i = T(z_i)
 *     q_i  = clamp(round_half_even(T(T(x / s) + zp_i)), qmin, qmax);  y_i = T(T(q_i - zp_i) * s)
 *     r    = xf - float32(y_i);  e_i = tree(|r|)
 *     better = i == 0 or (live and e_i < e_best)     (strict; a NaN error is below nothing)
 *     better: (e_i, zp_i, i) is the best so far; not better: the group is finished for good (live = false); a constant
 *     group (mx == mn: the scale is its lower bound) is finished after candidate 0
 *     thr  = inv_beta[i] (p = 1) or inv_beta[i] / sqrt(|r|) (p = 0.5);  w_e = sign(r) * max(|r| - thr, 0)
 *     z_{i+1} = tree(float32(q_i) - (xf - w_e) * inv_s) * (1 / g)
 *   every float32 operation rounded on its own.  tree(v): within each 16-byte chunk of the group the even-indexed
 *   elements added in order and the odd-indexed likewise, the two sums added, the per-chunk values then reduced by halves,
 *   t[:h] + t[h:].  y = y_k, zp = zp_k (a value of T, in general no integer), scale = s, stat as above, idx = k as uint8
 *   [groups], k the kept index.  With n_iters = 0 every output has the bits of bvq_group_shifted_fwd.
 * Backward: zp_k is a constant.  dx as in bvq_group_shifted_bwd at (s, zp_k); the group's scale gradient is the rounded
 * float32 sum (+ gscale, nullable) and goes through / thr_div, the straight-through clamp_min and |mx - mn| to the first
 * element equal to mx and, negated, to the first equal to mn.  The zero-point has no gradient path.  stat, zp: the
 * forward's outputs.
 * One launch each way, no workspace, no atomics.  Covered: what the asymmetric group-wise entries cover, and n_iters, lp
 * and the table as above; anything else returns BVQ_ERR_UNSUPPORTED with a bvq_last_error() text, found before anything
 * touches the device; bvq_group_hqo_supported answers 1 / 0 for a descriptor, x, an iteration count and an lp code. */
int bvq_group_hqo_supported(const bvq_quant_desc* desc, const void* x, int n_iters, int lp);
int bvq_group_hqo_fwd(const bvq_quant_desc* desc, const void* x, const float* inv_beta, int n_iters, int lp,
                      double min_val, int use_min, double thr_div, void* y, void* scale, void* zp, void* stat, void* idx,
                      bvq_stream_t stream);
int bvq_group_hqo_bwd(const bvq_quant_desc* desc, const void* g, const void* x, const void* stat, const void* zp,
                      const void* gscale, double min_val, int use_min, double thr_div, void* dx, bvq_stream_t stream);

/* ---- AWQ: the candidates of an activation-aware column-factor search over a group-wise weight ---------------------------
 * AWQ (Lin et al. 2023; no reference counterpart) multiplies every input column of a linear weight by a factor before the
 * group-wise quantizer and divides it out behind it.  x is the weight [R, K] of dtype T, contiguous; the descriptor is
 * that of the group-wise section (symmetric: zp_per_channel = 0) or of the asymmetric one (zp_per_channel = 1, zp_dtype =
 * T) with channels = R * K / g groups; table: [n, K] column factors of dtype T on the DEVICE, row i those of candidate i;
 * 1 <= n <= 64; k = K, a multiple of the group size g.  min_val / use_min / thr_div as in the group-wise section.
 * Candidate i, every operation rounding to T, col = flat index mod K:
 *     xs = T(x * table[i][col])
 *     scale (and zp): the statistics -> scale (-> zero-point) chain of bvq_group_quant_fwd (bvq_group_shifted_fwd) on each
 *         group of xs
 *     yq = the forward chain of that entry on xs at (scale, zp), rounding points unchanged
 *     y_i = T(yq / table[i][col])                      the correctly rounded float32 quotient, then rounded to T
 *   y: [n, R, K]; scale: [n, groups]; zp: [n, groups], asymmetric only (null otherwise), all in T.  n * R * K * sizeof(T)
 *   may exceed 4 GiB.  There is no backward: AWQ is applied after training and the layer is frozen afterwards.
 * With n = 1 and factors of one, y, scale and zp have the bits of bvq_group_quant_fwd / bvq_group_shifted_fwd.
 * One launch: x is read once and kept in registers, the factors come from cache, one y is written per candidate; no LDS,
 * no workspace, no atomics.  Covered: what the group-wise entries cover; x, table and y on 16-byte boundaries; K a multiple
 * of g with K * sizeof(T) < 2^31; n as above.  Anything else returns BVQ_ERR_UNSUPPORTED with a bvq_last_error() text,
 * found before anything touches the device; bvq_group_awq_supported answers 1 / 0 (y may be null there: not yet
 * allocated). */
int bvq_group_awq_supported(const bvq_quant_desc* desc, const void* x, const void* table, const void* y, int64_t k,
                            int n);
int bvq_group_awq_fwd(const bvq_quant_desc* desc, const void* x, const void* table, int64_t k, int n, double min_val,
                      int use_min, double thr_div, void* y, void* scale, void* zp, bvq_stream_t stream);

/* ---- asymmetric per-row activations: one scale and one integer zero-point per row, from the row itself ----------------
 * The per-token quantizer of the dynamic activation quantizers (ShiftedUint8DynamicActPerRowFloat).  x is [rows, H],
 * contiguous; the descriptor has outer = 1, channels = rows, inner = H, x_dtype = ct_dtype = scale_dtype = zp_dtype = T,
 * scale_per_channel = zp_per_channel = 1.  min_val / use_min / thr_div as in the group-wise section.  The arithmetic is
 * that of the asymmetric group-wise entries above with "group" read as "row", every operation rounding to T:
 *     mx = max x, mn = min x over the row            (a NaN anywhere in the row is both)
 *     scale = T(clamp_min(|T(mx - mn)|, min_val) / thr_div)
 *     m0 = mn <= 0 ? mn : 0;  zp = clamp(round_half_even(T(T(-m0 / scale) + 0)), qmin, qmax)
 *     q = clamp(round_half_even(T(T(x / scale) + zp)), qmin, qmax);  y = T(T(q - zp) * scale)
 *   bvq_row_shifted_fwd: y like x; scale, zp: [rows] in T; stat: [2 * rows] in T, the maxima then the minima.  A row
 *     with a NaN has NaN scale, zp, stat and y; no other row sees it.
 *   bvq_row_shifted_bwd: the autograd of that graph, as bvq_group_shifted_bwd states it: the row's scale and zero-point
 *     gradients are float32 sums rounded to T, joined by gscale / gzp (nullable, [rows] in T); the gradient of mx is
 *     added to the first element of the row equal to mx, that of mn to the first equal to mn -- first BY POSITION, the
 *     lowest index in the row (-0 equals +0; a NaN statistic is equal to nothing) -- before dx is stored.  stat: the
 *     forward's output; scale and zero-point are derived from it again, same bits.
 * Geometry.  A row is C = H * sizeof(T) / 16 chunks of 16 bytes and is held in registers from its only load to its only
 * store: by one wave for C <= 128 (four rows per 256-thread workgroup, two loads per lane), by one workgroup of four
 * waves for C <= 512 (two loads per lane) and for C <= 2048 (eight).  Lane l of wave w holds chunks j * 64 W + 64 w + l
 * (W waves per row, j the load).  The two ordered keys of the forward, and the two sums and two positions of the
 * backward, cross a wave by xor butterflies and the row's waves through LDS with one barrier.
 * Sum order.  Each of the two float32 sums of the backward adds: in a lane, the terms of its chunks in ascending j,
 * inside a chunk in ascending element pairs, the two terms of an element to the two halves of a pair accumulator, then
 * the halves; across the 64 lanes, the xor butterfly 32, 16, 8, 4, 2, 1; across the row's waves, ((w0 + w1) + w2) + w3.
 * That order depends on H, T and the geometry above alone: the same inputs give the same bits on every run.  Only this
 * ORDER differs from the per-channel kernels, which can move the two deposited elements by a rounding.
 * ONE launch each way: no workspace, no atomics, no arrival words, nothing between workgroups.
 * Covered: T float32, bfloat16 or float16; BVQ_ROUND; BVQ_PRE_NONE; BVQ_OUT_DEQUANT; both clamp modes; every tensor
 * pointer on a 16-byte boundary; H * sizeof(T) any multiple of 16 from 16 up to bvq_row_shifted_max_row_bytes() (32768:
 * 16384 16-bit or 8192 float32 elements); any rows >= 1.  Anything else returns BVQ_ERR_UNSUPPORTED with a
 * bvq_last_error() text, found before anything touches the device; bvq_row_shifted_supported answers 1 / 0 for a
 * descriptor and x. */
int64_t bvq_row_shifted_max_row_bytes(void);
int bvq_row_shifted_supported(const bvq_quant_desc* desc, const void* x);
int bvq_row_shifted_fwd(const bvq_quant_desc* desc, const void* x, double min_val, int use_min, double thr_div,
                        void* y, void* scale, void* zp, void* stat, bvq_stream_t stream);
int bvq_row_shifted_bwd(const bvq_quant_desc* desc, const void* g, const void* x, const void* stat,
                        const void* gscale, const void* gzp, double min_val, int use_min, double thr_div, void* dx,
                        bvq_stream_t stream);

/* ---- weight-normalised weights: per output channel w = g * v / norm(v), quantized with a learned scale ------------------
 * The weight-norm quantizer (L2 norm, half-even rounding) and the accumulator-aware quantizer A2Q (Colbert et al. 2023:
 * L1 norm, round-to-zero, g capped at T * s) of later Brevitas releases; no reference counterpart.  x is the weight
 * viewed [rows, K], contiguous, of dtype T; the descriptor has outer = 1, channels = rows, inner = K, x_dtype = T,
 * ct_dtype = scale_dtype = BVQ_F32, scale_per_channel = 1, zp_per_channel = 0, qmin = -qmax (narrow signed range),
 * round_mode = BVQ_ROUND_TO_ZERO with BVQ_NORM_L1 and BVQ_ROUND with BVQ_NORM_L2.  scale (s > 0), g (> 0), norm, dscale
 * and dg are float32 [rows].  Every operation is a float32 operation, whatever T (x is widened exactly):
 *     n   = norm(x) > norm_min ? norm(x) : norm_min       norm = sum |x_i| (L1) or sqrt(sum x_i^2) (L2)
 *     g'  = g <= T * s ? g : T * s                         T = (float)t_bound; a tie goes to g; +inf never caps
 *     p   = (s * n) / g'                                   two operations, in this order
 *     t_i = x_i / p (IEEE division);  r_i = R(t_i);  q_i = clamp(r_i, -qmax, qmax);  y_i = T(q_i * s)
 *   bvq_weight_norm_fwd: y like x, norm[row] = n.  In real arithmetic sum |q_i| <= sum |t_i| = g' / s <= T for L1.
 *   bvq_weight_norm_bwd, given gy = dL/dy in T and the forward's norm (p, t, r, q are rebuilt with the same bits);
 *   m_i = clamp_ste or not (r_i > qmax or r_i < -qmax):
 *     A = sum gy_i * m_i * t_i;  B = sum gy_i * q_i;  c1 = g' / n;  sA = s * A;  c2 = n > norm_min ? sA / n : 0
 *     dx_i = T(gy_i * m_i * c1 - c2 * sign(x_i))  (L1, sign(0) = 0)   |   T(gy_i * m_i * c1 - (c2 / n) * x_i)  (L2)
 *     dg' = sA / g';  g <= T * s: dscale = B - A, dg = dg';  otherwise: dscale = (B - A) + T * dg', dg = 0
 * Geometry and exchanges are those of the asymmetric per-row entries above: a row of C = K * sizeof(T) / 16 chunks in the
 * registers of one wave (C <= 128) or one workgroup of four waves (C <= 512: two loads per lane, C <= 2048: eight).
 * Sum order (the norm's sum, A and B alike).  In a lane, the terms of its chunks in ascending load j, inside a chunk in
 * ascending element pairs, element 2k to the first and 2k + 1 to the second half of a pair accumulator, then the halves;
 * across the 64 lanes, the xor butterfly 32, 16, 8, 4, 2, 1; across the row's waves, ((w0 + w1) + w2) + w3.  It depends
 * on K, T and the geometry alone: the same inputs give the same bits on every run.
 * ONE launch each way: x (and gy) read once, y (dx) written once; no workspace, no atomics, nothing between workgroups.
 * Covered: T float32, bfloat16 or float16; x, y, gy and dx on 16-byte boundaries; K * sizeof(T) any multiple of 16 from 16
 * up to bvq_row_shifted_max_row_bytes(); any rows >= 1; t_bound > 0 (+inf allowed) and norm_min > 0.  A null descriptor
 * or pointer, an unknown norm kind, t_bound or norm_min not positive: BVQ_ERR_INVALID; anything else not covered:
 * BVQ_ERR_UNSUPPORTED; both with a bvq_last_error() text, found before anything touches the device.
 * bvq_weight_norm_supported answers 1 / 0 for a descriptor, the scalars and x. */
typedef enum bvq_norm_kind { BVQ_NORM_L1 = 0, BVQ_NORM_L2 = 1 } bvq_norm_kind;
int bvq_weight_norm_supported(const bvq_quant_desc* desc, int norm_kind, double t_bound, double norm_min,
                              const void* x);
int bvq_weight_norm_fwd(const bvq_quant_desc* desc, int norm_kind, double t_bound, double norm_min, const void* x,
                        const float* scale, const float* g, void* y, float* norm, bvq_stream_t stream);
int bvq_weight_norm_bwd(const bvq_quant_desc* desc, int norm_kind, double t_bound, double norm_min, const void* gy,
                        const void* x, const float* scale, const float* g, const float* norm, void* dx, float* dscale,
                        float* dg, bvq_stream_t stream);

/* ---- GPTQ: the column loop of one block of up to 128 input columns -----------------------------------------------------
 * GPTQ (Frantar et al. 2022; `gptq_mode` of later Brevitas releases, no reference counterpart) quantizes a weight one
 * input column at a time and pushes each column's error onto the columns not yet quantized.  Definition, which the
 * composed route of brevitas_amd/graph/gptq.py and this kernel compute with the same bits:
 *   W  [R, K] of dtype T (a conv weight flattened to K = in * kh * kw), Wf its float32 working copy,
 *   U  [K, K] float32, the upper Cholesky factor of the damped inverse Hessian of the layer's inputs,
 *   blocks of B = 128 columns (the last may be shorter), group size g dividing K.
 * For each block [c0, c1), for i = c0 .. c1 - 1, for every row r:
 *   group start  if i % g == 0 and the parameters are computed in the loop: scale, zp of (r, i / g) are what
 *                bvq_group_quant_fwd (symmetric) or bvq_group_shifted_fwd (asymmetric) computes for the group
 *                T(Wf[r, i : i + g]) as it stands, partly updated; same min_val, thr_div and rounding points
 *   quantize     q = the value of T those entries store for the element T(Wf[r, i]) at that scale, zp; Q[r, i] = q
 *   error        e = (Wf[r, i] - float32(q)) / U[i, i], float32, IEEE division; E[r, i - c0] = e
 *   update       for j = i + 1 .. c1 - 1: Wf[r, j] = Wf[r, j] - e * U[i, j], the product rounded to float32, then the
 *                difference rounded (no fused multiply-add)
 * and after each block Wf[:, c1:] -= E @ U[c0:c1, c1:] as one float32 matrix product, which is the caller's.
 * bvq_gptq_block runs that loop for ONE block in one launch: one wave per row, the block's columns in registers (two
 * per lane), a group start as a segmented butterfly; no workspace, no atomics.  The kernel is the one column-loop frame
 * of csrc/bvq_column_loop.h, which bvq_gpfq_block below shares, with GPTQ's rule: a rule states what a lane's running
 * state is (here the working copy itself), the value that is quantized, the error and the update right of i; the loop,
 * its parameters, prefetch and stores, and the checks of the entry are the frame's.  It reads the block's columns of wf
 * ([rows, cols] float32) and the [block_cols, block_cols] triangle of u ([cols, cols] float32) and writes the block's
 * columns of q ([rows, cols] of T) and err ([rows, block_cols] float32).  desc: outer 1, channels = rows * cols / g,
 * inner = g, scale_per_channel, x_dtype = ct_dtype = scale_dtype; zp_per_channel = 1 with zp_dtype = x_dtype for an
 * asymmetric quantizer, whose zp is then required.  scale, zp: [rows, cols / g] of T;
 *   computed = 1: the block's entries are WRITTEN; g is 16, 32, 64 or 128 and divides col0 and block_cols;
 *   computed = 0: they are READ (computed once from the original weight by the caller); any g dividing cols.
 * min_val / use_min / thr_div as in bvq_group_quant_fwd (read when computed = 1).
 * Checked before anything touches the device, with a bvq_last_error() text: null pointers (BVQ_ERR_INVALID), wf, u, q or
 * err off a 16-byte boundary and a group size the loop cannot compute (BVQ_ERR_UNSUPPORTED), block_cols outside
 * 1 .. 128, columns outside the weight and a col0 that is no multiple of g where computed (BVQ_ERR_INVALID).
 * bvq_gptq_block_supported answers 1 / 0. */
int bvq_gptq_block_supported(const bvq_quant_desc* desc, int64_t rows, int64_t cols, int64_t col0, int block_cols,
                             int computed, const void* wf, const void* u, const void* q);
int bvq_gptq_block(const bvq_quant_desc* desc, const float* wf, const float* u, int64_t rows, int64_t cols,
                   int64_t col0, int block_cols, int computed, double min_val, int use_min, double thr_div, void* q,
                   float* err, void* scale, void* zp, bvq_stream_t stream);

/* ---- GPFQ: the column loop of one block of up to 128 input columns -----------------------------------------------------
 * GPFQ (greedy path-following quantization: Lybrand & Saab 2021; Zhang, Zhou & Saab 2023; `gpfq_mode` of later Brevitas
 * releases, no reference counterpart) picks each input column's code so that the quantized layer on the quantized
 * path's input X~ follows the float layer on the float input X.  Definition, which the composed route of
 * brevitas_amd/graph/gpfq.py and this kernel compute with the same bits:
 *   W  [R, K] of dtype T (a conv weight flattened to K = in * kh * kw), Wf = float32(W), never changed,
 *   H  [K, K] float32 = mean X~^T X~,   D [K, K] float32 = mean (X - X~)^T X~, one running-mean weighting for both,
 *   C  [R, K] float32, the running correction, C = Wf @ triu(D) (diagonal included) as one float32 matrix product,
 *   scale, zp of the layer's quantizer taken once from W, group size g dividing K; blocks of B = 128 columns.
 * For each block [c0, c1), for i = c0 .. c1 - 1, for every row r:
 *   value        v = Wf[r, i] + C[r, i] / H[i, i] where H[i, i] > 0 (IEEE division, then the sum: two roundings),
 *                else v = Wf[r, i]: a column whose input never fired is rounded to nearest
 *   quantize     q = the value of T that bvq_group_quant_fwd / bvq_group_shifted_fwd store for the element T(v) at the
 *                scale, zp of (r, i / g); Q[r, i] = q
 *   error        e = Wf[r, i] - float32(q), against the original weight, not v; E[r, i - c0] = e
 *   update       for j = i + 1 .. c1 - 1: C[r, j] = C[r, j] + e * H[i, j], the product rounded to float32, then the sum
 *                rounded (no fused multiply-add)
 * and after each block C[:, c1:] += E @ H[c0:c1, c1:] as one float32 matrix product, which is the caller's.
 * (The textbook numerator sum_j w_j <X_j, X~_i> - sum_j q_j <X~_j, X~_i> is the same number and cancels in float32.)
 * bvq_gpfq_block runs that loop for ONE block in one launch: one wave per row, the block's columns of wf and c in
 * registers (two per lane); no workspace, no atomics.  The kernel is the frame of bvq_gptq_block with GPFQ's rule: the
 * running state is c beside the read-only weight, and value, error and update are the three lines above; parameters are
 * given only.  It reads the block's columns of wf and c ([rows, cols] float32),
 * the [block_cols, block_cols] triangle of h ([cols, cols] float32) and scale, zp ([rows, cols / g] of T; zp required for
 * an asymmetric quantizer, else ignored), and writes the block's columns of q ([rows, cols] of T) and err ([rows,
 * block_cols] float32) and nothing else: c is not written.  desc: as for bvq_gptq_block with computed = 0 -- outer 1,
 * channels = rows * cols / g, inner = g (any g dividing cols; a group may have begun before the block),
 * scale_per_channel, x_dtype = ct_dtype = scale_dtype; zp_per_channel = 1 with zp_dtype = x_dtype for an asymmetric
 * quantizer.
 * Checked before anything touches the device, with a bvq_last_error() text: null pointers (BVQ_ERR_INVALID), wf, c, h, q
 * or err off a 16-byte boundary (BVQ_ERR_UNSUPPORTED), block_cols outside 1 .. 128 and columns outside the weight
 * (BVQ_ERR_INVALID).  bvq_gpfq_block_supported answers 1 / 0. */
int bvq_gpfq_block_supported(const bvq_quant_desc* desc, int64_t rows, int64_t cols, int64_t col0, int block_cols,
                             const void* wf, const void* c, const void* h, const void* q);
int bvq_gpfq_block(const bvq_quant_desc* desc, const float* wf, const float* c, const float* h, int64_t rows,
                   int64_t cols, int64_t col0, int block_cols, void* q, float* err, const void* scale, const void* zp,
                   bvq_stream_t stream);

/* ---- Learned rounding: IntQuant with floor(t) + h(value), one trainable offset per element ------------------------------
 * AdaRound (Nagel et al. 2020; LearnedRoundSte of later Brevitas releases, no reference counterpart): the weights are
 * frozen and `value`, shaped like x, is trained.  desc is the descriptor of bvq_fakequant_fwd for x [outer, channels,
 * inner]; T = x_dtype = ct_dtype is also value's dtype; scale and zero-point have one element or `channels` elements
 * each, in scale_dtype / zp_dtype, and scalar_mode, qmin / qmax and clamp_ste mean what they mean there.  Every line is
 * one torch op of the composed route (brevitas_amd/core/function_wrapper/learned_round.py inside IntQuant), rounded to
 * T where torch's device kernel rounds it; c0f = float(c0), c1f = float(c1):
 *   h, BVQ_LR_HARD_SIGMOID (c0 = zeta - gamma, c1 = gamma; Python-float operands enter in float32 opmath):
 *     sg = sigmoid(value) ; m = sg * c0f ; pre = m + c1f ; p = clamp(pre, 0, 1)          hard: p > 0.5
 *   h, BVQ_LR_SIGMOID (c0 = temperature, c1 unused; a division by a host scalar is a multiplication by 1.0f / c0f):
 *     u = value * (1.0f / c0f) ; sg = sigmoid(u) ; p = sg                                hard: value > 0
 *   forward:  t = x / scale ; t = t + zp ; f = floor(t) ; r = f + p (hard: + 0 or 1)
 *             c = where(r > qmax, qmax, r), then where(c < qmin, qmin, c) (a NaN passes) ; y = (c - zp) * scale
 *   backward, given g = dL/dy in T (soft h only):
 *             dc = g * scale ; dr = dc where clamp_ste or not (r > qmax or r < qmin), else 0
 *             dx = dr / scale                                                            (dx nullable: not computed)
 *             hard sigmoid: dp = dr where 0 <= pre <= 1 else 0 ; dp = dp * c0f ; dvalue = sigmoid_backward(dp, sg)
 *             sigmoid:      dvalue = sigmoid_backward(dr, sg) * (1.0f / c0f)
 *   with sigmoid and sigmoid_backward as torch's device kernels compute them (brevitas_amd/csrc/bvq_act.h).  The
 *   products with a host scalar (* c0f, * (1.0f / c0f)) round the float32 product to T.  torch's float16 kernel does so
 *   in its vectorised body only (its tail path rounds the exact product once and returns +0 for a -0 product), so the
 *   Python routing takes these entries for float16 only where the two cannot differ ("Learned rounding").
 *   Gradients of scale and zero-point are not computed.
 * One launch each way: a flat stream of 16-byte lane accesses, no workspace, no atomics, no LDS.  forward reads x and
 * value and writes y; backward reads g, x and value and writes dvalue, and dx when it is given.
 * Covered: float32 / bfloat16 / float16; BVQ_PRE_NONE; BVQ_OUT_DEQUANT; a one-element scale and zero-point on any
 * shape whose bytes are a multiple of 16, or per-channel operands with outer = 1 and inner * sizeof(T) a multiple of 16
 * (a weight [R, K], or the regrouped [R * G, g]); fewer than 2^31 16-byte chunks and 2^30 channels; x, value, y, g, dvalue and dx on
 * 16-byte boundaries.  Anything else returns BVQ_ERR_UNSUPPORTED with a bvq_last_error() text, found before anything
 * touches the device; bvq_learned_round_supported answers 1 / 0 for a descriptor and the forward's tensors. */
typedef enum bvq_learned_round_impl { BVQ_LR_HARD_SIGMOID = 0, BVQ_LR_SIGMOID = 1 } bvq_learned_round_impl;
int bvq_learned_round_supported(const bvq_quant_desc* desc, const void* x, const void* value, const void* y);
int bvq_learned_round_fwd(const bvq_quant_desc* desc, const void* x, const void* value, const void* scale,
                          const void* zp, int impl, double c0, double c1, int hard, void* y, bvq_stream_t stream);
int bvq_learned_round_bwd(const bvq_quant_desc* desc, const void* g, const void* x, const void* value,
                          const void* scale, const void* zp, int impl, double c0, double c1, void* dvalue, void* dx,
                          bvq_stream_t stream);

/* ---- MX block-scaled quantizers: groups sharing one power-of-two scale, minifloat or MXINT8 elements -----------------
 * The OCP Microscaling formats the gfx950 matrix units take natively, as quantize-dequantize for training (no
 * reference counterpart; later Brevitas releases: MXFloat8e4m3Weight, MXFloat8e4m3Act, MXInt8Weight ...).  x is
 * contiguous, dtype T, cut into `groups` groups of `group_size` consecutive elements.  Element formats (exponent bits
 * e, mantissa bits m, emin = 2 - 2^(e-1)):
 *     E4M3 (OCP FP8, no inf)  emax  8, max_val 448      E3M2  emax 4, max_val 28      E2M1  emax 2, max_val 6
 *     E5M2                    emax 15, max_val 57344    E2M3  emax 2, max_val 7.5     INT8  k / 64, |k| <= 127, emax 0
 * Forward, per group, in float32 and exact up to the last step:
 *     a   = max |x_i|; a NaN or Inf: scale and every y_i of the group are NaN
 *     E   = floor(log2 a) - emax (BVQ_MX_FLOOR, the OCP rule; read from a's exponent), + 1 if a > max_val * 2^E
 *           (BVQ_MX_CEIL: the smallest power of two with which nothing saturates); a == 0 counts as -inf; then
 *           clamped to [-126, 127]: the scale is always a normal float32 and the E8M0 code of 2^-127 never arises
 *     p_i = x_i * 2^-E (ldexp)
 *     r_i = p_i rounded half-even to a multiple of 2^(max(floor(log2 |p_i|), emin) - m) (INT8: of 2^-6), sign kept
 *     q_i = clamp(r_i, -max_val, max_val), inside_i = |r_i| <= max_val
 *     y_i = T(q_i * 2^E), scale = 2^E as float32 for every T
 * Backward (g through y; gscale, nullable float32 [groups], through the returned scale), mask_i = inside_i or clamp_ste:
 *     dx_i = g_i * mask_i;  S = sum_i g_i * (q_i - p_i * mask_i) in float32;  da = (gscale + S) * (2^E / a), the floor /
 *     ceil of the exponent taken straight-through, and no da when a == 0, E was clamped or a is not finite;
 *     sign(x_k) * da is added to dx_k at the first k of the group with |x_k| == a.
 * One launch each way on the walk of the group-wise kernels: no workspace, no atomics; the backward recomputes a and E
 * from x.  The order in which a group's float32 terms are added is fixed by the kernel (segmented butterfly).
 * Covered: float32 / bfloat16 / float16; group_size 16, 32, 64, 128 or 256; every tensor pointer on a 16-byte boundary.
 * Anything else returns BVQ_ERR_UNSUPPORTED with a bvq_last_error() text, found before anything touches the device;
 * bvq_mx_quant_supported answers 1 / 0.  The packed element codes and E8M0 scale bytes of the same q_i and E are
 * the "MX wire format" section below (bvq_mx_encode, bvq_mx_decode). */
typedef enum bvq_mx_format {
  BVQ_MX_E4M3 = 0,
  BVQ_MX_E5M2 = 1,
  BVQ_MX_E3M2 = 2,
  BVQ_MX_E2M3 = 3,
  BVQ_MX_E2M1 = 4,
  BVQ_MX_INT8 = 5
} bvq_mx_format;
typedef enum bvq_mx_scale_rule { BVQ_MX_FLOOR = 0, BVQ_MX_CEIL = 1 } bvq_mx_scale_rule;
int bvq_mx_quant_supported(int dtype, int64_t groups, int group_size, int format, const void* x);
int bvq_mx_quant_fwd(int dtype, int64_t groups, int group_size, int format, int scale_rule, const void* x, void* y,
                     void* scale, bvq_stream_t stream);
int bvq_mx_quant_bwd(int dtype, int64_t groups, int group_size, int format, int scale_rule, int clamp_ste,
                     const void* g, const void* x, const void* gscale, void* dx, bvq_stream_t stream);

/* ---- MX wire format: packed element codes and E8M0 scale bytes (OCP Microscaling v1.0) ----------------------------------
 * With q_i and E of the MX section above (its steps unchanged):
 * Scale byte (E8M0), one per group: E + 127, which lies in [1, 254]; 0xFF for a group whose abs-max is NaN or Inf.
 *     Byte 0 (2^-127) is never produced: E is clamped to -126.
 * Element code of q_i: sign bit on top, then the exponent field, then the mantissa field.
 *     format  code width  bias  max_val -> code
 *     E4M3    8 bits       7    448   -> 0x7E
 *     E5M2    8 bits      15    57344 -> 0x7B
 *     E3M2    6 bits       3    28    -> 0x1F
 *     E2M3    6 bits       1    7.5   -> 0x1F
 *     E2M1    4 bits       1    6     -> 0x7
 *     |q_i| below 2^emin is a subnormal code (exponent field 0); the sign of q_i is kept on a zero; the NaN and Inf
 *     codes of E4M3 and E5M2 are never produced.  MXINT8: the two's-complement int8 k = q_i * 64, |k| <= 127; a
 *     negative zero becomes 0.  Every element code of a group that is not finite is 0: its scale byte 0xFF makes the
 *     block NaN.
 * Packing, in memory order, with the group boundaries of the fake-quantizer:
 *     8-bit formats  one byte per element
 *     E2M1           two elements per byte: element 2j in bits 0-3, element 2j + 1 in bits 4-7
 *     E3M2, E2M3     a dense little-endian bit stream: element j of the tensor occupies bits [6j, 6j + 6), so 4
 *                    elements fill 3 bytes and a group of 32 fills 24
 *     A tensor of n elements gives n * bits / 8 code bytes and n / group_size scale bytes.
 * Decode is the inverse on ANY byte pattern, not only those the encoder emits: scale byte 0 reads as 2^-127 and 0xFF
 * makes every element of the group NaN; the E4M3 codes 0x7F and 0xFF read as NaN; E5M2 codes with exponent field 31
 * read as +-Inf (mantissa 0) or NaN; MXINT8 -128 reads as -2.0.  y_i = T(v_i * 2^E) with the product in float32; it is
 * exact (v_i has at most 7 significant bits, and the smallest magnitude of any format times 2^-127 is 2^-143).  On the
 * encoder's own output the result is therefore the y of bvq_mx_quant_fwd bit for bit, with two exceptions: a NaN equals
 * any NaN, and a negative zero of MXINT8 comes back positive.
 * bvq_mx_encode: one launch on the walk of bvq_mx_quant_fwd with the same arithmetic for E and q_i; x is read once, the
 * codes and the scale bytes are written once (16-byte and dword stores assembled across lanes; byte stores only for a
 * last scale dword that the tensor ends inside), nothing is written past n * bits / 8 code bytes and `groups` scale
 * bytes; no workspace, no atomics.  bvq_mx_decode: one launch, codes and scale bytes -> y of dtype T.
 * Covered, both ways: float32 / bfloat16 / float16; group_size 16, 32, 64, 128 or 256; x, codes, scale_e8m0 and y on
 * 16-byte boundaries.  Anything else returns BVQ_ERR_UNSUPPORTED with a bvq_last_error() text, found before anything
 * touches the device; bvq_mx_encode_supported answers 1 / 0. */
int bvq_mx_encode_supported(int dtype, int64_t groups, int group_size, int format, const void* x);
int bvq_mx_encode(int dtype, int64_t groups, int group_size, int format, int scale_rule, const void* x, void* codes,
                  void* scale_e8m0, bvq_stream_t stream);
int bvq_mx_decode(int dtype, int64_t groups, int group_size, int format, const void* codes, const void* scale_e8m0,
                  void* y, bvq_stream_t stream);

/* ---- Hadamard transform: y = scale * (I (x) H_b) x along the last dimension ---------------------------------------------
 * The online rotation of QuaRot / SpinQuant style quantization (brevitas_amd.function.hadamard, nn.RotatedModule) and
 * the product of the reference's HadamardClassifier (B/nn/hadamard_classifier.py, a dense matrix there).  x is
 * [rows, cols] of dtype T, contiguous; block (b) is a power of two, 2 <= b <= cols, b | cols; H_b is the Sylvester
 * (natural-order) +-1 matrix.  Definition, which the composed route of brevitas_amd/_aten.py and this kernel compute with
 * the same bits:
 *   1. every element is widened to float32;
 *   2. stages h = 1, 2, 4 .. b / 2 in this ascending order; in a stage every pair (i, i + h) with (i & h) == 0 inside a
 *      block becomes (u + v, u - v), u the value at i and v the value at i + h, each one correctly rounded float32
 *      addition or subtraction;
 *   3. one float32 multiply by (float)scale;
 *   4. one rounding to T (nearest even).
 * Intermediates are float32 from the load to the multiply, through LDS as well.  The transform is symmetric: its
 * gradient is the same call on the incoming gradient.
 * Geometry: the row walk of the per-row entries above -- a row of C = cols * sizeof(T) / 16 chunks in the registers of
 * one wave (C <= 128) or one workgroup of four waves (C <= 512: two loads per lane, C <= 2048: eight), lane l of wave w
 * holding chunks j * 64 W + 64 w + l.  The bits of an element's index are, from the low end, its place in the chunk, the
 * lane, the wave, the load j; the stages of the first and last class are register arithmetic, the six lane stages
 * cross-lane exchanges on the VALU (DPP moves, v_permlane16_swap / v_permlane32_swap), the two wave stages ONE exchange through LDS per load (two alternating float32 slices of one load,
 * 16 KiB per workgroup for the 16-bit types and 8 KiB for float32, one barrier per load).  A smaller block stops the
 * sequence early.  A row is whole in registers between its only load and its only store, so y may be x.
 * ONE launch: x read once, y written once; no workspace, no atomics, nothing between workgroups.
 * Covered: T float32, bfloat16 or float16; cols * sizeof(T) a multiple of 16 up to 32768 (a longer last dimension is the
 * caller's to view as [rows * H / c, c], b | c | H: the transform is block-diagonal); x and y on 16-byte boundaries.  A
 * bad dtype, rows or cols < 1, a block that is no power of two >= 2 or does not divide cols, a null pointer:
 * BVQ_ERR_INVALID; a row length or an alignment not covered: BVQ_ERR_UNSUPPORTED; both with a bvq_last_error() text,
 * found before anything touches the device.  bvq_hadamard_supported answers 1 / 0. */
int bvq_hadamard_supported(int dtype, int64_t rows, int64_t cols, int64_t block, const void* x, const void* y);
int bvq_hadamard(int dtype, const void* x, int64_t rows, int64_t cols, int64_t block, double scale, void* y,
                 bvq_stream_t stream);

/* Diagnostic entry (no reference counterpart): the float32 quotient the float16 quantizer kernels compute for a
 * numerator a[i] and a scale scales[j] -- the product with the correctly rounded reciprocal, corrected by one exact
 * remainder step (brevitas_amd/csrc/bvq_fakequant.h, DivF16R) -- out[j * n_a + i], float32 device buffers.  The
 * tests compare every float16 numerator x every float16 scale in [2^-14, 2^14] with a / s (tests/test_gpu_fastdiv.py). */
int bvq_selftest_div_f16r(const float* a, int32_t n_a, const float* scales, int32_t n_s, float* out,
                          bvq_stream_t stream);

/* Diagnostic entry (no reference counterpart): the fused activation pre_op (BVQ_PRE_SIGMOID / BVQ_PRE_TANH) as the
 * quantizer kernels compute it, element by element on n elements of dtype: act_out[i] = act(x[i]) and
 * dact_out[i] = act_backward(g[i], act_out[i]), both rounded to dtype, so that the tests can compare them with
 * torch.sigmoid / torch.tanh and their autograd on the device. */
int bvq_selftest_pre_op(int pre_op, int dtype, const void* x, const void* g, void* act_out, void* dact_out, int64_t n,
                        bvq_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* BVQ_H_ */
