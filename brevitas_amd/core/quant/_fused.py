"""Autograd entry points of the fused quantizer kernels.

FakeQuantFn        x, scale, zero_point  ->  y                  (IntQuant.forward in one kernel)
StatsFakeQuantFn   x                     ->  y, scale, stat     (AbsMax -> scale -> IntQuant in
                                                                 three kernels, backward with the
                                                                 arg-max deposit folded into dx)

Both reproduce the reference's type promotion: the compute dtype is torch.result_type(x, scale),
every intermediate is rounded to it, the output has it, and the gradient w.r.t. x comes back in
x's dtype.  Layouts the kernels do not cover make `plan()` return None and the caller falls back
to the op-by-op composition (same results, more passes).
"""
import math
from typing import NamedTuple, Optional

import torch
from torch import Tensor
from torch.autograd import Function

import brevitas_amd.config as config
from brevitas_amd import _native as nat

_FLOATS = (torch.float32, torch.bfloat16, torch.float16)


class Plan(NamedTuple):
    outer: int
    channels: int
    inner: int
    scale_pc: bool
    zp_pc: bool
    ct: torch.dtype
    nhwc: bool = False  # x is a dense channels_last tensor taken in memory order: [N*H*W, C] rows, channel last


def is_nhwc(x: Tensor, channel_dim) -> bool:
    """per-channel (dim 1) quantization of a dense channels_last tensor: its memory IS [N*H*W, C], which the
    column-mapped kernels take as it lies (no NCHW copy and back)"""
    return channel_dim == 1 and x.dim() == 4 and not x.is_contiguous() \
        and x.is_contiguous(memory_format=torch.channels_last)


def split_at_channel(x: Tensor, cd: int):
    """x as [outer, channels, inner] around its dim `cd` -> (outer, channels, inner, nhwc); nhwc: see Plan.nhwc"""
    if is_nhwc(x, cd):
        return x.numel() // x.shape[1], x.shape[1], 1, True
    return math.prod(x.shape[:cd]), x.shape[cd], math.prod(x.shape[cd + 1:]), False


def _channel_dim(x: Tensor, t: Tensor):
    """None: one element (per-tensor); int: the single broadcast dim; -1: not a per-channel layout"""
    if t.numel() == 1:
        return None
    if t.dim() > x.dim():
        return -1
    shape = (1,) * (x.dim() - t.dim()) + tuple(t.shape)
    nz = [i for i, s in enumerate(shape) if s != 1]
    if len(nz) != 1 or shape[nz[0]] != x.shape[nz[0]]:
        return -1
    return nz[0]


def plan(x: Tensor, scale: Tensor, zp: Tensor) -> Optional[Plan]:
    """how (and whether) the fused kernels can run IntQuant on these operands"""
    if not (x.is_cuda and scale.is_cuda and zp.is_cuda) or x.dim() == 0 or x.numel() == 0:
        return None
    if x.dtype not in _FLOATS or scale.dtype not in _FLOATS or zp.dtype not in _FLOATS:
        return None
    if scale.dim() > x.dim() or zp.dim() > x.dim():
        return None
    sd, zd = _channel_dim(x, scale), _channel_dim(x, zp)
    if sd == -1 or zd == -1 or (sd is not None and zd is not None and sd != zd):
        return None
    ct = torch.result_type(x, scale)
    # a 0-dim zero-point never promotes a dimensioned tensor; a dimensioned one must not either
    if zp.dim() > 0 and torch.promote_types(ct, zp.dtype) != ct:
        return None
    if not (ct == x.dtype or ct == torch.float32):
        return None
    cd = sd if sd is not None else zd
    if cd is None:
        return Plan(1, 1, x.numel(), False, False, ct)
    outer, channels, inner, nhwc = split_at_channel(x, cd)
    return Plan(outer, channels, inner, sd is not None, zd is not None, ct, nhwc)


_ACT_OPS = {nat.PRE_RELU: torch.relu, nat.PRE_SIGMOID: torch.sigmoid, nat.PRE_TANH: torch.tanh}
ACT_PRE_OPS = (nat.PRE_SIGMOID, nat.PRE_TANH)  # the activations of csrc/bvq_act.h


def apply_pre_op(x: Tensor, pre_op: int) -> Tensor:
    """the activation `pre_op` (include/bvq.h, bvq_pre_op) as its own torch op: the route where it is not fused"""
    if pre_op == nat.PRE_NONE:
        return x
    return _ACT_OPS[pre_op](x)


def act_fusable(x: Tensor, p: Optional['Plan'], pre_op: int) -> bool:
    """sigmoid / tanh fold into the row-mapped quantizer kernels: dequantized output in x's dtype, no column-mapped
    (channels_last per-channel) layout, a dtype whose activation the kernels reproduce (act_dtype_ok)"""
    # x off a 16-byte boundary: the kernels would tile it (and add up the scale gradient) unlike the fresh, aligned
    # activation tensor of the materialised route
    return act_dtype_ok(x, pre_op) and p is not None and not p.nhwc and p.ct == x.dtype and x.data_ptr() % 16 == 0


def act_dtype_ok(x: Tensor, pre_op: int) -> bool:
    """the kernels' activation and its backward equal torch's for x's dtype: sigmoid in every dtype, tanh in float32
    (torch's 16-bit tanh / tanh_backward are not reproduced on every input)"""
    return pre_op != nat.PRE_TANH or x.dtype == torch.float32


def scalar_mode():
    return nat.SCALAR_CAST if config.SCALAR_OPERAND_MODE == 'device' else nat.SCALAR_OPMATH


def make_desc(p: Plan, x: Tensor, scale: Tensor, zp: Tensor, qmin, qmax, round_mode, clamp_ste, out_kind,
              pre_op=nat.PRE_NONE):
    """the descriptor of a Plan: dtypes from the operands, the compute dtype from the plan"""
    return nat.QuantDesc(outer=p.outer, channels=p.channels, inner=p.inner, x_dtype=nat.dtype_code(x.dtype),
                         ct_dtype=nat.dtype_code(p.ct), scale_dtype=nat.dtype_code(scale.dtype),
                         zp_dtype=nat.dtype_code(zp.dtype), scale_per_channel=int(p.scale_pc),
                         zp_per_channel=int(p.zp_pc), qmin=qmin, qmax=qmax, round_mode=round_mode,
                         scalar_mode=scalar_mode(), clamp_ste=int(clamp_ste), out_kind=out_kind, pre_op=pre_op)


def channel_desc(outer, channels, inner, dtype, qmin, qmax, round_mode, clamp_ste, scale_dtype=None,
                 zp_dtype=torch.float32, scale_pc=True, zp_pc=False, pre_op=nat.PRE_NONE):
    """the descriptor of the statistic-scaled kernels: x of `dtype` as [outer, channels, inner], computed and dequantized
    in that dtype, one scale per channel (or group) in `scale_dtype` (x's unless named), a zero zero-point (0-dim
    float32) unless zp_dtype / zp_pc say one per channel"""
    code = nat.dtype_code(dtype)
    return nat.QuantDesc(outer=outer, channels=channels, inner=inner, x_dtype=code, ct_dtype=code,
                         scale_dtype=code if scale_dtype is None else nat.dtype_code(scale_dtype),
                         zp_dtype=nat.dtype_code(zp_dtype), scale_per_channel=int(scale_pc), zp_per_channel=int(zp_pc),
                         qmin=qmin, qmax=qmax, round_mode=round_mode, scalar_mode=scalar_mode(),
                         clamp_ste=int(clamp_ste), out_kind=nat.OUT_DEQUANT, pre_op=pre_op)


def _reduce_like(sums: Tensor, like: Tensor) -> Tensor:
    """per-channel float32 sums -> gradient shaped and typed like `like`"""
    if like.numel() == 1 and sums.numel() > 1:
        sums = sums.sum()
    return sums.reshape(like.shape).to(like.dtype)


def _memory_order(x: Tensor, channels: int, nhwc: bool = False):
    """-> (contiguous tensor holding x's elements, permutation that maps a same-ordered result back to x's
    logical layout or None).  A per-tensor quantizer does not care about element order, so a dense
    channels_last tensor (the layout MIOpen prefers) is taken as it lies in memory instead of being copied to
    NCHW and back; every other case is `x.contiguous()` like the reference's own reshape."""
    if nhwc:
        return x.permute(0, 2, 3, 1), (0, 3, 1, 2)
    if x.is_contiguous() or channels != 1:
        return x.contiguous(), None
    if x.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last):
        return x.permute(0, 2, 3, 1), (0, 3, 1, 2)
    if x.dim() == 5 and x.is_contiguous(memory_format=torch.channels_last_3d):
        return x.permute(0, 2, 3, 4, 1), (0, 4, 1, 2, 3)
    return x.contiguous(), None


def _like_memory_order(t: Tensor, back) -> Tensor:
    """bring an incoming gradient into the element order the forward used"""
    if back is None:
        return t.contiguous()
    inv = [0] * len(back)
    for i, b in enumerate(back):
        inv[b] = i
    return t.permute(inv).contiguous()


def _restore(t: Tensor, back) -> Tensor:
    return t if back is None else t.permute(back)


def _quantize(p: Plan, xc: Tensor, back, scale: Tensor, zp: Tensor, qmin, qmax, round_mode, clamp_ste, out_kind, pre_op):
    """the quantizer kernel on xc = _memory_order(x)[0] -> (descriptor, y in x's logical layout)"""
    sc = scale.reshape(-1).contiguous()
    zc = zp.reshape(-1).contiguous()
    desc = make_desc(p, xc, sc, zc, qmin, qmax, round_mode, clamp_ste, out_kind, pre_op)
    return desc, _restore(nat.fakequant_fwd(desc, xc, sc, zc), back)


def _incoming(gy: Optional[Tensor], desc, xc: Tensor, back) -> Tensor:
    """y's gradient as the backward kernels take it: in the compute dtype and the forward's element order; zeros when
    none arrived (only `scale` was used downstream)"""
    ct = nat.TORCH_DTYPES[desc.ct_dtype]
    if gy is None:
        return torch.zeros(xc.shape, dtype=ct, device=xc.device)
    return _like_memory_order(gy.to(ct), back)


class FakeQuantFn(Function):
    """IntQuant.forward / IntQuant.to_int on the fused kernel (B/core/quant/int_base.py:63-97)"""

    @staticmethod
    def forward(ctx, x, scale, zp, p, qmin, qmax, round_mode, clamp_ste, out_kind, pre_op=nat.PRE_NONE):
        xc, back = _memory_order(x, p.channels, p.nhwc)
        desc, y = _quantize(p, xc, back, scale, zp, qmin, qmax, round_mode, clamp_ste, out_kind, pre_op)
        ctx.desc = desc
        ctx.back = back
        ctx.save_for_backward(xc, scale, zp)
        if out_kind == nat.OUT_INT:
            ctx.mark_non_differentiable(y)
        return y

    @staticmethod
    def backward(ctx, gy):
        xc, scale, zp = ctx.saved_tensors
        desc = ctx.desc
        need_ds, need_dz = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        gy = _incoming(gy, desc, xc, ctx.back)
        dx, ds, dz = nat.fakequant_bwd(desc, gy, xc, scale.reshape(-1).contiguous(), zp.reshape(-1).contiguous(),
                                       need_ds, need_dz)
        if ctx.back is not None:
            dx = dx.permute(ctx.back)
        ds = _reduce_like(ds, scale) if need_ds else None
        dz = _reduce_like(dz, zp) if need_dz else None
        return dx, ds, dz, None, None, None, None, None, None, None


class FakeQuantBoundsFn(Function):
    """IntQuant.forward whose integer range is a pair of 0-dim TENSORS (a learned bit width: min_int / max_int of the
    bit-width tensor, B/core/bit_width/parameter.py:23-100, B/function/ops.py:132-191): the fused kernels read the
    bounds from device memory, and the backward returns, next to dx and dscale, the gradient tensor_clamp's two
    torch.where send to the bounds (plain TensorClamp only; a straight-through clamp gives the bounds none)."""

    @staticmethod
    def forward(ctx, x, scale, zp, qmin_t, qmax_t, p, round_mode, clamp_ste, pre_op):
        xc, back = _memory_order(x, p.channels, p.nhwc)
        sc = scale.reshape(-1).contiguous()
        zc = zp.reshape(-1).contiguous()
        bounds = torch.stack([qmin_t.detach().reshape(()), qmax_t.detach().reshape(())]).float()
        desc = make_desc(p, xc, sc, zc, 0.0, 0.0, round_mode, clamp_ste, nat.OUT_DEQUANT, pre_op)
        y = nat.fakequant_fwd_bounds(desc, xc, sc, zc, bounds)
        ctx.desc, ctx.back = desc, back
        ctx.save_for_backward(xc, scale, zp, bounds, qmin_t, qmax_t)
        return y if back is None else y.permute(back)

    @staticmethod
    def backward(ctx, gy):
        xc, scale, zp, bounds, qmin_t, qmax_t = ctx.saved_tensors
        desc = ctx.desc
        gy = _incoming(gy, desc, xc, ctx.back)
        need_db = (ctx.needs_input_grad[3] or ctx.needs_input_grad[4]) and not desc.clamp_ste
        dx, ds, db = nat.fakequant_bwd_bounds(desc, gy, xc, scale.reshape(-1).contiguous(), zp.reshape(-1).contiguous(),
                                              bounds, need_db)
        dx = _restore(dx, ctx.back) if ctx.needs_input_grad[0] else None
        ds = _reduce_like(ds, scale) if ctx.needs_input_grad[1] else None
        dmin = dmax = None
        if need_db:
            # the reference sums where()'s masked gradient in the clamp's dtype, then casts to the bound's
            sums = db.sum(dim=1).to(gy.dtype)
            dmin = sums[0].to(qmin_t.dtype).reshape(qmin_t.shape) if ctx.needs_input_grad[3] else None
            dmax = sums[1].to(qmax_t.dtype).reshape(qmax_t.shape) if ctx.needs_input_grad[4] else None
        return dx, ds, None, dmin, dmax, None, None, None, None


class LearnedScaleFakeQuantFn(Function):
    """scale = |clamp_min(value, min_val)| / int_threshold  ->  IntQuant with that scale and a zero zero-point:
    the steady state of the learned-scale activation quantizers (ParameterScaling, and
    ParameterFromRuntimeStatsScaling after its collection phase -- the default Int8ActPerTensorFloat;
    B/core/scaling/standalone.py:75-152,155-298, B/core/quant/int.py:157-163).

    Forward: one launch for the scale (instead of clamp, |.|, division), the quantizer kernel.  Backward: the
    quantizer's backward kernel, its scale-gradient sums, and -- in the LAST reduction launch -- the chain
    dscale -> d(threshold) -> d(value) with torch's rounding points (instead of a cast, a division, a
    sign-multiply and their launches).  Returns (y, scale)."""

    @staticmethod
    def forward(ctx, x, value, p, min_val, thr_div, scale_dtype, qmin, qmax, round_mode, clamp_ste, pre_op):
        ctx.set_materialize_grads(False)
        xc, back = _memory_order(x, p.channels, p.nhwc)
        sc = nat.learned_scale(value, min_val, thr_div, scale_dtype)
        zp = _zero_zero_point(x.device)
        desc, y = _quantize(p, xc, back, sc, zp, qmin, qmax, round_mode, clamp_ste, nat.OUT_DEQUANT, pre_op)
        ctx.desc, ctx.back, ctx.args = desc, back, (min_val, thr_div)
        ctx.save_for_backward(xc, sc, zp, value)
        return y, sc.view(value.shape)

    @staticmethod
    def backward(ctx, gy, gscale):
        xc, sc, zp, value = ctx.saved_tensors
        desc = ctx.desc
        min_val, thr_div = ctx.args
        if gy is None:  # only `scale` was used downstream: its own small autograd chain, no tensor pass
            if gscale is None:
                return (None,) * 11
            v = value.detach()
            if min_val:
                v = torch.clamp_min(v, min_val)
            sign = torch.ge(v, 0.0).to(v.dtype) - torch.lt(v, 0.0).to(v.dtype)
            return None, (sign * (gscale.reshape(value.shape) / thr_div).to(v.dtype)), *(None,) * 9
        gy = _incoming(gy, desc, xc, ctx.back)
        gs = gscale.reshape(-1).contiguous().to(sc.dtype) if gscale is not None else None
        dx, _, dvalue = nat.fakequant_bwd_learned(desc, gy, xc, sc, zp.reshape(-1), value, min_val, thr_div, gs)
        if not ctx.needs_input_grad[0]:
            dx = None
        elif ctx.back is not None:
            dx = dx.permute(ctx.back)
        return dx, dvalue.view(value.shape), None, None, None, None, None, None, None, None, None


class LearnedRoundFakeQuantFn(Function):
    """IntQuant whose float_to_int_impl is a LearnedRoundSte (core/function_wrapper/learned_round.py): x, value -> y, one
    launch each way (csrc/bvq_learned_round.hip).  Returns dvalue, and dx when x asks for it; scale, zero-point and bit
    width get no gradient here -- the caller has checked that none wants one, and what the kernels cover
    (IntQuant._learned_round_args).  hard: eval mode, h(value) is 0 or 1 and nothing is differentiable."""

    @staticmethod
    def forward(ctx, x, value, scale, zp, p, qmin, qmax, clamp_ste, kind, consts, hard):
        sc = scale.detach().reshape(-1).contiguous()
        zc = zp.detach().reshape(-1).contiguous()
        desc = make_desc(p, x, sc, zc, qmin, qmax, nat.FLOOR, clamp_ste, nat.OUT_DEQUANT)
        y = nat.learned_round_fwd(desc, x, value, sc, zc, kind, consts, hard)
        if hard:
            ctx.mark_non_differentiable(y)
        else:
            ctx.desc, ctx.kind, ctx.consts = desc, kind, consts
            ctx.save_for_backward(x, value, sc, zc)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, value, sc, zc = ctx.saved_tensors
        gy, _ = _group_grads(x, gy, [])
        dvalue, dx = nat.learned_round_bwd(ctx.desc, gy, x, value, sc, zc, ctx.kind, ctx.consts,
                                           ctx.needs_input_grad[0])
        return (dx, dvalue.view(value.shape) if ctx.needs_input_grad[1] else None) + (None,) * 9


class VariantFn(Function):
    """BinaryQuant / ClampedBinaryQuant / TernaryQuant / DecoupledIntQuant / TruncIntQuant on their fused kernels
    (include/bvq.h, bvq_variant_fwd / bvq_variant_bwd): one read + one write forward, two reads + one write backward,
    the scale gradients on the same reads.  `opts`: kind plus the kind's parameters (variant_plan below)."""

    @staticmethod
    def forward(ctx, x, scale, pre_scale, zp, pre_zp, p, opts):
        xc = x.contiguous()
        sc = scale.reshape(-1).contiguous()
        ps = pre_scale.reshape(-1).contiguous() if pre_scale is not None else None
        zc = zp.reshape(-1).contiguous() if zp is not None else None
        pz = pre_zp.reshape(-1).contiguous() if pre_zp is not None else None
        zdt = (zc if zc is not None else pz if pz is not None else _zero_zero_point(x.device)).dtype
        desc = nat.VariantDesc(p.outer, p.channels, p.inner, opts['kind'], nat.dtype_code(x.dtype),
                               nat.dtype_code(opts['ct']), nat.dtype_code(sc.dtype), nat.dtype_code(zdt), int(p.scale_pc),
                               opts.get('round_mode', nat.ROUND), int(opts.get('clamp_ste', False)), scalar_mode(),
                               opts.get('qmin', 0.0), opts.get('qmax', 0.0), opts.get('threshold', 0.0),
                               opts.get('trunc_scale', 1.0))
        y = nat.variant_fwd(desc, xc, sc, ps, zc, pz)
        ctx.desc = desc
        ctx.save_for_backward(xc, sc, ps, zc, pz)
        ctx.shapes = (scale.shape, scale.dtype, None if pre_scale is None else (pre_scale.shape, pre_scale.dtype))
        return y

    @staticmethod
    def backward(ctx, gy):
        xc, sc, ps, zc, pz = ctx.saved_tensors
        desc = ctx.desc
        need_ds, need_dp = ctx.needs_input_grad[1], ctx.needs_input_grad[2] and ps is not None
        dx, ds, dp = nat.variant_bwd(desc, _incoming(gy, desc, xc, None), xc, sc, ps, zc, pz, need_ds, need_dp)
        sshape, sdt, pre = ctx.shapes
        ds = ds.reshape(sshape).to(sdt) if need_ds else None
        dp = dp.reshape(pre[0]).to(pre[1]) if need_dp else None
        return (dx if ctx.needs_input_grad[0] else None), ds, dp, None, None, None, None


def _dimensioned_wider_scalar(x: Tensor, t: Optional[Tensor]) -> bool:
    """a ONE-element operand that still has dimensions (shape (1,), (1,1,1,1)) and a dtype wider than x's: torch's type
    promotion treats it as a tensor, not as a scalar -- every op with it computes and returns in ITS dtype -- while the
    variant kernels' one-element operands follow the 0-dim rule (rounded to x's dtype, bvq_scalar_mode).  Such operands
    take the op-by-op route."""
    return t is not None and t.numel() == 1 and t.dim() > 0 and torch.promote_types(x.dtype, t.dtype) != x.dtype


def variant_plan(x: Tensor, scale: Tensor, *others: Optional[Tensor]) -> Optional[Plan]:
    """layout plan for a variant kernel: x against `scale`; every other scale-like operand must share scale's shape
    and dtype, every zero-point must be a single element that needs no gradient"""
    if not config.FUSED_PATHS or torch._C._get_tracing_state() is not None:
        return None
    if _dimensioned_wider_scalar(x, scale):
        return None
    p = plan(x, scale, _zero_zero_point(x.device) if x.is_cuda else scale)
    if p is None or p.nhwc or not x.is_contiguous():
        return None
    for t in others:
        if t is not None and (t.shape != scale.shape or t.dtype != scale.dtype or not t.is_cuda):
            return None
    return p


def scalar_zero_point_ok(*zps: Optional[Tensor], x: Optional[Tensor] = None) -> bool:
    """x given: also refuse a dimensioned one-element zero-point that would promote x (see _dimensioned_wider_scalar)"""
    return all(z is None or (z.numel() == 1 and z.is_cuda and z.dtype in _FLOATS and not z.requires_grad
                             and not (x is not None and _dimensioned_wider_scalar(x, z))) for z in zps)


class StatsPlan(NamedTuple):
    outer: int
    channels: int
    inner: int
    scaling_shape: tuple
    min_val: float
    int_threshold: float  # host value of int_scaling_impl(bit_width)
    nhwc: bool = False    # see Plan.nhwc


_ZERO_ZP = {}


def _zero_zero_point(device):
    """the 0-dim float32 zero the ZeroZeroPoint module returns, one per device (no fill kernel per call)"""
    z = _ZERO_ZP.get(device)
    if z is None:
        z = torch.zeros((), dtype=torch.float32, device=device)
        _ZERO_ZP[device] = z
    return z


_AS_DTYPE = {}


def _as_dtype_value(v: float, dtype: torch.dtype) -> float:
    """v after torch converts it to `dtype` (what a 0-dim float32 operand becomes next to a dimensioned
    tensor of that dtype on the device)"""
    key = (v, dtype)
    r = _AS_DTYPE.get(key)
    if r is None:
        r = _AS_DTYPE[key] = float(torch.tensor(v, dtype=torch.float32).to(dtype))
    return r


class ScaleRule(NamedTuple):
    scale_dtype: torch.dtype  # of scale = stat / int_threshold
    thr_div: float            # the value that division divides by
    quot_dtype: torch.dtype   # of the backward's dscale / int_threshold
    thr_bwd: float            # the value that one divides by


def scale_rule(dtype: torch.dtype, scaling_shape, int_threshold: float, thr_dtype: torch.dtype = torch.float32,
               thr_as_stored: bool = False) -> ScaleRule:
    """torch's type promotion in `t / int_threshold`, t of `dtype` and shaped `scaling_shape` (forward: the statistic,
    which has x's dtype; backward: the scale's gradient, which has the scale's), int_threshold the 0-dim tensor of
    `thr_dtype` whose host value is given.  A dimensioned t keeps its dtype and the threshold is converted to it; a
    0-dim t promotes with the threshold's dtype.  The 0-dim case divides by the host value as it is on the
    statistic-scaled routes, and by that value as `thr_dtype` holds it where `thr_as_stored` (the learned-scale route,
    whose int_threshold has the bit width's dtype): equal unless the threshold is not representable in thr_dtype
    (32767 next to a bfloat16 bit width), so each route keeps its own."""
    if len(scaling_shape) > 0:
        thr = _as_dtype_value(int_threshold, dtype)
        return ScaleRule(dtype, thr, dtype, thr)
    scale_dtype = torch.promote_types(dtype, thr_dtype)
    thr = _as_dtype_value(int_threshold, thr_dtype) if thr_as_stored else int_threshold
    return ScaleRule(scale_dtype, thr, torch.promote_types(scale_dtype, thr_dtype), thr)


def _running_buffer(runtime, channels: int) -> Optional[Tensor]:
    """the running-statistic buffer of a _RuntimeStats when the kernels can fold the statistic into it (a plain
    [channels] device tensor), else None; None for no runtime"""
    if runtime is None:
        return None
    buf = runtime.running_stats
    return buf if buf.is_cuda and buf.is_contiguous() and buf.numel() == channels and buf.dtype in _FLOATS else None


def stats_scale(flat: Tensor, int_threshold: Tensor, sp, group, pre_op, running=None):
    """AbsMax statistic of the [outer, channels, inner] tensor `flat` and the scale derived from it:
    -> (stat [channels] in x's dtype, scale shaped sp.scaling_shape).  group: the tensor is one batch shard.
    running: (buffer, momentum, first_batch) of a _RuntimeStats to fold the statistic into in the same launch
    (sharded: the statistic -> scale launch behind the all-reduce)."""
    rule = scale_rule(flat.dtype, sp.scaling_shape, sp.int_threshold, int_threshold.dtype)
    fold = {} if running is None else dict(zip(('running', 'momentum', 'first_batch'), running))
    if group is None:
        # statistic -> clamp_min -> / int_threshold in the reduction's own finishing launch
        stat, scale = nat.absmax_scale(flat, sp.outer, sp.channels, sp.inner, sp.min_val, rule.thr_div,
                                       rule.scale_dtype, pre_op, **fold)
    else:
        # batch-sharded tensor: the statistic of the whole batch is the max over the shards, then the same in one launch
        from brevitas_amd.distributed import sync_stat_max
        stat32 = sync_stat_max(nat.stats(nat.STAT_ABSMAX, flat, sp.outer, sp.channels, sp.inner, out_f32=True,
                                         pre_op=pre_op), group)
        stat, scale = nat.scale_from_stat(stat32, flat.dtype, sp.min_val, rule.thr_div, rule.scale_dtype, **fold)
    return stat, scale.view(sp.scaling_shape)


class StatsFakeQuantFn(Function):
    """AbsMax statistic -> clamp_min(min_val) -> / int_threshold -> IntQuant, zero zero-point.

    The resolved graphs of Int8WeightPerChannelFloat (StatsFromParameterScaling) and of stats-scaled
    activations (RuntimeStatsScaling in training): SURVEY 8a.  Forward: read x (reduce), read x, write
    y.  Backward: read g, read x, write dx; the statistic's gradient is deposited on the arg-max
    element(s) of dx in place instead of materialising the dense gradient torch.max would return.
    """

    @staticmethod
    def forward(ctx, x, int_threshold, sp, qmin, qmax, round_mode, clamp_ste, group=None, pre_op=nat.PRE_NONE,
                runtime=None):
        ctx.set_materialize_grads(False)  # an unused `scale` output must not cost a zero-fill + add
        ctx.pre_op = pre_op
        xc, back = _memory_order(x, sp.channels, sp.nhwc)
        ctx.back = back
        zp = _zero_zero_point(x.device)
        # _RuntimeStats' running average rides on the launch that finishes the statistic when its buffer is a plain
        # [channels] device tensor (the module is told through `bvq_running_folded`)
        running = _running_buffer(runtime, sp.channels)
        fused = None
        if group is None and config.FUSED_PATHS and x.dtype in _FLOATS:
            # one launch: the channel stays in registers between the reduction and the quantization
            # (x is read once).  Covers channels that fit a team's registers; None otherwise.
            rule = scale_rule(x.dtype, sp.scaling_shape, sp.int_threshold, int_threshold.dtype)
            desc = channel_desc(sp.outer, sp.channels, sp.inner, x.dtype, qmin, qmax, round_mode, clamp_ste,
                                scale_dtype=rule.scale_dtype, scale_pc=sp.channels > 1, pre_op=pre_op)
            fused = nat.stats_fakequant_fwd(desc, xc, sp.min_val, rule.thr_div, rule.scale_dtype)
            if fused is None and len(sp.scaling_shape) > 0 and sp.channels > 1 and \
                    (runtime is None or running is not None):
                # a channel larger than one workgroup: held by a cluster of workgroups, x still read once
                fused = nat.absmax_fakequant_cluster(
                    desc, xc, sp.min_val, rule.thr_div, rule.scale_dtype, running,
                    runtime.momentum if running is not None else 0.0,
                    runtime.first_batch if running is not None else False)
                if fused is not None and running is not None:
                    runtime.bvq_running_folded = True
        if fused is not None:
            stat, scale, y = fused
            scale = scale.view(sp.scaling_shape)
            y = _restore(y, back)
        else:
            if running is not None:
                running = (running, runtime.momentum, runtime.first_batch)
                runtime.bvq_running_folded = True
            stat, scale = stats_scale(xc.reshape(-1), int_threshold, sp, group, pre_op, running)
            p = Plan(sp.outer, sp.channels, sp.inner, sp.channels > 1, False, torch.result_type(x, scale), sp.nhwc)
            if not (p.ct == x.dtype or p.ct == torch.float32):
                raise nat.BvqError('StatsFakeQuantFn: unsupported operand layout (caller must pre-check)')
            desc, y = _quantize(p, xc, back, scale, zp, qmin, qmax, round_mode, clamp_ste, nat.OUT_DEQUANT, pre_op)
        ctx.desc = desc
        ctx.sp = sp
        ctx.group = group
        ctx.save_for_backward(xc, scale, zp, stat, int_threshold)
        stat_out = stat.view(sp.scaling_shape)
        ctx.mark_non_differentiable(stat_out)
        return y, scale, stat_out

    @staticmethod
    def backward(ctx, gy, gscale, _gstat):
        xc, scale, zp, stat, int_threshold = ctx.saved_tensors
        dx = stats_backward(xc, scale, zp, stat, int_threshold, ctx.desc, ctx.sp, ctx.group, ctx.pre_op, ctx.back, gy,
                            gscale)
        return dx, None, None, None, None, None, None, None, None, None


def unit_call(x: Tensor, unit_len: int, zp_per_unit: bool, int_threshold: float, qmin: float, qmax: float, clamp_ste):
    """-> (descriptor, threshold divisor) that the wrappers of a per-unit family (nat.UnitFamily) take for x as
    numel / unit_len units of `unit_len` consecutive elements: one scale per unit and, zp_per_unit, one zero-point, in
    x's dtype"""
    units = x.numel() // unit_len
    desc = channel_desc(1, units, unit_len, x.dtype, qmin, qmax, nat.ROUND, clamp_ste,
                        zp_dtype=x.dtype if zp_per_unit else torch.float32, zp_pc=zp_per_unit)
    return desc, scale_rule(x.dtype, (units, 1), int_threshold).thr_div


def group_quant_call(x: Tensor, group_size: int, int_threshold: float, qmin: float, qmax: float, clamp_ste):
    """unit_call for nat.group_quant_* and group_mse_*: x in groups of `group_size`"""
    return unit_call(x, group_size, False, int_threshold, qmin, qmax, clamp_ste)


def group_shifted_call(x: Tensor, group_size: int, int_threshold: float, qmin: float, qmax: float, clamp_ste):
    """unit_call for nat.group_shifted_*: one zero-point per group"""
    return unit_call(x, group_size, True, int_threshold, qmin, qmax, clamp_ste)


def row_shifted_call(x: Tensor, int_threshold: float, qmin: float, qmax: float, clamp_ste):
    """unit_call for nat.row_shifted_*: x as [rows, H] = [numel / shape[-1], shape[-1]], one zero-point per row"""
    return unit_call(x, x.shape[-1], True, int_threshold, qmin, qmax, clamp_ste)


def _group_grads(x: Tensor, gy, side, side_dtype=None, align_side=False):
    """The backward prelude of the Functions on the group walk: gy and the gradients `side` that arrived through the
    per-group outputs, any of them None -> (gy, side) as the kernels take them, or None when nothing arrived.  gy: x's
    dtype, contiguous, on a 16-byte boundary, zeros when only a per-group output was used downstream; side: flat,
    contiguous, `side_dtype` (x's unless named), None kept, on a 16-byte boundary when `align_side`."""
    if gy is None and all(s is None for s in side):
        return None
    gy = torch.zeros_like(x) if gy is None else gy.to(x.dtype).contiguous()
    side = [None if s is None else s.to(side_dtype or x.dtype).reshape(-1).contiguous() for s in side]
    if align_side:
        side = [s.clone() if s is not None and s.data_ptr() % 16 != 0 else s for s in side]
    if gy.data_ptr() % 16 != 0:
        gy = gy.clone()
    return gy, side


class GroupStatsFakeQuantFn(Function):
    """Group-wise weights: AbsMax per group of `group_size` consecutive elements -> clamp_min(min_val) -> / int_threshold
    -> IntQuant with a zero zero-point, x -> (y like x, scale [groups, 1]).  One launch each way (csrc/bvq_group_quant.hip):
    a group lives in a fraction of one wave, so the statistic, the scale gradient and the arg-max deposit never leave
    registers.  The caller has checked what the kernels cover (GroupwiseRescalingIntQuant._group_plan)."""

    @staticmethod
    def forward(ctx, x, group_size, min_val, int_threshold, qmin, qmax, clamp_ste):
        ctx.set_materialize_grads(False)  # an unused `scale` output must not cost a zero-fill + add
        desc, thr_div = unit_call(x, group_size, False, int_threshold, qmin, qmax, clamp_ste)
        y, scale, stat = nat.group_quant_fwd(desc, x, min_val, thr_div)
        ctx.desc, ctx.min_val, ctx.thr_div = desc, min_val, thr_div
        ctx.save_for_backward(x, scale, stat)
        return y, scale.view(-1, 1)

    @staticmethod
    def backward(ctx, gy, gscale):
        x, scale, stat = ctx.saved_tensors
        grads = _group_grads(x, gy, [gscale], align_side=nat.GROUP_QUANT.align_side)
        if grads is None:
            return (None,) * 7
        gy, (gscale,) = grads
        dx = nat.group_quant_bwd(ctx.desc, gy, x, scale, stat, gscale, ctx.min_val, ctx.thr_div)
        return (dx,) + (None,) * 6


class GroupShiftedFakeQuantFn(Function):
    """Asymmetric group-wise weights: per group of `group_size` consecutive elements, scale = clamp_min(|max - min|,
    min_val) / int_threshold, integer zero-point = to_int(-min(min, 0)), IntQuant with unsigned codes;
    x -> (y like x, scale [groups, 1], zero_point [groups, 1]).  One launch each way (csrc/bvq_group_shifted.hip): both
    statistics, both gradient sums and the two deposits stay in registers.  Gradients arriving through the returned
    scale and zero-point join the group's sums.  The caller has checked what the kernels cover
    (GroupwiseRescalingIntQuant._group_plan)."""

    @staticmethod
    def forward(ctx, x, group_size, min_val, int_threshold, qmin, qmax, clamp_ste):
        ctx.set_materialize_grads(False)  # unused `scale` / `zero_point` outputs must not cost a zero-fill + add
        desc, thr_div = unit_call(x, group_size, True, int_threshold, qmin, qmax, clamp_ste)
        y, scale, zp, stat = nat.group_shifted_fwd(desc, x, min_val, thr_div)
        ctx.desc, ctx.min_val, ctx.thr_div = desc, min_val, thr_div
        ctx.save_for_backward(x, stat)
        return y, scale.view(-1, 1), zp.view(-1, 1)

    @staticmethod
    def backward(ctx, gy, gscale, gzp):
        x, stat = ctx.saved_tensors
        grads = _group_grads(x, gy, [gscale, gzp], align_side=nat.GROUP_SHIFTED.align_side)
        if grads is None:
            return (None,) * 7
        gy, (gscale, gzp) = grads
        dx = nat.group_shifted_bwd(ctx.desc, gy, x, stat, gscale, gzp, ctx.min_val, ctx.thr_div)
        return (dx,) + (None,) * 6


class RowShiftedFakeQuantFn(Function):
    """Asymmetric per-row (per-token) dynamic activations: GroupShiftedFakeQuantFn with a row of x.shape[-1] elements in
    the place of a group; x -> (y like x, scale [rows, 1], zero_point [rows, 1]).  One launch each way
    (csrc/bvq_row_shifted.hip): a row stays in the registers of one wave or one workgroup.  The caller has checked what
    the kernels cover (DynamicActIntQuant._route)."""

    @staticmethod
    def forward(ctx, x, min_val, int_threshold, qmin, qmax, clamp_ste):
        ctx.set_materialize_grads(False)  # unused `scale` / `zero_point` outputs must not cost a zero-fill + add
        desc, thr_div = unit_call(x, x.shape[-1], True, int_threshold, qmin, qmax, clamp_ste)
        y, scale, zp, stat = nat.row_shifted_fwd(desc, x, min_val, thr_div)
        ctx.desc, ctx.min_val, ctx.thr_div = desc, min_val, thr_div
        ctx.save_for_backward(x, stat)
        return y, scale.view(-1, 1), zp.view(-1, 1)

    @staticmethod
    def backward(ctx, gy, gscale, gzp):
        x, stat = ctx.saved_tensors
        grads = _group_grads(x, gy, [gscale, gzp], align_side=nat.ROW_SHIFTED.align_side)
        if grads is None:
            return (None,) * 6
        gy, (gscale, gzp) = grads
        dx = nat.row_shifted_bwd(ctx.desc, gy, x, stat, gscale, gzp, ctx.min_val, ctx.thr_div)
        return (dx,) + (None,) * 5


def weight_norm_call(x: Tensor, qmax: float, round_mode: int, clamp_ste):
    """-> the descriptor nat.weight_norm_fwd / weight_norm_bwd take for the weight x as [x.shape[0], K]: float32
    arithmetic and scales whatever x's dtype, the narrow signed range [-qmax, qmax]"""
    rows = x.shape[0]
    desc = channel_desc(1, rows, x.numel() // rows, x.dtype, -qmax, qmax, round_mode, clamp_ste,
                        scale_dtype=torch.float32)
    desc.ct_dtype = nat.F32
    return desc


class WeightNormFakeQuantFn(Function):
    """Weight-normalised weights (WeightNormIntQuant): per output channel n = norm(v), g' = min(g, T s), p = s n / g',
    y = clamp(R(v / p)) s.  (x, value_s, value_g) -> (y like x, scale like value_s, n float32 [rows]) with the learned
    parameters as they are stored: s = clamp_min(value_s, s_min) and g = clamp_min(value_g, g_min), both bounds positive,
    are the forwards of ParameterScaling's restriction (the |.| of a positive number is the number), and its backward
    -- a straight-through clamp, then the sign of a positive number -- is the identity, so dvalue_s = ds (+ what arrives
    through the returned scale) and dvalue_g = dg.  One launch each way (csrc/bvq_weight_norm.hip) beside the two
    clamps: a channel stays in the registers of one wave or one workgroup.  n is saved for the backward and is no
    differentiable output.  The caller has checked what the kernels cover (WeightNormIntQuant._fused_call)."""

    @staticmethod
    def forward(ctx, x, value_s, value_g, s_min, g_min, desc, norm_kind, t_bound, norm_min):
        ctx.set_materialize_grads(False)  # an unused `scale` output must not cost a zero-fill + add
        scale = torch.clamp_min(value_s.detach(), s_min)
        s = scale.reshape(-1).float()
        g = torch.clamp_min(value_g.detach(), g_min).reshape(-1).float()
        y, n = nat.weight_norm_fwd(desc, norm_kind, t_bound, norm_min, x, s, g)
        ctx.desc, ctx.call = desc, (norm_kind, t_bound, norm_min)
        ctx.like = (value_s.shape, value_s.dtype, value_g.shape, value_g.dtype)
        ctx.save_for_backward(x, s, g, n)
        ctx.mark_non_differentiable(n)
        return y, scale, n

    @staticmethod
    def backward(ctx, gy, gscale, _gn):
        x, s, g, n = ctx.saved_tensors
        s_shape, s_dtype, g_shape, g_dtype = ctx.like
        if gy is None:   # only the returned scale was used downstream
            return (None, gscale, None) + (None,) * 6
        gy, _ = _group_grads(x, gy, [])
        dx, dscale, dg = nat.weight_norm_bwd(ctx.desc, *ctx.call, gy, x, s, g, n)
        dscale = dscale.reshape(s_shape).to(s_dtype)
        if gscale is not None:
            dscale = dscale + gscale
        return (dx, dscale, dg.reshape(g_shape).to(g_dtype)) + (None,) * 6


class GroupMSEFakeQuantFn(Function):
    """Group-wise weights with a searched clipping threshold (GroupwiseMSEIntQuant): GroupStatsFakeQuantFn with, per
    group, the first of the candidate thresholds AbsMax * ratio_i that has the smallest squared quantization error,
    x -> (y like x, scale [groups, 1], idx uint8 [groups]).  One launch each way (csrc/bvq_group_mse.hip): the search
    runs on the registers that hold the group.  idx is a constant of the backward.  `table`: nat.mse_ratio_table.  The
    caller has checked what the kernels cover (GroupwiseMSEIntQuant.forward)."""

    @staticmethod
    def forward(ctx, x, group_size, min_val, int_threshold, qmin, qmax, clamp_ste, table):
        ctx.set_materialize_grads(False)  # an unused `scale` output must not cost a zero-fill + add
        desc, thr_div = unit_call(x, group_size, False, int_threshold, qmin, qmax, clamp_ste)
        y, scale, stat, idx = nat.group_mse_fwd(desc, x, table, min_val, thr_div)
        ctx.desc, ctx.min_val, ctx.thr_div, ctx.table = desc, min_val, thr_div, table
        ctx.save_for_backward(x, stat, idx)
        ctx.mark_non_differentiable(idx)
        return y, scale.view(-1, 1), idx

    @staticmethod
    def backward(ctx, gy, gscale, _gidx):
        x, stat, idx = ctx.saved_tensors
        grads = _group_grads(x, gy, [gscale], align_side=nat.GROUP_MSE.align_side)
        if grads is None:
            return (None,) * 8
        gy, (gscale,) = grads
        dx = nat.group_mse_bwd(ctx.desc, gy, x, stat, idx, gscale, ctx.table, ctx.min_val, ctx.thr_div)
        return (dx,) + (None,) * 7


class GroupHQOFakeQuantFn(Function):
    """Asymmetric group-wise weights with a searched zero-point (GroupwiseHQOIntQuant): GroupShiftedFakeQuantFn with,
    per group, the zero-point moved by up to len(table) - 1 half-quadratic proximal steps and the first candidate with
    the smallest summed |error| kept; x -> (y like x, scale [groups, 1], zero_point [groups, 1]: the kept one, a value
    of x's dtype, idx uint8 [groups]: the kept candidate).  One launch each way (csrc/bvq_group_hqo.hip): the search
    runs on the registers that hold the group.  zero_point and idx are constants of the backward.  `table`:
    nat.hqo_beta_table, `lp`: nat.HQO_LP.  The caller has checked what the kernels cover
    (GroupwiseHQOIntQuant.forward)."""

    @staticmethod
    def forward(ctx, x, group_size, min_val, int_threshold, qmin, qmax, clamp_ste, table, lp):
        ctx.set_materialize_grads(False)  # an unused `scale` output must not cost a zero-fill + add
        desc, thr_div = unit_call(x, group_size, True, int_threshold, qmin, qmax, clamp_ste)
        y, scale, zp, stat, idx = nat.group_hqo_fwd(desc, x, table, lp, min_val, thr_div)
        ctx.desc, ctx.min_val, ctx.thr_div = desc, min_val, thr_div
        ctx.save_for_backward(x, stat, zp)
        zp = zp.view(-1, 1)
        ctx.mark_non_differentiable(zp, idx)
        return y, scale.view(-1, 1), zp, idx

    @staticmethod
    def backward(ctx, gy, gscale, _gzp, _gidx):
        x, stat, zp = ctx.saved_tensors
        grads = _group_grads(x, gy, [gscale], align_side=nat.GROUP_HQO.align_side)
        if grads is None:
            return (None,) * 9
        gy, (gscale,) = grads
        dx = nat.group_hqo_bwd(ctx.desc, gy, x, stat, zp, gscale, ctx.min_val, ctx.thr_div)
        return (dx,) + (None,) * 8


class MXQuantFn(Function):
    """MX block-scaled quantizer (core/quant/mx.py): x -> (y like x, float32 scale [groups]).  One launch each way
    (csrc/bvq_mx_quant.hip); the backward recomputes each group's abs-max and exponent from x, so only x is saved.  The
    caller has checked what the kernels cover (MXQuant.fused_route)."""

    @staticmethod
    def forward(ctx, x, group_size, fmt, scale_rule, clamp_ste):
        ctx.set_materialize_grads(False)  # an unused `scale` output must not cost a zero-fill
        y, scale = nat.mx_quant_fwd(x, group_size, fmt, scale_rule)
        ctx.args = (group_size, fmt, scale_rule, clamp_ste)
        ctx.save_for_backward(x)
        return y, scale

    @staticmethod
    def backward(ctx, gy, gscale):
        x, = ctx.saved_tensors
        grads = _group_grads(x, gy, [gscale], torch.float32, align_side=True)   # as bvq_mx_quant_bwd wants its gscale
        if grads is None:
            return (None,) * 5
        gy, (gscale,) = grads
        return (nat.mx_quant_bwd(gy, x, gscale, *ctx.args),) + (None,) * 4


class StatsGraphFakeQuantFn(Function):
    """AbsMax statistic -> ANY scale-shaped map (`post`: a _StatsScaling with affine rescaling, a power-of-two
    restriction, ...) -> / int_threshold -> IntQuant, zero zero-point (B/core/scaling/runtime.py:19-72,
    B/core/quant/int.py:155-163).

    The tensor-sized work stays on the fused kernels -- statistic (1 read), quantizer (1 read + 1 write), backward
    (2 reads + 1 write, with the scale-gradient sums and the arg-max positions on the same reads) -- and only the map
    itself runs as torch ops on `channels`-sized tensors, recorded here and differentiated by autograd on those small
    tensors: dscale -> (d statistic, d affine_weight, d affine_bias); the statistic's gradient is then deposited on the
    arg-max elements in place.  The op-by-op route it replaces sends the statistic's gradient through AbsMax's own
    backward (a second pass over x writing a dense gradient) and adds the two x-sized gradients: 11 tensor passes
    instead of 6.  `params`: post's parameters, passed so that autograd sees them as inputs."""

    @staticmethod
    def forward(ctx, x, int_threshold, sp, qmin, qmax, round_mode, clamp_ste, pre_op, post, *params):
        ctx.set_materialize_grads(False)
        xc, back = _memory_order(x, sp.channels, sp.nhwc)
        flat = xc.reshape(-1)
        stat = nat.stats(nat.STAT_ABSMAX, flat, sp.outer, sp.channels, sp.inner, pre_op=pre_op).view(sp.scaling_shape)
        with torch.enable_grad():
            s_leaf = stat.detach().requires_grad_(True)
            scale_g = post(s_leaf) / int_threshold
        scale = scale_g.detach()
        zp = _zero_zero_point(x.device)
        p = plan(xc if back is None else x, scale, zp)
        if p is None or p.zp_pc or p.nhwc != sp.nhwc:
            raise nat.BvqError('StatsGraphFakeQuantFn: operand layout not covered by the quantizer kernels')
        desc, y = _quantize(p, xc, back, scale, zp, qmin, qmax, round_mode, clamp_ste, nat.OUT_DEQUANT, pre_op)
        ctx.desc, ctx.sp, ctx.back, ctx.pre_op = desc, sp, back, pre_op
        ctx.graph = (s_leaf, scale_g, params)
        ctx.save_for_backward(xc, scale, zp, stat)
        ctx.mark_non_differentiable(stat)
        return y, scale, stat

    @staticmethod
    def backward(ctx, gy, gscale, _gstat):
        xc, scale, zp, stat = ctx.saved_tensors
        desc, sp = ctx.desc, ctx.sp
        s_leaf, scale_g, params = ctx.graph
        none = (None,) * 9
        if gy is None and gscale is None:
            return none + (None,) * len(params)
        gy = _incoming(gy, desc, xc, ctx.back)
        stat_x = stat.reshape(-1).to(xc.dtype).contiguous()
        dx, ds, _, ties = nat.fakequant_bwd(desc, gy, xc, scale.reshape(-1).contiguous(), zp.reshape(-1), True, False,
                                            tie_stat=stat_x)
        dscale = _reduce_like(ds, scale)
        if gscale is not None:
            dscale = dscale + gscale
        grads = torch.autograd.grad(scale_g, (s_leaf,) + tuple(params), dscale, retain_graph=True, allow_unused=True)
        dstat = grads[0]
        if dstat is not None:
            nat.stat_tie_apply(nat.MATCH_ABS, xc.reshape(-1), stat_x, dstat.reshape(-1).to(xc.dtype).contiguous(), ties,
                               dx.reshape(-1), sp.outer, sp.channels, sp.inner, mode_add=True, pre_op=ctx.pre_op)
        return (_restore(dx, ctx.back),) + none[1:] + tuple(grads[1:])


def _list_views(params, sp):
    """(flat tensors, outers, inners) of a shared quantizer's parameters as the list kernel takes them"""
    flats = [t.detach().reshape(-1) for t in params]
    return flats, [1] * len(params), [t.numel() // sp.channels for t in params]


def list_stats_supported(params, sp) -> bool:
    """the one-launch statistic over a parameter list applies (nat.absmax_scale_list would not return None)"""
    if not config.FUSED_PATHS or params[0].dtype not in _FLOATS or sp.outer != 1 or sp.nhwc:
        return False
    flats, outers, inners = _list_views(params, sp)
    st = nat.stream_ptr(flats[0].device)
    if sp.channels > 1 and nat.arrival_buffer(flats[0].device, st, max(2 * sp.channels, 18)) is None:
        return False
    return nat.absmax_list_supported(flats, outers, sp.channels, inners)


class ListStatsFakeQuantFn(Function):
    """StatsFakeQuantFn for a weight quantizer SHARED by several layers: the statistic is AbsMax over the concatenation
    of all tracked parameters' views (B/core/stats/stats_wrapper.py:83-114, _ParameterListStats with more than one
    parameter; B/core/scaling/standalone.py StatsFromParameterScaling), the tensor quantized is one of them.

    Forward, two launches: the statistic of the whole list + scale (nat.absmax_scale_list: the concatenation is never
    built), the quantizer kernel on x.  Backward: the quantizer's backward on x (dx, the scale-gradient sums and x's own
    arg-max positions on the same reads); the other parameters are scanned for the positions attaining the statistic,
    and the statistic's gradient goes where torch's backward of max over the concatenation puts it -- per channel on
    the FIRST position in concatenation order (extra parameters are concatenated in front: the highest list index
    that attains it), for a whole-tensor statistic evenly over all ties of all parameters -- into dx for x, into zero
    tensors for the others.  The reference reads
    and writes every parameter for torch.cat, reduces the copy, and in backward writes a dense gradient of the
    concatenation and slices it."""

    @staticmethod
    def forward(ctx, x, int_threshold, sp, qmin, qmax, round_mode, clamp_ste, index, *params):
        ctx.set_materialize_grads(False)
        flats, outers, inners = _list_views(params, sp)
        rule = scale_rule(x.dtype, sp.scaling_shape, sp.int_threshold, int_threshold.dtype)
        out = nat.absmax_scale_list(flats, outers, sp.channels, inners, sp.min_val, rule.thr_div, rule.scale_dtype)
        if out is None:
            raise nat.BvqError('ListStatsFakeQuantFn: list not covered (caller must pre-check list_stats_supported)')
        stat, scale = out
        scale = scale.view(sp.scaling_shape)
        zp = _zero_zero_point(x.device)
        xc = x.detach()
        p = Plan(sp.outer, sp.channels, sp.inner, sp.channels > 1, False, torch.result_type(x, scale), False)
        if not (p.ct == x.dtype or p.ct == torch.float32):
            raise nat.BvqError('ListStatsFakeQuantFn: unsupported operand layout')
        desc, y = _quantize(p, xc, None, scale, zp, qmin, qmax, round_mode, clamp_ste, nat.OUT_DEQUANT, nat.PRE_NONE)
        ctx.desc, ctx.sp, ctx.index, ctx.inners = desc, sp, index, inners
        ctx.save_for_backward(scale, zp, stat, int_threshold, *params)
        stat_out = stat.view(sp.scaling_shape)
        ctx.mark_non_differentiable(stat_out)
        return y, scale, stat_out

    @staticmethod
    def backward(ctx, gy, gscale, _gstat):
        scale, zp, stat, int_threshold = ctx.saved_tensors[:4]
        params = ctx.saved_tensors[4:]
        desc, sp, index = ctx.desc, ctx.sp, ctx.index
        none = (None,) * 8
        if gy is None and gscale is None:
            return none + (None,) * len(params)
        x = params[index].detach()
        gy = _incoming(gy, desc, x, None)
        stat_x = stat.reshape(-1).to(x.dtype).contiguous()
        dx, ds, _, own = nat.fakequant_bwd(desc, gy, x, scale.reshape(-1).contiguous(), zp.reshape(-1), True, False,
                                           tie_stat=stat_x)
        ds = _reduce_like(ds, scale)
        if gscale is not None:
            ds = ds + gscale
        # scale = thr / int_threshold  ->  dthr = dscale / int_threshold ; clamp_min_ste passes it on
        dstat = (ds / int_threshold).to(stat.dtype).reshape(-1).contiguous()
        ch = sp.channels
        # the other parameters: one read each, which also writes the zeros their non-attaining elements receive
        # (0 * sgn(x): the reference's gradient of |x| there, signed zeros included)
        outs = [dx if i == index else torch.empty_like(t, memory_format=torch.contiguous_format)
                for i, t in enumerate(params)]
        infos = [own if i == index else
                 nat.stat_tie_scan(nat.MATCH_ABS, t.detach().reshape(-1), stat_x, 1, ch, ctx.inners[i],
                                   dx_zero_fill=outs[i].reshape(-1))
                 for i, t in enumerate(params)]
        total = None
        if ch > 1:
            # the deposit of channel c belongs to the first tensor IN CONCATENATION ORDER that attains the statistic
            # there; every extra parameter is concatenated in FRONT of what came before
            # (B/core/stats/view_wrapper.py:49-50), so that order is the list's, reversed
            order = list(range(len(infos)))[::-1]
            first = torch.stack([infos[i][:ch] for i in order])                # [n, channels], -1: not attained
            has = first >= 0
            owner = torch.where(has.any(0), has.to(torch.int8).argmax(0), torch.full_like(first[0], -1))
            for r, i in enumerate(order):
                infos[i][:ch] = torch.where(owner == r, infos[i][:ch], torch.full_like(infos[i][:ch], -1))
        else:
            total = torch.stack([w[0] for w in infos]).sum().reshape(1)        # ties of the whole list share evenly
        for i, t in enumerate(params):
            nat.stat_tie_apply(nat.MATCH_ABS, t.detach().reshape(-1), stat_x, dstat, infos[i], outs[i].reshape(-1), 1, ch,
                               ctx.inners[i], mode_add=(i == index), total_ties=total)
        return (dx,) + none[1:] + tuple(g if i != index else None for i, g in enumerate(outs))


def stats_backward(xc, scale, zp, stat, int_threshold, desc, sp, group, pre_op, back, gy, gscale):
    """backward of StatsFakeQuantFn (also the fallback of the C++ node, brevitas_amd/csrc/bvq_autograd.cpp) -> dx or None;
    sp: anything with outer / channels / inner / int_threshold"""
    if gy is None and gscale is None:
        return None
    gy = _incoming(gy, desc, xc, back)
    # dscale / int_threshold: the forward's division, on the scale's gradient
    rule = scale_rule(scale.dtype, scale.shape, sp.int_threshold, int_threshold.dtype)
    if group is None and gscale is None and sp.channels > 1 and scale.numel() == sp.channels:
        # per-channel scale, nothing else feeding the scale's gradient: two launches in all -- the backward
        # kernel (dx, per-unit dscale sums and arg-max positions) and one finishing kernel that sums,
        # converts dscale into the statistic's gradient and deposits it (None: layout not covered)
        dx = nat.fakequant_bwd_stats(desc, gy, xc, scale.reshape(-1).contiguous(), zp.reshape(-1), stat,
                                     scale.dtype, rule.thr_bwd, rule.quot_dtype)
        if dx is not None:
            return _restore(dx, back)
    if group is not None and gscale is None and sp.channels > 1 and scale.numel() == sp.channels:
        # batch shard, per-channel scale: the backward kernel (its last-arriving wave per channel writes the shard's
        # all-gather message: double dscale sums + the claim on the deposit), ONE all-gather, one launch that adds the
        # shards' sums in double and deposits the statistic's gradient on the owning shard
        import torch.distributed as dist
        rank, world = dist.get_rank(group), dist.get_world_size(group)
        out = nat.fakequant_bwd_shard(desc, gy, xc, scale.reshape(-1).contiguous(), zp.reshape(-1), stat, rank)
        if out is not None:
            dx, msg, pos = out
            if world > 1:
                gathered = torch.empty(world * msg.numel(), dtype=msg.dtype, device=msg.device)
                dist.all_gather_into_tensor(gathered, msg, group=group)
            else:
                gathered = msg
            nat.shard_unpack_deposit(xc.reshape(-1), dx.reshape(-1), gathered, world, sp.channels, rank, pos, sp.inner,
                                     scale.dtype, rule.thr_bwd, rule.quot_dtype, pre_op)
            return _restore(dx, back)
    # one pass: dx, the scale-gradient sums and the positions attaining the statistic
    dx, ds, _, ties = nat.fakequant_bwd(desc, gy, xc, scale.reshape(-1).contiguous(), zp.reshape(-1), True,
                                        False, tie_stat=stat)
    total_ties = None
    if group is None and gscale is None and ds.numel() == scale.numel():
        # dscale -> dstat -> deposit in one launch (same rounding points as the ops below)
        nat.stat_tie_apply_dscale(xc.reshape(-1), stat, ds, scale.dtype, rule.thr_bwd, rule.quot_dtype, ties,
                                  dx.reshape(-1), sp.outer, sp.channels, sp.inner, pre_op=pre_op)
        return _restore(dx, back)
    if group is not None:
        # sum the shards' partial sums, and agree on which shard deposits the statistic's gradient
        from brevitas_amd.distributed import sync_backward
        if gscale is not None:
            ds = ds + gscale.reshape(-1).to(ds.dtype)
            gscale = None
        ds, ties, total_ties = sync_backward(ds, ties, sp.channels, group)
    ds = _reduce_like(ds, scale)
    if gscale is not None:
        ds = ds + gscale
    # scale = thr / int_threshold  ->  dthr = dscale / int_threshold ; clamp_min_ste passes it on
    dstat = (ds / int_threshold).to(stat.dtype).reshape(-1).contiguous()
    nat.stat_tie_apply(nat.MATCH_ABS, xc.reshape(-1), stat, dstat, ties, dx.reshape(-1), sp.outer,
                       sp.channels, sp.inner, mode_add=True, total_ties=total_ties, pre_op=pre_op)
    return _restore(dx, back)


# ---- the weight quantizer's autograd node in C++ (brevitas_amd/csrc/bvq_autograd.cpp) ------------------------------
# Optional host-side accelerator: one native call each way instead of the Python Function + ctypes wrappers (85 -> ~50 us
# of host time per weight-sized step).  Built in-tree by brevitas_amd/csrc/build.py; when the module is absent the
# Python Function above serves every call -- same kernels, same results either way.
_FAST = None          # the loaded extension module, False after a failed attempt
_FAST_PATH = None


class _SpLike(NamedTuple):
    outer: int
    channels: int
    inner: int
    int_threshold: float


def _fast_backward_fallback(xc, scale, zp, stat, int_threshold, dv, qr, shape, gy, gscale, group=None):
    """what the C++ nodes cannot do themselves (a gradient arriving through `scale`, an unaligned or strided gradient,
    a batch-sharded whole-tensor statistic)"""
    desc = nat.QuantDesc.from_dv(dv, qr[0], qr[1])
    sp = _SpLike(desc.outer, desc.channels, desc.inner, qr[3])  # qr: qmin, qmax, thr_bwd, the threshold's host value
    return stats_backward(xc, scale.view(shape), zp, stat, int_threshold, desc, sp, group, desc.pre_op, None, gy, gscale)


def _fast_module():
    global _FAST, _FAST_PATH
    if _FAST is None:
        import importlib.util
        import os
        _FAST = False
        path = os.path.join(os.path.dirname(nat.LIB_PATH), '_bvq_autograd.so')
        if config.CPP_AUTOGRAD and os.path.exists(path):
            try:
                spec = importlib.util.spec_from_file_location('_bvq_autograd', path)
                mod = importlib.util.module_from_spec(spec)
                spec.loader.exec_module(mod)
                mod.init(nat.LIB_PATH, _fast_backward_fallback)   # raises on another ABI version of libbvq.so
                _FAST, _FAST_PATH = mod, path
            except Exception:  # noqa: BLE001  (an extension built against another torch: the Python route serves)
                _FAST = False
    return _FAST


def _fast_gate(x, sp):
    """the C++ node's module when it can take x (a dense device tensor in NCHW order, no timers bracketing the calls,
    the current device), else None"""
    mod = _fast_module()
    if not mod or not x.is_cuda or sp.nhwc or not x.is_contiguous() or x.dtype not in _FLOATS or not config.FUSED_PATHS:
        return None
    timer = nat._timer
    if timer is not None and getattr(timer, 'enabled', True):
        return None  # bench.py is bracketing the C-ABI calls of this step with HIP events: keep them visible
    if x.device.index is not None and x.device.index != torch.cuda.current_device():
        return None  # the node launches on the current device: the Python route switches devices around its calls
    return mod


def _node_dv(sp, dtype, scale_dtype, round_mode, clamp_ste, pre_op):
    """channel_desc(sp.outer, sp.channels, sp.inner, dtype, ..., scale_dtype=scale_dtype, scale_pc=sp.channels > 1,
    pre_op=pre_op).to_dv(), written out: the node builds its own bvq_quant_desc from these integers, and a ctypes
    struct made only to be read back costs 2 of the ~48 us a weight step spends on the host (tools/host_cost.py).
    tests/test_fused_host_rules.py holds the two equal."""
    code = nat.dtype_code(dtype)
    return (sp.outer, sp.channels, sp.inner, code, code, nat.dtype_code(scale_dtype), nat.F32, int(sp.channels > 1), 0,
            round_mode, scalar_mode(), int(clamp_ste), nat.OUT_DEQUANT, pre_op, 0)


def fast_stats_fakequant(x, int_threshold, sp, qmin, qmax, round_mode, clamp_ste, pre_op):
    """StatsFakeQuantFn through the C++ node -> (y, scale, stat), or None: not a case it covers (per-tensor scale,
    channels_last / strided input, layouts outside the one-launch forward, no extension built, timers active)"""
    mod = _fast_gate(x, sp)
    if mod is None or sp.channels <= 1:
        return None
    # (more than one channel: the scaling shape is dimensioned, and the rule's backward pair is the node's)
    rule = scale_rule(x.dtype, sp.scaling_shape, sp.int_threshold, int_threshold.dtype)
    dv = _node_dv(sp, x.dtype, rule.scale_dtype, round_mode, clamp_ste, pre_op)
    st = nat.stream_ptr(x.device)
    arrive = nat.arrival_buffer(x.device, st, sp.channels) if nat.ONEPASS_BWD else None
    return mod.stats_fakequant(x, _zero_zero_point(x.device), int_threshold, arrive, dv, float(qmin), float(qmax),
                               float(sp.min_val or 0.0), bool(sp.min_val), float(rule.thr_div), float(rule.thr_bwd),
                               float(sp.int_threshold), dv[5], list(sp.scaling_shape), st)


def fast_act_stats_fakequant(x, int_threshold, sp, qmin, qmax, round_mode, clamp_ste, pre_op, group, runtime):
    """The activation route of StatsFakeQuantFn (statistic kernel + quantizer kernel, the running statistic folded in,
    optionally batch-sharded with its two collectives) through the C++ node -> (y, scale, stat) with
    `runtime.bvq_running_folded` set, or None: not a case it covers (channels_last / strided / unaligned input, a running
    buffer that is not a plain [channels] device tensor, no extension built, timers active)."""
    mod = _fast_gate(x, sp)
    if mod is None or not hasattr(mod, 'act_stats_fakequant') or x.numel() == 0:
        return None
    if group is not None and not config.CPP_AUTOGRAD_SHARDED:
        return None
    running = _running_buffer(runtime, sp.channels)
    if runtime is not None and running is None:
        return None
    momentum, first = (runtime.momentum, runtime.first_batch) if runtime is not None else (0.0, False)
    rule = scale_rule(x.dtype, sp.scaling_shape, sp.int_threshold, int_threshold.dtype)
    if sp.channels > 1 and len(sp.scaling_shape) == 0:
        return None
    ct = torch.result_type(x, torch.empty(sp.scaling_shape, dtype=rule.scale_dtype, device='meta'))
    if ct != x.dtype:
        return None
    dv = _node_dv(sp, x.dtype, rule.scale_dtype, round_mode, clamp_ste, pre_op)
    st = nat.stream_ptr(x.device)
    arrive = nat.arrival_buffer(x.device, st, max(2 * sp.channels, 18))
    out = mod.act_stats_fakequant(x, _zero_zero_point(x.device), int_threshold, running, arrive, dv, float(qmin),
                                  float(qmax), float(sp.min_val or 0.0), bool(sp.min_val), float(rule.thr_div),
                                  float(rule.thr_bwd), float(sp.int_threshold), dv[5], nat.dtype_code(rule.quot_dtype),
                                  list(sp.scaling_shape), st, float(momentum), bool(first), group)
    if out is not None and runtime is not None:
        runtime.bvq_running_folded = True
    return out


# ---- many weights, one launch each way (brevitas_amd.core.quant.weight_group) -----------------------------------------
class WeightListFakeQuantFn(Function):
    """StatsFakeQuantFn for EVERY covered per-channel weight of a model at once: one bvq_weight_quant_list_fwd launch per
    chunk of the list forward (at most nat.WEIGHT_LIST_MAX weights whose channels fit the arrival buffer), one
    bvq_weight_quant_list_bwd launch per chunk backward, one autograd node instead of one per weight.  Each weight gets
    the bits its own StatsFakeQuantFn would give it (same kernels per tensor, same tiling, same sums).

    Inputs: `wl` (the group's _WeightList: the item array of include/bvq.h with each weight's static fields, its chunks,
    and what the per-tensor route needs) and the weights.  Outputs: every weight's y, then every weight's scale (scaling
    shape); those of a weight that needs no gradient are not differentiable, as its own StatsFakeQuantFn would make them.
    Backward: a weight whose scale received a gradient (a bias quantizer fed w_scale), or whose gradient is strided,
    misaligned or of another dtype, takes stats_backward alone, like the per-layer node; a weight none of whose outputs
    received a gradient gets none; the rest go through the list kernel, one call per chunk."""

    @staticmethod
    def forward(ctx, wl, *ws):
        ctx.set_materialize_grads(False)  # an unused output stays None: no zero-fill, no launch
        n = len(ws)
        ys, stats, scales = [], [], []
        for lo, hi in wl.chunks:
            y, stat, scale = nat.weight_quant_list_fwd(wl.items, lo, ws[lo:hi], wl.scale_dtype, wl.round_mode)
            ys += y
            stats.append(stat)
            scales.append(scale)
        out_scales = []
        for (lo, hi), scale in zip(wl.chunks, scales):
            for i, s in enumerate(torch.split(scale, wl.channels[lo:hi]), lo):
                out_scales.append(s.view(wl.shapes[i]))
        frozen = [i for i in range(n) if not ctx.needs_input_grad[1 + i]]
        if frozen:
            ctx.mark_non_differentiable(*[ys[i] for i in frozen], *[out_scales[i] for i in frozen])
        # the weights are kept without save_for_backward's version check: a weight updated in place inside the block
        # leaves this node (its layer re-quantizes it on its own) while the others still need it.  Versions are
        # checked in backward for the weights that receive a gradient.
        ctx.wl, ctx.ws, ctx.versions = wl, ws, [w._version for w in ws]
        ctx.stats, ctx.scales = stats, scales
        return (*ys, *out_scales)

    @staticmethod
    def backward(ctx, *grads):
        wl, ws = ctx.wl, ctx.ws
        n = len(ws)
        dxs = [None] * n
        direct = [[] for _ in wl.chunks]  # per forward chunk, the weights its list call takes
        for i in range(n):
            gy, gs = grads[i], grads[n + i]
            if (gy is None and gs is None) or not ctx.needs_input_grad[1 + i]:
                continue
            if ws[i]._version != ctx.versions[i]:
                raise RuntimeError('WeightListFakeQuantFn: weight %d was modified in place after the group quantized it'
                                   ' and before its gradient was computed' % i)
            if gs is None and gy.dtype == ws[i].dtype and gy.is_contiguous() and gy.data_ptr() & 15 == 0:
                direct[wl.chunk_of[i]].append(i)
            else:
                dxs[i] = WeightListFakeQuantFn._single(ctx, i, gy, gs)
        for idx in direct:
            if not idx:
                continue
            if idx[-1] - idx[0] == len(idx) - 1:  # a run of the forward's items
                items, first = wl.items, idx[0]
            else:
                items, first = (nat.WeightItem * len(idx))(), 0
                for j, i in enumerate(idx):
                    items[j] = wl.items[i]
            out = nat.weight_quant_list_bwd(items, first, [grads[i] for i in idx], [ws[i] for i in idx],
                                            [WeightListFakeQuantFn._ptr(ctx, ctx.stats, i) for i in idx],
                                            [WeightListFakeQuantFn._ptr(ctx, ctx.scales, i) for i in idx],
                                            wl.scale_dtype, wl.scale_dtype, wl.round_mode)
            for j, i in enumerate(idx):
                dxs[i] = out[j] if out is not None else WeightListFakeQuantFn._single(ctx, i, grads[i], None)
        return (None, *dxs)

    @staticmethod
    def _ptr(ctx, bufs, i):
        """address of weight i's per-channel vector in the forward's statistic / scale buffers"""
        buf = bufs[ctx.wl.chunk_of[i]]
        return buf.data_ptr() + ctx.wl.offsets[i] * buf.element_size()

    @staticmethod
    def _single(ctx, i, gy, gscale):
        """weight i alone through the per-tensor backward (StatsFakeQuantFn's)"""
        wl, w = ctx.wl, ctx.ws[i]
        c, o, ch = wl.chunk_of[i], wl.offsets[i], wl.channels[i]
        stat = ctx.stats[c][o:o + ch]
        scale = ctx.scales[c][o:o + ch].view(wl.shapes[i])
        return stats_backward(w, scale, _zero_zero_point(w.device), stat, wl.int_thresholds[i], wl.descs[i], wl.sps[i],
                              None, nat.PRE_NONE, None, gy, gscale)
