"""What the quantizer modules recognise of their sub-module graph before they pick a kernel route: stated once, read by
IntQuant / DecoupledIntQuant (int_base.py), RescalingIntQuant and the group-wise classes (int.py), DynamicActIntQuant
(dynamic.py), MXQuant (mx.py), WeightQuantGroup and graph/gptq.py.  Host logic only: module types, Python attributes and
tensor metadata, no device call.  DESIGN.md §9, "Routes", lists which template leads to which Function."""
from collections import namedtuple
from typing import Any, Callable, Optional

import brevitas_amd.core.quant.int_base as _int_base  # (imports this module in turn: IntQuant is read at call time)
from brevitas_amd.core.quant.delay import _NoDelay
from brevitas_amd.core.scaling.int_scaling import IntScaling
from brevitas_amd.core.stats.stats_op import AbsMinMax, NegativeMinOrZero
from brevitas_amd.function.ops import int_range_host

GROUP_SIZES = (16, 32, 64, 128, 256)  # the group sizes the sub-wave group walk covers (csrc/bvq_group_walk.h)


# what kernel_int_quant finds: the host-known bit width (None with host_bw=False), nat.ROUND ... of float_to_int_impl
# (None with rounding=False), tensor_clamp_impl's straight-through flag
KernelIntQuant = namedtuple('KernelIntQuant', 'bw round_mode clamp_ste')
# ... and plain_int_quant: the integer range and IntScaling's value at the bit width, on the host
PlainIntQuant = namedtuple('PlainIntQuant', 'qmin qmax round_mode clamp_ste int_thr')


def _template(name: str, fields: str):
    """a namedtuple whose fields can also be read by name, t['qmin'], as those of the dicts the templates replace"""
    base = namedtuple(name, fields)
    return type(name, (base,), {'__slots__': (), '__getitem__': lambda t, k: getattr(t, k) if type(k) is str
                                else base.__getitem__(t, k)})


# RescalingIntQuant, the statistic -> scale chain of a stats-scaled weight or activation.  runtime: the _RuntimeStats of an
# activation, None for a weight; weight: the tracked weight, None for an activation; shared: every tracked weight of a
# quantizer shared by several layers, or None; view: the statistic's view module; shape: of the scale; min_val: the plain
# lower bound of the threshold, None with `post`, a statistic -> threshold map that is no plain lower bound
StatsTemplate = _template('StatsTemplate', 'runtime weight shared view shape min_val post per_channel int_thr qmin qmax '
                                           'round_mode clamp_ste')
# GroupwiseRescalingIntQuant, the one-kernel graphs: symmetric, or `shifted` (shifted_zero_point)
GroupTemplate = _template('GroupTemplate', 'weight shape min_val int_thr qmin qmax clamp_ste shifted')
# DynamicActIntQuant, the graph its kernels compute
DynamicTemplate = _template('DynamicTemplate', 'shifted min_val int_thr qmin qmax round_mode clamp_ste')


def round_mode_of(float_to_int_impl) -> Optional[int]:
    return getattr(float_to_int_impl, 'bvq_round_mode', None)


def clamp_ste_of(tensor_clamp_impl) -> Optional[bool]:
    return getattr(tensor_clamp_impl, 'bvq_clamp_ste', None)


def kernel_int_quant(iq, bit_width, host_bw: bool = True, rounding: bool = True) -> Optional[KernelIntQuant]:
    """a rounding and a clamp the kernels know and a host-known bit width, else None.  `host_bw=False`: the integer range
    comes from device tensors (a learned bit width); `rounding=False`: float_to_int_impl is the caller's business"""
    bw = getattr(bit_width, 'bvq_host_value', None)
    round_mode = round_mode_of(iq.float_to_int_impl)
    clamp_ste = clamp_ste_of(iq.tensor_clamp_impl)
    if clamp_ste is None or (rounding and round_mode is None) or (host_bw and bw is None):
        return None
    return KernelIntQuant(bw, round_mode, clamp_ste)


def plain_int_quant(iq, int_scaling_impl, bit_width) -> Optional[PlainIntQuant]:
    """kernel_int_quant of exactly IntQuant, without delay, under IntScaling -> the integer range and the threshold on
    the host, else None.  The zero-point is the caller's: each says which zero-point graphs it accepts"""
    k = kernel_int_quant(iq, bit_width) if type(iq) is _int_base.IntQuant and type(int_scaling_impl) is IntScaling \
        and isinstance(iq.delay_wrapper.delay_impl, _NoDelay) else None
    if k is None:
        return None
    qmin, qmax = int_range_host(iq.signed, iq.narrow_range, k.bw)
    return PlainIntQuant(qmin, qmax, k.round_mode, k.clamp_ste, int_scaling_impl.host_value(k.bw))


def shifted_zero_point(iq, scale_stats, zp_stats, scale_shift_zero_point, reduce_dims) -> bool:
    """the asymmetric graph the shifted kernels compute: the scale from AbsMinMax and the zero-point from NegativeMinOrZero
    over the same reduction, quantized by `iq`'s own to_int, whose "+ min_int" is "+ 0" for the unsigned full range"""
    return type(scale_stats) is AbsMinMax and type(zp_stats) is NegativeMinOrZero and \
        scale_stats.stats_reduce_dim in reduce_dims and zp_stats.stats_reduce_dim in reduce_dims and \
        scale_shift_zero_point.int_quant is iq and bool(scale_shift_zero_point.quantize_zero_point) and \
        not iq.signed and not iq.narrow_range


def same_tensor(w, x) -> bool:
    """x is the tracked tensor w, or a tensor over the same storage with the same layout and dtype"""
    return w is x or (w.data_ptr() == x.data_ptr() and w.shape == x.shape and w.stride() == x.stride()
                      and w.dtype == x.dtype)


def cached(module, slot: str, key: tuple, build: Callable[[], Any]):
    """module's template in `slot`, rebuilt by build() when `key` -- everything the builder reads -- changed"""
    hit = module.__dict__.get(slot)
    if hit is not None and hit[0] == key:
        return hit[1]
    value = build()
    module.__dict__[slot] = (key, value)
    return value


def graph_key(q, bit_width) -> tuple:
    """the part of every template key that names the sub-modules a plain_int_quant reads"""
    # every forward builds it, so the sub-modules are taken from `_modules`: nn.Module.__getattr__ would cost more than
    # the rest of the lookup
    m = q._modules
    im = getattr(m.get('int_quant'), '_modules', m)
    return (id(m.get('int_quant')), id(m.get('scaling_impl')), id(m.get('zero_point_impl')), id(m.get('int_scaling_impl')),
            getattr(bit_width, 'bvq_host_value', None), id(im.get('float_to_int_impl')), id(im.get('tensor_clamp_impl')),
            id(getattr(im.get('delay_wrapper'), '_modules', m).get('delay_impl')))
