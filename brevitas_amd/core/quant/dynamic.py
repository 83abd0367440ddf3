"""DynamicActIntQuant: integer activation quantizers whose scale (and zero-point) come from the tensor being quantized,
in training and in eval alike (the Int8DynamicAct... / ShiftedUint8DynamicAct... quantizers of later Brevitas releases;
DESIGN.md §9, "Dynamic activation quantizers").

x has any rank >= 1 and a last dimension H; rows = numel / H.  Each result is, by definition, that of an existing
resolved weight graph applied to x2 = x.reshape(rows, H) as the tracked tensor:

    granularity 'tensor'   the per-tensor graph            scale ()                          statistic of all of x
    granularity 'row'      the per-channel graph           scale x.shape[:-1] + (1,)         per row (per token)
    granularity 'group'    the group-wise graph            scale x.shape[:-1] + (H / g, 1)   per g elements of a row

symmetric (ZeroZeroPoint, AbsMax) or asymmetric (RuntimeDynamicStatsZeroPoint of NegativeMinOrZero, AbsMinMax).  The
sub-modules carry the reference's attribute names; none of them has a parameter or a buffer.

Routes ("Routes", row "dynamic").  The composed route is the sub-modules applied one after the other to
the viewed tensor; it serves CPU tensors, config.FUSED_PATHS off, non-contiguous or misaligned inputs and every shape the
kernels refuse.  On the device _route picks the per-channel weight kernels, the group walk or the shifted row kernel.
"""
from typing import Optional, Tuple

import torch
from torch import Tensor
from torch.nn import Module

import brevitas_amd.config as config
from brevitas_amd import _native as nat
from brevitas_amd.core.quant import _fused
from brevitas_amd.core.quant import _recognise as rec
from brevitas_amd.core.scaling.runtime import RuntimeDynamicStatsScaling
from brevitas_amd.core.stats.stats_op import AbsMax
from brevitas_amd.core.zero_point import RuntimeDynamicStatsZeroPoint, ZeroZeroPoint

GRANULARITIES = ('tensor', 'row', 'group')


class DynamicActIntQuant(torch.nn.Module):
    """x -> (y, scale, zero_point, bit_width); see the module docstring.  `per_row`: True unless granularity is 'tensor'
    (an externally scaled bias quantizer needs one input scale, brevitas_amd.nn)."""

    def __init__(self, int_quant: Module, scaling_impl: Module, int_scaling_impl: Module, zero_point_impl: Module,
                 bit_width_impl: Module, granularity: str, group_size: Optional[int] = None):
        super().__init__()
        if granularity not in GRANULARITIES:
            raise ValueError("granularity %r ('tensor', 'row' or 'group')" % (granularity,))
        if granularity == 'group' and (group_size is None or int(group_size) < 1):
            raise ValueError('group_size must be positive, got %r' % (group_size,))
        self.int_quant = int_quant
        self.scaling_impl = scaling_impl
        self.int_scaling_impl = int_scaling_impl
        self.zero_point_impl = zero_point_impl
        self.msb_clamp_bit_width_impl = bit_width_impl
        self.granularity = granularity
        self.group_size = int(group_size) if granularity == 'group' else None

    def extra_repr(self):
        return 'granularity=%s' % self.granularity + (', group_size=%d' % self.group_size if self.group_size else '')

    @property
    def per_row(self) -> bool:
        return self.granularity != 'tensor'

    def _view(self, x: Tensor) -> Tuple[Tensor, Tuple[int, ...]]:
        """-> (x as the sub-modules take it: [rows, H] or [groups, g]; the shape of the scale)"""
        if x.dim() < 1 or x.numel() == 0:
            raise ValueError('dynamic activation quantizer: a tensor of shape %s has no rows' % (tuple(x.shape),))
        h = x.shape[-1]
        if self.granularity == 'tensor':
            return x.reshape(-1, h), ()
        if self.granularity == 'row':
            return x.reshape(-1, h), tuple(x.shape[:-1]) + (1,)
        g = self.group_size
        if h % g != 0:
            raise ValueError('dynamic activation quantizer: the last dimension of a tensor of shape %s is no multiple '
                             'of the group size %d' % (tuple(x.shape), g))
        return x.reshape(-1, g), tuple(x.shape[:-1]) + (h // g, 1)

    def _template(self, bit_width: Tensor):
        """the rec.DynamicTemplate when the sub-modules are the graph the kernels compute (rec.plain_int_quant, the plain
        lower bound of the scale, AbsMax or rec.shifted_zero_point), else None; cached like _stats_template"""
        iq, sc, zpi = self.int_quant, self.scaling_impl, self.zero_point_impl
        ssz = getattr(zpi, 'scale_shift_zero_point', None)
        # everything _build_template reads: the sub-modules, the statistics under them and the flags of the graph
        key = (config.FUSED_PATHS, self.granularity, getattr(iq, 'signed', None), getattr(iq, 'narrow_range', None),
               id(getattr(sc, 'stats_scaling_impl', None)), id(getattr(getattr(sc, 'stats', None), 'stats_impl', None)),
               id(getattr(getattr(zpi, 'stats', None), 'stats_impl', None)), id(ssz), id(getattr(ssz, 'int_quant', None)),
               getattr(ssz, 'quantize_zero_point', None)) + rec.graph_key(self, bit_width)
        return rec.cached(self, '_bvq_dynamic_template', key, lambda: self._build_template(bit_width))

    def _build_template(self, bit_width: Tensor):
        iq, sc, zpi = self.int_quant, self.scaling_impl, self.zero_point_impl
        plain = rec.plain_int_quant(iq, self.int_scaling_impl, bit_width) if config.FUSED_PATHS else None
        if plain is None or type(sc) is not RuntimeDynamicStatsScaling:
            return None
        min_val = sc.stats_scaling_impl.bvq_plain_min_val()
        if min_val is None:
            return None
        dims = (None,) if self.granularity == 'tensor' else (1, -1)
        shifted = type(zpi) is RuntimeDynamicStatsZeroPoint
        if shifted:
            # next to the shared predicate: this class takes any rounding on its symmetric routes, the shifted kernels
            # round half to even only
            if plain.round_mode != nat.ROUND or not rec.shifted_zero_point(
                    iq, sc.stats.stats_impl, zpi.stats.stats_impl, zpi.scale_shift_zero_point, dims):
                return None
        elif type(zpi) is not ZeroZeroPoint or type(sc.stats.stats_impl) is not AbsMax or \
                sc.stats.stats_impl.stats_reduce_dim not in dims:
            return None
        return rec.DynamicTemplate(shifted, min_val, plain.int_thr, *plain[:4])   # qmin, qmax, round_mode, clamp_ste

    def _route(self, xv: Tensor, bit_width: Tensor):
        """the device route of the viewed tensor -> (y, scale, zero_point or None), or None: the composed route"""
        if not (config.FUSED_PATHS and xv.is_cuda and xv.dtype in _fused._FLOATS and xv.is_contiguous()
                and xv.data_ptr() % 16 == 0) or torch._C._get_tracing_state() is not None:
            return None
        tmpl = self._template(bit_width)
        if tmpl is None:
            return None
        shifted, min_val, int_thr, qmin, qmax, round_mode, clamp_ste = tmpl
        rows, h = xv.shape
        if self.granularity == 'group' or (shifted and self.granularity == 'row' and h in rec.GROUP_SIZES):
            if h not in rec.GROUP_SIZES or round_mode != nat.ROUND:
                return None
            if shifted:
                return _fused.GroupShiftedFakeQuantFn.apply(xv, h, min_val, int_thr, qmin, qmax, clamp_ste)
            return _fused.GroupStatsFakeQuantFn.apply(xv, h, min_val, int_thr, qmin, qmax, clamp_ste) + (None,)
        if shifted:
            if self.granularity == 'tensor':
                return None  # no asymmetric per-tensor kernel
            desc, _ = _fused.row_shifted_call(xv, int_thr, qmin, qmax, clamp_ste)
            if not nat.row_shifted_supported(desc, xv):
                return None
            return _fused.RowShiftedFakeQuantFn.apply(xv, min_val, int_thr, qmin, qmax, clamp_ste)
        # symmetric, per tensor or per row: the statistic-scaled weight route on x2, no running statistic
        if self.granularity == 'row' and rows == 1:
            return None  # one row: the per-channel kernels take more than one channel
        if self.granularity == 'tensor':
            sp = _fused.StatsPlan(1, 1, xv.numel(), (), min_val, int_thr)
        else:
            sp = _fused.StatsPlan(1, rows, h, (rows, 1), min_val, int_thr)
        y, scale, _ = _fused.StatsFakeQuantFn.apply(xv, self.int_scaling_impl(bit_width), sp, qmin, qmax, round_mode,
                                                    clamp_ste, None, nat.PRE_NONE, None)
        return y, scale, None

    def forward(self, x: Tensor) -> Tuple[Tensor, Optional[Tensor], Optional[Tensor], Tensor]:
        bit_width = self.msb_clamp_bit_width_impl()
        if getattr(self, 'bvq_collect_only', False):   # calibration: nothing to collect, the tensor passes untouched
            return x, None, None, bit_width
        xv, shape = self._view(x)
        out = self._route(xv, bit_width)
        if out is not None:
            y, scale, zero_point = out
        else:
            # the sub-modules one after the other (the reference's own sequence, B/core/quant/int.py:157-163)
            threshold = self.scaling_impl(xv)
            scale = threshold / self.int_scaling_impl(bit_width)
            zero_point = self.zero_point_impl(xv, scale, bit_width)
            y = self.int_quant(scale, zero_point, bit_width, xv)
        scale = scale.reshape(shape)
        if zero_point is None:
            zero_point = self.zero_point_impl(xv, scale, bit_width)
        elif type(self.zero_point_impl) is not ZeroZeroPoint and zero_point.numel() == scale.numel():
            zero_point = zero_point.reshape(shape)  # a statistic of the rows: one value per row, like the scale
        return y.reshape(x.shape), scale, zero_point, bit_width
