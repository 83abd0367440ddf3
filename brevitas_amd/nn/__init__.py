"""Thin quantized layers: the call sequence of QuantWBIOL.forward_impl (B/nn/quant_layer.py:302-365)
reduced to what configs 4 and 5 need -- quantize the input, re-quantize the weight (every forward, as
the reference does in training), run the float conv / linear on the dequantized tensors.  Brevitas'
own layers (proxies, QuantTensor, export) are out of scope; these exist so that the engine can be
driven end to end without them.
"""
from typing import Callable, Optional

import torch
import torch.nn.functional as F

from brevitas_amd.core.function_wrapper import Identity
from brevitas_amd.core.quant import RescalingIntQuant
from brevitas_amd.core.quant.weight_group import WeightQuantGroup

from .hadamard import HadamardClassifier, HadamardRotation, RotatedModule

__all__ = ['QuantConv2d', 'QuantLinear', 'QuantIdentity', 'QuantReLU', 'QuantSigmoid', 'QuantTanh', 'QuantHardTanh',
           'WeightQuantGroup', 'HadamardRotation', 'RotatedModule', 'HadamardClassifier']

WeightQuantFactory = Callable[[torch.nn.Parameter], RescalingIntQuant]


class _QuantWeightMixin:

    def _init_quant(self, weight_quant: Optional[WeightQuantFactory], input_quant: Optional[torch.nn.Module],
                    bias_quant=None):
        self.weight_quant = weight_quant(self.weight) if weight_quant is not None else None
        self.input_quant = input_quant
        # bias_quant: a module `q(bias, scale)` fed the accumulator's scale (Int8Bias ...), or a factory taking
        # the bias parameter for quantizers with a scale of their own (Int8BiasPerTensorFloatInternalScaling)
        if bias_quant is not None and self.bias is not None and not isinstance(bias_quant, torch.nn.Module):
            bias_quant = bias_quant(self.bias)
        self.bias_quant = bias_quant if self.bias is not None else None
        from brevitas_amd.core.quant.int import GroupwiseRescalingIntQuant, PrescaledRestrictIntQuant
        from brevitas_amd.core.quant.mx import MXQuant
        if isinstance(self.weight_quant, (GroupwiseRescalingIntQuant, MXQuant)) and \
                isinstance(self.bias_quant, PrescaledRestrictIntQuant):
            # one scale per group of input weights: the accumulator the bias is added to has no single scale
            raise ValueError('a group-wise weight quantizer cannot be combined with an externally scaled bias quantizer '
                             '(Int8Bias ... Int32Bias); use a bias quantizer with internal scaling')
        from brevitas_amd.core.quant.dynamic import DynamicActIntQuant
        if isinstance(self.input_quant, DynamicActIntQuant) and self.input_quant.per_row and \
                isinstance(self.bias_quant, PrescaledRestrictIntQuant):
            # one input scale per row (or per group of a row): again no single scale of the accumulator
            raise ValueError('a per-row or per-group dynamic input quantizer (Int8DynamicActPerRowFloat, '
                             'ShiftedUint8DynamicActPerGroupFloat, ...) cannot be combined with an externally scaled bias '
                             'quantizer (Int8Bias ... Int32Bias); use a per-tensor dynamic input quantizer or a bias '
                             'quantizer with internal scaling')
        from brevitas_amd.core.quant.int import WeightNormIntQuant
        if isinstance(self.weight_quant, WeightNormIntQuant) and self.weight_quant.input_bit_width is not None and \
                self.input_quant is not None:
            # an accumulator-aware weight quantizer bounds sum |q| for inputs of a stated width and signedness: an input
            # quantizer whose constant bit width or signedness says otherwise would void the guarantee silently
            want_bw, want_signed = self.weight_quant.input_bit_width, self.weight_quant.input_signed
            bw_impl = getattr(self.input_quant, 'msb_clamp_bit_width_impl', None)
            got_bw = getattr(bw_impl, '_host_value', None)
            got_signed = getattr(getattr(self.input_quant, 'int_quant', None), 'signed', None)
            if (got_bw is not None and got_bw != want_bw) or (got_signed is not None and got_signed != want_signed):
                def say(bw, signed):
                    return '%s-bit %s' % ('?' if bw is None else bw,
                                          '(un)signed' if signed is None else 'signed' if signed else 'unsigned')
                raise ValueError('the accumulator-aware weight quantizer assumes %s inputs (input_bit_width, '
                                 'input_signed), the input quantizer produces %s ones'
                                 % (say(want_bw, want_signed), say(got_bw, got_signed)))

    def _quant_all(self, x):
        """-> (x, w, bias) as the float op consumes them (B/nn/quant_layer.py:302-333)"""
        in_scale = None
        if self.input_quant is not None and not getattr(self, 'bvq_disable_input_quant', False):  # bias correction
            x, in_scale, _, _ = self.input_quant(x)
        w, w_scale, _, _ = self.quant_weight()
        bias = self.bias
        if self.bias_quant is not None and not getattr(self, 'bvq_disable_weight_quant', False):
            from brevitas_amd.core.quant.int import PrescaledRestrictIntQuant
            if isinstance(self.bias_quant, PrescaledRestrictIntQuant):
                if in_scale is None or w_scale is None:
                    raise RuntimeError('Input scale required')  # B/proxy/parameter_quant.py: requires_input_scale
                # the accumulator's scale, one per output channel (or one in all): quant_weight.scale * quant_input.scale
                out_scale = (w_scale.reshape(-1) * in_scale.reshape(-1)).reshape(-1)
                bias = self.bias_quant(self.bias, out_scale)[0]
            else:
                bias = self.bias_quant(self.bias)[0]
        return x, w, bias

    def quant_weight(self):
        """-> (dequantized weight, scale, zero_point, bit_width); identity if no weight quantizer"""
        if self.weight_quant is None or getattr(self, 'bvq_disable_weight_quant', False):  # calibration
            return self.weight, None, None, None
        if self._buffers.get('frozen_weight_scale') is not None:
            # frozen (graph/gptq.py: freeze_weight_quant): the weight holds dequantized codes whose scales the
            # quantizer would not reproduce
            return (self.weight, self.frozen_weight_scale, self.frozen_weight_zero_point,
                    self.weight_quant.msb_clamp_bit_width_impl())
        return self.weight_quant(self.weight)

    def packed_weight(self):
        """-> MXPacked: the weight as packed MX element codes and E8M0 scale bytes (an MX weight quantizer only)"""
        from brevitas_amd.core.quant.mx import MXQuant
        if not isinstance(self.weight_quant, MXQuant):
            raise TypeError('packed_weight: the weight quantizer %s is no MX quantizer'
                            % type(self.weight_quant).__name__)
        return self.weight_quant.to_mx_codes(self.weight)

    def quant_input(self, x):
        return self.input_quant(x)[0] if self.input_quant is not None else x


class QuantConv2d(_QuantWeightMixin, torch.nn.Conv2d):
    """torch.nn.Conv2d with an input quantizer and a per-forward weight quantizer
    (B/nn/quant_conv.py:116-206).  `weight_quant` is a factory taking the layer's weight,
    e.g. brevitas_amd.quant.Int8WeightPerChannelFloat; `input_quant` a tensor_quant module."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1,
                 bias=True, weight_quant: Optional[WeightQuantFactory] = None,
                 input_quant: Optional[torch.nn.Module] = None, bias_quant=None, device=None, dtype=None):
        torch.nn.Conv2d.__init__(self, in_channels, out_channels, kernel_size, stride, padding, dilation, groups,
                                 bias, device=device, dtype=dtype)
        self._init_quant(weight_quant, input_quant, bias_quant)
        if device is not None:
            self.to(device)  # the quantizers' buffers / parameters follow the layer

    def forward(self, x):
        x, w, bias = self._quant_all(x)
        return F.conv2d(x, w, bias, self.stride, self.padding, self.dilation, self.groups)


class QuantLinear(_QuantWeightMixin, torch.nn.Linear):
    """torch.nn.Linear counterpart (B/nn/quant_linear.py:22-73)"""

    def __init__(self, in_features, out_features, bias=True, weight_quant: Optional[WeightQuantFactory] = None,
                 input_quant: Optional[torch.nn.Module] = None, bias_quant=None, device=None, dtype=None):
        torch.nn.Linear.__init__(self, in_features, out_features, bias, device=device, dtype=dtype)
        self._init_quant(weight_quant, input_quant, bias_quant)
        if device is not None:
            self.to(device)

    def forward(self, x):
        x, w, bias = self._quant_all(x)
        return F.linear(x, w, bias)


class QuantIdentity(torch.nn.Module):
    """an activation quantizer as a layer (B/nn/quant_activation.py)"""

    def __init__(self, act_quant: torch.nn.Module):
        super().__init__()
        self.act_quant = act_quant

    def forward(self, x):
        return self.act_quant(x)[0]


_DEFAULT = object()  # act_quant not given: the layer's default quantizer


class _QuantActivation(torch.nn.Module):
    """A non-linear activation followed by its quantizer (QuantNLAL, B/nn/quant_activation.py:14-100, with the proxy of
    B/proxy/runtime_quant.py:102-164): `act_quant` is a tensor_quant module, or None for the plain activation.  The
    quantized form owns a FusedActivationQuantProxy (`act_quant`), which folds ReLU, sigmoid and tanh into the
    quantizer's kernels where they apply; forward returns the dequantized tensor."""

    def __init__(self, act_impl: torch.nn.Module, act_quant: Optional[torch.nn.Module]):
        super().__init__()
        from brevitas_amd.proxy import FusedActivationQuantProxy
        self.act_impl = act_impl
        if act_quant is None:
            self.act_quant = None
        else:
            # the quantizer's clamp replaces a HardTanh (_is_act_enabled, B/proxy/runtime_quant.py:38-45)
            fused_act = Identity() if isinstance(act_impl, torch.nn.Hardtanh) else act_impl
            self.act_quant = FusedActivationQuantProxy(fused_act, act_quant)

    def forward(self, x):
        if self.act_quant is None:
            return self.act_impl(x)
        return self.act_quant(x)[0]


def _default(act_quant, factory):
    return factory() if act_quant is _DEFAULT else act_quant


class QuantReLU(_QuantActivation):
    """nn.ReLU + act_quant (default Uint8ActPerTensorFloat)"""

    def __init__(self, act_quant=_DEFAULT):
        from brevitas_amd.quant import Uint8ActPerTensorFloat
        super().__init__(torch.nn.ReLU(), _default(act_quant, Uint8ActPerTensorFloat))


class QuantSigmoid(_QuantActivation):
    """nn.Sigmoid + act_quant (default Uint8ActPerTensorFloat)"""

    def __init__(self, act_quant=_DEFAULT):
        from brevitas_amd.quant import Uint8ActPerTensorFloat
        super().__init__(torch.nn.Sigmoid(), _default(act_quant, Uint8ActPerTensorFloat))


class QuantTanh(_QuantActivation):
    """nn.Tanh + act_quant (default Int8ActPerTensorFloat)"""

    def __init__(self, act_quant=_DEFAULT):
        from brevitas_amd.quant import Int8ActPerTensorFloat
        super().__init__(torch.nn.Tanh(), _default(act_quant, Int8ActPerTensorFloat))


class QuantHardTanh(_QuantActivation):
    """nn.Hardtanh(min_val, max_val) + act_quant (default Int8ActPerTensorFloatMinMaxInit(min_val, max_val)).  With a
    quantizer the HardTanh itself is dropped -- the quantizer's clamp replaces it -- except in a calibration forward,
    which hands on hardtanh(x) as the reference's calibration hook does (B/graph/calibrate.py:112-123)."""

    def __init__(self, min_val: float = -1.0, max_val: float = 1.0, act_quant=_DEFAULT):
        from brevitas_amd.quant import Int8ActPerTensorFloatMinMaxInit
        if act_quant is _DEFAULT:
            act_quant = Int8ActPerTensorFloatMinMaxInit(min_val, max_val)
        super().__init__(torch.nn.Hardtanh(min_val, max_val), act_quant)
        self.min_val, self.max_val = float(min_val), float(max_val)

    def forward(self, x):
        y = super().forward(x)
        if self.act_quant is not None and getattr(self.act_quant.tensor_quant, 'bvq_collect_only', False):
            y = F.hardtanh(y, self.min_val, self.max_val)
        return y
