"""Resolved module graphs of the named quantizers on the accelerated path.

In Brevitas these are injector classes (B/quant/scaled_int.py:144-193) that the solvers
(B/quant/solver/*.py) resolve into a `tensor_quant` module graph; the injector machinery itself is
out of scope, so the functions here assemble exactly the graphs the solvers produce
(SURVEY 8a lists them with file:line) from brevitas_amd's same-named modules.  Each returns the
`tensor_quant` a proxy would own: `q(x) -> (y, scale, zero_point, bit_width)`.
"""
from typing import List, Optional, Sequence, Union

import torch

from brevitas_amd.core.bit_width import BitWidthConst
from brevitas_amd.core.function_wrapper import (CeilSte, OverOutputChannelView, OverSubChannelBlockView, OverTensorView,
                                                RoundSte, TensorClamp, TensorClampSte)
from brevitas_amd.core.quant import (DynamicActIntQuant, GroupwiseHQOIntQuant, GroupwiseMSEIntQuant,
                                     GroupwiseRescalingIntQuant, IntQuant, MXQuant, PrescaledRestrictIntQuant, RescalingIntQuant, WeightNormIntQuant)
from brevitas_amd.core.restrict_val import FloatRestrictValue, PowerOfTwoRestrictValue
from brevitas_amd.core.scaling import (AccumulatorAwareParameterPreScaling, IntScaling,
                                       ParameterFromRuntimeStatsScaling, ParameterPreScalingWeightNorm, ParameterScaling,
                                       PowerOfTwoIntScaling, RuntimeDynamicStatsScaling, RuntimeStatsScaling,
                                       StatsFromParameterScaling)
from brevitas_amd.core.stats import (AbsMax, AbsMinMax, AbsPercentile, NegativeMinOrZero, NegativePercentileOrZero,
                                     PercentileInterval)
from brevitas_amd.core.zero_point import (ParameterFromRuntimeZeroPoint, RuntimeDynamicStatsZeroPoint,
                                          StatsFromParameterZeroPoint, ZeroZeroPoint)

__all__ = ['Int8WeightPerChannelFloat', 'Int4WeightPerChannelFloat', 'Int8WeightPerGroupFloat',
           'Int4WeightPerGroupFloat', 'Int8WeightPerGroupFloatMSE', 'Int4WeightPerGroupFloatMSE',
           'Int8WeightPerTensorFloat',
           'Int8ActPerTensorFloat', 'Uint8ActPerTensorFloat', 'Int8ActPerChannelFloat',
           'ShiftedUint8WeightPerTensorFloat', 'ShiftedUint8WeightPerChannelFloat', 'ShiftedUint8ActPerTensorFloat',
           'ShiftedUint8WeightPerGroupFloat', 'ShiftedUint4WeightPerGroupFloat',
           'ShiftedUint8WeightPerGroupFloatHQO', 'ShiftedUint4WeightPerGroupFloatHQO',
           'Int8WeightPerTensorFixedPoint', 'Int8WeightPerChannelFixedPoint', 'Int8ActPerTensorFixedPoint',
           'Int8ActPerTensorFloatMinMaxInit', 'Uint8ActPerTensorFloatMaxInit',
           'Uint8ActPerTensorFixedPoint', 'Uint8ActPerTensorFixedPointMaxInit', 'Int8Bias', 'Int16Bias', 'Int24Bias',
           'Int32Bias', 'Int8BiasPerTensorFloatInternalScaling', 'Int8BiasPerTensorFixedPointInternalScaling',
           'MXFloat8e4m3Weight', 'MXFloat8e5m2Weight', 'MXFloat6e3m2Weight', 'MXFloat6e2m3Weight', 'MXFloat4e2m1Weight',
           'MXInt8Weight', 'MXFloat8e4m3Act', 'MXFloat8e5m2Act', 'MXFloat6e3m2Act', 'MXFloat6e2m3Act', 'MXFloat4e2m1Act',
           'MXInt8Act',
           'Int8DynamicActPerTensorFloat', 'Int8DynamicActPerRowFloat', 'Int8DynamicActPerGroupFloat',
           'ShiftedUint8DynamicActPerTensorFloat', 'ShiftedUint8DynamicActPerRowFloat',
           'ShiftedUint8DynamicActPerGroupFloat',
           'Int8WeightNormL2PerChannelFloat', 'Int8AccumulatorAwareWeightQuant', 'Int4AccumulatorAwareWeightQuant']

SCALING_MIN_VAL = 1e-10  # B/quant/base.py:115-123, 169-182


def _params(weights) -> List[torch.nn.Parameter]:
    return list(weights) if isinstance(weights, (list, tuple)) else [weights]


def Int8WeightPerChannelFloat(weights: Union[torch.nn.Parameter, Sequence[torch.nn.Parameter]],
                              bit_width: int = 8) -> RescalingIntQuant:
    """NarrowIntQuant + MaxStatsScaling + PerChannelFloatScaling8bit + WeightQuantSolver
    (B/quant/scaled_int.py:157-167): scale[c] = max(max_k |w[c,k]|, 1e-10) / (2^(b-1) - 1), narrow signed range,
    straight-through clamp; weights are re-quantized on every forward."""
    tracked = _params(weights)
    w = tracked[0]
    shape = (w.shape[0],) + (1,) * (w.dim() - 1)
    return RescalingIntQuant(
        IntQuant(narrow_range=True, signed=True, float_to_int_impl=RoundSte(), tensor_clamp_impl=TensorClampSte()),
        StatsFromParameterScaling(AbsMax(1), OverOutputChannelView(None), 1, tracked, FloatRestrictValue(), shape,
                                  affine_rescaling=False, scaling_min_val=SCALING_MIN_VAL),
        IntScaling(signed=True, narrow_range=True), ZeroZeroPoint(), BitWidthConst(bit_width))


def Int4WeightPerChannelFloat(weights) -> RescalingIntQuant:
    """not in this reference snapshot; defined as Int8WeightPerChannelFloat with bit_width = 4"""
    return Int8WeightPerChannelFloat(weights, bit_width=4)


def _group_tracked_weight(weights, group_size: int) -> tuple:
    """(the one tracked weight as a list, group size, scaling shape) of a group-wise weight quantizer, checked"""
    tracked = _params(weights)
    if len(tracked) != 1:
        raise ValueError('a group-wise weight quantizer tracks exactly one weight, got a list of %d' % len(tracked))
    w = tracked[0]
    group_size = int(group_size)
    if w.dim() < 2 or group_size < 1 or (w.numel() // max(w.shape[0], 1)) % group_size != 0:
        raise ValueError('a weight of shape %s has no whole groups of %d elements per output channel'
                         % (tuple(w.shape), group_size))
    return tracked, group_size, (w.numel() // group_size, 1)


def _group_weight_modules(weights, group_size: int, bit_width: int) -> tuple:
    """the constructor arguments of GroupwiseRescalingIntQuant for one tracked weight, its shape checked here"""
    tracked, group_size, shape = _group_tracked_weight(weights, group_size)
    return (
        IntQuant(narrow_range=True, signed=True, float_to_int_impl=RoundSte(), tensor_clamp_impl=TensorClampSte()),
        StatsFromParameterScaling(AbsMax(1), OverSubChannelBlockView(group_size), 1, tracked, FloatRestrictValue(),
                                  shape, affine_rescaling=False, scaling_min_val=SCALING_MIN_VAL),
        IntScaling(signed=True, narrow_range=True), ZeroZeroPoint(), BitWidthConst(bit_width), group_size)


def Int8WeightPerGroupFloat(weights: Union[torch.nn.Parameter, Sequence[torch.nn.Parameter]], group_size: int = 128,
                            bit_width: int = 8) -> GroupwiseRescalingIntQuant:
    """Int8WeightPerChannelFloat with one scale per `group_size` consecutive input weights of each output channel
    (Int8WeightPerGroupFloat of later Brevitas releases; not in this reference snapshot): the per-channel graph on the
    weight regrouped as [out * K / group_size, group_size], K = Cin * kh * kw in memory order.  y has the weight's
    shape, scale is (out, K / group_size, 1).  In a layer: weight_quant=functools.partial(Int8WeightPerGroupFloat,
    group_size=64).  One tracked weight only: the groups of several weights do not line up."""
    return GroupwiseRescalingIntQuant(*_group_weight_modules(weights, group_size, bit_width))


def Int4WeightPerGroupFloat(weights, group_size: int = 128) -> GroupwiseRescalingIntQuant:
    """Int8WeightPerGroupFloat with bit_width = 4: the usual weight-only format of LLM-sized linear layers"""
    return Int8WeightPerGroupFloat(weights, group_size=group_size, bit_width=4)


def Int8WeightPerGroupFloatMSE(weights, group_size: int = 128, bit_width: int = 8, mse_iters: int = 20,
                               mse_step: float = 0.025,
                               mse_ratios: Optional[Sequence[float]] = None) -> GroupwiseMSEIntQuant:
    """Int8WeightPerGroupFloat whose threshold is searched per group (core/quant/int.py: GroupwiseMSEIntQuant; the
    `MSE` statistic of later Brevitas releases and the clip search of AWQ-style recipes, not in this reference
    snapshot): of the candidates abs-max * ratio a group takes the first one with the smallest squared quantization
    error.  ratios = [1 - i * mse_step for i in range(mse_iters)] unless `mse_ratios` lists them (the first is 1, every
    one in (0, 1]).  Same outputs, state-dict keys and layer use as Int8WeightPerGroupFloat:
    weight_quant=functools.partial(Int4WeightPerGroupFloatMSE, group_size=64); the chosen candidates of the last forward
    are `last_mse_index`."""
    if mse_ratios is None:
        if int(mse_iters) < 1:
            raise ValueError('mse_iters must be at least 1, got %r' % (mse_iters,))
        mse_ratios = [1.0 - i * float(mse_step) for i in range(int(mse_iters))]
    return GroupwiseMSEIntQuant(*_group_weight_modules(weights, group_size, bit_width), mse_ratios)


def Int4WeightPerGroupFloatMSE(weights, group_size: int = 128, mse_iters: int = 20, mse_step: float = 0.025,
                               mse_ratios: Optional[Sequence[float]] = None) -> GroupwiseMSEIntQuant:
    """Int8WeightPerGroupFloatMSE with bit_width = 4: at 4 bits nearly every group clips below its abs-max"""
    return Int8WeightPerGroupFloatMSE(weights, group_size=group_size, bit_width=4, mse_iters=mse_iters,
                                      mse_step=mse_step, mse_ratios=mse_ratios)


def _mx_weight(element_format: str, weights, group_size: int, scale_rule: str) -> MXQuant:
    """an MX weight quantizer (core/quant/mx.py; MXFloat8e4m3Weight ... of later Brevitas releases, not in this
    reference snapshot): groups of `group_size` consecutive input weights of each output channel, K = Cin * kh * kw in
    memory order, share one power-of-two scale; straight-through clamp, as the integer weight quantizers.  y has the
    weight's shape, scale is float32 (out, K / group_size, 1).  One tracked weight, its shape checked here."""
    tracked = _params(weights)
    if len(tracked) != 1:
        raise ValueError('an MX weight quantizer tracks exactly one weight, got a list of %d' % len(tracked))
    w = tracked[0]
    group_size = int(group_size)
    if w.dim() < 2 or group_size < 1 or (w.numel() // max(w.shape[0], 1)) % group_size != 0:
        raise ValueError('a weight of shape %s has no whole groups of %d elements per output channel'
                         % (tuple(w.shape), group_size))
    return MXQuant(element_format, group_size=group_size, scale_rule=scale_rule, clamp_ste=True, group_axis='flat')


def _mx_act(element_format: str, group_size: int, scale_rule: str) -> MXQuant:
    """an MX activation quantizer: dynamic, one power-of-two scale per `group_size` elements of the last dimension,
    plain clamp; scale is float32 x.shape[:-1] + (x.shape[-1] / group_size, 1)"""
    return MXQuant(element_format, group_size=int(group_size), scale_rule=scale_rule, clamp_ste=False,
                   group_axis='last')


def MXFloat8e4m3Weight(weights, group_size: int = 32, scale_rule: str = 'floor') -> MXQuant:
    return _mx_weight('e4m3', weights, group_size, scale_rule)


def MXFloat8e5m2Weight(weights, group_size: int = 32, scale_rule: str = 'floor') -> MXQuant:
    return _mx_weight('e5m2', weights, group_size, scale_rule)


def MXFloat6e3m2Weight(weights, group_size: int = 32, scale_rule: str = 'floor') -> MXQuant:
    return _mx_weight('e3m2', weights, group_size, scale_rule)


def MXFloat6e2m3Weight(weights, group_size: int = 32, scale_rule: str = 'floor') -> MXQuant:
    return _mx_weight('e2m3', weights, group_size, scale_rule)


def MXFloat4e2m1Weight(weights, group_size: int = 32, scale_rule: str = 'floor') -> MXQuant:
    return _mx_weight('e2m1', weights, group_size, scale_rule)


def MXInt8Weight(weights, group_size: int = 32, scale_rule: str = 'floor') -> MXQuant:
    return _mx_weight('int8', weights, group_size, scale_rule)


def MXFloat8e4m3Act(group_size: int = 32, scale_rule: str = 'floor') -> MXQuant:
    return _mx_act('e4m3', group_size, scale_rule)


def MXFloat8e5m2Act(group_size: int = 32, scale_rule: str = 'floor') -> MXQuant:
    return _mx_act('e5m2', group_size, scale_rule)


def MXFloat6e3m2Act(group_size: int = 32, scale_rule: str = 'floor') -> MXQuant:
    return _mx_act('e3m2', group_size, scale_rule)


def MXFloat6e2m3Act(group_size: int = 32, scale_rule: str = 'floor') -> MXQuant:
    return _mx_act('e2m3', group_size, scale_rule)


def MXFloat4e2m1Act(group_size: int = 32, scale_rule: str = 'floor') -> MXQuant:
    return _mx_act('e2m1', group_size, scale_rule)


def MXInt8Act(group_size: int = 32, scale_rule: str = 'floor') -> MXQuant:
    return _mx_act('int8', group_size, scale_rule)


def _weight_norm_scaling(weights, bit_width: int) -> tuple:
    """(the one tracked weight, its learned per-channel scale starting at absmax_c / qmax) of a weight-norm quantizer"""
    tracked = _params(weights)
    if len(tracked) != 1:
        raise ValueError('a weight-norm quantizer tracks exactly one weight, got a list of %d' % len(tracked))
    w = tracked[0]
    if w.dim() < 2 or w.numel() == 0:
        raise ValueError('a weight-norm quantizer needs a weight of at least 2 dimensions, got shape %s'
                         % (tuple(w.shape),))
    shape = (w.shape[0],) + (1,) * (w.dim() - 1)
    absmax = w.detach().reshape(w.shape[0], -1).float().abs().max(dim=1).values.reshape(shape)
    init = torch.clamp_min(absmax, SCALING_MIN_VAL) / float(2 ** (bit_width - 1) - 1)
    return w, ParameterScaling(init, shape, FloatRestrictValue(), scaling_min_val=SCALING_MIN_VAL)


def Int8WeightNormL2PerChannelFloat(weights, bit_width: int = 8) -> WeightNormIntQuant:
    """Per output channel w = g * v / ||v||_2 quantized with a learned scale s to the narrow signed range, half-even
    rounding, straight-through clamp (Int8WeightNormL2PerChannelFloat of later Brevitas releases; not in this reference
    snapshot).  g starts at ||v||_2 and s at absmax / (2^(b-1) - 1), so that y reproduces v to within one code step at
    step 0.  Parameters: scaling_impl.value (s) and pre_scaling_impl.value (g), both (out, 1, ..., 1)."""
    w, scaling = _weight_norm_scaling(weights, bit_width)
    return WeightNormIntQuant(scaling, ParameterPreScalingWeightNorm(w, 'l2'), BitWidthConst(bit_width), 'l2')


def Int8AccumulatorAwareWeightQuant(weights, accumulator_bit_width: int = 32, input_bit_width: int = 8,
                                    input_signed: bool = False, bit_width: int = 8) -> WeightNormIntQuant:
    """A2Q (Int8AccumulatorAwareWeightQuant of later Brevitas releases; not in this reference snapshot): the weight-norm
    quantizer over the L1 norm with round-to-zero, its g capped at T * s, T = (2^(P-1) - 1) * 2^(sigma - N) for a P-bit
    accumulator and N-bit inputs (sigma = 1 when they are signed), so that the integer weights of every output channel
    satisfy sum |q| <= T and a dot product with such inputs cannot overflow the accumulator.  In a layer:
    weight_quant=functools.partial(Int8AccumulatorAwareWeightQuant, accumulator_bit_width=16); the layer checks its
    input quantizer against input_bit_width / input_signed."""
    w, scaling = _weight_norm_scaling(weights, bit_width)
    pre = AccumulatorAwareParameterPreScaling(w, accumulator_bit_width, input_bit_width, input_signed)
    return WeightNormIntQuant(scaling, pre, BitWidthConst(bit_width), 'l1')


def Int4AccumulatorAwareWeightQuant(weights, accumulator_bit_width: int = 32, input_bit_width: int = 8,
                                    input_signed: bool = False) -> WeightNormIntQuant:
    """Int8AccumulatorAwareWeightQuant with bit_width = 4"""
    return Int8AccumulatorAwareWeightQuant(weights, accumulator_bit_width, input_bit_width, input_signed, bit_width=4)


def Int8WeightPerTensorFloat(weights, bit_width: int = 8) -> RescalingIntQuant:
    """B/quant/scaled_int.py:144-154: one scale for the whole weight tensor"""
    tracked = _params(weights)
    return RescalingIntQuant(
        IntQuant(narrow_range=True, signed=True, float_to_int_impl=RoundSte(), tensor_clamp_impl=TensorClampSte()),
        StatsFromParameterScaling(AbsMax(), OverTensorView(), 0, tracked, FloatRestrictValue(), (),
                                  affine_rescaling=False, scaling_min_val=SCALING_MIN_VAL),
        IntScaling(signed=True, narrow_range=True), ZeroZeroPoint(), BitWidthConst(bit_width))


def _act_quant(signed: bool, bit_width: int, scaling_impl_type: str, collect_stats_steps: int,
               channels: Optional[int], scaling_init: Optional[float], scaling_stats_op: str = 'max'
               ) -> RescalingIntQuant:
    if channels is None:
        # the reference's default statistic is the 99.999th percentile (B/quant/base.py:68-75);
        # scaling_stats_op='max' is its supported StatsOp.MAX override
        stats = AbsPercentile(99.999, None) if scaling_stats_op == 'percentile' else AbsMax()
        view, shape = OverTensorView(), ()
    else:
        # scaling_per_output_channel=True, per_channel_broadcastable_shape=(1,C,1,1),
        # scaling_stats_permute_dims=(1,0,2,3)  (B/quant/solver/act.py:91-105)
        view, stats, shape = OverOutputChannelView((1, 0, 2, 3)), AbsMax(1), (1, channels, 1, 1)
    if scaling_impl_type == 'parameter_from_stats':
        scaling = ParameterFromRuntimeStatsScaling(collect_stats_steps, stats, view, shape, FloatRestrictValue(),
                                                   0.1, SCALING_MIN_VAL)
    elif scaling_impl_type == 'stats':
        scaling = RuntimeStatsScaling(stats, view, FloatRestrictValue(), shape, affine_rescaling=False,
                                      scaling_stats_momentum=0.1, scaling_min_val=SCALING_MIN_VAL)
    elif scaling_impl_type == 'parameter':
        scaling = ParameterScaling(scaling_init, shape if shape else None, FloatRestrictValue(), SCALING_MIN_VAL)
    else:
        raise ValueError("scaling_impl_type must be 'parameter_from_stats', 'stats' or 'parameter'")
    return RescalingIntQuant(
        IntQuant(narrow_range=False, signed=signed, float_to_int_impl=RoundSte(), tensor_clamp_impl=TensorClamp()),
        scaling, IntScaling(signed=signed, narrow_range=False), ZeroZeroPoint(), BitWidthConst(bit_width))


def Int8ActPerTensorFloat(scaling_impl_type: str = 'parameter_from_stats', collect_stats_steps: int = 300,
                          bit_width: int = 8, scaling_init: Optional[float] = None,
                          scaling_stats_op: str = 'percentile') -> RescalingIntQuant:
    """IntQuant + ParamFromRuntimePercentileScaling + PerTensorFloatScaling8bit + ActQuantSolver
    (B/quant/scaled_int.py:170-180): collects the 99.999th percentile of |x| (scaling_stats_op='max':
    AbsMax, the reference's StatsOp.MAX override) for `collect_stats_steps` training steps, then learns
    the scale."""
    return _act_quant(True, bit_width, scaling_impl_type, collect_stats_steps, None, scaling_init,
                      scaling_stats_op)


def Uint8ActPerTensorFloat(scaling_impl_type: str = 'parameter_from_stats', collect_stats_steps: int = 300,
                           bit_width: int = 8, scaling_init: Optional[float] = None,
                           scaling_stats_op: str = 'percentile') -> RescalingIntQuant:
    """unsigned variant for post-ReLU activations (B/quant/scaled_int.py:183-193)"""
    return _act_quant(False, bit_width, scaling_impl_type, collect_stats_steps, None, scaling_init,
                      scaling_stats_op)


def _act_min_max_init(signed: bool, min_val: float, max_val: float, bit_width: int) -> RescalingIntQuant:
    # MinMaxScalingInit (B/quant/solver/act.py:17-23): a float32 scalar max(|min_val|, |max_val|)
    init = torch.tensor(max(abs(float(min_val)), abs(float(max_val))))
    return RescalingIntQuant(
        IntQuant(narrow_range=False, signed=signed, float_to_int_impl=RoundSte(), tensor_clamp_impl=TensorClamp()),
        ParameterScaling(init, None, FloatRestrictValue(), None),
        IntScaling(signed=signed, narrow_range=False), ZeroZeroPoint(), BitWidthConst(bit_width))


def Int8ActPerTensorFloatMinMaxInit(min_val: float, max_val: float, bit_width: int = 8) -> RescalingIntQuant:
    """IntQuant + ParamMinMaxInitScaling + PerTensorFloatScaling8bit + ActQuantSolver (B/quant/scaled_int.py:32-46):
    a learned per-tensor scale initialised to max(|min_val|, |max_val|) / 2^(b-1); the default of QuantHardTanh"""
    return _act_min_max_init(True, min_val, max_val, bit_width)


def Uint8ActPerTensorFloatMaxInit(max_val: float, bit_width: int = 8) -> RescalingIntQuant:
    """UintQuant + ParamMinMaxInitScaling + PerTensorFloatScaling8bit + ActQuantSolver (B/quant/scaled_int.py:49-62):
    min_val = 0, a learned per-tensor scale initialised to |max_val| / (2^b - 1)"""
    return _act_min_max_init(False, 0.0, max_val, bit_width)


def Int8ActPerChannelFloat(channels: int, scaling_impl_type: str = 'stats', collect_stats_steps: int = 300,
                           bit_width: int = 8) -> RescalingIntQuant:
    """Int8ActPerTensorFloat with scaling_per_output_channel=True over NCHW channel `channels`
    (the layout of BASELINE.json's metric)"""
    return _act_quant(True, bit_width, scaling_impl_type, collect_stats_steps, channels, None)


def _shifted_weight_quant(weights, per_channel: bool, bit_width: int) -> RescalingIntQuant:
    """ShiftedMinUintQuant + MinMaxStatsScaling (B/quant/base.py:60-65,137-150): unsigned codes, scale from
    max - min, integer zero-point from -min / scale; both statistics are back-propagated through"""
    tracked = _params(weights)
    w = tracked[0]
    if per_channel:
        shape = (w.shape[0],) + (1,) * (w.dim() - 1)
        view = lambda: OverOutputChannelView(None)  # noqa: E731
        scale_stat, zp_stat, cat = AbsMinMax(1), NegativeMinOrZero(1), 1
    else:
        shape = ()
        view = lambda: OverTensorView()  # noqa: E731
        scale_stat, zp_stat, cat = AbsMinMax(), NegativeMinOrZero(), 0
    int_quant = IntQuant(narrow_range=False, signed=False, float_to_int_impl=RoundSte(),
                         tensor_clamp_impl=TensorClampSte())
    return RescalingIntQuant(
        int_quant,
        StatsFromParameterScaling(scale_stat, view(), cat, tracked, FloatRestrictValue(), shape,
                                  affine_rescaling=False, scaling_min_val=SCALING_MIN_VAL),
        IntScaling(signed=False, narrow_range=False),
        StatsFromParameterZeroPoint(int_quant, True, view(), cat, zp_stat, shape, tracked),
        BitWidthConst(bit_width))


def ShiftedUint8WeightPerTensorFloat(weights, bit_width: int = 8) -> RescalingIntQuant:
    """B/quant/shifted_scaled_int.py:37-52"""
    return _shifted_weight_quant(weights, False, bit_width)


def ShiftedUint8WeightPerChannelFloat(weights, bit_width: int = 8) -> RescalingIntQuant:
    """B/quant/shifted_scaled_int.py:55-70"""
    return _shifted_weight_quant(weights, True, bit_width)


def ShiftedUint8WeightPerGroupFloat(weights: Union[torch.nn.Parameter, Sequence[torch.nn.Parameter]],
                                    group_size: int = 128, bit_width: int = 8) -> GroupwiseRescalingIntQuant:
    """ShiftedUint8WeightPerChannelFloat with one scale and one integer zero-point per `group_size` consecutive input
    weights of each output channel (ShiftedUint8WeightPerGroupFloat of later Brevitas releases, the unsigned format of
    AWQ / GPTQ style checkpoints; not in this reference snapshot): the per-channel graph on the weight regrouped as
    [out * K / group_size, group_size], K = Cin * kh * kw in memory order.  Per group
        scale = max(|max - min|, 1e-10) / (2^b - 1),  zero_point = clamp(round(-min(min, 0) / scale), 0, 2^b - 1),
        y = (clamp(round(w / scale + zero_point), 0, 2^b - 1) - zero_point) * scale.
    y has the weight's shape; scale and zero_point are (out, K / group_size, 1), the zero-point integer-valued in the
    weight's dtype; both statistics are back-propagated through.  In a layer:
    weight_quant=functools.partial(ShiftedUint4WeightPerGroupFloat, group_size=64).  One tracked weight only.

    The range is the reference's max - min: a group of positive values only gets zero-point 0 and clips its upper part,
    one of negative values only gets 2^b - 1 and clips likewise, a constant non-zero group gets the lower bound of the
    scale.  y and the gradients stay finite in all of them."""
    return GroupwiseRescalingIntQuant(*_shifted_group_weight_modules(weights, group_size, bit_width))


def _shifted_group_weight_modules(weights, group_size: int, bit_width: int) -> tuple:
    """the constructor arguments of the asymmetric GroupwiseRescalingIntQuant for one tracked weight, its shape checked
    here"""
    tracked, group_size, shape = _group_tracked_weight(weights, group_size)
    int_quant = IntQuant(narrow_range=False, signed=False, float_to_int_impl=RoundSte(),
                         tensor_clamp_impl=TensorClampSte())
    return (
        int_quant,
        StatsFromParameterScaling(AbsMinMax(1), OverSubChannelBlockView(group_size), 1, tracked, FloatRestrictValue(),
                                  shape, affine_rescaling=False, scaling_min_val=SCALING_MIN_VAL),
        IntScaling(signed=False, narrow_range=False),
        StatsFromParameterZeroPoint(int_quant, True, OverSubChannelBlockView(group_size), 1, NegativeMinOrZero(1), shape,
                                    tracked),
        BitWidthConst(bit_width), group_size)


def ShiftedUint4WeightPerGroupFloat(weights, group_size: int = 128) -> GroupwiseRescalingIntQuant:
    """ShiftedUint8WeightPerGroupFloat with bit_width = 4: the usual asymmetric weight-only format of LLM-sized layers"""
    return ShiftedUint8WeightPerGroupFloat(weights, group_size=group_size, bit_width=4)


def ShiftedUint8WeightPerGroupFloatHQO(weights, group_size: int = 128, bit_width: int = 8, hqo_iters: int = 20,
                                       hqo_beta: float = 10.0, hqo_kappa: float = 1.01,
                                       hqo_lp_norm: float = 0.5) -> GroupwiseHQOIntQuant:
    """ShiftedUint8WeightPerGroupFloat whose zero-point is searched per group by half-quadratic optimisation
    (core/quant/int.py: GroupwiseHQOIntQuant; HQQ, HalfQuadraticOptimizerZeroPoint of later Brevitas releases, not in
    this reference snapshot): data-free, up to `hqo_iters` proximal steps of the l_p norm p = `hqo_lp_norm` at the
    strength hqo_beta * hqo_kappa^i move a real-valued zero-point from the integer one towards a lower summed |w - y|;
    the scale stays max - min.  Same outputs, state-dict keys and layer use as ShiftedUint8WeightPerGroupFloat:
    weight_quant=functools.partial(ShiftedUint4WeightPerGroupFloatHQO, group_size=64); zero_point is a value of the
    weight's dtype, in general no integer, and receives no gradient; the kept candidates of the last forward are
    `last_hqo_index`.  Group sizes 16, 32, 64, 128 and 256.  With 8 bits in bfloat16 the zero-point has almost no
    fractional bits and nearly every group keeps the integer one."""
    return GroupwiseHQOIntQuant(*_shifted_group_weight_modules(weights, group_size, bit_width), hqo_iters=hqo_iters,
                                hqo_beta=hqo_beta, hqo_kappa=hqo_kappa, hqo_lp_norm=hqo_lp_norm)


def ShiftedUint4WeightPerGroupFloatHQO(weights, group_size: int = 128, hqo_iters: int = 20, hqo_beta: float = 10.0,
                                       hqo_kappa: float = 1.01, hqo_lp_norm: float = 0.5) -> GroupwiseHQOIntQuant:
    """ShiftedUint8WeightPerGroupFloatHQO with bit_width = 4: where the zero-point's fraction matters most"""
    return ShiftedUint8WeightPerGroupFloatHQO(weights, group_size=group_size, bit_width=4, hqo_iters=hqo_iters,
                                              hqo_beta=hqo_beta, hqo_kappa=hqo_kappa, hqo_lp_norm=hqo_lp_norm)


def ShiftedUint8ActPerTensorFloat(collect_stats_steps: int = 300, bit_width: int = 8) -> RescalingIntQuant:
    """ShiftedParamFromPercentileUintQuant + ParamFromRuntimePercentileIntervalScaling
    (B/quant/shifted_scaled_int.py:19-34, base.py:87-95,153-166): scale from the 0.001..99.999 percentile
    interval and zero-point from the 0.001th percentile, both collected for `collect_stats_steps`
    training steps and then learned"""
    int_quant = IntQuant(narrow_range=False, signed=False, float_to_int_impl=RoundSte(), tensor_clamp_impl=TensorClamp())
    return RescalingIntQuant(
        int_quant,
        ParameterFromRuntimeStatsScaling(collect_stats_steps, PercentileInterval(0.001, 99.999, None),
                                         OverTensorView(), (), FloatRestrictValue(), 0.1, SCALING_MIN_VAL),
        IntScaling(signed=False, narrow_range=False),
        ParameterFromRuntimeZeroPoint(collect_stats_steps, int_quant, True, NegativePercentileOrZero(0.001, None),
                                      (), OverTensorView(), 0.1),
        BitWidthConst(bit_width))


# ---- dynamic activation quantizers: scale (and zero-point) from the tensor being quantized -----------------------------

def _dynamic_act_quant(shifted: bool, granularity: str, bit_width: int, group_size: Optional[int] = None
                       ) -> DynamicActIntQuant:
    """The weight graph of the same granularity with the current input, viewed [rows, H], in the tracked weight's place
    (core/quant/dynamic.py): plain clamp, full range, scaling_min_val 1e-10, float scales.  Stateless."""
    if granularity == 'tensor':
        view, dim, shape = OverTensorView, None, ()
    elif granularity == 'row':
        view, dim, shape = (lambda: OverOutputChannelView(None)), 1, (-1, 1)
    else:
        view, dim, shape = (lambda: OverSubChannelBlockView(int(group_size))), 1, (-1, 1)
    int_quant = IntQuant(narrow_range=False, signed=not shifted, float_to_int_impl=RoundSte(),
                         tensor_clamp_impl=TensorClamp())
    scaling = RuntimeDynamicStatsScaling(AbsMinMax(dim) if shifted else AbsMax(dim), view(), FloatRestrictValue(), shape,
                                         SCALING_MIN_VAL)
    zero_point = RuntimeDynamicStatsZeroPoint(int_quant, True, view(), NegativeMinOrZero(dim), shape) if shifted \
        else ZeroZeroPoint()
    return DynamicActIntQuant(int_quant, scaling, IntScaling(signed=not shifted, narrow_range=False), zero_point,
                              BitWidthConst(bit_width), granularity, group_size)


def Int8DynamicActPerTensorFloat(bit_width: int = 8) -> DynamicActIntQuant:
    """Int8DynamicActPerTensorFloat of later Brevitas releases: one scale, max |x| / 2^(b-1) of the current input, in
    training and in eval; no buffer, no parameter.  The Int8WeightPerTensorFloat graph on the input with a plain clamp and
    the full signed range.  scale is 0-dim (float32 for every input dtype, as a 0-dim statistic promotes)."""
    return _dynamic_act_quant(False, 'tensor', bit_width)


def Int8DynamicActPerRowFloat(bit_width: int = 8) -> DynamicActIntQuant:
    """one scale per row of the last dimension (per token): the Int8WeightPerChannelFloat graph on x.reshape(rows, H);
    scale is x.shape[:-1] + (1,) in x's dtype"""
    return _dynamic_act_quant(False, 'row', bit_width)


def Int8DynamicActPerGroupFloat(group_size: int = 32, bit_width: int = 8) -> DynamicActIntQuant:
    """one scale per `group_size` consecutive elements of the last dimension: the Int8WeightPerGroupFloat graph on
    x.reshape(rows, H); scale is x.shape[:-1] + (H / group_size, 1).  H must be a multiple of the group size."""
    return _dynamic_act_quant(False, 'group', bit_width, group_size)


def ShiftedUint8DynamicActPerTensorFloat(bit_width: int = 8) -> DynamicActIntQuant:
    """asymmetric: unsigned codes, scale = max(|max - min|, 1e-10) / (2^b - 1) and an integer zero-point from the current
    input; the ShiftedUint8WeightPerTensorFloat graph on the input with a plain clamp.  Runs as the composed route on the
    device too."""
    return _dynamic_act_quant(True, 'tensor', bit_width)


def ShiftedUint8DynamicActPerRowFloat(bit_width: int = 8) -> DynamicActIntQuant:
    """one scale and one integer zero-point per row of the last dimension (per token): the
    ShiftedUint8WeightPerChannelFloat graph on x.reshape(rows, H); one kernel each way for rows of up to 32 KiB
    (csrc/bvq_row_shifted.hip).  scale and zero_point are x.shape[:-1] + (1,) in x's dtype."""
    return _dynamic_act_quant(True, 'row', bit_width)


def ShiftedUint8DynamicActPerGroupFloat(group_size: int = 32, bit_width: int = 8) -> DynamicActIntQuant:
    """one scale and one integer zero-point per `group_size` consecutive elements of the last dimension: the
    ShiftedUint8WeightPerGroupFloat graph on x.reshape(rows, H); scale and zero_point are
    x.shape[:-1] + (H / group_size, 1)"""
    return _dynamic_act_quant(True, 'group', bit_width, group_size)


# ---- fixed point: power-of-two scales (B/quant/fixed_point.py:23-73, PerTensorPoTScaling8bit B/quant/base.py:185-191)

def _pot():
    return PowerOfTwoRestrictValue(CeilSte())


def Int8WeightPerTensorFixedPoint(weights, bit_width: int = 8) -> RescalingIntQuant:
    """NarrowIntQuant + MaxStatsScaling + PerTensorPoTScaling8bit (B/quant/fixed_point.py:23-34):
    scale = 2^ceil(log2 max|w|) / 2^(b-1); the radix point follows the back-propagated statistic"""
    tracked = _params(weights)
    return RescalingIntQuant(
        IntQuant(narrow_range=True, signed=True, float_to_int_impl=RoundSte(), tensor_clamp_impl=TensorClampSte()),
        StatsFromParameterScaling(AbsMax(), OverTensorView(), 0, tracked, _pot(), (), affine_rescaling=False,
                                  scaling_min_val=SCALING_MIN_VAL),
        PowerOfTwoIntScaling(signed=True), ZeroZeroPoint(), BitWidthConst(bit_width))


def Int8WeightPerChannelFixedPoint(weights, bit_width: int = 8) -> RescalingIntQuant:
    """Int8WeightPerTensorFixedPoint with scaling_per_output_channel=True: one radix point per output channel"""
    tracked = _params(weights)
    w = tracked[0]
    shape = (w.shape[0],) + (1,) * (w.dim() - 1)
    return RescalingIntQuant(
        IntQuant(narrow_range=True, signed=True, float_to_int_impl=RoundSte(), tensor_clamp_impl=TensorClampSte()),
        StatsFromParameterScaling(AbsMax(1), OverOutputChannelView(None), 1, tracked, _pot(), shape,
                                  affine_rescaling=False, scaling_min_val=SCALING_MIN_VAL),
        PowerOfTwoIntScaling(signed=True), ZeroZeroPoint(), BitWidthConst(bit_width))


def _act_fixed_point(signed: bool, collect_stats_steps: int, bit_width: int) -> RescalingIntQuant:
    return RescalingIntQuant(
        IntQuant(narrow_range=False, signed=signed, float_to_int_impl=RoundSte(), tensor_clamp_impl=TensorClamp()),
        ParameterFromRuntimeStatsScaling(collect_stats_steps, AbsPercentile(99.999, None), OverTensorView(), (),
                                         _pot(), 0.1, SCALING_MIN_VAL),
        PowerOfTwoIntScaling(signed=signed), ZeroZeroPoint(), BitWidthConst(bit_width))


def Int8ActPerTensorFixedPoint(collect_stats_steps: int = 300, bit_width: int = 8) -> RescalingIntQuant:
    """IntQuant + ParamFromRuntimePercentileScaling + PerTensorPoTScaling8bit (B/quant/fixed_point.py:37-47):
    log2 of the 99.999th percentile is collected, then learned; the scale is 2^ceil(value) / 2^(b-1)"""
    return _act_fixed_point(True, collect_stats_steps, bit_width)


def Uint8ActPerTensorFixedPoint(collect_stats_steps: int = 300, bit_width: int = 8) -> RescalingIntQuant:
    """unsigned variant (B/quant/fixed_point.py:50-60)"""
    return _act_fixed_point(False, collect_stats_steps, bit_width)


def Uint8ActPerTensorFixedPointMaxInit(max_val: float, bit_width: int = 8) -> RescalingIntQuant:
    """UintQuant + ParamMinMaxInitScaling + PerTensorPoTScaling8bit (B/quant/fixed_point.py:63-76): learned
    radix point initialised from a user-defined max_val"""
    return RescalingIntQuant(
        IntQuant(narrow_range=False, signed=False, float_to_int_impl=RoundSte(), tensor_clamp_impl=TensorClamp()),
        ParameterScaling(max_val, None, _pot(), None),
        PowerOfTwoIntScaling(signed=False), ZeroZeroPoint(), BitWidthConst(bit_width))


# ---- bias quantizers (B/quant/scaled_int.py:64-132, fixed_point.py:79-90) ---------------------------------

def _int_bias(bit_width: int) -> PrescaledRestrictIntQuant:
    return PrescaledRestrictIntQuant(
        IntQuant(narrow_range=False, signed=True, float_to_int_impl=RoundSte(), tensor_clamp_impl=TensorClamp()),
        BitWidthConst(bit_width))


def Int8Bias() -> PrescaledRestrictIntQuant:
    """IntBias with bit_width = 8 (B/quant/scaled_int.py:78-88): `q(bias, scale)` with the scale of the
    accumulator the bias is added to, typically quant_input_scale * quant_weight_scale (one per output channel)"""
    return _int_bias(8)


def Int16Bias() -> PrescaledRestrictIntQuant:
    return _int_bias(16)


def Int24Bias() -> PrescaledRestrictIntQuant:
    return _int_bias(24)


def Int32Bias() -> PrescaledRestrictIntQuant:
    return _int_bias(32)


def Int8BiasPerTensorFloatInternalScaling(bias: torch.nn.Parameter, bit_width: int = 8) -> RescalingIntQuant:
    """IntQuant + MaxStatsScaling + PerTensorFloatScaling8bit + BiasQuantSolver (B/quant/scaled_int.py:135-141):
    the bias quantized with a scale of its own, from its abs-max (requires no input scale)"""
    return RescalingIntQuant(
        IntQuant(narrow_range=False, signed=True, float_to_int_impl=RoundSte(), tensor_clamp_impl=TensorClamp()),
        StatsFromParameterScaling(AbsMax(), OverTensorView(), 0, [bias], FloatRestrictValue(), (),
                                  affine_rescaling=False, scaling_min_val=SCALING_MIN_VAL),
        IntScaling(signed=True, narrow_range=False), ZeroZeroPoint(), BitWidthConst(bit_width))


def Int8BiasPerTensorFixedPointInternalScaling(bias: torch.nn.Parameter, bit_width: int = 8) -> RescalingIntQuant:
    """IntQuant + MaxStatsScaling + PerTensorPoTScaling8bit + BiasQuantSolver (B/quant/fixed_point.py:79-90)"""
    return RescalingIntQuant(
        IntQuant(narrow_range=False, signed=True, float_to_int_impl=RoundSte(), tensor_clamp_impl=TensorClamp()),
        StatsFromParameterScaling(AbsMax(), OverTensorView(), 0, [bias], _pot(), (), affine_rescaling=False,
                                  scaling_min_val=SCALING_MIN_VAL),
        PowerOfTwoIntScaling(signed=True), ZeroZeroPoint(), BitWidthConst(bit_width))
