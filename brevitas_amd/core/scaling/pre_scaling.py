"""Pre-scaling parameters of the weight-normalised quantizers (ParameterPreScalingWeightNorm and
AccumulatorAwareParameterPreScaling of later Brevitas releases; not in the reference snapshot): the learned per-channel
`g` of  w = g * v / norm(v).  WeightNormIntQuant (core/quant/int.py) owns one as `pre_scaling_impl`, so the state-dict
key is `pre_scaling_impl.value`."""
import math
from typing import Optional

import torch
from torch import Tensor
from torch.nn import Parameter

from brevitas_amd.core._state import TolerantLoad
from brevitas_amd.core.restrict_val import _RestrictClampValue
from brevitas_amd.function.ops_ste import abs_binary_sign_grad

PRE_SCALING_MIN_VAL = 1e-10
NORM_KINDS = ('l1', 'l2')


def channel_norms(weight: Tensor, norm: str) -> Tensor:
    """float32 L1 / L2 norm of every output channel (dim 0) of `weight`, shaped (out, 1, ..., 1)"""
    if norm not in NORM_KINDS:
        raise ValueError("norm must be 'l1' or 'l2', got %r" % (norm,))
    v = weight.detach().reshape(weight.shape[0], -1).float()
    n = v.abs().sum(1) if norm == 'l1' else torch.sqrt((v * v).sum(1))
    return n.reshape((weight.shape[0],) + (1,) * (weight.dim() - 1))


class ParameterPreScalingWeightNorm(TolerantLoad, torch.nn.Module):
    """g = |clamp_min(value, pre_scaling_min_val)|, one per output channel, restricted like ParameterScaling.  `value`
    starts at the channel norms of the tracked weight, so that g / norm(v) = 1 and the quantizer reproduces v to
    within one code step at step 0."""

    bvq_float_checkpoint_ok = ('value',)

    def __init__(self, tracked_weight: Tensor, norm: str = 'l2', pre_scaling_min_val: float = PRE_SCALING_MIN_VAL,
                 pre_scaling_init: Optional[Tensor] = None) -> None:
        super().__init__()
        self.norm = norm
        init = channel_norms(tracked_weight, norm) if pre_scaling_init is None else pre_scaling_init.detach().clone()
        self.value = Parameter(init.to(tracked_weight.device))
        self.restrict_clamp_scaling = _RestrictClampValue(pre_scaling_min_val, None)

    def upper_bound(self) -> float:
        """T, the largest g / s the quantizer lets through: none here"""
        return math.inf

    def forward(self, placeholder: Tensor) -> Tensor:
        return abs_binary_sign_grad(self.restrict_clamp_scaling(self.value))

    def bvq_learned_scale(self):
        """(value, min_val): g is exactly |clamp_min_ste(value, min_val)|, like ParameterScaling.bvq_learned_scale"""
        return self.value, getattr(self.restrict_clamp_scaling.clamp_min_ste, 'min_val', None)


class AccumulatorAwareParameterPreScaling(ParameterPreScalingWeightNorm):
    """ParameterPreScalingWeightNorm over the L1 norm whose g the quantizer caps at T * s, with
    T = (2^(P-1) - 1) * 2^(sigma - N) for a P-bit accumulator and N-bit inputs (sigma = 1 for signed inputs): the
    integer weights of every output channel then satisfy sum |q| <= T, and a dot product with such inputs cannot
    overflow the accumulator (A2Q, Colbert et al. 2023)."""

    def __init__(self, tracked_weight: Tensor, accumulator_bit_width: int = 32, input_bit_width: int = 8,
                 input_signed: bool = False, pre_scaling_min_val: float = PRE_SCALING_MIN_VAL,
                 pre_scaling_init: Optional[Tensor] = None) -> None:
        super().__init__(tracked_weight, 'l1', pre_scaling_min_val, pre_scaling_init)
        if int(accumulator_bit_width) < 2 or int(input_bit_width) < 1:
            raise ValueError('accumulator_bit_width >= 2 and input_bit_width >= 1, got %r and %r'
                             % (accumulator_bit_width, input_bit_width))
        self.accumulator_bit_width = int(accumulator_bit_width)
        self.input_bit_width = int(input_bit_width)
        self.input_signed = bool(input_signed)

    def upper_bound(self) -> float:
        """T as the float32 the quantizer computes with: the formula's value, rounded toward zero where float32 does not
        hold it (P > 25), so that rounding never loosens the bound"""
        key = (self.accumulator_bit_width, self.input_bit_width, self.input_signed)
        cached = self.__dict__.get('_bvq_bound')
        if cached is None or cached[0] != key:
            sigma = 1 if self.input_signed else 0
            exact = float(2 ** (self.accumulator_bit_width - 1) - 1) * 2.0 ** (sigma - self.input_bit_width)
            t = torch.tensor(exact, dtype=torch.float32)
            if float(t) > exact:
                t = torch.nextafter(t, torch.tensor(0.0))
            cached = self.__dict__['_bvq_bound'] = (key, float(t))
        return cached[1]
