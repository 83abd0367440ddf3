"""Learned rounding (AdaRound, Nagel et al. 2020; `LearnedRoundSte` of later Brevitas releases, no counterpart in the
reference snapshot): a float_to_int_impl that rounds down and adds a trainable offset h(value) in [0, 1] per element.

    floor_ste(t) + h(value)                     training: h soft, differentiable in `value`
    floor_ste(t) + (h(value) > 1/2)             eval: 0 or 1

Names, constructor arguments and semantics follow later Brevitas.  DESIGN.md §9, "Learned rounding", and include/bvq.h
state the op sequence; IntQuant recognises `bvq_learned_round` and runs the whole quantizer as one HIP kernel each way
where that kernel applies (core/quant/_fused.py, LearnedRoundFakeQuantFn), else it calls this module as a function.
"""
import torch
from torch import Tensor
from torch.nn import Module, Parameter

from brevitas_amd import _native as nat
from brevitas_amd.function.ops_ste import floor_ste

__all__ = ['LearnedRoundHardSigmoid', 'LearnedRoundSigmoid', 'LearnedRoundSte', 'learned_round_init']

# learned_round_init(LearnedRoundSigmoid): the fractional part is kept this far from 0 and 1, so that the logit is finite
# (|value| <= temperature * log(2^20) ~ 13.9 * temperature) and sigmoid(value / temperature) is still off 0 and 1 in
# float32, bfloat16 and float16
SIGMOID_INIT_MARGIN = 2.0 ** -20


_F16_AGREE = {}


def f16_products_agree(scalar32: float) -> bool:
    """float16 tensor * host scalar is the same bits whichever way torch's device kernel rounds it.  Its vectorised body
    rounds the float32 product to float16, its tail path rounds the exact product once (a mixed-precision fma); they can
    differ only where the float32 product is inexact and lands on a float16 tie.  True if that happens for no finite
    float16 factor (checked once per scalar, on the host): float(1.2) and powers of two agree, float(1.4) does not for
    every tenth sigmoid value."""
    ok = _F16_AGREE.get(scalar32)
    if ok is None:
        a = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(torch.float16)
        a = a[torch.isfinite(a)].double()
        b = torch.tensor(scalar32, dtype=torch.float32).double()
        exact = a * b                                   # 11 x 24 significant bits: exact in float64
        p = exact.float().double()                      # the float32 product
        mag = p.abs()
        live = (mag > 0) & (mag < 65504.0) & (p != exact)
        _, exp = torch.frexp(mag)                       # mag = m * 2^exp, m in [0.5, 1)
        grid = torch.clamp(exp - 1, min=-14) - 10       # log2 of the float16 spacing at mag
        q = torch.ldexp(mag, 1 - grid)                  # mag in half spacings: a tie is an odd integer
        tie = (q == torch.floor(q)) & (torch.remainder(q, 2.0) == 1.0)
        ok = _F16_AGREE[scalar32] = not bool((live & tie).any())
    return ok


def _f32(v: float) -> float:
    return torch.tensor(v, dtype=torch.float32).item()


class LearnedRoundHardSigmoid(Module):
    """h(p) = clamp(sigmoid(p) * (zeta - gamma) + gamma, 0, 1): the rectified sigmoid of AdaRound, which reaches 0 and 1
    at finite p; eval: h(p) > 0.5"""
    bvq_learned_round_kind = nat.LR_HARD_SIGMOID

    def __init__(self, learned_round_zeta: float = 1.1, learned_round_gamma: float = -0.1) -> None:
        super().__init__()
        self.learned_round_zeta = float(learned_round_zeta)
        self.learned_round_gamma = float(learned_round_gamma)

    def bvq_constants(self):
        """(c0, c1) of include/bvq.h: the two Python floats the forward's mul and add take"""
        return self.learned_round_zeta - self.learned_round_gamma, self.learned_round_gamma

    def bvq_f16_ok(self) -> bool:
        """the fused kernels hold torch's float16 bits for this impl: the products with zeta - gamma do not depend on
        which of its two roundings torch's kernel takes (f16_products_agree)"""
        return f16_products_agree(_f32(self.learned_round_zeta - self.learned_round_gamma))

    def forward(self, p: Tensor, training: bool) -> Tensor:
        p = torch.sigmoid(p)
        p = p * (self.learned_round_zeta - self.learned_round_gamma)
        p = p + self.learned_round_gamma
        p = torch.clamp(p, 0.0, 1.0)
        if not training:
            return p > 0.5
        return p


class LearnedRoundSigmoid(Module):
    """h(p) = sigmoid(p / temperature); eval: p > 0"""
    bvq_learned_round_kind = nat.LR_SIGMOID

    def __init__(self, learned_round_temperature: float = 1.0) -> None:
        super().__init__()
        if not float(learned_round_temperature) > 0.0:
            raise ValueError('learned_round_temperature must be positive, got %r' % (learned_round_temperature,))
        self.learned_round_temperature = float(learned_round_temperature)

    def bvq_constants(self):
        return self.learned_round_temperature, 0.0

    def bvq_f16_ok(self) -> bool:
        """float16 stays composed: the backward's `/ temperature` is a product whose -0 results (a saturated sigmoid
        under a negative gradient) torch's kernel returns as -0 from its vectorised body and as +0 from its tail path"""
        return False

    def forward(self, p: Tensor, training: bool) -> Tensor:
        if not training:
            return p > 0
        return torch.sigmoid(p / self.learned_round_temperature)


class LearnedRoundSte(Module):
    """float_to_int_impl with one trainable offset per element: forward(x) = floor_ste(x) + impl(value, training).
    `value` (state-dict key `...float_to_int_impl.value`) is viewed as x.shape when only the shapes differ -- the generic
    group-wise route hands IntQuant the weight regrouped as [rows * groups, group size].  No `bvq_round_mode`: the
    recognised statistic graphs decline, the scale comes from their generic route, and IntQuant takes the learned-round
    kernels through `bvq_learned_round`."""

    def __init__(self, learned_round_impl: Module, learned_round_init: Tensor, device=None, dtype=None) -> None:
        super().__init__()
        self.learned_round_impl = learned_round_impl
        init = learned_round_init.detach().clone()
        if device is not None or dtype is not None:
            init = init.to(device=device, dtype=dtype)
        self.value = Parameter(init)

    def bvq_learned_round(self):
        """(impl kind, (c0, c1), value) for the fused kernels, or None for an impl they do not know"""
        impl = self.learned_round_impl
        if type(impl) not in (LearnedRoundHardSigmoid, LearnedRoundSigmoid):
            return None
        return impl.bvq_learned_round_kind, impl.bvq_constants(), self.value

    def _value_like(self, x: Tensor) -> Tensor:
        v = self.value
        if v.shape != x.shape:
            if v.numel() != x.numel():
                raise ValueError('LearnedRoundSte: value of shape %s cannot round a tensor of shape %s'
                                 % (tuple(v.shape), tuple(x.shape)))
            v = v.view(x.shape)
        return v

    def forward(self, x: Tensor) -> Tensor:
        p = self.learned_round_impl(self._value_like(x), self.training)
        return floor_ste(x) + p.to(x.dtype)


def learned_round_init(impl: Module, t: Tensor) -> Tensor:
    """The `value` at which h reproduces t = x / scale + zero_point: with rest = t - floor(t),
      LearnedRoundHardSigmoid   -log((zeta - gamma) / (rest - gamma) - 1), finite for every rest in [0, 1)
      LearnedRoundSigmoid       temperature * (log(rest) - log1p(-rest)), rest clamped to [m, 1 - m], m = 2^-20
                                (SIGMOID_INIT_MARGIN)
    computed in float32 and returned in t's dtype.  The soft output then is t, up to rounding, and the hard output is
    round-to-nearest, except that an exact tie goes down."""
    tf = t.detach().float()
    rest = tf - torch.floor(tf)
    if isinstance(impl, LearnedRoundHardSigmoid):
        zeta, gamma = impl.learned_round_zeta, impl.learned_round_gamma
        v = -torch.log((zeta - gamma) / (rest - gamma) - 1.0)
    elif isinstance(impl, LearnedRoundSigmoid):
        rest = rest.clamp(SIGMOID_INIT_MARGIN, 1.0 - SIGMOID_INIT_MARGIN)
        v = impl.learned_round_temperature * (torch.log(rest) - torch.log1p(-rest))
    else:
        raise TypeError('learned_round_init: %s is not a learned-round impl' % type(impl).__name__)
    return v.to(t.dtype)
