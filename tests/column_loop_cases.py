"""What tests/test_gpu_gptq.py and tests/test_gpu_gpfq.py share: the bit comparison of two tensors and the small models
their mode tests calibrate (each with its round-to-nearest copy, the float model and correlated inputs)."""
import copy
import functools

import torch

from brevitas_amd import quant as Q
from brevitas_amd.nn import QuantConv2d, QuantLinear, QuantReLU


def _same_bits(a, b, what):
    if a is None:
        assert b is None
        return
    assert a.dtype == b.dtype and a.shape == b.shape, what
    ai = a.contiguous().view(torch.int32 if a.element_size() == 4 else torch.int16)
    bi = b.contiguous().view(torch.int32 if b.element_size() == 4 else torch.int16)
    bad = (ai != bi) & ~(a.isnan() & b.isnan())
    assert not bad.any(), '%s: %d of %d differ, first at %s' % (what, int(bad.sum()), bad.numel(),
                                                                 bad.nonzero()[0].tolist())


def _float_twin(model, float_model):
    """the float model with the weights and biases of the quantized one's layers"""
    for quant, plain in zip(model, float_model):
        if hasattr(plain, 'weight'):
            plain.load_state_dict({k: v for k, v in quant.state_dict().items() if k in ('weight', 'bias')})
    return float_model


def linear_models(dev):
    """QuantLinear -> QuantReLU -> QuantLinear (4-bit, groups of 32, the second asymmetric), its round-to-nearest copy,
    the float model and correlated inputs"""
    torch.manual_seed(5)
    model = torch.nn.Sequential(
        QuantLinear(64, 96, weight_quant=functools.partial(Q.Int4WeightPerGroupFloat, group_size=32)),
        QuantReLU(Q.Uint8ActPerTensorFloat(scaling_impl_type='stats', scaling_stats_op='max')),
        QuantLinear(96, 32, weight_quant=functools.partial(Q.ShiftedUint4WeightPerGroupFloat, group_size=32))).to(dev)
    rtn = copy.deepcopy(model)
    float_model = torch.nn.Sequential(torch.nn.Linear(64, 96), torch.nn.ReLU(), torch.nn.Linear(96, 32)).to(dev)
    gen = torch.Generator().manual_seed(6)
    x = (torch.randn(512, 64, generator=gen) @ (torch.eye(64) + 2 * torch.randn(64, 64, generator=gen) / 8.0)).to(dev)
    return model, rtn, _float_twin(model, float_model), x


def conv_models(dev):
    """a QuantConv2d 3x3 (4-bit, groups of 16), its round-to-nearest copy, the float layer and correlated inputs"""
    torch.manual_seed(7)
    model = torch.nn.Sequential(
        QuantConv2d(16, 16, 3, padding=1, weight_quant=functools.partial(Q.Int4WeightPerGroupFloat, group_size=16))).to(dev)
    rtn = copy.deepcopy(model)
    float_model = torch.nn.Sequential(torch.nn.Conv2d(16, 16, 3, padding=1)).to(dev)
    gen = torch.Generator().manual_seed(8)
    x = torch.randn(4, 16, 12, 12, generator=gen)
    x = (x + 0.8 * x.roll(1, dims=1) + 0.5 * x.roll(1, dims=3)).to(dev)  # correlated inputs
    return model, rtn, _float_twin(model, float_model), x
