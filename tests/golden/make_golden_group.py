"""Generate tests/golden/group_quant.npz by RUNNING THE REFERENCE on CPU: the group-wise weight quantizer is, by
definition, the reference's per-output-channel weight graph (Int8WeightPerChannelFloat resolved: NarrowIntQuant +
MaxStatsScaling + PerChannelFloatScaling, B/quant/scaled_int.py:157-167) applied to the weight regrouped as
[out * K / g, g], K = numel / out, groups being g consecutive elements in memory order.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_group.py

Imports the reference the way tests/golden/make_golden.py does (a namespace stub for brevitas.inject; the graph is
assembled by hand).  Per case: x (the weight, in its own shape), the incoming gradient g, y, scale [out, K / g, 1] and
dx.  float32 and bfloat16: the reference runs float16 on the CPU too, but scaling_min_val = 1e-10 underflows there and an
all-zero group yields NaN gradients, so float16 is checked on the device only.  bf16 stored as uint16 bit patterns;
inputs from torch.manual_seed(123456).

Planted in every case, in the case's dtype so that the ties are exact:
  group 1: all zero (the lower bound of the scale);
  group 2: -max at element 2 and +max at element g - 3, in different 16-byte chunks (the first must win);
  group 3: -max at element 5 and +max at element 6, inside one 16-byte chunk in both dtypes;
  group 4: the maximum is the group's last element.
"""
import json
import os
import sys
import types

REF = '/root/reference/src'
HERE = os.path.dirname(os.path.abspath(__file__))

stub = types.ModuleType('brevitas.inject')
stub.__path__ = [os.path.join(REF, 'brevitas', 'inject')]
sys.modules['brevitas.inject'] = stub
sys.path.insert(0, REF)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from brevitas.core.bit_width import BitWidthConst  # noqa: E402
from brevitas.core.function_wrapper import OverOutputChannelView, RoundSte, TensorClampSte  # noqa: E402
from brevitas.core.quant import IntQuant, RescalingIntQuant  # noqa: E402
from brevitas.core.restrict_val import FloatRestrictValue  # noqa: E402
from brevitas.core.scaling import IntScaling, StatsFromParameterScaling  # noqa: E402
from brevitas.core.stats import AbsMax  # noqa: E402
from brevitas.core.zero_point import ZeroZeroPoint  # noqa: E402

DT = {'f32': torch.float32, 'bf16': torch.bfloat16}
# (weight shape, group size, bit width): out x K = 24x256, 6x384, 5x512, 16x64 and 8x144 (a conv weight)
CASES = [((24, 256), 32, 4), ((6, 384), 128, 8), ((5, 512), 256, 4), ((16, 64), 64, 8), ((8, 16, 3, 3), 16, 4)]
ZERO_GROUP, TIE_FAR_GROUP, TIE_NEAR_GROUP, LAST_GROUP = 1, 2, 3, 4


def enc(t):
    t = t.detach().contiguous()
    if t.dtype in (torch.bfloat16, torch.float16):
        return t.view(torch.int16).numpy().view(np.uint16).copy()
    return t.numpy().copy()


def per_channel_weight_quant(weight, bit_width):
    shape = (weight.shape[0], 1)
    return RescalingIntQuant(
        IntQuant(narrow_range=True, signed=True, float_to_int_impl=RoundSte(), tensor_clamp_impl=TensorClampSte()),
        StatsFromParameterScaling(AbsMax(1), OverOutputChannelView(None), 1, [weight], FloatRestrictValue(), shape,
                                  affine_rescaling=False, scaling_min_val=1e-10),
        IntScaling(signed=True, narrow_range=True), ZeroZeroPoint(), BitWidthConst(bit_width))


def plant(w2):
    """w2: the weight as [groups, g] in its dtype, modified in place"""
    g = w2.shape[1]
    w2[ZERO_GROUP] = 0.0
    for grp, (first, second) in ((TIE_FAR_GROUP, (2, g - 3)), (TIE_NEAR_GROUP, (5, 6))):
        m = (w2[grp].abs().max().float() * 1.25).to(w2.dtype)
        w2[grp, first] = -m
        w2[grp, second] = m
    w2[LAST_GROUP, g - 1] = (w2[LAST_GROUP].abs().max().float() * 1.5).to(w2.dtype)


def main():
    torch.manual_seed(123456)
    meta, arrays = [], {}
    for shape, g, bits in CASES:
        for dn, dt in DT.items():
            w = (torch.randn(shape) * 0.02).to(dt)
            plant(w.view(-1, g))
            out, k = shape[0], w.numel() // shape[0]
            w2 = torch.nn.Parameter(w.view(-1, g).clone())
            q = per_channel_weight_quant(w2, bits)
            y, scale, zp, _ = q(w2)
            grad = torch.randn(shape).to(dt)
            y.backward(grad.view(-1, g))
            assert float(zp) == 0.0 and bool(torch.isfinite(w2.grad.float()).all())
            idx = len(meta)
            for name, t in (('x', w), ('g', grad), ('y', y.view(shape)), ('scale', scale.view(out, k // g, 1)),
                            ('dx', w2.grad.view(shape))):
                arrays['c%d_%s' % (idx, name)] = enc(t)
            meta.append(dict(shape=list(shape), group_size=g, bit_width=bits, dtype=dn,
                             dtypes={n: dn for n in ('x', 'g', 'y', 'scale', 'dx')}))
    path = os.path.join(HERE, 'group_quant.npz')
    np.savez_compressed(path, __meta__=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), **arrays)
    print('%s: %d cases, %.1f KB' % (path, len(meta), os.path.getsize(path) / 1024))


if __name__ == '__main__':
    main()
