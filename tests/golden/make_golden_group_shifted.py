"""Generate tests/golden/group_shifted.npz by RUNNING THE REFERENCE on CPU: the asymmetric group-wise weight quantizer is,
by definition, the reference's resolved ShiftedUint8WeightPerChannelFloat graph (ShiftedMinUintQuant + MinMaxStatsScaling
+ PerChannelFloatScaling, B/quant/shifted_scaled_int.py:55-70, B/quant/base.py:60-65,137-150) applied to the weight
regrouped as [out * K / g, g], K = numel / out, groups being g consecutive elements in memory order.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_group_shifted.py

Imports the reference the way tests/golden/make_golden_group.py does.  Per case: x (the weight, in its own shape), the
incoming gradient g, y, scale and zp [out, K / g, 1] and dx.  float32 and bfloat16 only, float16 is checked on the device
only (the reason is in make_golden_group.py).  bf16 stored as uint16 bit patterns; inputs from torch.manual_seed(654321).

Planted in every case, in the case's dtype so that the ties are exact (PLANTED names the groups):
  zero       all zero (the lower bound of the scale, zero-point 0);
  constant   a constant non-zero value (max == min: both statistics on element 0, the lower bound of the scale);
  positive   positive values only (zero-point 0, the upper part clips);
  negative   negative values only (zero-point 2^b - 1, clips likewise);
  min_far    the minimum at elements 2 and g - 3, in different 16-byte chunks;   min_near   at 5 and 6, inside one chunk;
  max_far    the maximum at elements 1 and g - 2;                                max_near   at 4 and 5;
  ends       the maximum at the group's first element and the minimum at its last;
  zeros      both -0.0 and +0.0 (-0.0 first) and negative values: the maximum is zero.
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
from brevitas.core.stats import AbsMinMax, NegativeMinOrZero  # noqa: E402
from brevitas.core.zero_point import StatsFromParameterZeroPoint  # noqa: E402

DT = {'f32': torch.float32, 'bf16': torch.bfloat16}
# (weight shape, group size, bit width): out x K = 24x256, 6x384, 5x512, 16x64 and 8x144 (a conv weight)
CASES = [((24, 256), 32, 4), ((6, 384), 128, 8), ((5, 512), 256, 4), ((16, 64), 64, 8), ((8, 16, 3, 3), 16, 4)]
PLANTED = dict(zero=0, constant=1, positive=2, negative=3, min_far=4, min_near=5, max_far=6, max_near=7, ends=8, zeros=9)


def enc(t):
    t = t.detach().contiguous()
    if t.dtype in (torch.bfloat16, torch.float16):
        return t.view(torch.int16).numpy().view(np.uint16).copy()
    return t.numpy().copy()


def shifted_per_channel_weight_quant(weight, bit_width):
    shape = (weight.shape[0], 1)
    int_quant = IntQuant(narrow_range=False, signed=False, float_to_int_impl=RoundSte(),
                         tensor_clamp_impl=TensorClampSte())
    return RescalingIntQuant(
        int_quant,
        StatsFromParameterScaling(AbsMinMax(1), OverOutputChannelView(None), 1, [weight], FloatRestrictValue(), shape,
                                  affine_rescaling=False, scaling_min_val=1e-10),
        IntScaling(signed=False, narrow_range=False),
        StatsFromParameterZeroPoint(int_quant, True, OverOutputChannelView(None), 1, NegativeMinOrZero(1), shape,
                                    [weight]),
        BitWidthConst(bit_width))


def plant(w2):
    """w2: the weight as [groups, g] in its dtype, modified in place"""
    g = w2.shape[1]
    P = PLANTED
    w2[P['zero']] = 0.0
    w2[P['constant']] = 0.015625
    w2[P['positive']] = w2[P['positive']].abs() + 0.01
    w2[P['negative']] = -(w2[P['negative']].abs()) - 0.01
    for grp, sign, (first, second) in ((P['min_far'], -1, (2, g - 3)), (P['min_near'], -1, (5, 6)),
                                       (P['max_far'], 1, (1, g - 2)), (P['max_near'], 1, (4, 5))):
        m = (w2[grp].abs().max().float() * 1.25).to(w2.dtype) * sign
        w2[grp, first] = m
        w2[grp, second] = m
    m = (w2[P['ends']].abs().max().float() * 1.5).to(w2.dtype)
    w2[P['ends'], 0] = m
    w2[P['ends'], g - 1] = -m
    w2[P['zeros']] = -(w2[P['zeros']].abs()) - 0.001
    w2[P['zeros'], 3] = -0.0
    w2[P['zeros'], g - 4] = 0.0


def main():
    torch.manual_seed(654321)
    meta, arrays = [], {}
    for shape, g, bits in CASES:
        for dn, dt in DT.items():
            w = (torch.randn(shape) * 0.02).to(dt)
            plant(w.view(-1, g))
            out, k = shape[0], w.numel() // shape[0]
            w2 = torch.nn.Parameter(w.view(-1, g).clone())
            q = shifted_per_channel_weight_quant(w2, bits)
            y, scale, zp, _ = q(w2)
            grad = torch.randn(shape).to(dt)
            y.backward(grad.view(-1, g))
            assert bool(torch.isfinite(w2.grad.float()).all()) and bool(torch.isfinite(y.float()).all())
            assert zp.dtype == dt and scale.dtype == dt and tuple(zp.shape) == (w2.shape[0], 1)
            idx = len(meta)
            for name, t in (('x', w), ('g', grad), ('y', y.view(shape)), ('scale', scale.view(out, k // g, 1)),
                            ('zp', zp.view(out, k // g, 1)), ('dx', w2.grad.view(shape))):
                arrays['c%d_%s' % (idx, name)] = enc(t)
            meta.append(dict(shape=list(shape), group_size=g, bit_width=bits, dtype=dn, planted=PLANTED,
                             dtypes={n: dn for n in ('x', 'g', 'y', 'scale', 'zp', 'dx')}))
    path = os.path.join(HERE, 'group_shifted.npz')
    np.savez_compressed(path, __meta__=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), **arrays)
    print('%s: %d cases, %.1f KB' % (path, len(meta), os.path.getsize(path) / 1024))


if __name__ == '__main__':
    main()
