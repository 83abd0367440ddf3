"""Generate tests/golden/dynamic_act.npz by RUNNING THE REFERENCE on CPU: a dynamic activation quantizer is, by
definition, an existing resolved weight graph of the reference applied to x2 = x.reshape(rows, H) as the tracked
parameter, with the plain TensorClamp and the full (not narrow) range:

    Int8DynamicActPerTensorFloat          Int8WeightPerTensorFloat          (B/quant/scaled_int.py:144-154)
    Int8DynamicActPerRowFloat             Int8WeightPerChannelFloat         (B/quant/scaled_int.py:157-167)
    Int8DynamicActPerGroupFloat           the per-channel graph on x2 regrouped as [rows * H / g, g]
    ShiftedUint8DynamicActPerTensorFloat  ShiftedUint8WeightPerTensorFloat  (B/quant/shifted_scaled_int.py:37-52)
    ShiftedUint8DynamicActPerRowFloat     ShiftedUint8WeightPerChannelFloat (B/quant/shifted_scaled_int.py:55-70)
    ShiftedUint8DynamicActPerGroupFloat   the shifted per-channel graph on x2 regrouped as [rows * H / g, g]

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_dynamic_act.py

Imports the reference the way tests/golden/make_golden_group_shifted.py does.  12 rows; H in {40, 536, 1032} for the
per-tensor and per-row graphs (none a group size of the kernels; 536 and 1032 leave a ragged last wave load in both
element sizes), H = 1024 with g = 32 for the per-group graphs.  float32 and bfloat16 (float16 is checked on the device
only, the reason is in make_golden_group.py), bit widths 8 and 4.  The per-row and per-group graphs run every
(H, dtype, bit width); the two per-tensor graphs run all four (dtype, bit width) at H = 40 and two of them at each of
H = 536 and 1032, chosen so that every H meets both dtypes and both bit widths (PER_TENSOR_AT).

Twelve rows of a thousand elements in fifty-odd cases are 2 MB of raw results, so the file (under 512 KB) holds them
without loss in fewer bytes.  tests/dynamic_golden.py undoes it; main() checks here that undoing it returns the
reference's bits:
  inputs   once per H, shared by the dtypes, graphs and bit widths: `in_<H>_x` float32, the bfloat16 input being its
           rounding (the rows are planted in float32; rounding keeps every tie, sign and order they are made of), and
           `in_<H>_g`, multiples of 1/8 in [-2, 2] drawn at random, the same values in both dtypes;
  y        as the reference's own integer codes q = int_quant.to_int(scale, zp, bit_width, x) (`c<i>_q`, uint8 for the
           unsigned graphs, int8 for the signed): y is (q - zp) * scale, the last two ops of its forward, in the
           case's dtype, with a -0.0 at the flat positions `c<i>_nz` (an integer code holds no sign of zero);
  dx       as its bit pattern XOR the bit pattern of g (`c<i>_dxg`): the straight-through gradient is g nearly
           everywhere;
  scale, zp  as they are.
x is torch.randn * 0.02 from torch.manual_seed(24680).  bf16 is stored as uint16 bit patterns.

Planted in every input the ten rows of make_golden_group_shifted.py with a row of H elements in a group's place (PLANTED
names the rows; the "far" ties are at elements 2 and H - 3, 1 and H - 2).  The per-group input plants them in its first
ten GROUPS instead.
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
from brevitas.core.function_wrapper import OverOutputChannelView, OverTensorView, RoundSte, TensorClamp  # noqa: E402
from brevitas.core.quant import IntQuant, RescalingIntQuant  # noqa: E402
from brevitas.core.restrict_val import FloatRestrictValue  # noqa: E402
from brevitas.core.scaling import IntScaling, StatsFromParameterScaling  # noqa: E402
from brevitas.core.stats import AbsMax, AbsMinMax, NegativeMinOrZero  # noqa: E402
from brevitas.core.zero_point import StatsFromParameterZeroPoint, ZeroZeroPoint  # noqa: E402

sys.path.insert(0, HERE)
from make_golden_group_shifted import PLANTED, enc, plant  # noqa: E402

DT = {'f32': torch.float32, 'bf16': torch.bfloat16}
ROWS = 12
ROW_H = (40, 536, 1032)
GROUP_H, GROUP_G = 1024, 32
BITS = (8, 4)
# (dtype, bit width) of the per-tensor graphs at each H, symmetric / asymmetric
PER_TENSOR_AT = {40: {False: [('f32', 8), ('f32', 4), ('bf16', 8), ('bf16', 4)],
                      True: [('f32', 8), ('f32', 4), ('bf16', 8), ('bf16', 4)]},
                 536: {False: [('f32', 4), ('bf16', 8)], True: [('f32', 8), ('bf16', 4)]},
                 1032: {False: [('f32', 8), ('bf16', 4)], True: [('f32', 4), ('bf16', 8)]}}
QUANTIZERS = {('tensor', False): 'Int8DynamicActPerTensorFloat', ('row', False): 'Int8DynamicActPerRowFloat',
              ('group', False): 'Int8DynamicActPerGroupFloat',
              ('tensor', True): 'ShiftedUint8DynamicActPerTensorFloat',
              ('row', True): 'ShiftedUint8DynamicActPerRowFloat',
              ('group', True): 'ShiftedUint8DynamicActPerGroupFloat'}


def weight_graph(w2, per_tensor, shifted, bit_width):
    """the resolved weight graph on the tracked [channels, K] parameter w2, TensorClamp, full range"""
    if per_tensor:
        shape, view, dim, cat = (), OverTensorView, None, 0
    else:
        shape, view, dim, cat = (w2.shape[0], 1), (lambda: OverOutputChannelView(None)), 1, 1
    int_quant = IntQuant(narrow_range=False, signed=not shifted, float_to_int_impl=RoundSte(),
                         tensor_clamp_impl=TensorClamp())
    scaling = StatsFromParameterScaling(AbsMinMax(dim) if shifted else AbsMax(dim), view(), cat, [w2],
                                        FloatRestrictValue(), shape, affine_rescaling=False, scaling_min_val=1e-10)
    zero_point = StatsFromParameterZeroPoint(int_quant, True, view(), cat, NegativeMinOrZero(dim), shape, [w2]) \
        if shifted else ZeroZeroPoint()
    return RescalingIntQuant(int_quant, scaling, IntScaling(signed=not shifted, narrow_range=False), zero_point,
                             BitWidthConst(bit_width))


def as_bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def main():
    torch.manual_seed(24680)
    meta, arrays = [], {}
    for h in ROW_H + (GROUP_H,):
        grouped = h == GROUP_H
        g = GROUP_G if grouped else h
        x32 = torch.randn(ROWS, h) * 0.02
        plant(x32.view(-1, g))
        grad32 = torch.randint(-16, 17, (ROWS, h)).float() / 8
        key = 'in_%d' % h
        arrays[key + '_x'], arrays[key + '_g'] = enc(x32), enc(grad32)
        for granularity in (('group',) if grouped else ('tensor', 'row')):
            for shifted in (False, True):
                if granularity == 'tensor':
                    combos = PER_TENSOR_AT[h][shifted]
                else:
                    combos = [(dn, bits) for dn in DT for bits in BITS]
                for dn, bits in combos:
                    dt = DT[dn]
                    x, grad = x32.to(dt), grad32.to(dt)
                    assert torch.equal(grad.float(), grad32)
                    w2 = torch.nn.Parameter(x.view(-1, g).clone())
                    quant = weight_graph(w2, granularity == 'tensor', shifted, bits)
                    y, scale, zp, bw = quant(w2)
                    y.backward(grad.view(-1, g))
                    dx = w2.grad
                    assert bool(torch.isfinite(dx.float()).all()) and bool(torch.isfinite(y.float()).all())
                    with torch.no_grad():
                        q = quant.int_quant.to_int(scale, zp, bw, w2)
                    codes = q.to(torch.uint8 if shifted else torch.int8)
                    assert torch.equal(codes.to(dt), q)
                    # what tests/dynamic_golden.py does with the stored forms returns the reference's bits
                    back = (codes.to(dt) - zp) * scale
                    neg_zero = torch.nonzero((y.reshape(-1) == 0) & torch.signbit(y.reshape(-1))).reshape(-1)
                    back.view(-1)[neg_zero] = -0.0
                    assert back.dtype == y.dtype and np.array_equal(as_bits(enc(back)), as_bits(enc(y)))
                    if granularity == 'tensor':
                        sshape = ()
                    elif granularity == 'row':
                        sshape = (ROWS, 1)
                    else:
                        sshape = (ROWS, h // g, 1)
                    zshape = sshape if shifted else ()
                    idx = len(meta)
                    arrays['c%d_q' % idx] = codes.view(ROWS, h).numpy().copy()
                    arrays['c%d_nz' % idx] = neg_zero.to(torch.int32).numpy().copy()
                    arrays['c%d_scale' % idx] = enc(scale.view(sshape))
                    arrays['c%d_zp' % idx] = enc(zp.view(zshape))
                    arrays['c%d_dxg' % idx] = as_bits(enc(dx.view(ROWS, h))) ^ as_bits(enc(grad))
                    sdn = 'f32' if scale.dtype == torch.float32 else dn
                    zdn = 'f32' if zp.dtype == torch.float32 else dn
                    meta.append(dict(quantizer=QUANTIZERS[(granularity, shifted)], granularity=granularity,
                                     shifted=shifted, shape=[ROWS, h], group_size=g if grouped else None,
                                     bit_width=bits, dtype=dn, inputs=key, planted=PLANTED,
                                     dtypes=dict(x=dn, g=dn, y=dn, dx=dn, scale=sdn, zp=zdn)))
    path = os.path.join(HERE, 'dynamic_act.npz')
    np.savez_compressed(path, __meta__=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), **arrays)
    print('%s: %d cases, %.1f KB' % (path, len(meta), os.path.getsize(path) / 1024))
    assert os.path.getsize(path) < 512 * 1024


if __name__ == '__main__':
    main()
