"""Generate tests/golden/act_layers.npz by RUNNING THE REFERENCE on CPU: the resolved graphs of the activation layers'
default quantizers (QuantReLU / QuantSigmoid: Uint8ActPerTensorFloat, QuantTanh: Int8ActPerTensorFloat, QuantHardTanh:
Int8ActPerTensorFloatMinMaxInit, and Uint8ActPerTensorFloatMaxInit) applied to act(x), as the reference's
FusedActivationQuantProxy does (B/proxy/runtime_quant.py:73-84, 102-164; a quantized HardTanh is dropped), in training
mode through the collection phase into the learned one.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_act.py

Imports the reference the way tests/golden/make_golden.py does (a namespace stub for brevitas.inject; the named
quantizers are assembled by hand as B/quant/scaled_int.py:32-62,170-193, B/quant/solver/act.py:17-23,64-89 resolve
them).  Per case and step: x, the incoming gradient g, y, scale, dx, and the gradient of the scale parameter once there
is one.  bf16 / f16 stored as uint16 bit patterns; inputs from torch.manual_seed(123456).
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
from brevitas.core.function_wrapper import OverTensorView, RoundSte, TensorClamp  # noqa: E402
from brevitas.core.quant import IntQuant, RescalingIntQuant  # noqa: E402
from brevitas.core.restrict_val import FloatRestrictValue  # noqa: E402
from brevitas.core.scaling import IntScaling, ParameterFromRuntimeStatsScaling, ParameterScaling  # noqa: E402
from brevitas.core.stats import AbsPercentile  # noqa: E402
from brevitas.core.zero_point import ZeroZeroPoint  # noqa: E402

DT = {'f32': torch.float32, 'bf16': torch.bfloat16, 'f16': torch.float16}
COLLECT = 2  # collect_stats_steps of the collect-then-learn quantizers: steps 0, 1 collect, 2 hands over, 3.. learn
STEPS = 5


def enc(t):
    t = t.detach().contiguous()
    if t.dtype in (torch.bfloat16, torch.float16):
        return t.view(torch.int16).numpy().view(np.uint16).copy()
    return t.numpy().copy()


def _int_quant(signed):
    return IntQuant(narrow_range=False, signed=signed, float_to_int_impl=RoundSte(), tensor_clamp_impl=TensorClamp())


def from_stats(signed):
    """Uint8ActPerTensorFloat / Int8ActPerTensorFloat (B/quant/scaled_int.py:170-193, base.py:68-75)"""
    return RescalingIntQuant(
        _int_quant(signed),
        ParameterFromRuntimeStatsScaling(COLLECT, AbsPercentile(99.999, None), OverTensorView(), (),
                                         FloatRestrictValue(), 0.1, 1e-10),
        IntScaling(signed=signed, narrow_range=False), ZeroZeroPoint(), BitWidthConst(8))


def min_max_init(signed, min_val, max_val):
    """Int8ActPerTensorFloatMinMaxInit / Uint8ActPerTensorFloatMaxInit: ParameterScaling initialised by
    MinMaxScalingInit (a float32 scalar max(|min_val|, |max_val|)), no scaling_min_val"""
    init = torch.tensor(max(abs(float(min_val)), abs(float(max_val))))
    return RescalingIntQuant(_int_quant(signed), ParameterScaling(init, None, FloatRestrictValue(), None),
                             IntScaling(signed=signed, narrow_range=False), ZeroZeroPoint(), BitWidthConst(8))


# layer, activation the proxy applies (HardTanh dropped under a quantizer), quantizer factory, its meta
LAYERS = [
    ('QuantReLU', torch.relu, lambda: from_stats(False), {}),
    ('QuantSigmoid', torch.sigmoid, lambda: from_stats(False), {}),
    ('QuantTanh', torch.tanh, lambda: from_stats(True), {}),
    ('QuantHardTanh', lambda t: t, lambda: min_max_init(True, -0.5, 0.8), {'min_val': -0.5, 'max_val': 0.8}),
    ('QuantSigmoid', torch.sigmoid, lambda: min_max_init(False, 0.0, 1.0), {'act_quant': 'Uint8ActPerTensorFloatMaxInit',
                                                                           'max_val': 1.0}),
]


def special(x):
    flat = x.view(-1)
    vals = [0.0, -0.0, float('inf'), float('-inf'), 40.0, -40.0, 1e-30, -1e-30, 0.49, -0.51]
    for i, v in enumerate(vals):
        flat[7 * i + 3] = v
    return x


def main():
    torch.manual_seed(123456)
    meta, arrays = [], {}
    for layer, act, qf, extra in LAYERS:
        for dn, dt in DT.items():
            q = qf().to(dt)
            idx = len(meta)
            for step in range(STEPS):
                x = special((torch.randn(2, 3, 7, 5) * 3).to(dt)).requires_grad_(True)
                g = torch.randn(2, 3, 7, 5).to(dt)
                y, scale, _, _ = q(act(x))
                y.backward(g)
                p = q.scaling_impl.value if hasattr(q.scaling_impl, 'value') else None
                for name, t in (('x', x), ('g', g), ('y', y), ('scale', scale), ('dx', x.grad)):
                    arrays['c%d_s%d_%s' % (idx, step, name)] = enc(t)
                if p is not None and p.grad is not None:
                    arrays['c%d_s%d_dvalue' % (idx, step)] = enc(p.grad)
                    p.grad = None
            meta.append(dict(layer=layer, dtype=dn, steps=STEPS, collect_stats_steps=COLLECT, **extra))
    path = os.path.join(HERE, 'act_layers.npz')
    np.savez_compressed(path, __meta__=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), **arrays)
    print(path, len(meta), 'cases')


if __name__ == '__main__':
    main()
