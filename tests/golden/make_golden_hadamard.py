"""Generate tests/golden/hadamard_classifier.npz by RUNNING THE REFERENCE's HadamardClassifier on the CPU.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_hadamard.py

Runs only in the build container: it imports brevitas.nn.hadamard_classifier from /root/reference/src (read-only) the
way make_golden.py imports the core: `brevitas.inject` needs the third-party `dependencies` package, which is not
installed, so a stub stands in for it -- here one that answers every name with an empty placeholder class, since the
layer's mixin imports injector names it never uses without a quantizer.  `brevitas.nn` and `brevitas.nn.mixin` are bare
namespace stubs, so that their __init__ files do not pull in every other layer.  The layer needs scipy (its dense matrix).
No reference file is modified or copied.

What is committed is the resulting .npz: for each (in, out) the input, the scale, the output, and the gradients of the
input and of scale for a stored output gradient, all float32, from torch.manual_seed(123456).
"""
import os
import sys
import types

REF = '/root/reference/src'
HERE = os.path.dirname(os.path.abspath(__file__))


class _Placeholders(types.ModuleType):

    def __getattr__(self, name):
        if name.startswith('__'):
            raise AttributeError(name)
        return type(name, (), {})


for _name in ('brevitas.inject', 'brevitas.nn', 'brevitas.nn.mixin'):
    _stub = (_Placeholders if _name == 'brevitas.inject' else types.ModuleType)(_name)
    _stub.__path__ = [os.path.join(REF, *_name.split('.'))]
    sys.modules[_name] = _stub
sys.path.insert(0, REF)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from brevitas.nn.hadamard_classifier import HadamardClassifier  # noqa: E402

CASES = ((24, 10), (64, 64), (10, 40))
BATCH = 6


def main():
    torch.manual_seed(123456)
    arrays = {}
    for i, (cin, cout) in enumerate(CASES):
        layer = HadamardClassifier(cin, cout)
        with torch.no_grad():
            layer.scale.mul_(1.0 + 0.25 * (i + 1))  # not the initial value: a loaded one
        x = torch.randn(BATCH, cin, requires_grad=True)
        g = torch.randn(BATCH, cout)
        y = layer(x).value
        y.backward(g)
        assert list(layer.state_dict().keys()) == ['scale']
        arrays['c%d_shape' % i] = np.array([cin, cout], dtype=np.int64)
        for key, t in (('x', x), ('g', g), ('scale', layer.scale), ('y', y), ('dx', x.grad), ('dscale', layer.scale.grad)):
            arrays['c%d_%s' % (i, key)] = t.detach().numpy().copy()
    np.savez(os.path.join(HERE, 'hadamard_classifier.npz'), **arrays)
    print('wrote hadamard_classifier.npz:', {k: v.shape for k, v in arrays.items()})


if __name__ == '__main__':
    main()
