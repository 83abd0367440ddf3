"""The Hadamard transform without a device: the composed route against a float64 dense Sylvester product, unit vectors,
the backward, the refusals of the function and of the C ABI, HadamardClassifier against the reference's layer (fixture
tests/golden/hadamard_classifier.npz, written by tests/golden/make_golden_hadamard.py), merging rotations into weights,
and the condition that a rotation helps a 4-bit layer with outlier channels."""
import copy
import functools
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from brevitas_amd import _native as nat
from brevitas_amd import quant as Q
from brevitas_amd.function.hadamard import hadamard_matrix, hadamard_transform
from brevitas_amd.graph import (gptq_mode, insert_online_rotation, merge_input_rotation, merge_output_rotation,
                                rotate_pair)
from brevitas_amd.nn import HadamardClassifier, HadamardRotation, QuantConv2d, QuantLinear, RotatedModule

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'hadamard_classifier.npz')
DTYPES = {'f32': torch.float32, 'bf16': torch.bfloat16, 'f16': torch.float16}
ROUND = {'f32': 2.0 ** -23, 'f16': 2.0 ** -11, 'bf16': 2.0 ** -8}  # the output rounding: r * |y64|
BLOCKS = (2, 8, 64, 1024)


def dense64(x, b, scale):
    """the float64 dense product, block by block"""
    h = hadamard_matrix(b, torch.float64)
    xb = x.double().reshape(*x.shape[:-1], -1, b)
    return (scale * (xb @ h)).reshape(x.shape)


def bound(x, y64, b, scale, r):
    """1.01 * scale * (log2 b + 1) * 2^-24 * ||x_block||_1 + r * |y64|: the first-order bound of log2 b float32 additions
    plus the multiply, and the output rounding"""
    l1 = x.double().abs().reshape(*x.shape[:-1], -1, b).sum(dim=-1, keepdim=True)
    l1 = l1.expand(*x.shape[:-1], x.shape[-1] // b, b).reshape(x.shape)
    return 1.01 * abs(scale) * (math.log2(b) + 1) * 2.0 ** -24 * l1 + r * y64.abs()


@pytest.mark.parametrize('b', BLOCKS)
@pytest.mark.parametrize('dt', list(DTYPES))
def test_composed_route_against_the_dense_sylvester_product(dt, b):
    torch.manual_seed(b)
    x = torch.randn(4, 3 * b).to(DTYPES[dt])
    scale = 1.0 / math.sqrt(b)
    y = hadamard_transform(x, b)
    assert y.dtype == x.dtype and y.shape == x.shape
    y64 = dense64(x, b, scale)
    assert ((y.double() - y64).abs() <= bound(x, y64, b, scale, ROUND[dt])).all()
    # leading shape, default block (the largest power of two dividing 3 b is b)
    assert torch.equal(hadamard_transform(x.reshape(2, 2, 3 * b)).reshape(4, 3 * b), y)


@pytest.mark.parametrize('b', BLOCKS)
@pytest.mark.parametrize('dt', list(DTYPES))
def test_unit_vectors_give_the_rows_of_the_matrix(dt, b):
    h = hadamard_matrix(b)
    for k in sorted({0, 1, b // 2, b - 2, b - 1}):
        e = torch.zeros(b, dtype=DTYPES[dt])
        e[k] = 1.0
        assert torch.equal(hadamard_transform(e, b, 1.0).float(), h[k]), (dt, b, k)


def test_matrix_is_sylvester():
    h = hadamard_matrix(8)
    assert torch.equal(h[:2, :4], torch.tensor([[1., 1, 1, 1], [1, -1, 1, -1]]))
    assert torch.equal(h @ h.t(), 8 * torch.eye(8))
    i = torch.arange(64)
    pop = sum(((i[:, None] & i[None, :]) >> s) & 1 for s in range(6))
    assert torch.equal(hadamard_matrix(64), (1 - 2 * (pop & 1)).float())
    with pytest.raises(ValueError, match='12'):
        hadamard_matrix(12)


@pytest.mark.parametrize('dt', list(DTYPES))
def test_backward_is_the_forward_on_the_gradient(dt):
    b = 64
    torch.manual_seed(5)
    x = torch.randn(3, 3 * b).to(DTYPES[dt]).requires_grad_(True)
    g = torch.randn(3, 3 * b).to(DTYPES[dt])
    hadamard_transform(x, b).backward(g)
    assert torch.equal(x.grad, hadamard_transform(g, b))
    x64 = x.detach().double().requires_grad_(True)
    dense64(x64, b, 1.0 / math.sqrt(b)).backward(g.double())
    assert ((x.grad.double() - x64.grad).abs() <= bound(g, x64.grad, b, 1.0 / math.sqrt(b), ROUND[dt])).all()


def test_refusals_of_the_function():
    x = torch.randn(2, 24)
    for bad in (6, 1, 16, 32, 0):
        with pytest.raises(ValueError, match=r'%d\b.*\b24\b' % bad):
            hadamard_transform(x, bad)
    assert hadamard_transform(x).shape == x.shape  # default: 8
    assert torch.equal(hadamard_transform(x), hadamard_transform(x, 8))
    with pytest.raises(TypeError, match='float64'):
        hadamard_transform(x.double())


def test_c_abi_refuses_before_the_device():
    had, sup = nat.lib.bvq_hadamard, nat.lib.bvq_hadamard_supported

    def refused(rc, word, *args):
        assert had(*args, None) == rc and word in nat.last_error(), (args, nat.last_error())
        assert sup(args[0], args[2], args[3], args[4], args[1], args[6]) == 0

    refused(-1, 'power of two', nat.BF16, None, 4, 24, 6, 1.0, None)
    refused(-1, 'power of two', nat.BF16, None, 4, 24, 1, 1.0, None)
    refused(-1, 'divide', nat.BF16, None, 4, 24, 32, 1.0, None)      # block > cols
    refused(-1, 'divide', nat.BF16, None, 4, 24, 16, 1.0, None)      # cols % block != 0
    refused(-2, '65536 bytes', nat.BF16, None, 4, 32768, 32, 1.0, None)  # a row above 32 KiB
    refused(-2, 'bytes', nat.BF16, None, 4, 12, 4, 1.0, None)         # a row of 24 bytes: no multiple of 16
    refused(-2, '16-byte', nat.BF16, 4096 + 8, 4, 64, 32, 1.0, 4096)  # a misaligned pointer value
    refused(-2, '16-byte', nat.BF16, 4096, 4, 64, 32, 1.0, 4096 + 2)
    refused(-1, 'dtype', 7, None, 4, 64, 32, 1.0, None)
    refused(-1, 'null', nat.F32, None, 4, 64, 32, 1.0, None)
    refused(-1, 'rows', nat.F32, None, 0, 64, 32, 1.0, None)


# ---- HadamardClassifier ----------------------------------------------------------------------------------------------

def _golden_cases():
    z = np.load(GOLDEN)
    n = len([k for k in z.files if k.endswith('_shape')])
    return [{k.split('_', 1)[1]: torch.from_numpy(z[k]) for k in z.files if k.startswith('c%d_' % i)} for i in range(n)]


def test_classifier_against_the_reference_layer():
    """the reference multiplies by the dense matrix (another summation order): the dense-product bound on the normalised
    input.  The gradients are sums the two sides order differently as well -- of `out` terms (the dense product's
    backward) and of batch * in terms (the norm's, taken over the whole tensor): n float32 additions deviate by at most
    n * 2^-24 of the sum of the terms' magnitudes, on either side."""
    cases = _golden_cases()
    assert [tuple(c['shape'].tolist()) for c in cases] == [(24, 10), (64, 64), (10, 40)]
    for c in cases:
        cin, cout = c['shape'].tolist()
        layer = HadamardClassifier(cin, cout)
        layer.load_state_dict({'scale': c['scale']}, strict=True)
        x = c['x'].clone().requires_grad_(True)
        y = layer(x)
        y.backward(c['g'])
        s, sz = float(c['scale']), layer.size
        x64 = c['x'].double()
        n64 = x64.norm() + 1e-8
        u = x64 / n64
        tol_y = 1.01 * abs(s) * (math.log2(sz) + 1) * 2.0 ** -24 * u.abs().sum(dim=1, keepdim=True) + \
            2.0 ** -23 * c['y'].double().abs()
        assert ((y.detach().double() - c['y'].double()).abs() <= tol_y).all(), (cin, cout)
        # magnitudes of the terms of each gradient (|H| is all ones)
        g64 = c['g'].double().abs()
        terms = x64.numel() + cout + math.log2(sz) + 8
        a = abs(s) * g64.sum(dim=1, keepdim=True).expand(-1, cin)           # |dL/du|
        mag_dx = a / n64 + x64.abs() * (a * x64.abs()).sum() / (n64 * n64 * x64.norm())
        assert ((x.grad.double() - c['dx'].double()).abs() <= 2 * terms * 2.0 ** -24 * mag_dx).all(), (cin, cout)
        mag_ds = (g64 * u.abs().sum(dim=1, keepdim=True)).sum()
        assert abs(float(layer.scale.grad) - float(c['dscale'])) <= \
            2 * (c['g'].numel() + math.log2(sz) + 8) * 2.0 ** -24 * float(mag_ds), (cin, cout)


def test_classifier_state_and_bit_width():
    layer = HadamardClassifier(24, 10)
    assert set(layer.state_dict().keys()) == {'scale'} and isinstance(layer.scale, torch.nn.Parameter)
    assert float(layer.scale.detach()) == pytest.approx(1 / math.sqrt(10))
    fixed = HadamardClassifier(24, 10, fixed_scale=True)
    assert set(fixed.state_dict().keys()) == {'scale'} and not list(fixed.parameters())
    fixed.load_state_dict({'scale': torch.tensor(0.5)}, strict=True)
    assert float(fixed.scale) == 0.5
    assert layer.size == 32 and HadamardClassifier(64, 64).size == 64 and HadamardClassifier(10, 40).size == 64
    # 8-bit unsigned inputs, 24 of them: 255 * 24 = 6120 -> 13 bits
    assert float(layer.max_output_bit_width(torch.tensor(8.0))) == 13.0
    # the definition, densely
    x = torch.randn(5, 24)
    want = -layer.scale * F.linear(x / (x.norm() + 1e-8), hadamard_matrix(32)[:10, :24])
    torch.testing.assert_close(layer(x), want, rtol=1e-5, atol=1e-6)


# ---- merging ---------------------------------------------------------------------------------------------------------

def _tol_linear(w, h, b):
    """elementwise bound [batch, out] on (W R)(R h) against W h in float32: a k-term sum on either side and the
    (log2 b + 1) operations of the two transforms, each at most 2^-24 of the sum of the magnitudes of its terms, which
    Cauchy-Schwarz bounds by sqrt(k) * ||w_row||_2 * ||h_row||_2 (R preserves the 2-norms)"""
    k = w.shape[1]
    ops = k + 2 * (math.log2(b) + 1) + 4
    return ops * 2.0 ** -24 * math.sqrt(k) * h.double().norm(dim=1, keepdim=True) * w.double().norm(dim=1)[None, :]


def test_rotate_pair_leaves_the_composition_unchanged():
    torch.manual_seed(7)
    model = torch.nn.Sequential(torch.nn.Linear(48, 96), torch.nn.Linear(96, 20))
    x = torch.randn(9, 48)
    want = model(x).detach()
    w0, b0 = model[0].weight.detach().clone(), model[0].bias.detach().clone()
    rotate_pair(model[0], model[1], 32)
    assert not torch.equal(model[0].weight, w0)
    mid = F.linear(x, w0, b0)
    w1 = model[1].weight.detach()
    tol_mid = _tol_linear(w0, x, 32) + 4 * 2.0 ** -24 * mid.double().abs().sum(dim=1, keepdim=True)
    tol = _tol_linear(w1, mid, 32) + tol_mid.norm(dim=1, keepdim=True) * w1.double().norm(dim=1)[None, :]
    assert ((model(x).detach().double() - want.double()).abs() <= tol).all()
    # what flows between the two is rotated
    torch.testing.assert_close(model[0](x), hadamard_transform(mid, 32), rtol=1e-4, atol=1e-5)
    # R is its own inverse: merging twice restores the weight
    lin = torch.nn.Linear(64, 8)
    w = lin.weight.detach().clone()
    merge_input_rotation(merge_input_rotation(lin))
    torch.testing.assert_close(lin.weight.detach(), w, rtol=1e-5, atol=1e-6)
    with pytest.raises(ValueError, match='96.*40'):
        rotate_pair(model[0], torch.nn.Linear(40, 4))


def test_insert_online_rotation_leaves_a_float_model_unchanged():
    torch.manual_seed(8)
    model = torch.nn.Sequential(torch.nn.Linear(24, 64), torch.nn.ReLU(),
                                torch.nn.Sequential(QuantLinear(64, 12), torch.nn.Tanh()))
    x = torch.randn(5, 24)
    want = model(x).detach()
    inner = model[2][0]
    rot = insert_online_rotation(model, '2.0', 16)
    assert isinstance(model[2][0], RotatedModule) and rot is model[2][0] and rot.layer is inner
    assert '2.0.layer.weight' in model.state_dict()
    assert any(m is inner for m in model.modules())
    h = F.relu(model[0](x)).detach()
    assert ((model(x).detach().double() - want.double()).abs() <= _tol_linear(inner.weight.detach(), h, 16)).all()
    assert torch.equal(HadamardRotation(16)(x[:, :16]), hadamard_transform(x[:, :16], 16))


def test_merging_refuses_what_it_does_not_cover():
    conv = QuantConv2d(4, 8, 3)
    for fn in (merge_input_rotation, merge_output_rotation):
        with pytest.raises(NotImplementedError, match='QuantConv2d'):
            fn(conv)
    with pytest.raises(NotImplementedError, match='Conv2d'):
        rotate_pair(torch.nn.Linear(4, 4), torch.nn.Conv2d(4, 4, 1))
    from brevitas_amd.graph import freeze_weight_quant
    lin = QuantLinear(32, 8, weight_quant=functools.partial(Q.Int4WeightPerGroupFloat, group_size=16))
    w, s, z, _ = lin.quant_weight()
    with torch.no_grad():
        lin.weight.copy_(w)
    freeze_weight_quant(lin, s.detach(), z.detach())
    for fn in (merge_input_rotation, merge_output_rotation):
        with pytest.raises(RuntimeError, match='rotate before quantizing'):
            fn(lin)
    with pytest.raises(RuntimeError, match='rotate before quantizing'):
        insert_online_rotation(torch.nn.Sequential(lin), '0')


def test_gptq_mode_finds_the_layer_inside_a_rotated_module():
    torch.manual_seed(9)
    model = torch.nn.Sequential(
        torch.nn.Linear(16, 32), torch.nn.ReLU(),
        QuantLinear(32, 12, weight_quant=functools.partial(Q.Int4WeightPerGroupFloat, group_size=16)))
    insert_online_rotation(model, '2', 32)
    inner = model[2].layer
    w_before = inner.weight.detach().clone()
    batches = [torch.randn(40, 16) for _ in range(2)]
    with gptq_mode(model) as gptq:
        assert [name for name, _ in gptq.layers] == ['2.layer']
        for b in batches:
            gptq.model(b)
        # the Hessian is that of the ROTATED input
        rows = torch.cat([hadamard_transform(F.relu(model[0](b)), 32) for b in batches]).detach()
        torch.testing.assert_close(gptq._h, (2.0 / 80) * (rows.t() @ rows), rtol=1e-4, atol=1e-5)
        res = gptq.update()
    assert torch.equal(inner.weight.detach(), res.q) and not torch.equal(res.q, w_before)
    assert inner._buffers.get('frozen_weight_scale') is not None
    assert model(batches[0]).shape == (40, 12)


# ---- it helps --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('seed', range(5))
def test_rotation_reduces_the_error_of_a_4_bit_layer_with_outlier_channels(seed):
    """int4 weights in groups of 32, per-token int4 inputs, three input channels scaled by 30: the relative output
    error is smaller with the online rotation than without (observed 0.115-0.129 against 0.260-0.300,
    profiles/hadamard.md)"""
    torch.manual_seed(seed)
    lin = QuantLinear(256, 64, weight_quant=functools.partial(Q.Int4WeightPerGroupFloat, group_size=32),
                      input_quant=Q.Int8DynamicActPerRowFloat(bit_width=4))
    x = torch.randn(32, 256)
    x[:, [3, 77, 200]] *= 30
    want = F.linear(x, lin.weight, lin.bias).detach()

    def rel_err(m):
        return float((m(x).detach() - want).norm() / want.norm())

    plain = rel_err(lin)
    model = torch.nn.Sequential(copy.deepcopy(lin))
    insert_online_rotation(model, '0', block_size=256)
    rotated = rel_err(model)
    print('seed %d: plain %.4f rotated %.4f' % (seed, plain, rotated))
    assert rotated < plain
