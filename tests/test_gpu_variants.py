"""Quantizer variants of the same elementwise family: binary, clamped binary, ternary,
decoupled and truncating quantizers against the reference (tests/golden/variants.npz: float32, bfloat16 and float16;
0-dim learned scales and per-channel ones, plain and straight-through clamps, non-zero zero-points, gradients of
both decoupled scales).  On a device tensor each runs as ONE forward kernel and ONE backward kernel
(include/bvq.h, bvq_variant_fwd / bvq_variant_bwd): y and dx bit-exact, scale gradients within the rounding of a
reduced sum (the reference rounds every product and the running sum to the tensor dtype)."""
import numpy as np
import pytest
import torch

import golden_util as G
from test_gpu_modules import SUM_RTOL, assert_bits

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CASES = G.load('variants')
DT = {'f32': torch.float32, 'bf16': torch.bfloat16, 'f16': torch.float16}


@pytest.fixture(autouse=True)
def cpu_scalar_semantics(monkeypatch):
    """the golden vectors come from torch CPU kernels, which keep a 0-dim float32 scale next to a 16-bit tensor in
    float32 (include/bvq.h, bvq_scalar_mode)"""
    import brevitas_amd.config as config
    monkeypatch.setattr(config, 'SCALAR_OPERAND_MODE', 'cpu')


def pick(name):
    return [c for c in CASES if c['quant'] == name]


def assert_sum(got, c, name, terms):
    """a gradient that is a sum of rounded products: the reference rounds every product AND the running sum to the
    tensor dtype (the dtype of dx), whatever dtype the parameter that receives the sum has"""
    want = c.f32(name).reshape(-1)
    got = got.detach().float().cpu().numpy().reshape(-1)
    tol = SUM_RTOL[c['dtypes']['dx']] * (np.abs(want) * 4 + terms)
    assert np.all(np.abs(got - want) <= tol), (name, got, want, tol)


@pytest.mark.parametrize('fused', [True, False], ids=['fused', 'generic'])
@pytest.mark.parametrize('c', pick('binary') + pick('clamped_binary') + pick('ternary'),
                         ids=lambda c: '%s-%s-%s' % (c['quant'], c['dtype'], c.get('tag')))
def test_sign_quantizers(c, fused, monkeypatch):
    import brevitas_amd.config as config
    from brevitas_amd.core.function_wrapper import TensorClampSte
    from brevitas_amd.core.quant import BinaryQuant, ClampedBinaryQuant, TernaryQuant
    from brevitas_amd.core.scaling import ParameterScaling
    monkeypatch.setattr(config, 'FUSED_PATHS', fused)
    if c.get('tag') == 'per_channel':
        v = c.torch('value')
        q = {'binary': lambda: BinaryQuant(ParameterScaling(v, tuple(v.shape))),
             'clamped_binary': lambda: ClampedBinaryQuant(ParameterScaling(v, tuple(v.shape)),
                                                          tensor_clamp_impl=TensorClampSte()),
             'ternary': lambda: TernaryQuant(ParameterScaling(v, tuple(v.shape)), 0.6)}[c['quant']]().to(DT[c['dtype']])
    else:
        q = {'binary': lambda: BinaryQuant(ParameterScaling(0.7)),
             'clamped_binary': lambda: ClampedBinaryQuant(ParameterScaling(0.7)),
             'ternary': lambda: TernaryQuant(ParameterScaling(0.9), 0.5)}[c['quant']]()
    q = q.to(DEV)
    x = c.torch('x', DEV).requires_grad_(True)
    y, scale, zp, bw = q(x)
    if not fused and c['dtype'] != 'f32' and c.get('tag') != 'per_channel':
        # op by op on the device, torch rounds a 0-dim float32 scale to the tensor dtype first: one ulp at most
        assert bool(((y.float().cpu() - c.torch('y').float()).abs() <= 2.0 ** -7 * c.torch('y').float().abs()).all())
        return
    assert_bits(y, c, 'y')
    assert_bits(scale, c, 'scale')
    assert float(zp) == float(c.f32('zp')) and float(bw) == float(c.f32('bit_width'))
    y.backward(c.torch('g', DEV))
    assert_bits(x.grad, c, 'dx')
    per_sum = x.numel() // q.scaling_impl.value.numel()
    assert_sum(q.scaling_impl.value.grad, c, 'dvalue', np.sqrt(per_sum) * float(np.abs(c.f32('g')).max()))


@pytest.mark.parametrize('fused', [True, False], ids=['fused', 'generic'])
@pytest.mark.parametrize('c', pick('decoupled'), ids=lambda c: '%s-%s' % (c['dtype'], c.get('tag')))
def test_decoupled(c, fused, monkeypatch):
    import brevitas_amd.config as config
    from brevitas_amd.core.bit_width import BitWidthConst
    from brevitas_amd.core.function_wrapper import TensorClamp
    from brevitas_amd.core.quant import DecoupledIntQuant
    monkeypatch.setattr(config, 'FUSED_PATHS', fused)
    x = c.torch('x', DEV).requires_grad_(True)
    t = lambda v: torch.tensor(v, device=DEV)  # noqa: E731
    bw = BitWidthConst(4).to(DEV)()
    if c.get('tag') == 'per_channel':
        dq = DecoupledIntQuant(narrow_range=False, signed=True, tensor_clamp_impl=TensorClamp()).to(DEV)
        pre_scale = c.torch('pre_scale', DEV).requires_grad_(True)
        scale = c.torch('scale', DEV).requires_grad_(True)
        y = dq(pre_scale, t(1.), scale, t(2.), bw, x)
    else:
        dq = DecoupledIntQuant(narrow_range=True, signed=True).to(DEV)
        pre_scale, scale = c.torch('pre_scale', DEV), c.torch('scale', DEV)
        y = dq(pre_scale, t(0.), scale, t(0.), bw, x)
    if not fused and c['dtype'] != 'f32' and c.get('tag') != 'per_channel':
        assert torch.allclose(y.float().cpu(), c.torch('y').float(), atol=0.02)  # 0-dim scales, device rounding
        return
    assert_bits(y, c, 'y')
    y.backward(c.torch('g', DEV))
    assert_bits(x.grad, c, 'dx')
    if c.get('tag') == 'per_channel':
        terms = np.sqrt(x.shape[1]) * float(np.abs(c.f32('g')).max()) * 16
        assert_sum(scale.grad, c, 'dscale', terms)
        assert_sum(pre_scale.grad, c, 'dpre_scale', terms * 64)


@pytest.mark.parametrize('fused', [True, False], ids=['fused', 'generic'])
@pytest.mark.parametrize('c', pick('trunc'), ids=lambda c: '%s-%s' % (c['round'], c['dtype']))
def test_trunc(c, fused, monkeypatch):
    import brevitas_amd.config as config
    from brevitas_amd.core.bit_width import BitWidthConst
    from brevitas_amd.core.function_wrapper import FloorSte, RoundSte
    from brevitas_amd.core.quant import TruncIntQuant
    monkeypatch.setattr(config, 'FUSED_PATHS', fused)
    tq = TruncIntQuant({'floor': FloorSte, 'round': RoundSte}[c['round']](), BitWidthConst(5)).to(DEV)
    x = c.torch('x', DEV).requires_grad_(True)
    in_bw = BitWidthConst(8).to(DEV)()  # a constant bit width handed on by the previous layer: known on the host
    y, scale, zp, bw = tq(x, torch.tensor(0.05, device=DEV), torch.tensor(0., device=DEV), in_bw)
    assert float(bw) == 5.0
    if not fused and c['dtype'] != 'f32':
        assert torch.allclose(y.float().cpu(), c.torch('y').float(), atol=0.06)  # 0-dim scale, device rounding
        return
    assert_bits(y, c, 'y')
    y.backward(c.torch('g', DEV))
    assert_bits(x.grad, c, 'dx')


def test_variant_kernels_are_the_route_taken(monkeypatch):
    """a device tensor with covered operands must run the fused kernels, not the op-by-op composition"""
    from brevitas_amd import _native as nat
    from brevitas_amd.core.quant import BinaryQuant, TernaryQuant
    from brevitas_amd.core.scaling import ParameterScaling
    calls = []
    real = nat.variant_fwd
    monkeypatch.setattr(nat, 'variant_fwd', lambda *a, **k: (calls.append(a[0].kind), real(*a, **k))[1])
    x = torch.randn(4, 33, device=DEV)
    BinaryQuant(ParameterScaling(0.5)).to(DEV)(x)
    TernaryQuant(ParameterScaling(0.5), 0.5).to(DEV)(x.to(torch.bfloat16))
    assert calls == [nat.VAR_BINARY, nat.VAR_TERNARY]


def test_dimensioned_one_element_operand_wider_than_x_takes_the_op_by_op_route(monkeypatch):
    """torch's type promotion: a one-element scale with dimensions -- shape (1,) -- and a wider dtype than x promotes
    every op to ITS dtype (the ternary threshold compare and the binary clamp then run in float32), a 0-dim one does
    not.  The fused kernels follow the 0-dim rule, so the dimensioned operand must take the op-by-op route and equal
    the reference composition bit for bit; same for a dimensioned float32 zero-point of the truncating quantizer."""
    from brevitas_amd import _native as nat
    from brevitas_amd.core.bit_width import BitWidthConst
    from brevitas_amd.core.function_wrapper import RoundSte
    from brevitas_amd.core.quant import ClampedBinaryQuant, TernaryQuant, TruncIntQuant
    from brevitas_amd.core.scaling import ParameterScaling
    calls = []
    real = nat.variant_fwd
    monkeypatch.setattr(nat, 'variant_fwd', lambda *a, **k: (calls.append(a[0].kind), real(*a, **k))[1])
    torch.manual_seed(3)
    x = (torch.randn(64, 33, device=DEV) * 0.5).to(torch.bfloat16)
    s1 = torch.tensor([0.40234375 + 2.0 ** -12], device=DEV)            # float32, shape (1,): not a bf16 value
    for make in (lambda: TernaryQuant(ParameterScaling(s1.detach().cpu().clone(), scaling_shape=(1,)), 0.5),
                 lambda: ClampedBinaryQuant(ParameterScaling(s1.detach().cpu().clone(), scaling_shape=(1,)))):
        y = make().to(DEV)(x)[0]
        y_cpu = make()(x.cpu())[0]            # the reference's op composition on CPU tensors (brevitas_amd/_aten.py)
        assert y.dtype == torch.float32       # promoted by the dimensioned float32 scale
        assert torch.equal(y.cpu(), y_cpu)
    tq = TruncIntQuant(RoundSte(), BitWidthConst(4)).to(DEV)
    zp1 = torch.tensor([1.0], device=DEV)                                # float32, shape (1,)
    sc = torch.tensor(0.125, device=DEV, dtype=torch.bfloat16)
    y = tq(x, sc, zp1, torch.tensor(8.0, device=DEV))[0]
    y_cpu = TruncIntQuant(RoundSte(), BitWidthConst(4))(x.cpu(), sc.cpu(), zp1.cpu(), torch.tensor(8.0))[0]
    assert y.dtype == torch.float32 and torch.equal(y.cpu(), y_cpu)
    assert calls == [], 'a dimensioned wider one-element operand reached a fused variant kernel'
    # the 0-dim forms of the same operands do take the kernels
    TernaryQuant(ParameterScaling(float(s1)), 0.5).to(DEV)(x)
    assert calls == [nat.VAR_TERNARY]


def test_doctests():
    from brevitas_amd.core.quant import DecoupledIntQuant, TernaryQuant
    from brevitas_amd.core.scaling import ConstScaling
    t = lambda v: torch.tensor(v, device=DEV)  # noqa: E731
    c = pick('decoupled_doctest')[0]
    y = DecoupledIntQuant(narrow_range=True, signed=True).to(DEV)(t(0.02), t(0.), t(0.01), t(0.), t(4.), c.torch('x', DEV))
    assert_bits(y, c, 'y')
    assert torch.allclose(y.cpu(), torch.tensor([0.02, -0.03, 0.07, -0.07]), atol=5e-5)
    c = pick('ternary_doctest')[0]
    y, scale, zp, bw = TernaryQuant(ConstScaling(1.0), 0.5).to(DEV)(c.torch('x', DEV))
    assert y.tolist() == [0.0, -1.0, 1.0] and float(scale) == 1.0 and float(zp) == 0.0 and float(bw) == 2.0


def _sums_close(got, want, name):
    """float32 sums in another order: the form and limit of test_gpu_fuzz.py"""
    got, want = got.double().cpu().reshape(-1), want.double().cpu().reshape(-1)
    mag = float(want.abs().max())
    assert bool(((got - want).abs() <= 2e-4 * (want.abs() + mag + 1.0)).all()), (name, got[:4], want[:4])


def _large_step(kind, shape, channels_last):
    """one forward and backward of `kind` on a seeded float32 tensor -> (y, dx, parameter gradients)"""
    from brevitas_amd.core.bit_width import BitWidthConst
    from brevitas_amd.core.function_wrapper import RoundSte, TensorClamp
    from brevitas_amd.core.quant import BinaryQuant, ClampedBinaryQuant, DecoupledIntQuant, TernaryQuant, TruncIntQuant
    from brevitas_amd.core.scaling import ParameterScaling
    gen = torch.Generator().manual_seed(11)
    ch = shape[1]
    v = torch.rand(1, ch, 1, 1, generator=gen) * 0.5 + 0.25
    x = torch.randn(shape, generator=gen)
    g = torch.randn(shape, generator=gen).to(DEV)
    x = x.to(DEV)
    if channels_last:
        x = x.contiguous(memory_format=torch.channels_last)
    x.requires_grad_(True)
    if kind in ('binary', 'clamped_binary', 'ternary'):
        q = {'binary': lambda: BinaryQuant(ParameterScaling(v, tuple(v.shape))),
             'clamped_binary': lambda: ClampedBinaryQuant(ParameterScaling(v, tuple(v.shape)),
                                                          tensor_clamp_impl=TensorClamp()),
             'ternary': lambda: TernaryQuant(ParameterScaling(v, tuple(v.shape)), 0.6)}[kind]().to(DEV)
        y = q(x)[0]
        params = [q.scaling_impl.value]
    elif kind == 'decoupled':
        dq = DecoupledIntQuant(narrow_range=False, signed=True, tensor_clamp_impl=TensorClamp()).to(DEV)
        pre_scale = (v * 0.1).to(DEV).requires_grad_(True)
        scale = (v * 0.12).to(DEV).requires_grad_(True)
        t = lambda s: torch.tensor(s, device=DEV)  # noqa: E731
        y = dq(pre_scale, t(1.), scale, t(2.), BitWidthConst(4).to(DEV)(), x)
        params = [scale, pre_scale]
    else:
        tq = TruncIntQuant(RoundSte(), BitWidthConst(5)).to(DEV)
        scale = torch.tensor(0.05, device=DEV, requires_grad=True)
        y = tq(x * 4, scale, torch.tensor(0., device=DEV), BitWidthConst(8).to(DEV)())[0]
        params = [scale]
    y.backward(g)
    return y.detach(), x.grad, [p.grad for p in params]


@pytest.mark.parametrize('layout', ['nchw', 'channels_last'])
@pytest.mark.parametrize('kind', ['binary', 'clamped_binary', 'ternary', 'decoupled', 'trunc'])
def test_large_fused_route_equals_op_by_op(kind, layout, monkeypatch):
    """float32 [32,64,28,28] (and a channels_last tensor): the fused kernels and the op-by-op route on the device give
    the same y and dx bits and the same parameter gradients up to the order of the float32 sums; the NCHW case takes
    the kernels"""
    import brevitas_amd.config as config
    from brevitas_amd import _native as nat
    shape, cl = ((32, 64, 28, 28), False) if layout == 'nchw' else ((8, 64, 28, 28), True)
    calls = []
    for name in ('variant_fwd', 'variant_bwd'):
        real = getattr(nat, name)
        monkeypatch.setattr(nat, name, lambda *a, _r=real, _n=name, **k: (calls.append(_n), _r(*a, **k))[1])
    monkeypatch.setattr(config, 'FUSED_PATHS', True)
    y1, dx1, p1 = _large_step(kind, shape, cl)
    if not cl:
        assert calls == ['variant_fwd', 'variant_bwd'], calls
    calls.clear()
    monkeypatch.setattr(config, 'FUSED_PATHS', False)
    y0, dx0, p0 = _large_step(kind, shape, cl)
    assert calls == []
    assert torch.equal(y1, y0), 'y'
    assert torch.equal(dx1, dx0), 'dx'
    for i, (a, b) in enumerate(zip(p1, p0)):
        _sums_close(a, b, 'parameter %d' % i)
