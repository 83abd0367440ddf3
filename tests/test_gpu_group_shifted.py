"""Asymmetric group-wise weight quantizers on the device: the one-kernel route (csrc/bvq_group_shifted.hip) against the
reference's golden vectors and against the per-channel asymmetric quantizer on the regrouped weight; the refusals, the
layers, WeightQuantGroup, graph capture and the guard elements behind every output.

Bars: y, scale and zp are bit-exact everywhere (a NaN equals a NaN).  dw is bit-exact except at the first element equal
to the minimum and the first equal to the maximum of each group, which receive reduced float32 sums: the group kernel
adds a group's terms in another order than the per-channel kernels, so those elements may differ by the roundings
derived at test_group_shifted_golden.deposit_ulps.
"""
import ctypes
import functools

import pytest
import torch

import golden_util as G
from test_group_shifted_golden import CASES, assert_dx, case, check_case, run_case, stat_positions, to_np

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
DT = {'f32': torch.float32, 'bf16': torch.bfloat16, 'f16': torch.float16}
# [out, K], group size: less than one wave load in every dtype; a whole wave per float32 group with a ragged last
# wave; a number of groups that is no multiple of the groups per load; several waves, workgroups and the full depth
# and 27 groups of 64, ragged in every dtype (the shapes of tests/test_gpu_group_quant.py)
SHAPES = [((3, 64), 16), ((5, 512), 256), ((7, 96), 32), ((64, 4096), 128), ((9, 192), 64)]
shapes = pytest.mark.parametrize('shape,g', SHAPES, ids=['3x64-g16', '5x512-g256', '7x96-g32', '64x4096-g128',
                                                         '9x192-g64'])
dtypes = pytest.mark.parametrize('dn', ['f32', 'bf16', 'f16'])


@pytest.fixture
def cpu_scalar_semantics(monkeypatch):
    """the golden vectors were produced by torch CPU kernels (include/bvq.h, bvq_scalar_mode)"""
    import brevitas_amd.config as config
    monkeypatch.setattr(config, 'SCALAR_OPERAND_MODE', 'cpu')


@pytest.fixture
def fused_calls(monkeypatch):
    """counts the launches of the asymmetric group kernels' forward wrapper"""
    from brevitas_amd import _native as nat
    calls = []
    real = nat.group_shifted_fwd

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)
    monkeypatch.setattr(nat, 'group_shifted_fwd', counted)
    return calls


def plant(w2):
    """the groups of tests/golden/make_golden_group_shifted.py, groups 0 .. 9 of w2 = [groups, g], in place"""
    g = w2.shape[1]
    w2[0] = 0.0                                   # all zero
    w2[1] = 0.015625                              # constant, non-zero
    w2[2] = w2[2].abs() + 0.01                    # positive values only
    w2[3] = -(w2[3].abs()) - 0.01                 # negative values only
    for grp, sign, (first, second) in ((4, -1, (2, g - 3)), (5, -1, (5, 6)), (6, 1, (1, g - 2)), (7, 1, (4, 5))):
        m = (w2[grp].abs().max().float() * 1.25).to(w2.dtype) * sign
        w2[grp, first], w2[grp, second] = m, m    # minimum / maximum tied across chunks and inside one
    m = (w2[8].abs().max().float() * 1.5).to(w2.dtype)
    w2[8, 0], w2[8, g - 1] = m, -m                # maximum first, minimum last
    w2[9] = -(w2[9].abs()) - 0.001
    w2[9, 3], w2[9, g - 4] = -0.0, 0.0            # the maximum is zero, -0.0 first


def make_weight(shape, g, dn, seed=654321):
    gen = torch.Generator().manual_seed(seed)
    w = (torch.randn(shape, generator=gen) * 0.02).to(DT[dn])
    plant(w.view(-1, g))
    grad = torch.randn(shape, generator=gen).to(DT[dn])
    gscale = torch.randn(w.numel() // g, generator=gen).to(DT[dn])
    gzp = (torch.randn(w.numel() // g, generator=gen) * 0.01).to(DT[dn])
    return w, grad, gscale, gzp


def set_clamp(q, ste):
    from brevitas_amd.core.function_wrapper import TensorClamp, TensorClampSte
    q.int_quant.tensor_clamp_impl = TensorClampSte() if ste else TensorClamp()
    return q


def step(q, w, grad, gscale=None, gzp=None):
    """grad None: y receives no gradient, the loss uses the returned scale and / or zero-point alone"""
    w.grad = None
    y, scale, zp, _ = q(w)
    outs, grads = ([y], [grad.view(y.shape)]) if grad is not None else ([], [])
    if gscale is not None:
        outs, grads = outs + [scale], grads + [gscale.view(scale.shape)]
    if gzp is not None:
        outs, grads = outs + [zp], grads + [gzp.view(zp.shape)]
    torch.autograd.backward(outs, grads)
    return y.detach(), scale.detach(), zp.detach(), w.grad.detach().clone()


def grouped_step(w0, g, bits, ste, grad, gscale=None, gzp=None):
    import brevitas_amd.quant as Q
    w = torch.nn.Parameter(w0.clone())
    q = set_clamp(Q.ShiftedUint8WeightPerGroupFloat(w, group_size=g, bit_width=bits).to(w.device), ste)
    return step(q, w, grad, gscale, gzp)


def per_channel_step(w0, g, bits, ste, grad, gscale=None, gzp=None):
    """the parent's route: the per-channel asymmetric quantizer on the regrouped weight"""
    import brevitas_amd.quant as Q
    w = torch.nn.Parameter(w0.detach().contiguous().view(-1, g).clone())
    q = set_clamp(Q.ShiftedUint8WeightPerChannelFloat(w, bit_width=bits).to(w.device), ste)
    return step(q, w, None if grad is None else grad.contiguous().view(-1, g), gscale, gzp)


def assert_same_bits(a, b, dn, what):
    assert G.same_bits(to_np(a).reshape(-1), to_np(b).reshape(-1), dn), what


def compare(got, want, w, grad, g, bits, dn, gscale=None, gzp=None, skip_groups=()):
    """(y, scale, zp, dw) of two routes -> the worst deposit difference in ulps"""
    for a, b, name in zip(got[:3], want[:3], ('y', 'scale', 'zp')):
        assert_same_bits(a, b, dn, name)
    return assert_dx(got[3].contiguous(), want[3], w, grad, want[1], want[2], g, bits, dn, gscale, gzp, skip_groups)


def compare_without_gy(got, want, w, g, bits, dn, gscale=None, gzp=None):
    """compare for two steps in which y received no gradient: dw is zero by value away from the first-minimum and
    first-maximum element of each group (or NaN where the other route's is NaN too), and the deposit bar holds at
    them.  The sign of such a zero is nobody's contract and assert_dx compares bits: "+ 0.0" makes -0 and +0 one.

    An expected difference, as the kernels stand: a group whose scale is zero (float16, where min_val = 1e-10 underflows:
    the all-zero and the constant group) or not finite.  The one-launch backward always runs, on zeros for y's gradient,
    and the arithmetic on x / scale gives NaN over the whole group; on the per-channel route autograd never enters the
    quantizer's backward when y is unused, and the group gets zeros and its deposits.  With a gradient for y both routes
    give NaN there.  Such groups may hold NaN here and are left out of the deposit bar; every other group is held to
    zero."""
    off = torch.ones(w.numel(), dtype=torch.bool)
    off[sorted(stat_positions(w, g))] = False
    scale = want[1].reshape(-1).float().cpu()
    degenerate = ~(scale.isfinite() & (scale != 0))
    dw, dw_ref = got[3].reshape(-1).float().cpu(), want[3].reshape(-1).float().cpu()
    ok = (dw == 0) | (dw.isnan() & (dw_ref.isnan() | degenerate.repeat_interleave(g)))
    assert bool(ok[off].all()), torch.nonzero(~ok & off).reshape(-1)[:8].tolist()
    return compare(got[:3] + (got[3] + 0.0,), want[:3] + (want[3] + 0.0,), w, torch.zeros_like(w), g, bits, dn, gscale,
                   gzp, skip_groups=set(torch.nonzero(degenerate).reshape(-1).tolist()))


# ---- golden ---------------------------------------------------------------------------------------------------------

@case
@pytest.mark.parametrize('fused', [True, False], ids=['fused', 'generic'])
def test_golden(c, fused, fused_calls, cpu_scalar_semantics, monkeypatch):
    import brevitas_amd.config as config
    monkeypatch.setattr(config, 'FUSED_PATHS', fused)
    worst = check_case(c, *run_case(c, DEV))
    assert len(fused_calls) == (1 if fused else 0)
    print('GROUP_SHIFTED_DEPOSIT_ULPS golden %s g=%d bits=%d fused=%d worst=%.3f'
          % (c['dtype'], c['group_size'], c['bit_width'], fused, worst))


# ---- device against device ------------------------------------------------------------------------------------------

@shapes
@dtypes
@pytest.mark.parametrize('bits', [4, 8])
@pytest.mark.parametrize('ste', [True, False], ids=['clamp_ste', 'clamp'])
def test_fused_route_against_the_per_channel_route(shape, g, dn, bits, ste, fused_calls):
    w, grad, _, _ = make_weight(shape, g, dn)
    w, grad = w.to(DEV), grad.to(DEV)
    got = grouped_step(w, g, bits, ste, grad)
    assert len(fused_calls) == 1
    assert tuple(got[1].shape) == tuple(got[2].shape) == (shape[0], shape[1] // g, 1)
    zf = got[2].float()
    finite = torch.isfinite(zf)
    assert bool((zf[finite] == zf[finite].round()).all()) and bool(((zf[finite] >= 0) & (zf[finite] <= 2 ** bits - 1)).all())
    worst = compare(got, per_channel_step(w, g, bits, ste, grad), w, grad, g, bits, dn)
    print('GROUP_SHIFTED_DEPOSIT_ULPS %s g=%d bits=%d ste=%d worst=%.3f' % (dn, g, bits, ste, worst))


@dtypes
@pytest.mark.parametrize('ste', [True, False], ids=['clamp_ste', 'clamp'])
def test_gradients_through_scale_and_zero_point(dn, ste, fused_calls):
    """the loss uses the returned scale and zero-point too: their gradients join the group's sums before the deposits"""
    shape, g = (7, 96), 32
    w, grad, gscale, gzp = make_weight(shape, g, dn)
    w, grad, gscale, gzp = w.to(DEV), grad.to(DEV), gscale.to(DEV), gzp.to(DEV)
    plain = grouped_step(w, g, 4, ste, grad)
    for gs, gz in ((gscale, None), (None, gzp), (gscale, gzp)):
        got = grouped_step(w, g, 4, ste, grad, gs, gz)
        worst = compare(got, per_channel_step(w, g, 4, ste, grad, gs, gz), w, grad, g, 4, dn, gs, gz)
        assert not torch.equal(got[3].float().nan_to_num(), plain[3].float().nan_to_num())  # the gradient arrived
        print('GROUP_SHIFTED_DEPOSIT_ULPS %s g=%d gscale=%d gzp=%d ste=%d worst=%.3f'
              % (dn, g, gs is not None, gz is not None, ste, worst))
    assert len(fused_calls) == 4
    for gs, gz in ((gscale, None), (None, gzp)):   # y receives no gradient: the kernel takes zeros for it
        got = grouped_step(w, g, 4, ste, None, gs, gz)
        worst = compare_without_gy(got, per_channel_step(w, g, 4, ste, None, gs, gz), w, g, 4, dn, gs, gz)
        assert bool(got[3].float().nan_to_num().any())  # the gradient arrived
        print('GROUP_SHIFTED_DEPOSIT_ULPS %s g=%d no gy gscale=%d gzp=%d ste=%d worst=%.3f'
              % (dn, g, gs is not None, gz is not None, ste, worst))
    assert len(fused_calls) == 6


@dtypes
def test_a_group_with_a_nan(dn, fused_calls):
    """a NaN reaches both statistics, whatever its sign and wherever it stands: the group's outputs are NaN"""
    shape, g = (7, 96), 32
    w, grad, _, _ = make_weight(shape, g, dn)
    w.view(-1, g)[10, 9] = float('nan')
    w.view(-1, g)[12, g - 1] = -float('nan')
    w, grad = w.to(DEV), grad.to(DEV)
    got = grouped_step(w, g, 8, True, grad)
    assert len(fused_calls) == 1
    compare(got, per_channel_step(w, g, 8, True, grad), w, grad, g, 8, dn, skip_groups=(10, 12))
    y, scale, zp = got[0], got[1], got[2]
    for grp in (10, 12):
        assert bool(torch.isnan(scale.reshape(-1)[grp])) and bool(torch.isnan(zp.reshape(-1)[grp]))
        assert bool(torch.isnan(y.view(-1, g)[grp]).all())
    if dn != 'f16':  # (float16: the lower bound of the scale underflows, the zero and the constant group are NaN too)
        assert int(torch.isnan(scale).sum()) == 2


def test_two_runs_give_the_same_bits(fused_calls):
    shape, g = (64, 4096), 128
    w, grad, gscale, gzp = make_weight(shape, g, 'bf16')
    w, grad, gscale, gzp = w.to(DEV), grad.to(DEV), gscale.to(DEV), gzp.to(DEV)
    a = grouped_step(w, g, 4, False, grad, gscale, gzp)
    b = grouped_step(w, g, 4, False, grad, gscale, gzp)
    assert len(fused_calls) == 2
    for s, t in zip(a, b):
        assert torch.equal(s.view(torch.int16), t.view(torch.int16))


# ---- refusals stay correct ------------------------------------------------------------------------------------------

@pytest.mark.parametrize('kind', ['misaligned', 'g48', 'non_contiguous'])
def test_refusals_take_the_generic_route(kind, fused_calls):
    dn, bits = 'bf16', 4
    gen = torch.Generator().manual_seed(7)
    if kind == 'misaligned':      # a weight view starting 2 bytes off a 16-byte boundary
        g = 32
        base = (torch.randn(8 * 96 + 8, generator=gen) * 0.02).to(DT[dn]).to(DEV)
        w = base[1:1 + 8 * 96].view(8, 96)
        assert w.data_ptr() % 16 == 2 and w.is_contiguous()
    elif kind == 'g48':
        g = 48
        w = (torch.randn(4, 96, generator=gen) * 0.02).to(DT[dn]).to(DEV)
    else:
        g = 32
        w = (torch.randn(96, 8, generator=gen) * 0.02).to(DT[dn]).to(DEV).t()
        assert not w.is_contiguous()
    grad = torch.randn(w.shape, generator=gen).to(DT[dn]).to(DEV)
    import brevitas_amd.quant as Q
    p = torch.nn.Parameter(w)
    assert p.data_ptr() == w.data_ptr() and p.stride() == w.stride()
    q = Q.ShiftedUint8WeightPerGroupFloat(p, group_size=g, bit_width=bits).to(DEV)
    got = step(q, p, grad)
    assert len(fused_calls) == 0
    assert tuple(got[0].shape) == tuple(w.shape)
    assert tuple(got[1].shape) == tuple(got[2].shape) == (w.shape[0], w.shape[1] // g, 1)
    got = (got[0].contiguous(), got[1], got[2], got[3].contiguous())
    compare(got, per_channel_step(w, g, bits, True, grad), w.contiguous(), grad.contiguous(), g, bits, dn)


# ---- layers ---------------------------------------------------------------------------------------------------------

def test_layers_forward_backward(fused_calls):
    """QuantLinear and QuantConv2d: the layer's output from its quantized weight, and the weight gradient against the
    composed route (the per-channel quantizer on the regrouped weight fed the same output gradient)"""
    import brevitas_amd.quant as Q
    from brevitas_amd.nn import QuantConv2d, QuantLinear
    torch.manual_seed(0)
    lin = QuantLinear(256, 64, weight_quant=functools.partial(Q.ShiftedUint4WeightPerGroupFloat, group_size=64),
                      device=DEV, dtype=torch.bfloat16)
    conv = QuantConv2d(16, 8, 3, padding=1,
                       weight_quant=functools.partial(Q.ShiftedUint4WeightPerGroupFloat, group_size=16),
                       device=DEV, dtype=torch.bfloat16)
    for layer, x, f in ((lin, torch.randn(4, 256, device=DEV, dtype=torch.bfloat16), torch.nn.functional.linear),
                        (conv, torch.randn(2, 16, 8, 8, device=DEV, dtype=torch.bfloat16),
                         functools.partial(torch.nn.functional.conv2d, padding=1))):
        n = len(fused_calls)
        g = layer.weight_quant.group_size
        x.requires_grad_(True)
        y = layer(x)
        y.float().sum().backward()
        assert len(fused_calls) == n + 1
        wq, scale, zp, _ = layer.quant_weight()
        k = layer.weight.numel() // layer.weight.shape[0]
        assert tuple(scale.shape) == tuple(zp.shape) == (layer.weight.shape[0], k // g, 1)
        assert torch.equal(y, f(x, wq, layer.bias))
        # the composed route: the same graph from the per-channel quantizer on the regrouped weight
        w2 = torch.nn.Parameter(layer.weight.detach().reshape(-1, g).clone())
        q2 = Q.ShiftedUint8WeightPerChannelFloat(w2, bit_width=4).to(DEV)
        wq2, scale2, zp2, _ = q2(w2)
        x2 = x.detach().clone().requires_grad_(True)
        y2 = f(x2, wq2.view(layer.weight.shape), layer.bias.detach())
        y2.float().sum().backward()
        assert torch.equal(y, y2) and torch.equal(x.grad, x2.grad)
        got = (wq.detach(), scale.detach(), zp.detach(), layer.weight.grad)
        want = (wq2.detach(), scale2.detach(), zp2.detach(), w2.grad)
        compare(got, want, layer.weight.detach(), _weight_grad(f, x, wq, layer), g, 4, 'bf16')


def _weight_grad(f, x, wq, layer):
    """the gradient arriving at the quantized weight for loss = sum(layer(x))"""
    wl = wq.detach().clone().requires_grad_(True)
    f(x.detach(), wl, layer.bias.detach()).float().sum().backward()
    return wl.grad


def test_weight_quant_group_with_an_asymmetric_group_wise_layer(fused_calls):
    """inside the block the group-wise layer keeps its own kernels and the per-channel layers the list launch: the bits
    of each layer's own route"""
    import brevitas_amd.quant as Q
    from brevitas_amd import WeightQuantGroup
    from brevitas_amd.nn import QuantLinear
    torch.manual_seed(1)
    model = torch.nn.Sequential(
        QuantLinear(128, 64, weight_quant=Q.Int8WeightPerChannelFloat, device=DEV, dtype=torch.bfloat16),
        QuantLinear(64, 32, weight_quant=functools.partial(Q.ShiftedUint4WeightPerGroupFloat, group_size=32),
                    device=DEV, dtype=torch.bfloat16),
        QuantLinear(32, 16, weight_quant=Q.Int8WeightPerChannelFloat, device=DEV, dtype=torch.bfloat16))
    x = torch.randn(8, 128, device=DEV, dtype=torch.bfloat16)

    def run():
        model.zero_grad(set_to_none=True)
        y = model(x)
        y.float().sum().backward()
        return [y.detach().clone()] + [p.grad.detach().clone() for p in model.parameters()]
    want = run()
    group = WeightQuantGroup(model)
    assert [n for n, _ in group.covered] == ['0.weight_quant', '2.weight_quant']
    assert '1.weight_quant' not in [n for n, _ in group.uncovered]  # no member at all
    n = len(fused_calls)
    with group:
        got = run()
    assert len(fused_calls) == n + 1
    for a, b in zip(got, want):
        assert torch.equal(a, b)


# ---- graph capture --------------------------------------------------------------------------------------------------

def test_step_in_a_graph(fused_calls):
    import brevitas_amd.quant as Q
    from test_gpu_graphs import _capture
    torch.manual_seed(123456)
    w = torch.nn.Parameter((torch.randn(32, 256, device=DEV) * 0.1).to(torch.bfloat16))
    g = torch.randn(32, 256, device=DEV).to(torch.bfloat16)
    q = Q.ShiftedUint4WeightPerGroupFloat(w, group_size=64).to(DEV)

    def one():
        w.grad = None
        y, scale, zp, _ = q(w)
        y.backward(g)
        return y, scale, zp, w.grad

    graph, static = _capture(one)
    assert len(fused_calls) == 4
    with torch.no_grad():
        w.mul_(1.5).add_(0.01)  # new values in the captured input
    graph.replay()
    torch.cuda.synchronize()
    got = [t.clone() for t in static]
    for a, b in zip(got, one()):
        assert torch.equal(a, b)


# ---- guard elements -------------------------------------------------------------------------------------------------

@dtypes
def test_guard_elements_behind_every_output_are_untouched(dn):
    """84 (168) chunks: a ragged last wave load; every output lies in a buffer with 64 sentinel elements behind it"""
    from brevitas_amd import _native as nat
    from brevitas_amd.core.quant import _fused
    shape, g, pad = (7, 96), 32, 64
    w, grad, gscale, gzp = make_weight(shape, g, dn)
    w, grad, gscale, gzp = w.to(DEV).reshape(-1), grad.to(DEV).reshape(-1), gscale.to(DEV), gzp.to(DEV)
    n, groups = w.numel(), w.numel() // g
    desc, thr_div = _fused.group_shifted_call(w, g, 15.0, 0.0, 15.0, False)
    assert nat.group_shifted_supported(desc, w)
    want = nat.group_shifted_fwd(desc, w, 1e-10, thr_div)
    want_dx = nat.group_shifted_bwd(desc, grad, w, want[3], gscale, gzp, 1e-10, thr_div)
    sentinel = 77.0
    bufs = {name: torch.full((size + pad,), sentinel, dtype=DT[dn], device=DEV)
            for name, size in (('y', n), ('scale', groups), ('zp', groups), ('stat', 2 * groups), ('dx', n))}
    args = nat._scale_args(1e-10, thr_div)
    nat._launch(w.device, 'bvq_group_shifted_fwd', None, ctypes.byref(desc), nat.ptr(w), *args, nat.ptr(bufs['y']),
                nat.ptr(bufs['scale']), nat.ptr(bufs['zp']), nat.ptr(bufs['stat']))
    nat._launch(w.device, 'bvq_group_shifted_bwd', None, ctypes.byref(desc), nat.ptr(grad), nat.ptr(w),
                nat.ptr(bufs['stat']), nat.ptr(gscale), nat.ptr(gzp), *args, nat.ptr(bufs['dx']))
    torch.cuda.synchronize()
    for (name, size), ref in zip((('y', n), ('scale', groups), ('zp', groups), ('stat', 2 * groups), ('dx', n)),
                                 tuple(want) + (want_dx,)):
        assert_same_bits(bufs[name][:size], ref.reshape(-1), dn, name)
        assert bool((bufs[name][size:] == sentinel).all()), name
