"""Group-wise weight quantizers on the device: the one-kernel route (csrc/bvq_group_quant.hip) against the reference's
golden vectors, the CPU oracle and the per-channel route on the regrouped weight; the refusals, the layers,
WeightQuantGroup and graph capture.

Bars: y and scale are bit-exact everywhere.  dw is bit-exact except at the first element attaining each group's
statistic, which receives a reduced float32 sum: the group kernel adds a group's terms in another order than the
per-channel kernels, so that element may differ by the roundings derived at `deposit_ulps`.
"""
import functools

import numpy as np
import pytest
import torch

import golden_util as G
from test_group_quant_golden import CASES, case, check_case, first_argmax_positions, run_case, to_np

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
DT = {'f32': torch.float32, 'bf16': torch.bfloat16, 'f16': torch.float16}
MANT = {'f32': 23, 'bf16': 7, 'f16': 10}
MIN_EXP = {'f32': -126, 'bf16': -126, 'f16': -14}
# [out, K], group size: less than one wave load in every dtype; a whole wave per float32 group with a ragged last
# wave; a number of groups that is no multiple of the groups per load; several waves, workgroups and the full depth
# and 27 groups of 64, ragged in every dtype
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
    """counts the launches of the group kernels' forward wrapper"""
    from brevitas_amd import _native as nat
    calls = []
    real = nat.group_quant_fwd

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)
    monkeypatch.setattr(nat, 'group_quant_fwd', counted)
    return calls


def deposit_ulps(dn, g):
    """cap of the difference at a deposit position, in units in the last place of the dtype at the magnitude of the
    values involved.  16-bit: the two float32 sums differ far below a 16-bit ulp, so only a rounding flip of the sum,
    of the quotient and of the final add can occur.  float32: two summation orders of g float32 terms differ by at
    most 2 (g - 1) 2^-24 sum|t|, and sum|t| <= sum|g| / 2 up to rounding."""
    return g + 4 if dn == 'f32' else 4


def ulp(v, dn):
    e = max(int(np.floor(np.log2(v))), MIN_EXP[dn])
    return 2.0 ** (e - MANT[dn])


def make_weight(shape, g, dn, seed=123456):
    gen = torch.Generator().manual_seed(seed)
    w = (torch.randn(shape, generator=gen) * 0.02).to(DT[dn])
    w2 = w.view(-1, g)
    w2[1] = 0.0                              # an all-zero group
    m = (w2[2].abs().max().float() * 1.25).to(w.dtype)
    w2[2, 1], w2[2, g - 2] = -m, m           # a tie across chunks: the first wins
    grad = torch.randn(shape, generator=gen).to(DT[dn])
    gscale = torch.randn(w.numel() // g, generator=gen).to(DT[dn])
    return w, grad, gscale


def set_clamp(q, ste):
    from brevitas_amd.core.function_wrapper import TensorClamp, TensorClampSte
    q.int_quant.tensor_clamp_impl = TensorClampSte() if ste else TensorClamp()
    return q


def step(q, w, grad, gscale=None):
    """grad None: y receives no gradient, the loss uses the returned scale alone"""
    w.grad = None
    y, scale, zp, _ = q(w)
    if gscale is None:
        y.backward(grad.view(y.shape))
    elif grad is None:
        scale.backward(gscale.view(scale.shape))
    else:
        torch.autograd.backward([y, scale], [grad.view(y.shape), gscale.view(scale.shape)])
    return y.detach(), scale.detach(), w.grad.detach().clone()


def grouped_step(w0, g, bits, ste, grad, gscale=None):
    import brevitas_amd.quant as Q
    w = torch.nn.Parameter(w0.clone())
    q = set_clamp(Q.Int8WeightPerGroupFloat(w, group_size=g, bit_width=bits).to(w.device), ste)
    return step(q, w, grad, gscale)


def per_channel_step(w0, g, bits, ste, grad, gscale=None):
    """the parent's route: the per-channel quantizer on the regrouped weight"""
    import brevitas_amd.quant as Q
    w = torch.nn.Parameter(w0.detach().contiguous().view(-1, g).clone())
    q = set_clamp(Q.Int8WeightPerChannelFloat(w, bit_width=bits).to(w.device), ste)
    return step(q, w, None if grad is None else grad.contiguous().view(-1, g), gscale)


def assert_same_bits(a, b, dn, what):
    assert G.same_bits(to_np(a).reshape(-1), to_np(b).reshape(-1), dn), what


def assert_dw(got, want, w, grad, g, bits, dn, skip_groups=()):
    """bit-equal away from the first attaining element of each group; there, within deposit_ulps -> worst ulps seen"""
    gotf = got.float().cpu().numpy().reshape(-1).astype(np.float64)
    wantf = want.float().cpu().numpy().reshape(-1).astype(np.float64)
    gf = grad.float().cpu().numpy().reshape(-1).astype(np.float64)
    bad = np.nonzero(to_np(got).reshape(-1) != to_np(want).reshape(-1))[0]
    bad = [int(i) for i in bad if i // g not in skip_groups and not (np.isnan(gotf[i]) and np.isnan(wantf[i]))]
    allowed = first_argmax_positions(w, g)
    assert set(bad) <= allowed, sorted(set(bad) - allowed)[:8]
    thr = 2.0 ** (bits - 1) - 1
    worst = 0.0
    for i in bad:
        grp = i // g
        mag = max(abs(gotf[i]), abs(wantf[i]), abs(wantf[i] - gf[i]), np.abs(gf[grp * g:(grp + 1) * g]).sum() / thr)
        assert mag > 0, (i, gotf[i], wantf[i])
        n = abs(gotf[i] - wantf[i]) / ulp(mag, dn)
        assert n <= deposit_ulps(dn, g), (i, gotf[i], wantf[i], n)
        worst = max(worst, n)
    return worst


def zero_off_the_deposits(dw, dw_ref, scale_ref, w, g):
    """dw of two steps in which y received no gradient (this file's and test_gpu_group_mse.py's): zero by value away
    from the first attaining element of each group, or NaN where the other route's is NaN too
    -> (dw, dw_ref, the groups to leave out of the deposit bar), the two with "+ 0.0", which makes -0 and +0 one: the
    sign of such a zero is nobody's contract, and assert_dw compares bits.

    An expected difference, as the kernels stand: a group whose scale is zero (float16, where min_val = 1e-10
    underflows: the all-zero group) or not finite.  The one-launch backward always runs, on zeros for y's gradient, and
    gives NaN over the whole group; on a route put together from several autograd nodes the quantizer's backward is
    never entered when y is unused, and the group gets zeros and its deposit.  Such groups may hold NaN and are left out
    of the deposit bar; every other group is held to zero."""
    off = torch.ones(w.numel(), dtype=torch.bool)
    off[sorted(first_argmax_positions(w, g))] = False
    sc = scale_ref.reshape(-1).float().cpu()
    degenerate = ~(sc.isfinite() & (sc != 0))
    got, ref = dw.reshape(-1).float().cpu(), dw_ref.reshape(-1).float().cpu()
    ok = (got == 0) | (got.isnan() & (ref.isnan() | degenerate.repeat_interleave(g)))
    assert bool(ok[off].all()), torch.nonzero(~ok & off).reshape(-1)[:8].tolist()
    return dw + 0.0, dw_ref + 0.0, set(torch.nonzero(degenerate).reshape(-1).tolist())


# ---- golden ---------------------------------------------------------------------------------------------------------

@case
@pytest.mark.parametrize('fused', [True, False], ids=['fused', 'generic'])
def test_golden(c, fused, fused_calls, cpu_scalar_semantics, monkeypatch):
    import brevitas_amd.config as config
    monkeypatch.setattr(config, 'FUSED_PATHS', fused)
    check_case(c, *run_case(c, DEV))
    assert len(fused_calls) == (1 if fused else 0)


# ---- oracle ---------------------------------------------------------------------------------------------------------

@shapes
@dtypes
def test_forward_matches_the_oracle(shape, g, dn, fused_calls):
    import oracle as O
    w, grad, _ = make_weight(shape, g, dn)
    y, scale, _ = grouped_step(w.to(DEV), g, 4, True, grad.to(DEV))
    assert len(fused_calls) == 1
    xn, code = O.from_torch(w.reshape(-1))
    gn, _ = O.from_torch(grad.reshape(-1))
    d = O.make_desc(1, w.numel() // g, g, code, code, code, O.F32, scale_per_channel=True, qmin=-7.0, qmax=7.0,
                    clamp_ste=True)
    y_o, _, scale_o, _, _ = O.step_stats_scaled(d, xn, gn, 1e-10, 7.0)
    assert G.same_bits(O.from_torch(y.reshape(-1))[0], y_o, dn)
    assert G.same_bits(O.from_torch(scale.reshape(-1))[0], scale_o, dn)
    assert tuple(scale.shape) == (shape[0], shape[1] // g, 1)


# ---- device against device ------------------------------------------------------------------------------------------

@shapes
@dtypes
@pytest.mark.parametrize('bits', [4, 8])
@pytest.mark.parametrize('ste', [True, False], ids=['clamp_ste', 'clamp'])
def test_fused_route_against_the_per_channel_route(shape, g, dn, bits, ste, fused_calls):
    w, grad, _ = make_weight(shape, g, dn)
    w, grad = w.to(DEV), grad.to(DEV)
    y, scale, dw = grouped_step(w, g, bits, ste, grad)
    assert len(fused_calls) == 1
    y_r, scale_r, dw_r = per_channel_step(w, g, bits, ste, grad)
    assert_same_bits(y, y_r, dn, 'y')
    assert_same_bits(scale, scale_r, dn, 'scale')
    worst = assert_dw(dw, dw_r, w, grad, g, bits, dn)
    print('GROUP_QUANT_DEPOSIT_ULPS %s g=%d bits=%d ste=%d worst=%.3f' % (dn, g, bits, ste, worst))


@dtypes
def test_gradient_through_the_scale(dn, fused_calls):
    """the loss uses the returned scale too: its gradient joins the group's scale gradient before the deposit"""
    shape, g = (7, 96), 32
    w, grad, gscale = make_weight(shape, g, dn)
    w, grad, gscale = w.to(DEV), grad.to(DEV), gscale.to(DEV)
    y, scale, dw = grouped_step(w, g, 4, True, grad, gscale)
    assert len(fused_calls) == 1
    y_r, scale_r, dw_r = per_channel_step(w, g, 4, True, grad, gscale)
    assert_same_bits(y, y_r, dn, 'y')
    assert_same_bits(scale, scale_r, dn, 'scale')
    assert_dw(dw, dw_r, w, grad, g, 4, dn)
    _, _, dw_plain = grouped_step(w, g, 4, True, grad)
    assert not torch.equal(dw, dw_plain)  # the scale's gradient arrived
    # the scale alone: y receives no gradient, the kernel takes zeros for it
    _, _, dw_s = grouped_step(w, g, 4, True, None, gscale)
    assert len(fused_calls) == 3
    _, scale_sr, dw_sr = per_channel_step(w, g, 4, True, None, gscale)
    dw_s0, dw_sr0, skip = zero_off_the_deposits(dw_s, dw_sr, scale_sr, w, g)
    assert_dw(dw_s0, dw_sr0, w, torch.zeros_like(grad), g, 4, dn, skip_groups=skip)
    assert bool(dw_s.float().nan_to_num().any())  # the scale's gradient arrived


@dtypes
def test_a_group_with_a_nan(dn, fused_calls):
    shape, g = (7, 96), 32
    w, grad, _ = make_weight(shape, g, dn)
    w.view(-1, g)[5, 9] = float('nan')
    w, grad = w.to(DEV), grad.to(DEV)
    y, scale, dw = grouped_step(w, g, 8, True, grad)
    assert len(fused_calls) == 1
    y_r, scale_r, dw_r = per_channel_step(w, g, 8, True, grad)
    assert_same_bits(y, y_r, dn, 'y')          # (every NaN equals every NaN)
    assert_same_bits(scale, scale_r, dn, 'scale')
    assert bool(torch.isnan(scale.reshape(-1)[5])) and bool(torch.isnan(y.view(-1, g)[5]).all())
    assert int(torch.isnan(scale).sum()) == 1
    assert_dw(dw, dw_r, w, grad, g, 8, dn, skip_groups=(5,))


def test_two_runs_give_the_same_bits(fused_calls):
    shape, g = (64, 4096), 128
    w, grad, gscale = make_weight(shape, g, 'bf16')
    w, grad, gscale = w.to(DEV), grad.to(DEV), gscale.to(DEV)
    a = grouped_step(w, g, 4, True, grad, gscale)
    b = grouped_step(w, g, 4, True, grad, gscale)
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
    q = Q.Int8WeightPerGroupFloat(p, group_size=g, bit_width=bits).to(DEV)
    y, scale, dw = step(q, p, grad)
    assert len(fused_calls) == 0
    y_r, scale_r, dw_r = per_channel_step(w, g, bits, True, grad)
    assert tuple(y.shape) == tuple(w.shape) and tuple(scale.shape) == (w.shape[0], w.shape[1] // g, 1)
    assert_same_bits(y.contiguous(), y_r, dn, 'y')
    assert_same_bits(scale, scale_r, dn, 'scale')
    assert_dw(dw.contiguous(), dw_r, w.contiguous(), grad.contiguous(), g, bits, dn)


# ---- layers ---------------------------------------------------------------------------------------------------------

def test_layers_forward_backward(fused_calls):
    import brevitas_amd.quant as Q
    from brevitas_amd.nn import QuantConv2d, QuantLinear
    torch.manual_seed(0)
    lin = QuantLinear(256, 64, weight_quant=functools.partial(Q.Int4WeightPerGroupFloat, group_size=64),
                      device=DEV, dtype=torch.bfloat16)
    conv = QuantConv2d(16, 8, 3, padding=1, weight_quant=functools.partial(Q.Int4WeightPerGroupFloat, group_size=16),
                       device=DEV, dtype=torch.bfloat16)
    for layer, x, f in ((lin, torch.randn(4, 256, device=DEV, dtype=torch.bfloat16), torch.nn.functional.linear),
                        (conv, torch.randn(2, 16, 8, 8, device=DEV, dtype=torch.bfloat16),
                         functools.partial(torch.nn.functional.conv2d, padding=1))):
        n = len(fused_calls)
        x.requires_grad_(True)
        y = layer(x)
        y.float().sum().backward()
        assert len(fused_calls) == n + 1
        wq, scale, _, _ = layer.quant_weight()
        k = layer.weight.numel() // layer.weight.shape[0]
        assert tuple(scale.shape) == (layer.weight.shape[0], k // layer.weight_quant.group_size, 1)
        assert torch.equal(y, f(x, wq, layer.bias))
        assert layer.weight.grad is not None and bool(torch.isfinite(layer.weight.grad.float()).all())
        assert float(layer.weight.grad.float().abs().max()) > 0 and x.grad is not None


def test_weight_quant_group_with_a_group_wise_layer(fused_calls):
    """inside the block the group-wise layer keeps its own kernels and the per-channel layers the list launch: the bits
    of each layer's own route"""
    import brevitas_amd.quant as Q
    from brevitas_amd import WeightQuantGroup
    from brevitas_amd.nn import QuantLinear
    torch.manual_seed(1)
    model = torch.nn.Sequential(
        QuantLinear(128, 64, weight_quant=Q.Int8WeightPerChannelFloat, device=DEV, dtype=torch.bfloat16),
        QuantLinear(64, 32, weight_quant=functools.partial(Q.Int4WeightPerGroupFloat, group_size=32), device=DEV,
                    dtype=torch.bfloat16),
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
    q = Q.Int4WeightPerGroupFloat(w, group_size=64).to(DEV)

    def one():
        w.grad = None
        y, scale, _, _ = q(w)
        y.backward(g)
        return y, scale, w.grad

    graph, (y_s, scale_s, dw_s) = _capture(one)
    assert len(fused_calls) == 4
    with torch.no_grad():
        w.mul_(1.5).add_(0.01)  # new values in the captured input
    graph.replay()
    torch.cuda.synchronize()
    got = (y_s.clone(), scale_s.clone(), dw_s.clone())
    y, scale, dw = one()
    assert torch.equal(got[0], y) and torch.equal(got[1], scale) and torch.equal(got[2], dw)
