"""Group-wise clip search (GroupwiseMSEIntQuant, Int*WeightPerGroupFloatMSE), what needs no device: the composed route
on CPU tensors against a float64 restatement of the semantics ("Group-wise clip search"), the reduction to
the plain group-wise quantizer, special groups, validation, the layers, and the host-side refusals of the C ABI.

The restatement (`restate`) is written here on torch CPU ops and shares nothing with the package: abs-max, threshold,
scale and the quantized values with a rounding to the weight's dtype after every step, the errors in float64.

Bar of the index (`check_index`): with m the float64 minimum over the candidates and e the float64 error at the chosen
candidate, e <= m (1 + 2 (g + 4) 2^-24): the search compares float32 sums of g non-negative terms, each term with at
most 3 roundings and a sum with (g - 1) more, and two such sums are compared.  On top of that at most 1 % of the groups
may choose another candidate than the float64 first minimum at all (float32 sums differ from float64 on exact ties
only).
"""
import ctypes
import functools

import pytest
import torch

DT = {'f32': torch.float32, 'bf16': torch.bfloat16, 'f16': torch.float16}
SEARCHES = [(10, .01), (20, .025), (64, .0125)]   # (candidates, step)


def ratios_of(n, step):
    return [1.0 - i * step for i in range(n)]


def make_groups(groups, g, dn, seed=123456):
    """random normal groups with a 6x outlier in every third group"""
    gen = torch.Generator().manual_seed(seed + g)
    x = torch.randn(groups, g, generator=gen)
    x[::3, 0] *= 6
    return x.to(DT[dn])


def restate(xg, ratios, bits, min_val=1e-10):
    """-> (float64 errors [n, groups], scales [n, groups] and y [n, groups, g] as float32 values of xg's dtype)"""
    T = xg.dtype

    def rnd(v):
        return v.to(T).float()
    qmax = float(2 ** (bits - 1) - 1)
    x = xg.float()
    a = x.abs().max(dim=1, keepdim=True).values
    lo = rnd(torch.tensor(min_val, dtype=torch.float32))
    errs, scales, ys = [], [], []
    for r in ratios:
        t = rnd(a * torch.tensor(r, dtype=torch.float32))
        thr = torch.where(t < lo, lo, t)                       # NaN passes
        s = rnd(thr / qmax)
        q = torch.round(rnd(x / s))
        q = torch.where(q > qmax, torch.tensor(qmax), q)
        q = torch.where(q < -qmax, torch.tensor(-qmax), q)
        y = rnd(q * s)
        errs.append(((y.double() - x.double()) ** 2).sum(dim=1))
        scales.append(s.reshape(-1))
        ys.append(y)
    return torch.stack(errs), torch.stack(scales), torch.stack(ys)


def first_minimum(errs):
    """the semantics' rule in float64: first candidate strictly below every earlier one"""
    best, idx = errs[0].clone(), torch.zeros(errs.shape[1], dtype=torch.int64)
    for i in range(1, errs.shape[0]):
        better = errs[i] < best
        idx = torch.where(better, torch.full_like(idx, i), idx)
        best = torch.where(better, errs[i], best)
    return idx, best


def check_index(idx, errs, g, skip=()):
    """the bar of the module docstring -> fraction of groups that chose a candidate below their abs-max"""
    idx = idx.reshape(-1).long().cpu()
    want, m = first_minimum(errs)
    e = errs.gather(0, idx.reshape(1, -1)).reshape(-1)
    nan = torch.isnan(errs).any(dim=0)   # a NaN or Inf group (float16: a group of zeros too, its scale is 0): candidate 0
    assert bool((idx[nan] == 0).all())
    keep = ~nan
    for s in skip:
        keep[s] = False
    bound = m * (1.0 + 2.0 * (g + 4) * 2.0 ** -24)
    bad = (keep & ~(e <= bound)).nonzero().reshape(-1)
    assert bad.numel() == 0, (bad[:8].tolist(), e[bad[:8]].tolist(), m[bad[:8]].tolist())
    assert bool((e[keep] <= errs[0][keep] * (1.0 + 2.0 * (g + 4) * 2.0 ** -24)).all())  # never worse than the abs-max
    differ = int((keep & (idx != want)).sum())
    assert differ <= 0.01 * idx.numel(), (differ, idx.numel())
    return float((idx[keep] > 0).float().mean())


def quantizer(w, g, bits, ratios):
    import brevitas_amd.quant as Q
    return Q.Int8WeightPerGroupFloatMSE(w, group_size=g, bit_width=bits, mse_ratios=ratios)


def to_bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def same_bits(a, b):
    """equal bit patterns, every NaN equal to every NaN"""
    a, b = a.detach().cpu(), b.detach().cpu()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return bool(((to_bits(a) == to_bits(b)) | (torch.isnan(a) & torch.isnan(b))).all())


# ---- known answer ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dn', ['f32', 'bf16', 'f16'])
def test_known_answer(dn):
    """One group of 16 at 3 bits (codes -3 .. 3): x = [6, 1, 1, ..., 1], ratios [1, 0.5, 0.5, 0.25], gradient of ones.
      ratio 1    : t = 6,   s = 2  : 6 -> 3 * 2 = 6 (error 0), every 1 -> round-half-even(0.5) = 0 (error 1): e = 15
      ratio 0.5  : t = 3,   s = 1  : 6 -> clamp(6) = 3 (error 9), every 1 -> 1 (error 0):                    e = 9
      ratio 0.5  : a tie with the candidate before: the earlier one stays
      ratio 0.25 : t = 1.5, s = 0.5: 6 -> 3 * 0.5 = 1.5 (error 20.25), every 1 -> 2 * 0.5 (error 0):         e = 20.25
    so k = 1, scale = 1, y = [3, 1, ..., 1].  Backward at s = 1 with the straight-through clamp: dx = g = 1 everywhere; the
    scale gradient is g * q - g * x / s = 3 - 6 = -3 from the clamped element and 0 elsewhere; dt = -3 / 3 = -1,
    da = dt * 0.5 = -0.5, added to the first element attaining the abs-max: dx[0] = 1 - 0.5 = 0.5."""
    x = torch.ones(1, 16)
    x[0, 0] = 6.0
    w = torch.nn.Parameter(x.to(DT[dn]))
    q = quantizer(w, 16, 3, [1.0, 0.5, 0.5, 0.25])
    y, scale, zp, bw = q(w)
    y.backward(torch.ones_like(y))
    assert q.last_mse_index.tolist() == [[1]] and q.last_mse_index.dtype == torch.uint8
    assert y.dtype == DT[dn] and y.float().tolist() == [[3.0] + [1.0] * 15]
    assert tuple(scale.shape) == (1, 1, 1) and float(scale.detach()) == 1.0 and float(zp) == 0.0 and float(bw) == 3.0
    assert w.grad.float().tolist() == [[0.5] + [1.0] * 15]
    errs, _, _ = restate(x.to(DT[dn]), q.mse_ratios, 3)
    assert errs.reshape(-1).tolist() == [15.0, 9.0, 9.0, 20.25]


# ---- the index against the float64 restatement ----------------------------------------------------------------------

@pytest.mark.parametrize('n,step', SEARCHES, ids=['n10', 'n20', 'n64'])
@pytest.mark.parametrize('bits', [3, 4])
@pytest.mark.parametrize('g', [16, 32, 128, 256])
def test_index_against_float64(g, bits, n, step):
    groups = 384
    ratios = ratios_of(n, step)
    xg = make_groups(groups, g, 'f32')
    w = torch.nn.Parameter(xg.reshape(groups // 4, 4 * g).clone())
    q = quantizer(w, g, bits, ratios)
    y, scale, _, _ = q(w)
    idx = q.last_mse_index
    assert tuple(idx.shape) == (groups // 4, 4) and idx.dtype == torch.uint8
    errs, scales, ys = restate(xg, ratios, bits)
    chose = check_index(idx, errs, g)
    print('GROUP_MSE_HOST g=%d bits=%d n=%d chose k>0: %.3f' % (g, bits, n, chose))
    if bits == 4 and g >= 32:
        assert chose > 0.5   # the search matters: over half the groups clip below their abs-max
    # y and scale are the restatement's values at the chosen candidate
    k = idx.reshape(-1).long()
    assert same_bits(scale.reshape(-1), scales.gather(0, k.reshape(1, -1)).reshape(-1))
    assert same_bits(y.reshape(groups, g), ys[k, torch.arange(groups)])


@pytest.mark.parametrize('dn', ['bf16', 'f16'])
def test_index_against_float64_16_bit(dn):
    g, bits, groups = 32, 4, 384
    ratios = ratios_of(20, .025)
    xg = make_groups(groups, g, dn)
    w = torch.nn.Parameter(xg.reshape(groups // 4, 4 * g).clone())
    q = quantizer(w, g, bits, ratios)
    y, scale, _, _ = q(w)
    errs, scales, ys = restate(xg, ratios, bits)
    assert check_index(q.last_mse_index, errs, g) > 0.5
    k = q.last_mse_index.reshape(-1).long()
    assert same_bits(scale.reshape(-1).float(), scales.gather(0, k.reshape(1, -1)).reshape(-1))
    assert same_bits(y.reshape(groups, g).float(), ys[k, torch.arange(groups)])


def test_the_two_steps_are_callable_on_their_own():
    """mse_index is the search alone; quantize_at_index quantizes at ANY given candidates, differentiably"""
    g, groups = 32, 24
    xg = make_groups(groups, g, 'f32')
    w = torch.nn.Parameter(xg.reshape(6, 4 * g).clone())
    q = quantizer(w, g, 4, ratios_of(20, .025))
    y, scale, _, _ = q(w)
    idx = q.mse_index(w)
    assert idx.dtype == torch.uint8 and torch.equal(idx.reshape(6, 4), q.last_mse_index)
    y2, scale2 = q.quantize_at_index(w, idx)
    assert same_bits(y2, y) and same_bits(scale2, scale)
    other = torch.full_like(idx, 7)
    y3, scale3 = q.quantize_at_index(w, other)
    errs, scales, ys = restate(xg, q.mse_ratios, 4)
    assert same_bits(scale3.reshape(-1), scales[7]) and same_bits(y3.reshape(groups, g), ys[7])
    y3.sum().backward()
    assert w.grad is not None and bool(torch.isfinite(w.grad).all())


# ---- reduction to the plain quantizer -------------------------------------------------------------------------------

def _step(q, w, grad, gscale):
    w.grad = None
    y, scale, _, _ = q(w)
    torch.autograd.backward([y, scale], [grad, gscale.reshape(scale.shape)])
    return y.detach(), scale.detach(), w.grad.detach().clone()


@pytest.mark.parametrize('dn', ['f32', 'bf16', 'f16'])
def test_one_ratio_is_the_plain_group_wise_quantizer(dn):
    import brevitas_amd.quant as Q
    g, groups = 32, 48
    xg = make_groups(groups, g, dn) * 0.02
    xg[1] = 0.0
    gen = torch.Generator().manual_seed(5)
    grad = torch.randn(12, 4 * g, generator=gen).to(DT[dn])
    gscale = torch.randn(groups, generator=gen).to(DT[dn])
    w = torch.nn.Parameter(xg.reshape(12, 4 * g).clone())
    plain = _step(Q.Int4WeightPerGroupFloat(w, group_size=g), w, grad, gscale)
    q = Q.Int4WeightPerGroupFloatMSE(w, group_size=g, mse_ratios=[1.0])
    mse = _step(q, w, grad, gscale)
    assert int(q.last_mse_index.max()) == 0
    for a, b, what in zip(mse, plain, ('y', 'scale', 'dw')):
        assert same_bits(a, b), what
    also = _step(Q.Int4WeightPerGroupFloatMSE(w, group_size=g, mse_iters=1), w, grad, gscale)
    for a, b, what in zip(also, plain, ('y', 'scale', 'dw')):
        assert same_bits(a, b), what


# ---- special groups -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dn', ['f32', 'bf16'])
def test_zero_nan_and_inf_groups(dn):
    """a group of zeros, one with a NaN and one with an Inf keep candidate 0 and the plain quantizer's bits; the groups
    around them search as usual"""
    import brevitas_amd.quant as Q
    g, groups = 16, 12
    xg = make_groups(groups, g, dn)
    xg[1] = 0.0
    xg[4, 3] = float('nan')
    xg[7, 5] = float('-inf')
    w = torch.nn.Parameter(xg.reshape(3, 4 * g).clone())
    q = Q.Int4WeightPerGroupFloatMSE(w, group_size=g)
    y, scale, _, _ = q(w)
    idx = q.last_mse_index.reshape(-1)
    assert idx[[1, 4, 7]].tolist() == [0, 0, 0]
    y_p, scale_p, _, _ = Q.Int4WeightPerGroupFloat(w, group_size=g)(w)
    for grp in (1, 4, 7):
        assert same_bits(y.reshape(groups, g)[grp], y_p.reshape(groups, g)[grp]), grp
        assert same_bits(scale.reshape(-1)[grp], scale_p.reshape(-1)[grp]), grp
    assert bool(torch.isnan(y.reshape(groups, g)[4]).all()) and bool(torch.isnan(scale.reshape(-1)[4]))
    assert float(y.reshape(groups, g)[1].abs().max()) == 0.0
    errs, _, _ = restate(xg, q.mse_ratios, 4)
    assert check_index(idx, errs, g, skip=(4, 7)) > 0.5


# ---- validation, state ----------------------------------------------------------------------------------------------

def test_ratio_validation():
    import brevitas_amd.quant as Q
    w = torch.nn.Parameter(torch.randn(4, 64))
    for bad, match in (([], 'empty'), ([0.9, 1.0], 'must be 1.0'), ([1.0, 0.0], r'\(0, 1\]'), ([1.0, 1.5], r'\(0, 1\]'),
                       ([1.0, -0.5], r'\(0, 1\]'), ([1.0, float('nan')], r'\(0, 1\]'),
                       ([1.0, float('inf')], r'\(0, 1\]'), (0.5, 'sequence')):
        with pytest.raises(ValueError, match=match):
            Q.Int4WeightPerGroupFloatMSE(w, group_size=32, mse_ratios=bad)
    with pytest.raises(ValueError, match='mse_iters'):
        Q.Int4WeightPerGroupFloatMSE(w, group_size=32, mse_iters=0)
    with pytest.raises(ValueError, match=r'\(0, 1\]'):
        Q.Int4WeightPerGroupFloatMSE(w, group_size=32, mse_iters=41)       # 1 - 40 * 0.025 = 0
    with pytest.raises(ValueError, match='no whole groups'):
        Q.Int4WeightPerGroupFloatMSE(w, group_size=48)
    q = Q.Int8WeightPerGroupFloatMSE(w, group_size=32)
    assert q.mse_ratios == tuple(1.0 - i * 0.025 for i in range(20)) and q.group_size == 32
    assert float(q.msb_clamp_bit_width_impl()) == 8.0
    assert float(Q.Int4WeightPerGroupFloatMSE(w, group_size=32).msb_clamp_bit_width_impl()) == 4.0
    assert 'Int8WeightPerGroupFloatMSE' in Q.__all__ and 'Int4WeightPerGroupFloatMSE' in Q.__all__


def test_no_new_state():
    import copy
    import brevitas_amd.quant as Q
    from brevitas_amd.core.quant import GroupwiseMSEIntQuant, GroupwiseRescalingIntQuant
    w = torch.nn.Parameter(torch.randn(4, 64))
    q = Q.Int4WeightPerGroupFloatMSE(w, group_size=32)
    p = Q.Int4WeightPerGroupFloat(w, group_size=32)
    assert isinstance(q, GroupwiseMSEIntQuant) and isinstance(q, GroupwiseRescalingIntQuant)
    assert q.last_mse_index is None
    q(w)
    assert list(q.state_dict().keys()) == list(p.state_dict().keys())
    assert [n for n, _ in q.named_parameters()] == [n for n, _ in p.named_parameters()]
    assert [n for n, _ in q.named_buffers()] == [n for n, _ in p.named_buffers()]
    q2 = copy.deepcopy(q)
    assert q2.mse_ratios == q.mse_ratios


# ---- layers, WeightQuantGroup ---------------------------------------------------------------------------------------

def test_layers_and_weight_quant_group_on_the_cpu():
    import brevitas_amd.quant as Q
    from brevitas_amd import WeightQuantGroup
    from brevitas_amd.core.quant import GroupwiseMSEIntQuant
    from brevitas_amd.nn import QuantConv2d, QuantLinear
    torch.manual_seed(0)
    lin = QuantLinear(128, 16, weight_quant=functools.partial(Q.Int4WeightPerGroupFloatMSE, group_size=64))
    conv = QuantConv2d(16, 4, 3, padding=1, weight_quant=functools.partial(Q.Int4WeightPerGroupFloatMSE, group_size=16,
                                                                          mse_iters=10, mse_step=0.05))
    for layer, x, f in ((lin, torch.randn(4, 128), torch.nn.functional.linear),
                        (conv, torch.randn(2, 16, 6, 6), functools.partial(torch.nn.functional.conv2d, padding=1))):
        assert isinstance(layer.weight_quant, GroupwiseMSEIntQuant)
        x.requires_grad_(True)
        y = layer(x)
        y.sum().backward()
        wq, scale, _, _ = layer.quant_weight()
        k = layer.weight.numel() // layer.weight.shape[0]
        groups = k // layer.weight_quant.group_size
        assert tuple(scale.shape) == (layer.weight.shape[0], groups, 1)
        assert tuple(layer.weight_quant.last_mse_index.shape) == (layer.weight.shape[0], groups)
        assert int(layer.weight_quant.last_mse_index.max()) > 0
        assert torch.equal(y, f(x, wq, layer.bias))
        assert layer.weight.grad is not None and bool(torch.isfinite(layer.weight.grad).all()) and x.grad is not None
    model = torch.nn.Sequential(QuantLinear(128, 64, weight_quant=Q.Int8WeightPerChannelFloat), lin)
    group = WeightQuantGroup(model)
    members = [n for n, _ in group.covered] + [n for n, _ in group.uncovered]
    assert members == ['0.weight_quant']   # the clip-search quantizer is no member: it keeps its own route


# ---- the C ABI's refusals, before any device is touched -------------------------------------------------------------

def test_abi_refusals():
    from brevitas_amd import _native as nat
    lib = nat.lib
    assert {'bvq_group_mse_supported', 'bvq_group_mse_fwd', 'bvq_group_mse_bwd'} <= set(nat.EXPORTS)
    p = ctypes.c_void_p(4096)          # never dereferenced: every call below is refused first
    off = ctypes.c_void_p(4098)
    one = nat.mse_ratio_table([1.0, 0.9])
    tab = ctypes.addressof(one)

    def desc(g=32, dt=nat.BF16, rm=nat.ROUND, outer=1, out_kind=nat.OUT_DEQUANT, pre=nat.PRE_NONE, ct=None):
        return nat.QuantDesc(outer, 8, g, dt, dt if ct is None else ct, dt, nat.F32, 1, 0, -7.0, 7.0, rm, 0, 1, out_kind,
                             pre)

    def fwd(d, x=p, table=tab, n=2, y=p):
        return lib.bvq_group_mse_fwd(ctypes.byref(d), x, table, n, 1e-10, 1, 7.0, y, p, p, p, None)

    def bwd(d, g=p, table=tab, n=2, idx=p):
        return lib.bvq_group_mse_bwd(ctypes.byref(d), g, p, p, idx, None, table, n, 1e-10, 1, 7.0, p, None)
    ok = desc()
    assert lib.bvq_group_mse_supported(ctypes.byref(ok), p, 20) == 1
    assert lib.bvq_group_mse_supported(ctypes.byref(ok), p, 1) == 1 and lib.bvq_group_mse_supported(ctypes.byref(ok), p, 64) == 1
    assert lib.bvq_group_mse_supported(None, p, 20) == 0
    assert lib.bvq_group_mse_supported(ctypes.byref(ok), None, 20) == 0
    assert lib.bvq_group_mse_supported(ctypes.byref(ok), off, 20) == 0
    for n in (0, -1, 65):
        assert lib.bvq_group_mse_supported(ctypes.byref(ok), p, n) == 0
        assert fwd(ok, n=n) == -2 and 'candidate ratios' in nat.last_error()
        assert bwd(ok, n=n) == -2 and 'candidate ratios' in nat.last_error()
    for bad in (desc(g=48), desc(rm=nat.FLOOR), desc(outer=2), desc(out_kind=nat.OUT_INT), desc(pre=nat.PRE_RELU),
                desc(dt=nat.F32, ct=nat.F32, g=8)):
        assert lib.bvq_group_mse_supported(ctypes.byref(bad), p, 20) == 0
        assert fwd(bad) == -2 and nat.last_error()
        assert bwd(bad) == -2 and nat.last_error()
    assert lib.bvq_group_mse_fwd(None, p, tab, 2, 1e-10, 1, 7.0, p, p, p, p, None) == -1
    assert lib.bvq_group_mse_bwd(None, p, p, p, p, None, tab, 2, 1e-10, 1, 7.0, p, None) == -1
    assert fwd(ok, x=None) == -1 and 'null' in nat.last_error()
    assert fwd(ok, table=None) == -1 and 'null' in nat.last_error()
    assert bwd(ok, idx=None) == -1 and 'null' in nat.last_error()
    assert bwd(ok, table=None) == -1 and 'null' in nat.last_error()
    assert fwd(ok, x=off) == -2 and '16-byte' in nat.last_error()
    assert fwd(ok, y=off) == -2 and '16-byte' in nat.last_error()
    assert bwd(ok, g=off) == -2 and '16-byte' in nat.last_error()
    for ratios, text in (([0.9, 1.0], 'ratio 0'), ([1.0, 0.0], 'ratio 1'), ([1.0, 1.25], 'ratio 1'),
                         ([1.0, -0.5], 'ratio 1'), ([1.0, float('nan')], 'ratio 1'), ([1.0, float('inf')], 'ratio 1')):
        t = nat.mse_ratio_table(ratios)
        assert fwd(ok, table=ctypes.addressof(t)) == -2 and text in nat.last_error(), ratios
        assert bwd(ok, table=ctypes.addressof(t)) == -2 and text in nat.last_error(), ratios
