"""Group-wise clip search on the device: the one-launch kernels (csrc/bvq_group_mse.hip) against the float64 restatement
of test_group_mse_host.py (the chosen candidates) and against the composed route fed the kernel's candidates (every
other bit); the reduction to the plain group-wise kernels, special groups, refusals, layers, graph capture and the
forced non-temporal build.

Bars.  idx: `check_index` of test_group_mse_host.py (its docstring derives it).  Given the kernel's idx, y, scale and
stat are bit-equal to the composed route.  dw is bit-equal except at the first element attaining each group's abs-max,
which receives a reduced float32 sum: the kernel adds a group's terms in another order than the per-channel kernels of
the composed route, so that element may differ by the roundings derived at `deposit_ulps` (the allowance of
test_gpu_group_quant.py, restated; the ratio only shrinks the deposited value).
"""
import functools

import numpy as np
import pytest
import torch

from test_group_mse_host import check_index, make_groups, ratios_of, restate, same_bits
from test_gpu_group_quant import zero_off_the_deposits
from test_gpu_group_walk import use_nt0  # noqa: F401  (fixture: the forced-NT build of the library)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
DT = {'f32': torch.float32, 'bf16': torch.bfloat16, 'f16': torch.float16}
ITEMSIZE = {'f32': 4, 'bf16': 2, 'f16': 2}
MANT = {'f32': 23, 'bf16': 7, 'f16': 10}
MIN_EXP = {'f32': -126, 'bf16': -126, 'f16': -14}
LANES, WAVES, FWD_DEPTH, BWD_DEPTH = 64, 4, 4, 2   # the walk's geometry (test_group_walk_host.py holds it to the sources)
RATIOS = ratios_of(20, .025)
dtypes = pytest.mark.parametrize('dn', ['f32', 'bf16', 'f16'])
sizes = pytest.mark.parametrize('g', [16, 32, 64, 128, 256])


@pytest.fixture
def fused_calls(monkeypatch):
    """counts the launches of the clip-search kernels' wrappers: {'fwd': n, 'bwd': n}"""
    from brevitas_amd import _native as nat
    calls = {'fwd': 0, 'bwd': 0}

    def count(name, key):
        real = getattr(nat, name)

        def counted(*a, **k):
            calls[key] += 1
            return real(*a, **k)
        monkeypatch.setattr(nat, name, counted)
    count('group_mse_fwd', 'fwd')
    count('group_mse_bwd', 'bwd')
    return calls


def shapes_of(dn, g):
    """[out, K] around every boundary of the walk for this L: a tensor that ends inside a wave load (3 rows of 5 groups),
    one workgroup's window of the forward minus and plus a group, the backward's window plus a group"""
    per_load = LANES // (g * ITEMSIZE[dn] // 16)
    fwd, bwd = per_load * FWD_DEPTH * WAVES, per_load * BWD_DEPTH * WAVES
    return [(3, 5 * g)] + [(c, g) for c in sorted({fwd - 1, fwd + 1, bwd + 1}) if c >= 1]


def deposit_ulps(dn, g):
    """cap of the difference at a deposit position, in units in the last place of the dtype at the magnitude of the
    values involved.  16-bit: the two float32 sums differ far below a 16-bit ulp, so only a rounding flip of the sum,
    of the quotient and of the final add can occur (the product with the ratio rounds a value that already flipped or
    did not).  float32: two summation orders of g float32 terms differ by at most 2 (g - 1) 2^-24 sum|t|, and
    sum|t| <= sum|g| / 2 up to rounding."""
    return g + 4 if dn == 'f32' else 4


def ulp(v, dn):
    e = max(int(np.floor(np.log2(v))), MIN_EXP[dn])
    return 2.0 ** (e - MANT[dn])


def first_argmax_positions(x, g):
    a = x.detach().float().cpu().reshape(-1, g).abs()
    first = (a == a.max(dim=1, keepdim=True).values).float().argmax(dim=1)
    return set((torch.arange(a.shape[0]) * g + first).tolist())


def assert_dw(got, want, w, grad, g, bits, dn, skip_groups=()):
    """bit-equal away from the first attaining element of each group; there, within deposit_ulps -> worst ulps seen"""
    gotf = got.float().cpu().numpy().reshape(-1).astype(np.float64)
    wantf = want.float().cpu().numpy().reshape(-1).astype(np.float64)
    gf = grad.float().cpu().numpy().reshape(-1).astype(np.float64)
    it = torch.int32 if dn == 'f32' else torch.int16
    bad = (got.reshape(-1).view(it) != want.reshape(-1).view(it)).nonzero().reshape(-1).tolist()
    bad = [i for i in bad if i // g not in skip_groups and not (np.isnan(gotf[i]) and np.isnan(wantf[i]))]
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


def make_weight(shape, g, dn, seed=123456):
    """the host test's groups (a 6x outlier in every third), scaled like a weight, with an all-zero group and a tie of
    the abs-max across chunks"""
    groups = shape[0] * shape[1] // g
    xg = (make_groups(groups, g, 'f32', seed) * 0.02).to(DT[dn])
    if groups > 2:
        xg[1] = 0.0
        m = (xg[2].abs().max().float() * 1.25).to(xg.dtype)
        xg[2, 1], xg[2, g - 2] = -m, m
    gen = torch.Generator().manual_seed(seed + 1)
    grad = torch.randn(shape, generator=gen).to(DT[dn])
    gscale = torch.randn(groups, generator=gen).to(DT[dn])
    return xg.reshape(shape).clone(), grad, gscale


def set_clamp(q, ste):
    from brevitas_amd.core.function_wrapper import TensorClamp, TensorClampSte
    q.int_quant.tensor_clamp_impl = TensorClampSte() if ste else TensorClamp()
    return q


def quantizer(w, g, bits, ratios, ste=True):
    import brevitas_amd.quant as Q
    return set_clamp(Q.Int8WeightPerGroupFloatMSE(w, group_size=g, bit_width=bits, mse_ratios=ratios).to(w.device), ste)


def backward(w, y, scale, grad, gscale):
    """grad None: y receives no gradient, the loss uses the returned scale alone"""
    w.grad = None
    if gscale is None:
        y.backward(grad.view(y.shape))
    elif grad is None:
        scale.backward(gscale.view(scale.shape))
    else:
        torch.autograd.backward([y, scale], [grad.view(y.shape), gscale.view(scale.shape)])
    return w.grad.detach().clone()


def fused_step(w0, g, bits, ratios, ste, grad, gscale=None):
    """-> (y, scale, dw, idx) of the module on a device weight"""
    w = torch.nn.Parameter(w0.clone())
    q = quantizer(w, g, bits, ratios, ste)
    y, scale, _, _ = q(w)
    dw = backward(w, y, scale, grad, gscale)
    return y.detach(), scale.detach(), dw, q.last_mse_index.clone()


def composed_step(w0, g, bits, ratios, ste, grad, gscale, idx):
    """the composed route at given candidates, its gradient by autograd through the sub-modules"""
    w = torch.nn.Parameter(w0.clone())
    q = quantizer(w, g, bits, ratios, ste)
    y, scale = q.quantize_at_index(w, idx)
    dw = backward(w, y, scale, grad, gscale)
    return y.detach(), scale.detach(), dw


def check_against_float64(idx, w, g, bits, ratios, skip=()):
    errs, _, _ = restate(w.detach().cpu().reshape(-1, g), ratios, bits)
    return check_index(idx, errs, g, skip)


# ---- forward and backward at every L and every edge of the walk -----------------------------------------------------

@sizes
@dtypes
def test_kernels_at_the_edges(dn, g, fused_calls):
    bits = 4
    worst, seen = 0.0, []
    for shape in shapes_of(dn, g):
        w, grad, gscale = make_weight(shape, g, dn)
        wd, gd, gsd = w.to(DEV), grad.to(DEV), gscale.to(DEV)
        n0 = dict(fused_calls)
        y, scale, dw, idx = fused_step(wd, g, bits, RATIOS, True, gd, gsd)
        assert fused_calls == {'fwd': n0['fwd'] + 1, 'bwd': n0['bwd'] + 1}
        assert tuple(scale.shape) == (shape[0], shape[1] // g, 1) and tuple(idx.shape) == (shape[0], shape[1] // g)
        seen.append((idx.reshape(-1).cpu(), restate(w.reshape(-1, g), RATIOS, bits)[0]))
        y_c, scale_c, dw_c = composed_step(wd, g, bits, RATIOS, True, gd, gsd, idx)
        assert fused_calls == {'fwd': n0['fwd'] + 1, 'bwd': n0['bwd'] + 1}   # the composed route launches neither
        assert same_bits(y, y_c), ('y', shape)
        assert same_bits(scale, scale_c), ('scale', shape)
        worst = max(worst, assert_dw(dw, dw_c, w, grad, g, bits, dn))
    # the candidates of all four tensors against the float64 restatement
    chose = check_index(torch.cat([i for i, _ in seen]), torch.cat([e for _, e in seen], dim=1), g)
    assert chose > 0.5
    print('GROUP_MSE_DEPOSIT_ULPS %s g=%d worst=%.3f chose k>0: %.3f' % (dn, g, worst, chose))


@dtypes
@pytest.mark.parametrize('n,step', [(1, .0), (20, .025), (64, .0125)], ids=['n1', 'n20', 'n64'])
@pytest.mark.parametrize('bits', [3, 4])
def test_candidate_counts_and_widths(dn, n, step, bits, fused_calls):
    shape, g = (24, 192), 32
    ratios = ratios_of(n, step)
    w, grad, _ = make_weight(shape, g, dn)
    wd, gd = w.to(DEV), grad.to(DEV)
    y, scale, dw, idx = fused_step(wd, g, bits, ratios, True, gd)
    assert fused_calls == {'fwd': 1, 'bwd': 1}
    chose = check_against_float64(idx, w, g, bits, ratios)
    assert int(idx.max()) < n and (chose > 0.5 or n == 1)
    y_c, scale_c, dw_c = composed_step(wd, g, bits, ratios, True, gd, None, idx)
    assert same_bits(y, y_c) and same_bits(scale, scale_c)
    assert_dw(dw, dw_c, w, grad, g, bits, dn)


@dtypes
@pytest.mark.parametrize('ste', [True, False], ids=['clamp_ste', 'clamp'])
@pytest.mark.parametrize('through_scale', [False, True, 'alone'], ids=['y', 'y_and_scale', 'scale_alone'])
def test_backward_against_the_composed_route(dn, ste, through_scale, fused_calls):
    shape, g, bits = (48, 192), 64, 4
    w, grad, gscale = make_weight(shape, g, dn)
    wd = w.to(DEV)
    gd = None if through_scale == 'alone' else grad.to(DEV)   # None: y receives no gradient
    gsd = gscale.to(DEV) if through_scale else None
    y, scale, dw, idx = fused_step(wd, g, bits, RATIOS, ste, gd, gsd)
    assert fused_calls == {'fwd': 1, 'bwd': 1}
    y_c, scale_c, dw_c = composed_step(wd, g, bits, RATIOS, ste, gd, gsd, idx)
    assert same_bits(y, y_c) and same_bits(scale, scale_c)
    if gd is None:
        # dw is the deposits alone
        dw0, dw_c0, skip = zero_off_the_deposits(dw, dw_c, scale_c, w, g)
        assert bool(dw.float().nan_to_num().any())  # the scale's gradient arrived
        assert_dw(dw0, dw_c0, w, torch.zeros_like(grad), g, bits, dn, skip_groups=skip)
        return
    assert_dw(dw, dw_c, w, grad, g, bits, dn)
    if through_scale:
        _, _, dw_plain, _ = fused_step(wd, g, bits, RATIOS, ste, gd)
        assert not torch.equal(dw, dw_plain)  # the scale's gradient arrived


@dtypes
def test_the_wrappers_outputs(dn, fused_calls):
    """nat.group_mse_fwd itself: y, scale, stat and idx; the statistic is the composed route's abs-max"""
    from brevitas_amd import _native as nat
    from brevitas_amd.core.quant import _fused
    shape, g, bits = (60, 512), 256, 4
    w, _, _ = make_weight(shape, g, dn)
    wd = torch.nn.Parameter(w.to(DEV))
    q = quantizer(wd, g, bits, RATIOS)
    desc, thr_div = _fused.group_quant_call(wd, g, 7.0, -7.0, 7.0, True)
    assert nat.group_mse_supported(desc, wd, len(RATIOS))
    y, scale, stat, idx = nat.group_mse_fwd(desc, wd.detach(), nat.mse_ratio_table(RATIOS), 1e-10, thr_div)
    assert idx.dtype == torch.uint8 and tuple(idx.shape) == (120,) and tuple(stat.shape) == (120,)
    assert same_bits(stat, w.reshape(-1, g).abs().max(dim=1).values)
    assert same_bits(stat.reshape(-1, 1), q.scaling_impl.parameter_list_stats().detach())
    y_c, scale_c = q.quantize_at_index(wd, idx)
    assert same_bits(y.reshape(shape), y_c) and same_bits(scale.reshape(60, 2, 1), scale_c)
    check_against_float64(idx, w, g, bits, RATIOS)


# ---- reduction, special groups, determinism -------------------------------------------------------------------------

@dtypes
@pytest.mark.parametrize('ste', [True, False], ids=['clamp_ste', 'clamp'])
def test_one_ratio_is_the_plain_fused_route(dn, ste, fused_calls):
    import brevitas_amd.quant as Q
    shape, g, bits = (24, 192), 32, 4
    w, grad, gscale = make_weight(shape, g, dn)
    wd, gd, gsd = w.to(DEV), grad.to(DEV), gscale.to(DEV)
    y, scale, dw, idx = fused_step(wd, g, bits, [1.0], ste, gd, gsd)
    assert fused_calls == {'fwd': 1, 'bwd': 1} and int(idx.max()) == 0
    p = torch.nn.Parameter(wd.clone())
    plain = set_clamp(Q.Int8WeightPerGroupFloat(p, group_size=g, bit_width=bits).to(DEV), ste)
    y_p, scale_p, _, _ = plain(p)
    dw_p = backward(p, y_p, scale_p, gd, gsd)
    assert same_bits(y, y_p) and same_bits(scale, scale_p) and same_bits(dw, dw_p)


@dtypes
def test_special_groups_and_two_runs(dn, fused_calls):
    import brevitas_amd.quant as Q
    shape, g, bits = (24, 192), 32, 4
    w, grad, gscale = make_weight(shape, g, dn)
    w.view(-1, g)[5, 9] = float('nan')
    w.view(-1, g)[8, 31] = float('inf')
    wd, gd, gsd = w.to(DEV), grad.to(DEV), gscale.to(DEV)
    a = fused_step(wd, g, bits, RATIOS, True, gd, gsd)
    b = fused_step(wd, g, bits, RATIOS, True, gd, gsd)
    assert fused_calls == {'fwd': 2, 'bwd': 2}
    it = torch.int32 if dn == 'f32' else torch.int16
    for s, t in zip(a[:3], b[:3]):
        assert torch.equal(s.view(it), t.view(it))           # the same bits, NaN patterns included
    assert torch.equal(a[3], b[3])
    y, scale, dw, idx = a
    assert idx.reshape(-1)[[1, 5, 8]].tolist() == [0, 0, 0]  # the zero, the NaN and the Inf group keep candidate 0
    check_against_float64(idx, w, g, bits, RATIOS, skip=(5, 8))
    p = torch.nn.Parameter(wd.clone())
    y_p, scale_p, _, _ = Q.Int8WeightPerGroupFloat(p, group_size=g, bit_width=bits).to(DEV)(p)
    for grp in (1, 5, 8):                                    # and the plain route's bits
        assert same_bits(y.view(-1, g)[grp], y_p.view(-1, g)[grp]) and same_bits(scale.view(-1)[grp], scale_p.view(-1)[grp])
    assert bool(torch.isnan(y.view(-1, g)[5]).all()) and bool(torch.isnan(y.view(-1, g)[8]).all())
    y_c, scale_c, dw_c = composed_step(wd, g, bits, RATIOS, True, gd, gsd, idx)
    assert same_bits(y, y_c) and same_bits(scale, scale_c)
    assert_dw(dw, dw_c, w, grad, g, bits, dn, skip_groups=(5, 8))


# ---- refusals take the composed route -------------------------------------------------------------------------------

@pytest.mark.parametrize('kind', ['misaligned', 'non_contiguous', 'g48', 'n65'])
def test_refusals_take_the_composed_route(kind, fused_calls):
    dn, bits, g, ratios = 'bf16', 4, 32, RATIOS
    gen = torch.Generator().manual_seed(7)
    if kind == 'misaligned':      # a weight view starting 2 bytes off a 16-byte boundary
        base = (torch.randn(48 * 96 + 8, generator=gen) * 0.02).to(DT[dn]).to(DEV)
        w = base[1:1 + 48 * 96].view(48, 96)
        assert w.data_ptr() % 16 == 2 and w.is_contiguous()
    elif kind == 'non_contiguous':
        w = (torch.randn(96, 48, generator=gen) * 0.02).to(DT[dn]).to(DEV).t()
        assert not w.is_contiguous()
    else:
        w = (torch.randn(48, 96, generator=gen) * 0.02).to(DT[dn]).to(DEV)
        if kind == 'g48':
            g = 48
        else:
            ratios = ratios_of(65, .0125)
    grad = torch.randn(w.shape, generator=gen).to(DT[dn]).to(DEV)
    p = torch.nn.Parameter(w)
    assert p.data_ptr() == w.data_ptr() and p.stride() == w.stride()
    q = quantizer(p, g, bits, ratios)
    y, scale, _, _ = q(p)
    dw = backward(p, y, scale, grad, None)
    assert fused_calls == {'fwd': 0, 'bwd': 0}
    idx = q.last_mse_index
    assert tuple(y.shape) == tuple(w.shape) and tuple(scale.shape) == (48, 96 // g, 1) and tuple(idx.shape) == (48, 96 // g)
    wc = w.detach().contiguous()
    # the restatement: the candidates, and the values at them
    errs, scales, ys = restate(wc.cpu().reshape(-1, g), ratios, bits)
    assert check_index(idx, errs, g) > 0.5
    k = idx.reshape(-1).long().cpu()
    assert same_bits(scale.reshape(-1).float(), scales.gather(0, k.reshape(1, -1)).reshape(-1))
    assert same_bits(y.contiguous().reshape(-1, g).float(), ys[k, torch.arange(k.numel())])
    assert bool(torch.isfinite(dw.float()).all()) and float(dw.float().abs().max()) > 0
    if kind in ('misaligned', 'non_contiguous'):
        # and the kernels on an aligned contiguous copy: the groups that chose the same candidate have the same bits
        y_f, scale_f, dw_f, idx_f = fused_step(wc, g, bits, ratios, True, grad.contiguous())
        assert fused_calls == {'fwd': 1, 'bwd': 1}
        agree = (idx_f == idx).reshape(-1)
        assert float(agree.float().mean()) >= 0.99
        assert same_bits(y.contiguous().view(-1, g)[agree], y_f.view(-1, g)[agree])
        assert same_bits(scale.reshape(-1)[agree], scale_f.reshape(-1)[agree])
        assert_dw(dw_f, dw.contiguous(), wc, grad.contiguous(), g, bits, dn,
                  skip_groups=set((~agree).nonzero().reshape(-1).tolist()))


def test_fused_paths_off_takes_the_composed_route(fused_calls, monkeypatch):
    import brevitas_amd.config as config
    shape, g, bits = (24, 192), 32, 4
    w, grad, _ = make_weight(shape, g, 'bf16')
    wd, gd = w.to(DEV), grad.to(DEV)
    y_f, scale_f, dw_f, idx_f = fused_step(wd, g, bits, RATIOS, True, gd)
    assert fused_calls == {'fwd': 1, 'bwd': 1}
    monkeypatch.setattr(config, 'FUSED_PATHS', False)
    y, scale, dw, idx = fused_step(wd, g, bits, RATIOS, True, gd)
    assert fused_calls == {'fwd': 1, 'bwd': 1}
    check_against_float64(idx, w, g, bits, RATIOS)
    agree = (idx_f == idx).reshape(-1)
    assert float(agree.float().mean()) >= 0.99
    assert same_bits(y.view(-1, g)[agree], y_f.view(-1, g)[agree]) and same_bits(scale.view(-1)[agree], scale_f.view(-1)[agree])


# ---- layers, graph capture, the non-temporal kernels ----------------------------------------------------------------

def test_layers_forward_backward(fused_calls):
    import brevitas_amd.quant as Q
    from brevitas_amd.nn import QuantConv2d, QuantLinear
    torch.manual_seed(0)
    lin = QuantLinear(256, 64, weight_quant=functools.partial(Q.Int4WeightPerGroupFloatMSE, group_size=64),
                      device=DEV, dtype=torch.bfloat16)
    conv = QuantConv2d(16, 8, 3, padding=1, weight_quant=functools.partial(Q.Int4WeightPerGroupFloatMSE, group_size=16),
                       device=DEV, dtype=torch.bfloat16)
    for layer, x, f in ((lin, torch.randn(4, 256, device=DEV, dtype=torch.bfloat16), torch.nn.functional.linear),
                        (conv, torch.randn(2, 16, 8, 8, device=DEV, dtype=torch.bfloat16),
                         functools.partial(torch.nn.functional.conv2d, padding=1))):
        n = dict(fused_calls)
        x.requires_grad_(True)
        y = layer(x)
        y.float().sum().backward()
        assert fused_calls == {'fwd': n['fwd'] + 1, 'bwd': n['bwd'] + 1}
        wq, scale, _, _ = layer.quant_weight()
        k = layer.weight.numel() // layer.weight.shape[0]
        assert tuple(scale.shape) == (layer.weight.shape[0], k // layer.weight_quant.group_size, 1)
        assert int(layer.weight_quant.last_mse_index.max()) > 0
        assert torch.equal(y, f(x, wq, layer.bias))
        assert layer.weight.grad is not None and bool(torch.isfinite(layer.weight.grad.float()).all())
        assert float(layer.weight.grad.float().abs().max()) > 0 and x.grad is not None


def test_step_in_a_graph(fused_calls):
    import brevitas_amd.quant as Q
    from test_gpu_graphs import _capture
    torch.manual_seed(123456)
    w = torch.nn.Parameter((torch.randn(32, 256, device=DEV) * 0.1).to(torch.bfloat16))
    g = torch.randn(32, 256, device=DEV).to(torch.bfloat16)
    q = Q.Int4WeightPerGroupFloatMSE(w, group_size=64).to(DEV)

    def one():
        w.grad = None
        y, scale, _, _ = q(w)
        y.backward(g)
        return y, scale, w.grad, q.last_mse_index

    graph, (y_s, scale_s, dw_s, idx_s) = _capture(one)
    assert fused_calls == {'fwd': 4, 'bwd': 4}
    with torch.no_grad():
        w.mul_(1.5).add_(0.01)  # new values in the captured input
    graph.replay()
    torch.cuda.synchronize()
    got = (y_s.clone(), scale_s.clone(), dw_s.clone(), idx_s.clone())
    y, scale, dw, idx = one()
    assert torch.equal(got[0], y) and torch.equal(got[1], scale) and torch.equal(got[2], dw) and torch.equal(got[3], idx)
    assert int(idx.max()) > 0


@dtypes
@pytest.mark.parametrize('g', [16, 256])
def test_the_non_temporal_kernels(dn, g, use_nt0, fused_calls):
    """the NT = true instantiations, through the library built with a non-temporal threshold of 0 bytes: the bits of the
    default library"""
    from brevitas_amd import _native as nat
    shape, bits = (3, 5 * g), 4
    w, grad, gscale = make_weight(shape, g, dn)
    wd, gd, gsd = w.to(DEV), grad.to(DEV), gscale.to(DEV)
    want = fused_step(wd, g, bits, RATIOS, True, gd, gsd)
    use_nt0()
    assert nat.lib.bvq_nt_threshold_bytes() == 0
    got = fused_step(wd, g, bits, RATIOS, True, gd, gsd)
    assert fused_calls == {'fwd': 2, 'bwd': 2}
    for a, b, what in zip(got, want, ('y', 'scale', 'dw', 'idx')):
        assert same_bits(a, b), what
