"""Group-wise HQO zero-point on the device: the one-launch kernels (csrc/bvq_group_hqo.hip) against the composed route
(_aten.group_hqo_search and the module's own sub-modules) run on the CPU on the same bits; the backward against the
composed route's autograd at the kernel's zero-points; special groups, the reduction to the plain asymmetric kernels,
refusals, a layer, graph capture and the forced non-temporal build.

Bars.  Forward: y, scale, zero-point and idx are bit-equal to the composed route on the CPU (a NaN equals a NaN): both
add a group's float32 terms in the one order of DESIGN.md §9, "Group-wise HQO zero-point".  Backward: dw is bit-equal to
the composed route's autograd except at the first element equal to the maximum and the first equal to the minimum of
each group, which receive a reduced float32 sum.  There the allowance of test_gpu_group_shifted.py applies
(test_group_shifted_golden.deposit_ulps, in units in the last place at a bound of every value on the deposit's way).  Its
derivation, restated: two routes that add the same float32 terms in another order and round at the same points differ
by the summation order -- n float32 addends differ by at most 2 (n - 1) 2^-24 sum|t|; the scale gradient has 2 g addends
and reaches the deposit divided by the integer threshold, the zero-point gradient g addends that reach it twice:
together 8 g - 6 units, which count against a float32 ulp only -- and by the roundings to the dtype behind the sums,
11 of them, each at most one ulp of its own value and carried into the next binade by a following quotient or product
at most once: 22.  Here the zero-point has no gradient, so its addends and five of the roundings are absent and the
bar is loose by that much; it is kept as it is stated for the asymmetric kernels.
"""
import functools

import pytest
import torch

from test_group_hqo_host import DT, plain, quantizer
from test_group_mse_host import same_bits
from test_group_shifted_golden import assert_dx
from test_gpu_group_mse import ITEMSIZE, shapes_of
from test_gpu_group_walk import use_nt0  # noqa: F401  (fixture: the forced-NT build of the library)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LANES, FWD_DEPTH = 64, 4
dtypes = pytest.mark.parametrize('dn', ['f32', 'bf16', 'f16'])
sizes = pytest.mark.parametrize('g', [16, 32, 64, 128, 256])


@pytest.fixture
def fused_calls(monkeypatch):
    """counts the launches of the HQO kernels' wrappers: {'fwd': n, 'bwd': n}"""
    from brevitas_amd import _native as nat
    calls = {'fwd': 0, 'bwd': 0}

    def count(name, key):
        real = getattr(nat, name)

        def counted(*a, **k):
            calls[key] += 1
            return real(*a, **k)
        monkeypatch.setattr(nat, name, counted)
    count('group_hqo_fwd', 'fwd')
    count('group_hqo_bwd', 'bwd')
    return calls


def make_weight(shape, g, dn, seed=123456):
    """weight-sized normal groups, each with one outlier of its own size at a position that moves from group to group,
    so that neighbouring groups of one wave load keep different candidates; an all-zero group and extrema tied across
    chunks where the tensor has room for them"""
    groups = shape[0] * shape[1] // g
    gen = torch.Generator().manual_seed(seed + g)
    xg = torch.randn(groups, g, generator=gen) * 0.05
    rows = torch.arange(groups)
    xg[rows, (rows * 7) % g] += torch.randn(groups, generator=gen) * 0.3
    xg = xg.to(DT[dn])
    if groups > 4:
        xg[1] = 0.0
        m = (xg[2].abs().max().float() * 1.25).to(xg.dtype)
        xg[2, 1], xg[2, g - 2] = m, m          # the maximum twice, in two chunks
        xg[4, 0], xg[4, g - 1] = -m, -m        # the minimum twice
    grad = torch.randn(shape, generator=gen).to(DT[dn])
    gscale = torch.randn(groups, generator=gen).to(DT[dn])
    return xg.reshape(shape).clone(), grad, gscale


def search_args(bits, p, iters=20):
    """hqo_beta at which the shrinkage acts on weights of this size: the residuals are at most half a step, about 0.01 at
    4 bits and 0.0006 at 8, and a residual is shrunk only where it exceeds 1 / beta_i (p = 1).  At the default beta of
    10 nothing is shrunk here and both norms compute the same zero-points."""
    return dict(hqo_iters=iters, hqo_lp_norm=p, hqo_beta={4: 300.0, 8: 5000.0}[bits], hqo_kappa=1.05)


def set_clamp(q, ste):
    from brevitas_amd.core.function_wrapper import TensorClamp, TensorClampSte
    q.int_quant.tensor_clamp_impl = TensorClampSte() if ste else TensorClamp()
    return q


def backward(w, y, scale, grad, gscale):
    w.grad = None
    if gscale is None:
        y.backward(grad.view(y.shape))
    else:
        torch.autograd.backward([y, scale], [grad.view(y.shape), gscale.view(scale.shape)])
    return w.grad.detach().clone()


def forward(w0, g, bits, **kw):
    """-> (y, scale, zero_point, idx) of the module on w0, wherever w0 lives; no gradient"""
    w = torch.nn.Parameter(w0.clone())
    q = quantizer(w, g, bits, **kw).to(w.device)
    with torch.no_grad():
        y, scale, zp, _ = q(w)
    return y, scale, zp, q.last_hqo_index.clone()


def fused_step(w0, g, bits, ste, grad, gscale=None, **kw):
    """-> (y, scale, zero_point, idx, dw) of the module on a device weight"""
    w = torch.nn.Parameter(w0.clone())
    q = set_clamp(quantizer(w, g, bits, **kw).to(w.device), ste)
    y, scale, zp, _ = q(w)
    dw = backward(w, y, scale, grad, gscale)
    return y.detach(), scale.detach(), zp.detach(), q.last_hqo_index.clone(), dw


def composed_step(w0, g, bits, ste, grad, gscale, zp, **kw):
    """the composed route at given zero-points, its gradient by autograd through the sub-modules"""
    w = torch.nn.Parameter(w0.clone())
    q = set_clamp(quantizer(w, g, bits, **kw).to(w.device), ste)
    y, scale = q.quantize_at_zero_point(w, zp)
    dw = backward(w, y, scale, grad, gscale)
    return y.detach(), scale.detach(), dw


def assert_forward(got, want, what):
    for a, b, name in zip(got, want, ('y', 'scale', 'zero_point', 'idx')):
        assert same_bits(a, b), (name, what)


# ---- forward: the kernel against the composed route on the CPU ------------------------------------------------------

@sizes
@dtypes
@pytest.mark.parametrize('bits', [4, 8])
@pytest.mark.parametrize('p', [1.0, 0.5], ids=['p1', 'p05'])
def test_forward_is_the_composed_route_on_the_cpu(dn, g, bits, p, fused_calls):
    """k takes several values among the groups of the first wave's window (where that holds fewer than 16 groups, among
    the first 16).  Not asserted for 8-bit codes in the 16-bit types: the zero-point, a value near 128, has no fractional
    bit in bfloat16 and three in float16, and nearly every group keeps candidate 0."""
    spread = set()
    for shape in shapes_of(dn, g):
        w, _, _ = make_weight(shape, g, dn)
        n0 = dict(fused_calls)
        got = forward(w.to(DEV), g, bits, **search_args(bits, p))
        assert fused_calls == {'fwd': n0['fwd'] + 1, 'bwd': n0['bwd']}
        want = forward(w, g, bits, **search_args(bits, p))
        assert fused_calls == {'fwd': n0['fwd'] + 1, 'bwd': n0['bwd']}   # the CPU takes the composed route
        assert tuple(got[1].shape) == tuple(got[2].shape) == (shape[0], shape[1] // g, 1)
        assert tuple(got[3].shape) == (shape[0], shape[1] // g) and got[3].dtype == torch.uint8
        assert_forward(got, want, shape)
        # the candidates kept by the groups of the first wave's window
        window = (LANES // (g * ITEMSIZE[dn] // 16)) * FWD_DEPTH
        spread |= set(got[3].reshape(-1)[:max(window, 16)].tolist())
    print('GROUP_HQO_K %s g=%d bits=%d p=%s kept in the first window: %s' % (dn, g, bits, p, sorted(spread)))
    if dn == 'f32' or bits != 8:
        assert len(spread) >= 2, sorted(spread)


@dtypes
def test_forward_with_63_iterations(dn, fused_calls):
    g, bits = 64, 4
    for shape in shapes_of(dn, g)[:2]:
        w, _, _ = make_weight(shape, g, dn)
        got = forward(w.to(DEV), g, bits, **search_args(bits, 0.5, 63))
        assert_forward(got, forward(w, g, bits, **search_args(bits, 0.5, 63)), shape)
        assert int(got[3].max()) > 0
    assert fused_calls == {'fwd': 2, 'bwd': 0}


@dtypes
@pytest.mark.parametrize('bits', [4, 8])
def test_zero_iterations_are_the_plain_kernel(dn, bits, fused_calls):
    """bvq_group_hqo_fwd with no iteration against bvq_group_shifted_fwd itself: y, scale, zero-point and statistics"""
    from brevitas_amd import _native as nat
    from brevitas_amd.core.quant import _fused
    shape, g = (7, 96), 32
    w, _, _ = make_weight(shape, g, dn)
    wd = w.to(DEV)
    desc, thr_div = _fused.group_shifted_call(wd, g, 2.0 ** bits - 1, 0.0, 2.0 ** bits - 1, True)
    assert nat.group_hqo_supported(desc, wd, 0, 1)
    for lp in (0, 1):
        y, scale, zp, stat, idx = nat.group_hqo_fwd(desc, wd, nat.hqo_beta_table(10.0, 1.01, 0), lp, 1e-10, thr_div)
        for a, b, name in zip((y, scale, zp, stat), nat.group_shifted_fwd(desc, wd, 1e-10, thr_div),
                              ('y', 'scale', 'zp', 'stat')):
            assert same_bits(a, b), name
        assert idx.dtype == torch.uint8 and tuple(idx.shape) == (21,) and not bool(idx.any())
    got = forward(wd, g, bits, hqo_iters=0)
    pw = torch.nn.Parameter(wd.clone())
    with torch.no_grad():
        want = plain(pw, g, bits).to(DEV)(pw)
    assert_forward(got[:3], want[:3], 'module')


# ---- backward: against the composed route's autograd at the kernel's zero-points ------------------------------------

@dtypes
@pytest.mark.parametrize('g', [16, 64, 256])
@pytest.mark.parametrize('ste', [True, False], ids=['clamp_ste', 'clamp'])
@pytest.mark.parametrize('through_scale', [False, True], ids=['y', 'y_and_scale'])
def test_backward_against_the_composed_route(dn, g, ste, through_scale, fused_calls):
    bits, worst = 4, 0.0
    for shape in shapes_of(dn, g)[:2]:   # the tensor ending inside a wave load, the backward's window plus a group
        w, grad, gscale = make_weight(shape, g, dn)
        wd, gd = w.to(DEV), grad.to(DEV)
        gsd = gscale.to(DEV) if through_scale else None
        n0 = dict(fused_calls)
        y, scale, zp, idx, dw = fused_step(wd, g, bits, ste, gd, gsd)
        assert fused_calls == {'fwd': n0['fwd'] + 1, 'bwd': n0['bwd'] + 1}
        y_c, scale_c, dw_c = composed_step(wd, g, bits, ste, gd, gsd, zp)
        assert fused_calls == {'fwd': n0['fwd'] + 1, 'bwd': n0['bwd'] + 1}   # the composed route launches neither
        assert same_bits(y, y_c) and same_bits(scale, scale_c)
        worst = max(worst, assert_dx(dw, dw_c, w, grad, scale_c, zp, g, bits, dn, gsd))
        assert bool(torch.isfinite(dw.float()).all()) or dn == 'f16'   # (float16: the zero group's scale is 0)
        if through_scale:
            dw_plain = fused_step(wd, g, bits, ste, gd)[4]
            assert not torch.equal(dw.float().nan_to_num(), dw_plain.float().nan_to_num())  # the gradient arrived
    print('GROUP_HQO_DEPOSIT_ULPS %s g=%d ste=%d gscale=%d worst=%.3f' % (dn, g, ste, through_scale, worst))


# ---- special groups -------------------------------------------------------------------------------------------------

@dtypes
def test_special_groups(dn, fused_calls):
    shape, g, bits = (24, 192), 32, 4
    w, grad, _ = make_weight(shape, g, dn)
    w2 = w.view(-1, g)
    w2[6, 9] = float('nan')
    w2[7, 31] = float('inf')
    w2[8, 0] = -float('inf')
    w2[9] = 0.015625                       # constant
    w2[10] = w2[10].abs() + 0.01           # positive values only
    w2[11] = -(w2[11].abs()) - 0.01        # negative values only
    special = [1, 6, 7, 8, 9]              # zero, NaN, Inf, -Inf, constant: candidate 0 and the plain route's bits
    wd, gd = w.to(DEV), grad.to(DEV)
    y, scale, zp, idx, dw = fused_step(wd, g, bits, True, gd)
    assert fused_calls == {'fwd': 1, 'bwd': 1}
    assert_forward((y, scale, zp, idx), forward(w, g, bits), 'cpu')
    assert idx.reshape(-1)[special].tolist() == [0] * 5 and int(idx.max()) > 0
    pw = torch.nn.Parameter(wd.clone())
    y_p, scale_p, zp_p, _ = plain(pw, g, bits).to(DEV)(pw)
    y_p.backward(gd)
    for a, b, name in ((y.view(-1, g), y_p.view(-1, g), 'y'), (scale.view(-1), scale_p.view(-1), 'scale'),
                       (zp.view(-1), zp_p.view(-1), 'zero_point')):
        assert same_bits(a[special], b[special]), name
    for grp in (6, 7, 8):
        assert bool(torch.isnan(y.view(-1, g)[grp]).all())
    # dx is finite where the plain route's is
    finite_plain = torch.isfinite(pw.grad.float()).view(-1, g).all(dim=1)
    finite = torch.isfinite(dw.float()).view(-1, g).all(dim=1)
    assert bool(finite[finite_plain].all()), torch.nonzero(finite_plain & ~finite).reshape(-1).tolist()
    assert bool(finite[[10, 11]].all()) and (dn == 'f16' or bool(finite[[1, 9]].all()))
    y_c, scale_c, dw_c = composed_step(wd, g, bits, True, gd, None, zp)
    assert same_bits(y, y_c) and same_bits(scale, scale_c)
    assert_dx(dw, dw_c, w, grad, scale_c, zp, g, bits, dn, skip_groups=(6, 7, 8))
    # two runs give the same bits
    again = fused_step(wd, g, bits, True, gd)
    for a, b in zip((y, scale, zp, idx, dw), again):
        assert same_bits(a, b)


# ---- routing --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('kind', ['misaligned', 'non_contiguous', 'p07', 'fused_off'])
def test_refusals_take_the_composed_route(kind, fused_calls, monkeypatch):
    import brevitas_amd.config as config
    dn, bits, g, p = 'bf16', 4, 32, 0.5
    w0, grad, _ = make_weight((48, 96), g, dn)
    if kind == 'misaligned':      # a weight view starting 2 bytes off a 16-byte boundary
        base = torch.zeros(48 * 96 + 8, dtype=DT[dn], device=DEV)
        w = base[1:1 + 48 * 96].view(48, 96)
        w.copy_(w0)
        assert w.data_ptr() % 16 == 2 and w.is_contiguous()
    elif kind == 'non_contiguous':
        w = w0.t().contiguous().to(DEV).t()
        assert not w.is_contiguous() and torch.equal(w.cpu(), w0)
    else:
        w = w0.to(DEV)
        if kind == 'p07':
            p = 0.7
        else:
            monkeypatch.setattr(config, 'FUSED_PATHS', False)
    pw = torch.nn.Parameter(w)
    assert pw.data_ptr() == w.data_ptr() and pw.stride() == w.stride()
    q = quantizer(pw, g, bits, hqo_lp_norm=p).to(DEV)
    y, scale, zp, _ = q(pw)
    dw = backward(pw, y, scale, grad.to(DEV), None)
    assert fused_calls == {'fwd': 0, 'bwd': 0}
    idx = q.last_hqo_index
    assert tuple(y.shape) == (48, 96) and tuple(scale.shape) == tuple(zp.shape) == (48, 3, 1) and tuple(idx.shape) == (48, 3)
    assert not zp.requires_grad and int(idx.max()) > 0
    assert bool(torch.isfinite(dw.float()).all()) and float(dw.float().abs().max()) > 0
    # the composed route on the device computes the bits of the composed route on the CPU ...
    want = forward(w0, g, bits, hqo_lp_norm=p)
    if kind != 'p07':   # (torch.pow is not one function on both)
        assert_forward((y.detach().contiguous(), scale.detach(), zp, idx), want, kind)
        # ... which are the kernels' on an aligned contiguous copy
        monkeypatch.setattr(config, 'FUSED_PATHS', True)
        assert_forward(forward(w0.to(DEV), g, bits, hqo_lp_norm=p), want, 'fused')
        assert fused_calls == {'fwd': 1, 'bwd': 0}


def test_a_cpu_weight_takes_the_composed_route(fused_calls):
    w0, grad, _ = make_weight((8, 128), 64, 'f32')
    w = torch.nn.Parameter(w0)
    q = quantizer(w, 64, 4)
    y, scale, zp, _ = q(w)
    y.backward(grad)
    assert fused_calls == {'fwd': 0, 'bwd': 0} and bool(torch.isfinite(w.grad).all())


# ---- a layer, graph capture, the non-temporal kernels ---------------------------------------------------------------

def test_quant_linear_training_step(fused_calls):
    import brevitas_amd.quant as Q
    from brevitas_amd.nn import QuantLinear
    torch.manual_seed(0)
    lin = QuantLinear(256, 64, weight_quant=functools.partial(Q.ShiftedUint4WeightPerGroupFloatHQO, group_size=64),
                      device=DEV, dtype=torch.bfloat16)
    opt = torch.optim.SGD(lin.parameters(), lr=0.01)
    x = torch.randn(4, 256, device=DEV, dtype=torch.bfloat16, requires_grad=True)
    before = lin.weight.detach().clone()
    y = lin(x)
    y.float().sum().backward()
    assert fused_calls == {'fwd': 1, 'bwd': 1}
    wq, scale, zp, _ = lin.quant_weight()
    assert tuple(scale.shape) == tuple(zp.shape) == (64, 4, 1) and not zp.requires_grad
    assert int(lin.weight_quant.last_hqo_index.max()) > 0
    assert torch.equal(y, torch.nn.functional.linear(x, wq, lin.bias))
    assert bool(torch.isfinite(lin.weight.grad.float()).all()) and float(lin.weight.grad.float().abs().max()) > 0
    assert x.grad is not None
    opt.step()
    assert not torch.equal(lin.weight.detach(), before)


def test_step_in_a_graph(fused_calls):
    import brevitas_amd.quant as Q
    from test_gpu_graphs import _capture
    torch.manual_seed(123456)
    w = torch.nn.Parameter((torch.randn(32, 256, device=DEV) * 0.1).to(torch.bfloat16))
    g = torch.randn(32, 256, device=DEV).to(torch.bfloat16)
    q = Q.ShiftedUint4WeightPerGroupFloatHQO(w, group_size=64).to(DEV)

    def one():
        w.grad = None
        y, scale, zp, _ = q(w)
        y.backward(g)
        return y, scale, zp, w.grad, q.last_hqo_index

    graph, static = _capture(one)
    assert fused_calls == {'fwd': 4, 'bwd': 4}
    with torch.no_grad():
        w.mul_(1.5).add_(0.01)  # new values in the captured input
    graph.replay()
    torch.cuda.synchronize()
    got = [t.clone() for t in static]
    want = one()
    for a, b in zip(got, want):
        assert same_bits(a, b)
    assert int(want[4].max()) > 0


@dtypes
@pytest.mark.parametrize('g', [16, 256])
def test_the_non_temporal_kernels(dn, g, use_nt0, fused_calls):  # noqa: F811
    """the NT = true instantiations, through the library built with a non-temporal threshold of 0 bytes: the bits of the
    default library"""
    from brevitas_amd import _native as nat
    shape, bits = (3, 5 * g), 4
    w, grad, gscale = make_weight(shape, g, dn)
    wd, gd, gsd = w.to(DEV), grad.to(DEV), gscale.to(DEV)
    want = [fused_step(wd, g, bits, True, gd, gsd, **search_args(bits, p)) for p in (1.0, 0.5)]
    assert not same_bits(want[0][2], want[1][2])   # the two norms keep different zero-points
    use_nt0()
    assert nat.lib.bvq_nt_threshold_bytes() == 0
    got = [fused_step(wd, g, bits, True, gd, gsd, **search_args(bits, p)) for p in (1.0, 0.5)]
    assert fused_calls == {'fwd': 4, 'bwd': 4}
    for a, b in zip(got, want):
        for s, t, what in zip(a, b, ('y', 'scale', 'zero_point', 'idx', 'dw')):
            assert same_bits(s, t), what
