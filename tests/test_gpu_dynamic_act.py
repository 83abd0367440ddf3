"""Dynamic activation quantizers on the device: the golden vectors of the reference on every route, the asymmetric
per-row kernels (csrc/bvq_row_shifted.hip) against the route they replace -- ShiftedUint8WeightPerChannelFloat on
x.view(rows, H) with the same clamp --, the refusals, the routing, the layers, graph capture and the guard elements
behind every output.

Bars: y, scale, zp and stat are bit-exact everywhere (a NaN equals a NaN).  dx is bit-exact except at the first element
equal to the minimum and the first equal to the maximum of each row, which receive reduced float32 sums: the row
kernel adds a row's terms in another order than the per-channel kernels, so those elements may differ by the roundings
derived at test_group_shifted_golden.deposit_ulps, with g := H.
"""
import ctypes
import functools

import pytest
import torch

import dynamic_golden as D
from test_gpu_group_shifted import assert_same_bits, compare, compare_without_gy, set_clamp, step

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
DT = {'f32': torch.float32, 'bf16': torch.bfloat16, 'f16': torch.float16}
SIZE = {'f32': 4, 'bf16': 2, 'f16': 2}
MAX_C = 2048   # bvq_row_shifted_max_row_bytes() / 16, checked below
# (16-byte chunks per row C, rows); H = C * 16 / sizeof(T).  'min': the shortest row the planted cases fit (16
# elements).  5: less than a wave load, no power of two.  67: one wave load and a ragged second.  1376: H = 11008 in
# bf16, several waves, ragged.  MAX_C: the longest row, and that row alone.  The kernels have three geometries -- one
# wave per row up to C = 128, one workgroup with two loads per lane up to C = 512, with eight above -- so 128 | 129 and
# 512 | 513 stand on the two sides of each boundary.
SHAPES = [('min', 13), (5, 7), (67, 12), (128, 12), (129, 12), (512, 12), (513, 12), (1376, 11), (MAX_C, 10),
          (MAX_C, 1)]
shapes = pytest.mark.parametrize('chunks,rows', SHAPES, ids=['C%s-r%d' % s for s in SHAPES])
dtypes = pytest.mark.parametrize('dn', ['f32', 'bf16', 'f16'])


def row_len(chunks, dn):
    return 16 if chunks == 'min' else chunks * 16 // SIZE[dn]


@pytest.fixture
def cpu_scalar_semantics(monkeypatch):
    """the golden vectors were produced by torch CPU kernels (include/bvq.h, bvq_scalar_mode)"""
    import brevitas_amd.config as config
    monkeypatch.setattr(config, 'SCALAR_OPERAND_MODE', 'cpu')


def _counter(monkeypatch, name):
    from brevitas_amd import _native as nat
    calls = []
    real = getattr(nat, name)

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)
    monkeypatch.setattr(nat, name, counted)
    return calls


@pytest.fixture
def fused_calls(monkeypatch):
    """counts the launches of the asymmetric row kernels' forward wrapper"""
    return _counter(monkeypatch, 'row_shifted_fwd')


def plant(x2, dn):
    """rows of x2 = [rows, H], in place, as many as there are: first the two ties only a row of several waves can get
    wrong, then the ten rows of tests/golden/make_golden_group_shifted.py"""
    rows, h = x2.shape
    vec = 16 // SIZE[dn]

    def big(r, factor):
        return (x2[r].abs().max().float() * factor).to(x2.dtype)

    def first_last(r):      # the maximum at the row's first element and at the last element of its last chunk
        m = big(r, 1.25)
        x2[r, 0], x2[r, h - 1] = m, m

    def same_chunk(r):      # the maximum and the minimum in one chunk, the last
        m = big(r, 1.5)
        x2[r, h - vec], x2[r, h - 1] = m, -m

    def zero(r):
        x2[r] = 0.0

    def constant(r):
        x2[r] = 0.015625

    def positive(r):
        x2[r] = x2[r].abs() + 0.01

    def negative(r):
        x2[r] = -(x2[r].abs()) - 0.01

    def tie(sign, first, second):
        def f(r):
            m = big(r, 1.25) * sign
            x2[r, first], x2[r, second] = m, m
        return f

    def ends(r):
        m = big(r, 1.5)
        x2[r, 0], x2[r, h - 1] = m, -m

    def zeros(r):
        x2[r] = -(x2[r].abs()) - 0.001
        x2[r, 3], x2[r, h - 4] = -0.0, 0.0

    planters = [first_last, same_chunk, ends, tie(-1, 2, h - 3), tie(1, 1, h - 2), zeros, constant, zero, positive,
                negative, tie(-1, 5, 6), tie(1, 4, 5)]
    for r, p in zip(range(rows), planters):
        p(r)


def make_input(chunks, rows, dn, seed=24680):
    h = row_len(chunks, dn)
    gen = torch.Generator().manual_seed(seed)
    x = (torch.randn(rows, h, generator=gen) * 0.02).to(DT[dn])
    plant(x, dn)
    grad = torch.randn(rows, h, generator=gen).to(DT[dn])
    gscale = torch.randn(rows, generator=gen).to(DT[dn])
    gzp = (torch.randn(rows, generator=gen) * 0.01).to(DT[dn])
    return x.to(DEV), grad.to(DEV), gscale.to(DEV), gzp.to(DEV)


def row_step(x0, bits, ste, grad, gscale=None, gzp=None):
    """the row kernels through their Function, whatever H"""
    from brevitas_amd.core.quant import _fused
    x = x0.clone().requires_grad_(True)
    qmax = float(2 ** bits - 1)
    y, scale, zp = _fused.RowShiftedFakeQuantFn.apply(x, 1e-10, qmax, 0.0, qmax, ste)
    outs, grads = ([y], [grad]) if grad is not None else ([], [])   # None: y receives no gradient
    if gscale is not None:
        outs, grads = outs + [scale], grads + [gscale.view(scale.shape)]
    if gzp is not None:
        outs, grads = outs + [zp], grads + [gzp.view(zp.shape)]
    torch.autograd.backward(outs, grads)
    return y.detach(), scale.detach(), zp.detach(), x.grad.detach().clone()


def module_step(x0, bits, ste, grad, gscale=None, gzp=None, make=None):
    import brevitas_amd.quant as Q
    x = torch.nn.Parameter(x0)   # (shares x0's memory: a view stays the view it is)
    q = set_clamp((make or Q.ShiftedUint8DynamicActPerRowFloat)(bit_width=bits).to(DEV), ste)
    return step(q, x, grad, gscale, gzp)


def per_channel_step(x0, bits, ste, grad, gscale=None, gzp=None):
    """the parent's route: the per-channel asymmetric weight quantizer on x.view(rows, H), the same clamp"""
    import brevitas_amd.quant as Q
    h = x0.shape[-1]
    w = torch.nn.Parameter(x0.detach().contiguous().view(-1, h).clone())
    q = set_clamp(Q.ShiftedUint8WeightPerChannelFloat(w, bit_width=bits).to(DEV), ste)
    return step(q, w, None if grad is None else grad.contiguous().view(-1, h), gscale, gzp)


def test_the_cap_is_the_one_the_shapes_assume():
    from brevitas_amd import _native as nat
    assert nat.row_shifted_max_row_bytes() == MAX_C * 16 >= 32768


# ---- golden ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('c', D.CASES, ids=D.IDS)
@pytest.mark.parametrize('fused', [True, False], ids=['fused', 'composed'])
def test_golden(c, fused, fused_calls, cpu_scalar_semantics, monkeypatch):
    import brevitas_amd.config as config
    monkeypatch.setattr(config, 'FUSED_PATHS', fused)
    if not fused and c['shifted'] and c['granularity'] == 'tensor' and c['dtype'] != 'f32':
        # Op by op on the device, `x / scale` with a 16-bit x and the 0-dim float32 scale of a per-tensor quantizer is
        # torch's DEVICE kernel, which rounds the scalar to x's dtype first, where the CPU kernel that made the golden
        # vectors keeps it in float32 ("0-dim float32 scale next to a bf16 tensor").  (max - min) / (2^b - 1)
        # is no bf16 value, so the reference itself, run on the device, does not give those bits (the symmetric
        # abs-max / 2^(b-1) is one, and stays held to them).  This route is held to the device's own semantics instead:
        # the bits of the quantizer kernel reading the scalar the device's way.
        monkeypatch.setattr(config, 'SCALAR_OPERAND_MODE', 'device')
        got = D.run_case(c, DEV)
        monkeypatch.setattr(config, 'FUSED_PATHS', True)
        want = D.run_case(c, DEV)
        for a, b, name in zip(got[:3], want[:3], ('y', 'scale', 'zp')):
            assert torch.equal(a, b), name
        D.assert_dx_tensor(got[3], want[3], c.torch('x'), c.torch('g'), want[1], want[2], c['bit_width'], c['dtype'])
        assert len(fused_calls) == 0
        return
    worst = D.check_case(c, *D.run_case(c, DEV))
    row_kernel = c['shifted'] and c['granularity'] == 'row'   # H = 40, 536, 1032: no group size
    assert len(fused_calls) == (1 if fused and row_kernel else 0)
    if worst is not None:
        print('ROW_SHIFTED_DEPOSIT_ULPS golden %s %s H=%d bits=%d fused=%d worst=%.3f'
              % (c['quantizer'], c['dtype'], c['shape'][1], c['bit_width'], fused, worst))


# ---- the row kernels against the parent's route ---------------------------------------------------------------------

@shapes
@dtypes
@pytest.mark.parametrize('bits', [4, 8])
@pytest.mark.parametrize('ste', [True, False], ids=['clamp_ste', 'clamp'])
def test_row_kernels_against_the_per_channel_route(chunks, rows, dn, bits, ste, fused_calls):
    from brevitas_amd import _native as nat
    from brevitas_amd.core.quant import _fused
    x, grad, _, _ = make_input(chunks, rows, dn)
    h = x.shape[1]
    got = row_step(x, bits, ste, grad)
    assert len(fused_calls) == 1
    assert tuple(got[1].shape) == tuple(got[2].shape) == (rows, 1)
    zf = got[2].float()
    finite = torch.isfinite(zf)
    assert bool((zf[finite] == zf[finite].round()).all()) and bool(((zf[finite] >= 0) & (zf[finite] <= 2 ** bits - 1)).all())
    # stat: the maxima then the minima, the bits of the parent's statistic kernel on the same rows.  (-0 equals +0 as a
    # statistic -- include/bvq.h -- and which of the two a row holding both reports is nobody's contract: "+ 0.0" makes
    # them one before the bits are compared.)
    desc, thr_div = _fused.row_shifted_call(x, 2.0 ** bits - 1, 0.0, 2.0 ** bits - 1, ste)
    assert nat.row_shifted_supported(desc, x)
    stat = nat.row_shifted_fwd(desc, x, 1e-10, thr_div)[3]
    want_stat = nat.stats(nat.STAT_MINMAX, x.reshape(-1), 1, rows, h)
    assert_same_bits(stat + 0.0, want_stat + 0.0, dn, 'stat')
    assert torch.equal(stat[:rows].float(), x.max(dim=1).values.float())
    assert torch.equal(stat[rows:].float(), x.min(dim=1).values.float())
    worst = compare(got, per_channel_step(x, bits, ste, grad), x, grad, h, bits, dn)
    print('ROW_SHIFTED_DEPOSIT_ULPS %s C=%s rows=%d bits=%d ste=%d worst=%.3f' % (dn, chunks, rows, bits, ste, worst))


@dtypes
@pytest.mark.parametrize('ste', [True, False], ids=['clamp_ste', 'clamp'])
def test_gradients_through_scale_and_zero_point(dn, ste, fused_calls):
    """the loss uses the returned scale and zero-point too: their gradients join the row's sums before the deposits"""
    x, grad, gscale, gzp = make_input(67, 12, dn)
    h = x.shape[1]
    plain = row_step(x, 4, ste, grad)
    for gs, gz in ((gscale, None), (None, gzp), (gscale, gzp)):
        got = row_step(x, 4, ste, grad, gs, gz)
        worst = compare(got, per_channel_step(x, 4, ste, grad, gs, gz), x, grad, h, 4, dn, gs, gz)
        assert not torch.equal(got[3].float().nan_to_num(), plain[3].float().nan_to_num())  # the gradient arrived
        print('ROW_SHIFTED_DEPOSIT_ULPS %s C=67 gscale=%d gzp=%d ste=%d worst=%.3f'
              % (dn, gs is not None, gz is not None, ste, worst))
    assert len(fused_calls) == 4


@dtypes
@pytest.mark.parametrize('chunks', [17, 67, 130], ids=['C17', 'C67', 'C130'])   # one wave; one wave; four waves
@pytest.mark.parametrize('ste', [True, False], ids=['clamp_ste', 'clamp'])
def test_gradients_through_scale_or_zero_point_alone(dn, chunks, ste, fused_calls):
    """y receives no gradient: the kernel takes zeros for it, and dx is the deposits alone"""
    x, _, gscale, gzp = make_input(chunks, 12, dn)
    h = x.shape[1]
    for gs, gz in ((gscale, None), (None, gzp)):
        got = row_step(x, 4, ste, None, gs, gz)
        worst = compare_without_gy(got, per_channel_step(x, 4, ste, None, gs, gz), x, h, 4, dn, gs, gz)
        assert bool(got[3].float().nan_to_num().any())  # the gradient arrived
        print('ROW_SHIFTED_DEPOSIT_ULPS %s C=%d no gy gscale=%d gzp=%d ste=%d worst=%.3f'
              % (dn, chunks, gs is not None, gz is not None, ste, worst))
    assert len(fused_calls) == 2


@dtypes
@pytest.mark.parametrize('chunks', [67, 1376])
def test_rows_with_a_nan(dn, chunks, fused_calls):
    """a NaN reaches both statistics, whatever its sign and wherever it stands: that row's outputs are NaN, and no other
    row sees it"""
    x, grad, _, _ = make_input(chunks, 12, dn)
    h = x.shape[1]
    x[10, 9] = float('nan')
    x[11, h - 1] = -float('nan')
    got = row_step(x, 8, True, grad)
    assert len(fused_calls) == 1
    compare(got, per_channel_step(x, 8, True, grad), x, grad, h, 8, dn, skip_groups=(10, 11))
    y, scale, zp = got[0], got[1], got[2]
    for r in (10, 11):
        assert bool(torch.isnan(scale.reshape(-1)[r])) and bool(torch.isnan(zp.reshape(-1)[r]))
        assert bool(torch.isnan(y[r]).all())
    clean, _, _, _ = make_input(chunks, 12, dn)
    want = row_step(clean, 8, True, grad)
    for a, b in zip(got, want):
        assert_same_bits(a[:10], b[:10], dn, 'rows without a NaN')


def test_two_runs_give_the_same_bits(fused_calls):
    x, grad, gscale, gzp = make_input(1376, 11, 'bf16')
    a = row_step(x, 4, False, grad, gscale, gzp)
    b = row_step(x, 4, False, grad, gscale, gzp)
    assert len(fused_calls) == 2
    for s, t in zip(a, b):
        assert torch.equal(s.view(torch.int16), t.view(torch.int16))


# ---- refusals stay correct ------------------------------------------------------------------------------------------

@pytest.mark.parametrize('kind', ['misaligned', 'ragged_row', 'non_contiguous', 'too_long'])
def test_refusals_take_the_composed_route(kind, fused_calls):
    dn, bits = 'bf16', 8
    gen = torch.Generator().manual_seed(7)
    rows, h = 6, 536
    if kind == 'misaligned':       # a view starting 2 bytes off a 16-byte boundary
        base = (torch.randn(rows * h + 8, generator=gen) * 0.02).to(DT[dn]).to(DEV)
        x = base[1:1 + rows * h].view(rows, h)
        assert x.data_ptr() % 16 == 2 and x.is_contiguous()
    elif kind == 'ragged_row':     # 88 bytes per row
        h = 44
        x = (torch.randn(rows, h, generator=gen) * 0.02).to(DT[dn]).to(DEV)
    elif kind == 'non_contiguous':
        x = (torch.randn(rows, 2 * h, generator=gen) * 0.02).to(DT[dn]).to(DEV)[:, :h]
        assert not x.is_contiguous()
    else:                          # one chunk longer than the cap
        h = MAX_C * 8 + 8
        x = (torch.randn(rows, h, generator=gen) * 0.02).to(DT[dn]).to(DEV)
    grad = torch.randn(rows, h, generator=gen).to(DT[dn]).to(DEV)
    got = module_step(x, bits, False, grad)
    assert len(fused_calls) == 0
    assert tuple(got[0].shape) == (rows, h) and tuple(got[1].shape) == tuple(got[2].shape) == (rows, 1)
    got = (got[0].contiguous(), got[1], got[2], got[3].contiguous())
    compare(got, per_channel_step(x, bits, False, grad), x.contiguous(), grad, h, bits, dn)


# ---- routing --------------------------------------------------------------------------------------------------------

def test_a_row_that_is_a_group_size_takes_the_group_kernels(fused_calls, monkeypatch):
    group_calls = _counter(monkeypatch, 'group_shifted_fwd')
    gen = torch.Generator().manual_seed(9)
    x = (torch.randn(3, 5, 128, generator=gen) * 0.02).to(torch.bfloat16).to(DEV)
    grad = torch.randn(3, 5, 128, generator=gen).to(torch.bfloat16).to(DEV)
    got = module_step(x, 8, False, grad)
    assert len(group_calls) == 1 and len(fused_calls) == 0
    assert tuple(got[1].shape) == tuple(got[2].shape) == (3, 5, 1)
    compare(got, per_channel_step(x, 8, False, grad), x, grad, 128, 8, 'bf16')


def test_the_symmetric_per_row_quantizer_is_the_per_channel_weight_route(monkeypatch):
    import brevitas_amd.quant as Q
    stats_calls = _counter(monkeypatch, 'stats_fakequant_fwd')
    gen = torch.Generator().manual_seed(10)
    x = (torch.randn(33, 536, generator=gen) * 0.02).to(torch.bfloat16).to(DEV)
    grad = torch.randn(33, 536, generator=gen).to(torch.bfloat16).to(DEV)
    got = module_step(x, 8, False, grad, make=Q.Int8DynamicActPerRowFloat)
    assert len(stats_calls) == 1
    # the weight quantizer with the dynamic quantizer's clamp and range (plain, not narrow)
    w = torch.nn.Parameter(x.clone())
    q = set_clamp(Q.Int8WeightPerChannelFloat(w).to(DEV), False)
    q.int_quant.narrow_range = False
    q.int_scaling_impl.narrow_range = False
    want = step(q, w, grad)
    assert tuple(got[1].shape) == (33, 1) and got[2].dim() == 0
    for a, b, name in zip(got, want, ('y', 'scale', 'zp', 'dx')):
        assert torch.equal(a.reshape(-1), b.reshape(-1)), name


@pytest.mark.parametrize('shifted', [False, True], ids=['symmetric', 'asymmetric'])
def test_the_per_group_quantizers_are_the_weight_group_quantizers(shifted, fused_calls):
    import brevitas_amd.quant as Q
    gen = torch.Generator().manual_seed(12)
    x = (torch.randn(9, 192, generator=gen) * 0.02).to(torch.bfloat16).to(DEV)
    grad = torch.randn(9, 192, generator=gen).to(torch.bfloat16).to(DEV)
    make = functools.partial(Q.ShiftedUint8DynamicActPerGroupFloat if shifted else Q.Int8DynamicActPerGroupFloat,
                             group_size=64)
    got = module_step(x, 8, False, grad, make=make)
    w = torch.nn.Parameter(x.clone())
    weight_quant = Q.ShiftedUint8WeightPerGroupFloat if shifted else Q.Int8WeightPerGroupFloat
    q = set_clamp(weight_quant(w, group_size=64).to(DEV), False)
    if not shifted:
        q.int_quant.narrow_range = False
        q.int_scaling_impl.narrow_range = False
    want = step(q, w, grad)
    assert len(fused_calls) == 0 and tuple(got[1].shape) == (9, 3, 1)
    for a, b, name in zip(got, want, ('y', 'scale', 'zp', 'dx')):
        assert torch.equal(a.reshape(-1), b.reshape(-1)), name


# ---- guard elements -------------------------------------------------------------------------------------------------

@dtypes
def test_guard_elements_behind_every_output_are_untouched(dn):
    """67 chunks per row, 7 rows: a ragged second wave load and a workgroup with one idle wave; every output lies in a
    buffer with 64 sentinel elements behind it"""
    from brevitas_amd import _native as nat
    from brevitas_amd.core.quant import _fused
    rows, pad = 7, 64
    x, grad, gscale, gzp = make_input(67, rows, dn)
    n = x.numel()
    desc, thr_div = _fused.row_shifted_call(x, 15.0, 0.0, 15.0, False)
    assert nat.row_shifted_supported(desc, x)
    want = nat.row_shifted_fwd(desc, x, 1e-10, thr_div)
    want_dx = nat.row_shifted_bwd(desc, grad, x, want[3], gscale, gzp, 1e-10, thr_div)
    sentinel = 77.0
    sizes = (('y', n), ('scale', rows), ('zp', rows), ('stat', 2 * rows), ('dx', n))
    bufs = {name: torch.full((size + pad,), sentinel, dtype=DT[dn], device=DEV) for name, size in sizes}
    args = nat._scale_args(1e-10, thr_div)
    nat._launch(x.device, 'bvq_row_shifted_fwd', None, ctypes.byref(desc), nat.ptr(x), *args, nat.ptr(bufs['y']),
                nat.ptr(bufs['scale']), nat.ptr(bufs['zp']), nat.ptr(bufs['stat']))
    nat._launch(x.device, 'bvq_row_shifted_bwd', None, ctypes.byref(desc), nat.ptr(grad), nat.ptr(x),
                nat.ptr(bufs['stat']), nat.ptr(gscale), nat.ptr(gzp), *args, nat.ptr(bufs['dx']))
    torch.cuda.synchronize()
    for (name, size), ref in zip(sizes, tuple(want) + (want_dx,)):
        assert_same_bits(bufs[name][:size], ref.reshape(-1), dn, name)
        assert bool((bufs[name][size:] == sentinel).all()), name


# ---- graph capture --------------------------------------------------------------------------------------------------

def test_step_in_a_graph(fused_calls):
    import brevitas_amd.quant as Q
    from test_gpu_graphs import _capture
    torch.manual_seed(123456)
    x = (torch.randn(4, 8, 1072, device=DEV) * 0.1).to(torch.bfloat16).requires_grad_(True)
    g = torch.randn(4, 8, 1072, device=DEV).to(torch.bfloat16)
    q = Q.ShiftedUint8DynamicActPerRowFloat().to(DEV)

    def one():
        x.grad = None
        y, scale, zp, _ = q(x)
        y.backward(g)
        return y, scale, zp, x.grad

    graph, static = _capture(one)
    assert len(fused_calls) == 4
    with torch.no_grad():
        x.mul_(1.5).add_(0.01)  # new values in the captured input
    graph.replay()
    torch.cuda.synchronize()
    got = [t.clone() for t in static]
    for a, b in zip(got, one()):
        assert torch.equal(a, b)


# ---- a layer --------------------------------------------------------------------------------------------------------

def test_quant_linear_with_a_per_token_input_quantizer(fused_calls, monkeypatch):
    """QuantLinear(1072, 64) with 4-bit group-wise weights and the asymmetric per-token input quantizer on a
    [3, 5, 1072] bfloat16 input: one row-kernel call per forward; output, input gradient and weight gradient against
    the same layer with the fused routes off"""
    import brevitas_amd.config as config
    import brevitas_amd.quant as Q
    from brevitas_amd.nn import QuantLinear
    torch.manual_seed(0)
    lin = QuantLinear(1072, 64, weight_quant=functools.partial(Q.Int4WeightPerGroupFloat, group_size=16),
                      input_quant=Q.ShiftedUint8DynamicActPerRowFloat(), device=DEV, dtype=torch.bfloat16)
    x0 = torch.randn(3, 5, 1072, device=DEV).to(torch.bfloat16)
    gout = torch.randn(3, 5, 64, device=DEV).to(torch.bfloat16)

    def run():
        lin.zero_grad(set_to_none=True)
        x = x0.clone().requires_grad_(True)
        out = lin(x)
        out.backward(gout)
        return out.detach(), x.grad.detach(), lin.weight.grad.detach().clone()
    out, dx, dw = run()
    assert len(fused_calls) == 1
    monkeypatch.setattr(config, 'FUSED_PATHS', False)
    out2, dx2, dw2 = run()
    assert len(fused_calls) == 1
    assert torch.equal(out, out2)
    # the gradient arriving at the quantized input, and the quantizer's scale and zero-point, for the bars on dx
    xq, scale, zp, _ = lin.input_quant(x0)
    wq = lin.quant_weight()[0].detach()
    gin = gout.reshape(-1, 64) @ wq
    compare((xq, scale, zp, dx.reshape(15, 1072)), (xq, scale, zp, dx2.reshape(15, 1072)), x0.reshape(15, 1072),
            gin, 1072, 8, 'bf16')
    # the weight gradient: both runs feed the weight quantizer's backward the same bits (gout^T @ xq, xq bit-equal); its
    # own fused and composed routes differ at the first arg-max of each weight group alone, by the rule of
    # tests/test_group_quant_golden.py
    from test_group_quant_golden import SUM_RTOL, first_argmax_positions
    bad = torch.nonzero(dw.reshape(-1).view(torch.int16) != dw2.reshape(-1).view(torch.int16)).reshape(-1).tolist()
    assert set(bad) <= first_argmax_positions(lin.weight, 16)
    bound = SUM_RTOL['bf16'] * 64 * max(1.0, float(dw2.float().abs().max()))
    assert all(abs(float(dw.reshape(-1)[i]) - float(dw2.reshape(-1)[i])) <= bound for i in bad)
