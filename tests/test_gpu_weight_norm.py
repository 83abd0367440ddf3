"""Weight-norm and accumulator-aware (A2Q) weight quantizers on the device: the row kernels of csrc/bvq_weight_norm.hip at
every geometry, the routing, the overflow bound, guard elements and graph capture.  tests/weight_norm_ref.py restates
the semantics on torch CPU ops and derives every bound used here, once.

Bars.  n: relative error <= (K + 4) 2^-24 against the float64 norm.  y: given the kernel's own n, the bits of the float32
chain on torch CPU ops, no element excepted.  ds, dg, dv: the bounds of weight_norm_ref (A is observed alone through
dg = s A / g', and B through ds = B - A).  Two runs: the same bits.
"""
import ctypes
import functools

import pytest
import torch

import weight_norm_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
DT = {'f32': torch.float32, 'bf16': torch.bfloat16, 'f16': torch.float16}
SIZE = {'f32': 4, 'bf16': 2, 'f16': 2}
MAX_C = 2048
# (16-byte chunks per row C, rows): the two sides of each geometry boundary (128 | 129, 512 | 513), ragged last waves
# (5, 67, 1376), the shortest and the longest row, and one case with a single row
SHAPES = [(1, 13), (5, 11), (67, 12), (128, 12), (129, 12), (512, 12), (513, 12), (1376, 11), (MAX_C, 10), (67, 1)]
shapes = pytest.mark.parametrize('chunks,rows', SHAPES, ids=['C%d-r%d' % s for s in SHAPES])
dtypes = pytest.mark.parametrize('dn', ['f32', 'bf16', 'f16'])
norms = pytest.mark.parametrize('norm', ['l1', 'l2'])
QMAX = 127.0


def kind_of(norm):
    from brevitas_amd import _native as nat
    return nat.NORM_L1 if norm == 'l1' else nat.NORM_L2


def desc_of(x, norm, clamp_ste):
    from brevitas_amd import _native as nat
    from brevitas_amd.core.quant import _fused
    return _fused.weight_norm_call(x, QMAX, nat.ROUND_TO_ZERO if norm == 'l1' else nat.ROUND, clamp_ste)


@functools.lru_cache(maxsize=None)
def case(chunks, rows, dn, norm, clamp_ste=False):
    """inputs on the CPU, the kernels' outputs (copied to the CPU) and the references, computed once per case and left
    unchanged.  Rows, as many as there are: 0 all zero, 1 constant, 2 +absmax at the first position, 3 -absmax at the
    last, 4 with g > T s (capped), 5 with g == T s exactly (the tie); the others have g = n * (0.6 .. 1.5), so some of
    their values clip.  T is twice the largest g / s before rows 4 and 5 are planted."""
    k = chunks * 16 // SIZE[dn]
    gen = torch.Generator().manual_seed(1000 * chunks + rows)
    v = (torch.randn(rows, k, generator=gen) * 0.02).to(DT[dn])
    if rows > 1:
        v[0] = 0.0
        v[1] = 0.015625
    if rows > 2:
        v[2, 0] = (v[2].float().abs().max() * 1.25).to(DT[dn])
    if rows > 3:
        v[3, k - 1] = -(v[3].float().abs().max() * 1.25).to(DT[dn])
    absmax = v.float().abs().max(1).values
    s = torch.clamp_min(absmax, 1e-10) / QMAX
    n0 = torch.clamp_min(R.norm64(v, norm), 1e-10).float()
    g = n0 * (0.6 + 0.9 * torch.rand(rows, generator=gen))
    T = float((2.0 * (g / s).max()).float())
    if rows > 4:
        g[4] = 3.0 * T * s[4]
    if rows > 5:
        g[5] = torch.tensor(T) * s[5]
    gy = torch.randn(rows, k, generator=gen).to(DT[dn])
    out = dict(k=k, v=v, s=s, g=g, gy=gy, T=T, dn=dn, norm=norm, clamp_ste=clamp_ste, chunks=chunks, rows=rows)
    out.update(run_kernels(out))
    out['again'] = [run_kernels(out)[name] for name in OUTPUTS]
    out['ref'] = R.closed_forms(v, s, g, gy, out['n'], T, QMAX, norm, clamp_ste)
    return out


OUTPUTS = ('y', 'n', 'dv', 'ds', 'dg')


def run_kernels(c, v=None):
    """one forward and one backward launch on the inputs of the case `c` (v: another weight in the place of c['v'])
    through the library brevitas_amd._native stands on at the time of the call -> the five outputs, copied to the CPU"""
    from brevitas_amd import _native as nat
    norm = c['norm']
    xd, sd, gd, gyd = ((c['v'] if v is None else v).to(DEV), c['s'].to(DEV), c['g'].to(DEV), c['gy'].to(DEV))
    desc = desc_of(xd, norm, c['clamp_ste'])
    assert nat.weight_norm_supported(desc, kind_of(norm), c['T'], R.NORM_MIN, xd)
    y, n = nat.weight_norm_fwd(desc, kind_of(norm), c['T'], R.NORM_MIN, xd, sd, gd)
    dv, ds, dg = nat.weight_norm_bwd(desc, kind_of(norm), c['T'], R.NORM_MIN, gyd, xd, sd, gd, n)
    torch.cuda.synchronize()
    return dict(zip(OUTPUTS, (t.cpu() for t in (y, n, dv, ds, dg))))


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


# ---- the bars, stated once: `c` is a case, or a case whose outputs were replaced by those of another run -------------

def check_norm(c, tag='WEIGHT_NORM n'):
    """|n - n64| <= (K + 4) 2^-24 n64: every term of the sum is non-negative, so the bound holds for any order of the
    additions (weight_norm_ref, "Norm"); a norm below norm_min is reported as norm_min"""
    n64 = R.norm64(c['v'], c['norm'])
    nmin = float(torch.tensor(R.NORM_MIN, dtype=torch.float32))
    want = torch.where(n64 > nmin, n64, torch.full_like(n64, nmin))
    err = (c['n'].double() - want).abs() / want
    print('%s %s %s C=%d rows=%d worst=%.3g of %.3g' % (tag, c['dn'], c['norm'], c['chunks'], c['rows'], float(err.max()),
                                                        (c['k'] + 4) * R.U))
    assert bool((err <= (c['k'] + 4) * R.U).all())
    if c['rows'] > 1:
        assert float(c['n'][0]) == nmin


def check_forward(c):
    """given the kernel's own n, the bits of the float32 chain on torch CPU ops, no element excepted"""
    want = R.forward_from_n(c['v'], c['s'], c['g'], c['n'], c['T'], QMAX, c['norm'])
    assert torch.equal(bits(c['y']), bits(want))
    assert not torch.isnan(c['y'].float()).any()
    if c['rows'] > 1:
        assert float(c['y'][0].float().abs().max()) == 0.0                       # the all-zero row


def check_backward(c, tag='WEIGHT_NORM bwd'):
    """ds, dg and dv within the bounds of weight_norm_ref against c['ref'], the closed forms at c['n']"""
    ref, k, dt = c['ref'], c['k'], DT[c['dn']]
    for name in ('ds', 'dg', 'dv'):
        assert torch.isfinite(c[name].float()).all(), name
    ds_err = (c['ds'].double() - ref['ds']).abs()
    ds_bound = R.sum_bound(k) * (ref['SA'] + ref['SB'])
    dg_err = (c['dg'].double() - ref['dg']).abs()
    dg_bound = ref['s_over_gp'] * R.sum_bound(k) * ref['SA']
    dv_err = (c['dv'].double() - ref['dv']).abs()
    dv_bound = R.dv_bound(ref, k, dt)
    print('%s %s %s C=%d rows=%d ds %.3g dg %.3g dv %.3g (worst share of the bound)'
          % (tag, c['dn'], c['norm'], c['chunks'], c['rows'], float((ds_err / ds_bound.clamp_min(1e-300)).max()),
             float((dg_err / dg_bound.clamp_min(1e-300)).max()), float((dv_err / dv_bound.clamp_min(1e-300)).max())))
    assert bool((ds_err <= ds_bound).all())
    assert bool((dg_err <= dg_bound).all())
    assert bool((dv_err <= dv_bound).all())
    if c['rows'] > 4:
        assert float(c['dg'][4]) == 0.0                                          # capped: g gets nothing
    if c['rows'] > 5:
        assert float(c['dg'][5]) != 0.0                                          # the tie: g gets it
    if c['rows'] > 1:
        # the all-zero row: n was clamped, no gradient through the norm: dv = gy * g' / n, rounded once
        want0 = (c['gy'][0].double() * (c['g'][0].double() / c['n'][0].double()))
        assert bool(((c['dv'][0].double() - want0).abs() <= 3 * R.U * want0.abs() + R.half_ulp(want0, dt) * 1.01).all())


# ---- the kernels at every geometry ----------------------------------------------------------------------------------

@shapes
@dtypes
@norms
def test_norm_against_float64(chunks, rows, dn, norm):
    """|n - n64| <= (K + 4) 2^-24 n64: every term of the sum is non-negative, so the bound holds for any order of the
    additions (weight_norm_ref, "Norm"); a norm below norm_min is reported as norm_min"""
    check_norm(case(chunks, rows, dn, norm))


@shapes
@dtypes
@norms
def test_forward_has_the_bits_of_the_float32_chain(chunks, rows, dn, norm):
    c = case(chunks, rows, dn, norm)
    check_forward(c)
    if rows > 1:
        t, r, q, gp, capped, p = R.chain(c['v'], c['s'], c['g'], c['n'], c['T'], QMAX, norm)
        assert capped.reshape(-1)[:6].tolist() == [False, False, False, False, True, False]   # the tie goes to g
        assert float(q.abs().max()) == QMAX                                      # something sits at the clamp


@shapes
@dtypes
@norms
def test_backward_within_the_bounds(chunks, rows, dn, norm):
    check_backward(case(chunks, rows, dn, norm))


@shapes
@dtypes
@norms
def test_two_runs_give_the_same_bits(chunks, rows, dn, norm):
    c = case(chunks, rows, dn, norm)
    for a, b in zip((c['y'], c['n'], c['dv'], c['ds'], c['dg']), c['again']):
        assert torch.equal(bits(a), bits(b))


@dtypes
@norms
def test_straight_through_clamp(dn, norm):
    """clamp_ste: clipped elements pass their gradient too"""
    c, plain = case(67, 12, dn, norm, True), case(67, 12, dn, norm, False)
    ref, k = c['ref'], c['k']
    assert bool(((c['dv'].double() - ref['dv']).abs() <= R.dv_bound(ref, k, DT[dn])).all())
    assert bool(((c['ds'].double() - ref['ds']).abs() <= R.sum_bound(k) * (ref['SA'] + ref['SB'])).all())
    assert bool(((c['dg'].double() - ref['dg']).abs() <= ref['s_over_gp'] * R.sum_bound(k) * ref['SA']).all())
    assert torch.equal(bits(c['y']), bits(plain['y']))
    assert not torch.equal(bits(c['dv']), bits(plain['dv']))   # something was clipped, and its gradient differs


# ---- end to end -----------------------------------------------------------------------------------------------------

def build_pair(shape, dn, make, seed, g_factor=1.0):
    """the same quantizer on the device and on the CPU, float32 parameters, the same weight"""
    gen = torch.Generator().manual_seed(seed)
    w0 = (torch.randn(shape, generator=gen) * 0.03).to(DT[dn])
    wc, wd = torch.nn.Parameter(w0.clone()), torch.nn.Parameter(w0.clone().to(DEV))
    qc = make(wc)
    qd = make(wd).to(DEV)
    with torch.no_grad():
        qc.pre_scaling_impl.value.mul_(g_factor)
        qd.pre_scaling_impl.value.copy_(qc.pre_scaling_impl.value)
        qd.scaling_impl.value.copy_(qc.scaling_impl.value)
    return qc, wc, qd, wd


def compare_codes(qc, wc, yc, qd, yd, norm):
    """Codes of the device module against the composed route on the CPU.  Both compute t = v g' / (s n) with a relative
    error of at most (K + 4) 2^-24 (the norm's sum (K - 1), s n, the division by g' and v / p one each), so their codes
    can differ only where the float64 t, from the float32 values of s and g, lies within |t| (K + 4) 2^-24 of a point
    where R changes its value -- an integer for round-to-zero, an odd multiple of 1/2 for half-even rounding -- and
    then by one.  The share of such elements may not exceed 2 %."""
    rows = wc.shape[0]
    v = wc.detach().reshape(rows, -1)
    k = v.shape[1]
    s = qc.scaling_impl(wc).detach().reshape(-1).double()
    g = qc.pre_scaling_impl(wc).detach().reshape(-1).double()
    T = qc.pre_scaling_impl.upper_bound()
    n64 = torch.clamp_min(R.norm64(v, norm), R.NORM_MIN)
    gp = torch.minimum(g, T * s)
    t64 = v.double() * (gp / (s * n64)).reshape(-1, 1)
    edge = t64 if norm == 'l1' else t64 - 0.5
    near = (edge - torch.round(edge)).abs() <= t64.abs() * (k + 4) * R.U
    cc = torch.round(yc.detach().reshape(rows, -1).double() / s.reshape(-1, 1))
    cd = torch.round(yd.detach().cpu().reshape(rows, -1).double() / s.reshape(-1, 1))
    diff = (cc - cd).abs()
    share = float(near.double().mean())
    print('WEIGHT_NORM e2e %s K=%d near %.4f differing %d' % (norm, k, share, int((diff != 0).sum())))
    assert share <= 0.02
    assert bool((diff[~near] == 0).all()) and bool((diff <= 1).all())
    # and the dequantized values are those codes times the scale
    same = diff == 0
    assert torch.equal(yc.detach().reshape(rows, -1)[same].float(), yd.detach().cpu().reshape(rows, -1)[same].float())


@pytest.fixture
def launches(monkeypatch):
    from brevitas_amd import _native as nat
    calls = {'fwd': 0, 'bwd': 0}
    for key in calls:
        real = getattr(nat, 'weight_norm_' + key)

        def counted(*a, _real=real, _key=key, **kw):
            calls[_key] += 1
            return _real(*a, **kw)
        monkeypatch.setattr(nat, 'weight_norm_' + key, counted)
    return calls


@pytest.mark.parametrize('shape', [(24, 1024), (16, 256), (12, 8, 3, 3)], ids=['K1024', 'K256', 'conv-K72'])
@pytest.mark.parametrize('dn', ['f32', 'bf16'])
@norms
def test_module_on_the_device_against_the_composed_route_on_the_cpu(shape, dn, norm, launches):
    import brevitas_amd.quant as Q
    make = functools.partial(Q.Int8AccumulatorAwareWeightQuant, accumulator_bit_width=24) if norm == 'l1' \
        else Q.Int8WeightNormL2PerChannelFloat
    qc, wc, qd, wd = build_pair(shape, dn, make, 77)
    yc, sc, _, _ = qc(wc)
    yd, sd, zp, bw = qd(wd)
    assert launches == {'fwd': 1, 'bwd': 0}
    assert yd.dtype == DT[dn] and yd.shape == wd.shape and tuple(sd.shape) == (shape[0],) + (1,) * (len(shape) - 1)
    assert torch.equal(sd.cpu(), sc) and float(zp) == 0.0 and float(bw) == 8.0
    compare_codes(qc, wc, yc, qd, yd, norm)
    gen = torch.Generator().manual_seed(5)
    gy = torch.randn(shape, generator=gen).to(DT[dn])
    yc.backward(gy)
    yd.backward(gy.to(DEV))
    assert launches == {'fwd': 1, 'bwd': 1}            # exactly one launch each way
    for a, b, name in ((wd.grad, wc.grad, 'dv'), (qd.scaling_impl.value.grad, qc.scaling_impl.value.grad, 'ds'),
                       (qd.pre_scaling_impl.value.grad, qc.pre_scaling_impl.value.grad, 'dg')):
        assert a is not None and a.shape == b.shape and torch.isfinite(a.float()).all(), name


# ---- routing --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('kind', ['too_long', 'ragged_row', 'misaligned'])
def test_refusals_take_the_composed_route_on_the_device(kind, launches):
    import brevitas_amd.quant as Q
    make = functools.partial(Q.Int8AccumulatorAwareWeightQuant, accumulator_bit_width=24)
    dn = 'bf16'
    if kind == 'too_long':          # 32 KiB + 16 bytes per row
        shape = (3, MAX_C * 8 + 8)
    elif kind == 'ragged_row':      # 24 bytes per row
        shape = (6, 12)
    else:
        shape = (6, 256)
    # (g = 0.93 n: the largest element of a row then sits at t = 118.1, not exactly on the integer 127, which in a row
    # of 12 elements would alone put 8 % of them in the band)
    qc, wc, qd, wd = build_pair(shape, dn, make, 31, g_factor=0.93)
    xd = wd
    if kind == 'misaligned':        # a view of the weight starting 2 bytes off a 16-byte boundary
        base = torch.zeros(wd.numel() + 8, dtype=DT[dn], device=DEV)
        xd = base[1:1 + wd.numel()].view(shape)
        with torch.no_grad():
            xd.copy_(wd)
        xd.requires_grad_(True)
        assert xd.data_ptr() % 16 == 2 and xd.is_contiguous()
    yc = qc(wc)[0]
    yd = qd(xd)[0]
    yd.sum().backward()
    assert launches == {'fwd': 0, 'bwd': 0}
    assert torch.isfinite(xd.grad.float()).all()
    # the end-to-end rule (the row of 16392 elements has its g capped at T s, so its |t| and with them the band are
    # small: 0.07 % of its elements lie inside)
    compare_codes(qc, wc, yc, qd, yd, 'l1')


# ---- overflow bound -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('acc,n_in,signed,wbits', [(16, 8, False, 8), (12, 4, True, 4), (32, 8, False, 8)])
def test_the_kernel_s_codes_respect_the_accumulator_bound(acc, n_in, signed, wbits, launches):
    import brevitas_amd.quant as Q
    make = functools.partial(Q.Int8AccumulatorAwareWeightQuant, accumulator_bit_width=acc, input_bit_width=n_in,
                             input_signed=signed, bit_width=wbits)
    qc, wc, qd, wd = build_pair((12, 256), 'f32', make, acc, g_factor=8.0)
    yd, sd, _, _ = qd(wd)
    assert launches['fwd'] == 1
    T = qd.pre_scaling_impl.upper_bound()
    codes = torch.round(yd.detach().double() / sd.detach().double()).reshape(12, -1)
    assert torch.equal((codes * sd.detach().double().reshape(-1, 1)).float(), yd.detach().reshape(12, -1))
    sums = codes.abs().sum(1)
    assert int(codes.abs().max()) <= 2 ** (wbits - 1) - 1
    assert bool((sums <= T).all()), (float(sums.max()), T)
    capped = (qd.pre_scaling_impl(wd).reshape(-1) > T * sd.reshape(-1))
    assert bool(capped.all()) if acc < 32 else not bool(capped.any())
    assert bool((qd.int_weight(wd).reshape(12, -1).double().abs().sum(1) <= T).all())


# ---- guard elements -------------------------------------------------------------------------------------------------

@dtypes
@norms
def test_guard_elements_behind_every_output_are_untouched(dn, norm):
    """67 chunks per row, 7 rows: a ragged second wave load and a workgroup with one idle wave; every output lies in a
    buffer with 64 sentinel elements behind it"""
    from brevitas_amd import _native as nat
    c = case(67, 12, dn, norm)
    rows, pad, sentinel = 7, 64, 77.0
    v, s, g, gy = (c[name][:rows].contiguous().to(DEV) for name in ('v', 's', 'g', 'gy'))
    n_el = v.numel()
    desc = desc_of(v, norm, False)
    y, n = nat.weight_norm_fwd(desc, kind_of(norm), c['T'], R.NORM_MIN, v, s, g)
    dv, ds, dg = nat.weight_norm_bwd(desc, kind_of(norm), c['T'], R.NORM_MIN, gy, v, s, g, n)
    sizes = (('y', n_el, DT[dn]), ('n', rows, torch.float32), ('dv', n_el, DT[dn]), ('ds', rows, torch.float32),
             ('dg', rows, torch.float32))
    bufs = {name: torch.full((size + pad,), sentinel, dtype=dt, device=DEV) for name, size, dt in sizes}
    args = (ctypes.byref(desc), int(kind_of(norm)), float(c['T']), R.NORM_MIN)
    nat._launch(v.device, 'bvq_weight_norm_fwd', None, *args, nat.ptr(v), nat.ptr(s), nat.ptr(g), nat.ptr(bufs['y']),
                nat.ptr(bufs['n']))
    nat._launch(v.device, 'bvq_weight_norm_bwd', None, *args, nat.ptr(gy), nat.ptr(v), nat.ptr(s), nat.ptr(g),
                nat.ptr(bufs['n']), nat.ptr(bufs['dv']), nat.ptr(bufs['ds']), nat.ptr(bufs['dg']))
    torch.cuda.synchronize()
    for (name, size, _), ref in zip(sizes, (y, n, dv, ds, dg)):
        assert torch.equal(bits(bufs[name][:size]), bits(ref.reshape(-1))), name
        assert bool((bufs[name][size:] == sentinel).all()), name
    assert torch.equal(bits(y.cpu()), bits(c['y'][:rows]))   # a row's result does not depend on the rows beside it


# ---- graph capture --------------------------------------------------------------------------------------------------

def test_training_step_in_a_graph(launches):
    """one training step of QuantLinear(256, 64) with the A2Q weight quantizer, captured on a single stream (the step
    has no parallel branches), replays to the eager bits"""
    import brevitas_amd.quant as Q
    from brevitas_amd.nn import QuantLinear
    from test_gpu_graphs import _capture
    torch.manual_seed(2468)
    lin = QuantLinear(256, 64, weight_quant=functools.partial(Q.Int8AccumulatorAwareWeightQuant,
                                                              accumulator_bit_width=16), device=DEV)
    x = torch.rand(8, 256, device=DEV)
    gout = torch.randn(8, 64, device=DEV)
    params = [lin.weight, lin.bias, lin.weight_quant.scaling_impl.value, lin.weight_quant.pre_scaling_impl.value]

    def one():
        for p in params:
            p.grad = None
        out = lin(x)
        out.backward(gout)
        return (out,) + tuple(p.grad for p in params)

    graph, static = _capture(one)
    assert launches == {'fwd': 4, 'bwd': 4}
    with torch.no_grad():
        x.mul_(0.5).add_(0.1)          # new values in the captured input
        lin.weight.mul_(1.1)
    graph.replay()
    torch.cuda.synchronize()
    got = [t.clone() for t in static]
    for a, b in zip(got, one()):
        assert torch.equal(a, b)
