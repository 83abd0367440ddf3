"""The row walk (csrc/bvq_row_walk.h) where its own suites do not reach: every NT = true instantiation of the asymmetric
per-token kernels (csrc/bvq_row_shifted.hip) and of the weight-norm / A2Q kernels (csrc/bvq_weight_norm.hip), through the
forced-NT build of the library (brevitas_amd/libbvq_nt0.so, made by __graft_entry__.build()); the guard elements behind
every output under NT; and the rows of a weight that are not finite.

No bar of its own.  NT against the default library: bit for bit, every output.  Per-token kernels: compare of
test_gpu_dynamic_act.py against the per-channel route.  Weight-norm: the bars of test_gpu_weight_norm.py, derived in
weight_norm_ref.py -- the norm against float64, the forward bits from the kernel's own n, the backward bounds.
"""
import ctypes

import pytest
import torch

import test_gpu_dynamic_act as DA
import test_gpu_weight_norm as WN
import weight_norm_ref as R
from test_group_walk_host import NT_BYTES
from test_gpu_group_walk import use_nt0  # noqa: F401  (the fixture that switches to the forced-NT library)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
DT = WN.DT
# (16-byte chunks per row C, rows): one ragged case per geometry -- C = 129 leaves whole waves of the row past its end
# (wave 3 starts at chunk 192) -- and the longest row
SHAPES = [(67, 11), (129, 5), (1376, 5), (2048, 2)]
shapes = pytest.mark.parametrize('chunks,rows', SHAPES, ids=['C%d-r%d' % s for s in SHAPES])
dtypes = pytest.mark.parametrize('dn', ['f32', 'bf16', 'f16'])
norms = pytest.mark.parametrize('norm', ['l1', 'l2'])
BITS = 4


def nat():
    from brevitas_amd import _native
    return _native


@pytest.fixture
def launches(monkeypatch):
    """name -> the non-temporal threshold of the library each launch of the four row wrappers went to, call by call"""
    n = nat()
    calls = {}
    for name in ('row_shifted_fwd', 'row_shifted_bwd', 'weight_norm_fwd', 'weight_norm_bwd'):
        real = getattr(n, name)
        calls[name] = []

        def counted(*a, _real=real, _name=name, **k):
            calls[_name].append(int(n.lib.bvq_nt_threshold_bytes()))
            return _real(*a, **k)
        monkeypatch.setattr(n, name, counted)
    return calls


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(WN.bits(a), WN.bits(b)))


# ---- the NT instantiations ------------------------------------------------------------------------------------------

def token_step(x, grad, gscale, gzp, ste):
    """forward and backward through the Function, and the statistics of one more forward launch
    -> (y, scale, zp, dx, stat)"""
    from brevitas_amd.core.quant import _fused
    out = DA.row_step(x, BITS, ste, grad, gscale, gzp)
    desc, thr_div = _fused.row_shifted_call(x, 2.0 ** BITS - 1, 0.0, 2.0 ** BITS - 1, ste)
    assert nat().row_shifted_supported(desc, x)
    return out + (nat().row_shifted_fwd(desc, x, 1e-10, thr_div)[3],)


@shapes
@dtypes
def test_row_shifted_nt(chunks, rows, dn, use_nt0, launches):
    """row_shifted_fwd / _bwd_kernel<T, kW, kD, true> of the geometry of C, both clamp modes, with gradients arriving
    through scale and zero-point"""
    x, grad, gscale, gzp = DA.make_input(chunks, rows, dn)
    h = x.shape[1]
    modes = (True, False)
    assert nat().lib.bvq_nt_threshold_bytes() == NT_BYTES == 256 << 20
    plain = [token_step(x, grad, gscale, gzp, ste) for ste in modes]
    # the reference route runs on the default library: the per-channel kernels' NT variants are not the subject
    refs = [DA.per_channel_step(x, BITS, ste, grad, gscale, gzp) for ste in modes]
    assert launches['row_shifted_fwd'] == [NT_BYTES] * 4 and launches['row_shifted_bwd'] == [NT_BYTES] * 2
    use_nt0()
    assert nat().lib.bvq_nt_threshold_bytes() == 0
    worst = 0.0
    for ste, want, ref in zip(modes, plain, refs):
        out = token_step(x, grad, gscale, gzp, ste)
        for a, b, what in zip(out, want, ('y', 'scale', 'zp', 'dx', 'stat')):
            assert same_bits(a, b), '%s of the NT kernel differs from the default library (ste=%d)' % (what, ste)
        worst = max(worst, DA.compare(out[:4], ref, x, grad, h, BITS, dn, gscale, gzp))
    assert launches['row_shifted_fwd'] == [NT_BYTES] * 4 + [0] * 4 and launches['row_shifted_bwd'] == [NT_BYTES] * 2 + [0] * 2
    print('ROW_WALK_NT ROW_SHIFTED_DEPOSIT_ULPS %s C=%d rows=%d bits=%d worst=%.3f' % (dn, chunks, rows, BITS, worst))


WN_CASES = [(c, r, False) for c, r in SHAPES] + [(67, 11, True)]


@pytest.mark.parametrize('chunks,rows,clamp_ste', WN_CASES, ids=['C%d-r%d-ste%d' % c for c in WN_CASES])
@dtypes
@norms
def test_weight_norm_nt(chunks, rows, clamp_ste, dn, norm, use_nt0, launches):
    """weight_norm_fwd / _bwd_kernel<T, kNorm, kW, kD, true> of the geometry of C on the planted rows of the case, as
    many as there are: zero, constant, the extremes at both ends, capped, the tie"""
    assert nat().lib.bvq_nt_threshold_bytes() == NT_BYTES == 256 << 20
    c = WN.case(chunks, rows, dn, norm, clamp_ste)      # its inputs, and the references at the default library's n
    plain = WN.run_kernels(c)
    assert launches['weight_norm_fwd'][-1] == launches['weight_norm_bwd'][-1] == NT_BYTES
    before = len(launches['weight_norm_fwd']), len(launches['weight_norm_bwd'])
    use_nt0()
    assert nat().lib.bvq_nt_threshold_bytes() == 0
    got = WN.run_kernels(c)
    assert launches['weight_norm_fwd'][before[0]:] == [0] and launches['weight_norm_bwd'][before[1]:] == [0]
    for name in WN.OUTPUTS:
        assert same_bits(got[name], plain[name]), '%s of the NT kernel differs from the default library' % name
        assert same_bits(got[name], c[name]), name
    # and the family's own bars on the NT outputs (n has the default library's bits, so c['ref'] is the reference at it)
    nt = dict(c, **got)
    WN.check_norm(nt, 'ROW_WALK_NT WEIGHT_NORM n')
    WN.check_forward(nt)
    WN.check_backward(nt, 'ROW_WALK_NT WEIGHT_NORM bwd')


# ---- guard elements under NT ----------------------------------------------------------------------------------------

@dtypes
def test_guard_elements_behind_every_output_are_untouched_nt(dn, use_nt0):
    """67 chunks per row, 7 rows: a ragged second wave load and a workgroup with one idle wave; every output of both
    families lies in a buffer with 64 sentinel elements behind it.  A lane past the row's end relies on the descriptor to
    drop its store, and the nt bit of the instruction must not change that."""
    from brevitas_amd.core.quant import _fused
    rows, pad, sentinel = 7, 64, 77.0
    # the per-token kernels
    x, grad, gscale, gzp = DA.make_input(67, rows, dn)
    n_el = x.numel()
    desc, thr_div = _fused.row_shifted_call(x, 15.0, 0.0, 15.0, False)
    assert nat().row_shifted_supported(desc, x)
    want = nat().row_shifted_fwd(desc, x, 1e-10, thr_div)
    want_dx = nat().row_shifted_bwd(desc, grad, x, want[3], gscale, gzp, 1e-10, thr_div)
    # the weight-norm kernels, both norms
    c = {norm: WN.case(67, 12, dn, norm) for norm in ('l1', 'l2')}
    use_nt0()
    n = nat()
    assert n.lib.bvq_nt_threshold_bytes() == 0
    sizes = (('y', n_el), ('scale', rows), ('zp', rows), ('stat', 2 * rows), ('dx', n_el))
    bufs = {name: torch.full((size + pad,), sentinel, dtype=DT[dn], device=DEV) for name, size in sizes}
    args = n._scale_args(1e-10, thr_div)
    n._launch(x.device, 'bvq_row_shifted_fwd', None, ctypes.byref(desc), n.ptr(x), *args, n.ptr(bufs['y']),
              n.ptr(bufs['scale']), n.ptr(bufs['zp']), n.ptr(bufs['stat']))
    n._launch(x.device, 'bvq_row_shifted_bwd', None, ctypes.byref(desc), n.ptr(grad), n.ptr(x), n.ptr(bufs['stat']),
              n.ptr(gscale), n.ptr(gzp), *args, n.ptr(bufs['dx']))
    torch.cuda.synchronize()
    for (name, size), ref in zip(sizes, tuple(want) + (want_dx,)):
        DA.assert_same_bits(bufs[name][:size], ref.reshape(-1), dn, name)
        assert bool((bufs[name][size:] == sentinel).all()), name
    for norm in ('l1', 'l2'):
        cc = c[norm]
        v, s, g, gy = (cc[name][:rows].contiguous().to(DEV) for name in ('v', 's', 'g', 'gy'))
        wdesc = WN.desc_of(v, norm, False)
        sizes = (('y', n_el, DT[dn]), ('n', rows, torch.float32), ('dv', n_el, DT[dn]), ('ds', rows, torch.float32),
                 ('dg', rows, torch.float32))
        bufs = {name: torch.full((size + pad,), sentinel, dtype=dt, device=DEV) for name, size, dt in sizes}
        args = (ctypes.byref(wdesc), int(WN.kind_of(norm)), float(cc['T']), R.NORM_MIN)
        n._launch(v.device, 'bvq_weight_norm_fwd', None, *args, n.ptr(v), n.ptr(s), n.ptr(g), n.ptr(bufs['y']),
                  n.ptr(bufs['n']))
        n._launch(v.device, 'bvq_weight_norm_bwd', None, *args, n.ptr(gy), n.ptr(v), n.ptr(s), n.ptr(g),
                  n.ptr(bufs['n']), n.ptr(bufs['dv']), n.ptr(bufs['ds']), n.ptr(bufs['dg']))
        torch.cuda.synchronize()
        for name, size, _ in sizes:
            # a row's result does not depend on the rows beside it: the first 7 rows of the case's 12
            ref = cc[name][:rows].reshape(-1)
            assert same_bits(bufs[name][:size].cpu(), ref), '%s %s' % (norm, name)
            assert bool((bufs[name][size:] == sentinel).all()), '%s %s' % (norm, name)


# ---- weight-norm rows that are not finite ---------------------------------------------------------------------------

def dirty_weight(c):
    """the case's weight with row 9 holding one NaN, row 10 +inf at its last element and row 11 finite values whose norm
    overflows float32 (|v| = 2e19: every square is beyond it; |v| = 3e38: the second term of the sum is)"""
    v, k = c['v'].clone(), c['k']
    gen = torch.Generator().manual_seed(k)
    v[9, k // 3] = float('nan')
    v[10, k - 1] = float('inf')
    sign = torch.where(torch.rand(k, generator=gen) < 0.5, -1.0, 1.0)
    v[11] = (sign * (3e38 if c['norm'] == 'l1' else 2e19)).to(v.dtype)
    assert bool(torch.isfinite(v[11].float()).all()) and bool(torch.isfinite(R.norm64(v, c['norm'])[11]))
    return v


def module_on(v, c):
    """the quantizer module on the device for the weight v, with the case's s and g (T is the module's own: no row from
    9 on is capped under either)"""
    import functools
    import brevitas_amd.quant as Q
    make = functools.partial(Q.Int8AccumulatorAwareWeightQuant, accumulator_bit_width=32) if c['norm'] == 'l1' \
        else Q.Int8WeightNormL2PerChannelFloat
    q = make(torch.nn.Parameter(c['v'].clone())).to(DEV)     # initialised from the clean weight
    q.clamp_ste = False
    with torch.no_grad():
        q.scaling_impl.value.copy_(c['s'].reshape(q.scaling_impl.value.shape))
        q.pre_scaling_impl.value.copy_(c['g'].reshape(q.pre_scaling_impl.value.shape))
    assert bool((c['g'][9:].double() <= min(c['T'], q.pre_scaling_impl.upper_bound()) * c['s'][9:].double()).all())
    return q, torch.nn.Parameter(v.clone().to(DEV))


@pytest.mark.parametrize('chunks', [67, 1376])
@pytest.mark.parametrize('dn', ['f32', 'bf16'])
@norms
def test_weight_norm_rows_that_are_not_finite(chunks, dn, norm, launches, monkeypatch):
    """With one wave per row four rows share a workgroup (C = 67), with one workgroup per row the norm crosses LDS
    (C = 1376).  n = norm > norm_min ? norm : norm_min sends a NaN norm to norm_min; an inf or an overflowing sum gives
    n = inf, p = inf and t = 0 for every finite element.  No other row sees any of it."""
    import brevitas_amd.config as config
    c = WN.case(chunks, 12, dn, norm)
    v = dirty_weight(c)
    got = WN.run_kernels(c, v)
    assert len(launches['weight_norm_fwd']) >= 1 and len(launches['weight_norm_bwd']) >= 1
    nmin = float(torch.tensor(R.NORM_MIN, dtype=torch.float32))
    n = got['n']
    assert float(n[9]) == nmin and float(n[10]) == float('inf') and float(n[11]) == float('inf')
    # forward: the bits of the chain at the kernel's n wherever that is no NaN, NaN exactly where it is one
    want = R.forward_from_n(v, c['s'], c['g'], n, c['T'], WN.QMAX, norm)
    nan = torch.isnan(want.float())
    assert torch.equal(torch.isnan(got['y'].float()), nan)
    assert torch.equal(WN.bits(got['y'])[~nan], WN.bits(want)[~nan])
    assert nan[9].nonzero().reshape(-1).tolist() == [c['k'] // 3] and nan[10].nonzero().reshape(-1).tolist() == [c['k'] - 1]
    assert not nan[:9].any() and not nan[11].any()
    assert float(got['y'][11].float().abs().max()) == 0.0
    # backward: the NaN pattern of the closed forms, the finite entries within the bounds
    ref = R.closed_forms(v, c['s'], c['g'], c['gy'], n, c['T'], WN.QMAX, norm, False)
    k = c['k']
    bounds = {'ds': R.sum_bound(k) * (ref['SA'] + ref['SB']), 'dg': ref['s_over_gp'] * R.sum_bound(k) * ref['SA'],
              'dv': R.dv_bound(ref, k, DT[dn])}
    share = {}
    for name in ('ds', 'dg', 'dv'):
        rnan = torch.isnan(ref[name])
        assert torch.equal(torch.isnan(got[name].float()), rnan), name
        assert not torch.isinf(got[name].float()).any(), name
        err = (got[name].double() - ref[name]).abs()[~rnan]
        assert bool((err <= bounds[name][~rnan]).all()), name
        share[name] = float((err / bounds[name][~rnan].clamp_min(1e-300)).max())
        assert not rnan.reshape(12, -1)[:9].any() and not rnan.reshape(12, -1)[11].any(), name
    assert bool(torch.isnan(ref['ds'][9:11]).all()) and bool(torch.isnan(ref['dv'][10]).all())
    assert int(torch.isnan(ref['dv'][9]).sum()) == (0 if norm == 'l1' else 1)   # n was clamped: A stays out of dv
    assert float(got['ds'][11]) == 0.0 and float(got['dg'][11]) == 0.0 and float(got['dv'][11].float().abs().max()) == 0.0
    print('WEIGHT_NORM nonfinite %s %s C=%d ds %.3g dg %.3g dv %.3g (worst share of the bound, finite entries)'
          % (dn, norm, chunks, share['ds'], share['dg'], share['dv']))
    # rows 0 .. 8: the bits of the same call on the clean tensor
    for name in WN.OUTPUTS:
        assert same_bits(got[name][:9], c[name][:9]), name
    # the composed route on the device: the same n rule and the same NaN pattern
    fwd_before = len(launches['weight_norm_fwd'])
    monkeypatch.setattr(config, 'FUSED_PATHS', False)
    q, w = module_on(v, c)
    y = q(w)[0]
    y.backward(c['gy'].to(DEV))
    assert len(launches['weight_norm_fwd']) == fwd_before
    with torch.no_grad():
        n_c = q.composed(w, q.scaling_impl(w), q.pre_scaling_impl(w), WN.QMAX)[1].reshape(-1).cpu()
    assert float(n_c[9]) == nmin and float(n_c[10]) == float('inf') and float(n_c[11]) == float('inf')
    for a, b, name in ((y.detach(), got['y'], 'y'), (w.grad, got['dv'], 'dv'),
                       (q.scaling_impl.value.grad.reshape(-1), got['ds'], 'ds'),
                       (q.pre_scaling_impl.value.grad.reshape(-1), got['dg'], 'dg')):
        assert torch.equal(torch.isnan(a.float()).cpu(), torch.isnan(b.float())), 'composed route: %s' % name
    assert float(y.detach()[11].float().abs().max()) == 0.0 and float(w.grad[11].float().abs().max()) == 0.0
    assert float(q.scaling_impl.value.grad.reshape(-1)[11]) == 0.0 and float(q.pre_scaling_impl.value.grad.reshape(-1)[11]) == 0.0
