"""Asymmetric group-wise weight quantizers (ShiftedUint8WeightPerGroupFloat / ShiftedUint4WeightPerGroupFloat) on the CPU
route against golden vectors produced by the reference: its resolved ShiftedUint8WeightPerChannelFloat graph applied to
the weight regrouped as [out * K / g, g] (tests/golden/make_golden_group_shifted.py), plus the module surface -- shapes,
state-dict keys, the errors -- and the argument checks of the C ABI entries, which need no device.

Bars: y, scale and zp are bit-exact.  dx is bit-exact except at the first element equal to the minimum and the first
equal to the maximum of each group, which receive reduced sums; there it is held to `deposit_ulps`.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import golden_util as G

DT = {'f32': torch.float32, 'bf16': torch.bfloat16, 'f16': torch.float16}
MANT = {'f32': 23, 'bf16': 7, 'f16': 10}
MIN_EXP = {'f32': -126, 'bf16': -126, 'f16': -14}
CASES = G.load('group_shifted')
case = pytest.mark.parametrize('c', CASES, ids=G.ids(CASES, ['shape', 'group_size', 'bit_width', 'dtype']))


@pytest.fixture(autouse=True)
def cpu_scalar_semantics(monkeypatch):
    """the golden vectors were produced by torch CPU kernels (include/bvq.h, bvq_scalar_mode)"""
    import brevitas_amd.config as config
    monkeypatch.setattr(config, 'SCALAR_OPERAND_MODE', 'cpu')


def to_np(t):
    t = t.detach().cpu().contiguous()
    if t.dtype in (torch.bfloat16, torch.float16):
        return t.view(torch.int16).numpy().view(np.uint16)
    return t.numpy()


def assert_bits(t, c, name):
    want = c.arr(name)
    got = to_np(t).reshape(want.shape)
    assert G.same_bits(got, want, c['dtypes'][name]), (name, G.mismatch_report(got, want, 0))


def deposit_ulps(dn, g):
    """Cap of the difference at a deposit position, in units in the last place of the dtype at `deposit_magnitude`, a
    bound of every value on the way there, so that one ulp of any of them is at most one ulp of it.

    Two routes that add the same float32 terms in another order and round at the same points can differ by:
      * the summation order.  n float32 addends t: at most 2 (n - 1) 2^-24 sum|t|.  The scale gradient has 2 g addends,
        which reach the deposit divided by the integer threshold: 2 (2 g - 1) units.  The zero-point gradient has g and
        reaches it twice, as dzp / scale and as -dzp * ((n / s) / s) / threshold: 2 * 2 (g - 1).  Together 8 g - 6.
        Against a 16-bit ulp these are nothing: what is left there are rounding flips;
      * the roundings to the dtype behind the sums: the two sums (2), the joins with gscale, gzp and the zero-point's
        share of the scale gradient (3), dzp / scale, its product with (n / s) / s and v / threshold (3), and the final
        adds on dx, the zero-point statistic's, the scale statistic's and, on a constant group, the one of the two
        deposits to each other (3): 11, each at most one ulp of its own value, which a following quotient or product can
        carry into the next binade, where it counts twice: 22."""
    return 22 + (8 * g - 6 if dn == 'f32' else 0)


def ulp(v, dn):
    e = max(int(np.floor(np.log2(v))), MIN_EXP[dn])
    return 2.0 ** (e - MANT[dn])


def stat_positions(x, g):
    """flat indices of the first element equal to the minimum and of the first equal to the maximum of every group of g
    consecutive elements (-0 equals +0)"""
    a = x.detach().float().cpu().reshape(-1, g)
    base = torch.arange(a.shape[0]) * g
    first_max = (a == a.max(dim=1, keepdim=True).values).float().argmax(dim=1)
    first_min = (a == a.min(dim=1, keepdim=True).values).float().argmax(dim=1)
    return set((base + first_max).tolist()) | set((base + first_min).tolist())


def deposit_magnitude(x, grad, scale, zp, g, bits, gscale=None, gzp=None):
    """per group, a bound of every value on a deposit's way, from the inputs and the REFERENCE's scale and zero-point:
    sum |g| (|q - zp| + |x / s|) / threshold for the scale gradient, 2 sum |g| for the two ways of the zero-point
    gradient, and what arrives through the returned scale and zero-point"""
    thr = 2.0 ** bits - 1
    xf = x.detach().double().cpu().reshape(-1, g)
    gf = grad.detach().double().cpu().reshape(-1, g).abs()
    s = scale.detach().double().cpu().reshape(-1, 1)
    z = zp.detach().double().cpu().reshape(-1, 1)
    t = xf / s
    q = torch.clamp(torch.round(t + z), 0, thr)
    mag = (gf * ((q - z).abs() + t.abs())).sum(dim=1) / thr + 2 * gf.sum(dim=1)
    if gscale is not None:
        mag = mag + gscale.detach().double().cpu().reshape(-1).abs() / thr
    if gzp is not None:
        mag = mag + 2 * gzp.detach().double().cpu().reshape(-1).abs() / s.reshape(-1)
    return mag.numpy()


def assert_dx(got, want, x, grad, scale, zp, g, bits, dn, gscale=None, gzp=None, skip_groups=()):
    """bit-equal away from the first-minimum and first-maximum element of each group (that set, computed from x, is a
    condition); there within deposit_ulps -> the worst ulps seen"""
    gotb, wantb = to_np(got).reshape(-1), to_np(want).reshape(-1)
    gotf = got.detach().float().cpu().numpy().reshape(-1).astype(np.float64)
    wantf = want.detach().float().cpu().numpy().reshape(-1).astype(np.float64)
    if dn == 'f32':
        gotb, wantb = gotb.view(np.uint32), wantb.view(np.uint32)
    bad = [int(i) for i in np.nonzero(gotb != wantb)[0]
           if i // g not in skip_groups and not (np.isnan(gotf[i]) and np.isnan(wantf[i]))]
    allowed = stat_positions(x, g)
    assert set(bad) <= allowed, sorted(set(bad) - allowed)[:8]
    mags = deposit_magnitude(x, grad, scale, zp, g, bits, gscale, gzp)
    worst = 0.0
    for i in bad:
        mag = max(abs(gotf[i]), abs(wantf[i]), mags[i // g])
        assert np.isfinite(mag) and mag > 0, (i, gotf[i], wantf[i], mag)
        n = abs(gotf[i] - wantf[i]) / ulp(mag, dn)
        assert n <= deposit_ulps(dn, g), (i, gotf[i], wantf[i], n)
        worst = max(worst, n)
    return worst


def group_quantizer(w, c):
    import brevitas_amd.quant as Q
    if c['bit_width'] == 4:
        return Q.ShiftedUint4WeightPerGroupFloat(w, group_size=c['group_size'])
    return Q.ShiftedUint8WeightPerGroupFloat(w, group_size=c['group_size'], bit_width=c['bit_width'])


def run_case(c, device):
    """one training step of the group-wise quantizer on the golden weight -> (y, scale, zero_point, dx)"""
    w = torch.nn.Parameter(c.torch('x', device))
    q = group_quantizer(w, c).to(device)
    y, scale, zp, bw = q(w)
    assert float(bw) == c['bit_width']
    y.backward(c.torch('g', device))
    return y, scale, zp, w.grad


def check_case(c, y, scale, zp, dx):
    """-> the worst deposit difference in ulps"""
    out, g, bits = c['shape'][0], c['group_size'], c['bit_width']
    k = int(np.prod(c['shape'])) // out
    dt = DT[c['dtype']]
    assert tuple(y.shape) == tuple(c['shape']) and y.dtype == dt
    assert tuple(scale.shape) == (out, k // g, 1) and scale.dtype == dt
    assert tuple(zp.shape) == (out, k // g, 1) and zp.dtype == dt
    zf = zp.detach().float().cpu()
    assert bool((zf == zf.round()).all()) and float(zf.min()) >= 0 and float(zf.max()) <= 2 ** bits - 1
    assert_bits(y, c, 'y')
    assert_bits(scale, c, 'scale')
    assert_bits(zp, c, 'zp')
    return assert_dx(dx, c.torch('dx'), c.torch('x'), c.torch('g'), c.torch('scale'), c.torch('zp'), g, bits,
                     c['dtype'])


@case
def test_golden_inputs_hold_the_planted_groups(c):
    """the cases cannot be passed on inputs that avoid the corners"""
    g, P = c['group_size'], c['planted']
    x = c.torch('x').reshape(-1, g)
    xf = x.float()
    zp = c.torch('zp').float().reshape(-1)
    chunk = 16 // (4 if c['dtype'] == 'f32' else 2)
    assert bool((xf[P['zero']] == 0).all())
    assert bool((xf[P['constant']] == xf[P['constant'], 0]).all()) and float(xf[P['constant'], 0]) != 0
    assert bool((xf[P['positive']] > 0).all()) and float(zp[P['positive']]) == 0
    assert bool((xf[P['negative']] < 0).all()) and float(zp[P['negative']]) == 2 ** c['bit_width'] - 1

    def hits(grp, fn):
        return torch.nonzero(xf[grp] == fn(xf[grp])).reshape(-1).tolist()
    far, near = hits(P['min_far'], torch.min), hits(P['min_near'], torch.min)
    assert len(far) == 2 and far[0] // chunk != far[1] // chunk and len(near) == 2 and near[0] // chunk == near[1] // chunk
    far, near = hits(P['max_far'], torch.max), hits(P['max_near'], torch.max)
    assert len(far) == 2 and far[0] // chunk != far[1] // chunk and len(near) == 2 and near[0] // chunk == near[1] // chunk
    assert hits(P['ends'], torch.max) == [0] and hits(P['ends'], torch.min) == [g - 1]
    zeros = x[P['zeros']]
    signs = torch.signbit(zeros[zeros.float() == 0]).tolist()
    assert float(xf[P['zeros']].max()) == 0 and signs == [True, False]
    assert bool(np.isfinite(c.f32('dx')).all())


@case
def test_cpu_route_matches_the_reference(c):
    worst = check_case(c, *run_case(c, 'cpu'))
    print('GROUP_SHIFTED_DEPOSIT_ULPS cpu %s g=%d bits=%d worst=%.3f' % (c['dtype'], c['group_size'], c['bit_width'],
                                                                         worst))


def test_zero_zero_point_route_returns_the_bits_of_the_symmetric_golden():
    """GroupwiseRescalingIntQuant with ZeroZeroPoint on a CPU tensor: what it returned before the asymmetric graph came"""
    from test_group_quant_golden import CASES as SYM, check_case as check_sym, run_case as run_sym
    for c in SYM:
        check_sym(c, *run_sym(c, 'cpu'))


def test_state_dict_keys_are_those_of_the_per_channel_quantizer():
    import brevitas_amd.quant as Q
    w = torch.nn.Parameter(torch.randn(8, 64))
    grouped = Q.ShiftedUint8WeightPerGroupFloat(w, group_size=32)
    per_channel = Q.ShiftedUint8WeightPerChannelFloat(w)
    assert sorted(grouped.state_dict().keys()) == sorted(per_channel.state_dict().keys())
    assert [n for n, _ in grouped.named_children()] == [n for n, _ in per_channel.named_children()]
    assert [n for n, _ in grouped.named_parameters()] == [n for n, _ in per_channel.named_parameters()]
    assert [n for n, _ in grouped.named_buffers()] == [n for n, _ in per_channel.named_buffers()]


def test_module_surface():
    from brevitas_amd.core.quant import GroupwiseRescalingIntQuant
    import brevitas_amd.quant as Q
    assert 'ShiftedUint8WeightPerGroupFloat' in Q.__all__ and 'ShiftedUint4WeightPerGroupFloat' in Q.__all__
    q = Q.ShiftedUint4WeightPerGroupFloat(torch.nn.Parameter(torch.randn(4, 256)))
    assert isinstance(q, GroupwiseRescalingIntQuant) and q.group_size == 128
    assert float(q.msb_clamp_bit_width_impl()) == 4.0
    assert not q.int_quant.signed and not q.int_quant.narrow_range
    q8 = Q.ShiftedUint8WeightPerGroupFloat(torch.nn.Parameter(torch.randn(4, 256)))
    assert q8.group_size == 128 and float(q8.msb_clamp_bit_width_impl()) == 8.0


def test_errors():
    import brevitas_amd.quant as Q
    from brevitas_amd.nn import QuantLinear
    w = torch.nn.Parameter(torch.randn(8, 64))
    with pytest.raises(ValueError, match=r'\(8, 64\).*48'):   # K % g != 0, at construction
        Q.ShiftedUint8WeightPerGroupFloat(w, group_size=48)
    with pytest.raises(ValueError, match='exactly one weight'):
        Q.ShiftedUint4WeightPerGroupFloat([w, torch.nn.Parameter(torch.randn(8, 64))], group_size=32)
    q = Q.ShiftedUint8WeightPerGroupFloat(w, group_size=32)
    with pytest.raises(ValueError, match=r'\(8, 40\).*32'):   # at call time
        q(torch.randn(8, 40))
    grouped = functools.partial(Q.ShiftedUint4WeightPerGroupFloat, group_size=32)
    with pytest.raises(ValueError, match='group-wise'):
        QuantLinear(64, 8, weight_quant=grouped, bias_quant=Q.Int8Bias(),
                    input_quant=Q.Int8ActPerTensorFloat(scaling_impl_type='stats', scaling_stats_op='max'))


def test_quant_linear_with_a_partial_factory():
    """QuantLinear with the asymmetric group-wise weight quantizer equals F.linear on the golden-checked weight"""
    import brevitas_amd.quant as Q
    from brevitas_amd.nn import QuantConv2d, QuantLinear
    c = next(k for k in CASES if k['shape'] == [24, 256] and k['dtype'] == 'f32')
    lin = QuantLinear(256, 24, bias=False,
                      weight_quant=functools.partial(Q.ShiftedUint4WeightPerGroupFloat, group_size=32))
    with torch.no_grad():
        lin.weight.copy_(c.torch('x'))
    torch.manual_seed(0)
    x = torch.randn(3, 256, requires_grad=True)
    wq, scale, zp, _ = lin.quant_weight()
    assert_bits(wq, c, 'y')
    assert tuple(scale.shape) == (24, 8, 1) and tuple(zp.shape) == (24, 8, 1)
    y = lin(x)
    y.sum().backward()
    assert torch.equal(y, torch.nn.functional.linear(x, c.torch('y')))
    assert lin.weight.grad is not None and bool(torch.isfinite(lin.weight.grad).all())
    conv = QuantConv2d(16, 8, 3, bias=False,
                       weight_quant=functools.partial(Q.ShiftedUint4WeightPerGroupFloat, group_size=16))
    assert conv(torch.randn(1, 16, 5, 5)).shape == (1, 8, 3, 3)


def test_weight_quant_group_leaves_the_quantizer_out():
    import brevitas_amd.quant as Q
    from brevitas_amd import WeightQuantGroup
    from brevitas_amd.nn import QuantLinear
    model = torch.nn.Sequential(
        QuantLinear(64, 16, weight_quant=functools.partial(Q.ShiftedUint4WeightPerGroupFloat, group_size=32)),
        QuantLinear(16, 8, weight_quant=Q.Int8WeightPerChannelFloat))
    group = WeightQuantGroup(model)
    assert [n for n, _ in group.covered] + [n for n, _ in group.uncovered] == ['1.weight_quant']
    x = torch.randn(2, 64)
    want = model(x)
    with group:
        got = model(x)
    assert torch.equal(got, want)


def test_cabi_argument_checks_need_no_device():
    from brevitas_amd import _native as nat
    lib = nat.lib
    assert lib.bvq_group_shifted_fwd(None, None, 0.0, 0, 1.0, None, None, None, None, None) == -1
    assert 'descriptor' in nat.last_error()
    assert lib.bvq_group_shifted_bwd(None, None, None, None, None, None, 0.0, 0, 1.0, None, None) == -1
    assert lib.bvq_group_shifted_supported(None, None) == 0

    def desc(inner, dt=nat.BF16, ct=None, zdt=None, zp_pc=1, out_kind=nat.OUT_DEQUANT, pre_op=nat.PRE_NONE):
        return nat.QuantDesc(1, 12, inner, dt, dt if ct is None else ct, dt, dt if zdt is None else zdt, 1, zp_pc, 0.0,
                             15.0, nat.ROUND, 0, 1, out_kind, pre_op)
    aligned = ctypes.c_void_p(4096)  # never dereferenced: every check below fails before any device work
    for d, word in ((desc(48), 'group size 48'), (desc(64, out_kind=nat.OUT_INT), 'integer output'),
                    (desc(64, pre_op=nat.PRE_RELU), 'pre_op'), (desc(64, ct=nat.F32), 'dtype'),
                    (desc(64, zdt=nat.F32), 'zero-point dtype'), (desc(64, zp_pc=0), 'zero-point per channel')):
        assert lib.bvq_group_shifted_supported(ctypes.byref(d), aligned) == 0
        rc = lib.bvq_group_shifted_fwd(ctypes.byref(d), aligned, 1e-10, 1, 15.0, aligned, aligned, aligned, aligned, None)
        assert rc == -2 and word in nat.last_error(), (rc, nat.last_error())
        rc = lib.bvq_group_shifted_bwd(ctypes.byref(d), aligned, aligned, aligned, None, None, 1e-10, 1, 15.0, aligned,
                                       None)
        assert rc == -2 and word in nat.last_error(), (rc, nat.last_error())
    for dt in (nat.BF16, nat.F16, nat.F32):
        for inner in (16, 32, 64, 128, 256):
            assert lib.bvq_group_shifted_supported(ctypes.byref(desc(inner, dt=dt)), aligned) == 1
    ok = desc(64)
    assert lib.bvq_group_shifted_supported(ctypes.byref(ok), ctypes.c_void_p(4098)) == 0   # off a 16-byte boundary
    rc = lib.bvq_group_shifted_fwd(ctypes.byref(ok), ctypes.c_void_p(4098), 1e-10, 1, 15.0, aligned, aligned, aligned,
                                   aligned, None)
    assert rc == -2 and '16-byte' in nat.last_error()
    assert lib.bvq_group_shifted_fwd(ctypes.byref(ok), None, 1e-10, 1, 15.0, aligned, aligned, aligned, aligned,
                                     None) == -1
    # the symmetric entries still refuse a descriptor with zero-points per group, and the other way round
    assert lib.bvq_group_quant_supported(ctypes.byref(ok), aligned) == 0
