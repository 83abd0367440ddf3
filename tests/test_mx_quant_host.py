"""MX block-scaled quantizers on the CPU: the composed route (brevitas_amd/core/quant/mx.py) against the definition
restated here twice, sharing nothing with the package -- a numpy float64 oracle that enumerates each format's value set
and takes the nearest value with ties to the even index, and the closed rounding formula in float64, used by the
float64 torch.autograd reference of the backward.  The GPU tests (test_gpu_mx_quant.py) import the oracle and the bars.

Bars: y and scale are bit-exact (sign of zero included; every NaN equals every NaN).  dx is bit-equal to gy * mask
except at the first arg-max of each group, which receives a float32 sum of g terms: there
    |dx - dx_ref| <= (g + 4) * 2^-24 * (|gs| + sum_i |gy_i (q_i - p_i mask_i)|) * X / a + ulp_T(|dx_ref|)
-- g - 1 additions, the product roundings, the add of gs, the multiply, the divide, and the final rounding to T.
"""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

DT = {'f32': torch.float32, 'bf16': torch.bfloat16, 'f16': torch.float16}
INT_VIEW = {'f32': torch.int32, 'bf16': torch.int16, 'f16': torch.int16}
MANT = {'f32': 23, 'bf16': 7, 'f16': 10}
MIN_EXP = {'f32': -126, 'bf16': -126, 'f16': -14}
# name -> (exponent bits, mantissa bits, emax, max_val, bit width); int8 is k / 64, k in [-127, 127]
FORMATS = {'e4m3': (4, 3, 8, 448.0, 8), 'e5m2': (5, 2, 15, 57344.0, 8), 'e3m2': (3, 2, 4, 28.0, 6),
           'e2m3': (2, 3, 2, 7.5, 6), 'e2m1': (2, 1, 2, 6.0, 4), 'int8': (None, 6, 0, 127.0 / 64.0, 8)}
RULES = ('floor', 'ceil')
formats = pytest.mark.parametrize('fmt', list(FORMATS))
rules = pytest.mark.parametrize('rule', RULES)
dtypes = pytest.mark.parametrize('dn', ['f32', 'bf16', 'f16'])


# ---- the definition, restated ---------------------------------------------------------------------------------------

def emin_of(fmt):
    e = FORMATS[fmt][0]
    return None if e is None else 1 - (2 ** (e - 1) - 1)


@functools.lru_cache(None)
def value_set(fmt):
    """the non-negative values of the format, ascending: index parity is the parity of the code's last mantissa bit"""
    e, m, emax, max_val, _ = FORMATS[fmt]
    if e is None:
        return np.arange(128, dtype=np.float64) / 64.0
    emin = emin_of(fmt)
    vals = [k * 2.0 ** (emin - m) for k in range(2 ** m)]
    for ex in range(emin, emax + 1):
        vals += [(1 + k / 2.0 ** m) * 2.0 ** ex for k in range(2 ** m)]
    vals = np.array([v for v in vals if v <= max_val], dtype=np.float64)
    assert vals[-1] == max_val and np.all(np.diff(vals) > 0)
    return vals


def nearest_in_set(p, fmt):
    """p (float64) -> the value of the format nearest to it, ties to the even index, the sign of p kept"""
    grid = value_set(fmt)
    ap = np.abs(p)
    hi = np.clip(np.searchsorted(grid, ap, side='left'), 0, len(grid) - 1)
    lo = np.clip(hi - 1, 0, len(grid) - 1)
    dlo, dhi = np.abs(ap - grid[lo]), np.abs(grid[hi] - ap)
    pick = np.where(dlo < dhi, lo, np.where(dhi < dlo, hi, np.where(lo % 2 == 0, lo, hi)))
    return np.copysign(grid[pick], p)


def round_unbounded(p, fmt):
    """the closed form of step 4 in float64: half-even to a multiple of 2^(max(floor(log2 |p|), emin) - m)"""
    _, m, _, _, _ = FORMATS[fmt]
    emin = emin_of(fmt)
    if emin is None:
        qe = np.full(p.shape, -6.0)
    else:
        ex = np.frexp(p)[1].astype(np.float64) - 1
        qe = np.maximum(np.where(p == 0, emin, ex), emin) - m
    return np.round(p / 2.0 ** qe) * 2.0 ** qe


def oracle(x, g, fmt, rule):
    """x: tensor of T, whole groups of g in memory order -> dict of float64 arrays [groups, g] / [groups] and y as T"""
    _, _, emax, max_val, _ = FORMATS[fmt]
    xd = x.detach().cpu().double().numpy().reshape(-1, g)
    n = xd.shape[0]
    with np.errstate(invalid='ignore'):
        a = np.abs(xd).max(axis=1)
    finite = np.isfinite(a)
    exps, clamped = np.zeros(n), np.zeros(n, dtype=bool)
    for i in range(n):
        if not finite[i]:
            continue
        if a[i] == 0:
            e = -10 ** 6
        else:
            e = math.frexp(a[i])[1] - 1 - emax
            if rule == 'ceil' and a[i] > max_val * 2.0 ** e:
                e += 1
        exps[i] = min(max(e, -126), 127)
        clamped[i] = exps[i] != e
    big_x = 2.0 ** exps
    with np.errstate(invalid='ignore', over='ignore'):
        p = np.where(finite[:, None], xd / big_x[:, None], np.nan)
        ok = np.where(finite[:, None], p, 0.0)
        q = np.where(finite[:, None], nearest_in_set(ok, fmt), np.nan)
        r = np.where(finite[:, None], round_unbounded(ok, fmt), np.nan)
        # the two restatements agree: clamp after the closed-form rounding is the nearest value of the set
        assert np.array_equal(np.clip(r, -max_val, max_val), q, equal_nan=True)
        assert np.array_equal(np.signbit(r), np.signbit(q))
        y = torch.from_numpy((q * big_x[:, None]).astype(np.float32)).to(x.dtype).reshape(x.shape)
        inside = np.abs(r) <= max_val
    scale = np.where(finite, big_x, np.nan).astype(np.float32)
    return dict(x=xd, a=a, finite=finite, clamped=clamped, E=exps, X=big_x, p=p, q=q, r=r, inside=inside, y=y,
                scale=scale, saturated=int((np.abs(ok) > max_val).sum()))


def same_bits(a, b):
    """bitwise equality of two tensors of one dtype, every NaN equal to every NaN"""
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    it = {4: torch.int32, 2: torch.int16}[a.element_size()]
    return bool(((a.view(it) == b.view(it)) | (torch.isnan(a) & torch.isnan(b))).all())


def first_mismatch(a, b):
    a, b = a.detach().cpu().reshape(-1), b.detach().cpu().reshape(-1)
    it = {4: torch.int32, 2: torch.int16}[a.element_size()]
    bad = torch.nonzero((a.view(it) != b.view(it)) & ~(torch.isnan(a) & torch.isnan(b))).reshape(-1)[:5]
    return 'mismatches at %s: got %s want %s' % (bad.tolist(), a[bad].tolist(), b[bad].tolist())


def ulp(v, dn):
    e = MIN_EXP[dn] if v == 0 else max(int(math.floor(math.log2(abs(v)))), MIN_EXP[dn])
    return 2.0 ** (e - MANT[dn])


# ---- inputs ---------------------------------------------------------------------------------------------------------

def make_weight(shape, dn, seed=123456):
    gen = torch.Generator().manual_seed(seed)
    w = (torch.randn(shape, generator=gen) * 3).to(DT[dn])
    grad = torch.randn(shape, generator=gen).to(DT[dn])
    return w, grad, gen


def midpoint_input(fmt, dn):
    """groups of 32: a pilot of max_val * 2^s (so E = s under both rules) and every midpoint between adjacent values of
    the format times 2^s, with alternating signs; then groups whose largest element lies above max_val * 2^s, which
    saturate under 'floor' and move the exponent under 'ceil'"""
    grid = value_set(fmt)
    max_val = FORMATS[fmt][3]
    mids = ((grid[:-1] + grid[1:]) / 2).tolist()
    rows = []
    shifts = (-3, 0) if dn == 'f16' else (-40, -3, 0, 9)
    for s in shifts:
        for i in range(0, len(mids), 31):
            part = mids[i:i + 31]
            part = [v * (-1) ** k for k, v in enumerate(part)] + [0.0] * (31 - len(part))
            rows.append([max_val * 2.0 ** s] + [v * 2.0 ** s for v in part])
        over = max_val + (grid[-1] - grid[-2]) / 2        # half-way to the next value of the unbounded grid
        tail = mids[-30:] + [0.0] * max(0, 30 - len(mids))
        rows.append([-over * 2.0 ** s, max_val * 2.0 ** s] + [v * 2.0 ** s for v in tail])
    return torch.tensor(rows, dtype=torch.float64).to(DT[dn])


@functools.lru_cache(None)
def _bf16_sweep():
    pats = torch.arange(0, 0x4181, dtype=torch.int32)                       # +0 .. +16.0
    pats = torch.cat([pats, (pats | 0x8000) - 0x10000]).to(torch.int16)     # and the same with the sign bit
    vals = pats.view(torch.bfloat16)
    assert bool(torch.isfinite(vals).all()) and float(vals.float().abs().max()) == 16.0
    n = -(-vals.numel() // 31)
    body = torch.zeros(n * 31, dtype=torch.bfloat16)
    body[:vals.numel()] = vals
    pilot = torch.full((n, 1), 24.0, dtype=torch.bfloat16)
    pilot[1::2] = -24.0
    return torch.cat([pilot, body.view(n, 31)], dim=1).contiguous()


def bf16_sweep(dn):
    """every finite bf16 pattern with |v| <= 16, 31 to a group, plus a pilot of +-24 per group: p visits every bf16
    value of every binade relative to the scale"""
    return _bf16_sweep().to(DT[dn])


def mx(fmt, g=32, rule='floor', clamp_ste=False, axis='flat'):
    from brevitas_amd.core.quant.mx import MXQuant
    return MXQuant(fmt, group_size=g, scale_rule=rule, clamp_ste=clamp_ste, group_axis=axis)


def step(q, x, grad, gscale=None, clone=True):
    """forward + backward of a quantizer on a fresh leaf (clone=False: on x's own storage) -> (y, scale, dx)"""
    leaf = (x.detach().clone() if clone else x.detach()).requires_grad_(True)
    y, scale, _, _ = q(leaf)
    if gscale is None:
        y.backward(grad.view(y.shape))
    else:
        torch.autograd.backward([y, scale], [grad.view(y.shape), gscale.view(scale.shape)])
    return y.detach(), scale.detach(), leaf.grad.detach()


def check_forward(y, scale, ref):
    assert same_bits(y.reshape(-1), ref['y'].reshape(-1)), first_mismatch(y, ref['y'])
    assert scale.dtype == torch.float32
    assert same_bits(scale.reshape(-1), torch.from_numpy(ref['scale'])), first_mismatch(scale,
                                                                                         torch.from_numpy(ref['scale']))


# ---- 1: forward against the oracle ----------------------------------------------------------------------------------

@formats
@rules
@dtypes
def test_forward_matches_the_oracle(fmt, rule, dn):
    w, _, _ = make_weight((64, 64), dn)
    inputs = [w, midpoint_input(fmt, dn), bf16_sweep(dn)]
    saturated = ties = 0
    for x in inputs:
        ref = oracle(x, 32, fmt, rule)
        y, scale, _, _ = mx(fmt, 32, rule)(x)
        check_forward(y, scale, ref)
        saturated += ref['saturated']
        ok = np.where(ref['finite'][:, None], ref['p'], 0.0)
        grid = value_set(fmt)
        mids = (grid[:-1] + grid[1:]) / 2
        ties += int(np.isin(np.abs(ok), mids).sum())
    # conditions on the inputs: the OCP rule saturates somewhere, the ceil rule nowhere; ties are hit
    assert (saturated > 0) if rule == 'floor' else (saturated == 0), saturated
    assert ties > 0


# ---- 2: the float8 casts of torch ----------------------------------------------------------------------------------

@pytest.mark.parametrize('fmt,f8', [('e4m3', torch.float8_e4m3fn), ('e5m2', torch.float8_e5m2)])
@rules
def test_q_is_the_float8_cast_of_torch(fmt, f8, rule):
    from brevitas_amd.core.quant.mx import MX_FORMATS, _group_terms
    max_val = FORMATS[fmt][3]
    for x in (make_weight((64, 64), 'f32')[0], midpoint_input(fmt, 'f32'), bf16_sweep('f32')):
        t = _group_terms(x.reshape(-1, 32).float(), MX_FORMATS[fmt], rule == 'ceil')
        want = t['p'].clamp(-max_val, max_val).to(f8).float()
        assert same_bits(t['q'], want), first_mismatch(t['q'], want)


# ---- 3: edge groups -------------------------------------------------------------------------------------------------

def edge_all_zero(dn):
    x = torch.zeros(2, 32, dtype=DT[dn])
    x[0, 3], x[0, 7] = -0.0, -0.0
    x[1] = torch.linspace(-1, 1, 32).to(DT[dn])
    return x


@formats
@dtypes
def test_an_all_zero_group(fmt, dn):
    x = edge_all_zero(dn)
    grad = torch.ones_like(x)
    gs = torch.ones(2)
    y, scale, dx = step(mx(fmt, clamp_ste=True), x, grad, gs)
    assert float(scale.reshape(-1)[0]) == 2.0 ** -126
    assert same_bits(y[0], x[0])                      # +-0 with their signs
    assert same_bits(dx[0], grad[0])                  # no deposit
    check_forward(y, scale, oracle(x, 32, fmt, 'floor'))


@formats
@dtypes
@pytest.mark.parametrize('bad', [float('nan'), float('inf'), float('-inf')])
def test_a_group_with_a_nan_or_an_inf(fmt, dn, bad):
    x, grad, _ = make_weight((3, 32), dn)
    x[1, 9] = bad
    y, scale, dx = step(mx(fmt), x, grad)
    assert bool(torch.isnan(scale.reshape(-1)[1])) and bool(torch.isnan(y[1]).all())
    assert int(torch.isnan(scale).sum()) == 1 and not bool(torch.isnan(y[0]).any() | torch.isnan(y[2]).any())
    check_forward(y, scale, oracle(x, 32, fmt, 'floor'))
    assert bool(torch.isfinite(dx.float()).all())     # nothing flows through a, and nothing is invented


@formats
@pytest.mark.parametrize('dn', ['f32', 'bf16'])
def test_the_exponent_clamp(fmt, dn):
    x = torch.zeros(1, 32, dtype=DT[dn])
    x[0, 5], x[0, 6] = 2.0 ** -120, -2.0 ** -123
    grad = torch.full_like(x, 0.5)
    y, scale, dx = step(mx(fmt, clamp_ste=True), x, grad, torch.ones(1))
    ref = oracle(x, 32, fmt, 'floor')
    emax = FORMATS[fmt][2]
    assert bool(ref['clamped'][0]) == (-120 - emax < -126)
    check_forward(y, scale, ref)
    if ref['clamped'][0]:
        assert float(scale) == 2.0 ** -126 and same_bits(dx, grad)  # no deposit


@formats
@rules
def test_float16_subnormals(fmt, rule):
    x = (torch.arange(-16, 16, dtype=torch.float32) * 2.0 ** -24).to(torch.float16).view(1, 32)
    assert float(x.float().abs().max()) < 2.0 ** -14
    y, scale, _, _ = mx(fmt, rule=rule)(x)
    check_forward(y, scale, oracle(x, 32, fmt, rule))


def test_float16_overflow_to_inf_under_ceil():
    """a = 65504 with e2m1 and 'ceil': E = 14, p = 3.998 rounds to 4, y = 4 * 2^14 = 65536 is beyond float16"""
    x = torch.zeros(1, 32, dtype=torch.float16)
    x[0, 0], x[0, 1] = 65504.0, -65504.0
    y, scale, _, _ = mx('e2m1', rule='ceil')(x)
    assert float(scale) == 2.0 ** 14
    assert float(y[0, 0]) == float('inf') and float(y[0, 1]) == float('-inf')
    check_forward(y, scale, oracle(x, 32, 'e2m1', 'ceil'))


def tie_input(dn, g=32):
    x, grad, _ = make_weight((4, g), dn)
    m = (x[2].float().abs().max() * 1.25).to(x.dtype)
    x[2, 1], x[2, g - 2] = -m, m                     # the abs-max twice, in two 16-byte chunks: the first wins
    return x, grad


@formats
@dtypes
def test_a_tie_for_the_abs_max_deposits_on_the_first(fmt, dn):
    x, grad = tie_input(dn)
    gs = torch.full((4,), 3.0)
    _, _, dx = step(mx(fmt, clamp_ste=True), x, grad, gs)
    assert not same_bits(dx[2, 1:2], grad[2, 1:2])                           # the first received the deposit
    moved = torch.nonzero(dx[2].view(INT_VIEW[dn]) != grad[2].view(INT_VIEW[dn])).reshape(-1).tolist()
    assert moved == [1], moved


# ---- 4: backward against float64 autograd ---------------------------------------------------------------------------

def autograd_reference(x, grad, gs, g, fmt, rule, clamp_ste):
    """float64 torch.autograd over the straight-through composition -> (dx_ref [groups, g], oracle dict)"""
    max_val = FORMATS[fmt][3]
    ref = oracle(x, g, fmt, rule)
    xl = torch.from_numpy(ref['x']).clone().requires_grad_(True)
    a = xl.abs().amax(dim=1, keepdim=True)
    lg = torch.log2(a)
    big_x = 2.0 ** (lg + (torch.from_numpy(ref['E']).reshape(-1, 1) - lg).detach())
    # log2 and the power round: the value is put back to the exact 2^E (the gradient stays that of the expression),
    # or an input on a rounding tie -- every other bfloat16 value against a 3-bit mantissa -- would round the other way
    big_x = big_x + (torch.from_numpy(ref['X']).reshape(-1, 1) - big_x).detach()
    p = xl / big_x
    r = p + (torch.from_numpy(round_unbounded(p.detach().numpy(), fmt)) - p).detach()
    q = r.clamp(-max_val, max_val)
    if clamp_ste:
        q = r + (q - r).detach()
    y = q * big_x
    loss = (y * grad.double().reshape(-1, g)).sum()
    if gs is not None:
        loss = loss + (big_x.reshape(-1) * gs.double().reshape(-1)).sum()
    loss.backward()
    return xl.grad.numpy(), ref


def assert_dx(dx, x, grad, gs, g, fmt, rule, clamp_ste, dn):
    """dx against the bars of this file's docstring -> the worst deposit difference seen, in ulps of T"""
    dx_ref, ref = autograd_reference(x, grad, gs, g, fmt, rule, clamp_ste)
    ax = np.abs(ref['x'])
    assert np.all((ax == ref['a'][:, None]).sum(axis=1) == 1), 'the inputs of this check have no abs-max ties'
    assert ref['finite'].all() and not ref['clamped'].any()
    first = ax.argmax(axis=1)
    mask = ref['inside'] | bool(clamp_ste)
    plain = torch.where(torch.from_numpy(mask), grad.cpu().reshape(-1, g), torch.zeros((), dtype=grad.dtype))
    got = dx.detach().cpu().reshape(-1, g)
    differs = (got.view(INT_VIEW[dn]) != plain.view(INT_VIEW[dn])).numpy()
    rows, cols = np.nonzero(differs)
    allowed = set(zip(range(len(first)), first.tolist()))
    assert set(zip(rows.tolist(), cols.tolist())) <= allowed, sorted(set(zip(rows.tolist(), cols.tolist())) - allowed)[:8]
    gd = grad.cpu().double().numpy().reshape(-1, g)
    terms = np.abs(gd * (ref['q'] - ref['p'] * mask)).sum(axis=1)
    gsa = np.zeros(len(first)) if gs is None else np.abs(gs.cpu().double().numpy().reshape(-1))
    gotd = got.double().numpy()
    worst = 0.0
    for i, k in enumerate(first.tolist()):
        u = ulp(dx_ref[i, k], dn)
        tol = (g + 4) * 2.0 ** -24 * (gsa[i] + terms[i]) * ref['X'][i] / ref['a'][i] + u
        diff = abs(gotd[i, k] - dx_ref[i, k])
        assert diff <= tol, (i, k, gotd[i, k], dx_ref[i, k], diff, tol)
        worst = max(worst, diff / u)
    return worst


@formats
@rules
@pytest.mark.parametrize('ste', [True, False], ids=['clamp_ste', 'clamp'])
@pytest.mark.parametrize('with_gs', [True, False], ids=['gs', 'no_gs'])
def test_backward_matches_float64_autograd(fmt, rule, ste, with_gs):
    x, grad, gen = make_weight((16, 64), 'f32')
    x[0, 3] = 4 * 255.0 / 128    # its group's abs-max, 1.992 * 2^2: beyond max_val * 2^E of every format under 'floor'
    gs = torch.randn(32, generator=gen) if with_gs else None
    _, _, dx = step(mx(fmt, 32, rule, ste), x, grad, gs)
    assert_dx(dx, x, grad, gs, 32, fmt, rule, ste, 'f32')
    if not ste and rule == 'floor':
        ref = oracle(x, 32, fmt, rule)
        assert not ref['inside'].all()      # the plain clamp masked something


# ---- 5: module surface ----------------------------------------------------------------------------------------------

def test_module_surface():
    import brevitas_amd.quant as Q
    from brevitas_amd.core.quant import MXQuant
    q = mx('e4m3')
    assert isinstance(q, MXQuant)
    assert len(q.state_dict()) == 0 and not list(q.parameters())
    x = torch.randn(6, 4, 4, 4)
    y, scale, zp, bw = q(x)
    assert y.shape == x.shape and y.dtype == x.dtype
    assert tuple(scale.shape) == (6, 2, 1) and scale.dtype == torch.float32
    assert float(zp) == 0.0 and zp.dim() == 0
    x = torch.randn(2, 5, 64, dtype=torch.bfloat16)
    y, scale, _, _ = mx('e2m1', axis='last')(x)
    assert tuple(scale.shape) == (2, 5, 2, 1) and scale.dtype == torch.float32 and y.dtype == torch.bfloat16
    for fmt, bits in (('e4m3', 8), ('e5m2', 8), ('e3m2', 6), ('e2m3', 6), ('e2m1', 4), ('int8', 8)):
        assert float(mx(fmt)(torch.randn(2, 32))[3]) == bits
    with pytest.raises(ValueError, match=r'\(6, 3, 4\)'):
        q(torch.randn(6, 3, 4))              # K = 12
    with pytest.raises(ValueError, match=r'\(2, 5, 48\)'):
        mx('e4m3', axis='last')(torch.randn(2, 5, 48))
    with pytest.raises(ValueError):
        mx('e9m9')
    with pytest.raises(ValueError):
        mx('e4m3', rule='nearest')
    with pytest.raises(ValueError, match=r'\(8, 48\)'):
        Q.MXFloat8e4m3Weight(torch.nn.Parameter(torch.randn(8, 48)))
    names = [p + s for p in ('MXFloat8e4m3', 'MXFloat8e5m2', 'MXFloat6e3m2', 'MXFloat6e2m3', 'MXFloat4e2m1', 'MXInt8')
             for s in ('Weight', 'Act')]
    assert set(names) <= set(Q.__all__)
    wq = Q.MXInt8Weight(torch.nn.Parameter(torch.randn(8, 64)), group_size=16, scale_rule='ceil')
    assert (wq.element_format, wq.group_size, wq.scale_rule, wq.clamp_ste, wq.group_axis) == \
        ('int8', 16, 'ceil', True, 'flat')
    aq = Q.MXFloat6e2m3Act(group_size=64)
    assert (aq.element_format, aq.group_size, aq.scale_rule, aq.clamp_ste, aq.group_axis) == \
        ('e2m3', 64, 'floor', False, 'last')


def test_collect_only_returns_the_input_untouched():
    q = mx('e4m3', axis='last')
    x = torch.randn(4, 64)
    q.bvq_collect_only = True
    y, scale, zp, bw = q(x)
    assert y is x and scale is None and zp is None and float(bw) == 8
    q.bvq_collect_only = False
    assert q(x)[1] is not None


def test_layers_and_their_refusals():
    import brevitas_amd.quant as Q
    from brevitas_amd import WeightQuantGroup
    from brevitas_amd.graph.calibrate import calibration_mode
    from brevitas_amd.nn import QuantConv2d, QuantLinear
    torch.manual_seed(0)
    with pytest.raises(ValueError, match='externally scaled bias'):
        QuantLinear(64, 8, weight_quant=Q.MXFloat4e2m1Weight, input_quant=Q.MXFloat8e4m3Act(), bias_quant=Q.Int8Bias())
    lin = QuantLinear(64, 8, weight_quant=Q.MXFloat4e2m1Weight, input_quant=Q.MXFloat8e4m3Act())
    conv = QuantConv2d(8, 4, 2, weight_quant=functools.partial(Q.MXInt8Weight, scale_rule='ceil'))
    for layer, x in ((lin, torch.randn(4, 64)), (conv, torch.randn(2, 8, 5, 5))):
        x.requires_grad_(True)
        layer(x).sum().backward()
        assert layer.weight.grad is not None and x.grad is not None
        wq, scale, _, _ = layer.quant_weight()
        assert tuple(scale.shape) == (layer.weight.shape[0], layer.weight[0].numel() // 32, 1)
        assert not torch.equal(wq, layer.weight)
    model = torch.nn.Sequential(lin)
    group = WeightQuantGroup(model)
    assert not group.covered and '0.weight_quant' not in [n for n, _ in group.uncovered]  # no member at all
    x = torch.randn(4, 64)
    quantized = model(x)
    with calibration_mode(model):
        floating = model(x)
    assert torch.equal(floating, torch.nn.functional.linear(x, lin.weight, lin.bias))
    assert torch.equal(model(x), quantized) and not torch.equal(quantized, floating)


# ---- 6: the C ABI refuses what it does not cover before any device is touched ----------------------------------------

def test_abi_refusals():
    from brevitas_amd import _native as nat
    ok = dict(dtype=nat.BF16, groups=4, group_size=32, format=nat.MX_E4M3)
    aligned, off = ctypes.c_void_p(0x10000), ctypes.c_void_p(0x10002)   # never dereferenced: the checks come first
    assert nat.lib.bvq_mx_quant_supported(ok['dtype'], ok['groups'], ok['group_size'], ok['format'], aligned) == 1
    for bad in (dict(dtype=7), dict(group_size=48), dict(group_size=8), dict(format=6), dict(format=-1)):
        a = dict(ok, **bad)
        assert nat.lib.bvq_mx_quant_supported(a['dtype'], a['groups'], a['group_size'], a['format'], aligned) == 0
        for rc in (nat.lib.bvq_mx_quant_fwd(a['dtype'], a['groups'], a['group_size'], a['format'], nat.MX_FLOOR, aligned,
                                            aligned, aligned, None),
                   nat.lib.bvq_mx_quant_bwd(a['dtype'], a['groups'], a['group_size'], a['format'], nat.MX_FLOOR, 0,
                                            aligned, aligned, None, aligned, None)):
            assert rc == -2 and nat.last_error(), (bad, rc)
    assert nat.lib.bvq_mx_quant_supported(ok['dtype'], ok['groups'], ok['group_size'], ok['format'], off) == 0
    rc = nat.lib.bvq_mx_quant_fwd(ok['dtype'], ok['groups'], ok['group_size'], ok['format'], nat.MX_CEIL, off, aligned,
                                  aligned, None)
    assert rc == -2 and '16-byte' in nat.last_error()
    rc = nat.lib.bvq_mx_quant_bwd(ok['dtype'], ok['groups'], ok['group_size'], ok['format'], nat.MX_CEIL, 1, aligned, off,
                                  None, aligned, None)
    assert rc == -2 and '16-byte' in nat.last_error()
    rc = nat.lib.bvq_mx_quant_fwd(ok['dtype'], ok['groups'], ok['group_size'], ok['format'], 2, aligned, aligned,
                                  aligned, None)
    assert rc == -2 and 'scale rule' in nat.last_error()
    x = torch.zeros(64, dtype=torch.bfloat16)
    assert nat.mx_quant_supported(x, 32, nat.MX_E2M1) and not nat.mx_quant_supported(x[1:33], 32, nat.MX_E2M1)
    assert not nat.mx_quant_supported(x, 48, nat.MX_E2M1)
