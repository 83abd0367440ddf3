"""Who receives the gradient of a max / min statistic that several elements attain, on every route that deposits one.

The reference has two rules: a whole-tensor torch.max / torch.min shares the gradient evenly over all ties
(grad / mask.sum()), a statistic reduced along a dim (torch.max(x, dim)[0]) puts all of it on the first tie.  The bar
everywhere here is torch's own autograd of the reference's expression, written out in plain torch inside the test and
run on the same device in the same dtype, compared bit for bit; behind a permuted view, where autograd drops the sign
of zeros, values are compared instead (as tests/test_gpu_ste_stats_modules.py does).

A. bvq_stat_bwd, bvq_stat_tie_scan and bvq_stat_tie_apply on a flat tensor with 1 .. n ties, on both sides of the tie
   list's capacity (kTieCap = 1024 of csrc/bvq_ties.h: above it tie_apply_full_kernel rescans the tensor), dense and
   additive, aligned and one element off a 16-byte boundary; the count in tie_info[0] and the listed positions.  The
   counts 257 and 1025 (bfloat16), 2049 (float16) and 66000 (float16: not finite) are not representable in the
   gradient's dtype: the share the kernels deposit there must be device torch's, printed as TIE_SHARE lines.
B. the same bookkeeping written by the fused per-tensor quantizer backward (bvq_fakequant_bwd with tie_stat), under
   no pre-op and under ReLU, and the two deposits that follow it; one end-to-end step of the per-tensor weight
   quantizer on values whose every float32 sum is exact in any order, against the plain-torch graph.
C. the statistic modules along a dim with ONE channel (every per-channel quantizer of a one-output-channel layer
   takes this route) and with several.

The flat length is two work units of the statistic kernels at full vector width plus a ragged tail of three elements
(make_tiling of csrc/bvq_common.hip cuts a long row into pieces of K_PIECE_CHUNKS * K_WAVE 16-byte chunks): 4099
for float32, 8195 for the 16-bit types, where 4099 elements are a single unit and a tail."""
import functools
import math

import pytest
import torch

from test_gpu_cols import bits
from test_gpu_grad_sums import K_PIECE_CHUNKS, K_WAVE

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
DT = {'f32': torch.float32, 'bf16': torch.bfloat16, 'f16': torch.float16}
dtypes = pytest.mark.parametrize('dn', ['f32', 'bf16', 'f16'])
TIE_CAP = 1024        # kTieCap
STAT = 4.0            # the planted extremum; every other element lies in [-3, 3]
KINDS = {             # the reference's whole-tensor expressions
    'abs': lambda t: torch.max(torch.abs(t)),
    'max': lambda t: torch.max(t),
    'min': lambda t: torch.min(t),
}


def nat():
    from brevitas_amd import _native
    return _native


def match_of(kind):
    return nat().MATCH_ABS if kind == 'abs' else nat().MATCH_VALUE


def flat_len(dn):
    """two full-width units and a tail of 3: the smallest length of this form that spans three units"""
    vec = 16 // DT[dn].itemsize
    unit = K_PIECE_CHUNKS * K_WAVE * vec
    n = 2 * unit + 3
    assert n % vec == 3 and -(-n // unit) == 3
    return n


def tie_counts(n):
    return (1, 2, 257, TIE_CAP - 1, TIE_CAP, TIE_CAP + 1, 2 * TIE_CAP + 1, n)


def tie_positions(n, count):
    """`count` positions, scattered with a fixed seed: the first in element 0, the last two in the ragged tail"""
    if count == n:
        return torch.arange(n)
    fixed = {1: [0], 2: [0, n - 1]}.get(count, [0, n - 2, n - 1])
    gen = torch.Generator().manual_seed(1000 + count)
    rest = torch.randperm(n - 3, generator=gen)[:count - len(fixed)] + 1      # out of 1 .. n - 3
    return torch.cat([torch.tensor(fixed, dtype=torch.int64), rest]).sort().values


@functools.lru_cache(None)
def flat_input(dn, kind, count, relu=False):
    """(x, tie mask) on the CPU, shared and left unchanged.  abs: +-STAT with the signs mixed among the ties (all +
    under ReLU, which also gets elements of -9: larger in magnitude than the statistic, they must not tie);
    max: +STAT; min: -STAT; everything else randn clamped to [-3, 3]"""
    n = flat_len(dn)
    gen = torch.Generator().manual_seed(77)
    x = torch.randn(n, generator=gen).clamp_(-3, 3)
    pos = tie_positions(n, count)
    mask = torch.zeros(n, dtype=torch.bool)
    mask[pos] = True
    sign = torch.ones(count)
    if kind == 'abs' and not relu:
        sign[1::2] = -1.0
        if count > 2:
            sign[-1] = 1.0      # the two tail ties differ in sign
            sign[-2] = -1.0
    x[pos] = (-STAT if kind == 'min' else STAT) * sign
    if relu and count < n:
        free = (~mask).nonzero().reshape(-1)
        x[free[[1, free.numel() // 2, -1]]] = -9.0
    x = x.to(DT[dn])
    # every non-tie strictly below the statistic after conversion to the dtype
    rest = x[~mask].float()
    if rest.numel():
        if kind == 'abs':
            rest = torch.relu(rest) if relu else rest.abs()
        assert float((-rest if kind == 'min' else rest).max()) < STAT
    return x, mask


def place(x, misaligned):
    """x on the device, from a 16-byte boundary or one element past one (2 bytes for the 16-bit types)"""
    buf = torch.empty(x.numel() + 16, dtype=x.dtype, device=DEV)
    assert buf.data_ptr() % 16 == 0
    view = buf[1:1 + x.numel()] if misaligned else buf[:x.numel()]
    view.copy_(x)
    assert view.data_ptr() % 16 == (x.element_size() if misaligned else 0)
    return view


def torch_grad(x, fn, g):
    """autograd of fn on a copy of x -> (statistic, gradient)"""
    xi = x.clone().requires_grad_(True)
    stat = fn(xi)
    stat.backward(g)
    return stat.detach(), xi.grad


def hexbits(t):
    return '0x%0*x' % (2 * t.element_size(), int(bits(t.reshape(-1)[:1])[0]) & ((1 << 8 * t.element_size()) - 1))


def check_tie_info(info, mask, count):
    """tie_info of a whole-tensor statistic: word 0 the number of ties exactly (above the list's capacity too), then
    the first min(count, kTieCap) list words distinct and all of them tie positions"""
    head = info[:2 + min(count, TIE_CAP)].cpu()
    assert int(head[0]) == count, 'tie_info[0] = %d for %d ties' % (int(head[0]), count)
    words = head[2:]
    assert bool(((words >= 0) & (words < mask.numel())).all())
    assert words.unique().numel() == words.numel(), 'a position is listed twice'
    assert bool(mask[words].all()), 'a listed position is no tie'


# ---- A: the native whole-tensor backward at the list's edges ----------------------------------------------------------

@dtypes
@pytest.mark.parametrize('kind', list(KINDS))
def test_whole_tensor_backward_at_the_tie_list_edges(dn, kind):
    n = flat_len(dn)
    g = torch.tensor(3.0, device=DEV, dtype=DT[dn])
    base = ((torch.arange(n, device=DEV) % 7 - 3).float() * 0.25).to(DT[dn])     # a non-zero dx to add onto
    bad = []
    for count in tie_counts(n):
        x, mask = flat_input(dn, kind, count)
        for mis in (False, True):
            xs = place(x, mis)
            stat, want = torch_grad(xs, KINDS[kind], g)
            assert float(stat) == (-STAT if kind == 'min' else STAT)
            dense = nat().stat_bwd(match_of(kind), xs, stat.reshape(1), g.reshape(1), 1, 1, n)
            if kind == 'max' and not mis:
                print('TIE_SHARE %s %d torch=%s kernel=%s' % (dn, count, hexbits(want), hexbits(dense)))
            if not torch.equal(bits(dense), bits(want)):
                bad.append((count, mis, 'dense', int((bits(dense) != bits(want)).sum())))
            added = nat().stat_bwd(match_of(kind), xs, stat.reshape(1), g.reshape(1), 1, 1, n, dx=base.clone())
            if not torch.equal(bits(added), bits(base + want)):
                bad.append((count, mis, 'additive', int((bits(added) != bits(base + want)).sum())))
            check_tie_info(nat().stat_tie_scan(match_of(kind), xs, stat.reshape(1), 1, 1, n), mask, count)
            # a negative gradient, as values: device torch's zeros are then mask * share = 0 * (a negative share),
            # negative zeros, where CPU torch and the kernels fill in +0
            _, want = torch_grad(xs, KINDS[kind], -g)
            dense = nat().stat_bwd(match_of(kind), xs, stat.reshape(1), (-g).reshape(1), 1, 1, n)
            if not torch.equal(dense, want):
                bad.append((count, mis, 'negative gradient', int((dense != want).sum())))
    assert not bad, '(ties, misaligned, mode, differing elements): %s' % bad


@pytest.mark.parametrize('kind', list(KINDS))
def test_a_tie_count_that_is_not_finite_in_float16(kind):
    """a constant float16 tensor of 66000 elements: the count is above 65519, infinite in float16"""
    n = 66000
    x = torch.full((n,), -STAT if kind == 'min' else STAT, dtype=torch.float16)
    if kind == 'abs':
        x[1::2] = -STAT
    xs = place(x, False)
    g = torch.tensor(3.0, device=DEV, dtype=torch.float16)
    stat, want = torch_grad(xs, KINDS[kind], g)
    dense = nat().stat_bwd(match_of(kind), xs, stat.reshape(1), g.reshape(1), 1, 1, n)
    if kind == 'max':
        print('TIE_SHARE f16 %d torch=%s kernel=%s' % (n, hexbits(want), hexbits(dense)))
    base = torch.full_like(xs, 0.5)
    added = nat().stat_bwd(match_of(kind), xs, stat.reshape(1), g.reshape(1), 1, 1, n, dx=base.clone())
    info = nat().stat_tie_scan(match_of(kind), xs, stat.reshape(1), 1, 1, n)
    check_tie_info(info, torch.ones(n, dtype=torch.bool), n)
    assert torch.equal(bits(dense), bits(want))
    assert torch.equal(bits(added), bits(base + want))


# ---- B: the fused per-tensor backward's ties --------------------------------------------------------------------------

PRE_FN = {0: lambda t: t, 1: torch.relu}


@dtypes
@pytest.mark.parametrize('pre', [0, 1], ids=['none', 'relu'])
def test_fused_per_tensor_backward_records_and_deposits_ties(dn, pre):
    """bvq_fakequant_bwd with channels == 1 records the ties of max |pre(x)| on its own read; then a given float32
    dscale is deposited onto the dx it returned: by bvq_stat_tie_apply_dscale (the share is torch's, through autograd
    of the statistic from dstat = (dscale.to(scale dtype) / int_threshold).to(x dtype)), and by bvq_stat_tie_apply
    with an explicit total -- five ties more than this tensor holds, as if another shard held them -- against
    dstat / total formed by torch.  One dscale value: no summation order enters."""
    n, dt = flat_len(dn), DT[dn]
    code = nat().dtype_code(dt)
    fn = PRE_FN[pre]
    zp = torch.zeros(1, device=DEV)
    thr = torch.tensor(128.0, device=DEV)
    dscale = torch.tensor([-37.5], device=DEV)
    gen = torch.Generator().manual_seed(5)
    gy = torch.randn(n, generator=gen).to(dt).to(DEV)
    desc = nat().QuantDesc(1, 1, n, code, code, code, nat().F32, 0, 0, -128.0, 127.0, 0, 0, 0, nat().OUT_DEQUANT, pre)
    bad = []
    for count in (3, TIE_CAP - 1, TIE_CAP, TIE_CAP + 1, n):
        x, mask = flat_input(dn, 'abs', count, relu=bool(pre))
        xs = place(x, False)
        stat = torch.max(torch.abs(fn(xs))).reshape(1)
        assert float(stat) == STAT and torch.equal((torch.abs(fn(xs)) == stat).cpu(), mask)
        scale = stat / thr
        dx, ds, _, ties = nat().fakequant_bwd(desc, gy, xs, scale, zp, True, False, tie_stat=stat)
        check_tie_info(ties, mask, count)
        on_ties = mask.to(DEV)
        dstat = (dscale.to(dt) / thr).to(dt)
        _, spread = torch_grad(xs, lambda t: torch.max(torch.abs(fn(t))), dstat.reshape(()))
        want = torch.where(on_ties, dx + spread, dx)
        got = nat().stat_tie_apply_dscale(xs, stat, dscale, dt, 128.0, dt, ties, dx.clone(), 1, 1, n, pre_op=pre)
        if not torch.equal(bits(got), bits(want)):
            bad.append((count, 'apply_dscale', int((bits(got) != bits(want)).sum())))
        for total in (count, count + 5):
            total_t = torch.tensor([total], device=DEV, dtype=torch.int64)
            share = dstat / total_t
            want = torch.where(on_ties, dx + share * torch.sign(fn(xs)), dx)
            got = nat().stat_tie_apply(nat().MATCH_ABS, xs, stat, dstat, ties, dx.clone(), 1, 1, n, True,
                                       total_ties=total_t, pre_op=pre)
            if not torch.equal(bits(got), bits(want)):
                bad.append((count, 'apply total=%d' % total, int((bits(got) != bits(want)).sum())))
    assert not bad, '(ties, deposit, differing elements): %s' % bad


def test_per_tensor_weight_quantizer_step_with_1025_ties():
    """RescalingIntQuant with a whole-tensor AbsMax scale (signed, not narrow: int_threshold 128) through the module
    surface, float32, against the reference's graph in plain torch on the device, w.grad bit for bit.  The inputs sit
    on a dyadic grid -- the maximum 4.0 with 1025 ties of either sign, everything else a multiple of 2^-7 below 1, the
    gradients +-0.5, +-1, +-2 -- so the scale is 2^-5 and every term of the scale gradient is a multiple of 2^-3: sums
    below 2^24 of those are exact in float32 in any order and any grouping (asserted in float64 on the CPU)."""
    from test_gpu_modules import mods
    n = flat_len('f32')
    _, mask = flat_input('f32', 'abs', TIE_CAP + 1)
    gen = torch.Generator().manual_seed(9)
    w0 = torch.randint(-127, 128, (n,), generator=gen).float() * 2.0 ** -7
    sign = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0)
    w0 = torch.where(mask, STAT * sign, w0)
    assert int(mask.sum()) == TIE_CAP + 1 and float(w0[~mask].abs().max()) < 1.0
    assert bool((w0[mask] > 0).any()) and bool((w0[mask] < 0).any())
    gy0 = 2.0 ** torch.randint(-1, 2, (n,), generator=gen).float()
    gy0 = gy0 * torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0)
    # exactness, in float64: v = w / scale, q = clamp(round(v)); the graph sums gy q and gy v (unclamped elements),
    # the kernels gy (q - v) or gy q
    v = w0.double() / 2.0 ** -5
    q = torch.round(v).clamp(-128.0, 127.0)
    inside = v <= 127.0
    terms = torch.cat([gy0.double() * q, (gy0.double() * v)[inside]])
    unit = 2.0 ** -3
    assert torch.equal(terms / unit, torch.round(terms / unit)) and float(terms.abs().sum()) / unit < 2.0 ** 24

    m = mods()
    w = torch.nn.Parameter(w0.to(DEV))
    quant = m['RescalingIntQuant'](
        m['IntQuant'](narrow_range=False, signed=True, float_to_int_impl=m['RoundSte'](),
                      tensor_clamp_impl=m['TensorClamp']()),
        m['StatsFromParameterScaling'](m['AbsMax'](), m['OverTensorView'](), 0, [w], m['FloatRestrictValue'](), (),
                                       affine_rescaling=False, scaling_min_val=1e-10),
        m['IntScaling'](signed=True, narrow_range=False), m['ZeroZeroPoint'](), m['BitWidthConst'](8)).to(DEV)
    gy = gy0.to(DEV)
    y, scale, _, _ = quant(w)
    y.backward(gy)

    ref = w0.to(DEV).requires_grad_(True)
    stat = torch.max(torch.abs(ref.reshape(-1)))
    threshold = stat + (torch.clamp_min(stat, 1e-10) - stat).detach()          # clamp_min_ste
    ref_scale = threshold / torch.tensor(128.0, device=DEV)
    zero = torch.tensor(0.0, device=DEV)
    t = ref / ref_scale + zero
    t = t + (torch.round(t) - t).detach()                                       # round_ste
    lo, hi = torch.tensor(-128.0, device=DEV), torch.tensor(127.0, device=DEV)
    t = torch.where(t > hi, hi, t)                                              # tensor_clamp
    t = torch.where(t < lo, lo, t)
    ref_y = (t - zero) * ref_scale
    ref_y.backward(gy)
    assert float(ref_scale.detach()) == 2.0 ** -5
    assert torch.equal(bits(scale.detach().reshape(1)), bits(ref_scale.detach().reshape(1)))
    assert torch.equal(y.detach(), ref_y.detach())      # (values: the subject is the gradient)
    assert torch.equal(bits(w.grad), bits(ref.grad))
    # the statistic's gradient did reach the ties: a clamped tie (+4.0 -> 128 > 127) has no other gradient
    clamped = (w0 == STAT).to(DEV)
    assert bool((w.grad[clamped] != 0).all()) and w.grad[clamped].unique().numel() == 1


# ---- C: statistic modules along a dim, one channel and many ----------------------------------------------------------

def _abs_max_dim(t, dim):
    return torch.max(torch.abs(t), dim=dim)[0]


def _l2(t):
    per_channel_max = _abs_max_dim(t, 1)
    return torch.norm(per_channel_max, p=2) / math.sqrt(per_channel_max.view(-1).shape[0])


def _negative_min_or_zero(t):
    min_val = torch.min(t, dim=1)[0]
    zero = torch.zeros((), dtype=min_val.dtype, device=min_val.device)
    return torch.where(min_val <= zero, min_val, zero)


MODULES = {   # name: (constructor arguments, the reference's expression on the [C, K] view)
    'AbsMax': ((1,), lambda t: _abs_max_dim(t, 1)),
    'AbsMinMax': ((1,), lambda t: torch.abs(torch.max(t, dim=1)[0] - torch.min(t, dim=1)[0])),
    'NegativeMinOrZero': ((1,), _negative_min_or_zero),
    'AbsMaxAve': ((1,), lambda t: torch.mean(_abs_max_dim(t, 1))),
    'AbsMaxL2': ((1,), _l2),
    'AbsMax0': ((0,), lambda t: _abs_max_dim(t, 0)),
}


def _module(name):
    import brevitas_amd.core.stats as S
    return getattr(S, name.rstrip('0'))(*MODULES[name][0])


def _planted_row(k, gen):
    """k values in [-2, 2] with the extrema planted: -5 at 7 and k - 7 (the minimum twice, and the first tie of
    max |x|), +5 at 20 and k - 5 (the maximum twice)"""
    row = torch.rand(k, generator=gen) * 4 - 2
    row[[7, k - 7]] = -5.0
    row[[20, k - 5]] = 5.0
    return row


#            id            shape           view permutation    modules
ONE_CHANNEL = [
    ('1x40', (1, 40), None, ('AbsMax', 'AbsMinMax', 'NegativeMinOrZero', 'AbsMaxAve', 'AbsMaxL2')),
    ('1x4099', (1, 4099), None, ('AbsMax', 'AbsMinMax', 'NegativeMinOrZero', 'AbsMaxAve', 'AbsMaxL2')),
    ('1x4099const', (1, 4099), None, ('AbsMax', 'AbsMinMax', 'NegativeMinOrZero', 'AbsMaxAve', 'AbsMaxL2')),
    ('4099x1', (4099, 1), None, ('AbsMax0',)),
    ('1x3x5x5', (1, 3, 5, 5), (), ('AbsMax', 'AbsMinMax', 'NegativeMinOrZero', 'AbsMaxAve', 'AbsMaxL2')),
    ('5x1x4x4', (5, 1, 4, 4), (1, 0, 2, 3), ('AbsMax', 'AbsMinMax', 'NegativeMinOrZero', 'AbsMaxAve', 'AbsMaxL2')),
]


@functools.lru_cache(None)
def one_channel_input(case, dn):
    shape = next(c[1] for c in ONE_CHANNEL if c[0] == case)
    k = math.prod(shape)
    if case.endswith('const'):
        return torch.full(shape, -1.5).to(DT[dn])      # every element ties, more of them than the tie list holds
    return _planted_row(k, torch.Generator().manual_seed(31)).reshape(shape).to(DT[dn])


def _view(perm):
    from brevitas_amd.core.function_wrapper import OverOutputChannelView
    if perm is None:
        return lambda t: t                              # already [C, K] (or [K, C] for dim 0)
    return OverOutputChannelView(perm or None)


def check_module(name, x, perm, gout):
    """the module against its expression in torch, both behind the same view: the statistic bit for bit, the gradient
    bit for bit -- as values behind a permuting view"""
    view = _view(perm)
    xi = x.clone().requires_grad_(True)
    out = _module(name)(view(xi))
    want_out, want = torch_grad(x, lambda t: MODULES[name][1](view(t)), gout.reshape(out.shape))
    assert out.shape == want_out.shape and torch.equal(bits(out.detach().reshape(-1)), bits(want_out.reshape(-1))), name
    out.backward(gout.reshape(out.shape))
    if perm:
        assert torch.equal(xi.grad, want), name
    else:
        assert torch.equal(bits(xi.grad), bits(want)), name
    return want


@dtypes
@pytest.mark.parametrize('case', [c[0] for c in ONE_CHANNEL])
def test_one_channel_statistic_along_a_dim_deposits_on_the_first_tie(case, dn):
    _, shape, perm, names = next(c for c in ONE_CHANNEL if c[0] == case)
    x = one_channel_input(case, dn).to(DEV)
    gout = torch.tensor([1.5], device=DEV, dtype=DT[dn])
    for name in names:
        want = check_module(name, x, perm, gout)
        if name in ('AbsMax', 'AbsMax0'):   # the rule itself, whatever torch does: one element holds the gradient
            assert int((want != 0).sum()) == 1


MANY = (3, 4, 5000)     # (outer, channels, inner): a channel spans several units and all three outer slices


@functools.lru_cache(None)
def many_channel_input(dn):
    """channel 0: max |x| three times, in two slices and two units -- (1, 100) is the first in (outer, inner) order;
    channel 1: all equal; channel 2: all zero; channel 3: the maximum and the minimum twice each, the later slice
    holding the earlier inner position"""
    gen = torch.Generator().manual_seed(41)
    x = torch.rand(MANY, generator=gen) * 4 - 2
    x[1, 0, 4500], x[2, 0, 10], x[1, 0, 100] = 5.0, -5.0, -5.0
    x[:, 1, :] = -1.5
    x[:, 2, :] = 0.0
    x[2, 3, 4999], x[0, 3, 3000] = 5.0, 5.0
    x[1, 3, 0], x[0, 3, 4999] = -5.0, -5.0
    return x.to(DT[dn])


@dtypes
def test_many_channel_statistic_along_a_dim_deposits_on_the_first_tie(dn):
    x = many_channel_input(dn).to(DEV)
    gout = torch.tensor([1.5, -2.0, 0.75, 3.0], device=DEV, dtype=DT[dn])
    g1 = torch.tensor([1.5], device=DEV, dtype=DT[dn])
    for name in ('AbsMax', 'AbsMinMax', 'NegativeMinOrZero', 'AbsMaxAve', 'AbsMaxL2'):
        scalar = name in ('AbsMaxAve', 'AbsMaxL2')
        want = check_module(name, x, (1, 0, 2), g1 if scalar else gout)
        if name == 'AbsMax':
            assert want[1, 0, 100] == -1.5 and want[0, 1, 0] == 2.0 and want[0, 3, 3000] == 3.0
            assert int((want != 0).sum()) == 3
    # the same layout in place, [outer, channels, inner] as the fused routes hand it to bvq_stat_bwd
    outer, ch, inner = MANY
    rows = lambda t: t.permute(1, 0, 2).reshape(ch, -1)     # noqa: E731
    for kind, fn in (('abs', lambda t: _abs_max_dim(rows(t), 1)), ('max', lambda t: torch.max(rows(t), dim=1)[0]),
                     ('min', lambda t: torch.min(rows(t), dim=1)[0])):
        stat, want = torch_grad(x, fn, gout)
        got = nat().stat_bwd(match_of(kind), x.reshape(-1), stat, gout, outer, ch, inner)
        assert torch.equal(got.reshape(MANY), want), kind
