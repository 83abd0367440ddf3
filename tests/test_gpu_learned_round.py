"""Learned rounding on the device (csrc/bvq_learned_round.hip, _fused.LearnedRoundFakeQuantFn, graph/learned_round.py).

No bar of its own: y (soft and hard), dvalue and dx of the two kernels hold the bits of the composed route -- IntQuant
calling LearnedRoundSte op by op -- on the device, and, where the sigmoid leaves no room for a differing expf, on the CPU.
A NaN equals any NaN (its payload is not part of the definition); everything else is compared bit for bit.  float16 with
an impl whose scalar products torch's own float16 kernels round in two ways (`fusable`) is held to its route
instead: IntQuant must leave it composed.  The window
constants are those of the group walk, restated in test_group_walk_host.py."""
import math

import pytest
import torch

import test_learned_round_host as H
from test_group_walk_host import BWD_DEPTH, FWD_DEPTH, LANES, WAVES
from test_gpu_group_walk import use_nt0  # noqa: F401  (the fixture that switches to the forced-NT library)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
DT = {'f32': torch.float32, 'bf16': torch.bfloat16, 'f16': torch.float16}
dtypes = pytest.mark.parametrize('dn', ['f32', 'bf16', 'f16'])
impls = pytest.mark.parametrize('kind,kwargs', H.IMPLS, ids=['hard', 'hard12', 'sigmoid', 'sigmoid05'])
LOG11 = math.log(11.0)


def nat():
    from brevitas_amd import _native
    return _native


def same_bits(a, b):
    """same shape and dtype, NaN where the other has one, the same bits everywhere else"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    it = {4: torch.int32, 2: torch.int16}[a.element_size()]
    a, b = a.contiguous(), b.contiguous()
    na, nb = torch.isnan(a), torch.isnan(b)
    return bool(torch.equal(na, nb)) and bool(torch.equal(a.view(it)[~na], b.view(it)[~nb]))


@pytest.fixture
def launches(monkeypatch):
    """counts the calls of the two launching wrappers"""
    n = nat()
    calls = {}
    for name in ('learned_round_fwd', 'learned_round_bwd'):
        real = getattr(n, name)
        calls[name] = 0

        def counted(*a, _real=real, _name=name, **k):
            calls[_name] += 1
            return _real(*a, **k)
        monkeypatch.setattr(n, name, counted)
    return calls


# ---- inputs ------------------------------------------------------------------------------------------------------------

def window_chunks():
    """16-byte chunks one workgroup owns, forward and backward"""
    return WAVES * FWD_DEPTH * LANES, WAVES * BWD_DEPTH * LANES


def shapes(dtype):
    """(shape, per-channel) at the smallest sizes that can go wrong"""
    vec = 16 // torch.empty((), dtype=dtype).element_size()
    out = [((1, vec), False),            # one chunk
           ((5, 24), True),              # three (six) chunks a row: rows change inside one wave load
           ((6, 16), True), ((3, 128), True)]   # regrouped [R * G, g]
    for win in window_chunks():          # per tensor: one chunk short of, at and one chunk past a workgroup's window
        out += [((c * vec,), False) for c in (win - 1, win, win + 1)]
    return out


def make_case(dtype, shape, per_channel, bits, signed, seed):
    """x with values beyond the range on both sides, exactly at qmin / qmax, +-0 and a NaN; value at 0, at its init, at
    +-log 11 (the inclusive edge of the hard sigmoid's clamp), at +-30 and random; a per-channel integer zero-point for
    the unsigned range, a zero one for the signed"""
    gen = torch.Generator().manual_seed(seed)
    qmin, qmax = (-(2 ** (bits - 1)), 2 ** (bits - 1) - 1) if signed else (0, 2 ** bits - 1)
    rows = shape[0] if per_channel else 1
    n = math.prod(shape)
    scale = (torch.rand(rows, 1, generator=gen) * 0.05 + 0.01).to(dtype)
    if per_channel and not signed:
        zp = torch.randint(1, 2 ** bits - 1, (rows, 1), generator=gen).to(dtype)
    else:
        zp = torch.tensor(0.0, dtype=dtype)
    if not per_channel:
        scale = scale.reshape(())
    span = (qmax - qmin) * 0.75
    t = (torch.rand(shape, generator=gen) - 0.5) * 2 * span + (qmax + qmin) / 2
    x = ((t - zp.float()) * scale.float()).to(dtype)
    flat = x.view(-1)
    sf, zf = scale.float().reshape(-1)[0], zp.float().reshape(-1)[0]
    special = [(qmin - zf) * sf, (qmax - zf) * sf, 0.0, -0.0, float('nan'), (qmax + 5 - zf) * sf, (qmin - 5 - zf) * sf]
    for i, v in enumerate(special[:n]):
        flat[i] = v
    value = (torch.randn(shape, generator=gen) * 2.0).to(dtype)
    vf = value.view(-1)
    for i, v in enumerate([0.0, LOG11, -LOG11, 30.0, -30.0][:max(n - 1, 0)]):
        vf[n - 1 - i] = v
    g = torch.randn(shape, generator=gen).to(dtype)
    return x, value, scale, zp, g


def with_init(impl, x, value, scale, zp):
    """the middle third of value at learned_round_init of the very t"""
    from brevitas_amd.core.function_wrapper import learned_round_init
    t = x / scale + zp
    init = learned_round_init(impl, torch.nan_to_num(t))
    n = value.numel()
    value.view(-1)[n // 3:2 * n // 3] = init.view(-1)[n // 3:2 * n // 3]
    return value


def int_quant(impl, value, bits, signed, ste, device):
    from brevitas_amd.core.bit_width import BitWidthConst
    from brevitas_amd.core.function_wrapper import LearnedRoundSte, TensorClamp, TensorClampSte
    from brevitas_amd.core.quant.int_base import IntQuant
    lr = LearnedRoundSte(impl, value)
    iq = IntQuant(False, signed, float_to_int_impl=lr, tensor_clamp_impl=TensorClampSte() if ste else TensorClamp())
    return iq.to(device), BitWidthConst(bits).to(device)()


def composed(monkeypatch, impl, x, value, scale, zp, g, bits, signed, ste, device):
    """IntQuant op by op on `device` -> (y soft, y hard, dvalue, dx)"""
    import brevitas_amd.config as config
    x, value, scale, zp, g = (t.to(device) for t in (x, value, scale, zp, g))
    iq, bw = int_quant(impl, value, bits, signed, ste, device)
    xr = x.clone().requires_grad_(True)
    with monkeypatch.context() as m:
        m.setattr(config, 'FUSED_PATHS', False)
        y = iq(scale, zp, bw, xr)
        y.backward(g)
        iq.eval()
        with torch.no_grad():
            hard = iq(scale, zp, bw, x)
    return y.detach(), hard, iq.float_to_int_impl.value.grad, xr.grad


def fused(impl, x, value, scale, zp, g, bits, signed, ste):
    """the two kernels through their brevitas_amd._native wrappers -> (y soft, y hard, dvalue, dx)"""
    from brevitas_amd.core.quant import _fused
    from brevitas_amd.function.ops import int_range_host
    n = nat()
    x, value, scale, zp, g = (t.to(DEV) for t in (x, value, scale, zp, g))
    p = _fused.plan(x, scale, zp)
    assert p is not None and p.ct == x.dtype
    qmin, qmax = int_range_host(signed, False, bits)
    sc, zc = scale.reshape(-1).contiguous(), zp.reshape(-1).contiguous()
    desc = _fused.make_desc(p, x, sc, zc, qmin, qmax, n.FLOOR, ste, n.OUT_DEQUANT)
    assert n.learned_round_supported(desc, x, value), n.last_error()
    kind, consts = impl.bvq_learned_round_kind, impl.bvq_constants()
    y = n.learned_round_fwd(desc, x, value, sc, zc, kind, consts, False)
    hard = n.learned_round_fwd(desc, x, value, sc, zc, kind, consts, True)
    dvalue, dx = n.learned_round_bwd(desc, g, x, value, sc, zc, kind, consts, True)
    dvalue2, none = n.learned_round_bwd(desc, g, x, value, sc, zc, kind, consts, False)
    assert none is None and same_bits(dvalue, dvalue2)
    return y, hard, dvalue, dx


def compare(got, want, what):
    for name, a, b in zip(('y soft', 'y hard', 'dvalue', 'dx'), got, want):
        b = b.to(a.device)
        if not same_bits(a, b):
            bad = ~((a == b) | (torch.isnan(a) & torch.isnan(b)))
            idx = bad.nonzero()[:4].tolist()
            raise AssertionError('%s: %s differs at %d elements, first %s: %s vs %s'
                                 % (what, name, int(bad.sum()), idx, a[bad][:4].tolist(), b[bad][:4].tolist()))


def fusable(dtype, impl):
    """float16 takes the kernels only where torch's two float16 roundings of `tensor * scalar` cannot differ:
    the hard sigmoid at its defaults does, at zeta - gamma = 1.4 it does not, the plain sigmoid never"""
    return dtype != torch.float16 or impl.bvq_f16_ok()


def check_declined(monkeypatch, launches, impl, dtype):
    """IntQuant leaves these operands to the composed route: no launch of the kernels, no node of theirs"""
    import brevitas_amd.config as config
    monkeypatch.setattr(config, 'FUSED_PATHS', True)
    for shape, pc in (((5, 24), True), ((1024,), False)):
        x, value, scale, zp, g = (t.to(DEV) for t in make_case(dtype, shape, pc, 4, False, 3))
        iq, bw = int_quant(impl, value, 4, False, True, DEV)
        y = iq(scale, zp, bw, x)
        y.backward(g)
        assert not has_node(y, 'LearnedRoundFakeQuantFnBackward')
        iq.eval()
        with torch.no_grad():
            iq(scale, zp, bw, x)
    assert launches['learned_round_fwd'] == 0 and launches['learned_round_bwd'] == 0


def has_node(t, name):
    seen, todo = set(), [t.grad_fn]
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        if type(fn).__name__ == name:
            return True
        todo += [f for f, _ in fn.next_functions]
    return False


# ---- the kernels against the composed chain on the device -------------------------------------------------------------

@dtypes
@impls
def test_kernels_match_the_composed_chain_on_the_device(dn, kind, kwargs, monkeypatch, launches):
    dtype = DT[dn]
    impl = H.make_impl(kind, kwargs)
    if not fusable(dtype, impl):
        return check_declined(monkeypatch, launches, impl, dtype)
    seed = 0
    for shape, pc in shapes(dtype):
        small = math.prod(shape) <= 512
        for bits, signed, ste in ((3, True, True), (4, False, False), (8, True, False), (4, True, True),
                                  (8, False, True), (3, False, False)):
            if not small and (bits, signed) != (4, False):
                continue   # the window edges: one setting, the walk does not depend on it
            seed += 1
            x, value, scale, zp, g = make_case(dtype, shape, pc, bits, signed, seed)
            value = with_init(impl, x, value, scale, zp)
            want = composed(monkeypatch, impl, x, value, scale, zp, g, bits, signed, ste, DEV)
            got = fused(impl, x, value, scale, zp, g, bits, signed, ste)
            compare(got, want, '%s %s bits %d signed %s ste %s' % (dn, shape, bits, signed, ste))


@dtypes
@impls
def test_kernels_match_the_composed_chain_on_the_cpu(dn, kind, kwargs, monkeypatch, launches):
    """the anchor that does not lean on torch's device kernels: soft offsets with value in {0, +-30}, where sigmoid is
    0.5, 1 or so small that the hard sigmoid's `+ gamma` absorbs it.  The plain sigmoid keeps that small number: in
    float32 its last bit is expf's, so -30 is left to the device comparison there; in bfloat16 sigmoid(-30) = 9.3576e-14
    and sigmoid(-60) = 8.756e-27 lie 0.23 and 0.1 of a bfloat16 spacing from the nearest rounding boundary, thousands of
    float32 ulps, so -30 is anchored.  Hard offsets: arbitrary |value| >= 1e-3"""
    dtype = DT[dn]
    impl = H.make_impl(kind, kwargs)
    if not fusable(dtype, impl):
        return check_declined(monkeypatch, launches, impl, dtype)
    choices = torch.tensor([0.0, 30.0, -30.0] if kind == 'hard_sigmoid' or dn != 'f32' else [0.0, 30.0])
    for i, (shape, pc, bits, signed, ste) in enumerate((((5, 24), True, 4, False, False), ((6, 16), True, 3, True, True),
                                                        ((1000,), False, 8, True, False))):
        x, value, scale, zp, g = make_case(dtype, shape, pc, bits, signed, 100 + i)
        gen = torch.Generator().manual_seed(i)
        soft_value = choices[torch.randint(0, len(choices), shape, generator=gen)].to(dtype)
        want = composed(monkeypatch, impl, x, soft_value, scale, zp, g, bits, signed, ste, 'cpu')
        got = fused(impl, x, soft_value, scale, zp, g, bits, signed, ste)
        compare(got, want, 'soft %s %s' % (dn, shape))
        hard_value = torch.where(value.float().abs() < 1e-3, torch.ones_like(value), value)
        want = composed(monkeypatch, impl, x, hard_value, scale, zp, g, bits, signed, ste, 'cpu')
        got = fused(impl, x, hard_value, scale, zp, g, bits, signed, ste)
        compare(got[1:2], want[1:2], 'hard %s %s' % (dn, shape))


# ---- what the kernels do not cover takes the composed route -------------------------------------------------------------

@dtypes
def test_ragged_rows_and_misaligned_views_take_the_composed_route(dn, monkeypatch, launches):
    import brevitas_amd.config as config
    dtype = DT[dn]
    impl = H.make_impl('hard_sigmoid', {})
    x, value, scale, zp, g = (t.to(DEV) for t in make_case(dtype, (4, 27), True, 4, True, 7))
    base = torch.randn(6 * 16 + 1, device=DEV).to(dtype)
    cases = [('ragged', x, value, scale), ('misaligned', base[1:].view(6, 16), torch.zeros(6, 16, device=DEV, dtype=dtype),
                                            torch.full((6, 1), 0.05, device=DEV, dtype=dtype))]
    for what, xx, vv, ss in cases:
        outs = []
        for on in (True, False):
            monkeypatch.setattr(config, 'FUSED_PATHS', on)
            iq, bw = int_quant(impl, vv.clone(), 4, True, True, DEV)
            y = iq(ss, zp, bw, xx)
            y.backward(torch.ones_like(y))
            outs.append((y.detach(), iq.float_to_int_impl.value.grad))
        assert launches['learned_round_fwd'] == 0 and launches['learned_round_bwd'] == 0, what
        assert same_bits(outs[0][0], outs[1][0]) and same_bits(outs[0][1], outs[1][1]), what
    # the same operands, whole chunks and aligned: the kernels run
    monkeypatch.setattr(config, 'FUSED_PATHS', True)
    iq, bw = int_quant(impl, torch.zeros(6, 16, device=DEV, dtype=dtype), 4, True, True, DEV)
    iq(cases[1][3], zp, bw, base[:96].view(6, 16)).sum().backward()
    assert launches['learned_round_fwd'] == 1 and launches['learned_round_bwd'] == 1


# ---- module level --------------------------------------------------------------------------------------------------------

def layers(dtype):
    import brevitas_amd.quant as Q
    from brevitas_amd.nn import QuantConv2d, QuantLinear
    kw = dict(bias=False, device=DEV, dtype=dtype)
    return [('int8 per channel', lambda: QuantLinear(48, 24, weight_quant=Q.Int8WeightPerChannelFloat, **kw)),
            ('int4 g16', lambda: QuantLinear(48, 24, weight_quant=lambda w: Q.Int4WeightPerGroupFloat(w, 16), **kw)),
            ('int4 g128', lambda: QuantLinear(256, 8, weight_quant=lambda w: Q.Int4WeightPerGroupFloat(w, 128), **kw)),
            ('uint4 g16', lambda: QuantLinear(48, 24, weight_quant=lambda w: Q.ShiftedUint4WeightPerGroupFloat(w, 16),
                                              **kw)),
            ('conv 3x3', lambda: QuantConv2d(8, 16, 3, weight_quant=Q.Int8WeightPerChannelFloat, **kw))]


@dtypes
def test_layers_in_the_mode_take_the_kernels_with_the_composed_bits(dn, monkeypatch, launches):
    import brevitas_amd.config as config
    from brevitas_amd.graph import learned_round_mode
    dtype = DT[dn]
    for name, make in layers(dtype):
        torch.manual_seed(3)
        layer = make()
        g = torch.randn_like(layer.weight)
        with learned_round_mode(layer) as lr:
            value = lr.parameters()[0]
            with torch.no_grad():
                value.add_(torch.randn_like(value) * 0.5)
            outs = {}
            for route, fused_on, w_grad in (('fused', True, False), ('composed', False, False), ('w grad', True, True)):
                monkeypatch.setattr(config, 'FUSED_PATHS', fused_on)
                layer.weight.requires_grad_(w_grad)
                value.grad = None
                before = launches['learned_round_fwd'], launches['learned_round_bwd']
                y = layer.quant_weight()[0]
                y.backward(g)
                ran = launches['learned_round_fwd'] - before[0], launches['learned_round_bwd'] - before[1]
                took = has_node(y, 'LearnedRoundFakeQuantFnBackward')
                assert took == (route == 'fused') and ran == ((1, 1) if took else (0, 0)), (name, route, ran)
                outs[route] = (y.detach(), value.grad.clone())
            layer.weight.requires_grad_(False)
            layer.weight.grad = None
            for route in ('composed', 'w grad'):
                assert same_bits(outs['fused'][0], outs[route][0]) and same_bits(outs['fused'][1], outs[route][1]), \
                    (name, route)
            monkeypatch.setattr(config, 'FUSED_PATHS', True)
            before = launches['learned_round_fwd']
            lr.finish()                                  # eval mode under no_grad: the forward kernel, hard offsets
            assert launches['learned_round_fwd'] == before + 1, name
        assert layer._buffers.get('frozen_weight_scale') is not None


# ---- the NT kernels ----------------------------------------------------------------------------------------------------

@dtypes
@pytest.mark.parametrize('kind,kwargs', [H.IMPLS[0], H.IMPLS[3]], ids=['hard', 'sigmoid05'])
def test_nt_kernels(dn, kind, kwargs, use_nt0, monkeypatch, launches):
    dtype = DT[dn]
    impl = H.make_impl(kind, kwargs)
    if not fusable(dtype, impl):
        return check_declined(monkeypatch, launches, impl, dtype)
    x, value, scale, zp, g = make_case(dtype, (37, 40), True, 4, False, 11)
    want = composed(monkeypatch, impl, x, value, scale, zp, g, 4, False, False, DEV)
    use_nt0()
    got = fused(impl, x, value, scale, zp, g, 4, False, False)
    compare(got, want, 'NT %s' % dn)


# ---- a captured step ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dn', ['f32', 'bf16'])
def test_a_captured_step_replays_to_the_eager_bits(dn, launches):
    import brevitas_amd.quant as Q
    from brevitas_amd.graph import learned_round_mode
    from brevitas_amd.nn import QuantLinear
    from test_gpu_graphs import _capture
    torch.manual_seed(5)
    layer = QuantLinear(64, 32, bias=False, weight_quant=lambda w: Q.Int4WeightPerGroupFloat(w, 16), device=DEV,
                        dtype=DT[dn])
    g = torch.randn_like(layer.weight)
    with learned_round_mode(layer) as lr:
        value = lr.parameters()[0]

        def step():
            value.grad = None
            y = layer.quant_weight()[0]
            y.backward(g)
            return y, value.grad

        graph, (y_s, dv_s) = _capture(step)
        assert launches['learned_round_bwd'] >= 4
        for trial in range(2):
            with torch.no_grad():
                value.add_(torch.randn_like(value))
            graph.replay()
            torch.cuda.synchronize()
            got = y_s.clone(), dv_s.clone()
            y, dv = step()
            assert same_bits(got[0], y.detach()) and same_bits(got[1], dv), trial


# ---- it works ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('seed', [0, 1, 2, 3])
@pytest.mark.parametrize('grouped', [False, True])
def test_it_works_on_the_device(seed, grouped, launches):
    ratio, changed = H.works_case(seed, grouped, DEV)
    print('ratio %.3f changed %.3f' % (ratio, changed))
    assert launches['learned_round_fwd'] == 201 and launches['learned_round_bwd'] == 200   # the fused route, every step
    assert ratio <= 0.8
    assert changed >= 0.05
