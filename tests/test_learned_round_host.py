"""Learned rounding (core/function_wrapper/learned_round.py, graph/learned_round.py) on the composed route, which needs no
device: known answers on exactly representable inputs, the module surface, the bookkeeping of learned_round_mode, and
that optimising the offsets beats round-to-nearest.

Bars.  Hard offsets after learned_round_init: equal to the RoundSte quantizer on every element (no input is a tie).
Soft offsets: max |y / scale - clamp(t)| <= eps, one ulp of the dtype at 1: the fractional parts are multiples of 1 / 8, so
floor + offset and the dequantization are exact once the offset is, and the offset (below 1) is reproduced up to the
rounding of `value` (|value| < 2.4, slope of h at most 0.3) and of the ops behind the sigmoid, a few quarter-ulps at 1.
(Measured: eps / 2 at the most.  A per-element ulp cannot hold: elements with a small |t| reach 4 of theirs.)  Gradient of `value`: float64 central
differences on the CPU route.  "It works": the caps of the issue, conditions and not measurements -- an output error at
most 0.8 of round-to-nearest's and at least 5 % of the codes changed (measured with this recipe on the CPU route:
0.45 - 0.57 and 13 - 17 %, profiles/learned_round.md)."""
import math

import pytest
import torch

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
SCALE = 2.0 ** -4
IMPLS = [('hard_sigmoid', {}), ('hard_sigmoid', dict(learned_round_zeta=1.2, learned_round_gamma=-0.2)),
         ('sigmoid', {}), ('sigmoid', dict(learned_round_temperature=0.5))]


def make_impl(kind, kwargs):
    from brevitas_amd.core.function_wrapper import LearnedRoundHardSigmoid, LearnedRoundSigmoid
    return (LearnedRoundHardSigmoid if kind == 'hard_sigmoid' else LearnedRoundSigmoid)(**kwargs)


def exact_inputs(dtype):
    """x = scale * (k + r), k in -8..7, r in {1, 2, 3, 5, 6, 7} / 8: exact in all three dtypes, no tie, both ends of
    the 4-bit range (7.875 rounds to 8 and clips)"""
    k = torch.arange(-8, 8, dtype=torch.float32).reshape(-1, 1)
    r = torch.tensor([1, 2, 3, 5, 6, 7], dtype=torch.float32).reshape(1, -1) / 8
    return (SCALE * (k + r)).to(dtype)


def int_quant_pair(impl, x, bits=4):
    """(IntQuant with learned rounding initialised for x, the RoundSte IntQuant, its operands)"""
    from brevitas_amd.core.bit_width import BitWidthConst
    from brevitas_amd.core.function_wrapper import LearnedRoundSte, TensorClampSte, learned_round_init
    from brevitas_amd.core.quant.int_base import IntQuant
    scale = torch.tensor(SCALE, dtype=x.dtype)
    zp = torch.tensor(0.0, dtype=x.dtype)
    bw = BitWidthConst(bits)()
    t = x / scale + zp
    lr = LearnedRoundSte(impl, learned_round_init(impl, t))
    learned = IntQuant(False, True, float_to_int_impl=lr, tensor_clamp_impl=TensorClampSte())
    nearest = IntQuant(False, True, tensor_clamp_impl=TensorClampSte())
    return learned, nearest, (scale, zp, bw), t


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('kind,kwargs', IMPLS)
def test_known_answers_on_exact_inputs(dtype, kind, kwargs):
    x = exact_inputs(dtype)
    learned, nearest, ops, t = int_quant_pair(make_impl(kind, kwargs), x)
    want = nearest(*ops, x)
    learned.eval()
    hard = learned(*ops, x)
    assert hard.dtype == dtype and torch.equal(hard, want)
    learned.train()
    soft = learned(*ops, x)
    err = (soft.float() / SCALE - t.float().clamp(-8.0, 7.0)).abs().max().item()
    ulp = torch.finfo(dtype).eps
    print('soft error %s %s: %.3g (one ulp at 1: %.3g)' % (kind, dtype, err, ulp))
    assert err <= ulp


@pytest.mark.parametrize('kind,kwargs', IMPLS)
def test_init_is_finite_at_zero_and_near_one(kind, kwargs):
    from brevitas_amd.core.function_wrapper import learned_round_init
    impl = make_impl(kind, kwargs)
    t = torch.tensor([0.0, -3.0, 5.0, 1.0 - 2.0 ** -24, 2.0 ** -30])
    v = learned_round_init(impl, t)
    assert bool(torch.isfinite(v).all())
    if kind == 'hard_sigmoid' and not kwargs:
        assert abs(v[0].item() + math.log(11.0)) < 1e-6


def test_init_refuses_another_module():
    from brevitas_amd.core.function_wrapper import learned_round_init
    with pytest.raises(TypeError, match='learned-round impl'):
        learned_round_init(torch.nn.Identity(), torch.zeros(3))


def test_float16_product_agreement_against_brute_force():
    """f16_products_agree(s): no finite float16 a has RN16(RN32(a * s)) != RN16(a * s); numpy rounds float64 -> float16
    once, and a * s is exact in float64"""
    import numpy as np
    from brevitas_amd.core.function_wrapper.learned_round import f16_products_agree
    a = np.arange(65536, dtype=np.uint16).view(np.float16)
    a = a[np.isfinite(a)].astype(np.float64)
    for scalar, want in ((1.2000000000000002, True), (1.4, False), (1.0, True), (0.5, True), (1.1, None), (3.3333, None),
                         (1.0 / 0.7, None)):
        s32 = np.float32(scalar)
        exact = a * np.float64(s32)
        with np.errstate(over='ignore'):
            once, twice = exact.astype(np.float16), exact.astype(np.float32).astype(np.float16)
        differ = bool(((once != twice) & np.isfinite(once) & np.isfinite(twice)).any())
        got = f16_products_agree(float(s32))
        assert got == (not differ) or (differ is False and got is False), scalar   # conservative: may refuse a safe one
        if want is not None:
            assert got is want, scalar
    from brevitas_amd.core.function_wrapper import LearnedRoundHardSigmoid, LearnedRoundSigmoid
    assert LearnedRoundHardSigmoid().bvq_f16_ok() and not LearnedRoundHardSigmoid(1.2, -0.2).bvq_f16_ok()
    assert not LearnedRoundSigmoid().bvq_f16_ok()


# ---- module surface --------------------------------------------------------------------------------------------------

def linear(factory, inf=32, outf=16, **kw):
    import brevitas_amd.quant as Q
    from brevitas_amd.nn import QuantLinear
    f = getattr(Q, factory)
    return QuantLinear(inf, outf, bias=False, weight_quant=lambda w: f(w, **kw))


def test_state_dict_key_and_view_rule():
    from brevitas_amd.core.function_wrapper import LearnedRoundHardSigmoid, LearnedRoundSte
    from brevitas_amd.graph import insert_learned_round, remove_learned_round
    torch.manual_seed(0)
    layer = linear('Int4WeightPerGroupFloat', group_size=16)
    lr = insert_learned_round(layer)
    assert 'weight_quant.int_quant.float_to_int_impl.value' in layer.state_dict()
    assert lr.value.shape == layer.weight.shape and lr.training and not layer.weight.requires_grad
    assert not hasattr(lr, 'bvq_round_mode')
    y = layer.quant_weight()[0]          # the generic group-wise route regroups the weight: value is viewed as [32, 16]
    assert y.shape == layer.weight.shape and y.grad_fn is not None
    remove_learned_round(layer, harden=False)
    assert layer.weight.requires_grad and 'weight_quant.int_quant.float_to_int_impl.value' not in layer.state_dict()
    m = LearnedRoundSte(LearnedRoundHardSigmoid(), torch.zeros(4, 6))
    assert m(torch.zeros(3, 8)).shape == (3, 8)
    with pytest.raises(ValueError, match=r'\(4, 6\).*\(5, 5\)'):
        m(torch.zeros(5, 5))


@pytest.mark.parametrize('kind,kwargs', IMPLS)
@pytest.mark.parametrize('ste', [True, False])
def test_value_gradient_against_central_differences(kind, kwargs, ste):
    """float64 on the CPU route; inputs beyond the range on both sides, so that the plain clamp masks some and the
    straight-through one passes some"""
    from brevitas_amd.core.bit_width import BitWidthConst
    from brevitas_amd.core.function_wrapper import LearnedRoundSte, TensorClamp, TensorClampSte
    from brevitas_amd.core.quant.int_base import IntQuant
    torch.manual_seed(1)
    x = (torch.randn(6, 8, dtype=torch.float64) * 0.4)
    scale = torch.full((6, 1), 0.07, dtype=torch.float64)
    zp = torch.tensor(0.0, dtype=torch.float64)
    value = torch.randn(6, 8, dtype=torch.float64) * 2.0
    value[0, :4] = torch.tensor([0.0, 30.0, -30.0, math.log(11.0)], dtype=torch.float64)
    lr = LearnedRoundSte(make_impl(kind, kwargs), value)
    iq = IntQuant(False, True, float_to_int_impl=lr, tensor_clamp_impl=TensorClampSte() if ste else TensorClamp())
    bw = BitWidthConst(3)()
    g = torch.randn(6, 8, dtype=torch.float64)

    def loss():
        return (iq(scale, zp, bw, x) * g).sum()
    loss().backward()
    grad = lr.value.grad.clone()
    assert grad.abs().max() > 0
    num = torch.zeros_like(grad)
    eps = 1e-6
    with torch.no_grad():
        for i in range(value.numel()):
            old = lr.value.view(-1)[i].item()
            lr.value.view(-1)[i] = old + eps
            up = loss().item()
            lr.value.view(-1)[i] = old - eps
            down = loss().item()
            lr.value.view(-1)[i] = old
            num.view(-1)[i] = (up - down) / (2 * eps)
    # the hard sigmoid's clamp has a kink at its two edges (|value| = log((zeta - 2 gamma) / -gamma) ...): not compared
    pre = torch.sigmoid(value)
    if kind == 'hard_sigmoid':
        z, gm = lr.learned_round_impl.learned_round_zeta, lr.learned_round_impl.learned_round_gamma
        pre = pre * (z - gm) + gm
    smooth = ((pre - 0.0).abs() > 1e-4) & ((pre - 1.0).abs() > 1e-4)
    assert smooth.sum() >= value.numel() - 2
    # where the sum left the 3-bit range the function is flat: the plain clamp gives 0 like the differences, the
    # straight-through one passes dL/dy * scale * h'(value), compared with h' from the differences of h alone
    with torch.no_grad():
        r = torch.floor(x / scale + zp) + lr.learned_round_impl(value, True)
        inside = (r >= -4.0) & (r <= 3.0)
        dh = (lr.learned_round_impl(value + eps, True) - lr.learned_round_impl(value - eps, True)) / (2 * eps)
    assert 0 < inside.sum() < value.numel()
    assert torch.allclose(grad[smooth & inside], num[smooth & inside], rtol=1e-5, atol=1e-8)
    want_out = g * scale * dh if ste else torch.zeros_like(g)
    assert torch.allclose(grad[smooth & ~inside], want_out[smooth & ~inside], rtol=1e-5, atol=1e-8)


# ---- learned_round_mode ----------------------------------------------------------------------------------------------

def test_refusals_name_the_layer_and_change_nothing():
    import brevitas_amd.quant as Q
    from brevitas_amd.core.function_wrapper import FloorSte
    from brevitas_amd.graph import freeze_weight_quant, learned_round_mode
    torch.manual_seed(0)
    good = linear('Int8WeightPerChannelFloat')
    cases = []
    cases.append((linear('MXInt8Weight'), 'MXQuant'))
    cases.append((linear('Int4WeightPerGroupFloatMSE', group_size=16), 'clip-search'))
    floor = linear('Int8WeightPerChannelFloat')
    floor.weight_quant.int_quant.float_to_int_impl = FloorSte()
    cases.append((floor, 'half-even'))
    frozen = linear('Int8WeightPerChannelFloat')
    with torch.no_grad():
        _, s, z, _ = frozen.quant_weight()
    freeze_weight_quant(frozen, s, z)
    cases.append((frozen, 'frozen'))
    from brevitas_amd.core.bit_width.parameter import BitWidthParameter
    learned_bw = linear('Int8WeightPerChannelFloat')
    learned_bw.weight_quant.msb_clamp_bit_width_impl = BitWidthParameter(4)
    cases.append((learned_bw, 'learned bit width'))
    for bad, why in cases:
        model = torch.nn.Sequential(good, bad)
        before = good.weight_quant.int_quant.float_to_int_impl
        with pytest.raises(TypeError, match=r"layer '1'.*" + why):
            with learned_round_mode(model):
                pass
        assert good.weight_quant.int_quant.float_to_int_impl is before and good.weight.requires_grad
    from brevitas_amd.graph import insert_learned_round
    from brevitas_amd.nn import _QuantWeightMixin

    class OtherLayer(_QuantWeightMixin, torch.nn.Linear):   # a weight-quantized layer of a type the mode does not know
        def __init__(self):
            torch.nn.Linear.__init__(self, 32, 16, bias=False)
            self._init_quant(Q.Int8WeightPerChannelFloat, None)
    other = OtherLayer()
    with pytest.raises(TypeError, match=r"layer '1' \(OtherLayer\).*QuantLinear and QuantConv2d only"):
        with learned_round_mode(torch.nn.Sequential(good, other)):
            pass
    assert good.weight.requires_grad and other.weight.requires_grad
    with pytest.raises(TypeError, match='QuantLinear and QuantConv2d only'):
        insert_learned_round(torch.nn.Linear(4, 4))
    with pytest.raises(ValueError, match='impl'):
        with learned_round_mode(torch.nn.Sequential(good), impl='tanh'):
            pass
    assert good.weight.requires_grad


def test_mode_restores_on_normal_and_exceptional_exit():
    from brevitas_amd.core.function_wrapper import LearnedRoundSte
    from brevitas_amd.graph import learned_round_mode
    torch.manual_seed(0)
    a, b = linear('Int8WeightPerChannelFloat'), linear('ShiftedUint4WeightPerGroupFloat', group_size=16)
    b.weight.requires_grad_(False)
    model = torch.nn.Sequential(a, b)
    impls = [m.weight_quant.int_quant.float_to_int_impl for m in (a, b)]
    w = [m.weight.detach().clone() for m in (a, b)]

    def restored():
        return all(m.weight_quant.int_quant.float_to_int_impl is i for m, i in zip((a, b), impls)) and \
            a.weight.requires_grad and not b.weight.requires_grad and \
            all(torch.equal(m.weight, x) and m._buffers.get('frozen_weight_scale') is None for m, x in zip((a, b), w))
    with learned_round_mode(model, impl='sigmoid', learned_round_temperature=2.0) as lr:
        assert len(lr.parameters()) == 2 and all(p.requires_grad for p in lr.parameters())
        assert all(isinstance(m.weight_quant.int_quant.float_to_int_impl, LearnedRoundSte) for m in (a, b))
        assert not a.weight.requires_grad
        assert lr.regulariser(2.0).item() > 0
    assert restored()
    with pytest.raises(RuntimeError, match='boom'):
        with learned_round_mode(model):
            raise RuntimeError('boom')
    assert restored()


@pytest.mark.parametrize('factory,kw,qmin,qmax', [('Int4WeightPerChannelFloat', {}, -8, 7),
                                                  ('ShiftedUint4WeightPerGroupFloat', dict(group_size=16), 0, 15)])
def test_finish_freezes_integer_codes(factory, kw, qmin, qmax):
    from brevitas_amd.graph import learned_round_mode
    torch.manual_seed(0)
    layer = linear(factory, **kw)
    before = layer.weight_quant.int_quant.float_to_int_impl
    with learned_round_mode(layer) as lr:
        with torch.no_grad():
            lr.parameters()[0].add_(torch.randn_like(lr.parameters()[0]))
        lr.finish()
        assert lr.parameters() == []
    assert layer.weight_quant.int_quant.float_to_int_impl is before and layer.weight.requires_grad
    scale, zp = layer.frozen_weight_scale, layer.frozen_weight_zero_point
    w = layer.weight.detach().reshape(scale.shape[0], -1, layer.weight.shape[1] // max(scale.shape[1] if scale.dim() == 3 else 1, 1))
    s = scale.reshape(scale.shape[0], -1, 1)
    z = zp.reshape(s.shape) if zp.numel() == s.numel() else zp
    codes = w / s + z
    assert torch.allclose(codes, codes.round(), atol=1e-4)
    assert codes.round().min() >= qmin and codes.round().max() <= qmax
    out = layer.quant_weight()
    assert out[0] is layer.weight and out[1] is layer.frozen_weight_scale and out[2] is layer.frozen_weight_zero_point


def test_weight_quant_group_names_a_layer_in_the_mode():
    from brevitas_amd.core.quant.weight_group import WeightQuantGroup
    from brevitas_amd.graph import learned_round_mode
    torch.manual_seed(0)
    model = torch.nn.Sequential(linear('Int8WeightPerChannelFloat'))
    with learned_round_mode(model):
        unc = dict(WeightQuantGroup(model).uncovered)
        assert 'learned rounding' in unc['0.weight_quant']


# ---- it works --------------------------------------------------------------------------------------------------------

def optimise(layer, x, steps=200):
    """the recipe of the issue -> (output error / round-to-nearest's, share of the codes that differ from it)"""
    from brevitas_amd.graph import learned_round_mode
    w = layer.weight.detach().clone()
    with torch.no_grad():
        rtn, scale, zp, _ = layer.quant_weight()
        rtn = rtn.clone()
    with learned_round_mode(layer) as lr:
        opt = torch.optim.Adam(lr.parameters(), lr=1e-2)
        for s in range(steps):
            beta = 20.0 + (2.0 - 20.0) * s / (steps - 1)
            wq = layer.quant_weight()[0]
            loss = (x @ (wq - w).t()).pow(2).mean() + 0.01 * lr.regulariser(beta)
            opt.zero_grad()
            loss.backward()
            opt.step()
        lr.finish()
    q = layer.weight.detach()
    ratio = ((x @ (q - w).t()).pow(2).mean() / (x @ (rtn - w).t()).pow(2).mean()).item()
    s = scale.reshape(w.shape[0], -1, 1)
    g = w.shape[1] // s.shape[1]
    changed = ((q.reshape(w.shape[0], -1, g) / s).round() != (rtn.reshape(w.shape[0], -1, g) / s).round())
    return ratio, changed.float().mean().item()


def works_case(seed, grouped, device='cpu'):
    torch.manual_seed(seed)
    layer = linear('Int4WeightPerGroupFloat', group_size=16) if grouped else linear('Int4WeightPerChannelFloat')
    x = torch.randn(256, 32) @ torch.randn(32, 32) / math.sqrt(32)
    return optimise(layer.to(device), x.to(device))


@pytest.mark.parametrize('seed', [0, 1, 2, 3])
@pytest.mark.parametrize('grouped', [False, True])
def test_it_works(seed, grouped):
    ratio, changed = works_case(seed, grouped)
    print('ratio %.3f changed %.3f' % (ratio, changed))
    assert ratio <= 0.8
    assert changed >= 0.05
