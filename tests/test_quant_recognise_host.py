"""core/quant/_recognise.py and the templates the quantizer classes build with it, on CPU modules: a template depends on
the module structure only.  The literals are the dicts and tuples the classes built before the recognition was gathered
in one module (StatsTemplate / GroupTemplate took the dicts' keys, DynamicTemplate the tuple of _fused_args)."""
import pytest
import torch

import brevitas_amd.config as config
import brevitas_amd.quant as Q
from brevitas_amd import _native as nat
from brevitas_amd.core.bit_width import BitWidthParameter
from brevitas_amd.core.function_wrapper import FloorSte, RoundSte, TensorClampSte
from brevitas_amd.core.quant import IntQuant, _recognise as rec
from brevitas_amd.core.quant.delay import DelayWrapper
from brevitas_amd.core.stats import AbsMax, AbsMinMax

import route_cases

R = nat.ROUND


def weight(*shape):
    return torch.nn.Parameter(torch.randn(*shape))


def template(q):
    bw = q.msb_clamp_bit_width_impl()
    if hasattr(q, '_template'):
        return q._template(bw)
    return q._group_template(bw) if hasattr(q, 'group_size') else q._stats_template(bw)


# name -> (factory, (shape, min_val, per_channel, int_thr, qmin, qmax, round_mode, clamp_ste) or None)
STATS = {
    'per_tensor': (lambda: Q.Int8WeightPerTensorFloat(weight(4, 32)), ((), 1e-10, False, 127.0, -127.0, 127.0, R, True)),
    'per_channel': (lambda: Q.Int8WeightPerChannelFloat(weight(4, 32)),
                    ((4, 1), 1e-10, True, 127.0, -127.0, 127.0, R, True)),
    'int4': (lambda: Q.Int4WeightPerChannelFloat(weight(4, 32)), ((4, 1), 1e-10, True, 7.0, -7.0, 7.0, R, True)),
    'shared2': (lambda: Q.Int8WeightPerChannelFloat([weight(4, 32), weight(4, 32)]),
                ((4, 1), 1e-10, True, 127.0, -127.0, 127.0, R, True)),
    'affine': (lambda: route_cases._affine_weight(weight(4, 32)), ((4, 1), None, True, 127.0, -127.0, 127.0, R, True)),
    'act_per_channel': (lambda: Q.Int8ActPerChannelFloat(3, 'stats'),
                        ((1, 3, 1, 1), 1e-10, True, 128.0, -128.0, 127.0, R, False)),
    'act_per_tensor': (lambda: Q.Int8ActPerTensorFloat('stats', scaling_stats_op='max'),
                       ((), 1e-10, False, 128.0, -128.0, 127.0, R, False)),
    'uint_act_per_tensor': (lambda: Q.Uint8ActPerTensorFloat('stats', scaling_stats_op='max'),
                            ((), 1e-10, False, 255.0, 0.0, 255.0, R, False)),
    'affine_act': (lambda: route_cases._affine_act(3), ((1, 3, 1, 1), None, True, 128.0, -128.0, 127.0, R, False)),
    # no stats-scaled template: a power-of-two int scaling, a statistics zero-point, a learned scale
    'fixed_point': (lambda: Q.Int8WeightPerChannelFixedPoint(weight(4, 32)), None),
    'shifted': (lambda: Q.ShiftedUint8WeightPerChannelFloat(weight(4, 32)), None),
    'from_stats': (lambda: Q.Int8ActPerTensorFloat('parameter_from_stats', 2, scaling_stats_op='max'), None),
    'min_max_init': (lambda: Q.Int8ActPerTensorFloatMinMaxInit(-1.0, 1.0), None),
}
GROUPS = {   # (shape, min_val, int_thr, qmin, qmax, clamp_ste, shifted)
    'group16': (lambda: Q.Int8WeightPerGroupFloat(weight(4, 32), 16), ((8, 1), 1e-10, 127.0, -127.0, 127.0, True, False)),
    'int4_group16': (lambda: Q.Int4WeightPerGroupFloat(weight(4, 32), 16), ((8, 1), 1e-10, 7.0, -7.0, 7.0, True, False)),
    'shifted_group16': (lambda: Q.ShiftedUint8WeightPerGroupFloat(weight(4, 32), 16),
                        ((8, 1), 1e-10, 255.0, 0.0, 255.0, True, True)),
    'mse': (lambda: Q.Int8WeightPerGroupFloatMSE(weight(4, 32), 16), ((8, 1), 1e-10, 127.0, -127.0, 127.0, True, False)),
    'group48': (lambda: Q.Int8WeightPerGroupFloat(weight(4, 96), 48), None),
}
SYMMETRIC, SHIFTED = (False, 1e-10, 128.0, -128.0, 127.0, R, False), (True, 1e-10, 255.0, 0.0, 255.0, R, False)
DYNAMICS = {
    'Int8DynamicActPerTensorFloat': SYMMETRIC, 'Int8DynamicActPerRowFloat': SYMMETRIC,
    'Int8DynamicActPerGroupFloat': SYMMETRIC, 'ShiftedUint8DynamicActPerTensorFloat': SHIFTED,
    'ShiftedUint8DynamicActPerRowFloat': SHIFTED, 'ShiftedUint8DynamicActPerGroupFloat': SHIFTED,
}


@pytest.mark.parametrize('name', sorted(STATS))
def test_stats_template(name):
    factory, want = STATS[name]
    q = factory().train()
    t = template(q)
    if want is None:
        assert t is None
        return
    assert type(t) is rec.StatsTemplate
    assert (t.shape, t.min_val, t.per_channel, t.int_thr, t.qmin, t.qmax, t.round_mode, t.clamp_ste) == want
    sc = q.scaling_impl
    if name.startswith(('act', 'uint_act', 'affine_act')):
        assert t.runtime is sc.runtime_stats and t.weight is None and t.shared is None
        assert t.view is sc.runtime_stats.stats_input_view_shape_impl
    else:
        pls = sc.parameter_list_stats
        assert t.runtime is None and t.weight is pls.first_tracked_param.parameter
        assert t.view is pls.first_tracked_param.view_shape_impl
        if name == 'shared2':
            assert len(t.shared) == 2 and t.shared[0] is t.weight
            assert t.shared[1] is pls.extra_tracked_params_list[0].parameter
        else:
            assert t.shared is None
    assert t.post is (sc.stats_scaling_impl if name.startswith('affine') else None)


@pytest.mark.parametrize('name', sorted(GROUPS))
def test_group_template(name):
    factory, want = GROUPS[name]
    q = factory()
    t = template(q)
    if want is None:
        assert t is None
        return
    assert type(t) is rec.GroupTemplate and t[1:] == want
    assert t.weight is q.scaling_impl.parameter_list_stats.first_tracked_param.parameter
    assert (t['int_thr'], t['qmin'], t['shifted']) == (t.int_thr, t.qmin, t.shifted) and t[0] is t.weight   # by key too


@pytest.mark.parametrize('name', sorted(DYNAMICS))
def test_dynamic_template(name):
    t = template(getattr(Q, name)())
    assert type(t) is rec.DynamicTemplate and tuple(t) == DYNAMICS[name]


# ---- one deviation each: no template (or, for a map that is no plain lower bound, the `post` form above) ----------------

def _delay(q):
    q.int_quant.delay_wrapper = DelayWrapper(3)


def _learned_bit_width(q):
    q.msb_clamp_bit_width_impl = BitWidthParameter(8)


def _other_statistic(q):
    sc = q.scaling_impl
    stats = sc.parameter_list_stats.stats if hasattr(sc, 'parameter_list_stats') else \
        sc.runtime_stats.stats if hasattr(sc, 'runtime_stats') else sc.stats
    other = AbsMax if type(stats.stats_impl) is AbsMinMax else AbsMinMax
    stats.stats_impl = other(stats.stats_impl.stats_reduce_dim)


def _own_int_quant(q):
    q.zero_point_impl.scale_shift_zero_point.int_quant = IntQuant(False, False, RoundSte(), TensorClampSte())


def _signed(q):
    q.int_quant.signed = True


def _narrow(q):
    q.int_quant.narrow_range = True


def _floor(q):
    q.int_quant.float_to_int_impl = FloorSte()


PLAIN = (lambda: Q.Int8WeightPerChannelFloat(weight(4, 32)), lambda: Q.Int8ActPerChannelFloat(3, 'stats').train(),
         lambda: Q.Int8WeightPerGroupFloat(weight(4, 32), 16), lambda: Q.Int8DynamicActPerRowFloat())
SHIFTED_ONES = (lambda: Q.ShiftedUint8WeightPerGroupFloat(weight(4, 32), 16),
                lambda: Q.ShiftedUint8DynamicActPerRowFloat(), lambda: Q.ShiftedUint8DynamicActPerTensorFloat())


@pytest.mark.parametrize('deviate', [_delay, _learned_bit_width, _other_statistic])
@pytest.mark.parametrize('factory', PLAIN + SHIFTED_ONES)
def test_one_deviation_gives_no_template(factory, deviate):
    q = factory()
    assert template(q) is not None
    q = factory()
    deviate(q)
    assert template(q) is None


@pytest.mark.parametrize('deviate', [_own_int_quant, _signed, _narrow, _floor])
@pytest.mark.parametrize('factory', SHIFTED_ONES)
def test_one_deviation_of_the_shifted_graph_gives_no_template(factory, deviate):
    q = factory()
    deviate(q)
    assert template(q) is None


def test_rounding_modes_the_symmetric_graphs_take():
    """the stats-scaled and the dynamic symmetric graphs carry any known rounding; the group walk rounds half to even"""
    for factory in PLAIN:
        q = factory()
        _floor(q)
        t = template(q)
        if hasattr(q, 'group_size') and not hasattr(q, '_template'):
            assert t is None
        else:
            assert t.round_mode == nat.FLOOR


def test_kernel_and_plain_int_quant():
    q = Q.Int8WeightPerChannelFloat(weight(4, 32))
    iq, bw = q.int_quant, q.msb_clamp_bit_width_impl()
    assert rec.kernel_int_quant(iq, bw) == (8, R, True)
    assert rec.plain_int_quant(iq, q.int_scaling_impl, bw) == (-127.0, 127.0, R, True, 127.0)
    learned = BitWidthParameter(8)()
    assert rec.kernel_int_quant(iq, learned) is None
    assert rec.kernel_int_quant(iq, learned, host_bw=False) == (None, R, True)
    iq.float_to_int_impl = torch.nn.Identity()
    assert rec.kernel_int_quant(iq, bw) is None and rec.kernel_int_quant(iq, bw, rounding=False) == (8, None, True)
    iq.tensor_clamp_impl = torch.nn.Identity()
    assert rec.kernel_int_quant(iq, bw, rounding=False) is None
    fixed = Q.Int8WeightPerChannelFixedPoint(weight(4, 32))   # PowerOfTwoIntScaling
    assert rec.plain_int_quant(fixed.int_quant, fixed.int_scaling_impl, fixed.msb_clamp_bit_width_impl()) is None


def test_same_tensor():
    w = weight(4, 32)
    assert rec.same_tensor(w, w) and rec.same_tensor(w, w.detach()) and rec.same_tensor(w, w.view(4, 32))
    assert not rec.same_tensor(w, w.detach().clone())          # a tracked weight that is another tensor
    assert not rec.same_tensor(w, w.view(8, 16)) and not rec.same_tensor(w, w.t()) and not rec.same_tensor(w, w[1:])
    assert not rec.same_tensor(w, w.detach().view(torch.int32))
    assert not rec.same_tensor(w, torch.as_strided(w.detach(), (4, 16), (32, 2)))
    assert not rec.same_tensor(w[:1], torch.as_strided(w.detach(), (1, 32), (1, 1)))   # both contiguous


@pytest.mark.parametrize('factory', [PLAIN[1], PLAIN[2], PLAIN[3], SHIFTED_ONES[0], SHIFTED_ONES[1]])
def test_template_cache(factory, monkeypatch):
    q = factory()
    t = template(q)
    assert t is not None and template(q) is t
    monkeypatch.setattr(config, 'FUSED_PATHS', False)
    assert template(q) is None
    monkeypatch.setattr(config, 'FUSED_PATHS', True)
    t2 = template(q)
    assert t2 == t and t2 is not t and template(q) is t2
    q.int_quant.float_to_int_impl = RoundSte()
    t3 = template(q)
    assert t3 == t and t3 is not t2
    if hasattr(q.scaling_impl, 'runtime_stats'):   # frozen statistics: the scale no longer reads x
        q.eval()
        assert template(q) is None
        q.train()
        assert template(q) == t and template(q) is not t3


def test_group_sizes_are_one_constant():
    from brevitas_amd.core.quant import dynamic, mx
    from brevitas_amd.graph import gptq
    assert rec.GROUP_SIZES == (16, 32, 64, 128, 256) and mx.GROUP_SIZES is rec.GROUP_SIZES
    assert gptq._FUSED_GROUPS == (16, 32, 64, 128) and dynamic.rec is rec
