"""The host-side rules of brevitas_amd/core/quant/_fused.py that decide which bits the kernels produce, each stated once:
the type promotion of scale = statistic / int_threshold (scale_rule), the two descriptor builders (make_desc,
channel_desc), the descriptor <-> `dv` tuple of the C++ autograd node, and the running-statistic buffer test.  Expected
values are literals: the promotion table was evaluated once from the inline code the helper replaced, the descriptors
are the positional forms their call sites used to write out."""
import os
import re
from types import SimpleNamespace

import pytest
import torch

from brevitas_amd import _native as nat
from brevitas_amd.core.quant import _fused

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (x dtype, scaling shape, int_threshold) -> (scale_dtype, thr_div, quot_dtype, thr_bwd); the threshold tensor is float32
RULE = [
    (F32, (), 127.0, (F32, 127.0, F32, 127.0)),
    (F32, (), 7.0, (F32, 7.0, F32, 7.0)),
    (F32, (), 255.0, (F32, 255.0, F32, 255.0)),
    (F32, (), 32767.0, (F32, 32767.0, F32, 32767.0)),
    (F32, (8, 1), 127.0, (F32, 127.0, F32, 127.0)),
    (F32, (8, 1), 7.0, (F32, 7.0, F32, 7.0)),
    (F32, (8, 1), 255.0, (F32, 255.0, F32, 255.0)),
    (F32, (8, 1), 32767.0, (F32, 32767.0, F32, 32767.0)),
    (BF16, (), 127.0, (F32, 127.0, F32, 127.0)),
    (BF16, (), 7.0, (F32, 7.0, F32, 7.0)),
    (BF16, (), 255.0, (F32, 255.0, F32, 255.0)),
    (BF16, (), 32767.0, (F32, 32767.0, F32, 32767.0)),
    (BF16, (8, 1), 127.0, (BF16, 127.0, BF16, 127.0)),
    (BF16, (8, 1), 7.0, (BF16, 7.0, BF16, 7.0)),
    (BF16, (8, 1), 255.0, (BF16, 255.0, BF16, 255.0)),
    (BF16, (8, 1), 32767.0, (BF16, 32768.0, BF16, 32768.0)),   # 32767 is no bfloat16
    (F16, (), 127.0, (F32, 127.0, F32, 127.0)),
    (F16, (), 7.0, (F32, 7.0, F32, 7.0)),
    (F16, (), 255.0, (F32, 255.0, F32, 255.0)),
    (F16, (), 32767.0, (F32, 32767.0, F32, 32767.0)),
    (F16, (8, 1), 127.0, (F16, 127.0, F16, 127.0)),
    (F16, (8, 1), 7.0, (F16, 7.0, F16, 7.0)),
    (F16, (8, 1), 255.0, (F16, 255.0, F16, 255.0)),
    (F16, (8, 1), 32767.0, (F16, 32768.0, F16, 32768.0)),      # nor a float16
]

# the learned-scale route (RescalingIntQuant._learned_scale_args) next to a bfloat16 bit width:
# (value dtype, value shape, int_threshold) -> (scale_dtype, thr_div).  Its 0-dim rows divide by the threshold as
# bfloat16 holds it, where the statistic-scaled routes above keep the host value.
LEARNED_BF16_BIT_WIDTH = [
    (F32, (), 127.0, (F32, 127.0)),
    (F32, (), 32767.0, (F32, 32768.0)),
    (F32, (8, 1), 127.0, (F32, 127.0)),
    (F32, (8, 1), 32767.0, (F32, 32767.0)),
    (BF16, (), 127.0, (BF16, 127.0)),
    (BF16, (), 32767.0, (BF16, 32768.0)),
    (BF16, (8, 1), 127.0, (BF16, 127.0)),
    (BF16, (8, 1), 32767.0, (BF16, 32768.0)),
    (F16, (), 127.0, (F32, 127.0)),
    (F16, (), 32767.0, (F32, 32768.0)),
    (F16, (8, 1), 127.0, (F16, 127.0)),
    (F16, (8, 1), 32767.0, (F16, 32768.0)),
]


@pytest.mark.parametrize('dtype, shape, thr, want', RULE)
def test_scale_rule_table(dtype, shape, thr, want):
    assert tuple(_fused.scale_rule(dtype, shape, thr, F32)) == want
    assert tuple(_fused.scale_rule(dtype, shape, thr)) == want    # float32 is what IntScaling returns: the default


@pytest.mark.parametrize('dtype, shape, thr, want', LEARNED_BF16_BIT_WIDTH)
def test_scale_rule_of_the_learned_scale_route(dtype, shape, thr, want):
    rule = _fused.scale_rule(dtype, shape, thr, BF16, thr_as_stored=True)
    assert (rule.scale_dtype, rule.thr_div) == want


# ---- descriptors -----------------------------------------------------------------------------------------------------

def _same(a, b):
    assert bytes(a) == bytes(b)


def _code(dtype):
    return nat.dtype_code(dtype)


def test_make_desc_per_tensor_plan():
    x, scale, zp = torch.empty(4, 6, dtype=BF16), torch.empty((), dtype=F32), torch.empty((), dtype=F32)
    p = _fused.Plan(1, 1, 24, False, False, F32)
    _same(_fused.make_desc(p, x, scale, zp, -128.0, 127.0, nat.ROUND, False, nat.OUT_DEQUANT),
          nat.QuantDesc(1, 1, 24, nat.BF16, nat.F32, nat.F32, nat.F32, 0, 0, -128.0, 127.0, nat.ROUND,
                        _fused.scalar_mode(), 0, nat.OUT_DEQUANT, nat.PRE_NONE))


def test_make_desc_per_channel_plan():
    x, scale, zp = torch.empty(2, 5, 3, dtype=F16), torch.empty(5, 1, dtype=F16), torch.empty(5, 1, dtype=F16)
    p = _fused.Plan(2, 5, 3, True, True, F16)
    _same(_fused.make_desc(p, x, scale, zp, 0.0, 15.0, nat.FLOOR, True, nat.OUT_INT, nat.PRE_RELU),
          nat.QuantDesc(2, 5, 3, nat.F16, nat.F16, nat.F16, nat.F16, 1, 1, 0.0, 15.0, nat.FLOOR,
                        _fused.scalar_mode(), 1, nat.OUT_INT, nat.PRE_RELU))


def test_make_desc_nhwc_plan():
    x = torch.empty(2, 5, 3, 4, dtype=BF16).contiguous(memory_format=torch.channels_last)
    assert _fused.split_at_channel(x, 1) == (24, 5, 1, True)
    assert _fused.split_at_channel(x.contiguous(), 1) == (2, 5, 12, False)
    assert _fused.split_at_channel(x.contiguous(), 0) == (1, 2, 60, False)
    assert _fused.split_at_channel(x.contiguous(), 3) == (30, 4, 1, False)
    outer, channels, inner, nhwc = _fused.split_at_channel(x, 1)
    p = _fused.Plan(outer, channels, inner, True, False, BF16, nhwc)
    scale, zp = torch.empty(1, 5, 1, 1, dtype=BF16), torch.empty((), dtype=F32)
    _same(_fused.make_desc(p, x.permute(0, 2, 3, 1), scale, zp, -8.0, 7.0, nat.ROUND, False, nat.OUT_DEQUANT),
          nat.QuantDesc(24, 5, 1, nat.BF16, nat.BF16, nat.BF16, nat.F32, 1, 0, -8.0, 7.0, nat.ROUND,
                        _fused.scalar_mode(), 0, nat.OUT_DEQUANT, nat.PRE_NONE))


@pytest.mark.parametrize('channels, scale_dtype', [(16, BF16), (1, F32)])
def test_stats_descriptor(channels, scale_dtype):
    """StatsFakeQuantFn's one-launch forward and the two C++-node entry points: x's dtype, the rule's scale dtype"""
    code = _code(BF16)
    d = _fused.channel_desc(4, channels, 56, BF16, -128.0, 127.0, nat.ROUND, True, scale_dtype=scale_dtype,
                            scale_pc=channels > 1, pre_op=nat.PRE_SIGMOID)
    _same(d, nat.QuantDesc(4, channels, 56, code, code, _code(scale_dtype), nat.F32, int(channels > 1), 0, -128.0,
                           127.0, nat.ROUND, _fused.scalar_mode(), 1, nat.OUT_DEQUANT, nat.PRE_SIGMOID))
    # ... and as the node takes it: the tuple fast_stats_fakequant / fast_act_stats_fakequant wrote out by hand, which
    # _node_dv now writes out once for both without building the struct
    dv = (4, channels, 56, code, code, _code(scale_dtype), nat.F32, int(channels > 1), 0, nat.ROUND,
          _fused.scalar_mode(), 1, nat.OUT_DEQUANT, nat.PRE_SIGMOID, 0)
    assert d.to_dv() == dv
    sp = _fused.StatsPlan(4, channels, 56, (channels, 1) if channels > 1 else (), 1e-8, 127.0)
    assert _fused._node_dv(sp, BF16, scale_dtype, nat.ROUND, True, nat.PRE_SIGMOID) == dv


@pytest.mark.parametrize('dtype', [F32, BF16, F16])
def test_group_and_group_shifted_descriptors(dtype):
    x = torch.empty(6, 64, dtype=dtype)
    code = _code(dtype)
    desc, thr_div = _fused.group_quant_call(x, 32, 32767.0, -7.0, 7.0, True)
    _same(desc, nat.QuantDesc(1, 12, 32, code, code, code, nat.F32, 1, 0, -7.0, 7.0, nat.ROUND, _fused.scalar_mode(), 1,
                              nat.OUT_DEQUANT, nat.PRE_NONE))
    assert thr_div == (32767.0 if dtype == F32 else 32768.0)
    desc, thr_div = _fused.group_shifted_call(x, 16, 15.0, 0.0, 15.0, False)
    _same(desc, nat.QuantDesc(1, 24, 16, code, code, code, code, 1, 1, 0.0, 15.0, nat.ROUND, _fused.scalar_mode(), 0,
                              nat.OUT_DEQUANT, nat.PRE_NONE))
    assert thr_div == 15.0
    # one group in all: still one scale per group
    assert _fused.group_quant_call(x[:1, :32], 32, 7.0, -7.0, 7.0, True)[0].scale_per_channel == 1


def test_weight_list_descriptors():
    from brevitas_amd.core.quant.weight_group import _Entry, _WeightList
    quant = SimpleNamespace(int_scaling_impl=lambda bw: bw)
    tmpl = SimpleNamespace(qmin=-128.0, qmax=127.0, round_mode=nat.FLOOR, clamp_ste=True)
    entries = [_Entry(None, quant, torch.empty(c, 9, dtype=BF16), _fused.StatsPlan(1, c, 9, (c, 1), 1e-8, 32767.0), tmpl,
                      torch.tensor(16.0)) for c in (8, 24)]
    wl = _WeightList(entries)
    for d, it, c in zip(wl.descs, wl.items, (8, 24)):
        _same(d, nat.QuantDesc(1, c, 9, nat.BF16, nat.BF16, nat.BF16, nat.F32, 1, 0, -128.0, 127.0, nat.FLOOR,
                               _fused.scalar_mode(), 1, nat.OUT_DEQUANT, nat.PRE_NONE))
        assert it.int_threshold == 32768.0  # converted to the weight's dtype
    assert wl.scale_dtype == BF16


@pytest.mark.parametrize('shifted', [False, True])
def test_gptq_descriptors(shifted):
    import brevitas_amd.quant as Q
    from brevitas_amd.graph import gptq
    w = torch.nn.Parameter(torch.randn(8, 64))
    quantizer = (Q.ShiftedUint4WeightPerGroupFloat if shifted else Q.Int4WeightPerGroupFloat)(w, 32)
    plan = gptq._plan(quantizer, 64, False)
    assert plan.shifted == shifted and plan.computed
    for dtype in (F32, F16):
        code = _code(dtype)
        fa = gptq.fused_block_args(plan, 8, 64, dtype)
        clamp_ste = quantizer.int_quant.tensor_clamp_impl.bvq_clamp_ste
        _same(fa.desc, nat.QuantDesc(1, 16, 32, code, code, code, code if shifted else nat.F32, 1, int(shifted), plan.qmin,
                                     plan.qmax, nat.ROUND, _fused.scalar_mode(), int(bool(clamp_ste)), nat.OUT_DEQUANT,
                                     nat.PRE_NONE))
        assert fa.thr_div == (15.0 if shifted else 7.0) and fa.min_val is not None
    given = gptq._plan(quantizer, 64, True)   # static groups: nothing is computed in the loop, nothing divided
    fa = gptq.fused_block_args(given, 8, 64, F32)
    assert (fa.min_val, fa.thr_div) == (None, 1.0) and fa.desc.zp_per_channel == int(shifted)


# ---- descriptor <-> dv -----------------------------------------------------------------------------------------------

def test_dv_round_trip_in_the_order_the_node_reads():
    d = nat.QuantDesc(3, 5, 7, nat.BF16, nat.F32, nat.F16, nat.BF16, 1, 0, -8.0, 7.0, nat.FLOOR, 1, 1, nat.OUT_INT,
                      nat.PRE_TANH, 2)
    dv = d.to_dv()
    assert dv == (3, 5, 7, nat.BF16, nat.F32, nat.F16, nat.BF16, 1, 0, nat.FLOOR, 1, 1, nat.OUT_INT, nat.PRE_TANH, 2)
    _same(nat.QuantDesc.from_dv(dv, d.qmin, d.qmax), d)
    # the node hands back its own entries behind the descriptor's 15 (desc_ints): they are not the descriptor's
    _same(nat.QuantDesc.from_dv(list(dv) + [nat.F16, 0, nat.F32], -8.0, 7.0), d)
    # ... and the order is the one desc_from() of the node reads
    src = open(os.path.join(ROOT, 'brevitas_amd', 'csrc', 'bvq_autograd.cpp')).read()
    body = src[src.index('bvq_quant_desc desc_from('):]
    body = body[:body.index('return d;')]
    read = sorted((int(i), f) for f, i in re.findall(r'd\.(\w+) = (?:\(int32_t\))?dv\[(\d+)\]', body))
    assert [f for _, f in read] == list(nat.QuantDesc.DV_FIELDS) and [i for i, _ in read] == list(range(15))


def test_fallback_rebuilds_the_descriptor_of_the_node(monkeypatch):
    seen = {}
    monkeypatch.setattr(_fused, 'stats_backward', lambda *a: seen.setdefault('args', a))
    d = _fused.channel_desc(2, 5, 7, BF16, -128.0, 127.0, nat.ROUND, True, pre_op=nat.PRE_SIGMOID)
    scale = torch.ones(5, dtype=BF16)
    _fused._fast_backward_fallback('x', scale, 'zp', 'stat', 'thr', list(d.to_dv()) + [nat.BF16, 0, nat.BF16],
                                   [-128.0, 127.0, 128.0, 127.0], (5, 1), 'gy', None)
    xc, sc, zp, stat, thr, desc, sp, group, pre_op, back, gy, gscale = seen['args']
    _same(desc, d)
    assert tuple(sp) == (2, 5, 7, 127.0) and sc.shape == (5, 1) and (group, pre_op, back) == (None, nat.PRE_SIGMOID, None)


# ---- running-statistic buffer ----------------------------------------------------------------------------------------

def _buffer(is_cuda=True, contiguous=True, numel=16, dtype=F32):
    """what _running_buffer reads of a tensor (a device tensor cannot be made here)"""
    return SimpleNamespace(is_cuda=is_cuda, is_contiguous=lambda: contiguous, numel=lambda: numel, dtype=dtype)


def test_running_buffer():
    def got(buf, channels=16):
        return _fused._running_buffer(SimpleNamespace(running_stats=buf), channels)

    assert _fused._running_buffer(None, 16) is None
    assert got(torch.zeros(16)) is None                              # a CPU buffer
    assert got(_buffer(is_cuda=False)) is None
    assert got(_buffer(numel=1)) is None and got(_buffer(), channels=8) is None   # another element count
    assert got(_buffer(dtype=torch.float64)) is None and got(_buffer(dtype=torch.int32)) is None
    assert got(_buffer(contiguous=False)) is None                    # a strided view
    assert got(torch.zeros(16, 2)[:, 0]) is None
    for dtype in (F32, BF16, F16):
        ok = _buffer(dtype=dtype)
        assert got(ok) is ok
