"""Dynamic activation quantizers (Int8DynamicAct... / ShiftedUint8DynamicAct..., brevitas_amd.quant) on the composed
route with CPU tensors against golden vectors produced by the reference: its resolved weight graphs applied to
x.reshape(rows, H) with a plain clamp (tests/golden/make_golden_dynamic_act.py), plus the module surface -- shapes, no
state, the errors, the bias-quantizer refusal, calibration pass-through, a layer -- and the argument checks of the C ABI
entries of the row kernels, which need no device.

Bars (tests/dynamic_golden.py): y, scale and zp are bit-exact.  dx is bit-exact except at each row's (group's, the
tensor's) deposit positions; there the asymmetric cases are held to `deposit_ulps` of tests/test_group_shifted_golden.py
with g := the number of elements sharing the statistics, the symmetric ones to the rule of
tests/test_group_quant_golden.py.
"""
import ctypes
import functools

import pytest
import torch

import dynamic_golden as D

CASES = D.CASES
case = pytest.mark.parametrize('c', CASES, ids=D.IDS)
NAMES = ['Int8DynamicActPerTensorFloat', 'Int8DynamicActPerRowFloat', 'Int8DynamicActPerGroupFloat',
         'ShiftedUint8DynamicActPerTensorFloat', 'ShiftedUint8DynamicActPerRowFloat',
         'ShiftedUint8DynamicActPerGroupFloat']


@pytest.fixture(autouse=True)
def cpu_scalar_semantics(monkeypatch):
    """the golden vectors were produced by torch CPU kernels (include/bvq.h, bvq_scalar_mode)"""
    import brevitas_amd.config as config
    monkeypatch.setattr(config, 'SCALAR_OPERAND_MODE', 'cpu')


def test_the_fixture_covers_what_it_says():
    assert sorted({c['quantizer'] for c in CASES}) == sorted(NAMES)
    for name in NAMES:
        mine = [c for c in CASES if c['quantizer'] == name]
        assert {c['dtype'] for c in mine} == {'f32', 'bf16'} and {c['bit_width'] for c in mine} == {4, 8}
        hs = {c['shape'][1] for c in mine}
        assert hs == ({1024} if 'Group' in name else {40, 536, 1032})
        assert all(c['shape'][0] == 12 for c in mine)
        for h in hs:   # every H meets both dtypes and both bit widths
            at = [c for c in mine if c['shape'][1] == h]
            assert {c['dtype'] for c in at} == {'f32', 'bf16'} and {c['bit_width'] for c in at} == {4, 8}
    full = [c for c in CASES if c['granularity'] != 'tensor']
    assert len(full) == 2 * 3 * 4 + 2 * 4   # the per-row and per-group graphs run every (H, dtype, bit width)
    import os
    assert os.path.getsize(os.path.join(D.G.GOLDEN_DIR, 'dynamic_act.npz')) < 512 * 1024


@case
def test_golden_inputs_hold_the_planted_rows(c):
    """the cases cannot be passed on inputs that avoid the corners (the ten rows of make_golden_group_shifted.py)"""
    unit = c['group_size'] or c['shape'][1]
    P = c['planted']
    x = c.torch('x').reshape(-1, unit)
    xf = x.float()
    chunk = 16 // (4 if c['dtype'] == 'f32' else 2)
    assert bool((xf[P['zero']] == 0).all())
    assert bool((xf[P['constant']] == xf[P['constant'], 0]).all()) and float(xf[P['constant'], 0]) != 0
    assert bool((xf[P['positive']] > 0).all()) and bool((xf[P['negative']] < 0).all())
    if c['shifted'] and c['granularity'] != 'tensor':
        zp = c.torch('zp').float().reshape(-1)
        assert float(zp[P['positive']]) == 0 and float(zp[P['negative']]) == 2 ** c['bit_width'] - 1

    def hits(row, fn):
        return torch.nonzero(xf[row] == fn(xf[row])).reshape(-1).tolist()
    assert hits(P['min_far'], torch.min) == [2, unit - 3] and hits(P['max_far'], torch.max) == [1, unit - 2]
    assert 2 // chunk != (unit - 3) // chunk and 1 // chunk != (unit - 2) // chunk
    assert hits(P['min_near'], torch.min) == [5, 6] and hits(P['max_near'], torch.max) == [4, 5]
    assert 5 // chunk == 6 // chunk and 4 // chunk == 5 // chunk
    assert hits(P['ends'], torch.max) == [0] and hits(P['ends'], torch.min) == [unit - 1]
    zeros = x[P['zeros']]
    assert float(xf[P['zeros']].max()) == 0 and torch.signbit(zeros[zeros.float() == 0]).tolist() == [True, False]


@case
def test_cpu_route_matches_the_reference(c):
    worst = D.check_case(c, *D.run_case(c, 'cpu'))
    if worst is not None:
        print('DYNAMIC_ACT_DEPOSIT_ULPS cpu %s %s H=%d bits=%d worst=%.3f'
              % (c['quantizer'], c['dtype'], c['shape'][1], c['bit_width'], worst))


@pytest.mark.parametrize('name', NAMES)
def test_shapes_state_and_modes(name):
    """scale and zero-point shapes for 1-D, 2-D and 3-D inputs; train and eval agree; nothing in the state dict"""
    import brevitas_amd.quant as Q
    q = getattr(Q, name)(**({'group_size': 16} if 'Group' in name else {}))
    assert name in Q.__all__
    # (the constants of BitWidthConst and ZeroZeroPoint are StatelessBuffers: they move with .to(), nothing is saved)
    assert len(q.state_dict()) == 0 and not list(q.parameters())
    assert all(b.numel() == 1 for b in q.buffers()) and len(list(q.buffers())) <= 2
    torch.manual_seed(3)
    for shape in ((64,), (5, 64), (2, 5, 64)):
        x = torch.randn(shape)
        q.train()
        y, scale, zp, bw = q(x)
        q.eval()
        y2, scale2, zp2, _ = q(x)
        assert torch.equal(y, y2) and torch.equal(scale, scale2) and torch.equal(zp, zp2)
        lead = tuple(shape[:-1])
        want = () if 'Tensor' in name else lead + ((1,) if 'Row' in name else (4, 1))
        assert tuple(y.shape) == shape and tuple(scale.shape) == want and float(bw) == 8.0
        assert tuple(zp.shape) == (want if 'Shifted' in name else ())
        assert scale.dtype == torch.float32
        # the definition: the same bits as the quantizer on the 2-D view
        yv, sv, zv, _ = q(x.reshape(-1, 64))
        assert torch.equal(yv.reshape(shape), y) and torch.equal(sv.reshape(want), scale)
    q4 = getattr(Q, name)(bit_width=4, **({'group_size': 16} if 'Group' in name else {}))
    y4 = q4(torch.randn(3, 64))[0]
    assert float(q4.msb_clamp_bit_width_impl()) == 4.0 and y4.unique().numel() <= 3 * 4 * 16


def test_bfloat16_scale_dtypes_follow_the_promotion_rule():
    """a dimensioned statistic keeps x's dtype, a 0-dim one promotes with the float32 threshold (_fused.scale_rule)"""
    import brevitas_amd.quant as Q
    x = torch.randn(4, 32).to(torch.bfloat16)
    assert Q.Int8DynamicActPerRowFloat()(x)[1].dtype == torch.bfloat16
    assert Q.ShiftedUint8DynamicActPerGroupFloat(group_size=16)(x)[2].dtype == torch.bfloat16
    assert Q.Int8DynamicActPerTensorFloat()(x)[1].dtype == torch.float32


def test_gradients_through_scale_and_zero_point_count():
    import brevitas_amd.quant as Q
    q = Q.ShiftedUint8DynamicActPerRowFloat()
    x = torch.randn(3, 40, requires_grad=True)
    _, scale, zp, _ = q(x)
    gs, = torch.autograd.grad(scale.sum(), x, retain_graph=True)
    assert int((gs != 0).sum()) == 6   # the maximum and the minimum of each row
    # the zero-point is rounded straight-through: its gradient reaches the minimum (and, through the scale, both)
    gz, = torch.autograd.grad(zp.sum(), x)
    assert 3 <= int((gz != 0).sum()) <= 6


def test_errors():
    import brevitas_amd.quant as Q
    from brevitas_amd.core.quant import DynamicActIntQuant
    with pytest.raises(ValueError, match=r'\(4, 40\).*32'):
        Q.Int8DynamicActPerGroupFloat(group_size=32)(torch.randn(4, 40))
    with pytest.raises(ValueError, match=r'\(4, 40\).*16'):
        Q.ShiftedUint8DynamicActPerGroupFloat(group_size=16)(torch.randn(4, 40))
    with pytest.raises(ValueError, match='group_size'):
        Q.Int8DynamicActPerGroupFloat(group_size=0)
    with pytest.raises(ValueError, match='no rows'):
        Q.Int8DynamicActPerRowFloat()(torch.tensor(1.0))
    q = Q.Int8DynamicActPerRowFloat()
    with pytest.raises(ValueError, match='granularity'):
        DynamicActIntQuant(q.int_quant, q.scaling_impl, q.int_scaling_impl, q.zero_point_impl,
                           q.msb_clamp_bit_width_impl, 'channel')


def test_bias_quantizer_refusal_names_both():
    import brevitas_amd.quant as Q
    from brevitas_amd.nn import QuantConv2d, QuantLinear
    for make in (Q.Int8DynamicActPerRowFloat, Q.ShiftedUint8DynamicActPerRowFloat,
                 functools.partial(Q.Int8DynamicActPerGroupFloat, group_size=16),
                 functools.partial(Q.ShiftedUint8DynamicActPerGroupFloat, group_size=16)):
        for bias_quant in (Q.Int8Bias, Q.Int32Bias):
            with pytest.raises(ValueError, match='dynamic input quantizer.*externally scaled bias quantizer'):
                QuantLinear(64, 8, weight_quant=Q.Int8WeightPerChannelFloat, input_quant=make(), bias_quant=bias_quant())
    with pytest.raises(ValueError, match='dynamic input quantizer'):
        QuantConv2d(4, 8, 3, weight_quant=Q.Int8WeightPerChannelFloat, input_quant=Q.Int8DynamicActPerRowFloat(),
                    bias_quant=Q.Int16Bias())
    # a per-tensor dynamic input scale is one scale: it works with them, and so does a bias with a scale of its own
    for make in (Q.Int8DynamicActPerTensorFloat, Q.ShiftedUint8DynamicActPerTensorFloat):
        lin = QuantLinear(64, 8, weight_quant=Q.Int8WeightPerChannelFloat, input_quant=make(), bias_quant=Q.Int16Bias())
        assert lin(torch.randn(3, 64)).shape == (3, 8)
    lin = QuantLinear(64, 8, weight_quant=Q.Int8WeightPerChannelFloat, input_quant=Q.Int8DynamicActPerRowFloat(),
                      bias_quant=Q.Int8BiasPerTensorFloatInternalScaling)
    assert lin(torch.randn(3, 64)).shape == (3, 8)


def test_layers_accept_the_quantizers_and_calibration_passes_the_tensor_through():
    import brevitas_amd.quant as Q
    from brevitas_amd.graph.calibrate import bias_correction_mode, calibration_mode
    from brevitas_amd.nn import QuantIdentity, QuantLinear, QuantReLU
    torch.manual_seed(5)
    x = torch.randn(2, 5, 64)
    relu = QuantReLU(Q.ShiftedUint8DynamicActPerRowFloat())
    assert not hasattr(relu.act_quant.tensor_quant, 'bvq_forward_pre')
    want = Q.ShiftedUint8DynamicActPerRowFloat()(torch.relu(x))[0]   # activation first, then the quantizer
    assert torch.equal(relu(x), want)
    ident = QuantIdentity(Q.Int8DynamicActPerGroupFloat(group_size=16))
    assert torch.equal(ident(x), Q.Int8DynamicActPerGroupFloat(group_size=16)(x)[0])
    model = torch.nn.Sequential(ident, relu, QuantLinear(64, 8, weight_quant=Q.Int8WeightPerChannelFloat,
                                                         input_quant=Q.Int8DynamicActPerRowFloat()))
    quantized = model(x)
    floating = torch.nn.functional.linear(torch.relu(x), model[2].weight, model[2].bias)
    assert not torch.equal(quantized, floating)
    with calibration_mode(model):
        assert model[2].input_quant.bvq_collect_only and ident.act_quant.bvq_collect_only
        passed = model[2].input_quant(x)
        assert passed[0] is x and passed[1] is None and passed[2] is None and float(passed[3]) == 8.0
        assert torch.equal(model(x), floating)
    assert torch.equal(model(x), quantized)
    with bias_correction_mode(model):   # its float pass switches the layer's input quantizer off as a whole
        model(x)
    assert bool(torch.isfinite(model(x)).all()) and not model[2].input_quant.bvq_collect_only


def test_quant_linear_forward_and_backward_equal_the_layer_assembled_by_hand():
    """QuantLinear with Int4WeightPerGroupFloat and ShiftedUint8DynamicActPerRowFloat on a [2, 5, 64] input against the
    composed pieces applied by hand: the statistics, the scale, the zero-point and IntQuant on x.reshape(10, 64)"""
    import brevitas_amd.quant as Q
    from brevitas_amd.nn import QuantLinear
    torch.manual_seed(11)
    lin = QuantLinear(64, 12, weight_quant=functools.partial(Q.Int4WeightPerGroupFloat, group_size=16),
                      input_quant=Q.ShiftedUint8DynamicActPerRowFloat())
    x = torch.randn(2, 5, 64, requires_grad=True)
    gout = torch.randn(2, 5, 12)
    out = lin(x)
    out.backward(gout)
    got = (out.detach().clone(), x.grad.clone(), lin.weight.grad.clone(), lin.bias.grad.clone())
    lin.zero_grad()

    q = lin.input_quant
    x2 = x.detach().clone().requires_grad_(True)
    xv = x2.reshape(10, 64)
    bw = q.msb_clamp_bit_width_impl()
    mx, mn = xv.max(dim=1).values, xv.min(dim=1).values
    threshold = torch.clamp_min(torch.abs(mx - mn), 1e-10).view(10, 1)
    assert torch.equal(threshold.detach(), q.scaling_impl(xv).detach())
    scale = threshold / q.int_scaling_impl(bw)
    offset = -torch.where(mn <= 0, mn, torch.zeros(())).view(10, 1)
    zp = q.int_quant.to_int(scale, q.int_quant.min_int(bw), bw, offset)
    xq = q.int_quant(scale, zp, bw, xv).reshape(2, 5, 64)
    wq = lin.weight_quant(lin.weight)[0]
    want = torch.nn.functional.linear(xq, wq, lin.bias)
    want.backward(gout)
    assert torch.equal(got[0], want.detach())
    assert torch.equal(got[1], x2.grad) and torch.equal(got[2], lin.weight.grad) and torch.equal(got[3], lin.bias.grad)
    y, s, z, _ = q(x.detach())
    assert tuple(s.shape) == (2, 5, 1) and tuple(z.shape) == (2, 5, 1)
    assert torch.equal(s.reshape(10, 1), scale.detach()) and torch.equal(z.reshape(10, 1), zp.detach())


def test_cabi_argument_checks_need_no_device():
    from brevitas_amd import _native as nat
    lib = nat.lib
    cap = nat.row_shifted_max_row_bytes()
    assert cap >= 32768 and cap % 16 == 0
    assert lib.bvq_row_shifted_fwd(None, None, 0.0, 0, 1.0, None, None, None, None, None) == -1
    assert 'descriptor' in nat.last_error()
    assert lib.bvq_row_shifted_bwd(None, None, None, None, None, None, 0.0, 0, 1.0, None, None) == -1
    assert lib.bvq_row_shifted_supported(None, None) == 0

    def desc(inner, dt=nat.BF16, ct=None, zdt=None, zp_pc=1, out_kind=nat.OUT_DEQUANT, pre_op=nat.PRE_NONE,
             round_mode=nat.ROUND, rows=12):
        return nat.QuantDesc(1, rows, inner, dt, dt if ct is None else ct, dt, dt if zdt is None else zdt, 1, zp_pc, 0.0,
                             255.0, round_mode, 0, 0, out_kind, pre_op)
    aligned = ctypes.c_void_p(4096)  # never dereferenced: every check below fails before any device work
    for d, word in ((desc(44), 'a row of 88 bytes'), (desc(cap // 2 + 8), 'a row of %d bytes' % (cap + 16)),
                    (desc(64, out_kind=nat.OUT_INT), 'integer output'), (desc(64, pre_op=nat.PRE_RELU), 'pre_op'),
                    (desc(64, ct=nat.F32), 'dtype'), (desc(64, zdt=nat.F32), 'zero-point dtype'),
                    (desc(64, zp_pc=0), 'zero-point per channel'), (desc(64, round_mode=nat.FLOOR), 'round_mode')):
        assert lib.bvq_row_shifted_supported(ctypes.byref(d), aligned) == 0
        rc = lib.bvq_row_shifted_fwd(ctypes.byref(d), aligned, 1e-10, 1, 255.0, aligned, aligned, aligned, aligned, None)
        assert rc == -2 and word in nat.last_error(), (rc, nat.last_error())
        rc = lib.bvq_row_shifted_bwd(ctypes.byref(d), aligned, aligned, aligned, None, None, 1e-10, 1, 255.0, aligned,
                                     None)
        assert rc == -2 and word in nat.last_error(), (rc, nat.last_error())
    for dt, size in ((nat.BF16, 2), (nat.F16, 2), (nat.F32, 4)):
        for row_bytes in (16, 48, 80, 1072, 2048, 2064, 8192, 8208, 22016, cap):
            for rows in (1, 7, 100000):
                assert lib.bvq_row_shifted_supported(ctypes.byref(desc(row_bytes // size, dt=dt, rows=rows)), aligned) == 1
    ok = desc(536)
    assert lib.bvq_row_shifted_supported(ctypes.byref(ok), ctypes.c_void_p(4098)) == 0   # off a 16-byte boundary
    rc = lib.bvq_row_shifted_fwd(ctypes.byref(ok), ctypes.c_void_p(4098), 1e-10, 1, 255.0, aligned, aligned, aligned,
                                 aligned, None)
    assert rc == -2 and '16-byte' in nat.last_error()
    assert lib.bvq_row_shifted_fwd(ctypes.byref(ok), None, 1e-10, 1, 255.0, aligned, aligned, aligned, aligned,
                                   None) == -1
    # the group-wise entries still hold their own bound to `inner`
    assert lib.bvq_group_shifted_supported(ctypes.byref(ok), aligned) == 0
    assert lib.bvq_group_shifted_supported(ctypes.byref(desc(64)), aligned) == 1
