"""GPFQ on the device: the column-loop kernel of one block (csrc/bvq_gpfq.hip) against the composed block step run on the
CPU -- full blocks, ragged blocks (partial lane masks, a layer narrower than a block), groups that began before the
block, planted dead columns, rounding ties and clamped rows --, the fused route of a whole layer against the composed
route on the device, K on and off the block grid, and gpfq_mode on small models.

Bars: Q and E of a block are bit-exact against the CPU (the kernel and the composed step compute the same definition
with the same roundings); the two routes of a whole layer are bit-identical on the device, their first product
and their tail updates being the same calls on the same bits."""
import functools

import pytest
import torch
import torch.nn.functional as F

from brevitas_amd import quant as Q
from brevitas_amd.graph import gpfq as P
from brevitas_amd.graph import gptq as G
from brevitas_amd.graph import gpfq_mode, gpfq_quantize_weight

from column_loop_cases import _same_bits, conv_models, linear_models

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
DT = {'f32': torch.float32, 'bf16': torch.bfloat16, 'f16': torch.float16}

# name -> (factory of the quantizer for a weight, group size or None: one group per row or per tensor)
QUANTS = {
    'sym4_g32': (lambda w: Q.Int4WeightPerGroupFloat(w, 32), 32),
    'asym4_g32': (lambda w: Q.ShiftedUint4WeightPerGroupFloat(w, 32), 32),
    'sym8_channel': (lambda w: Q.Int8WeightPerChannelFloat(w), None),
    'asym8_channel': (lambda w: Q.ShiftedUint8WeightPerChannelFloat(w), None),
    'sym8_tensor': (lambda w: Q.Int8WeightPerTensorFloat(w), None),
}
# group sizes that do not divide 128: (factory, k); the block is [128, k), its first group began 32 columns before it
STRADDLING = {
    'asym4_g96': (lambda w: Q.ShiftedUint4WeightPerGroupFloat(w, 96), 192),
    'sym4_g48': (lambda w: Q.Int4WeightPerGroupFloat(w, 48), 240),
}
COL0 = 128  # the block under test is the second one: its column offset and its group offset are not zero
# (block_cols, col0): neither lane mask full, the first full and the second not, and a layer narrower than a block
BLOCKS = [(128, COL0), (64, COL0), (1, COL0), (2, COL0), (63, COL0), (65, COL0), (127, COL0), (72, 0)]


@functools.lru_cache(maxsize=None)
def _statistics(k):
    """H and D [k, k] of a random calibration set with a drifted quantized path, on the CPU: computed once per size and
    left unchanged"""
    gen = torch.Generator().manual_seed(k)
    x = torch.randn(3 * k, k, generator=gen) @ (torch.eye(k) + 2 * torch.randn(k, k, generator=gen) / k ** 0.5)
    xq = x + 0.05 * torch.randn(3 * k, k, generator=gen)
    return (2.0 / x.shape[0]) * (xq.t() @ xq), (2.0 / x.shape[0]) * ((x - xq).t() @ xq)


def _run_block(make, dn, bc, col0, k, plant=None, rows=(5,)):
    """the block [col0, col0 + bc) of a weight [max(rows), k] with a running correction that earlier blocks have moved:
    the composed step on the CPU once, and the kernel on the device for the first r rows of it, r in rows -- rows are
    independent and the parameters are given, so the first r rows of the reference are the reference of a layer of r
    rows -> ((q, err) of the CPU, {r: (q, err) of the device}, the plan, scale, zp, w), the block's columns only.
    plant(w, c, h): changes to the weight (before the quantizer sees it), the correction and the Gram matrix"""
    from brevitas_amd import _native as nat
    dtype, top = DT[dn], max(rows)
    gen = torch.Generator().manual_seed(1000 * bc + col0)
    w0 = (0.05 * torch.randn(top, k, generator=gen)).to(dtype)
    h, d = (t.clone() for t in _statistics(k))
    c = P.initial_correction(w0.float(), d) + 0.003 * torch.randn(top, k, generator=gen)
    if plant is not None:
        plant(w0, c, h)
    w = torch.nn.Parameter(w0)
    plan = P._plan(make(w), k)
    scale, zp, _, _ = G._given_params(plan, w)
    wf = w.detach().float()
    q = torch.zeros(top, k, dtype=dtype)
    err = P.composed_block(plan, wf, c.clone(), h, col0, col0 + bc, q, scale.clone(), None if zp is None else zp.clone())
    cpu = (q[:, col0:col0 + bc], err)
    h_d, devs = h.to(DEV), {}
    for r in rows:
        wf_d, c_d, scale_d = wf[:r].to(DEV), c[:r].to(DEV), scale[:r].contiguous().to(DEV)
        zp_d = zp[:r].contiguous().to(DEV) if zp is not None else None
        q_d = torch.zeros(r, k, dtype=dtype, device=DEV)
        desc = P.fused_block_desc(plan, r, k, dtype)
        assert desc is not None
        assert nat.gpfq_block_supported(desc, wf_d, c_d, h_d, q_d, col0, bc)
        err_d = P.fused_block(desc, wf_d, c_d, h_d, col0, col0 + bc, q_d, scale_d, zp_d)
        torch.cuda.synchronize()
        # the weight, the correction and the parameters are read only; nothing outside the block is written
        assert torch.equal(wf_d.cpu(), wf[:r]) and torch.equal(c_d.cpu(), c[:r]) and torch.equal(h_d.cpu(), h)
        assert torch.equal(scale_d.cpu(), scale[:r]) and (zp is None or torch.equal(zp_d.cpu(), zp[:r]))
        assert not q_d[:, :col0].any() and not q_d[:, col0 + bc:].any()
        devs[r] = (q_d[:, col0:col0 + bc].cpu(), err_d.cpu())
    return cpu, devs, plan, scale, zp, w.detach()


def _assert_block(cpu, devs, what=''):
    for r, dev in devs.items():
        _same_bits(cpu[0][:r], dev[0], 'Q, %s %d rows' % (what, r))
        _same_bits(cpu[1][:r], dev[1], 'E, %s %d rows' % (what, r))


all_dtypes = pytest.mark.parametrize('dn', ['f32', 'bf16', 'f16'])
ROWS = (1, 5, 80)  # five rows: a second workgroup with one live wave


@all_dtypes
@pytest.mark.parametrize('name', sorted(QUANTS))
def test_block_kernel_is_the_composed_block_step(name, dn):
    """every block of BLOCKS at 1, 5 and 80 rows"""
    make, g = QUANTS[name]
    for bc, col0 in BLOCKS:
        # one group per row: the block ends the layer; groups of 32: the layer goes on behind the block, which may end
        # inside a group
        k = col0 + bc if g is None else (256 if col0 else 96)
        cpu, devs, _, _, _, _ = _run_block(make, dn, bc, col0, k, rows=ROWS)
        _assert_block(cpu, devs, 'block of %d columns at %d,' % (bc, col0))


@all_dtypes
@pytest.mark.parametrize('name', sorted(STRADDLING))
def test_block_kernel_group_that_began_before_the_block(name, dn):
    """a group size that does not divide 128: the block's first columns belong to a group that began in the block before,
    so the first change of parameters comes after 64 (g = 96) or 16 (g = 48) steps, not after g; 1, 5 and 80 rows"""
    make, k = STRADDLING[name]
    cpu, devs, _, _, _, _ = _run_block(make, dn, k - COL0, COL0, k, rows=ROWS)
    _assert_block(cpu, devs)


# ---- planted cases ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dn', ['f32', 'bf16'])
@pytest.mark.parametrize('name', ['sym8_channel', 'asym4_g32'])
def test_block_kernel_dead_column_inside_the_block(name, dn):
    """H[t, t] = 0 with its row and column: the column gets the round-to-nearest code of its own weight"""
    make, g = QUANTS[name]
    t = 37

    def plant(w, c, h):
        h[COL0 + t, :] = 0.0
        h[:, COL0 + t] = 0.0
    k = 256
    cpu, devs, plan, scale, zp, w = _run_block(make, dn, 128, COL0, k, plant)
    _assert_block(cpu, devs)
    dev = devs[5]
    # round-to-nearest of the column, by the quantizer's own IntQuant
    grp = (COL0 + t) // plan.group
    z = zp[:, grp:grp + 1] if zp is not None else plan.quant.zero_point_impl(w, scale, plan.bit_width)
    rtn = plan.quant.int_quant(scale[:, grp:grp + 1].contiguous(), z, plan.bit_width, w[:, COL0 + t:COL0 + t + 1])
    assert torch.equal(dev[0][:, t], rtn[:, 0])
    assert torch.equal(dev[1][:, t], w[:, COL0 + t].float() - rtn[:, 0].float())


@all_dtypes
def test_block_kernel_value_on_a_rounding_tie_goes_to_the_even_code(dn):
    """rows 0 and 1 have the scale 2^-8 (abs-max 127 / 256); at the block's first column H[t, t] = 2 and C = 2^-8, so
    v = w + 2^-9 sits on 2.5 and on 3.5 code units exactly: codes 2 and 4"""
    def plant(w, c, h):
        w[:2, 5] = 127.0 / 256.0
        w[0, COL0] = 2.0 / 256.0
        w[1, COL0] = 3.0 / 256.0
        c[:2, COL0] = 1.0 / 256.0
        h[COL0, COL0] = 2.0
    cpu, devs, _, scale, _, _ = _run_block(QUANTS['sym8_channel'][0], dn, 64, COL0, COL0 + 64, plant)
    _assert_block(cpu, devs)
    dev = devs[5]
    assert float(scale[0, 0]) == float(scale[1, 0]) == 2.0 ** -8
    assert float(dev[0][0, 0]) == 2.0 / 256.0 and float(dev[0][1, 0]) == 4.0 / 256.0


@pytest.mark.parametrize('dn', ['f32', 'bf16'])
@pytest.mark.parametrize('name', ['sym8_channel', 'asym8_channel', 'sym4_g32'])
def test_block_kernel_large_correction_clamps_at_both_ends(name, dn):
    """row 1 of C is large and positive, row 2 large and negative: v leaves the code range at either end"""
    make, g = QUANTS[name]

    def plant(w, c, h):
        c[1] = 1e3
        c[2] = -1e3
    k = COL0 + 128 if g is None else 256
    cpu, devs, plan, scale, zp, _ = _run_block(make, dn, 128, COL0, k, plant)
    _assert_block(cpu, devs)
    dev = devs[5]
    grp = COL0 // plan.group
    s = scale[:, grp:grp + 1].contiguous()
    z = zp[:, grp:grp + 1].contiguous() if zp is not None else plan.quant.zero_point_impl(s, s, plan.bit_width)
    big = torch.full((5, 1), 1e3, dtype=DT[dn])
    top = plan.quant.int_quant(s, z, plan.bit_width, big)[:, 0]
    bottom = plan.quant.int_quant(s, z, plan.bit_width, -big)[:, 0]
    assert float(dev[0][1, 0]) == float(top[1]) and float(dev[0][2, 0]) == float(bottom[2])
    assert float(top[1]) > float(bottom[1])


# ---- a whole layer ---------------------------------------------------------------------------------------------------

LAYERS = [('asym8_channel', k, rows) for k in (72, 200, 256, 384) for rows in (5, 80)]
LAYERS += [('sym8_tensor', 200, 80), ('sym4_g32', 256, 80), ('asym4_g32', 384, 5), ('asym4_g96', 384, 80),
           ('sym4_g48', 240, 5)]


@pytest.mark.parametrize('dn', ['f32', 'bf16'])
@pytest.mark.parametrize('name,k,rows', LAYERS, ids=['%s-k%d-r%d' % c for c in LAYERS])
def test_whole_layer_fused_route_is_the_composed_route(name, k, rows, dn, monkeypatch):
    """K on and off the block grid: one launch per block, the last one ragged, or the only block the whole layer"""
    import brevitas_amd.config as config
    from brevitas_amd import _native as nat
    make = STRADDLING[name][0] if name in STRADDLING else QUANTS[name][0]
    gen = torch.Generator().manual_seed(k + rows)
    w = torch.nn.Parameter((0.05 * torch.randn(rows, k, generator=gen)).to(DT[dn]).to(DEV))
    x = torch.randn(2 * k, k, generator=gen) @ (torch.eye(k) + 2 * torch.randn(k, k, generator=gen) / k ** 0.5)
    xq = x + 0.05 * torch.randn(2 * k, k, generator=gen)
    x[:, 7] = 0.0  # a dead input column
    xq[:, 7] = 0.0
    h = ((2.0 / x.shape[0]) * (xq.t() @ xq)).to(DEV)
    d = ((2.0 / x.shape[0]) * ((x - xq).t() @ xq)).to(DEV)
    quant = make(w).to(DEV)
    launches = []
    real = nat.gpfq_block
    monkeypatch.setattr(nat, 'gpfq_block', lambda *a, **kw: (launches.append(a[5]), real(*a, **kw))[1])
    fused = gpfq_quantize_weight(w, h, d, quant)
    assert launches == [min(128, k - c0) for c0 in range(0, k, 128)]  # one launch per block, the last one ragged
    monkeypatch.setattr(config, 'FUSED_PATHS', False)
    composed = gpfq_quantize_weight(w, h, d, quant)
    assert len(launches) == (k + 127) // 128
    _same_bits(composed.q.cpu(), fused.q.cpu(), 'Q')
    _same_bits(composed.scale.cpu(), fused.scale.cpu(), 'scale')
    _same_bits(composed.zero_point.cpu(), fused.zero_point.cpu(), 'zp')
    if name != 'sym8_tensor' or dn == 'f32':  # (a per-tensor scale of a 16-bit weight is rounded to its dtype)
        _, scale, zp, _ = quant(w)
        _same_bits(fused.scale.cpu(), scale.detach().cpu(), 'scale of the original weight')
        _same_bits(fused.zero_point.cpu(), zp.detach().cpu(), 'zp of the original weight')
        # the dead column is rounded to nearest
        assert torch.equal(fused.q[:, 7], quant(w)[0].detach()[:, 7])


# ---- gpfq_mode -------------------------------------------------------------------------------------------------------

def _output_errors(model, float_model, rtn, x):
    """(|gpfq model - float model|, |round-to-nearest model - float model|) on the calibration batch"""
    with torch.no_grad():
        want = float_model(x)
        return float((model(x) - want).norm()), float((rtn(x) - want).norm())


def test_gpfq_mode_on_a_linear_model():
    """(on the CPU, with the composed route and these seeds: output error 4.398 against round-to-nearest's 6.314)"""
    model, rtn, float_model, x = linear_models(DEV)
    with gpfq_mode(model) as gpfq:
        assert gpfq.num_layers == 2
        for _ in range(gpfq.num_layers):
            gpfq.model(x)
            gpfq.update()
    with torch.no_grad():
        for layer, inp in ((model[0], x), (model[2], model[1](model[0](x)))):
            assert torch.equal(layer(inp), F.linear(inp, layer.weight, layer.bias))
            assert layer.quant_weight()[1] is layer.frozen_weight_scale
    err_gpfq, err_rtn = _output_errors(model, float_model, rtn, x)
    print('linear model: output error gpfq %.5f, round-to-nearest %.5f' % (err_gpfq, err_rtn))
    assert err_gpfq < err_rtn


def test_gpfq_mode_on_a_conv_layer():
    """(on the CPU, with the composed route and these seeds: output error 3.888 against round-to-nearest's 4.691)"""
    model, rtn, float_model, x = conv_models(DEV)
    with gpfq_mode(model) as gpfq:
        gpfq.model(x)
        res = gpfq.update()
    assert res.q.shape == model[0].weight.shape and res.scale.shape == (16, 9, 1)
    with torch.no_grad():
        assert torch.equal(model(x), F.conv2d(x, model[0].weight, model[0].bias, padding=1))
        assert model[0].quant_weight()[1] is model[0].frozen_weight_scale
    err_gpfq, err_rtn = _output_errors(model, float_model, rtn, x)
    print('conv layer: output error gpfq %.5f, round-to-nearest %.5f' % (err_gpfq, err_rtn))
    assert err_gpfq < err_rtn
