"""GPTQ on the device: the column-loop kernel of one block (csrc/bvq_gptq.hip) against the composed block step run on the
CPU -- full blocks, ragged blocks (partial lane masks, a layer narrower than a block) and given groups that began before
the block --, the fused route of a whole layer against the composed route on the device, K on and off the block grid,
and gptq_mode on small models.

Bars: Q, E, scale and zp of a block are bit-exact against the CPU (the kernel and the composed step compute the same
definition with the same roundings); the two routes of a whole layer are bit-identical on the device, their
tail updates being the same calls on the same bits."""
import functools

import pytest
import torch
import torch.nn.functional as F

from brevitas_amd import quant as Q
from brevitas_amd.graph import gptq as G
from brevitas_amd.graph import gptq_mode, gptq_quantize_weight

from column_loop_cases import _same_bits, conv_models, linear_models

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
DT = {'f32': torch.float32, 'bf16': torch.bfloat16, 'f16': torch.float16}

# name -> (factory of the quantizer for a weight, group size or None: one group per row, given)
QUANTS = {
    'sym3_g16': (lambda w: Q.Int8WeightPerGroupFloat(w, 16, bit_width=3), 16),
    'sym4_g32': (lambda w: Q.Int4WeightPerGroupFloat(w, 32), 32),
    'sym8_g64': (lambda w: Q.Int8WeightPerGroupFloat(w, 64), 64),
    'sym4_g128': (lambda w: Q.Int4WeightPerGroupFloat(w, 128), 128),
    'asym4_g16': (lambda w: Q.ShiftedUint4WeightPerGroupFloat(w, 16), 16),
    'asym4_g32': (lambda w: Q.ShiftedUint4WeightPerGroupFloat(w, 32), 32),
    'asym8_g32': (lambda w: Q.ShiftedUint8WeightPerGroupFloat(w, 32), 32),
    'asym4_g64': (lambda w: Q.ShiftedUint4WeightPerGroupFloat(w, 64), 64),
    'asym8_g128': (lambda w: Q.ShiftedUint8WeightPerGroupFloat(w, 128), 128),
    'sym8_channel_given': (lambda w: Q.Int8WeightPerChannelFloat(w), None),
    'sym4_channel_given': (lambda w: Q.Int4WeightPerChannelFloat(w), None),
    'asym8_channel_given': (lambda w: Q.ShiftedUint8WeightPerChannelFloat(w), None),
}
COL0 = 128  # the block under test is the second one: its column offset and its group offset are not zero


def _block_cases():
    for name, (_, g) in sorted(QUANTS.items()):
        for bc in (128, 64):
            if g is not None and bc % g:
                continue  # a group never straddles a block: block_cols is a multiple of the group size
            for rows in (1, 80):
                yield name, bc, rows


@functools.lru_cache(maxsize=None)
def _factor(k):
    """U [k, k] of a random calibration set, on the CPU: computed once per size and left unchanged"""
    gen = torch.Generator().manual_seed(k)
    x = torch.randn(3 * k, k, generator=gen) @ (torch.eye(k) + 2 * torch.randn(k, k, generator=gen) / k ** 0.5)
    return G.prepare_hessian((2.0 / x.shape[0]) * (x.t() @ x), torch.zeros(1, k), 0.01)


def _run_block(name, dn, rows, bc, plant=None, col0=COL0, static=False, make=None):
    """the block [col0, col0 + bc) of a random working copy [rows, col0 + bc] on the CPU (composed) and on the device
    (kernel) -> ((q, err, scale, zp) of the CPU, the same of the device), the block's columns and the entries of the
    groups that reach into it only.  static: a group-wise quantizer's scales and zero-points are given (static_groups);
    make: a quantizer factory in place of QUANTS[name], whose group size need not divide the block"""
    make = make or QUANTS[name][0]
    dtype = DT[dn]
    k = col0 + bc
    gen = torch.Generator().manual_seed(1000 * rows + bc)
    w = torch.nn.Parameter((0.05 * torch.randn(rows, k, generator=gen)).to(dtype))
    quant = make(w)
    plan = G._plan(quant, k, static)
    groups = k // plan.group
    wf = w.detach().float() + 0.003 * torch.randn(rows, k, generator=gen)  # a working copy already moved off the grid of T
    if plant is not None:
        plant(wf[:, col0:])
    u = _factor(k)
    if plan.computed:
        scale = torch.zeros(rows, groups, dtype=dtype)
        zp = torch.zeros(rows, groups, dtype=dtype) if plan.shifted else None
    else:
        scale, zp, _, _ = G._given_params(plan, w)
    out = []
    for dev in ('cpu', DEV):
        wf_d, u_d, scale_d = wf.clone().to(dev), u.to(dev), scale.clone().to(dev)
        zp_d = zp.clone().to(dev) if zp is not None else None
        q_d = torch.zeros(rows, k, dtype=dtype, device=dev)
        if dev == 'cpu':
            err = G.composed_block(plan, wf_d, u_d, col0, k, q_d, scale_d, zp_d)
        else:
            fa = G.fused_block_args(plan, rows, k, dtype)
            assert fa is not None
            from brevitas_amd import _native as nat
            assert nat.gptq_block_supported(fa.desc, wf_d, u_d, q_d, col0, bc, plan.computed)
            keep = wf_d.clone()
            err = G.fused_block(fa, plan, wf_d, u_d, col0, k, q_d, scale_d, zp_d)
            torch.cuda.synchronize()
            assert torch.equal(wf_d, keep)                      # the working copy is read only
            assert not q_d[:, :col0].any()                      # nothing outside the block is written
            if plan.computed:
                assert not scale_d[:, :col0 // plan.group].any()
            else:                                               # given: read only
                assert torch.equal(scale_d.cpu(), scale) and (zp is None or torch.equal(zp_d.cpu(), zp))
        g0 = col0 // plan.group
        out.append((q_d[:, col0:].cpu(), err.cpu(), scale_d[:, g0:].cpu(), zp_d[:, g0:].cpu() if zp is not None else None))
    return out


@pytest.mark.parametrize('dn', ['f32', 'bf16', 'f16'])
@pytest.mark.parametrize('name,bc,rows', list(_block_cases()),
                         ids=['%s-bc%d-r%d' % c for c in _block_cases()])
def test_block_kernel_is_the_composed_block_step(name, bc, rows, dn):
    cpu, dev = _run_block(name, dn, rows, bc)
    for a, b, what in zip(cpu, dev, ('Q', 'E', 'scale', 'zp')):
        _same_bits(a, b, what)


@pytest.mark.parametrize('dn', ['f32', 'bf16', 'f16'])
@pytest.mark.parametrize('name', ['sym4_g32', 'asym4_g32'])
def test_block_kernel_constant_group_and_rounding_tie(name, dn):
    """the first group of the block is all equal in row 0; in row 1 it spans exactly the code range with scale 1 and its
    first element sits on a rounding tie, which goes to the even code"""
    sym = name.startswith('sym')

    def plant(block):
        block[0, :32] = 0.25
        block[1, :32] = 1.0
        block[1, 0] = 2.5                       # 2.5 / 1 -> 2 (half to even)
        block[1, 1] = 7.0 if sym else 15.0      # abs-max 7 / 7, or max - min = 15 / 15: scale 1
        if not sym:
            block[1, 2] = 0.0                   # minimum 0: zero-point 0
    cpu, dev = _run_block(name, dn, 4, 64, plant)
    for a, b, what in zip(cpu, dev, ('Q', 'E', 'scale', 'zp')):
        _same_bits(a, b, what)
    q, _, scale, _ = dev
    assert float(scale[1, 0]) == 1.0 and float(q[1, 0]) == 2.0


# ---- ragged blocks: partial lane masks, a block that is the whole layer, groups that began before the block -----------

# five rows: a second workgroup with one live wave
ragged = pytest.mark.parametrize('rows', [1, 5])
all_dtypes = pytest.mark.parametrize('dn', ['f32', 'bf16', 'f16'])
# given group-wise parameters whose group size does not divide 128: (factory, k); the block is [128, k)
STRADDLING = {
    'asym4_g96': (lambda w: Q.ShiftedUint4WeightPerGroupFloat(w, 96), 192),   # group 1 = [96, 192) began 32 columns ago
    'sym4_g48': (lambda w: Q.Int4WeightPerGroupFloat(w, 48), 240),            # group 2 = [96, 144) began 32 columns ago
}


def _assert_block(cpu, dev):
    for a, b, what in zip(cpu, dev, ('Q', 'E', 'scale', 'zp')):
        _same_bits(a, b, what)


@all_dtypes
@ragged
@pytest.mark.parametrize('bc,col0', [(1, COL0), (2, COL0), (63, COL0), (65, COL0), (72, COL0), (127, COL0), (72, 0)],
                         ids=lambda v: str(v))
@pytest.mark.parametrize('name', ['sym8_channel_given', 'asym8_channel_given'])
def test_block_kernel_given_parameters_on_a_ragged_block(name, bc, col0, rows, dn):
    """one group per row, given: a block of 1, 2, 63, 65, 72 or 127 columns behind column 128 (neither lane mask is full,
    or the first is and the second is not), and a layer of 72 columns that is narrower than a block"""
    _assert_block(*_run_block(name, dn, rows, bc, col0=col0))


@all_dtypes
@ragged
@pytest.mark.parametrize('name,bc', [('sym3_g16', 16), ('sym3_g16', 48), ('sym3_g16', 112), ('asym4_g16', 16),
                                     ('asym4_g16', 48), ('asym4_g16', 112), ('sym4_g32', 32), ('sym4_g32', 96),
                                     ('asym4_g32', 32), ('asym4_g32', 96)])
def test_block_kernel_computed_parameters_on_a_short_block(name, bc, rows, dn):
    """scale and zero-point computed in the loop, the block a whole number of groups but shorter than 128 columns: the
    segments of the butterflies lie beside lanes that hold no column"""
    _assert_block(*_run_block(name, dn, rows, bc))


@all_dtypes
@ragged
@pytest.mark.parametrize('name', sorted(STRADDLING))
def test_block_kernel_given_group_that_began_before_the_block(name, rows, dn):
    """static_groups with a group size that does not divide 128: the block's first columns belong to a group that began
    in the block before, so the first change of parameters comes after 64 (g = 96) or 16 (g = 48) steps, not after g"""
    make, k = STRADDLING[name]
    _assert_block(*_run_block(name, dn, rows, k - COL0, static=True, make=make))


LAYERS = [(name, k, False, 80) for name, k in (
    ('sym8_channel_given', 72), ('asym8_channel_given', 72), ('sym8_channel_given', 200), ('asym8_channel_given', 200),
    ('sym3_g16', 144), ('asym4_g16', 144), ('sym4_g32', 320), ('asym4_g32', 320))]
LAYERS += [(name, STRADDLING[name][1], True, 80) for name in sorted(STRADDLING)]
LAYERS += [('asym8_channel_given', 200, False, 5)]


@pytest.mark.parametrize('dn', ['f32', 'bf16'])
@pytest.mark.parametrize('name,k,static,rows', LAYERS, ids=['%s-k%d-static%d-r%d' % c for c in LAYERS])
def test_whole_layer_off_the_block_grid_fused_route_is_the_composed_route(name, k, static, rows, dn, monkeypatch):
    """K no multiple of 128: the last block is ragged, or the only block is the whole layer; gptq_quantize_weight asks
    gptq_block_supported about block 0 alone"""
    import brevitas_amd.config as config
    from brevitas_amd import _native as nat
    make = STRADDLING[name][0] if name in STRADDLING else QUANTS[name][0]
    gen = torch.Generator().manual_seed(k + rows)
    w = torch.nn.Parameter((0.05 * torch.randn(rows, k, generator=gen)).to(DT[dn]).to(DEV))
    x = torch.randn(2 * k, k, generator=gen) @ (torch.eye(k) + 2 * torch.randn(k, k, generator=gen) / k ** 0.5)
    x[:, 7] = 0.0  # a dead input column
    h = ((2.0 / x.shape[0]) * (x.t() @ x)).to(DEV)
    quant = make(w).to(DEV)
    launches = []
    real = nat.gptq_block
    monkeypatch.setattr(nat, 'gptq_block', lambda *a, **kw: (launches.append(a[4]), real(*a, **kw))[1])
    fused = gptq_quantize_weight(w, h, quant, static_groups=static)
    assert launches == [min(128, k - c0) for c0 in range(0, k, 128)]  # one launch per block, the last one ragged
    monkeypatch.setattr(config, 'FUSED_PATHS', False)
    composed = gptq_quantize_weight(w, h, quant, static_groups=static)
    assert len(launches) == (k + 127) // 128
    _same_bits(composed.q.cpu(), fused.q.cpu(), 'Q')
    _same_bits(composed.scale.cpu(), fused.scale.cpu(), 'scale')
    _same_bits(composed.zero_point.cpu(), fused.zero_point.cpu(), 'zp')
    assert not fused.q[:, 7].any()


@pytest.mark.parametrize('dn', ['f32', 'bf16'])
@pytest.mark.parametrize('k', [256, 384])
@pytest.mark.parametrize('name', ['sym4_g32', 'asym4_g64', 'sym8_channel_given', 'asym8_g128'])
def test_whole_layer_fused_route_is_the_composed_route(name, k, dn, monkeypatch):
    import brevitas_amd.config as config
    from brevitas_amd import _native as nat
    make, _ = QUANTS[name]
    rows = 80
    gen = torch.Generator().manual_seed(k)
    w = torch.nn.Parameter((0.05 * torch.randn(rows, k, generator=gen)).to(DT[dn]).to(DEV))
    x = torch.randn(2 * k, k, generator=gen) @ (torch.eye(k) + 2 * torch.randn(k, k, generator=gen) / k ** 0.5)
    x[:, 7] = 0.0  # a dead input column
    h = ((2.0 / x.shape[0]) * (x.t() @ x)).to(DEV)
    quant = make(w).to(DEV)
    launches = []
    real = nat.gptq_block
    monkeypatch.setattr(nat, 'gptq_block', lambda *a, **kw: (launches.append(1), real(*a, **kw))[1])
    fused = gptq_quantize_weight(w, h, quant)
    assert len(launches) == (k + 127) // 128  # one launch per block
    monkeypatch.setattr(config, 'FUSED_PATHS', False)
    composed = gptq_quantize_weight(w, h, quant)
    assert len(launches) == (k + 127) // 128
    _same_bits(composed.q.cpu(), fused.q.cpu(), 'Q')
    _same_bits(composed.scale.cpu(), fused.scale.cpu(), 'scale')
    _same_bits(composed.zero_point.cpu(), fused.zero_point.cpu(), 'zp')
    assert not fused.q[:, 7].any()


def test_whole_layer_static_groups_fused_route_is_the_composed_route(monkeypatch):
    """static_groups: the group-wise scales and zero-points are given, computed once from the original weight"""
    import brevitas_amd.config as config
    k, rows = 384, 80
    gen = torch.Generator().manual_seed(21)
    w = torch.nn.Parameter((0.05 * torch.randn(rows, k, generator=gen)).to(torch.bfloat16).to(DEV))
    x = torch.randn(2 * k, k, generator=gen) @ (torch.eye(k) + 2 * torch.randn(k, k, generator=gen) / k ** 0.5)
    h = ((2.0 / x.shape[0]) * (x.t() @ x)).to(DEV)
    quant = Q.ShiftedUint4WeightPerGroupFloat(w, 64).to(DEV)
    fused = gptq_quantize_weight(w, h, quant, static_groups=True)
    _, scale, zp, _ = quant(w)
    _same_bits(fused.scale.cpu(), scale.detach().cpu(), 'scale')
    _same_bits(fused.zero_point.cpu(), zp.detach().cpu(), 'zp')
    monkeypatch.setattr(config, 'FUSED_PATHS', False)
    composed = gptq_quantize_weight(w, h, quant, static_groups=True)
    _same_bits(composed.q.cpu(), fused.q.cpu(), 'Q')


def _output_errors(model, float_model, make_rtn, x):
    """(|gptq model - float model|, |round-to-nearest model - float model|) on the calibration batch"""
    rtn = make_rtn()
    with torch.no_grad():
        want = float_model(x)
        return float((model(x) - want).norm()), float((rtn(x) - want).norm())


def test_gptq_mode_on_a_linear_model():
    model, rtn, float_model, x = linear_models(DEV)
    with gptq_mode(model) as gptq:
        assert gptq.num_layers == 2
        for _ in range(gptq.num_layers):
            gptq.model(x)
            gptq.update()
    with torch.no_grad():
        for layer, inp in ((model[0], x), (model[2], model[1](model[0](x)))):
            assert torch.equal(layer(inp), F.linear(inp, layer.weight, layer.bias))
            assert layer.quant_weight()[1] is layer.frozen_weight_scale
    err_gptq, err_rtn = _output_errors(model, float_model, lambda: rtn, x)
    print('linear model: output error gptq %.5f, round-to-nearest %.5f' % (err_gptq, err_rtn))
    assert err_gptq < err_rtn


def test_gptq_mode_on_a_conv_layer():
    model, rtn, float_model, x = conv_models(DEV)
    with gptq_mode(model) as gptq:
        gptq.model(x)
        res = gptq.update()
    assert res.q.shape == model[0].weight.shape and res.scale.shape == (16, 9, 1)
    with torch.no_grad():
        assert torch.equal(model(x), F.conv2d(x, model[0].weight, model[0].bias, padding=1))
    err_gptq, err_rtn = _output_errors(model, float_model, lambda: rtn, x)
    print('conv layer: output error gptq %.5f, round-to-nearest %.5f' % (err_gptq, err_rtn))
    assert err_gptq < err_rtn
