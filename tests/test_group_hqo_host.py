"""Group-wise HQO zero-point (ShiftedUint4/8WeightPerGroupFloatHQO, core/quant/int.py: GroupwiseHQOIntQuant) on the
composed route, no GPU: a group worked by hand, the fixed order of the sums, the properties of the search (the kept
error never exceeds candidate 0's, the iterations help on weights with outliers, zero iterations are the plain asymmetric
quantizer, special groups keep candidate 0), the module surface, the record of the per-unit family against a recording
stand-in library, the argument checks of the C ABI entries and the autograd of the composed route.

DESIGN.md §9, "Group-wise HQO zero-point", is the definition; _aten.group_hqo_search composes it from torch ops and
tests/test_gpu_group_hqo.py holds the kernels to its bits.
"""
import ctypes
import functools

import pytest
import torch

from test_group_mse_host import same_bits
from test_unit_families_host import DT as REC_DT, MIN_VAL, STREAM, _desc, _x, nat  # noqa: F401  (nat: a fixture)

DT = {'f32': torch.float32, 'bf16': torch.bfloat16, 'f16': torch.float16}
dtypes = pytest.mark.parametrize('dn', ['f32', 'bf16', 'f16'])


def outlier_weight(g, dn, seed=0):
    """randn(64, 4 g) * 0.05 with every 37th column times 6"""
    gen = torch.Generator().manual_seed(seed)
    w = torch.randn(64, 4 * g, generator=gen) * 0.05
    w[:, ::37] *= 6
    return w.to(DT[dn])


def quantizer(w, g, bits, **kw):
    import brevitas_amd.quant as Q
    return Q.ShiftedUint8WeightPerGroupFloatHQO(w, group_size=g, bit_width=bits, **kw)


def plain(w, g, bits):
    import brevitas_amd.quant as Q
    return Q.ShiftedUint8WeightPerGroupFloat(w, group_size=g, bit_width=bits)


def search(q, w):
    """the composed search of the module on w -> (zero_point [groups, 1], idx [groups], kept error, candidate 0's)"""
    bw = q.msb_clamp_bit_width_impl()
    with torch.no_grad():
        xg, scale = q._hqo_operands(w, bw)
        return q._hqo_search(xg, scale, bw)


# ---- a group by hand ------------------------------------------------------------------------------------------------

def test_hand_worked_group():
    """g = 16, float32, 2 bits (codes 0 .. 3), p = 1, beta = 4, kappa = 2: inv_beta = [0.25, 0.125, 0.0625].
    x = [0, 3, 1.5, 0.75 x 13]: mx = 3, mn = 0, s = 3 / 3 = 1, zp_0 = 0.  Every value below is dyadic, so no sum rounds.

      i = 0, zp = 0:        q = [0, 3, 2, 1 x 13] (1.5 rounds half to even), y = q, r = [0, 0, -0.5, -0.25 x 13]
                            e_0 = 0.5 + 13 * 0.25 = 3.75
          thr = 0.25:       w_e = [0, 0, -0.25, -0 x 13];  q - (x - w_e) = [0, 0, 2 - 1.75, (1 - 0.75) x 13] = 0.25 x 14
                            z_1 = 3.5 / 16 = 0.21875
      i = 1, zp = 0.21875:  x + zp = [0.21875, 3.21875, 1.71875, 0.96875 x 13], q as before,
                            y = q - zp = [-0.21875, 2.78125, 1.78125, 0.78125 x 13], r = [0.21875, 0.21875, -0.28125, -0.03125 x 13]
                            e_1 = 0.4375 + 0.28125 + 0.40625 = 1.125 < 3.75: kept
          thr = 0.125:      w_e = [0.09375, 0.09375, -0.15625, -0 x 13]
                            q - (x - w_e) = [0.09375, 0.09375, 2 - 1.65625 = 0.34375, 0.25 x 13], sum 3.78125
                            z_2 = 3.78125 / 16 = 0.236328125
      i = 2, zp = 0.236328125: q as before, r = [0.236328125, 0.236328125, -0.263671875, -0.013671875 x 13]
                            e_2 = 0.47265625 + 0.263671875 + 0.177734375 = 0.9140625 < 1.125: kept

    so with two iterations k = 2, zero_point = 0.236328125, and with one k = 1, zero_point = 0.21875."""
    x = torch.tensor([[0.0, 3.0, 1.5] + [0.75] * 13])
    q_codes = torch.tensor([[0.0, 3.0, 2.0] + [1.0] * 13])
    for iters, k, zp_want, e_want in ((2, 2, 0.236328125, 0.9140625), (1, 1, 0.21875, 1.125), (0, 0, 0.0, 3.75)):
        w = torch.nn.Parameter(x.clone())
        q = quantizer(w, 16, 2, hqo_iters=iters, hqo_beta=4.0, hqo_kappa=2.0, hqo_lp_norm=1.0)
        assert list(q._hqo_table()) == [0.25, 0.125, 0.0625][:iters + 1]
        zp, idx, e, e0 = search(q, w)
        assert idx.tolist() == [k] and zp.tolist() == [[zp_want]] and e.tolist() == [e_want] and e0.tolist() == [3.75]
        y, scale, zero_point, bw = q(w)
        assert scale.tolist() == [[[1.0]]] and zero_point.tolist() == [[[zp_want]]] and float(bw) == 2.0
        assert torch.equal(y, q_codes - zp_want) and q.last_hqo_index.tolist() == [[k]]


# ---- the order of the sums ------------------------------------------------------------------------------------------

def halving_sum(v, chunk):
    """tree_sum spelled element by element, in Python floats rounded to float32 after every add"""
    f32 = lambda a: torch.tensor(a, dtype=torch.float64).float().item()  # noqa: E731
    out = []
    for row in v.tolist():
        t = []
        for c in range(0, len(row), chunk):
            even, odd = row[c], row[c + 1]
            for k in range(2, chunk, 2):
                even, odd = f32(even + row[c + k]), f32(odd + row[c + k + 1])
            t.append(f32(even + odd))
        while len(t) > 1:
            h = len(t) // 2
            t = [f32(t[j] + t[j + h]) for j in range(h)]
        out.append(t[0])
    return torch.tensor(out, dtype=torch.float32)


@pytest.mark.parametrize('g,chunk', [(16, 4), (16, 8), (64, 8), (256, 4)])
def test_tree_sum_is_the_halving_order(g, chunk):
    from brevitas_amd import _aten
    gen = torch.Generator().manual_seed(g + chunk)
    v = torch.randn(24, g, generator=gen) * torch.logspace(-3, 3, g)
    got = _aten.tree_sum(v, chunk)
    assert same_bits(got, halving_sum(v, chunk))
    assert not same_bits(got, v.sum(dim=1))           # the input tells the orders apart
    assert not same_bits(got, _aten.tree_sum(v.roll(1, dims=1), chunk))
    with pytest.raises(ValueError, match='power of two'):
        _aten.tree_sum(torch.zeros(2, 48), 8)


# ---- properties of the search ---------------------------------------------------------------------------------------

@dtypes
@pytest.mark.parametrize('bits', [2, 4, 8])
@pytest.mark.parametrize('p', [1.0, 0.5, 0.7])
def test_kept_error_never_exceeds_candidate_zero(dn, bits, p):
    g = 32
    w = torch.nn.Parameter(outlier_weight(g, dn))
    q = quantizer(w, g, bits, hqo_lp_norm=p)
    zp, idx, e, e0 = search(q, w)
    assert bool((e <= e0).all()) and bool(((idx == 0) == (e == e0)).all())
    # the kept error is the error of the forward at the kept zero-point, summed in the same order
    from brevitas_amd import _aten
    y, scale, zero_point, _ = q(w)
    assert same_bits(zero_point.reshape(-1, 1), zp) and torch.equal(q.last_hqo_index.reshape(-1), idx)
    r = (w.detach().float() - y.detach().float()).reshape(-1, g)
    assert same_bits(_aten.tree_sum(r.abs(), 16 // w.element_size()), e)


@dtypes
def test_iterations_help_on_weights_with_outliers(dn):
    """The seeded outlier weight at 4 bits, g = 64, p = 0.5, 20 iterations.  The composed route reaches: float32 0.809 of
    the groups lowered, total error 0.9500 of candidate 0's, mean kept index 2.71; bfloat16 0.512, 0.9603, 1.41; float16
    0.777, 0.9518, 2.72."""
    g = 64
    w = torch.nn.Parameter(outlier_weight(g, dn))
    q = quantizer(w, g, 4)
    zp, idx, e, e0 = search(q, w)
    print('GROUP_HQO %s lowered %.3f total %.4f mean k %.2f' % (dn, float((e < e0).float().mean()),
                                                                 float(e.sum() / e0.sum()), float(idx.float().mean())))
    assert float(e.sum()) < float(e0.sum()) and int(idx.max()) > 0
    assert int(idx.max()) <= 20 and bool((zp.float() != zp.float().round()).any())


@dtypes
@pytest.mark.parametrize('bits', [4, 8])
def test_zero_iterations_are_the_plain_asymmetric_quantizer(dn, bits):
    g = 32
    w0 = outlier_weight(g, dn)
    w0.view(-1, g)[3] = 0.0
    w0.view(-1, g)[4] = 0.015625
    w = torch.nn.Parameter(w0)
    q = quantizer(w, g, bits, hqo_iters=0)
    got, want = q(w), plain(w, g, bits)(w)
    for a, b, name in zip(got[:3], want[:3], ('y', 'scale', 'zero_point')):
        assert same_bits(a, b), name
    assert not bool(q.last_hqo_index.any())


@dtypes
def test_special_groups_keep_candidate_zero(dn):
    g, bits = 32, 4
    w0 = outlier_weight(g, dn)
    w2 = w0.view(-1, g)
    w2[0] = 0.0
    w2[1] = 0.015625
    w2[2, 3] = float('nan')
    w2[3, 5] = float('inf')
    w2[4, 7] = -float('inf')
    w2[5] = -0.25
    w = torch.nn.Parameter(w0)
    q = quantizer(w, g, bits)
    y, scale, zp, _ = q(w)
    y_p, scale_p, zp_p, _ = plain(w, g, bits)(w)
    special = [0, 1, 2, 3, 4, 5]
    assert q.last_hqo_index.reshape(-1)[special].tolist() == [0] * 6
    assert int(q.last_hqo_index.max()) > 0
    for a, b, name in ((y.reshape(-1, g), y_p.reshape(-1, g), 'y'), (scale.reshape(-1), scale_p.reshape(-1), 'scale'),
                       (zp.reshape(-1), zp_p.reshape(-1), 'zero_point')):
        assert same_bits(a[special], b[special]), name
    # and every other group is untouched by its neighbours
    w1 = torch.nn.Parameter(outlier_weight(g, dn))
    y1, _, _, _ = quantizer(w1, g, bits)(w1)
    assert same_bits(y.reshape(-1, g)[6:], y1.reshape(-1, g)[6:])


# ---- the module surface ---------------------------------------------------------------------------------------------

def test_constructor_refusals():
    import brevitas_amd.quant as Q
    from brevitas_amd.core.quant import GroupwiseHQOIntQuant, GroupwiseRescalingIntQuant
    w = torch.nn.Parameter(torch.randn(8, 64))
    ok = Q.ShiftedUint4WeightPerGroupFloatHQO(w, group_size=32)
    assert isinstance(ok, GroupwiseHQOIntQuant) and isinstance(ok, GroupwiseRescalingIntQuant)
    assert (ok.hqo_iters, ok.hqo_beta, ok.hqo_kappa, ok.hqo_lp_norm) == (20, 10.0, 1.01, 0.5)
    assert float(ok.msb_clamp_bit_width_impl()) == 4.0 and ok.group_size == 32 and ok.last_hqo_index is None
    assert 'ShiftedUint8WeightPerGroupFloatHQO' in Q.__all__ and 'ShiftedUint4WeightPerGroupFloatHQO' in Q.__all__
    for kw in ({'hqo_iters': -1}, {'hqo_iters': 64}, {'hqo_iters': 2.5}, {'hqo_beta': 0.0}, {'hqo_beta': float('inf')},
               {'hqo_kappa': -1.0}, {'hqo_kappa': float('nan')}, {'hqo_lp_norm': 0.0}, {'hqo_lp_norm': 1.5},
               {'hqo_lp_norm': float('nan')}, {'hqo_kappa': 1e30, 'hqo_iters': 10}):
        with pytest.raises(ValueError, match='hqo_'):
            Q.ShiftedUint4WeightPerGroupFloatHQO(w, group_size=32, **kw)
    assert Q.ShiftedUint4WeightPerGroupFloatHQO(w, group_size=32, hqo_iters=63, hqo_lp_norm=1.0).hqo_iters == 63
    with pytest.raises(ValueError, match='group_size 8'):
        Q.ShiftedUint4WeightPerGroupFloatHQO(w, group_size=8)
    # the graph must be the asymmetric one, without a quantization delay
    sym = Q.Int8WeightPerGroupFloat(w, group_size=32)
    with pytest.raises(TypeError, match='asymmetric'):
        GroupwiseHQOIntQuant(sym.int_quant, sym.scaling_impl, sym.int_scaling_impl, sym.zero_point_impl,
                             sym.msb_clamp_bit_width_impl, 32)
    asym = Q.ShiftedUint8WeightPerGroupFloat(w, group_size=32)
    from brevitas_amd.core.quant.delay import DelayWrapper
    asym.int_quant.delay_wrapper = DelayWrapper(5)
    with pytest.raises(ValueError, match='quant_delay_steps'):
        GroupwiseHQOIntQuant(asym.int_quant, asym.scaling_impl, asym.int_scaling_impl, asym.zero_point_impl,
                             asym.msb_clamp_bit_width_impl, 32)
    with pytest.raises(ValueError, match=r'\(8, 40\).*32'):
        ok(torch.randn(8, 40))


def test_state_dict_keys_are_the_parents():
    import brevitas_amd.quant as Q
    w = torch.nn.Parameter(torch.randn(8, 64))
    q, parent = Q.ShiftedUint8WeightPerGroupFloatHQO(w, group_size=32), Q.ShiftedUint8WeightPerGroupFloat(w, group_size=32)
    q(w)
    assert sorted(q.state_dict().keys()) == sorted(parent.state_dict().keys())
    assert [n for n, _ in q.named_parameters()] == [n for n, _ in parent.named_parameters()]
    assert [n for n, _ in q.named_buffers()] == [n for n, _ in parent.named_buffers()]
    assert [n for n, _ in q.named_children()] == [n for n, _ in parent.named_children()]


def test_gptq_refuses_the_quantizer_by_name():
    import brevitas_amd.quant as Q
    from brevitas_amd.graph.gptq import _plan
    w = torch.nn.Parameter(torch.randn(8, 64))
    with pytest.raises(TypeError, match='GroupwiseHQOIntQuant.*zero-point is searched on the finished group'):
        _plan(Q.ShiftedUint4WeightPerGroupFloatHQO(w, group_size=32), 64, False)


def test_layers_take_the_factories():
    import brevitas_amd.quant as Q
    from brevitas_amd.nn import QuantConv2d, QuantLinear
    torch.manual_seed(0)
    lin = QuantLinear(128, 8, weight_quant=functools.partial(Q.ShiftedUint4WeightPerGroupFloatHQO, group_size=64))
    x = torch.randn(3, 128, requires_grad=True)
    y = lin(x)
    wq, scale, zp, _ = lin.quant_weight()
    assert tuple(scale.shape) == tuple(zp.shape) == (8, 2, 1) and not zp.requires_grad
    assert torch.equal(y, torch.nn.functional.linear(x, wq, lin.bias))
    y.sum().backward()
    assert lin.weight.grad is not None and bool(torch.isfinite(lin.weight.grad).all())
    conv = QuantConv2d(16, 8, 3, bias=False,
                       weight_quant=functools.partial(Q.ShiftedUint8WeightPerGroupFloatHQO, group_size=16))
    assert conv(torch.randn(1, 16, 5, 5)).shape == (1, 8, 3, 3)
    assert tuple(conv.weight_quant.last_hqo_index.shape) == (8, 9)


# ---- the record of the per-unit family, against a recording stand-in library --------------------------------------

def test_the_record_is_kept_out_of_the_table_of_four(nat):  # noqa: F811
    fam = nat.GROUP_HQO
    assert fam not in nat.UNIT_FAMILIES and len(nat.UNIT_FAMILIES) == 4
    assert (fam.supported, fam.fwd, fam.bwd) == ('bvq_group_hqo_supported', 'bvq_group_hqo_fwd', 'bvq_group_hqo_bwd')
    assert all(e in nat._SIG and e in nat.EXPORTS for e in (fam.supported, fam.fwd, fam.bwd))
    assert [o.name for o in fam.outs] == ['scale', 'zp', 'stat', 'idx'] and fam.saved == ('stat', 'zp')
    assert fam.side == ('gscale',) and fam.extra == ('inv_beta', 'n_iters', 'lp') and fam.bwd_extra == ()
    assert fam.zp_per_unit and not fam.align_side
    assert all(f.bwd_extra is None for f in nat.UNIT_FAMILIES)   # the four are as they were


def test_the_beta_table(nat):  # noqa: F811
    table = nat.hqo_beta_table(10.0, 1.01, 20)
    assert len(table) == 21 and table[0] == torch.tensor(0.1).item()
    want = [torch.tensor(1.0 / (10.0 * 1.01 ** i), dtype=torch.float64).float().item() for i in range(21)]
    assert list(table) == want
    assert list(nat.hqo_beta_table(4.0, 2.0, 0)) == [0.25]
    assert nat.HQO_LP == {1.0: 0, 0.5: 1} and nat.HQO_MAX_ITERS == 63


@pytest.mark.parametrize('min_val, use_min', [(None, 0), (0.0, 0), (MIN_VAL, 1)])
def test_wrappers_hand_the_entries_the_header_order(nat, min_val, use_min):  # noqa: F811
    fam = nat.GROUP_HQO
    x, unit_len, units = _x('group_shifted')
    desc, thr = _desc(fam, x, unit_len)
    table = nat.hqo_beta_table(10.0, 1.01, 20)
    assert nat.group_hqo_supported(desc, x, 20, 1) is False     # the stand-in answers 0
    (name, args), = nat.lib.calls
    assert name == fam.supported and len(args) == len(nat._SIG[name][1])
    assert args[0]._obj is desc and args[1:] == (x.data_ptr(), 20, 1)
    nat.lib.calls.clear()
    y, scale, zp, stat, idx = nat.group_hqo_fwd(desc, x, table, 1, min_val, thr)
    (name, args), = nat.lib.calls
    assert name == fam.fwd and len(args) == len(nat._SIG[name][1]) and args[-1] == STREAM
    assert args[0]._obj is desc and args[1] == x.data_ptr()
    assert args[2:5] == (ctypes.addressof(table), 20, 1)
    assert args[5:8] == (float(min_val or 0.0), use_min, float(thr))
    assert args[8:-1] == tuple(t.data_ptr() for t in (y, scale, zp, stat, idx))
    assert y.shape == x.shape and y.dtype == x.dtype and y.data_ptr() != x.data_ptr()
    assert scale.shape == zp.shape == (units,) and stat.shape == (2 * units,) and idx.shape == (units,)
    assert scale.dtype == zp.dtype == stat.dtype == x.dtype and idx.dtype == torch.uint8
    nat.lib.calls.clear()
    g, gscale = torch.ones_like(x), torch.zeros(units, dtype=REC_DT)
    dx = nat.group_hqo_bwd(desc, g, x, stat, zp, gscale, min_val, thr)
    (name, args), = nat.lib.calls
    assert name == fam.bwd and len(args) == len(nat._SIG[name][1]) and args[-1] == STREAM
    assert args[0]._obj is desc and args[1:6] == tuple(t.data_ptr() for t in (g, x, stat, zp, gscale))
    assert args[6:-1] == (float(min_val or 0.0), use_min, float(thr), dx.data_ptr())
    assert dx.shape == x.shape and dx.dtype == x.dtype
    nat.lib.calls.clear()
    nat.group_hqo_bwd(desc, g, x, stat, zp, None, min_val, thr)
    assert nat.lib.calls[0][1][5] is None
    with pytest.raises(AssertionError):   # the forward's host arguments are none of the backward's
        nat.unit_bwd(fam, desc, g, x, stat, zp, None, ctypes.addressof(table), 20, 1, min_val, thr)
    with pytest.raises(AssertionError):   # a strided saved tensor
        nat.group_hqo_bwd(desc, g, x, torch.zeros(4 * units, dtype=REC_DT)[::2], zp, None, min_val, thr)


def test_function_shapes_saves_and_marks(nat, monkeypatch):  # noqa: F811
    """GroupHQOFakeQuantFn with the two wrappers replaced by recording stand-ins"""
    from brevitas_amd.core.quant import _fused
    x, unit_len, units = _x('group_shifted')
    fam = nat.GROUP_HQO
    outs, fwd_calls, bwd_calls = {}, [], []

    def fwd(desc, x, *rest):
        fwd_calls.append((desc, x) + rest)
        outs.update({o.name: torch.full((o.per_unit * units,), 2, dtype=o.dtype or x.dtype) for o in fam.outs})
        return (x * 2, *outs.values())

    def bwd(desc, g, x, *rest):
        bwd_calls.append((desc, g, x) + rest)
        return torch.full_like(x, 3)
    monkeypatch.setattr(nat, 'group_hqo_fwd', fwd)
    monkeypatch.setattr(nat, 'group_hqo_bwd', bwd)
    table = nat.hqo_beta_table(10.0, 1.01, 20)
    x.requires_grad_(True)
    y, scale, zp, idx = _fused.GroupHQOFakeQuantFn.apply(x, unit_len, MIN_VAL, 15.0, 0.0, 15.0, True, table, 1)
    desc, thr = _desc(fam, x, unit_len)
    (call,) = fwd_calls
    assert bytes(call[0]) == bytes(desc) and call[1] is x and call[2:] == (table, 1, MIN_VAL, thr)
    assert y.requires_grad and scale.shape == (units, 1) and scale.requires_grad
    assert zp.shape == (units, 1) and not zp.requires_grad and zp.data_ptr() == outs['zp'].data_ptr()
    assert idx.shape == (units,) and idx.dtype == torch.uint8 and not idx.requires_grad
    gy, gs = torch.randn(x.shape).to(REC_DT), torch.randn(units, 1).to(REC_DT)
    torch.autograd.backward([y, scale], [gy, gs])
    (call,) = bwd_calls
    assert bytes(call[0]) == bytes(desc) and torch.equal(call[1], gy) and call[2].data_ptr() == x.data_ptr()
    assert [t.data_ptr() for t in call[3:5]] == [outs['stat'].data_ptr(), outs['zp'].data_ptr()]
    assert torch.equal(call[5], gs.view(-1)) and call[6:] == (MIN_VAL, thr)
    assert torch.equal(x.grad, torch.full_like(x, 3))


def test_cabi_argument_checks_need_no_device():
    from brevitas_amd import _native as nat  # noqa: F811
    lib = nat.lib
    assert {'bvq_group_hqo_supported', 'bvq_group_hqo_fwd', 'bvq_group_hqo_bwd'} <= set(nat.EXPORTS)
    p, off = ctypes.c_void_p(4096), ctypes.c_void_p(4098)   # never dereferenced: every check fails before any device work

    def desc(inner=64, dt=nat.BF16, zp_pc=1):
        return nat.QuantDesc(1, 12, inner, dt, dt, dt, dt, 1, zp_pc, 0.0, 15.0, nat.ROUND, 0, 1, nat.OUT_DEQUANT,
                             nat.PRE_NONE)
    ok = desc()
    table = nat.hqo_beta_table(10.0, 1.01, 63)

    def fwd(d, x, tab, n, lp, y=p):
        return lib.bvq_group_hqo_fwd(ctypes.byref(d), x, tab, n, lp, 1e-10, 1, 15.0, y, p, p, p, p, None)

    def bwd(d, g, dx=p):
        return lib.bvq_group_hqo_bwd(ctypes.byref(d), g, p, p, p, None, 1e-10, 1, 15.0, dx, None)
    for n in (0, 20, 63):
        for lp in (0, 1):
            assert lib.bvq_group_hqo_supported(ctypes.byref(ok), p, n, lp) == 1
    for dt in (nat.BF16, nat.F16, nat.F32):
        for inner in (16, 32, 64, 128, 256):
            assert lib.bvq_group_hqo_supported(ctypes.byref(desc(inner, dt)), p, 20, 1) == 1
    assert lib.bvq_group_hqo_supported(None, p, 20, 1) == 0 and lib.bvq_group_hqo_supported(ctypes.byref(ok), None, 20, 1) == 0
    assert lib.bvq_group_hqo_supported(ctypes.byref(ok), off, 20, 1) == 0
    assert lib.bvq_group_hqo_supported(ctypes.byref(desc(48)), p, 20, 1) == 0
    assert lib.bvq_group_hqo_supported(ctypes.byref(desc(zp_pc=0)), p, 20, 1) == 0
    for n, word in ((-1, '-1 iterations'), (64, '64 iterations')):
        assert lib.bvq_group_hqo_supported(ctypes.byref(ok), p, n, 1) == 0
        assert fwd(ok, p, table, n, 1) == -2 and word in nat.last_error(), nat.last_error()
    for lp in (-1, 2):
        assert lib.bvq_group_hqo_supported(ctypes.byref(ok), p, 20, lp) == 0
        assert fwd(ok, p, table, 20, lp) == -2 and 'lp code' in nat.last_error(), nat.last_error()
    for bad in (0.0, -0.1, float('nan'), float('inf')):
        tab = (ctypes.c_float * 3)(0.1, bad, 0.05)
        assert fwd(ok, p, tab, 2, 1) == -2 and 'inv_beta 1' in nat.last_error(), (bad, nat.last_error())
    assert fwd(ok, off, table, 20, 1) == -2 and '16-byte' in nat.last_error()
    assert fwd(ok, p, table, 20, 1, y=off) == -2 and '16-byte' in nat.last_error()
    assert bwd(ok, off) == -2 and '16-byte' in nat.last_error()
    assert bwd(ok, p, dx=off) == -2 and '16-byte' in nat.last_error()
    assert fwd(desc(48), p, table, 20, 1) == -2 and 'group size 48' in nat.last_error()
    assert bwd(desc(zp_pc=0), p) == -2 and 'zero-point per channel' in nat.last_error()
    assert fwd(ok, None, table, 20, 1) == -1 and fwd(ok, p, None, 20, 1) == -1
    assert lib.bvq_group_hqo_fwd(None, p, table, 20, 1, 1e-10, 1, 15.0, p, p, p, p, p, None) == -1
    assert lib.bvq_group_hqo_bwd(None, p, p, p, p, None, 1e-10, 1, 15.0, p, None) == -1


# ---- autograd of the composed route ---------------------------------------------------------------------------------

@dtypes
def test_no_gradient_through_the_zero_point(dn):
    """the searched zero-point is a constant: the weight's gradient is that of the composed route at the kept
    zero-points"""
    g, bits = 32, 4
    w0 = outlier_weight(g, dn)
    gen = torch.Generator().manual_seed(3)
    grad = torch.randn(w0.shape, generator=gen).to(DT[dn])
    gscale = torch.randn(w0.numel() // g, generator=gen).to(DT[dn])
    w = torch.nn.Parameter(w0.clone())
    q = quantizer(w, g, bits)
    y, scale, zp, _ = q(w)
    assert not zp.requires_grad and zp.grad_fn is None and y.requires_grad and scale.requires_grad
    torch.autograd.backward([y, scale], [grad, gscale.view(scale.shape)])
    dw = w.grad.clone()
    w.grad = None
    y2, scale2 = q.quantize_at_zero_point(w, zp)
    assert same_bits(y2, y) and same_bits(scale2, scale)
    torch.autograd.backward([y2, scale2], [grad, gscale.view(scale.shape)])
    assert same_bits(w.grad, dw) and bool(torch.isfinite(dw.float()).all())
    assert same_bits(q.hqo_zero_point(w), zp)
    # the plain quantizer returns its zero-point inside the graph; this one does not, whatever the iteration count
    w3 = torch.nn.Parameter(w0.clone())
    y3, _, zp3, _ = quantizer(w3, g, bits, hqo_iters=0)(w3)
    w4 = torch.nn.Parameter(w0.clone())
    y4, _, zp4, _ = plain(w4, g, bits)(w4)
    assert same_bits(y3, y4) and same_bits(zp3, zp4) and zp4.requires_grad and not zp3.requires_grad
