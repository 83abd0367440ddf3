"""AWQ on the host (brevitas_amd/graph/awq.py): the candidate table, the composed candidates against the quantizer
itself, the search on a known case, ties and non-finite candidates, awq_mode on a small model, the refusals, and the
independence of every result from the step size.  Everything here runs the composed route on the CPU; the device route
is held against it in tests/test_gpu_awq.py, which takes its inputs from here."""
import functools

import pytest
import torch
import torch.nn.functional as F

import brevitas_amd.config as config
from brevitas_amd import quant as Q
from brevitas_amd.graph import (awq_candidates, awq_losses, awq_mode, awq_scale_weight, awq_table, freeze_awq_weight)
from brevitas_amd.nn import QuantConv2d, QuantLinear
from test_group_mse_host import same_bits

DT = {'f32': torch.float32, 'bf16': torch.bfloat16, 'f16': torch.float16}
FACTORIES = {'sym': Q.Int4WeightPerGroupFloat, 'asym': Q.ShiftedUint4WeightPerGroupFloat}


def search_inputs(dtype=torch.float32, device='cpu'):
    """the known case: a small weight, and calibration rows of which six input columns are 30 times the others
    -> (weight parameter, Hessian as gptq_mode accumulates it, act_mean), computed on the CPU and moved"""
    torch.manual_seed(123456)
    w = torch.randn(24, 96) * 0.02
    x = torch.randn(512, 96)
    x[:, 0:56:11] *= 30.0
    h = (2.0 / x.shape[0]) * (x.t() @ x)
    return torch.nn.Parameter(w.to(dtype).to(device)), h.to(device), x.abs().mean(0).to(device)


# ---- the table -------------------------------------------------------------------------------------------------------

def test_table_rows():
    torch.manual_seed(1)
    am = torch.rand(64) * 4.0 + 0.01
    am[5] = 0.0                                    # a dead column
    t = awq_table(am, 20, torch.float32)
    assert t.shape == (20, 64) and t.dtype == torch.float32
    assert torch.equal(t[0], torch.ones(64))       # exactly: the search can always fall back to round-to-nearest
    assert bool(torch.isfinite(t).all()) and bool((t > 0).all())
    # s / sqrt(max * min): max * min == 1 up to the roundings of the square root, the two quotients and the product
    torch.testing.assert_close(t.max(1).values * t.min(1).values, torch.ones(20), rtol=4 * 2.0 ** -23, atol=0)
    # the exponent grows along the rows: a column above the geometric middle rises, one below falls
    assert bool((t[1:, am.argmax()] > t[:-1, am.argmax()]).all())
    assert awq_table(am, 20, torch.bfloat16).dtype == torch.bfloat16
    assert torch.equal(awq_table(am, 20, torch.bfloat16), t.to(torch.bfloat16))
    with pytest.raises(ValueError, match='n_grid'):
        awq_table(am, 0, torch.float32)


# ---- candidates ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dn', list(DT))
@pytest.mark.parametrize('kind', list(FACTORIES))
def test_ones_are_the_quantizer_itself(kind, dn):
    torch.manual_seed(7)
    w = torch.nn.Parameter((torch.randn(6, 96) * 0.05).to(DT[dn]))
    q = FACTORIES[kind](w, 32)
    with torch.no_grad():
        want_y, want_s, want_z, _ = q(w)
    y, s, z = awq_candidates(w, torch.ones(1, 96, dtype=DT[dn]), q)
    assert y.shape == (1, 6, 96)
    assert same_bits(y[0], want_y) and same_bits(s[0], want_s)
    assert same_bits(z[0] if kind == 'asym' else z, want_z)


def test_candidates_restate_the_definition():
    """mul, the quantizer on the scaled weight as its own parameter, div"""
    torch.manual_seed(8)
    w = torch.nn.Parameter((torch.randn(5, 64) * 0.05).to(torch.bfloat16))
    table = (torch.rand(3, 64) * 3 + 0.25).to(torch.bfloat16)
    for kind, make in FACTORIES.items():
        y, s, z = awq_candidates(w, table, make(w, 16))
        for i in range(3):
            ws = torch.nn.Parameter(w.detach() * table[i])
            with torch.no_grad():
                yq, sq, zq, _ = make(ws, 16)(ws)
            assert same_bits(y[i], yq / table[i]) and same_bits(s[i], sq), (kind, i)
            assert same_bits(z[i] if kind == 'asym' else z, zq), (kind, i)


@pytest.mark.parametrize('kind', list(FACTORIES))
def test_step_size_changes_no_bit(kind, monkeypatch):
    w, h, am = search_inputs()
    q = FACTORIES[kind](w, 32)
    table = awq_table(am, 7, w.dtype)
    whole = awq_candidates(w, table, q)
    res = awq_scale_weight(w, h, am, q, n_grid=7)
    monkeypatch.setattr(config, 'AWQ_CANDIDATE_BYTES', 1)    # one candidate per step
    for a, b in zip(awq_candidates(w, table, q), whole):
        assert same_bits(a, b)
    one = awq_scale_weight(w, h, am, q, n_grid=7)
    assert one.index == res.index
    for name in ('q', 'scale', 'zero_point', 'input_scale', 'losses'):
        assert same_bits(getattr(one, name), getattr(res, name)), name


# ---- the search ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('kind', list(FACTORIES))
def test_search_known_answer(kind):
    w, h, am = search_inputs()
    before = w.detach().clone()
    res = awq_scale_weight(w, h, am, FACTORIES[kind](w, 32), n_grid=20)
    print('kept %d, losses %s' % (res.index, [float('%.6g' % v) for v in res.losses]))
    assert torch.equal(w.detach(), before)                        # nothing is changed in place
    assert res.index > 0                                          # salient columns: plain rounding is not the best
    assert float(res.losses[res.index]) < float(res.losses[0])
    assert float(res.losses[res.index]) == float(res.losses.min())
    assert res.losses.dtype == torch.float32 and res.losses.shape == (20,)
    table = awq_table(am, 20, w.dtype)
    assert torch.equal(res.input_scale, table[res.index])
    y, s, z = awq_candidates(w, table, FACTORIES[kind](w, 32))
    assert same_bits(res.q, y[res.index]) and same_bits(res.scale, s[res.index])
    assert same_bits(res.zero_point, z[res.index] if kind == 'asym' else z)
    assert same_bits(res.losses, awq_losses(y, w, h))
    assert float(res.bit_width) == 4.0
    # the codes: round(weight * input_scale / scale + zero_point) reproduces q
    g = (w.detach() * res.input_scale).reshape(24, 3, 32)
    zp = res.zero_point if kind == 'asym' else 0.0
    lo, hi = (0.0, 15.0) if kind == 'asym' else (-8.0, 7.0)
    codes = torch.clamp(torch.round(g / res.scale + zp), lo, hi)
    assert same_bits(((codes - zp) * res.scale).reshape(24, 96) / res.input_scale, res.q)


def test_ties_keep_the_earlier_and_inf_is_never_kept(monkeypatch):
    import brevitas_amd.graph.awq as A
    w, h, am = search_inputs()
    q = Q.Int4WeightPerGroupFloat(w, 32)
    good = awq_table(am, 20, w.dtype)[8]

    def table_of(rows):
        monkeypatch.setattr(A, 'awq_table', lambda act_mean, n_grid, dtype: torch.stack(rows).to(dtype))
        return awq_scale_weight(w, h, am, q, n_grid=len(rows), name='fc')
    res = table_of([torch.ones(96), good, good])
    assert res.index == 1 and float(res.losses[1]) == float(res.losses[2])
    bad = good.clone()
    bad[3] = float('inf')
    res = table_of([bad, torch.ones(96), bad])
    assert res.index == 1 and not bool(torch.isfinite(res.losses[[0, 2]]).any())
    with pytest.raises(RuntimeError, match="'fc'"):
        table_of([bad, bad])


# ---- awq_mode --------------------------------------------------------------------------------------------------------

def _mlp():
    torch.manual_seed(3)
    return torch.nn.Sequential(
        QuantLinear(32, 48, weight_quant=functools.partial(Q.Int4WeightPerGroupFloat, group_size=16)),
        torch.nn.ReLU(),
        QuantLinear(48, 16, weight_quant=functools.partial(Q.ShiftedUint4WeightPerGroupFloat, group_size=16)))


def test_awq_mode_on_a_cpu_mlp():
    model = _mlp()
    torch.manual_seed(4)
    batches = [torch.randn(40, 32) for _ in range(3)]
    for b in batches:
        b[:, ::9] *= 20.0
    w1 = model[0].weight.detach().clone()
    with awq_mode(model, n_grid=10) as awq:
        assert [name for name, _ in awq.layers] == ['0', '2']
        for b in batches:
            assert awq.model(b) is None                     # the forward stops behind the current layer
        x1 = torch.cat(batches)
        torch.testing.assert_close(awq.act_mean, x1.abs().mean(0), rtol=1e-5, atol=0)
        torch.testing.assert_close(awq._h, (2.0 / 120) * (x1.t() @ x1), rtol=1e-4, atol=1e-5)
        want1 = awq_scale_weight(model[0].weight, awq._h, awq.act_mean, model[0].weight_quant, n_grid=10)
        r1 = awq.update()
        assert r1.index == want1.index and torch.equal(r1.q, want1.q)
        # frozen: the weight holds q, quant_weight() answers from the buffers, the factor is a buffer of its own
        assert torch.equal(model[0].weight.detach(), r1.q) and not torch.equal(r1.q, w1)
        w, s, z, bw = model[0].quant_weight()
        assert w is model[0].weight and s is model[0].frozen_weight_scale and torch.equal(s, r1.scale)
        assert torch.equal(model[0].awq_input_scale, r1.input_scale) and model[0].awq_input_scale.shape == (32,)
        for b in batches:
            awq.model(b)
        # the second layer calibrates on the frozen first
        x2 = torch.cat([F.relu(F.linear(b, r1.q, model[0].bias)) for b in batches]).detach()
        torch.testing.assert_close(awq.act_mean, x2.abs().mean(0), rtol=1e-5, atol=0)
        torch.testing.assert_close(awq._h, (2.0 / 120) * (x2.t() @ x2), rtol=1e-4, atol=1e-5)
        r2 = awq.update()
        with pytest.raises(RuntimeError, match='awq_mode.update: every layer'):
            awq.update()
    assert 'forward' not in model[0].__dict__ and 'forward' not in model[2].__dict__
    x = batches[0]
    assert torch.equal(model[0](x), F.linear(x, r1.q, model[0].bias))
    assert torch.equal(model(x), F.linear(F.relu(F.linear(x, r1.q, model[0].bias)), r2.q, model[2].bias))
    # the state dict carries the factor; it loads into a fresh model frozen the same way
    sd = model.state_dict()
    assert {'0.awq_input_scale', '2.awq_input_scale', '0.frozen_weight_scale', '2.frozen_weight_zero_point'} <= set(sd)
    fresh = _mlp()
    for i in (0, 2):
        k = fresh[i].weight.shape[1]
        freeze_awq_weight(fresh[i], torch.zeros(fresh[i].weight.shape[0], k // 16, 1), torch.zeros(()), torch.ones(k))
    fresh[2].frozen_weight_zero_point = torch.zeros_like(sd['2.frozen_weight_zero_point'])
    fresh.load_state_dict(sd)
    assert torch.equal(fresh[0].awq_input_scale, r1.input_scale)
    assert torch.equal(fresh[2].awq_input_scale, r2.input_scale)
    assert torch.equal(fresh(x), model(x))
    # a frozen layer is skipped, as GPTQ skips it
    with awq_mode(model) as again:
        assert again.num_layers == 0


def test_gptq_mode_is_unchanged_by_the_shared_machinery():
    from brevitas_amd.graph import gptq_mode
    model = _mlp()
    with gptq_mode(model) as gptq:
        with pytest.raises(RuntimeError, match=r"gptq_mode.update: layer '0' has seen no calibration batch"):
            gptq.update()
        gptq.model(torch.randn(64, 32))
        assert not hasattr(gptq, '_abs') and gptq._n == 64
        gptq.update()
    assert 'awq_input_scale' not in model[0]._buffers and model[0].frozen_weight_scale is not None


# ---- refusals --------------------------------------------------------------------------------------------------------

def _linear(factory, **kw):
    return torch.nn.Sequential(QuantLinear(64, 8, weight_quant=functools.partial(factory, **kw) if kw else factory))


def test_refusals_are_raised_on_entry_and_name_the_quantizer():
    from brevitas_amd.core.bit_width import BitWidthParameter
    from brevitas_amd.core.function_wrapper import FloorSte
    cases = [(_linear(Q.Int4WeightPerGroupFloatMSE, group_size=32), TypeError, 'GroupwiseMSEIntQuant'),
             (_linear(Q.ShiftedUint4WeightPerGroupFloatHQO, group_size=32), TypeError, 'GroupwiseHQOIntQuant'),
             (_linear(Q.MXInt8Weight, group_size=32), TypeError, 'MXQuant'),
             (_linear(Q.Int8WeightNormL2PerChannelFloat), TypeError, 'WeightNormIntQuant'),
             (_linear(Q.Int8WeightPerChannelFloat), TypeError, 'RescalingIntQuant.*per column'),
             (_linear(Q.Int8WeightPerTensorFloat), TypeError, 'RescalingIntQuant.*per column')]
    learned = _linear(Q.Int4WeightPerGroupFloat, group_size=32)
    learned[0].weight_quant.msb_clamp_bit_width_impl = BitWidthParameter(4)
    cases.append((learned, TypeError, 'awq: GroupwiseRescalingIntQuant with a learned bit width'))
    floor = _linear(Q.Int4WeightPerGroupFloat, group_size=32)
    floor[0].weight_quant.int_quant.float_to_int_impl = FloorSte()
    cases.append((floor, TypeError, 'awq: GroupwiseRescalingIntQuant.*half-even'))
    conv = torch.nn.Sequential(QuantConv2d(32, 8, 1, weight_quant=functools.partial(Q.Int4WeightPerGroupFloat,
                                                                                   group_size=32)))
    cases.append((conv, NotImplementedError, r"'0' \(QuantConv2d.*GroupwiseRescalingIntQuant"))
    for model, exc, match in cases:
        before = [p.detach().clone() for p in model.parameters()]
        with pytest.raises(exc, match=match):
            awq_mode(model).__enter__()
        assert 'forward' not in model[0].__dict__
        assert all(torch.equal(a, b) for a, b in zip(before, model.parameters()))
    w = torch.nn.Parameter(torch.randn(8, 64))
    with pytest.raises(TypeError, match='GroupwiseMSEIntQuant'):
        awq_candidates(w, torch.ones(1, 64), Q.Int4WeightPerGroupFloatMSE(w, 32))
    with pytest.raises(ValueError, match='table'):
        awq_candidates(w, torch.ones(1, 32), Q.Int4WeightPerGroupFloat(w, 32))
