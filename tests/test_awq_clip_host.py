"""AWQ's clip search on the host (brevitas_amd/graph/awq.py: awq_clip_weight): the composed route against a float64
reference built from GroupwiseMSEIntQuant.quantize_at_index, the ratios, the refusals, awq_mode(clip=True).  The device
route is held against the same reference in tests/test_gpu_awq_clip.py, which takes its inputs and checks from here.

The bound on a float32 loss is derived: B = (2 g + 8) * 2^-24 * |d|^T |hb| |d| covers two length-g float32
accumulations in any order plus the rounding of d."""
import copy
import functools

import pytest
import torch

from brevitas_amd import quant as Q
from brevitas_amd.graph import awq_clip_ratios, awq_clip_weight, awq_mode, awq_scale_weight, hessian_blocks
from brevitas_amd.nn import QuantLinear
from test_group_mse_host import same_bits

DT = {'f32': torch.float32, 'bf16': torch.bfloat16, 'f16': torch.float16}


def clip_inputs(rows, k, g, dn, seed=1234):
    """-> (weight [rows, k] with ~3 % outliers and one all-zero group, H [k, k] of 64 calibration rows with one dead
    column), on the CPU"""
    gen = torch.Generator().manual_seed(seed + 7 * rows + k)
    w = torch.randn(rows, k, generator=gen)
    w = torch.where(torch.rand(rows, k, generator=gen) < 0.03, w * 6.0, w)
    w[rows // 2, :g] = 0.0
    x = torch.randn(64, k, generator=gen) * torch.randn(k, generator=gen).exp()
    x[:, k // 3] = 0.0
    return w.to(DT[dn]), (2.0 / 64) * (x.t() @ x)


def first_min(losses):
    """per group the first candidate strictly below every earlier one"""
    idx, best = torch.zeros(losses.shape[:2], dtype=torch.uint8), losses[..., 0]
    for i in range(1, losses.shape[-1]):
        better = losses[..., i] < best
        idx, best = torch.where(better, torch.full_like(idx, i), idx), torch.where(better, losses[..., i], best)
    return idx


def check_search(x, g, bits, hb, ratios, index, losses, y, scale, stat=None):
    """the four assertions of the clip search for x [R, K] (CPU tensors throughout; y None: a caller that holds
    y / input_scale only)"""
    rows, nj = x.shape[0], x.shape[1] // g
    xp = torch.nn.Parameter(x)
    mse = Q.Int8WeightPerGroupFloatMSE(xp, group_size=g, bit_width=bits, mse_ratios=ratios.tolist())
    l64, bound = [], []
    with torch.no_grad():
        for i in range(len(ratios)):
            yi = mse.quantize_at_index(xp, torch.full((rows * nj,), i, dtype=torch.uint8))[0]
            d = (yi.double() - x.double()).reshape(rows, nj, g)
            l64.append(torch.einsum('rja,jab,rjb->rj', d, hb.double(), d))
            bound.append((2 * g + 8) * 2.0 ** -24 * torch.einsum('rja,jab,rjb->rj', d.abs(), hb.double().abs(), d.abs()))
        want_y, want_scale = mse.quantize_at_index(xp, index)
    l64, bound = torch.stack(l64, -1), torch.stack(bound, -1)
    finite = torch.isfinite(l64)     # a group whose scale is 0 / 0 (zeros, where the lower bound underflows) has NaN losses
    err = (losses.double() - l64).abs()
    print('worst |loss - L64| / B: %.3g' % float((err / bound.clamp_min(1e-300))[finite].max()))
    assert bool((err <= bound)[finite].all()) and torch.equal(torch.isfinite(losses), finite)  # 1
    assert torch.equal(index, first_min(losses))                                                # 2
    whole = finite.all(-1)
    slack = 2 * bound.max(-1).values
    picked = l64.gather(-1, index.long().unsqueeze(-1)).squeeze(-1)
    assert bool((picked <= l64.min(-1).values + slack)[whole].all())                            # 3
    low2 = l64.sort(-1).values[..., :2]
    clear = whole & ((low2[..., -1] - low2[..., 0] >= slack) | (len(ratios) == 1))
    print('groups with a clear float64 minimum: %d of %d' % (int(clear.sum()), clear.numel()))
    assert torch.equal(index[clear], first_min(l64)[clear]) and bool((index[~whole] == 0).all())
    assert (y is None or same_bits(y, want_y)) and same_bits(scale.reshape(want_scale.shape), want_scale)      # 4
    if stat is not None:
        assert same_bits(stat, x.abs().reshape(rows, nj, g).amax(-1))
    return index


@pytest.mark.parametrize('dn', ['f32', 'bf16'])
@pytest.mark.parametrize('bits', [4, 8])
def test_composed_route_against_float64(dn, bits):
    g = 32
    w, h = clip_inputs(33, 2 * g, g, dn)
    ratios = awq_clip_ratios()
    wp = torch.nn.Parameter(w)
    before = w.clone()
    res = awq_clip_weight(wp, h, Q.Int8WeightPerGroupFloat(wp, group_size=g, bit_width=bits), ratios=ratios)
    assert torch.equal(wp.detach(), before)
    assert res.index.shape == (33, 2) and res.index.dtype == torch.uint8 and res.losses.shape == (33, 2, 10)
    check_search(w, g, bits, hessian_blocks(h, g), ratios, res.index, res.losses, res.q, res.scale)
    assert bool((res.index == 0).any()) and bool((res.index > 0).any())


def test_ratios():
    r = awq_clip_ratios()
    assert r.dtype == torch.float32 and r.shape == (10,) and float(r[0]) == 1.0
    assert torch.equal(r, 1 - torch.arange(10, dtype=torch.float32) / 20)
    assert awq_clip_ratios(16, 1.0).shape == (16,) and float(awq_clip_ratios(4, 0.25)[0]) == 1.0
    with pytest.raises(ValueError, match='17 clip ratios'):
        awq_clip_ratios(34, 0.5)
    with pytest.raises(ValueError):
        awq_clip_ratios(20, 0.0)


def test_refusals_name_the_quantizer():
    w = torch.nn.Parameter(torch.randn(8, 64))
    h = torch.eye(64)
    with pytest.raises(TypeError, match='asymmetric quantizer GroupwiseRescalingIntQuant'):
        awq_clip_weight(w, h, Q.ShiftedUint4WeightPerGroupFloat(w, 32))
    with pytest.raises(TypeError, match='RescalingIntQuant.*per column'):
        awq_clip_weight(w, h, Q.Int8WeightPerChannelFloat(w))
    with pytest.raises(TypeError, match='GroupwiseMSEIntQuant'):
        awq_clip_weight(w, h, Q.Int4WeightPerGroupFloatMSE(w, 32))


def test_awq_mode_with_clip():
    torch.manual_seed(3)
    wq = functools.partial(Q.Int4WeightPerGroupFloat, group_size=16)
    model = torch.nn.Sequential(QuantLinear(32, 48, weight_quant=wq), torch.nn.ReLU(), QuantLinear(48, 16, weight_quant=wq))
    plain = copy.deepcopy(model)
    batches = [torch.randn(40, 32) * torch.linspace(0.2, 3.0, 32) for _ in range(3)]
    with awq_mode(plain, n_grid=10) as ref:
        for b in batches:
            ref.model(b)
        unclipped = ref.update()
    with awq_mode(model, n_grid=10, clip=True) as awq:
        for i in (0, 2):
            for b in batches:
                awq.model(b)
            w, h = model[i].weight.detach().clone(), awq._h.double()
            same_data = awq_scale_weight(model[i].weight, awq._h, awq.act_mean, model[i].weight_quant, n_grid=10)
            res = awq.update()
            clip = awq.last_clip
            assert clip.index.shape == (w.shape[0], w.shape[1] // 16) and torch.equal(res.q, clip.q)
            assert torch.equal(model[i].weight.detach(), clip.q) and torch.equal(model[i].frozen_weight_scale, clip.scale)
            assert torch.equal(model[i].awq_input_scale, same_data.input_scale) and res.index == same_data.index
            # the layer's output error: candidate 0 is the unclipped weight, so the search can only lower it, up to the
            # rounding bound of the two losses it compared in every group
            d = (same_data.q - w).double().reshape(w.shape[0], -1, 16)
            slack = 2 * (2 * 16 + 8) * 2.0 ** -24 * torch.einsum(
                'rja,jab,rjb->', d.abs(), hessian_blocks(h, 16).double().abs(), d.abs())
            err = [float(torch.trace((q - w).double() @ h @ (q - w).double().t())) for q in (clip.q, same_data.q)]
            print('layer %d: tr(dW H dW^T) clipped %.6g, unclipped %.6g' % (i, err[0], err[1]))
            assert err[0] <= err[1] + float(slack)
            assert bool((clip.index > 0).any())
            if i == 0:
                assert torch.equal(same_data.q, unclipped.q)      # clip=False computes what it computed before
    assert model[0].frozen_weight_scale is not None and model[2].frozen_weight_scale is not None
