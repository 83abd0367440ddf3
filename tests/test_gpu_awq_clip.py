"""AWQ's clip search on the device: the one-launch kernel (csrc/bvq_group_clip.hip) behind awq_clip_weight against the
float64 reference of tests/test_awq_clip_host.py (check_search: the derived bound on every loss, the pick against the
kernel's own losses and against the float64 minimum, y / scale / stat bit-equal to quantize_at_index), at R = 33 rows
(a ragged row tile) of two groups (two Hessian blocks), and at g = 32 the candidate counts 1 and 16, one row, more rows
than the 512 of a workgroup, and three groups per row."""
import pytest
import torch

import brevitas_amd.config as config
from brevitas_amd import _native as nat
from brevitas_amd import quant as Q
from brevitas_amd.graph import awq_clip_ratios, awq_clip_weight, hessian_blocks
from test_awq_clip_host import check_search, clip_inputs
from test_group_mse_host import same_bits

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SWEEP = [(g, dn, bits, 33, 2, 10) for g in (16, 32, 64, 128) for dn in ('f32', 'bf16', 'f16') for bits in (4, 8)]
EDGES = [(32, 'bf16', 4, 33, 2, 1), (32, 'bf16', 4, 33, 2, 16), (32, 'f32', 4, 1, 2, 10), (32, 'f16', 4, 517, 2, 10),
         (32, 'bf16', 8, 33, 3, 10)]


@pytest.fixture
def launches(monkeypatch):
    """what every launch of the kernel's wrapper returned: (y, scale, stat, idx, losses)"""
    out, real = [], nat.group_clip_fwd
    monkeypatch.setattr(nat, 'group_clip_fwd', lambda *a: out.append(real(*a)) or out[-1])
    return out


def searched(w, h, g, bits, ratios, input_scale=None):
    wd = torch.nn.Parameter(w.to(DEV))
    quant = Q.Int8WeightPerGroupFloat(wd, group_size=g, bit_width=bits).to(DEV)
    return awq_clip_weight(wd, h.to(DEV), quant, ratios=ratios, input_scale=input_scale)


@pytest.mark.parametrize('g,dn,bits,rows,groups,n', SWEEP + EDGES)
def test_kernel_against_float64(g, dn, bits, rows, groups, n, launches):
    w, h = clip_inputs(rows, groups * g, g, dn)
    ratios = awq_clip_ratios(2 * n, 0.5)
    res = searched(w, h, g, bits, ratios)
    assert len(launches) == 1 and res.losses.shape == (rows, groups, n)
    y, scale, stat, idx, losses = (t.cpu() for t in launches[0])
    assert same_bits(res.q.cpu(), y) and torch.equal(res.index.cpu(), idx)
    check_search(w, g, bits, hessian_blocks(h, g), ratios, idx, losses, y, scale, stat)
    if n > 1 and rows > 1:
        assert bool((idx == 0).any()) and bool((idx > 0).any())


def test_input_scale_fused_against_composed(launches, monkeypatch):
    g, bits = 32, 4
    w, h = clip_inputs(33, 2 * g, g, 'bf16')
    s = torch.exp2(torch.rand(2 * g, generator=torch.Generator().manual_seed(5)) * 2 - 1).to(torch.bfloat16)
    ratios = awq_clip_ratios()
    fused = searched(w, h, g, bits, ratios, s.to(DEV))
    monkeypatch.setattr(config, 'FUSED_PATHS', False)
    composed = searched(w, h, g, bits, ratios, s.to(DEV))
    assert len(launches) == 1
    for res in (fused, composed):
        check_search(w * s, g, bits, hessian_blocks(h, g, s), ratios, res.index.cpu(), res.losses.cpu(), None,
                     res.scale.cpu())
    same = (fused.index == composed.index).cpu()
    assert same_bits(fused.q.cpu().reshape(33, 2, g)[same], composed.q.cpu().reshape(33, 2, g)[same])
    assert same_bits(fused.scale.cpu()[same], composed.scale.cpu()[same])


def test_misaligned_view_takes_the_composed_route(launches):
    g, bits = 32, 4
    w, h = clip_inputs(33, 2 * g, g, 'f32')
    ratios = awq_clip_ratios()
    buf = torch.empty(w.numel() + 1, device=DEV)
    view = buf[1:].view(w.shape).copy_(w)
    quant = Q.Int8WeightPerGroupFloat(torch.nn.Parameter(view), group_size=g, bit_width=bits).to(DEV)
    from brevitas_amd.core.quant import _fused
    d = _fused.unit_call(view, g, False, 1.0, -8.0, 7.0, False)[0]
    hb = hessian_blocks(h.to(DEV), g)
    assert not nat.group_clip_supported(d, view, hb, 10) and nat.group_clip_supported(d, view.clone(), hb, 10)
    res = awq_clip_weight(view, h.to(DEV), quant, ratios=ratios)
    assert not launches
    check_search(w, g, bits, hessian_blocks(h, g), ratios, res.index.cpu(), res.losses.cpu(), res.q.cpu(),
                 res.scale.cpu())
