"""The oracle's gradient of tensor clamp bounds (orc_fakequant_bwd_bounds: a learned bit width, whose integer range is
a pair of tensors in the autograd graph) against torch CPU autograd of the reference's chain
x / scale + zp -> round_ste -> tensor_clamp(., qmin, qmax) -> (. - zp) * scale, with qmin / qmax as leaf tensors."""
import numpy as np
import pytest
import torch

DT = {'f32': torch.float32, 'bf16': torch.bfloat16, 'f16': torch.float16}


class _RoundSte(torch.autograd.Function):
    """round_ste: torch.round forward, identity backward (B/ops/autograd_ste_ops.py)"""

    @staticmethod
    def forward(ctx, t):
        return torch.round(t)

    @staticmethod
    def backward(ctx, g):
        return g


def _torch_bounds_grad(x, g, scale, zp, qmin, qmax, per_channel_bounds):
    """torch's d(qmin), d(qmax): per channel when per_channel_bounds (float32 only: the [1, C, 1] leaves then keep every
    op in x's dtype), else as 0-dim leaves (the reference's own form)"""
    ch = x.shape[1]
    if per_channel_bounds:
        lo = torch.full((ch,), qmin, requires_grad=True)
        hi = torch.full((ch,), qmax, requires_grad=True)
        lo_v, hi_v = lo.view(1, ch, 1), hi.view(1, ch, 1)
    else:
        lo = torch.tensor(qmin, requires_grad=True)
        hi = torch.tensor(qmax, requires_grad=True)
        lo_v, hi_v = lo, hi
    t = _RoundSte.apply(x / scale + zp)
    t = torch.where(t > hi_v, hi_v, t)   # tensor_clamp, B/function/ops.py:98-100
    t = torch.where(t < lo_v, lo_v, t)
    y = (t - zp) * scale
    y.backward(g)
    return lo.grad.double().numpy(), hi.grad.double().numpy()


def _case(oracle, dn, shape, bits, seed, per_channel):
    O = oracle
    dt = DT[dn]
    outer, ch, inner = shape
    gen = torch.Generator().manual_seed(seed)
    x = (torch.randn(shape, generator=gen) * 3 * 2.0 ** (bits - 3)).to(dt)  # clips on both sides at every width
    g = torch.randn(shape, generator=gen).to(dt)
    qmin, qmax = float(-(2 ** (bits - 1))), float(2 ** (bits - 1) - 1)
    if per_channel:
        scale = (torch.rand(1, ch, 1, generator=gen) * 0.4 + 0.1).to(dt)
    else:
        scale = torch.tensor(0.3, dtype=dt)
    zp = torch.tensor(1.0, dtype=dt)
    code = {'f32': O.F32, 'bf16': O.BF16, 'f16': O.F16}[dn]
    d = O.make_desc(outer, ch, inner, code, code, code, code, scale_per_channel=per_channel, qmin=qmin, qmax=qmax)
    xn, _ = O.from_torch(x.reshape(-1))
    gn, _ = O.from_torch(g.reshape(-1))
    sn, _ = O.from_torch(scale.reshape(-1))
    zn, _ = O.from_torch(zp.reshape(-1))
    db = O.fakequant_bwd_bounds(d, gn, xn, sn, zn).astype(np.float64)
    return x, g, scale, zp, qmin, qmax, db, d, (xn, gn, sn, zn)


@pytest.mark.parametrize('per_channel', [False, True], ids=['tensor', 'channel'])
@pytest.mark.parametrize('bits', [3, 4, 8])
def test_bounds_grad_float32_matches_autograd(oracle, bits, per_channel):
    x, g, scale, zp, qmin, qmax, db, _, _ = _case(oracle, 'f32', (6, 5, 97), bits, 17 + bits, per_channel)
    dlo, dhi = _torch_bounds_grad(x, g, scale, zp, qmin, qmax, per_channel)
    want = np.stack([np.atleast_1d(dlo), np.atleast_1d(dhi)])
    assert want.shape == db.shape
    assert np.abs(want).max() > 1.0, 'the case must clip elements on both sides'
    assert np.all(np.abs(db - want) <= 1e-6 * np.maximum(np.abs(want), 1.0)), (db, want)


@pytest.mark.parametrize('dn', ['bf16', 'f16'])
@pytest.mark.parametrize('bits', [3, 4])
def test_bounds_grad_16bit_within_sum_tolerance(oracle, dn, bits):
    """torch sums where()'s masked gradient in the 16-bit dtype before casting it to the float32 bound: agreement within
    the rounding of that sum"""
    x, g, scale, zp, qmin, qmax, db, _, _ = _case(oracle, dn, (4, 3, 250), bits, 99 + bits, False)
    dlo, dhi = _torch_bounds_grad(x, g, scale, zp, qmin, qmax, False)
    want = np.array([[float(dlo)], [float(dhi)]])
    rel = {'bf16': 2e-2, 'f16': 5e-3}[dn]
    mag = np.abs(want).max()
    assert mag > 1.0
    assert np.all(np.abs(db - want) <= rel * (np.abs(want) + mag + 1.0)), (db, want)


def test_bounds_grad_straight_through_clamp_is_zero(oracle):
    *_, db, d, (xn, gn, sn, zn) = _case(oracle, 'f32', (2, 3, 50), 3, 5, True)
    assert np.abs(db).max() > 0
    d.clamp_ste = 1
    assert np.array_equal(oracle.fakequant_bwd_bounds(d, gn, xn, sn, zn), np.zeros((2, 3), dtype=np.float32))
