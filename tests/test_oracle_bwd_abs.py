"""The oracle's per-channel error scale of the reduced gradients (orc_fakequant_bwd_abs): the sum of |term| over the terms
orc_fakequant_bwd adds up for dscale and dzp.  Where every term of a channel has one sign it is |dscale| itself; otherwise
it is at least that, and it never depends on the other channels."""
import numpy as np
import pytest
import torch

DT = {'f32': torch.float32, 'bf16': torch.bfloat16, 'f16': torch.float16}


def _run(O, dn, x, g, scale, zp, **kw):
    code = O.from_torch(torch.zeros(1, dtype=DT[dn]))[1]
    outer, ch, inner = x.shape
    od = O.make_desc(outer, ch, inner, code, code, code, O.F32, scale_per_channel=ch > 1, **kw)
    xn, _ = O.from_torch(x.reshape(-1))
    gn, _ = O.from_torch(g.reshape(-1))
    sn, _ = O.from_torch(scale.reshape(-1))
    zn = zp.numpy().astype(np.float32)
    _, ds, dz = O.fakequant_bwd(od, gn, xn, sn, zn)
    a_s, a_z = O.fakequant_bwd_abs(od, gn, xn, sn, zn)
    return ds, dz, a_s, a_z


@pytest.mark.parametrize('dn', list(DT))
def test_equals_magnitude_when_every_term_has_one_sign(oracle, dn):
    # x = 0, g > 0 and a zero-point of -200: every code is clamped to qmin = -128 (dt = 0, so the second dscale term is
    # -0), t5 = qmin - zp = 72 and the first term g * 72 > 0; every dzp term is 0 - g * s < 0
    gen = torch.Generator().manual_seed(11)
    outer, ch, inner = 4, 6, 50
    x = torch.zeros(outer, ch, inner, dtype=DT[dn])
    g = (torch.rand(outer, ch, inner, generator=gen) * (1 + torch.arange(ch).view(1, ch, 1) * 100.0) + 0.1).to(DT[dn])
    scale = torch.linspace(0.1, 2.0, ch).to(DT[dn])
    ds, dz, a_s, a_z = _run(oracle, dn, x, g, scale, torch.tensor([-200.0]))
    assert np.all(ds > 0) and np.all(dz < 0)
    assert np.array_equal(a_s.astype(np.float32), np.abs(ds))
    assert np.array_equal(a_z.astype(np.float32), np.abs(dz))


@pytest.mark.parametrize('dn', list(DT))
def test_at_least_magnitude_and_per_channel(oracle, dn):
    gen = torch.Generator().manual_seed(13)
    outer, ch, inner = 7, 5, 33
    x = (torch.randn(outer, ch, inner, generator=gen) * 3).to(DT[dn])
    g = torch.randn(outer, ch, inner, generator=gen).to(DT[dn])
    scale = torch.tensor([0.1, 0.2, 0.5, 1.0, 2.0]).to(DT[dn])  # (x / s / s stays finite in f16)
    for zp in (torch.zeros(1), torch.tensor([3.0])):
        for clamp_ste in (False, True):
            ds, dz, a_s, a_z = _run(oracle, dn, x, g, scale, zp, qmin=-8.0, qmax=7.0, clamp_ste=clamp_ste)
            exact = np.abs(ds.astype(np.float64))
            assert np.all(a_s >= exact * (1 - 2 ** -23))
            assert np.all(a_z >= np.abs(dz.astype(np.float64)) * (1 - 2 ** -23))
            assert np.all(a_s > exact)  # mixed signs: strictly larger here
    # a channel's scale does not change when another channel's values grow by orders of magnitude
    x2, g2 = x.clone(), g.clone()
    g2[:, 0] = (g[:, 0].float() * 1000).to(DT[dn])
    _, _, a_s1, _ = _run(oracle, dn, x, g, scale, torch.zeros(1))
    _, _, a_s2, _ = _run(oracle, dn, x2, g2, scale, torch.zeros(1))
    assert np.array_equal(a_s1[1:], a_s2[1:]) and a_s2[0] > 100 * a_s1[0]


def test_non_finite_terms(oracle):
    x = torch.tensor([1.0, float('nan'), 2.0, 3.0, 0.5, float('inf')]).view(2, 1, 3).expand(2, 2, 3).contiguous()
    g = torch.ones(2, 2, 3)
    g[1, 1, 0] = float('inf')
    ds, _, a_s, _ = _run(oracle, 'f32', x, g, torch.tensor([0.1, 0.2]), torch.zeros(1))
    assert not np.isfinite(ds).any() and not np.isfinite(a_s).any()


def test_per_tensor_has_one_entry(oracle):
    gen = torch.Generator().manual_seed(17)
    x = torch.randn(1, 1, 999, generator=gen)
    g = torch.randn(1, 1, 999, generator=gen)
    ds, dz, a_s, a_z = _run(oracle, 'f32', x, g, torch.tensor([0.02]), torch.zeros(1))
    assert a_s.shape == (1,) and a_z.shape == (1,)
    assert a_s[0] >= abs(float(ds[0])) and np.isfinite(a_s[0])
