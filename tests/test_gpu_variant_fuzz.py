"""Seeded sweep of the kernels outside the main quantizer against the CPU oracle, at shapes chosen to reach every path
they have:
  * bvq_variant_fwd / bvq_variant_bwd (binary, clamped binary, ternary, decoupled, truncating quantizers);
  * bvq_fakequant_fwd_bounds / bvq_fakequant_bwd_bounds (the integer range read from device memory, and its gradient);
  * the straight-through element-wise ops (bvq_unary, bvq_scalar_clamp, bvq_tensor_clamp[_bwd],
    bvq_abs_binary_sign_grad_bwd).
Paths: rows shorter than one vector, ragged 16-bit rows, several rows per unit, rows cut into pieces, 512 channels,
more than 1024 partials per channel (the split two-stage combine), and views that start past a 16-byte boundary (the
element-wise kernels).  Inputs carry NaN, +-inf, +-0, values exactly at the clamp bounds and the ternary threshold,
and quotients exactly halfway between integers.  y and dx bit-exact; the reduced gradients within float32 summation
error of the oracle's double sums; a second run gives the same bits everywhere."""
import numpy as np
import pytest
import torch

import golden_util as G
from test_gpu_cabi import ndesc, to_np

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
DT = {'f32': torch.float32, 'bf16': torch.bfloat16, 'f16': torch.float16}
CODE = {'f32': 0, 'bf16': 1, 'f16': 2}
LIM = {'f32': 2e-4, 'bf16': 2e-2, 'f16': 5e-3}  # the form and limits of test_gpu_fuzz.py
KINDS = ['binary', 'clamped_binary', 'ternary', 'decoupled', 'trunc']

# (tag, outer, channels, inner, per-channel, x dtype or None, storage offset in elements)
SHAPES = [
    ('inner1', 300, 33, 1, True, None, 0),            # rows shorter than one vector: the element-wise variant kernel
    ('inner3', 64, 16, 3, True, None, 0),
    ('inner7', 17, 8, 7, True, None, 0),
    ('rows49', 64, 16, 49, True, 'bf16', 0),          # ragged 16-bit rows, 16-byte accesses
    ('rows196', 8, 32, 196, True, 'f16', 0),
    ('rows3136', 4, 8, 3136, True, 'bf16', 0),
    ('rpu', 300, 4, 16, True, None, 0),               # several rows per unit
    ('pieces', 2, 3, 9000, True, None, 0),            # rows cut into pieces
    ('pieces_long', 1, 2, 40000, True, None, 0),
    ('c512', 64, 512, 9, True, None, 0),
    ('c512_4', 96, 512, 4, True, None, 0),
    ('tensor', 5, 7, 3, False, None, 0),
    ('tensor_mid', 16, 64, 49, False, None, 0),       # one row of several pieces
    ('skew_t', 1, 1, 70001, False, None, 1),          # one element past a 16-byte boundary: element-wise
    ('skew_c', 8, 16, 64, True, None, 2),             # whole chunks per row but a misaligned start: element-wise
]
# per-tensor, more than 1024 partials in the one channel: the split two-stage combine of launch_channel_sums
BIG = [('big_f32', 1, 1, 1_150_003, False, 'f32', 0), ('big_bf16', 1, 1, 4_300_001, False, 'bf16', 0),
       ('big_f16', 1, 1, 4_300_001, False, 'f16', 0)]


@pytest.fixture(scope='module')
def nat_lib():
    from brevitas_amd import _native
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return _native


def _sums_close(got, want, dn, name):
    got = got.double().cpu().numpy().reshape(-1)
    want = np.asarray(want, dtype=np.float64).reshape(-1)
    assert got.shape == want.shape, name
    fin = np.isfinite(want)
    assert not np.isfinite(got[~fin]).any(), (name, 'a non-finite sum came out finite')
    mag = np.abs(want[fin]).max() if fin.any() else 0.0
    err = np.abs(got[fin] - want[fin])
    assert np.all(err <= LIM[dn] * (np.abs(want[fin]) + mag + 1.0)), (name, got[fin][:8], want[fin][:8])


def _bits(got, want, dn):
    """device tensor against an oracle array: the same bits, every NaN equal to every NaN (the oracle writes torch CPU's
    canonical 16-bit NaN, the device keeps the payload)"""
    return G.same_bits(to_np(got).reshape(-1), np.asarray(want).reshape(-1), dn)


def _eq(dn, got, want):
    """two arrays of oracle format: the same bits, every NaN equal to every NaN"""
    return G.same_bits(np.asarray(got).reshape(-1), np.asarray(want).reshape(-1), dn)


def _same(a, b):
    """same bits, NaN payloads included"""
    return np.array_equal(to_np(a).reshape(-1).view(np.uint8), to_np(b).reshape(-1).view(np.uint8))


def _on_device(t, offset):
    """t on the device as a view that starts `offset` elements into its storage"""
    flat = t.reshape(-1)
    buf = torch.zeros(flat.numel() + offset, dtype=t.dtype, device=DEV)
    buf[offset:] = flat.to(DEV)
    return buf[offset:]


def _scales(rng, n, dn, fine):
    """o * 2^-e (o odd < 8): exact in every dtype, so x can sit exactly at a bound or halfway between two grid points;
    `fine` adds a low bit to float32 scales (SCALAR_CAST then rounds them)"""
    v = rng.choice([1.0, 3.0, 5.0, 7.0], n) * 2.0 ** -rng.randint(2, 7, n)
    if fine and dn == 'f32':
        v = v * (1.0 + 2.0 ** -12)
    return torch.tensor(v, dtype=torch.float32).to(DT[dn])


def _inject(x32, vals, rng, frac, specials):
    """x32 [outer, ch, inner] float32; vals float64 [K, ch] (or [K, 1]) per-channel edge values; the ones the x dtype
    cannot hold become 0.  A fraction `frac` of the elements takes one of them, or NaN / +-inf / +-0"""
    outer, ch, inner = x32.shape
    extra = [0.0, -0.0] + ([float('nan'), float('inf'), -float('inf')] if specials else [])
    table = np.concatenate([vals, np.array(extra)[:, None].repeat(vals.shape[1], 1)], 0)
    n = x32.numel()
    pick = rng.rand(n) < frac
    idx = np.nonzero(pick)[0]
    k = rng.randint(table.shape[0], size=idx.size)
    c = (idx // inner) % ch if table.shape[1] > 1 else np.zeros_like(idx)
    flat = x32.reshape(-1).numpy()
    flat[idx] = table[k, c]
    return torch.from_numpy(flat.reshape(outer, ch, inner))


def _representable(v, dn):
    t = torch.tensor(v, dtype=torch.float64)
    r = t.to(DT[dn]).double()
    return torch.where(r == t, t, torch.zeros_like(t)).numpy()


# ---- variant kernels --------------------------------------------------------------------------------------------

def _variant_cases():
    rng = np.random.RandomState(20261015)
    out = []
    for i, (tag, outer, ch, inner, pc, dn_forced, off) in enumerate(SHAPES + BIG):
        for kind in KINDS:
            dn = dn_forced or ['f32', 'bf16', 'f16'][rng.randint(3)]
            ct = dn if (dn == 'f32' or rng.randint(2)) else 'f32'
            if kind == 'ternary':
                ct = 'f32'  # mask.float() promotes
            bits = int([2, 3, 4, 5, 8][rng.randint(5)])
            signed, narrow = int(rng.randint(2)), int(rng.randint(2))
            has_zp = kind in ('decoupled', 'trunc') and rng.randint(3) > 0
            out.append(dict(
                tag=tag, kind=kind, outer=outer, ch=ch, inner=inner, pc=pc, off=off, dn=dn, ct=ct,
                sdn=['f32', 'bf16', 'f16'][rng.randint(3)], zdn=['f32', 'bf16', 'f16'][rng.randint(3)],
                cast=int(rng.randint(2)), ste=int(rng.randint(2)), rm=int(rng.randint(5)), bits=bits, signed=signed,
                narrow=narrow, thr=float([0.5, 0.75, 0.25][rng.randint(3)]), ts=float([2.0, 4.0, 16.0][rng.randint(3)]),
                zp=float([1.0, -2.0, 3.0][rng.randint(3)]) if has_zp else None,
                pzp=float([-1.0, 2.0][rng.randint(2)]) if kind == 'decoupled' and rng.randint(2) else None,
                fine=bool(rng.randint(4) == 0), specials=bool(rng.randint(2)) and not tag.startswith('big'),
                seed=int(rng.randint(1 << 30))))  # (NaN / inf would leave the split combine's sums unchecked)
    return out


def _int_range(bits, signed, narrow):
    if signed:
        return -(2.0 ** (bits - 1)) + (1 if narrow else 0), 2.0 ** (bits - 1) - 1
    return 0.0, 2.0 ** bits - 1 - (1 if narrow else 0)


def _variant_inputs(c):
    rng = np.random.RandomState(c['seed'])
    gen = torch.Generator().manual_seed(c['seed'])
    outer, ch, inner = c['outer'], c['ch'], c['inner']
    nsc = ch if c['pc'] else 1
    s = _scales(rng, nsc, c['sdn'], c['fine'])
    ps = _scales(rng, nsc, c['sdn'], c['fine']) if c['kind'] == 'decoupled' else None
    qmin, qmax = _int_range(c['bits'], c['signed'], c['narrow'])
    grid = (ps if ps is not None else s).double().numpy()  # the quotient's divisor
    kind = c['kind']
    if kind in ('binary', 'clamped_binary', 'ternary'):
        amp = 1.5
    elif kind == 'decoupled':
        amp = max(abs(qmin), qmax) + 2.0
    else:
        amp = 2.0 ** c['bits'] * c['ts'] / 2
    sv = s.double().numpy()
    if kind == 'clamped_binary':
        cb = sv if c['pc'] else s.to(DT[c['dn']]).double().numpy()  # the bound as the comparisons see it
        vals = np.stack([cb, -cb])
    elif kind == 'ternary':
        thr = (torch.tensor(c['thr'], dtype=torch.float32) * s.float()).to(s.dtype)
        thr = thr.double().numpy() if c['pc'] else thr.to(DT[c['dn']]).double().numpy()
        vals = np.stack([thr, -thr])
    elif kind == 'decoupled':
        ks = np.array([-8.5, -2.5, -1.5, -0.5, 0.5, 1.5, 2.5, 7.5, qmin - 0.5, qmax + 0.5, qmin, qmax])
        vals = ks[:, None] * grid[None, :]
    else:
        m = np.arange(-40, 40, dtype=np.float64)
        vals = np.concatenate([m[:, None] * grid[None, :], (m[:16] + 0.5)[:, None] * grid[None, :]])
    vals = _representable(vals, c['dn'])
    x32 = torch.randn(outer, ch, inner, generator=gen) * amp
    x32 = x32 * torch.from_numpy(grid).float().view(1, -1, 1)
    x32 = _inject(x32, vals, rng, 0.08, c['specials'])
    x = x32.to(DT[c['dn']])
    g = torch.randn(outer, ch, inner, generator=gen).to(DT[c['ct']])
    zp = torch.tensor([c['zp']]).to(DT[c['zdn']]) if c['zp'] is not None else None
    pzp = torch.tensor([c['pzp']]).to(DT[c['zdn']]) if c['pzp'] is not None else None
    return x, g, s, ps, zp, pzp, qmin, qmax


def _np(t):
    return None if t is None else _from(t)


def _from(t):
    import oracle
    return oracle.from_torch(t.reshape(-1))[0]


@pytest.mark.parametrize('c', _variant_cases(), ids=lambda c: '%s-%s-%s-%s' % (c['kind'], c['tag'], c['dn'], c['ct']))
def test_variant_against_oracle(oracle, c):
    from brevitas_amd import _native as nat
    O = oracle
    x, g, s, ps, zp, pzp, qmin, qmax = _variant_inputs(c)
    kind = KINDS.index(c['kind'])
    od = O.VariantDesc(c['outer'], c['ch'], c['inner'], kind, CODE[c['dn']], CODE[c['ct']], CODE[c['sdn']],
                       CODE[c['zdn']], int(c['pc']), c['rm'], c['ste'], O.SCALAR_CAST if c['cast'] else O.SCALAR_OPMATH,
                       qmin, qmax, c['thr'], c['ts'])
    d = nat.VariantDesc()
    for f, _ in nat.VariantDesc._fields_:
        setattr(d, f, getattr(od, f))
    xn, gn = _from(x), _from(g)
    y_o = O.variant_fwd(od, xn, _from(s), _np(ps), _np(zp), _np(pzp))
    dx_o, ds_o, dp_o = O.variant_bwd(od, gn, xn, _from(s), _np(ps), _np(zp), _np(pzp))
    dev = lambda t: None if t is None else t.to(DEV)  # noqa: E731
    xd, gd = _on_device(x, c['off']), _on_device(g, c['off'])
    args = (dev(s), dev(ps), dev(zp), dev(pzp))
    need_dp = ps is not None
    runs = []
    for _ in range(2):
        y = nat.variant_fwd(d, xd, *args)
        dx, ds, dp = nat.variant_bwd(d, gd, xd, *args, need_dscale=True, need_dpre=need_dp)
        runs.append((y, dx, ds, dp))
    y, dx, ds, dp = runs[0]
    assert _bits(y, y_o, c['ct']), 'y'
    assert _bits(dx, dx_o, c['dn']), 'dx'
    _sums_close(ds, ds_o, c['ct'], 'dscale')
    if need_dp:
        _sums_close(dp, dp_o, c['ct'], 'dpre_scale')
    for a, b, name in zip(runs[0], runs[1], ('y', 'dx', 'dscale', 'dpre_scale')):
        assert (a is None) == (b is None) and (a is None or _same(a, b)), ('second run differs', name)


# ---- integer range read from the device (learned bit width) ---------------------------------------------------

def _bounds_cases():
    rng = np.random.RandomState(4100)
    out = []
    for tag, outer, ch, inner, pc, dn_forced, off in SHAPES + BIG:
        for rep in range(2):
            dn = dn_forced or ['f32', 'bf16', 'f16'][rng.randint(3)]
            out.append(dict(
                tag=tag, rep=rep, outer=outer, ch=ch, inner=inner, pc=pc, off=off, dn=dn,
                ct=dn if (dn == 'f32' or rng.randint(3)) else 'f32', rm=int(rng.randint(5)),
                ste=int(rng.randint(4) == 0), bits=int([2, 3, 4, 6, 8][rng.randint(5)]), signed=int(rng.randint(2)),
                narrow=int(rng.randint(2)), zp_kind=['zero', 'scalar', 'channel'][rng.randint(3)],
                specials=bool(rng.randint(2)) and not tag.startswith('big'), seed=int(rng.randint(1 << 30))))
    return out


@pytest.mark.parametrize('c', _bounds_cases(), ids=lambda c: '%s-%d-%s-%s' % (c['tag'], c['rep'], c['dn'], c['ct']))
def test_bounds_against_oracle(oracle, c):
    from brevitas_amd import _native as nat
    O = oracle
    rng = np.random.RandomState(c['seed'])
    gen = torch.Generator().manual_seed(c['seed'])
    outer, ch, inner, dn = c['outer'], c['ch'], c['inner'], c['dn']
    qmin, qmax = _int_range(c['bits'], c['signed'], c['narrow'])
    nsc = ch if c['pc'] else 1
    s = _scales(rng, nsc, dn, False)
    if c['zp_kind'] == 'zero':
        zp = torch.zeros(1)
    elif c['zp_kind'] == 'scalar':
        zp = torch.tensor([2.0])
    else:
        zp = torch.randint(-3, 4, (ch,)).float()
    zp_pc = c['zp_kind'] == 'channel' and ch > 1
    grid = s.double().numpy()
    ks = np.array([-2.5, -1.5, -0.5, 0.5, 1.5, 2.5, qmin - 0.5, qmax + 0.5, qmin - 1, qmax + 1, qmin, qmax])
    vals = _representable(ks[:, None] * grid[None, :], dn)
    x32 = torch.randn(outer, ch, inner, generator=gen) * (max(abs(qmin), qmax) + 2)
    x32 = x32 * torch.from_numpy(grid).float().view(1, -1, 1)
    x = _inject(x32, vals, rng, 0.08, c['specials']).to(DT[dn])
    g = torch.randn(outer, ch, inner, generator=gen).to(DT[c['ct']])
    pcs = c['pc'] and ch > 1
    od = O.make_desc(outer, ch, inner, CODE[dn], CODE[c['ct']], CODE[dn], O.F32, scale_per_channel=pcs,
                     zp_per_channel=zp_pc, qmin=qmin, qmax=qmax, round_mode=c['rm'], clamp_ste=bool(c['ste']))
    xn, gn, sn, zn = _from(x), _from(g), _from(s), zp.numpy().astype(np.float32)
    y_o, _ = O.fakequant_fwd(od, xn, sn, zn, want_codes=False)
    dx_o, ds_o, _ = O.fakequant_bwd(od, gn, xn, sn, zn)
    db_o = O.fakequant_bwd_bounds(od, gn, xn, sn, zn)
    # the descriptor's own range is NOT the one in force: the kernels must read `bounds`
    d = ndesc(nat, od)
    d.qmin = qmin + 1.0
    d.qmax = max(qmax - 1.0, d.qmin)
    bounds = torch.tensor([qmin, qmax], dtype=torch.float32, device=DEV)
    xd, gd = _on_device(x, c['off']), _on_device(g, c['off'])
    sd, zd = s.to(DEV), zp.to(DEV)
    need_db = not c['ste']  # a straight-through clamp gives the bounds no gradient (dbounds null)
    runs = []
    for _ in range(2):
        y = nat.fakequant_fwd_bounds(d, xd, sd, zd, bounds)
        dx, ds, db = nat.fakequant_bwd_bounds(d, gd, xd, sd, zd, bounds, need_db)
        runs.append((y, dx, ds, db))
    y, dx, ds, db = runs[0]
    assert _bits(y, y_o, c['ct']), 'y'
    assert _bits(dx, dx_o, c['dn']), 'dx'
    _sums_close(ds, ds_o, c['ct'], 'dscale')
    if need_db:
        assert db.shape == db_o.shape
        _sums_close(db[0], db_o[0], c['ct'], 'd(qmin)')
        _sums_close(db[1], db_o[1], c['ct'], 'd(qmax)')
        if not c['specials']:
            assert np.abs(db_o).max() > 0, 'the case must clip'
    for a, b, name in zip(runs[0], runs[1], ('y', 'dx', 'dscale', 'dbounds')):
        assert (a is None) == (b is None) and (a is None or _same(a, b)), ('second run differs', name)


# ---- straight-through element-wise ops --------------------------------------------------------------------------

SIZES = [1, 2, 7, 8, 9, 63, 64, 65, 1000, 4097, 65539, 2 ** 21 + 5]
OFFSETS = [0, 1, 2, 3]
OPS = ['round', 'floor', 'ceil', 'round_to_zero', 'dpu_round', 'binary_sign', 'ternary_sign', 'abs']
_BUF = {}


def _ste_buffers(dn):
    """one host / device pair of random inputs (x, g, lo, hi) per dtype, with NaN, +-inf, +-0 and halfway values;
    every case below is a view into them"""
    if dn not in _BUF:
        n = SIZES[-1] + OFFSETS[-1]
        rng = np.random.RandomState(77 + CODE[dn])
        gen = torch.Generator().manual_seed(77 + CODE[dn])
        x32 = torch.randn(1, 1, n, generator=gen) * 6
        half = np.arange(-20, 20) + 0.5
        vals = np.concatenate([half, [1.0, -1.0, 2.0, -3.0, 0.25, -0.75]])[:, None]
        x = _inject(x32, vals, rng, 0.1, True).reshape(-1).to(DT[dn])
        g = torch.randn(n, generator=gen).to(DT[dn])
        lo = (torch.randn(n, generator=gen) * 3 - 1).to(DT[dn])
        hi = (torch.randn(n, generator=gen) * 3 + 1).to(DT[dn])
        eq = torch.rand(n, generator=gen) < 0.1  # bounds equal to x
        lo = torch.where(eq, x, lo)
        hi = torch.where(torch.roll(eq, 1), x, hi)
        host = tuple(_from(t) for t in (x, g, lo, hi))
        _BUF[dn] = (host, tuple(t.to(DEV) for t in (x, g, lo, hi)))
    return _BUF[dn]


def _views(dn):
    host, devb = _ste_buffers(dn)
    for n in SIZES:
        for off in (OFFSETS if n < SIZES[-1] else OFFSETS[:2]):
            yield n, off, tuple(a[off:off + n] for a in host), tuple(t[off:off + n] for t in devb)


@pytest.mark.parametrize('op', OPS)
@pytest.mark.parametrize('dn', ['f32', 'bf16', 'f16'])
def test_unary_against_oracle(oracle, nat_lib, dn, op):
    k = OPS.index(op)
    for n, off, (xn, _, _, _), (xd, _, _, _) in _views(dn):
        assert _eq(dn, to_np(nat_lib.unary(k, xd)), oracle.unary(k, xn, CODE[dn])), (n, off)


@pytest.mark.parametrize('which', ['lo', 'hi', 'both'])
@pytest.mark.parametrize('dn', ['f32', 'bf16', 'f16'])
def test_scalar_clamp_against_oracle(oracle, nat_lib, dn, which):
    lo = -1.3 if which in ('lo', 'both') else None
    hi = 2.7 if which in ('hi', 'both') else None
    for n, off, (xn, _, _, _), (xd, _, _, _) in _views(dn):
        got = to_np(nat_lib.scalar_clamp(xd, lo, hi))
        assert _eq(dn, got, oracle.scalar_clamp(xn, CODE[dn], lo, hi)), (n, off)


@pytest.mark.parametrize('full', [False, True], ids=['one_element', 'bounds_full'])
@pytest.mark.parametrize('dn', ['f32', 'bf16', 'f16'])
def test_tensor_clamp_against_oracle(oracle, nat_lib, dn, full):
    for n, off, (xn, gn, lon, hin), (xd, gd, lod, hid) in _views(dn):
        if not full:  # one element each, one of them equal to an element of x
            lon, hin, lod, hid = xn[n // 2:n // 2 + 1], hin[:1], xd[n // 2:n // 2 + 1], hid[:1]
        y = to_np(nat_lib.tensor_clamp(xd, lod, hid))
        assert _eq(dn, y, oracle.tensor_clamp(xn, lon, hin, CODE[dn])), ('fwd', n, off)
        dx = to_np(nat_lib.tensor_clamp_bwd(gd, xd, lod, hid))
        assert _eq(dn, dx, oracle.tensor_clamp_bwd(gn, xn, lon, hin, CODE[dn])), ('bwd', n, off)


@pytest.mark.parametrize('dn', ['f32', 'bf16', 'f16'])
def test_abs_binary_sign_grad_bwd_against_oracle(oracle, nat_lib, dn):
    for n, off, (xn, gn, _, _), (xd, gd, _, _) in _views(dn):
        got = to_np(nat_lib.abs_binary_sign_grad_bwd(gd, xd))
        assert _eq(dn, got, oracle.abs_binary_sign_grad_bwd(gn, xn, CODE[dn])), (n, off)


@pytest.mark.parametrize('off', [0, 1])
@pytest.mark.parametrize('dn', ['bf16', 'f16'])
def test_every_16bit_pattern(oracle, nat_lib, dn, off):
    """all 65536 bit patterns of x through every op; clamp bounds that are equal to x (and NaN bounds)"""
    O, code = oracle, CODE[dn]
    pat = np.arange(1 << 16, dtype=np.uint32).astype(np.uint16)
    rng = np.random.RandomState(5 + off)
    xn = pat.copy()
    gn = rng.permutation(pat)
    lon, hin = np.roll(xn, 1), np.roll(xn, -7)
    eq = rng.rand(xn.size) < 0.25
    lon[eq] = xn[eq]
    hin[np.roll(eq, 3)] = xn[np.roll(eq, 3)]
    dev = lambda a: _on_device(O.to_torch(a, code), off)  # noqa: E731
    xd, gd, lod, hid = dev(xn), dev(gn), dev(lon), dev(hin)
    for k in range(len(OPS)):
        assert _eq(dn, to_np(nat_lib.unary(k, xd)), O.unary(k, xn, code)), OPS[k]
    one = O.to_float32(xn[12345:12346], code)[0]  # a bound that is one of the patterns
    for lo, hi in ((-1.5, None), (None, float(one)), (float(one), 3.0)):
        assert _eq(dn, to_np(nat_lib.scalar_clamp(xd, lo, hi)), O.scalar_clamp(xn, code, lo, hi)), (lo, hi)
    assert _eq(dn, to_np(nat_lib.tensor_clamp(xd, lod, hid)), O.tensor_clamp(xn, lon, hin, code))
    assert _eq(dn, to_np(nat_lib.tensor_clamp_bwd(gd, xd, lod, hid)), O.tensor_clamp_bwd(gn, xn, lon, hin, code))
    l1, h1 = xn[777:778], xn[40000:40001]
    assert _eq(dn, to_np(nat_lib.tensor_clamp(xd, dev(l1), dev(h1))), O.tensor_clamp(xn, l1, h1, code))
    assert _eq(dn, to_np(nat_lib.tensor_clamp_bwd(gd, xd, dev(l1), dev(h1))), O.tensor_clamp_bwd(gn, xn, l1, h1, code))
    assert _eq(dn, to_np(nat_lib.abs_binary_sign_grad_bwd(gd, xd)), O.abs_binary_sign_grad_bwd(gn, xn, code))
