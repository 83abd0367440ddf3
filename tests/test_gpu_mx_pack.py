"""The MX wire format on the device: the one-kernel routes (bvq_mx_encode, bvq_mx_decode of csrc/bvq_mx_quant.hip)
against the composed route on the CPU and against the numpy encoder and code table of test_mx_pack_host.py; what the
encoder leaves untouched behind its outputs; the routes that refuse; graph capture.

Bars (test_mx_pack_host.py): codes and scale bytes are equal byte for byte; decoded values have the bits of the device
fake-quantizer's y (a NaN equals any NaN, an MXINT8 zero is compared by value).
"""
import functools

import numpy as np
import pytest
import torch

import test_mx_pack_host as P
import test_mx_quant_host as H
from test_mx_quant_host import DT, formats, rules

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
# the shapes of test_gpu_mx_quant.py -- less than a wave load, a ragged last wave, a group count that is no multiple of
# the groups per load ((7, 96) at g = 32 gives 504 FP6 code bytes, no multiple of 16), several workgroups, groups along
# the last dimension -- and 15 groups of 16: the scale bytes end inside a dword, and the 120 FP4 code bytes of float32
# inside 16 bytes
SHAPES = [((3, 64), 16, 'flat'), ((5, 512), 256, 'flat'), ((7, 96), 32, 'flat'), ((64, 4096), 128, 'flat'),
          ((2, 5, 64), 32, 'last'), ((3, 80), 16, 'flat'), ((9, 192), 64, 'flat')]   # and 27 ragged groups of 64
shapes = pytest.mark.parametrize('shape,g,axis', SHAPES, ids=['3x64-g16', '5x512-g256', '7x96-g32', '64x4096-g128',
                                                              '2x5x64-g32-last', '3x80-g16', '9x192-g64'])
dtypes = pytest.mark.parametrize('dn', ['f32', 'bf16', 'f16'])


@pytest.fixture
def fused_calls(monkeypatch):
    """counts the launches of the wire-format kernels' wrappers: [encode, decode]"""
    from brevitas_amd import _native as nat
    calls = [0, 0]
    real_enc, real_dec = nat.mx_encode, nat.mx_decode

    def enc(*a, **k):
        calls[0] += 1
        return real_enc(*a, **k)

    def dec(*a, **k):
        calls[1] += 1
        return real_dec(*a, **k)
    monkeypatch.setattr(nat, 'mx_encode', enc)
    monkeypatch.setattr(nat, 'mx_decode', dec)
    return calls


@functools.lru_cache(None)
def weight(shape, dn):
    """randn * 3 on the CPU, shared by the tests and left unchanged"""
    return H.make_weight(shape, dn)[0]


@functools.lru_cache(None)
def reference(shape, g, axis, dn, fmt, rule):
    """the composed route on the CPU and the numpy encoder, once per case"""
    x = weight(shape, dn)
    p = H.mx(fmt, g, rule, axis=axis).to_mx_codes(x)
    codes, scale = P.numpy_encode(x, g, fmt, rule)
    return p, codes, scale


def to_cpu(p):
    torch.cuda.synchronize()
    return p._replace(codes=p.codes.cpu(), scale_e8m0=p.scale_e8m0.cpu())


# ---- the fused encode and decode ------------------------------------------------------------------------------------

@shapes
@dtypes
@formats
@rules
def test_fused_encode_and_decode(shape, g, axis, dn, fmt, rule, fused_calls):
    x = weight(shape, dn)
    q = H.mx(fmt, g, rule, axis=axis).to(DEV)
    xd = x.to(DEV)
    pd = q.to_mx_codes(xd)
    assert fused_calls == [1, 0]
    p = to_cpu(pd)
    p_c, codes, scale = reference(shape, g, axis, dn, fmt, rule)
    assert p.codes.shape == p_c.codes.shape and p.scale_e8m0.shape == p_c.scale_e8m0.shape
    assert p[2:] == p_c[2:]
    P.assert_bytes(p.scale_e8m0, p_c.scale_e8m0.numpy(), 'scale bytes against the composed route')
    P.assert_bytes(p.codes, p_c.codes.numpy(), 'codes against the composed route')
    P.assert_bytes(p.scale_e8m0, scale, 'scale bytes against the numpy encoder')
    P.assert_bytes(p.codes, codes, 'codes against the numpy encoder')
    back = q.from_mx_codes(pd, DT[dn])
    assert fused_calls == [1, 1]
    y = q(xd)[0]
    P.assert_round_trip(back.cpu(), y.cpu(), fmt)


@shapes
@dtypes
@pytest.mark.parametrize('fmt', ['e4m3', 'e2m3', 'e2m1'])
def test_nothing_is_written_behind_the_outputs(shape, g, axis, dn, fmt):
    from brevitas_amd import _native as nat
    from brevitas_amd.core.quant.mx import MX_FORMATS
    x = weight(shape, dn)
    n = x.numel()
    nbytes, groups = n * P.BITS[fmt] // 8, n // g
    cbuf = torch.full((nbytes + 64,), 0xa5, dtype=torch.uint8, device=DEV)
    sbuf = torch.full((groups + 64,), 0xa5, dtype=torch.uint8, device=DEV)
    assert cbuf.data_ptr() % 16 == 0 and sbuf.data_ptr() % 16 == 0
    nat.mx_encode(x.to(DEV).reshape(-1), g, MX_FORMATS[fmt].code, nat.MX_FLOOR, codes=cbuf[:nbytes],
                  scale_e8m0=sbuf[:groups])
    torch.cuda.synchronize()
    cbuf, sbuf = cbuf.cpu(), sbuf.cpu()
    assert bool((cbuf[nbytes:] == 0xa5).all()), torch.nonzero(cbuf[nbytes:] != 0xa5).reshape(-1).tolist()
    assert bool((sbuf[groups:] == 0xa5).all()), torch.nonzero(sbuf[groups:] != 0xa5).reshape(-1).tolist()
    _, codes, scale = reference(shape, g, axis, dn, fmt, 'floor')
    P.assert_bytes(cbuf[:nbytes], codes, 'codes')
    P.assert_bytes(sbuf[:groups], scale, 'scale bytes')


@formats
@dtypes
@pytest.mark.parametrize('sb', P.SCALE_BYTES)
def test_every_code_decodes_to_the_table(fmt, dn, sb, fused_calls):
    cb, sc = P.every_code(fmt, sb)
    n = sc.size * 16
    got = H.mx(fmt, 16, axis='last').from_mx_codes(P.packed_of(cb, sc, fmt, 16, (n,), device=DEV), DT[dn])
    assert fused_calls == [0, 1]
    want = P.numpy_decode(cb, sc, 16, fmt, DT[dn])
    assert H.same_bits(got.cpu(), want), H.first_mismatch(got.cpu(), want)


# ---- edge groups, midpoints, every bfloat16 value -------------------------------------------------------------------

@formats
@rules
@dtypes
def test_edge_groups_midpoints_and_the_sweep(fmt, rule, dn, fused_calls):
    q = H.mx(fmt, 32, rule).to(DEV)
    for k, x in enumerate(P.sweep_inputs(fmt, dn)[1:]):
        xd = x.to(DEV)
        pd = q.to_mx_codes(xd)
        back = q.from_mx_codes(pd, DT[dn])
        assert fused_calls == [k + 1, k + 1]
        p = to_cpu(pd)
        codes, scale = P.numpy_encode(x, 32, fmt, rule)
        P.assert_bytes(p.scale_e8m0, scale, 'scale bytes')
        P.assert_bytes(p.codes, codes, 'codes')
        P.assert_round_trip(back.cpu(), q(xd)[0].cpu(), fmt)
    # the edge groups came last: a NaN and an Inf group are 0xFF over zero codes, the all-zero group keeps its signs
    assert p.scale_e8m0.reshape(-1).tolist()[1:3] == [255, 255] and int((p.scale_e8m0 == 255).sum()) == 2
    per_group = 32 * P.BITS[fmt] // 8
    assert not bool(p.codes.reshape(-1)[per_group:3 * per_group].any())
    assert bool(torch.isnan(back[1:3]).all()) and int(p.scale_e8m0.reshape(-1)[0]) == 1
    if fmt != 'int8':
        assert H.same_bits(back[0].cpu(), x[0])


# ---- the composed route on the device -------------------------------------------------------------------------------

@pytest.mark.parametrize('kind', ['fused_paths_off', 'g48', 'misaligned'])
@pytest.mark.parametrize('fmt', ['e4m3', 'e3m2', 'e2m1', 'int8'])
def test_the_composed_route_on_the_device(kind, fmt, fused_calls, monkeypatch):
    import brevitas_amd.config as config
    dn, g = 'bf16', 32
    gen = torch.Generator().manual_seed(7)
    if kind == 'g48':
        g = 48
    x = (torch.randn(8, 96, generator=gen) * 3).to(DT[dn])
    xd = x.to(DEV)
    q = H.mx(fmt, g).to(DEV)
    if kind == 'fused_paths_off':
        monkeypatch.setattr(config, 'FUSED_PATHS', False)
    elif kind == 'misaligned':       # a view starting 2 bytes off a 16-byte boundary
        base = torch.zeros(8 * 96 + 8, dtype=DT[dn], device=DEV)
        base[1:1 + 8 * 96] = xd.reshape(-1)
        xd = base[1:1 + 8 * 96].view(8, 96)
        assert xd.data_ptr() % 16 == 2 and xd.is_contiguous()
    pd = q.to_mx_codes(xd)
    if kind == 'misaligned':         # and packed bytes that start 2 bytes off
        cb = torch.zeros(pd.codes.numel() + 16, dtype=torch.uint8, device=DEV)
        cb[2:2 + pd.codes.numel()] = pd.codes.reshape(-1)
        pd = pd._replace(codes=cb[2:2 + pd.codes.numel()].view(pd.codes.shape))
        assert pd.codes.data_ptr() % 16 == 2
    back = q.from_mx_codes(pd, DT[dn])
    assert fused_calls == [0, 0]
    p = to_cpu(pd)
    p_c = H.mx(fmt, g).to_mx_codes(x)
    P.assert_bytes(p.codes, p_c.codes.numpy(), 'codes')
    P.assert_bytes(p.scale_e8m0, p_c.scale_e8m0.numpy(), 'scale bytes')
    codes, scale = P.numpy_encode(x, g, fmt, 'floor')
    P.assert_bytes(p.codes, codes, 'codes against the numpy encoder')
    P.assert_bytes(p.scale_e8m0, scale, 'scale bytes against the numpy encoder')
    assert H.same_bits(back.cpu(), H.mx(fmt, g).from_mx_codes(p_c, DT[dn]))
    P.assert_round_trip(back.cpu(), H.oracle(x, g, fmt, 'floor')['y'], fmt)


def test_packed_weight_of_a_layer_on_the_device(fused_calls):
    import brevitas_amd.quant as Q
    from brevitas_amd.nn import QuantLinear
    torch.manual_seed(0)
    lin = QuantLinear(128, 64, weight_quant=Q.MXFloat4e2m1Weight, dtype=torch.bfloat16).to(DEV)
    pd = lin.packed_weight()
    assert fused_calls == [1, 0]
    p = to_cpu(pd)
    codes, scale = P.numpy_encode(lin.weight.detach().cpu(), 32, 'e2m1', 'floor')
    assert tuple(p.codes.shape) == (64, 64) and tuple(p.scale_e8m0.shape) == (64, 4)
    P.assert_bytes(p.codes, codes, 'codes')
    P.assert_bytes(p.scale_e8m0, scale, 'scale bytes')


# ---- graph capture --------------------------------------------------------------------------------------------------

def test_encode_and_decode_in_a_graph(fused_calls):
    """one stream, no parallel branches: an encode + decode captured and replayed gives the eager bytes"""
    torch.manual_seed(123456)
    w = (torch.randn(32, 256, device=DEV) * 3).to(torch.bfloat16)
    q = H.mx('e2m3', 32).to(DEV)

    def one():
        p = q.to_mx_codes(w)
        return p.codes, p.scale_e8m0, q.from_mx_codes(p, torch.bfloat16)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            one()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        codes_s, scale_s, y_s = one()
    assert fused_calls == [4, 4]
    before = codes_s.clone()
    w.mul_(1.5).add_(0.01)  # new values in the captured input
    graph.replay()
    torch.cuda.synchronize()
    got = (codes_s.clone(), scale_s.clone(), y_s.clone())
    codes, scale, y = one()
    assert torch.equal(got[0], codes) and torch.equal(got[1], scale) and torch.equal(got[2], y)
    assert not torch.equal(before, codes)
    assert H.same_bits(y.cpu(), q(w)[0].cpu())
