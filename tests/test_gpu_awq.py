"""AWQ on the device: the candidates kernel (csrc/bvq_group_awq.hip) against the composed route (torch.mul, the
quantizer's own sub-modules, torch.div) run on the CPU on the same bits; special groups, the reduction to the plain
group kernels, the composed route on the device, the whole search, the forced non-temporal build and graph capture.

The bar: y, scale and zero-point of every candidate are bit-equal to the composed route on the CPU (a NaN equals a NaN).
A candidate has no reduction beyond the group's butterflies, which are exact (maxima and minima), so there is no
tolerance.  The losses of the search are float32 matrix products of two back ends: relative 1e-4."""
import pytest
import torch

import brevitas_amd.config as config
from brevitas_amd import quant as Q
from brevitas_amd.graph import awq_candidates, awq_scale_weight
from test_awq_host import DT, search_inputs
from test_group_mse_host import same_bits
from test_gpu_group_walk import use_nt0  # noqa: F401  (fixture: the forced-NT build of the library)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ITEMSIZE = {'f32': 4, 'bf16': 2, 'f16': 2}
WINDOW_BYTES = 4 * 4 * 64 * 16   # one workgroup's window: waves x loads per wave x lanes x 16 bytes
dtypes = pytest.mark.parametrize('dn', ['f32', 'bf16', 'f16'])
sizes = pytest.mark.parametrize('g', [16, 32, 64, 128, 256])
kinds = pytest.mark.parametrize('kind', ['sym', 'asym'])


def quantizer(w, g, bits, kind):
    make = Q.Int8WeightPerGroupFloat if kind == 'sym' else Q.ShiftedUint8WeightPerGroupFloat
    return make(w, group_size=g, bit_width=bits).to(w.device)


@pytest.fixture
def fused_calls(monkeypatch):
    """the candidate counts of the launches of the kernel's wrapper, call by call"""
    from brevitas_amd import _native as nat
    calls = []
    real = nat.group_awq_fwd

    def counted(desc, x, table, *a, **k):
        calls.append(table.shape[0])
        return real(desc, x, table, *a, **k)
    monkeypatch.setattr(nat, 'group_awq_fwd', counted)
    return calls


def shapes_of(dn, g):
    """[R, K] where the column of a chunk can go wrong: one group per row; rows that wrap inside a wave load; a group
    count that is no multiple of the groups per load and a chunk count that is no multiple of the window; more than one
    workgroup's window, ending inside a load"""
    rows = WINDOW_BYTES // (3 * g * ITEMSIZE[dn]) + 2
    return [(4, g), (5, 3 * g), (7, 5 * g), (rows, 3 * g)]


def make_case(shape, dn, n, seed=123456):
    """a weight-sized normal tensor and n rows of column factors between 1/4 and 4, the first of them ones"""
    gen = torch.Generator().manual_seed(seed + shape[0] * 1000 + shape[1])
    w = (torch.randn(shape, generator=gen) * 0.05).to(DT[dn])
    table = torch.exp2(torch.rand(n, shape[1], generator=gen) * 4 - 2)
    table[0] = 1.0
    return w, table.to(DT[dn])


def both(w0, table, g, bits, kind):
    """-> (the candidates on the device, the composed route on the CPU)"""
    wd = torch.nn.Parameter(w0.to(DEV))
    got = awq_candidates(wd, table.to(DEV), quantizer(wd, g, bits, kind))
    wc = torch.nn.Parameter(w0.clone())
    want = awq_candidates(wc, table, quantizer(wc, g, bits, kind))
    return got, want


def assert_same(got, want, n, what):
    """the first n candidates of `want`"""
    for a, b, name in zip(got, want, ('y', 'scale', 'zero_point')):
        b = b[:n] if b.dim() == 4 or name == 'y' else b
        assert same_bits(a, b), (name, what)


# ---- the sweep -------------------------------------------------------------------------------------------------------

@sizes
@dtypes
@kinds
@pytest.mark.parametrize('bits', [4, 8])
def test_candidates_are_the_composed_route_on_the_cpu(kind, dn, g, bits, fused_calls):
    for shape in shapes_of(dn, g):
        w, table = make_case(shape, dn, 20)
        wc = torch.nn.Parameter(w.clone())
        want = awq_candidates(wc, table, quantizer(wc, g, bits, kind))     # once: a candidate depends on its row alone
        assert not fused_calls
        for n in (1, 3, 20):
            wd = torch.nn.Parameter(w.to(DEV))
            got = awq_candidates(wd, table[:n].to(DEV), quantizer(wd, g, bits, kind))
            assert fused_calls == [n], (shape, n)                          # one launch
            fused_calls.clear()
            assert got[0].shape == (n,) + shape and got[1].shape == (n, shape[0], shape[1] // g, 1)
            assert_same(got, want, n, (shape, n))
        assert not same_bits(want[0][1], want[0][0])                       # the factors matter


# ---- special groups --------------------------------------------------------------------------------------------------

@dtypes
@kinds
@pytest.mark.parametrize('g', [16, 64])
def test_special_groups(kind, dn, g, fused_calls):
    """an all-zero group, a group with a NaN, one with +inf and one with -inf, a column factor that drives the scaled
    weight to inf (and one that is inf itself), extrema tied across chunks"""
    shape = (9, 3 * g)
    w, table = make_case(shape, dn, 3)
    xg = w.reshape(-1, g)
    xg[1] = 0.0
    xg[3, 5] = float('nan')
    xg[5, 2] = float('inf')
    xg[7, g - 1] = -float('inf')
    m = (xg[9].abs().max().float() * 1.25).to(xg.dtype)
    xg[9, 1], xg[9, g - 2] = m, m            # the maximum twice, in two chunks
    xg[11, 0], xg[11, g - 1] = -m, -m        # the minimum twice
    w = xg.reshape(shape).clone()
    w[8, g + 3] = 2.0
    big = {'f16': 6.0e4, 'bf16': 3.0e38, 'f32': 3.0e38}[dn]
    table[1, g + 3] = big                    # 2 * big overflows: an infinite element of the scaled weight
    table[2, 2 * g + 1] = float('inf')
    got, want = both(w, table, g, 4, kind)
    assert fused_calls == [3]
    assert_same(got, want, 3, (kind, dn, g))
    y = want[0].float()
    assert bool(torch.isinf((w * table[1])[8, g + 3]))
    # the NaN group is NaN; the first group of candidate 0 is an ordinary one (the all-zero group is 0 / 0 in float16,
    # where the scale's lower bound of 1e-10 rounds to zero: both routes say NaN there)
    assert bool(torch.isnan(y[0].reshape(-1, g)[3]).all()) and bool(torch.isfinite(y[0, 0, :g]).all())


# ---- n = 1 with factors of one: the plain group kernels --------------------------------------------------------------

@sizes
@dtypes
@kinds
def test_ones_are_the_plain_group_kernels(kind, dn, g):
    from brevitas_amd import _native as nat
    from brevitas_amd.core.quant import _fused
    shape = shapes_of(dn, g)[2]
    w = make_case(shape, dn, 1)[0].to(DEV)
    shifted = kind == 'asym'
    qmin, qmax, thr = (0.0, 15.0, 15.0) if shifted else (-8.0, 7.0, 8.0)
    desc, thr_div = _fused.unit_call(w, g, shifted, thr, qmin, qmax, True)
    ones = torch.ones(1, shape[1], dtype=w.dtype, device=DEV)
    assert nat.group_awq_supported(desc, w, ones)
    y, scale, zp = nat.group_awq_fwd(desc, w, ones, 1e-10, thr_div)
    plain = nat.unit_fwd(nat.GROUP_SHIFTED if shifted else nat.GROUP_QUANT, desc, w, 1e-10, thr_div)
    assert same_bits(y[0], plain[0]) and same_bits(scale[0], plain[1])
    assert zp is None if not shifted else same_bits(zp[0], plain[2])


def test_candidates_past_4_gib():
    """33 candidates of a 128 MiB weight in one launch: the last one lies wholly behind 2^32 bytes of y"""
    from brevitas_amd import _native as nat
    from brevitas_amd.core.quant import _fused

    def on_device(a, b):   # (no NaN here; 128 MiB tensors are not brought to the host)
        a, b = a.contiguous().view(torch.int16), b.contiguous().view(torch.int16)
        return a.shape == b.shape and bool(torch.equal(a, b))
    r = k = 8192
    gen = torch.Generator(device=DEV).manual_seed(123456)
    w = (torch.randn(r, k, device=DEV, generator=gen) * 0.05).to(torch.bfloat16)
    table = torch.exp2(torch.rand(33, k, device=DEV, generator=gen) * 4 - 2).to(torch.bfloat16)
    desc, thr_div = _fused.unit_call(w, 128, True, 15.0, 0.0, 15.0, True)
    assert nat.group_awq_supported(desc, w, table)
    y, scale, zp = nat.group_awq_fwd(desc, w, table, 1e-10, thr_div)
    assert y.numel() * y.element_size() > 1 << 32 and (y[32].data_ptr() - y.data_ptr()) >= 1 << 32
    for i in (0, 31, 32):
        y1, s1, z1 = nat.group_awq_fwd(desc, w, table[i:i + 1], 1e-10, thr_div)
        assert on_device(y[i], y1[0]) and on_device(scale[i], s1[0]) and on_device(zp[i], z1[0]), i
    # and the single candidate against the composition at the plain kernel: mul, group_shifted_fwd, div
    plain = nat.group_shifted_fwd(desc, (w * table[32]).reshape(-1), 1e-10, thr_div)
    assert on_device(y[32], plain[0].view(r, k) / table[32]) and on_device(scale[32], plain[1])


def test_supported_refuses_what_the_kernel_does_not_cover():
    from brevitas_amd import _native as nat
    from brevitas_amd.core.quant import _fused
    w = torch.zeros(4, 96, dtype=torch.bfloat16, device=DEV)
    desc, _ = _fused.unit_call(w, 32, True, 15.0, 0.0, 15.0, True)
    ones = torch.ones(65, 96, dtype=torch.bfloat16, device=DEV)
    assert nat.group_awq_supported(desc, w, ones[:64]) and nat.group_awq_supported(desc, w, ones[:1])
    assert not nat.group_awq_supported(desc, w, ones)                       # 65 candidates
    assert not nat.group_awq_supported(desc, w, ones[:0])
    assert not nat.group_awq_supported(desc, w, ones[:2, :48].contiguous())  # K = 48: no whole groups of 32
    assert not nat.group_awq_supported(desc, w, ones[:2].float())
    off = torch.ones(2 * 96 + 8, dtype=torch.bfloat16, device=DEV)[1:2 * 96 + 1].view(2, 96)
    assert off.data_ptr() % 16 != 0 and not nat.group_awq_supported(desc, w, off)
    d17, _ = _fused.unit_call(w[:, :68], 17, True, 15.0, 0.0, 15.0, True)
    assert not nat.group_awq_supported(d17, w, ones[:1])                    # what the group entries refuse
    with pytest.raises(nat.BvqError, match='bvq_group_awq_fwd'):
        nat.group_awq_fwd(desc, w, off, 1e-10, 15.0)


# ---- the composed route on the device --------------------------------------------------------------------------------

@dtypes
@kinds
def test_composed_route_on_the_device(kind, dn, fused_calls, monkeypatch):
    """a misaligned table, or FUSED_PATHS off: no launch of the kernel, the same bits"""
    g, shape = 32, (7, 160)
    w, table = make_case(shape, dn, 3)
    wc = torch.nn.Parameter(w.clone())
    want = awq_candidates(wc, table, quantizer(wc, g, 4, kind))
    wd = torch.nn.Parameter(w.to(DEV))
    q = quantizer(wd, g, 4, kind)
    off = torch.empty(table.numel() + 8, dtype=table.dtype, device=DEV)[1:table.numel() + 1].view(table.shape)
    off.copy_(table)
    assert off.data_ptr() % 16 != 0
    assert_same(awq_candidates(wd, off, q), want, 3, 'misaligned table')
    assert not fused_calls
    monkeypatch.setattr(config, 'FUSED_PATHS', False)
    assert_same(awq_candidates(wd, table.to(DEV), q), want, 3, 'FUSED_PATHS off')
    assert not fused_calls
    monkeypatch.setattr(config, 'FUSED_PATHS', True)
    assert_same(awq_candidates(wd, table.to(DEV), q), want, 3, 'fused')
    assert fused_calls == [3]
    fused_calls.clear()
    monkeypatch.setattr(config, 'AWQ_CANDIDATE_BYTES', 2 * w.numel() * w.element_size())
    assert_same(awq_candidates(wd, table.to(DEV), q), want, 3, 'two candidates per launch')
    assert fused_calls == [2, 1]


# ---- the whole search ------------------------------------------------------------------------------------------------

@kinds
@pytest.mark.parametrize('dn', ['f32', 'bf16'])
def test_search_on_the_device_is_the_search_on_the_cpu(kind, dn, fused_calls):
    make = {'sym': Q.Int4WeightPerGroupFloat, 'asym': Q.ShiftedUint4WeightPerGroupFloat}[kind]
    w, h, am = search_inputs(DT[dn])
    want = awq_scale_weight(w, h, am, make(w, 32), n_grid=20)
    wd, hd, amd = search_inputs(DT[dn], DEV)
    got = awq_scale_weight(wd, hd, amd, make(wd, 32).to(DEV), n_grid=20)
    assert fused_calls == [20]
    print('kept %d (cpu %d)' % (got.index, want.index))
    assert got.index == want.index and got.index > 0
    for name in ('q', 'scale', 'zero_point', 'input_scale'):
        assert same_bits(getattr(got, name), getattr(want, name)), name
    torch.testing.assert_close(got.losses.cpu(), want.losses, rtol=1e-4, atol=0)


# ---- the forced non-temporal build, graph capture --------------------------------------------------------------------

@dtypes
@kinds
def test_forced_nt_build(kind, dn, use_nt0, fused_calls):
    g = 64
    shape = shapes_of(dn, g)[3]
    w, table = make_case(shape, dn, 3)
    use_nt0()
    got, want = both(w, table, g, 4, kind)
    assert fused_calls == [3]
    assert_same(got, want, 3, (kind, dn))


@kinds
def test_one_launch_captured_and_replayed(kind):
    from brevitas_amd import _native as nat
    from brevitas_amd.core.quant import _fused
    g, shape = 128, (33, 384)
    w0, table = make_case(shape, 'bf16', 5)
    w, table = w0.to(DEV), table.to(DEV)
    shifted = kind == 'asym'
    qmin, qmax, thr = (0.0, 15.0, 15.0) if shifted else (-8.0, 7.0, 8.0)
    desc, thr_div = _fused.unit_call(w, g, shifted, thr, qmin, qmax, True)

    def one():
        return nat.group_awq_fwd(desc, w, table, 1e-10, thr_div)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        one()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):     # a single stream: no parallel branches
        captured = one()
    with torch.no_grad():
        w.mul_(1.25)
    want = one()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(captured, want):
        assert (a is None and b is None) or same_bits(a, b)
