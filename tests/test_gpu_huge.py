"""More than 2^31 elements in one call (a 4.6 GB bf16 activation; MI355X has 288 GB): the statistic, forward and
backward index with 64-bit offsets end to end.  Checked against torch's reduction and against the library's
own results on the first and last slices quantized separately (those paths are pinned by the golden vectors)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.mark.parametrize('layout', ['per_tensor', 'per_channel'])
def test_more_than_2_31_elements(layout):
    from brevitas_amd import _native as nat
    free, _ = torch.cuda.mem_get_info()
    if free < 40 << 30:
        pytest.skip('needs 40 GB of free device memory')
    outer, ch, inner = 9, 64, 4_000_000  # 2.304e9 elements
    n = outer * ch * inner
    assert n > 2 ** 31
    dt = torch.bfloat16
    x = torch.empty(n, device=DEV, dtype=dt)
    blk = ch * inner
    gen = torch.Generator(device=DEV).manual_seed(123456)
    for o in range(outer):  # filled in pieces: a float32 randn of the whole tensor would need another 9 GB
        x[o * blk:(o + 1) * blk] = torch.randn(blk, device=DEV, generator=gen).to(dt)
    x[n - 5] = 9.5  # the maximum of the last channel sits in the very last elements
    g = torch.empty_like(x)
    for o in range(outer):
        g[o * blk:(o + 1) * blk] = torch.randn(blk, device=DEV, generator=gen).to(dt)
    pc = layout == 'per_channel'
    lay = (outer, ch, inner) if pc else (1, 1, n)
    stat = nat.stats(nat.STAT_ABSMAX, x, *lay)
    want = x.view(outer, ch, inner).abs().amax(dim=(0, 2)) if pc else x.abs().max().reshape(1)
    assert torch.equal(stat, want)
    assert stat[-1].item() == 9.5
    scale = (stat.float().clamp_min(1e-10) / 128.0).to(dt)
    zp = torch.zeros(1, device=DEV)
    code = nat.dtype_code(dt)
    d = nat.QuantDesc(*lay, code, code, code, 0, int(pc), 0, -128.0, 127.0, 0, 0, 0, 0)
    y = nat.fakequant_fwd(d, x, scale, zp)
    dx, ds, _ = nat.fakequant_bwd(d, g, x, scale, zp, True, False)[:3]
    # the same elements through calls that stay far below 2^31: first and last row of the last channel
    for lo in (0, n - inner):
        c = (lo // inner) % ch if pc else 0
        sub = nat.QuantDesc(1, 1, inner, code, code, code, 0, 0, 0, -128.0, 127.0, 0, 0, 0, 0)
        s1 = scale[c:c + 1].contiguous()
        y1 = nat.fakequant_fwd(sub, x[lo:lo + inner], s1, zp)
        dx1 = nat.fakequant_bwd(sub, g[lo:lo + inner], x[lo:lo + inner], s1, zp, False, False)[0]
        assert torch.equal(y[lo:lo + inner], y1) and torch.equal(dx[lo:lo + inner], dx1)
    # dscale of the last channel against float64 sums of the per-element terms over its rows, piecewise
    c = ch - 1 if pc else 0
    tot = 0.0
    for o in range(outer):
        for cc in ([c] if pc else range(ch)):
            lo = (o * ch + cc) * inner
            sub = nat.QuantDesc(1, 1, inner, code, code, code, 0, 0, 0, -128.0, 127.0, 0, 0, 0, 0)
            part = nat.fakequant_bwd(sub, g[lo:lo + inner], x[lo:lo + inner], scale[c:c + 1].contiguous(), zp, True,
                                     False)[1]
            tot += float(part.double().sum())
    got = float(ds[c])
    assert abs(got - tot) <= 1e-3 * max(1.0, abs(tot)), (got, tot)


def test_percentile_of_more_than_2_31_elements():
    """the radix select's counters and rank are 64-bit: the k-th smallest |x| of 2.3e9 values, verified by counting"""
    from brevitas_amd import _native as nat
    free, _ = torch.cuda.mem_get_info()
    if free < 40 << 30:
        pytest.skip('needs 40 GB of free device memory')
    n = 2_304_000_000
    x = torch.empty(n, device=DEV, dtype=torch.bfloat16)
    gen = torch.Generator(device=DEV).manual_seed(123457)
    step = 256_000_000
    for lo in range(0, n, step):
        x[lo:lo + step] = torch.randn(min(step, n - lo), device=DEV, generator=gen).to(torch.bfloat16)
    k = int(0.99999 * n + 0.5)
    v = nat.kth_value(x, k, 1, 1, n, True)
    below = at_most = 0
    for lo in range(0, n, step):
        a = x[lo:lo + step].abs()
        below += int((a < v).sum())
        at_most += int((a <= v).sum())
    assert below < k <= at_most, (below, k, at_most)


# ---- the sub-wave group walk past 2^32 bytes ------------------------------------------------------------------------
# The walk (csrc/bvq_group_walk.h) computes a wave's first chunk in 64 bits and everything inside its window in 32 bits.
# numel = 2^31 + 2^20 + 7 * 32 bfloat16 elements is the smallest size whose byte offsets pass 2^32, with a ragged last
# window; x, g, y and dx together are about 17 GB.

WALK_N = 2 ** 31 + 2 ** 20 + 7 * 32
WALK_G = 32
WALK_SLICE = 4096
# group-aligned slices checked against the CPU references: the first, the two that straddle element 2^30 and element 2^31
# (byte offsets 2^31 and 2^32), and the last
WALK_SLICES = (0, 2 ** 30 - WALK_SLICE // 2, 2 ** 31 - WALK_SLICE // 2, WALK_N - WALK_SLICE)
WALK_PIECE = 2 ** 25      # elements of the piecewise calls: below the non-temporal threshold in both directions


def _walk_inputs(seed):
    """x, g (bfloat16, device) filled with randn in pieces; the checked slices of x without abs-max ties"""
    from test_gpu_mx_quant import untie
    n, dt = WALK_N, torch.bfloat16
    gen = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.empty(n, device=DEV, dtype=dt)
    g = torch.empty(n, device=DEV, dtype=dt)
    step = 1 << 27   # (a float32 randn of the whole tensor would need another 8.6 GB)
    for t in (x, g):
        for lo in range(0, n, step):
            m = min(step, n - lo)
            t[lo:lo + m] = torch.randn(m, device=DEV, generator=gen).to(dt)
    for lo in WALK_SLICES:
        assert lo % WALK_G == 0 and lo + WALK_SLICE <= n
        x[lo:lo + WALK_SLICE] = untie(x[lo:lo + WALK_SLICE].cpu(), WALK_G).to(DEV)
    return x, g


def test_mx_walk_past_2_32_bytes():
    """MX e4m3, groups of 32, bfloat16: forward, backward, encoder and decoder in one call each over 2^31 + 2^20 + 224
    elements.  Slices at the seams against the numpy oracle, the float64 autograd bar and the numpy encoder; the whole
    tensor, piece by piece, against the same wrappers on 2^25 elements (groups are independent and the sums have a
    fixed order: bit for bit)."""
    import test_gpu_group_walk as W
    import test_mx_pack_host as P
    import test_mx_quant_host as H
    from brevitas_amd import _native as nat
    free, _ = torch.cuda.mem_get_info()
    if free < 40 << 30:
        pytest.skip('needs 40 GB of free device memory')
    n, gsz, fmt = WALK_N, WALK_G, nat.MX_E4M3
    assert n * 2 > 2 ** 32
    x, g = _walk_inputs(123458)
    gs = torch.randn(n // gsz, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    y, scale = nat.mx_quant_fwd(x, gsz, fmt, nat.MX_FLOOR)
    dx = nat.mx_quant_bwd(g, x, gs, gsz, fmt, nat.MX_FLOOR, True)
    codes, sbytes = nat.mx_encode(x, gsz, fmt, nat.MX_FLOOR)
    back = nat.mx_decode(codes, sbytes, gsz, fmt, x.dtype)
    worst = 0.0
    for lo in WALK_SLICES:
        hi, glo, ghi = lo + WALK_SLICE, lo // gsz, (lo + WALK_SLICE) // gsz
        xs, gr, gss = x[lo:hi].cpu(), g[lo:hi].cpu(), gs[glo:ghi].cpu()
        H.check_forward(y[lo:hi].cpu(), scale[glo:ghi].cpu(), H.oracle(xs, gsz, 'e4m3', 'floor'))
        worst = max(worst, H.assert_dx(dx[lo:hi].cpu(), xs, gr, gss, gsz, 'e4m3', 'floor', True, 'bf16'))
        want_codes, want_scale = P.numpy_encode(xs, gsz, 'e4m3', 'floor')
        P.assert_bytes(codes[lo:hi], want_codes, 'codes at element %d' % lo)           # one byte per element
        P.assert_bytes(sbytes[glo:ghi], want_scale, 'scale bytes at element %d' % lo)
    print('MX_QUANT_DEPOSIT_ULPS huge bf16 e4m3 floor g=%d ste=1 worst=%.3f' % (gsz, worst))
    assert W.bits_equal(back, y), 'decoded values differ from the forward'
    del back
    for lo in range(0, n, WALK_PIECE):
        hi = min(lo + WALK_PIECE, n)
        glo, ghi = lo // gsz, hi // gsz
        y1, s1 = nat.mx_quant_fwd(x[lo:hi], gsz, fmt, nat.MX_FLOOR)
        dx1 = nat.mx_quant_bwd(g[lo:hi], x[lo:hi], gs[glo:ghi], gsz, fmt, nat.MX_FLOOR, True)
        c1, b1 = nat.mx_encode(x[lo:hi], gsz, fmt, nat.MX_FLOOR)
        assert W.bits_equal(y[lo:hi], y1) and W.bits_equal(scale[glo:ghi], s1), 'forward, piece at element %d' % lo
        assert W.bits_equal(dx[lo:hi], dx1), 'backward, piece at element %d' % lo
        assert W.bits_equal(codes[lo:hi], c1) and W.bits_equal(sbytes[glo:ghi], b1), 'encoder, piece at element %d' % lo


def test_group_walk_past_2_32_bytes():
    """group-wise integer, 8 bit, groups of 32, bfloat16, over the same size: slices at the seams against the CPU oracle
    (y, scale) and the per-channel route on the regrouped slice (assert_dw with its derived deposit_ulps); the whole
    tensor, piece by piece, against the same wrappers on 2^25 elements."""
    import test_gpu_group_quant as GQ
    import test_gpu_group_walk as W
    free, _ = torch.cuda.mem_get_info()
    if free < 40 << 30:
        pytest.skip('needs 40 GB of free device memory')
    n, gsz, bits = WALK_N, WALK_G, 8
    x, g = _walk_inputs(123459)
    gs = torch.randn(n // gsz, device=DEV, generator=torch.Generator(device=DEV).manual_seed(6)).to(x.dtype)
    y, scale, dw = W.group_step(x, g, gs, gsz, bits, True)
    worst = 0.0
    for lo in WALK_SLICES:
        hi, glo, ghi = lo + WALK_SLICE, lo // gsz, (lo + WALK_SLICE) // gsz
        xs, gr = x[lo:hi].contiguous(), g[lo:hi].contiguous()
        W.check_group_forward(y[lo:hi].cpu(), scale[glo:ghi].cpu(), xs.cpu(), gr.cpu(), gsz, bits, True, 'bf16')
        y_r, scale_r, dw_r = GQ.per_channel_step(xs, gsz, bits, True, gr, gs[glo:ghi].contiguous())
        GQ.assert_same_bits(y[lo:hi], y_r, 'bf16', 'y at element %d' % lo)
        GQ.assert_same_bits(scale[glo:ghi], scale_r, 'bf16', 'scale at element %d' % lo)
        worst = max(worst, GQ.assert_dw(dw[lo:hi], dw_r, xs, gr, gsz, bits, 'bf16'))
    print('GROUP_QUANT_DEPOSIT_ULPS huge bf16 g=%d bits=%d ste=1 worst=%.3f' % (gsz, bits, worst))
    for lo in range(0, n, WALK_PIECE):
        hi = min(lo + WALK_PIECE, n)
        glo, ghi = lo // gsz, hi // gsz
        y1, s1, dw1 = W.group_step(x[lo:hi], g[lo:hi], gs[glo:ghi], gsz, bits, True)
        assert W.bits_equal(y[lo:hi], y1) and W.bits_equal(scale[glo:ghi], s1), 'forward, piece at element %d' % lo
        assert W.bits_equal(dw[lo:hi], dw1), 'backward, piece at element %d' % lo
