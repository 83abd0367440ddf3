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


# ---- the row walk past 2^32 bytes -----------------------------------------------------------------------------------
# The row walk (csrc/bvq_row_walk.h) forms a row's base as row * cpr * vec in 64 bits and indexes the per-row outputs by
# the 64-bit row.  The smallest bfloat16 tensors whose row bases pass 2^32 bytes, one geometry each so that both forms of
# RowSlot::init are covered; x, g, y and dx together are about 17 GB.  Both calls stream more than the non-temporal
# threshold, their pieces less: the NT instantiations against the plain ones as well.

def _fill_randn(n, gen, std=1.0):
    """a bfloat16 device tensor of n elements, randn * std, filled in pieces"""
    t = torch.empty(n, device=DEV, dtype=torch.bfloat16)
    step = 1 << 27   # (a float32 randn of the whole tensor would need another 8.6 GB)
    for lo in range(0, n, step):
        m = min(step, n - lo)
        t[lo:lo + m] = (torch.randn(m, device=DEV, generator=gen) * std).to(torch.bfloat16)
    return t


def _seams(rows, row_bytes):
    """the first two rows, the two sides of byte offsets 2^31 and 2^32, and the last row"""
    a, b = 2 ** 31 // row_bytes, 2 ** 32 // row_bytes
    assert a * row_bytes == 2 ** 31 and b < rows - 1
    return [0, 1, a - 1, a, b - 1, b, rows - 1]


def test_row_shifted_walk_past_2_32_bytes():
    """the asymmetric per-token kernels, 8 bit, rows of 16384 bfloat16 (C = 2048: one workgroup per row), 2^17 + 5 rows,
    gradients arriving through scale and zero-point: the rows at the seams, with the ties and extrema of
    test_gpu_dynamic_act.plant among them, against the per-channel route (compare, with its derived deposit_ulps); the
    whole tensor, 2048 rows at a time, against the same wrappers bit for bit (rows are independent and the sum order is
    fixed by H)."""
    import test_gpu_dynamic_act as DA
    import test_gpu_group_walk as W
    from brevitas_amd import _native as nat
    from brevitas_amd.core.quant import _fused
    free, _ = torch.cuda.mem_get_info()
    if free < 40 << 30:
        pytest.skip('needs 40 GB of free device memory')
    h, rows, bits, ste, piece = 16384, 2 ** 17 + 5, 8, False, 2048
    assert rows * h * 2 > 2 ** 32
    qmax = 2.0 ** bits - 1
    seams = _seams(rows, h * 2)
    gen = torch.Generator(device=DEV).manual_seed(123460)
    x = _fill_randn(rows * h, gen, 0.02).view(rows, h)
    g = _fill_randn(rows * h, gen).view(rows, h)
    gscale = torch.randn(rows, device=DEV, generator=gen).to(x.dtype)
    gzp = (torch.randn(rows, device=DEV, generator=gen) * 0.01).to(x.dtype)
    xs = x[seams].cpu()
    DA.plant(xs[:6], 'bf16')
    xs[6, h - 1] = (xs[6].abs().max().float() * 1.25).to(xs.dtype)   # the last row's maximum on the tensor's last element
    x[seams] = xs.to(DEV)

    def run(xp, gp, gsp, gzpp):
        desc, thr_div = _fused.row_shifted_call(xp, qmax, 0.0, qmax, ste)
        assert nat.row_shifted_supported(desc, xp)
        y, scale, zp, stat = nat.row_shifted_fwd(desc, xp, 1e-10, thr_div)
        return y, scale, zp, stat, nat.row_shifted_bwd(desc, gp, xp, stat, gsp, gzpp, 1e-10, thr_div)

    y, scale, zp, stat, dx = run(x, g, gscale, gzp)
    xs, gr, gss, gzs = x[seams].contiguous(), g[seams].contiguous(), gscale[seams].contiguous(), gzp[seams].contiguous()
    got = (y[seams], scale[seams].view(-1, 1), zp[seams].view(-1, 1), dx[seams])
    worst = DA.compare(got, DA.per_channel_step(xs, bits, ste, gr, gss, gzs), xs, gr, h, bits, 'bf16', gss, gzs)
    print('ROW_SHIFTED_DEPOSIT_ULPS huge bf16 C=2048 rows=%d bits=%d ste=%d worst=%.3f' % (rows, bits, ste, worst))
    assert torch.equal(stat[:rows][seams].float(), xs.max(dim=1).values.float())
    assert torch.equal(stat[rows:][seams].float(), xs.min(dim=1).values.float())
    for lo in range(0, rows, piece):
        hi = min(lo + piece, rows)
        y1, s1, z1, st1, dx1 = run(x[lo:hi], g[lo:hi], gscale[lo:hi], gzp[lo:hi])
        where = 'piece at row %d' % lo
        assert W.bits_equal(y[lo:hi], y1) and W.bits_equal(scale[lo:hi], s1) and W.bits_equal(zp[lo:hi], z1), where
        assert W.bits_equal(stat[lo:hi], st1[:hi - lo]) and W.bits_equal(stat[rows + lo:rows + hi], st1[hi - lo:]), where
        assert W.bits_equal(dx[lo:hi], dx1), where


def test_weight_norm_walk_past_2_32_bytes():
    """the weight-norm kernels, rows of 1024 bfloat16 (C = 128: one wave per row, four rows per workgroup), 2^21 + 7
    rows, the L1 and then the L2 norm on the same tensors: the rows at the seams, which hold the planted rows of
    test_gpu_weight_norm.case, against the bars of weight_norm_ref; the whole tensor, 2^15 rows at a time, against the
    same wrappers bit for bit."""
    import test_gpu_group_walk as W
    import test_gpu_weight_norm as WN
    import weight_norm_ref as R
    from brevitas_amd import _native as nat
    free, _ = torch.cuda.mem_get_info()
    if free < 40 << 30:
        pytest.skip('needs 40 GB of free device memory')
    k, rows, piece = 1024, 2 ** 21 + 7, 2 ** 15
    assert rows * k * 2 > 2 ** 32
    seams = _seams(rows, k * 2)
    gen = torch.Generator(device=DEV).manual_seed(123461)
    v = _fill_randn(rows * k, gen, 0.02).view(rows, k)
    gy = _fill_randn(rows * k, gen).view(rows, k)
    vs = v[seams].cpu()
    vs[0] = 0.0
    vs[1] = 0.015625
    vs[2, 0] = (vs[2].float().abs().max() * 1.25).to(vs.dtype)
    vs[3, k - 1] = -(vs[3].float().abs().max() * 1.25).to(vs.dtype)
    vs[6, k - 1] = (vs[6].float().abs().max() * 1.25).to(vs.dtype)   # the last row's abs-max on the tensor's last element
    v[seams] = vs.to(DEV)
    absmax = torch.empty(rows, device=DEV)
    norm0 = {'l1': torch.empty(rows, device=DEV), 'l2': torch.empty(rows, device=DEV)}
    for lo in range(0, rows, piece):
        p = v[lo:lo + piece].double()
        absmax[lo:lo + piece] = p.abs().amax(1).float()
        norm0['l1'][lo:lo + piece] = p.abs().sum(1).float()
        norm0['l2'][lo:lo + piece] = torch.sqrt((p * p).sum(1)).float()
    del p
    s = torch.clamp_min(absmax, 1e-10) / WN.QMAX
    factor = 0.6 + 0.9 * torch.rand(rows, device=DEV, generator=gen)
    for norm in ('l1', 'l2'):
        gpar = torch.clamp_min(norm0[norm], 1e-10) * factor
        T = float((2.0 * (gpar / s).max()).float())
        gpar[seams[4]] = 3.0 * T * s[seams[4]]                     # capped
        gpar[seams[5]] = torch.tensor(T, device=DEV) * s[seams[5]]   # the tie, which goes to g
        kind = WN.kind_of(norm)

        def run(vp, gyp, sp, gp):
            desc = WN.desc_of(vp, norm, False)
            assert nat.weight_norm_supported(desc, kind, T, R.NORM_MIN, vp)
            y, n = nat.weight_norm_fwd(desc, kind, T, R.NORM_MIN, vp, sp, gp)
            return (y, n) + tuple(nat.weight_norm_bwd(desc, kind, T, R.NORM_MIN, gyp, vp, sp, gp, n))

        out = run(v, gy, s, gpar)
        c = dict(k=k, v=vs, s=s[seams].cpu(), g=gpar[seams].cpu(), gy=gy[seams].cpu(), T=T, dn='bf16', norm=norm,
                 clamp_ste=False, chunks=128, rows=len(seams))
        c.update({name: t[seams].cpu() for name, t in zip(WN.OUTPUTS, out)})
        c['ref'] = R.closed_forms(c['v'], c['s'], c['g'], c['gy'], c['n'], T, WN.QMAX, norm, False)
        WN.check_norm(c, 'WEIGHT_NORM huge n')
        WN.check_forward(c)
        WN.check_backward(c, 'WEIGHT_NORM huge bwd')
        for lo in range(0, rows, piece):
            hi = min(lo + piece, rows)
            part = run(v[lo:hi], gy[lo:hi], s[lo:hi], gpar[lo:hi])
            for name, a, b in zip(WN.OUTPUTS, out, part):
                assert W.bits_equal(a[lo:hi], b), '%s %s, piece at row %d' % (norm, name, lo)
        del out, part
