"""What the batch-shard backward must produce, restated on the CPU (helper module: neither a conftest nor a test).

bvq_fakequant_bwd_shard turns one batch shard into dx without the deposit, a float64 [2][channels] message (row 0: the
shard's dscale sums kept in double, row 1: its claim on the channel's deposit) and the shard's first arg-max position per
channel; bvq_shard_unpack_deposit turns the gathered messages into the summed dscale and, on the owning shard, the
deposit.  Given the messages, ownership, position, the summed dscale and the deposited value are exact functions:
expect_message / expect_unpack / expect_deposit restate them with torch CPU ops and numpy, so a test needs no tolerance
there.  The library's decomposition (which route a shard takes, how long its float32 chains get) is the one restated in
test_gpu_grad_sums.py and is taken from there unchanged."""
import numpy as np
import torch

from test_gpu_grad_sums import (DT, U, _bwd_tiling, _cols_plan, _pick_vec, bits, check_sums, desc_pair,  # noqa: F401
                                inputs, np_of, placed, route, same_bits, seed_of)

NO_OWNER = 2.0 ** 30  # kShardNoOwner: a shard that holds no arg-max of the channel
PRE_NONE, PRE_RELU = 0, 1


def pre(x, pre_op):
    """the pre-op the statistic was taken through: torch.relu or nothing"""
    return torch.relu(x) if pre_op == PRE_RELU else x


def split_rows(outer, sizes):
    """the contiguous outer-slices of a [outer, C, inner] batch, one per shard (a size of 0: an empty shard)"""
    assert sum(sizes) == outer and all(s >= 0 for s in sizes), (outer, sizes)
    out, start = [], 0
    for s in sizes:
        out.append(slice(start, start + s))
        start += s
    return out


def one_launch(outer, channels, inner, dn, round_half_even=True):
    """does a shard of this shape take the one-launch form (bvq_fakequant_bwd_stats_onepass_supported and the vector
    width check at launch): row-mapped, full 16-byte accesses, half-even rounding"""
    el = 4 if dn == 'f32' else 2
    if route(outer, channels, inner, dn, True)['kind'] != 'row':
        return False
    return round_half_even and _pick_vec(16 // el, outer * channels, inner, 0, el) == 16 // el


def expect_message(x_shard, stat, rank, pre_op=PRE_NONE):
    """-> (first_pos int64 [C], claim float64 [C]) of a CPU shard [outer, C, inner]: first_pos[c] = the smallest
    shard-local o * inner + i with |pre(x)| == stat[c], else -1; claim[c] = rank, or 2^30.  NaN attains nothing."""
    outer, ch, inner = x_shard.shape
    n = outer * inner
    first = torch.full((ch,), -1, dtype=torch.int64)
    if n:
        a = pre(x_shard.float(), pre_op).abs().permute(1, 0, 2).reshape(ch, n)
        hit = a == stat.float().reshape(ch, 1)  # (== is false for every NaN)
        where = torch.where(hit, torch.arange(n).expand(ch, n), torch.full((ch, n), n)).amin(dim=1)
        first = torch.where(where < n, where, torch.full_like(where, -1))
    claim = torch.where(first >= 0, torch.full((ch,), float(rank), dtype=torch.float64),
                        torch.full((ch,), NO_OWNER, dtype=torch.float64))
    return first, claim


def expect_unpack(gathered, world):
    """gathered: float64 [world][2][C] (numpy, any shape of that size) -> (dscale_total float32 [C]: the shards' sums
    added in float64 in rank order from 0.0 and rounded once, owner int64 [C]: the lowest claim, -1 where nobody claims)"""
    m = np.asarray(gathered, dtype=np.float64).reshape(world, 2, -1)
    total = np.zeros(m.shape[2], dtype=np.float64)
    with np.errstate(all='ignore'):
        for r in range(world):
            total = total + m[r, 0]
        ds = total.astype(np.float32)
    low = m[:, 1].min(axis=0)
    owner = np.where(low == NO_OWNER, -1, low).astype(np.int64)
    return ds, owner


def expect_deposit(dx_before, x_shard, first_pos, owner, rank, dscale_total, scale_dtype, int_threshold, quot_dtype,
                   pre_op=PRE_NONE):
    """dx of shard `rank` after bvq_shard_unpack_deposit, from its dx before ([outer, C, inner], CPU), with the rounding
    points of shard_unpack_deposit_kernel: v = ds.to(scale_dtype); v = (v / thr).to(quot_dtype); g = v.to(x.dtype);
    term = g * sgn(pre(x[flat])) in x's dtype; dx[flat] = (dx[flat] + term) in float32, stored in x's dtype -- on the
    owning rank only, at first_pos; every other element is untouched."""
    outer, ch, inner = x_shard.shape
    dx = dx_before.clone()
    ds = torch.from_numpy(np.asarray(dscale_total, dtype=np.float32).copy())
    v = ds.to(scale_dtype)
    v = (v.float() / torch.tensor(float(int_threshold), dtype=torch.float32)).to(quot_dtype)  # one float32 quotient
    g = v.to(x_shard.dtype).float()
    for c in range(ch):
        p = int(first_pos[c])
        if int(owner[c]) != rank or p < 0:
            continue
        o, i = divmod(p, inner)
        sgn = torch.sign(pre(x_shard[o, c, i].float(), pre_op))  # sgn(0) = 0
        term = (g[c] * sgn).to(x_shard.dtype)
        dx[o, c, i] = (dx[o, c, i].float() + term.float()).to(x_shard.dtype)
    return dx


def same_bits64(a, b):
    """float64 / int64 tensors bit for bit, every NaN equal to every other"""
    a, b = a.detach().cpu(), b.detach().cpu()
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    if a.dtype == torch.int64:
        return bool((a == b).all())
    nan = torch.isnan(a) & torch.isnan(b)
    return bool(((a.view(torch.int64) == b.view(torch.int64)) | nan).all())


def changed(before, after):
    """bool mask of the elements whose bits differ (NaN to NaN is no change)"""
    before, after = before.detach().cpu(), after.detach().cpu()
    return (bits(before) != bits(after)) & ~(torch.isnan(before) & torch.isnan(after))
