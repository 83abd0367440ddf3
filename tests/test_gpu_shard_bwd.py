"""bvq_fakequant_bwd_shard and bvq_shard_unpack_deposit with 1 to 8 shards on every route of the message writer, in ONE
process on one device: the shard entry is called once per shard, the messages are stacked where the all-gather would put
them, and the unpack entry is called once per rank.  With the messages in hand nothing needs a tolerance: ownership,
position, the summed dscale and the deposited value are exact functions of the gathered messages (shard_util.py); only
the shards' float32 partial sums are held to the project's derived bound K * 2^-24 * sum |term| (test_gpu_grad_sums.py).

Inputs: inputs() of test_gpu_grad_sums.py, then, on M = 16.0 (exactly representable, above everything else):
  channel 0: +M at the very first element of the batch (shard 0);
  channel 3: -M in a shard that is not the first, then, where the batch has later elements, +M twice, once at the very
    end of the last shard: the owner is the first in batch order and the deposit's sign is negative (under RELU a -M
    does not attain: the first +M owns);
  channel 4 (C > 4): the maximum lives only in the last shard;
  channel 5 (C > 5): at the last element of the last row of a middle shard;
  channel 1 keeps the NaN of inputs(): its statistic is NaN, nobody claims it, nothing is deposited, its sum is
    non-finite; channel 2 keeps the inf in g.
The statistic is the batch's amax |pre(x)| in x's dtype, the scale clamp_min(stat, 1e-10) / thr in the same dtype.  The
quotients at and half-way past the clamp bounds are then planted again against that final scale -- those of them that
stay below the statistic (at it, in the channels that carry no plant: a few more ties, across shards too): the kernels
take the statistic to BE the batch's maximum, so an element above it would not be an input the step can produce.  (At
thr = 128 a +-M is itself the quotient +-128: exactly at the lower bound, clamped at the upper.)

Which writer a shard takes is the library's decision and leaves no trace in its outputs: that the table reaches all three
rests on the restated route() and one_launch() (tests/test_shard_bwd_host.py, test_shard_table_reaches_its_routes), not
on anything observed here -- the arrival buffer is checked whenever the one-launch form is switched on, taken or not."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from shard_util import (DT, PRE_NONE, PRE_RELU, changed, check_sums, desc_pair, expect_deposit, expect_message,
                        expect_unpack, inputs, np_of, placed, pre, route, same_bits, same_bits64, seed_of, split_rows)

DEV = 'cuda:0'
M = 16.0
ROUND, FLOOR = 0, 1


def _eq(n, k):
    return (n,) * k


# (name, full batch (outer, C, inner), dtypes, [(rows per shard, route of each shard or one for all)], round mode, pre-op)
TABLE = [
    # row-mapped, one launch: the last-arriving wave writes the message
    ('row_arrive', (24, 16, 196), ('f32', 'bf16', 'f16'),
     [((12, 12), 'row'), (_eq(8, 3), 'row'), ((5, 5, 5, 5, 4), 'row'), (_eq(3, 8), 'row'), ((23, 1), 'row')], ROUND, PRE_NONE),
    # row-mapped, several pieces per row
    ('row_pieces', (4, 4, 20000), ('f32', 'bf16'), [((2, 2), 'row'), (_eq(1, 4), 'row'), ((3, 1), 'row')], ROUND, PRE_NONE),
    # row-mapped, one element per lane (L = 15 refuses the column plan): two launches
    ('row_scalar', (40, 5, 3), ('f32', 'bf16'), [((20, 20), 'row'), (_eq(8, 5), 'row')], ROUND, PRE_NONE),
    # row-mapped, two launches: the one-launch form is half-even only
    ('row_floor', (24, 16, 196), ('bf16',), [(_eq(8, 3), 'row')], FLOOR, PRE_NONE),
    # column-mapped; the 1-row shard is row-mapped, so one gather mixes routes
    ('cols_inner1', (512, 16, 1), ('f32', 'bf16', 'f16'),
     [((256, 256), 'cols'), (_eq(64, 8), 'cols'), ((511, 1), ('cols', 'row'))], ROUND, PRE_NONE),
    ('cols_inner2', (256, 32, 2), ('f32', 'bf16'), [((128, 128), 'cols'), ((100, 100, 56), 'cols')], ROUND, PRE_NONE),
    ('cols_inner49', (128, 64, 49), ('bf16', 'f16'), [((64, 64), 'cols'), ((43, 43, 42), 'cols')], ROUND, PRE_NONE),
    # column-mapped at >= 64 rows, row-mapped at 24
    ('cols_ragged196', (192, 16, 196), ('bf16', 'f16'),
     [((128, 64), 'cols'), (_eq(64, 3), 'cols'), (_eq(24, 8), 'row')], ROUND, PRE_NONE),
    # column-mapped, 1025 partials per channel in the finish
    ('cols_split1025', (128, 8, 1025), ('bf16',), [((64, 64), 'cols')], ROUND, PRE_NONE),
    # column-mapped, two fold launches
    ('cols_fold2', (20000, 8, 2), ('bf16', 'f32'), [((10000, 10000), 'cols')], ROUND, PRE_NONE),
    # the deposit's sign and match are taken of relu(x)
    ('relu_row', (24, 16, 196), ('bf16',), [(_eq(8, 3), 'row')], ROUND, PRE_RELU),
    ('relu_cols', (512, 16, 1), ('bf16',), [(_eq(64, 8), 'cols')], ROUND, PRE_RELU),
]
ROWS = {r[0]: r for r in TABLE}


def kinds_of(sizes, kinds):
    return (kinds,) * len(sizes) if isinstance(kinds, str) else tuple(kinds)


def _split_id(sizes):
    return '+'.join(str(s) for s in sizes) if len(set(sizes)) > 1 or len(sizes) < 3 else '%dx%d' % (len(sizes), sizes[0])


CASES = [pytest.param(r[0], dn, sizes, id='%s-%s-%s' % (r[0], dn, _split_id(sizes)))
         for r in TABLE for dn in r[2] for sizes, _ in r[3]]
WORLD1 = [pytest.param(r[0], dn, id='%s-%s' % (r[0], dn)) for r in TABLE for dn in r[2]]


# ---- inputs ---------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=4)
def _base(name, dn):
    return inputs(ROWS[name][1], dn, True, seed=seed_of('shard_' + name))


def thr_of(dn):
    return 127.0 if dn == 'f32' else 128.0


def plants(shape, sizes):
    """{channel: [(row, i, value)]} of the module docstring, for a split into `sizes` rows per shard"""
    outer, ch, inner = shape
    live = [k for k, s in enumerate(sizes) if s > 0]
    start = [sum(sizes[:k]) for k in range(len(sizes))]
    last = lambda k: start[k] + sizes[k] - 1  # noqa: E731
    p = {0: [(0, 0, M)]}
    k1 = live[min(1, len(live) - 1)]
    neg = (start[k1], 0)
    end = (outer - 1, inner - 1)
    kmid = live[len(live) // 2]
    later = []  # after the -M in batch order: the very end of the last shard, and one more element
    for q in (end, (last(kmid), inner - 1), (start[k1], inner // 2)):
        if q > neg and q not in later and len(later) < 2:
            later.append(q)
    p[3] = [(neg[0], neg[1], -M)] + [(o, i, M) for o, i in later]
    p[4] = [(start[live[-1]] + sizes[live[-1]] // 2, inner // 2, M)]
    p[5] = [(last(kmid), inner - 1, M)]
    return {c: lst for c, lst in p.items() if c < ch}


def make_case(name, dn, sizes):
    """-> dict of CPU tensors: x, g [outer, C, inner], stat, scale [C] (x's dtype), the plants"""
    _, shape, _, _, round_mode, pre_op = ROWS[name]
    outer, ch, inner = shape
    dt = DT[dn]
    x, g, _ = _base(name, dn)
    x, g = x.clone(), g.clone()
    pl = plants(shape, sizes)
    taken = torch.zeros(shape, dtype=torch.bool)
    taken[0, 1, 0] = True  # the NaN of inputs()
    for c, lst in pl.items():
        for o, i, v in lst:
            x[o, c, i] = v
            taken[o, c, i] = True
    thr = thr_of(dn)
    stat = pre(x.float(), pre_op).abs().amax(dim=(0, 2)).to(dt)
    scale = torch.clamp_min(stat, 1e-10) / thr
    assert scale.dtype == dt
    # the clamp-bound quotients once more, against the final scale, where they leave the statistic the batch's maximum
    gen = torch.Generator().manual_seed(seed_of('replant_' + name))
    n = outer * inner
    idx = torch.randperm(n, generator=gen)[:max(8, n // 50)]
    o_i, i_i = idx // inner, idx % inner
    kinds = torch.tensor([127.0, -128.0, 127.5, -128.5, 5.5, -0.5])
    q = kinds[torch.arange(idx.numel()) % kinds.numel()]
    for c in range(ch):
        if not bool(torch.isfinite(stat[c])):
            continue
        v = (q * scale[c].float()).to(dt)
        mag = pre(v.float(), pre_op).abs()
        ok = (mag < stat[c].float()) if c in pl else (mag <= stat[c].float())
        ok &= ~taken[o_i, c, i_i]
        x[o_i[ok], c, i_i[ok]] = v[ok]
    again = pre(x.float(), pre_op).abs().amax(dim=(0, 2)).to(dt)
    assert same_bits(again, stat), 'the statistic is no longer the maximum of the batch'
    for c, lst in pl.items():
        assert float(stat[c]) == M and int((pre(x[:, c].float(), pre_op).abs() == M).sum()) == sum(
            1 for _, _, v in lst if v > 0 or pre_op != PRE_RELU), (c, lst)
    return dict(x=x, g=g, stat=stat, scale=scale, thr=thr, plants=pl, shape=shape, round_mode=round_mode, pre_op=pre_op,
                dn=dn)


def descs(nat, O, shard_shape, case):
    od, d, _ = desc_pair(nat, O, shard_shape, case['dn'], True, pre_op=case['pre_op'])
    od.round_mode = d.round_mode = case['round_mode']
    return od, d


# ---- the protocol on one device -------------------------------------------------------------------------------------

def shard_call(nat, d, g, x, scale, zp, stat, rank, onepass):
    """nat.fakequant_bwd_shard twice on the same buffers: the same bits both times; the arrival buffer handed back zero"""
    outs = []
    for _ in range(2):
        out = nat.fakequant_bwd_shard(d, g, x, scale, zp, stat, rank)
        assert out is not None
        torch.cuda.synchronize()
        outs.append([t.cpu() for t in out])
        if onepass:
            dev = torch.device(DEV)
            arr = nat.arrival_buffer(dev, nat.stream_ptr(dev), int(d.channels))
            assert arr is not None and not bool(arr.any()), 'the arrival buffer was not handed back as zeros'
    (dx, msg, pos), (dx2, msg2, pos2) = outs
    assert same_bits(dx, dx2) and same_bits64(msg, msg2) and same_bits64(pos, pos2), 'two calls, two results'
    return dx, msg, pos


def empty_shard_call(nat, d, scale, zp, stat, rank):
    """the C entry itself with outer = 0 and null tensors, message and positions pre-filled: 0.0 / 2^30 / -1"""
    ch = int(d.channels)
    dev = torch.device(DEV)
    msg = torch.full((2 * ch,), 7.0, dtype=torch.float64, device=dev)
    pos = torch.full((ch,), 5, dtype=torch.int64, device=dev)
    nat.check(nat.lib.bvq_fakequant_bwd_shard(ctypes.byref(d), None, None, nat.ptr(scale), nat.ptr(zp), nat.ptr(stat), None,
                                              nat.ptr(msg), nat.ptr(pos), rank, None, 0, None, 0, nat.stream_ptr(dev)),
              'bvq_fakequant_bwd_shard')
    torch.cuda.synchronize()
    msg, pos = msg.cpu(), pos.cpu()
    assert bool((msg[:ch] == 0.0).all()) and bool((msg[ch:] == 2.0 ** 30).all()) and bool((pos == -1).all()), (msg, pos)
    return msg, pos


def run_protocol(nat, O, case, sizes, empty_through_c=False):
    """steps 1 to 9 of one case, with the one-launch backward on and off"""
    outer, ch, inner = case['shape']
    dn, pre_op, thr = case['dn'], case['pre_op'], case['thr']
    dt = DT[dn]
    world = len(sizes)
    x, g, stat, scale = case['x'], case['g'], case['stat'], case['scale']
    zp = torch.zeros(1)
    sn, zn = np_of(scale), zp.numpy()
    rows = split_rows(outer, sizes)
    # the oracle, once per shard and once for the whole batch
    ref = []
    for r, sl in enumerate(rows):
        xs, gs = x[sl].contiguous(), g[sl].contiguous()
        so = sizes[r]
        if so == 0:
            ref.append(dict(x=xs, first=torch.full((ch,), -1, dtype=torch.int64),
                            claim=torch.full((ch,), 2.0 ** 30, dtype=torch.float64)))
            continue
        od, d = descs(nat, O, (so, ch, inner), case)
        dx_o, ds_o, _ = O.fakequant_bwd(od, np_of(gs), np_of(xs), sn, zn)
        a_s, _ = O.fakequant_bwd_abs(od, np_of(gs), np_of(xs), sn, zn)
        first, claim = expect_message(xs, stat, r, pre_op)
        ref.append(dict(x=xs, g=gs, d=d, dx=O.to_torch(dx_o, od.x_dtype).reshape(so, ch, inner), ds=ds_o, abs=a_s,
                        first=first, claim=claim, route=route(so, ch, inner, dn, True)))
    odf, _ = descs(nat, O, (outer, ch, inner), case)
    _, ds_full, _ = O.fakequant_bwd(odf, np_of(g), np_of(x), sn, zn)
    abs_full, _ = O.fakequant_bwd_abs(odf, np_of(g), np_of(x), sn, zn)
    k_max = max(rf['route']['K'] for rf in ref if 'route' in rf)
    assert not np.isfinite(ds_full[1]), 'the NaN channel has a finite oracle sum'
    sd, zd, std = scale.to(DEV), zp.to(DEV), stat.to(DEV)
    xd = [placed(rf['x'], 0) if sizes[r] else None for r, rf in enumerate(ref)]
    gd = [placed(rf['g'], 0) if sizes[r] else None for r, rf in enumerate(ref)]
    messages = {}
    was = nat.ONEPASS_BWD
    try:
        for onepass in (True, False):
            nat.ONEPASS_BWD = onepass
            dxs, msgs, poss = [], [], []
            for r, rf in enumerate(ref):
                if sizes[r] == 0:
                    assert empty_through_c
                    _, d0 = descs(nat, O, (0, ch, inner), case)
                    msg, pos = empty_shard_call(nat, d0, sd, zd, std, r)
                    dx = torch.empty(0, dtype=dt)
                else:
                    dx, msg, pos = shard_call(nat, rf['d'], gd[r], xd[r], sd, zd, std, r, onepass)
                    what = '%s rank %d of %d (%s route)' % (dn, r, world, rf['route']['kind'])
                    # 2: dx before the deposit is the oracle's
                    assert same_bits(dx, rf['dx'].reshape(-1)), what + ': dx before the deposit differs from the oracle'
                    # 3: positions and claims exactly
                    assert torch.equal(pos, rf['first']), (what, pos, rf['first'])
                    assert torch.equal(msg[ch:], rf['claim']), (what, msg[ch:], rf['claim'])
                    # 4: the shard's sums within the derived bound
                    check_sums(msg[:ch].numpy(), rf['ds'], rf['abs'], rf['route']['K'], what + ' message sums')
                dxs.append(dx), msgs.append(msg), poss.append(pos)
            messages[onepass] = msgs
            # 7: the gather, then the unpack on every rank
            gathered = torch.cat(msgs)
            ds_want, owner = expect_unpack(gathered.numpy(), world)
            gathered_d = gathered.to(DEV)
            moved = torch.zeros(ch, dtype=torch.int64)
            for r, rf in enumerate(ref):
                dxr = dxs[r].to(DEV)
                xr = xd[r] if sizes[r] else torch.empty(0, dtype=dt, device=DEV)
                ds = nat.shard_unpack_deposit(xr, dxr, gathered_d, world, ch, r, poss[r].to(DEV), inner, dt, thr, dt,
                                              pre_op, want_dscale=True)
                torch.cuda.synchronize()
                ds = ds.cpu()
                assert same_bits(ds, torch.from_numpy(ds_want)), ('dscale_total on rank %d' % r, ds, ds_want)
                if sizes[r] == 0:
                    assert not bool((owner == r).any())
                    continue
                # 8: the deposit, from the kernel's own dx and dscale_total
                before = dxs[r].reshape(sizes[r], ch, inner)
                want = expect_deposit(before, rf['x'], poss[r], owner, r, ds.numpy(), dt, thr, dt, pre_op)
                after = dxr.cpu().reshape(sizes[r], ch, inner)
                assert same_bits(after, want), 'rank %d of %d: dx after the deposit' % (r, world)
                moved += changed(before, after).sum(dim=(0, 2))
            assert int(moved.max()) <= 1 and int(moved[1]) == 0, moved
            # ownership: the first shard, in rank order, that attains
            for c, lst in case['plants'].items():
                firsts = [r for r, rf in enumerate(ref) if int(rf['first'][c]) >= 0]
                assert int(owner[c]) == firsts[0], (c, owner[c], firsts)
            assert int(owner[1]) == -1 and int(owner[0]) == min(r for r in range(world) if sizes[r])
            # 9: the total against the oracle's sums of the whole batch
            check_sums(ds_want, ds_full, abs_full, k_max, '%s dscale_total of %d shards' % (dn, world))
    finally:
        nat.ONEPASS_BWD = was
    # 5: both forms sum the same partials in channel_finish
    for a, b in zip(messages[True], messages[False]):
        assert same_bits64(a, b), 'the message differs between the one-launch and the two-launch form'


@pytest.mark.gpu
@pytest.mark.parametrize('name,dn,sizes', CASES)
def test_shards_on_one_device(oracle, name, dn, sizes):
    from brevitas_amd import _native as nat
    run_protocol(nat, oracle, make_case(name, dn, sizes), sizes)


@pytest.mark.gpu
@pytest.mark.parametrize('name,dn', WORLD1)
def test_world_one_equals_the_unsharded_entry(oracle, name, dn):
    """10: the whole batch as the only shard: shard + unpack give the dx and dscale of bvq_fakequant_bwd_stats"""
    from brevitas_amd import _native as nat
    case = make_case(name, dn, (ROWS[name][1][0],))
    outer, ch, inner = case['shape']
    dt, thr, pre_op = DT[dn], case['thr'], case['pre_op']
    _, d = descs(nat, oracle, case['shape'], case)
    xd, gd = placed(case['x'], 0), placed(case['g'], 0)
    sd, zd, std = case['scale'].to(DEV), torch.zeros(1, device=DEV), case['stat'].to(DEV)
    was = nat.ONEPASS_BWD
    try:
        for onepass in (True, False):
            nat.ONEPASS_BWD = onepass
            dx_w, ds_w = nat.fakequant_bwd_stats(d, gd, xd, sd, zd, std, dt, thr, dt, want_dscale=True)
            dx, msg, pos = nat.fakequant_bwd_shard(d, gd, xd, sd, zd, std, 0)
            ds = nat.shard_unpack_deposit(xd, dx, msg, 1, ch, 0, pos, inner, dt, thr, dt, pre_op, want_dscale=True)
            torch.cuda.synchronize()
            assert same_bits(ds, ds_w), (onepass, ds.cpu(), ds_w.cpu())
            assert same_bits(dx, dx_w), onepass
    finally:
        nat.ONEPASS_BWD = was


# ---- the empty shard ------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize('name', ['row_arrive', 'cols_inner1'])
def test_empty_shard_claims_nothing(oracle, name):
    """[0, half, half]: the empty shard at rank 0 goes through the C entry with outer = 0; ownership falls to rank 1"""
    from brevitas_amd import _native as nat
    outer = ROWS[name][1][0]
    sizes = (0, outer // 2, outer // 2)
    run_protocol(nat, oracle, make_case(name, 'bf16', sizes), sizes, empty_through_c=True)


# ---- refusals: no launch --------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_refusals(oracle):
    from brevitas_amd import _native as nat
    O = oracle
    dev = torch.device(DEV)
    shape = (4, 8, 16)
    outer, ch, inner = shape
    x = torch.randn(shape).to(torch.bfloat16).to(dev).reshape(-1)
    g = torch.randn(shape).to(torch.bfloat16).to(dev).reshape(-1)
    stat = torch.full((ch,), 4.0, dtype=torch.bfloat16, device=dev)
    scale, zp = stat / 128.0, torch.zeros(1, device=dev)
    dx = torch.full_like(x, 3.0)
    gathered = torch.zeros(2 * 2 * ch, dtype=torch.float64, device=dev)  # rank 0 claims every channel at position 0
    gathered[3 * ch:] = 2.0 ** 30
    pos = torch.zeros(ch, dtype=torch.int64, device=dev)
    bf = torch.bfloat16

    def unpack(world=2, rank=0, thr=128.0, pre_op=nat.PRE_NONE, gath=gathered):
        nat.shard_unpack_deposit(x, dx, gath, world, ch, rank, pos, inner, bf, thr, bf, pre_op)

    for kw in (dict(rank=2), dict(rank=-1), dict(world=0, gath=gathered[:0]), dict(thr=float('nan')),
               dict(pre_op=nat.PRE_SIGMOID), dict(pre_op=nat.PRE_TANH), dict(pre_op=7)):
        with pytest.raises(nat.BvqError):
            unpack(**kw)
    # (a negative world: the wrapper's own size check is in the way, so straight at the C entry)
    assert nat.lib.bvq_shard_unpack_deposit(nat.BF16, nat.ptr(x), nat.ptr(dx), nat.ptr(gathered), -1, ch, 0, nat.ptr(pos),
                                            inner, nat.BF16, 128.0, nat.BF16, nat.PRE_NONE, None, nat.stream_ptr(dev)) != 0
    torch.cuda.synchronize()
    assert bool((dx == 3.0).all()), 'a refused unpack wrote dx'
    # the shard entry: sigmoid / tanh descriptors and a negative rank, straight at the C entry
    wsb = int(nat.lib.bvq_fakequant_bwd_stats_workspace_bytes(ctypes.byref(desc_pair(nat, O, shape, 'bf16', True)[1])))
    assert wsb > 0
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    msg = torch.full((2 * ch,), 7.0, dtype=torch.float64, device=dev)
    fp = torch.full((ch,), 5, dtype=torch.int64, device=dev)
    for pre_op, rank in ((nat.PRE_SIGMOID, 0), (nat.PRE_TANH, 0), (nat.PRE_NONE, -1)):
        _, d, _ = desc_pair(nat, O, shape, 'bf16', True, pre_op=pre_op)
        rc = nat.lib.bvq_fakequant_bwd_shard(ctypes.byref(d), nat.ptr(g), nat.ptr(x), nat.ptr(scale), nat.ptr(zp),
                                             nat.ptr(stat), nat.ptr(dx), nat.ptr(msg), nat.ptr(fp), rank, nat.ptr(ws), wsb,
                                             None, 0, nat.stream_ptr(dev))
        assert rc != 0, (pre_op, rank)
        if pre_op != nat.PRE_NONE:
            assert nat.fakequant_bwd_shard(d, g, x, scale, zp, stat, 0) is None
    torch.cuda.synchronize()
    assert bool((msg == 7.0).all()) and bool((fp == 5).all()) and bool((dx == 3.0).all()), 'a refused call wrote'
    # a per-tensor descriptor, and a view one element past a 16-byte boundary: not covered
    _, dpt, _ = desc_pair(nat, O, shape, 'bf16', False)
    assert nat.fakequant_bwd_shard(dpt, g, x, scale[:1].contiguous(), zp, stat[:1].contiguous(), 0) is None
    _, d, _ = desc_pair(nat, O, shape, 'bf16', True)
    assert nat.fakequant_bwd_shard(d, placed(g.cpu(), 1), placed(x.cpu(), 1), scale, zp, stat, 0) is None
