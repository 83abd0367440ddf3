"""The restatement of the batch-shard protocol (shard_util.py) checked on the CPU before any GPU test trusts it: against
the oracle's own pieces at world 1, against itself across world sizes, on a hand-written case, and the shape table of
test_gpu_shard_bwd.py against the restated route choice.

oracle.step_stats_scaled carries no deposit (its dx is the quantizer's alone: test_gpu_fullsize.py says so too), so the
world-1 check has two halves: the step's dx IS the dx the restatement starts from, bit for bit, and what the restatement
adds is what oracle.absmax_bwd -- the abs-max backward as autograd derives it, golden-tested -- adds for the same
statistic gradient."""
import numpy as np
import pytest
import torch

import oracle as O
from shard_util import (DT, NO_OWNER, PRE_RELU, _bwd_tiling, _pick_vec, changed, expect_deposit,
                        expect_message, expect_unpack, np_of, one_launch, route, same_bits, split_rows)

SHAPE = (6, 5, 12)
CODE = {'f32': O.F32, 'bf16': O.BF16, 'f16': O.F16}


@pytest.fixture(scope='module', autouse=True)
def _oracle_built():
    O.build()


def batch(dn):
    """a [6, 5, 12] batch: channel 2 holds a -/+ tie of its maximum (the -8 comes first), channel 4 a NaN"""
    gen = torch.Generator().manual_seed(61)
    x = (torch.randn(SHAPE, generator=gen) * 2).to(DT[dn])
    g = torch.randn(SHAPE, generator=gen).to(DT[dn])
    x[1, 2, 7], x[4, 2, 3] = -8.0, 8.0
    x[2, 4, 3] = float('nan')
    return x, g


def oracle_step(dn, x, g, thr):
    outer, ch, inner = x.shape
    od = O.make_desc(outer, ch, inner, CODE[dn], CODE[dn], CODE[dn], O.F32, scale_per_channel=True, qmin=-128.0,
                     qmax=127.0)
    return od, O.step_stats_scaled(od, np_of(x), np_of(g), 1e-10, thr)


def oracle_shard(dn, xs, gs, scale_n):
    outer, ch, inner = xs.shape
    od = O.make_desc(outer, ch, inner, CODE[dn], CODE[dn], CODE[dn], O.F32, scale_per_channel=True, qmin=-128.0,
                     qmax=127.0)
    dx, ds, _ = O.fakequant_bwd(od, np_of(gs), np_of(xs), scale_n, np.zeros(1, np.float32))
    return O.to_torch(dx, od.x_dtype).reshape(xs.shape), ds


def message(ds, claim):
    return np.concatenate([ds.astype(np.float64), claim.numpy()])


@pytest.mark.parametrize('dn', ['f32', 'bf16', 'f16'])
def test_world_one_reproduces_the_oracle(dn):
    dt = DT[dn]
    thr = 127.0 if dn == 'f32' else 128.0
    x, g = batch(dn)
    outer, ch, inner = SHAPE
    od, (_, dx_step, scale_n, stat32, _) = oracle_step(dn, x, g, thr)
    stat = torch.from_numpy(stat32).to(dt)
    dx_o, ds_o = oracle_shard(dn, x, g, scale_n)
    # the step's dx is the quantizer's alone
    assert same_bits(O.to_torch(dx_step, od.x_dtype).reshape(SHAPE), dx_o)
    first, claim = expect_message(x, stat, 0)
    assert int(first[2]) == 1 * inner + 7 and int(first[4]) == -1 and float(claim[4]) == NO_OWNER
    ds_total, owner = expect_unpack(message(ds_o, claim), 1)
    fin = np.isfinite(ds_o)
    assert np.array_equal(ds_total[fin].view(np.uint32), ds_o[fin].view(np.uint32)) and not np.isfinite(ds_total[~fin]).any()
    got = expect_deposit(dx_o, x, first, owner, 0, ds_total, dt, thr, dt)
    # the oracle's deposit: the statistic's gradient (the backward of scale = clamp_min(stat) / thr) through absmax_bwd
    gstat = (torch.from_numpy(ds_o).to(dt) / thr).to(dt)
    ab = O.to_torch(O.absmax_bwd(np_of(x), np_of(stat), np_of(gstat), CODE[dn], outer, ch, inner), CODE[dn]).reshape(SHAPE)
    want = torch.where(ab.float() != 0, (dx_o.float() + ab.float()).to(dt), dx_o)
    assert same_bits(got, want)
    moved = changed(dx_o, got).sum(dim=(0, 2))
    assert moved.tolist() == [1, 1, 1, 1, 0], moved  # one deposit per channel, none in the NaN channel
    assert bool(changed(dx_o, got)[1, 2, 7]) and not bool(changed(dx_o, got)[4, 2, 3])  # the first of the tie


@pytest.mark.parametrize('dn', ['f32', 'bf16', 'f16'])
def test_worlds_agree_on_element_owner_and_sum(dn):
    dt = DT[dn]
    thr = 127.0 if dn == 'f32' else 128.0
    x, g = batch(dn)
    outer, ch, inner = SHAPE
    _, (_, _, scale_n, stat32, _) = oracle_step(dn, x, g, thr)
    stat = torch.from_numpy(stat32).to(dt)
    first_full, _ = expect_message(x, stat, 0)
    landed = {}
    for world in (1, 2, 3, 6):
        rows = split_rows(outer, (outer // world,) * world)
        parts = []
        for r, sl in enumerate(rows):
            xs, gs = x[sl].contiguous(), g[sl].contiguous()
            dx_o, ds_o = oracle_shard(dn, xs, gs, scale_n)
            first, claim = expect_message(xs, stat, r)
            parts.append((xs, dx_o, first, message(ds_o, claim)))
        gathered = np.concatenate([p[3] for p in parts])
        per_rank = [expect_unpack(gathered.copy(), world) for _ in range(world)]
        ds_total, owner = per_rank[0]
        for ds_r, owner_r in per_rank:  # the same on every rank
            assert np.array_equal(ds_r.view(np.uint32), ds_total.view(np.uint32)) and np.array_equal(owner_r, owner)
        where = set()
        for r, (xs, dx_o, first, _) in enumerate(parts):
            got = expect_deposit(dx_o, xs, first, owner, r, ds_total, dt, thr, dt)
            for o, c, i in changed(dx_o, got).nonzero().tolist():
                where.add((rows[r].start + o, c, i))
                assert int(owner[c]) == r
        landed[world] = where
        for c in range(ch):  # the owner is the shard holding the first attaining element in batch order
            p = int(first_full[c])
            want = -1 if p < 0 else (p // inner) // (outer // world)
            assert int(owner[c]) == want, (world, c, owner[c], want)
    for world in (2, 3, 6):
        assert landed[world] == landed[1], (world, landed[world], landed[1])
    assert len(landed[1]) == 4 and (1, 2, 7) in landed[1]


def test_expect_message_by_hand():
    """two shards of [2, 4, 3]: channel 0 ties inside shard 0, channel 1 ties across the shards (-3 then +3), nobody
    attains channel 2's statistic, channel 3's statistic is zero (every zero attains it, -0.0 too)"""
    s0 = torch.tensor([[[1., 5., -5.], [0., 1., 2.], [1., 1., 1.], [-0., 0., 0.]],
                       [[5., 0., 0.], [2., -3., 0.], [1., 1., 1.], [0., 0., 0.]]])
    s1 = torch.tensor([[[4., 4., 4.], [0., 0., 0.], [2., 2., 2.], [0., 0., 0.]],
                       [[1., 1., 1.], [0., 0., 3.], [2., 2., 2.], [0., 0., 0.]]])
    stat = torch.tensor([5., 3., 9., 0.])
    f0, c0 = expect_message(s0, stat, 0)
    f1, c1 = expect_message(s1, stat, 1)
    assert f0.tolist() == [1, 4, -1, 0] and c0.tolist() == [0.0, 0.0, NO_OWNER, 0.0]
    assert f1.tolist() == [-1, 5, -1, 0] and c1.tolist() == [NO_OWNER, 1.0, NO_OWNER, 1.0]
    ds, owner = expect_unpack(np.concatenate([message(np.array([1, 2, 3, 4], np.float32), c0),
                                              message(np.array([.5, .5, .5, .5], np.float32), c1)]), 2)
    assert owner.tolist() == [0, 0, -1, 0] and ds.tolist() == [1.5, 2.5, 3.5, 4.5]
    # relu: a negative element attains nothing but a zero statistic; NaN attains nothing, not even a NaN statistic
    f, c = expect_message(torch.tensor([[[-3., 3.], [-1., float('nan')]]]), torch.tensor([3., float('nan')]), 2, PRE_RELU)
    assert f.tolist() == [1, -1] and c.tolist() == [2.0, NO_OWNER]
    # the deposit: sign of the owning element, sgn(0) = 0, the owner alone
    dx = torch.zeros(2, 4, 3)
    out = expect_deposit(dx, s0, f0, owner, 0, np.array([254., 127., 127., 127.], np.float32), torch.float32, 127.0,
                         torch.float32)
    assert out[0, 0, 1] == 2.0 and out[1, 1, 1] == -1.0 and int((out != 0).sum()) == 2
    assert not bool(expect_deposit(dx, s1, f1, owner, 1, np.ones(4, np.float32), torch.float32, 127.0,
                                   torch.float32).any())


def test_shard_table_reaches_its_routes():
    """every shard of every row, dtype and split of the GPU file's table takes the route the row names"""
    from test_gpu_shard_bwd import FLOOR, TABLE, kinds_of
    seen = set()
    for name, (outer, ch, inner), dts, splits, round_mode, pre_op in TABLE:
        assert outer * ch * inner <= 1_100_000, name
        for dn in dts:
            for sizes, kinds in splits:
                assert sum(sizes) == outer and 2 <= len(sizes) <= 8, (name, sizes)
                for so, kind in zip(sizes, kinds_of(sizes, kinds)):
                    r = route(so, ch, inner, dn, True)
                    assert r['kind'] == kind, (name, dn, sizes, so, r)
                    launches = 1 if one_launch(so, ch, inner, dn, round_mode != FLOOR) else 2
                    seen.add((kind, launches))
                    if name in ('row_arrive', 'relu_row'):
                        assert launches == 1, (name, dn, so)
                    if name in ('row_scalar', 'row_floor'):
                        assert launches == 2, (name, dn, so)
                    if name == 'row_pieces':
                        el = 4 if dn == 'f32' else 2
                        vec = _pick_vec(16 // el, so * ch, inner, 0, el)
                        _, ppr, _, nob = _bwd_tiling(so, ch, inner, vec)
                        assert ppr > 1 and nob >= 1 and launches == 1, (name, dn, so, ppr, nob)
                    if name == 'cols_split1025':
                        assert r['splits'] == 2 and inner > 1024, r
                    if name == 'cols_fold2':
                        assert r['folds'] == 2, r
                if not isinstance(kinds, str):
                    assert len(set(kinds)) > 1  # one gather mixes routes
    assert seen == {('row', 1), ('row', 2), ('cols', 2)}
