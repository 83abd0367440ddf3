"""Every form of the cluster forward (bvq_absmax_fakequant_cluster_form: a persistent grid of clusters walking the
channels, one-shot with one workgroup per channel and member, and the library's own choice for the shape) against the
CPU oracle, bit for bit: y, the statistic, the scale and the running statistic.  The oracle computes statistic, scale
and y (oracle.step_stats_scaled); the running average is _RuntimeStats' own three torch ops on the oracle's statistic.
Every dtype and rounding mode, no pre-op and ReLU, channel counts below and not dividing the number of clusters, a last
member that is partly filled, 64 members (the cap), NaN and inf, the forced fallback on small tensors, two launches back
to back without a host synchronisation (arrival words asserted zero on the buffer itself), a HIP-graph replay.  The one
condition that is not bit equality: no fallback is taken unless it is forced -- equal bits would hide that failure."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
DT = {'f32': torch.float32, 'bf16': torch.bfloat16, 'f16': torch.float16}
MOMENTUM = 0.1


def _forms(nat):
    return (('walk', nat.CLUSTER_WALK), ('oneshot', nat.CLUSTER_ONESHOT), ('auto', nat.CLUSTER_AUTO))


def bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def _desc(nat, x, outer, ch, inner, pre, rm):
    code = nat.dtype_code(x.dtype)
    return nat.QuantDesc(outer, ch, inner, code, code, code, nat.F32, 1, 0, -128.0, 127.0, rm, 0, 0, nat.OUT_DEQUANT, pre)


def _expected(x, outer, ch, inner, pre, rm, min_val, run0, first):
    """(y, stat, scale, running) as CPU tensors of x's dtype, from the oracle"""
    import oracle as O
    xn, code = O.from_torch(x.reshape(-1))
    d = O.make_desc(outer, ch, inner, code, code, code, O.F32, scale_per_channel=True, qmin=-128.0, qmax=127.0,
                    round_mode=rm, pre_op=pre)
    y, _, scale, stat32, _ = O.step_stats_scaled(d, xn, np.zeros_like(xn), min_val, 128.0)
    stat = torch.from_numpy(stat32.copy()).to(x.dtype)  # exact: the statistic is a value of x's dtype
    run = run0.detach().cpu().clone()
    if first:  # B/core/stats/stats_wrapper.py:61-66
        run *= stat
    else:
        run *= (1 - MOMENTUM)
        run += MOMENTUM * stat
    return O.to_torch(y, code), stat, O.to_torch(scale, code), run


def _run(nat, form, x, outer, ch, inner, pre, rm, min_val, run, first, fb, flags=0):
    d = _desc(nat, x, outer, ch, inner, pre, rm)
    got = nat.absmax_fakequant_cluster(d, x.reshape(-1), min_val, 128.0, x.dtype, run, MOMENTUM, first, flags, fb,
                                       form=form)
    assert got is not None, (outer, ch, inner)
    return got


def _same(got, want, what, nan_payload=True):
    """bit equality; nan_payload=False: a NaN must meet a NaN, its payload is not compared (the oracle returns the
    statistic as float32, and neither its cast to x's dtype nor the CPU's running average defines a NaN's payload;
    y and the scale come from the oracle in x's dtype and are compared whole)"""
    got, want = got.detach().cpu().reshape(-1), want.reshape(-1)
    if not nan_payload:
        assert torch.equal(got.isnan(), want.isnan()), what
        got, want = got.nan_to_num(nan=0.0, posinf=float('inf'), neginf=float('-inf')), \
            want.nan_to_num(nan=0.0, posinf=float('inf'), neginf=float('-inf'))
    assert torch.equal(bits(got), bits(want)), what


def _arrival_words(nat):
    torch.cuda.synchronize()
    return sum(int(b.count_nonzero()) for b in nat._arrive.values())


def _check(nat, x, pres=(0, 1), rms=(0,), min_val=1e-10, firsts=(True, False), flags=0):
    """every form on x [outer, ch, inner] against the oracle -> fallbacks taken"""
    outer, ch, inner = x.shape
    fb = torch.zeros(1, dtype=torch.int32, device=DEV)
    for pre in pres:
        for rm in rms:
            for first in firsts:
                run0 = torch.full((ch,), 2.0, device=DEV, dtype=x.dtype)
                y, stat, scale, running = _expected(x, outer, ch, inner, pre, rm, min_val, run0, first)
                for name, form in _forms(nat):
                    run = run0.clone()
                    sc, cc, yc = _run(nat, form, x, outer, ch, inner, pre, rm, min_val, run, first, fb, flags)
                    what = (name, tuple(x.shape), str(x.dtype), pre, rm, first)
                    _same(yc, y, ('y',) + what)
                    _same(sc, stat, ('stat',) + what, nan_payload=False)
                    _same(cc, scale, ('scale',) + what)
                    _same(run, running, ('running',) + what, nan_payload=False)
                    assert _arrival_words(nat) == 0, what
    return int(fb.item())


def _randn(shape, dn, seed=123456, mul=3.0):
    torch.manual_seed(seed)
    x = (torch.randn(*shape, device=DEV) * mul).to(DT[dn])
    x[0, 0, 0] = -0.0
    x[:, 1, :] = 0.0  # an all-zero channel: the lower bound on the scale decides
    return x


@pytest.mark.parametrize('rm', [0, 1, 2, 3, 4], ids=['round', 'floor', 'ceil', 'to_zero', 'dpu'])
@pytest.mark.parametrize('dn', ['bf16', 'f16', 'f32'])
def test_every_form_dtype_and_rounding_mode_equals_the_oracle(dn, rm):
    """[40, 24, 3136]: 3 members, the last with a slice for 8 of its 16 waves; 24 channels, fewer than the clusters"""
    from brevitas_amd import _native as nat
    x = _randn((40, 24, 3136), dn)
    assert _check(nat, x, pres=(0, 1), rms=(rm,), firsts=(False,)) == 0


SHAPES = [
    (130, 301, 392),   # 9 members, the last partly filled; 301 channels: 5 rounds and a bit of 56 clusters
    (256, 37, 784),    # 16 members like the headline; 37 channels: one round and a bit of 32 clusters
    (1024, 5, 256),    # 64 members, the cap; 5 channels, more clusters than channels
    (3, 7, 4096 + 64),  # rows of several slices
    (2, 3, 8),
]


@pytest.mark.parametrize('dn', ['bf16', 'f16', 'f32'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_every_form_and_shape_equals_the_oracle(dn, shape):
    from brevitas_amd import _native as nat
    x = _randn(shape, dn)
    assert _check(nat, x, pres=(0, 1), min_val=1e-10 if dn != 'f32' else 1e-3) == 0


def test_nan_and_inf():
    from brevitas_amd import _native as nat
    for dn in ('bf16', 'f16', 'f32'):
        x = _randn((40, 24, 3136), dn, seed=7, mul=1.0)
        x[3, 2, 100] = float('nan')
        x[39, 4, 3135] = float('-inf')
        x[17, 5, 8] = float('inf')
        assert _check(nat, x, firsts=(False,)) == 0


@pytest.mark.parametrize('shape', [(40, 24, 784), (130, 31, 392), (1024, 3, 64)], ids=lambda s: 'x'.join(map(str, s)))
def test_forced_fallback_gives_the_same_bits(shape):
    """small tensors only: on the fallback every workgroup reads its whole channel"""
    from brevitas_amd import _native as nat
    x = _randn(shape, 'bf16', seed=99)
    assert x.numel() * 2 < 4 << 20
    taken = _check(nat, x, pres=(0, 1), firsts=(False,), flags=nat.CLUSTER_FORCE_FALLBACK)
    members = (shape[0] + 15) // 16  # rows of one slice here
    assert taken == 2 * len(_forms(nat)) * members * shape[1]  # every workgroup of every channel, 2 pre-ops, every form


def test_two_launches_back_to_back_hand_the_words_back():
    """no host synchronisation between two launches on one stream: the second starts from the zeros the first left"""
    from brevitas_amd import _native as nat
    xa = _randn((130, 301, 392), 'bf16', seed=1)
    xb = _randn((130, 301, 392), 'bf16', seed=2)
    fb = torch.zeros(1, dtype=torch.int32, device=DEV)
    run0 = torch.full((301,), 2.0, device=DEV, dtype=torch.bfloat16)
    want = [_expected(x, 130, 301, 392, 0, 0, 1e-10, run0, False) for x in (xa, xb)]
    for name, form in _forms(nat):
        runs = [run0.clone(), run0.clone()]
        torch.cuda.synchronize()
        got = [_run(nat, form, x, 130, 301, 392, 0, 0, 1e-10, run, False, fb) for x, run in zip((xa, xb), runs)]
        torch.cuda.synchronize()
        assert nat._arrive and all(int(buf.count_nonzero()) == 0 for buf in nat._arrive.values()), name
        for (sc, cc, yc), run, (y, stat, scale, running) in zip(got, runs, want):
            _same(yc, y, ('y', name))
            _same(sc, stat, ('stat', name))
            _same(cc, scale, ('scale', name))
            _same(run, running, ('running', name))
    assert int(fb.item()) == 0


def test_graph_replay_gives_the_same_bits():
    from brevitas_amd import _native as nat
    shape = (130, 61, 392)
    x = _randn(shape, 'bf16', seed=5)
    fb = torch.zeros(1, dtype=torch.int32, device=DEV)
    run0 = torch.full((shape[1],), 2.0, device=DEV, dtype=torch.bfloat16)
    for name, form in _forms(nat):
        run = run0.clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):  # warm-up on the capture stream: its arrival buffer exists before the capture
            _run(nat, form, x, *shape, 0, 0, 1e-10, run, False, fb)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            sc, cc, yc = _run(nat, form, x, *shape, 0, 0, 1e-10, run, False, fb)
        for trial in range(2):
            with torch.no_grad():
                x.mul_(1.25)
                run.copy_(run0)
            y, stat, scale, running = _expected(x, *shape, 0, 0, 1e-10, run0, False)
            graph.replay()
            torch.cuda.synchronize()
            _same(yc, y, ('y', name, trial))
            _same(sc, stat, ('stat', name, trial))
            _same(cc, scale, ('scale', name, trial))
            _same(run, running, ('running', name, trial))
            assert _arrival_words(nat) == 0, (name, trial)
    assert int(fb.item()) == 0
