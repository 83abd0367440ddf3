"""The one-launch statistic + quantizer for channels held by a cluster of workgroups (bvq_absmax_fakequant_cluster)
against the routes it replaces -- bvq_absmax_scale (one-launch and two-launch statistic) + bvq_fakequant_fwd: y, the
statistic, the scale and the running statistic identical bit for bit, every dtype, ReLU pre-op, with and without the
lower bound on the scale, first and later batches, an all-zero channel, NaN and inf, channel counts that do not divide
the number of clusters, row counts that do not divide the rows of a workgroup.  Also: the arrival words are zero after
every launch, the forced fallback (each workgroup reads its whole channel itself) gives the same bits, no fallback is
taken in a normal run, and the module step, the C++ node and a HIP-graph replay agree with the two-launch route."""

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
DT = {'f32': torch.float32, 'bf16': torch.bfloat16, 'f16': torch.float16}


def bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def arrival_is_clean(nat):
    torch.cuda.synchronize()
    return all(int(b.count_nonzero()) == 0 for b in nat._arrive.values())


def _desc(nat, x, outer, ch, inner, pre):
    code = nat.dtype_code(x.dtype)
    return nat.QuantDesc(outer, ch, inner, code, code, code, nat.F32, 1, 0, -128.0, 127.0, nat.ROUND, 0, 0,
                         nat.OUT_DEQUANT, pre)


def _two_launch(nat, x, outer, ch, inner, pre, min_val, run, first, onepass):
    flat = x.reshape(-1)
    nat.ONEPASS = onepass
    try:
        stat, scale = nat.absmax_scale(flat, outer, ch, inner, min_val, 128.0, x.dtype, pre, running=run,
                                       momentum=0.1, first_batch=first)
    finally:
        nat.ONEPASS = True
    zp = torch.zeros(1, device=DEV)
    y = nat.fakequant_fwd(_desc(nat, x, outer, ch, inner, pre), flat, scale, zp)
    return y, stat, scale


def _check_all(nat, x, outer, ch, inner, pres=(0, 1), min_vals=(1e-10, None), flags=0):
    flat = x.reshape(-1)
    fb = torch.zeros(1, dtype=torch.int32, device=DEV)
    for pre in pres:
        d = _desc(nat, x, outer, ch, inner, pre)
        for min_val in min_vals:
            run_c = torch.full((ch,), 2.0, device=DEV, dtype=x.dtype)
            run_1, run_2 = run_c.clone(), run_c.clone()
            for first in (True, False):
                got = nat.absmax_fakequant_cluster(d, flat, min_val, 128.0, x.dtype, run_c, 0.1, first, flags, fb)
                assert got is not None, (outer, ch, inner)
                sc, cc, yc = got
                for onepass, run in ((True, run_1), (False, run_2)):
                    y, stat, scale = _two_launch(nat, x, outer, ch, inner, pre, min_val, run, first, onepass)
                    what = (pre, min_val, first, onepass)
                    assert torch.equal(bits(yc), bits(y.reshape(-1))), ('y',) + what
                    assert torch.equal(bits(sc), bits(stat)), ('stat',) + what
                    assert torch.equal(bits(cc), bits(scale)), ('scale',) + what
                    assert torch.equal(bits(run_c), bits(run)), ('running',) + what
                assert arrival_is_clean(nat)
    return int(fb.item())


SHAPES = [  # (outer, channels, inner)
    (256, 512, 3136),   # the headline: 16 workgroups per channel, 16 clusters
    (32, 512, 3136),
    (256, 64, 3136),
    (256, 37, 3136),    # channels that do not divide the clusters
    (40, 24, 3136),     # 3 workgroups per channel, the last one with no slice for eight of its waves
    (130, 301, 392),    # rows that do not divide a workgroup's, channels that do not divide the clusters
    (24, 48, 784),
    (9, 5, 1000),
    (3, 7, 4096 + 64),  # rows of several slices
    (2, 3, 8),
]
FAST = {(256, 512, 3136): ('bf16',), (32, 512, 3136): ('bf16', 'f16'), (256, 64, 3136): ('f32', 'bf16')}


@pytest.mark.parametrize('dn', ['f32', 'bf16', 'f16'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_cluster_equals_statistic_plus_quantizer(dn, shape):
    from brevitas_amd import _native as nat
    if shape in FAST and dn not in FAST[shape]:
        pytest.skip('large shape: covered in the other dtypes')
    outer, ch, inner = shape
    torch.manual_seed(123456)
    x = (torch.randn(outer, ch, inner, device=DEV) * 3).to(DT[dn])
    x[0, 0, 0] = -0.0
    x[:, 1, :] = 0.0  # an all-zero channel: the lower bound on the scale decides
    big = outer * ch * inner > 50_000_000
    fallbacks = _check_all(nat, x, outer, ch, inner, pres=(0,) if big else (0, 1),
                           min_vals=(1e-10,) if big else (1e-10, None))
    assert fallbacks == 0


def test_cluster_propagates_nan_and_inf():
    from brevitas_amd import _native as nat
    torch.manual_seed(7)
    for dn in ('bf16', 'f32'):
        x = torch.randn(40, 24, 3136, device=DEV).to(DT[dn])
        x[3, 2, 100] = float('nan')
        x[39, 4, 3135] = float('-inf')
        x[17, 5, 8] = float('inf')
        assert _check_all(nat, x, 40, 24, 3136) == 0


@pytest.mark.parametrize('shape', [(256, 64, 3136), (130, 301, 392), (40, 24, 3136)],
                         ids=lambda s: 'x'.join(map(str, s)))
def test_forced_fallback_gives_the_same_bits(shape):
    from brevitas_amd import _native as nat
    outer, ch, inner = shape
    torch.manual_seed(99)
    x = (torch.randn(outer, ch, inner, device=DEV) * 3).to(torch.bfloat16)
    x[:, 1, :] = 0.0
    taken = _check_all(nat, x, outer, ch, inner, pres=(0, 1), min_vals=(1e-10,), flags=nat.CLUSTER_FORCE_FALLBACK)
    words = int(nat.lib.bvq_absmax_fakequant_cluster_supported(_desc(nat, x, outer, ch, inner, 0), x.data_ptr(),
                                                               x.data_ptr() + x.numel() * 2 + 4096))
    members = words // ch - 1
    # every workgroup of every channel fell back, in each of the 2 pre-ops x 2 batches
    assert taken == 4 * members * ch


def _module_steps(x, g, steps=3):
    from bench import build_quantizer
    q = build_quantizer(x.shape[1], True, torch.device(DEV))
    out = []
    for _ in range(steps):
        xi = x.clone().requires_grad_(True)
        y, scale = q(xi)[:2]
        y.backward(g)
        out.append((y.detach(), scale.detach(), xi.grad, q.scaling_impl.runtime_stats.running_stats.detach().clone()))
    return out


@pytest.mark.parametrize('cpp', [True, False], ids=['cpp_node', 'python'])
def test_module_steps_match_the_two_launch_route(cpp):
    from brevitas_amd import _native as nat
    from brevitas_amd import config
    torch.manual_seed(123456)
    x = torch.randn(32, 512, 56, 56, device=DEV, dtype=torch.bfloat16)
    g = torch.randn_like(x)
    saved = config.CPP_AUTOGRAD
    try:
        config.CPP_AUTOGRAD = cpp
        res = []
        for on in (True, False):
            nat.ONEPASS = nat.ONEPASS_BWD = on
            res.append(_module_steps(x, g))
    finally:
        nat.ONEPASS = nat.ONEPASS_BWD = True
        config.CPP_AUTOGRAD = saved
    for sa, sb in zip(*res):
        for ta, tb in zip(sa, sb):
            assert torch.equal(bits(ta), bits(tb))
    assert arrival_is_clean(nat)


def test_cpp_node_matches_the_python_function():
    from brevitas_amd import config
    torch.manual_seed(4321)
    x = torch.randn(40, 24, 56, 56, device=DEV, dtype=torch.bfloat16) * 2
    g = torch.randn_like(x)
    saved = config.CPP_AUTOGRAD
    try:
        config.CPP_AUTOGRAD = True
        a = _module_steps(x, g)
        config.CPP_AUTOGRAD = False
        b = _module_steps(x, g)
    finally:
        config.CPP_AUTOGRAD = saved
    for sa, sb in zip(a, b):
        for ta, tb in zip(sa, sb):
            assert torch.equal(bits(ta), bits(tb))


def test_graph_replay_of_the_step_gives_the_same_bits():
    from bench import build_quantizer
    from brevitas_amd import _native as nat
    torch.manual_seed(123456)
    x = torch.randn(32, 64, 56, 56, device=DEV, dtype=torch.bfloat16).requires_grad_(True)
    g = torch.randn_like(x)
    qa = build_quantizer(64, True, torch.device(DEV))
    qb = build_quantizer(64, True, torch.device(DEV))

    def step(q):
        x.grad = None
        y = q(x)[0]
        y.backward(g)
        return y, x.grad

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):  # warm-up on the capture stream: its arrival buffer exists before the capture
            step(qa)
            step(qb)
        assert any(key[1] == side.cuda_stream for key in nat._arrive)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        y_s, dx_s = step(qa)
    for trial in range(2):
        with torch.no_grad():
            x.mul_(1.25)
        graph.replay()
        torch.cuda.synchronize()
        got = (y_s.clone(), dx_s.clone())
        with torch.cuda.stream(side):
            y, dx = step(qb)
        torch.cuda.synchronize()
        assert torch.equal(bits(got[0]), bits(y)) and torch.equal(bits(got[1]), bits(dx)), trial
        ra = qa.scaling_impl.runtime_stats.running_stats
        rb = qb.scaling_impl.runtime_stats.running_stats
        assert torch.equal(bits(ra), bits(rb)), trial
    assert arrival_is_clean(nat)
