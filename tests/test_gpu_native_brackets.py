"""What bench.py's KernelTimer sees of the ctypes binding: every wrapper of brevitas_amd._native that brackets its
C-ABI call runs once under a recording timer, and the recorded names are held against the table below (a name typed
wrongly in a bracket drops that kernel from the benchmark's breakdown without failing anything else).  The names are
not always the entry's: the abs-max entries are 'bvq_stats', the cluster forward is 'bvq_stats_fakequant_fwd', every
backward form of the stats-scaled and learned-scale graphs is 'bvq_fakequant_bwd'.  And the device guard: a call on a
tensor of a device that is not current runs there and leaves the current device alone."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
OUTER, CH, INNER = 4, 8, 256   # bfloat16: covered by the one-launch statistic, forward and backward
GROUPS, GSIZE = 64, 32


class _Recorder:
    def __init__(self):
        self.names = []

    def before(self, name):
        self.names.append(('before', name))

    def after(self, name):
        self.names.append(('after', name))


def _bits(t):
    return t.detach().contiguous().reshape(-1).view(torch.uint8)


def _cases(nat):
    """-> [(label, callable, names expected of one call)]"""
    torch.manual_seed(20251)
    dt = torch.bfloat16
    code = nat.dtype_code(dt)
    x = torch.randn(OUTER * CH * INNER, device=DEV).to(dt)
    g = torch.randn(OUTER * CH * INNER, device=DEV).to(dt)
    zp = torch.zeros(1, device=DEV)
    d = nat.QuantDesc(OUTER, CH, INNER, code, code, code, nat.F32, 1, 0, -128.0, 127.0, 0, 0, 0, nat.OUT_DEQUANT, 0)
    assert nat.lib.bvq_absmax_onepass_supported(code, x.data_ptr(), OUTER, CH, INNER)
    stat, scale = nat.absmax_scale(x, OUTER, CH, INNER, 1e-10, 128.0, dt)
    run = torch.ones(CH, device=DEV, dtype=dt)
    value = torch.full((CH,), 0.5, device=DEV, dtype=dt)
    gd = nat.QuantDesc(1, GROUPS, GSIZE, code, code, code, nat.F32, 1, 0, -8.0, 7.0, 0, 0, 0, nat.OUT_DEQUANT, 0)
    xg, gg = x[:GROUPS * GSIZE].contiguous(), g[:GROUPS * GSIZE].contiguous()
    assert nat.group_quant_supported(gd, xg) and nat.mx_quant_supported(xg, GSIZE, nat.MX_E4M3)
    _, gscale, gstat = nat.group_quant_fwd(gd, xg, 1e-10, 7.0)
    codes, e8m0 = nat.mx_encode(xg, GSIZE, nat.MX_E4M3, nat.MX_FLOOR)
    # the other per-unit families on the same tensors: one zero-point per group, per row of xg as [4, 512], two candidates
    from brevitas_amd.core.quant import _fused
    sd = nat.QuantDesc(1, GROUPS, GSIZE, code, code, code, code, 1, 1, 0.0, 15.0, 0, 0, 0, nat.OUT_DEQUANT, 0)
    rd = nat.QuantDesc(1, 4, 512, code, code, code, code, 1, 1, 0.0, 255.0, 0, 0, 0, nat.OUT_DEQUANT, 0)
    table = nat.mse_ratio_table([1.0, 0.75])
    xw, gw = xg.view(4, 512), gg.view(4, 512)
    assert nat.group_shifted_supported(sd, xg) and nat.row_shifted_supported(rd, xw)
    assert nat.group_mse_supported(gd, xg, len(table))
    sstat = nat.group_shifted_fwd(sd, xg, 1e-10, 15.0)[3]
    rstat = nat.row_shifted_fwd(rd, xw, 1e-10, 255.0)[3]
    _, _, mstat, midx = nat.group_mse_fwd(gd, xg, table, 1e-10, 7.0)
    wd = _fused.weight_norm_call(xw, 127.0, nat.ROUND_TO_ZERO, True)
    wn = (nat.NORM_L1, 2.0 ** 23 / 256, 1e-10)
    assert nat.weight_norm_supported(wd, *wn, xw)
    ws = (xw.float().abs().max(1).values / 127).contiguous()
    wg = xw.float().abs().sum(1).contiguous()
    wnorm = nat.weight_norm_fwd(wd, *wn, xw, ws, wg)[1]

    def some(fn):  # a route that may answer "not covered" must not do so here
        def run_it():
            assert fn() is not None
        return run_it

    def onepass(flag, fn, attr='ONEPASS'):
        def run_it():
            old = getattr(nat, attr)
            setattr(nat, attr, flag)
            try:
                assert fn() is not None
            finally:
                setattr(nat, attr, old)
        return run_it

    def weights():
        import brevitas_amd.quant as Q
        from brevitas_amd import WeightQuantGroup
        from brevitas_amd.nn import QuantConv2d
        model = torch.nn.Sequential(*[QuantConv2d(64, 64, 3, bias=False, weight_quant=Q.Int8WeightPerChannelFloat,
                                                  device=DEV, dtype=torch.float32) for _ in range(2)])
        group = WeightQuantGroup(model)
        assert len(group.covered) == 2
        with group:
            ys = [layer.quant_weight()[0] for layer in model]
        sum((y * torch.randn_like(y)).sum() for y in ys).backward()  # (contiguous gradients: the list backward)

    def stats():
        return nat.stats(nat.STAT_ABSMAX, x, OUTER, CH, INNER)

    def absmax():
        return nat.absmax_scale(x, OUTER, CH, INNER, 1e-10, 128.0, dt)

    def absmax_run():
        return nat.absmax_scale(x, OUTER, CH, INNER, 1e-10, 128.0, dt, running=run, momentum=0.1)

    def bwd_stats():
        return nat.fakequant_bwd_stats(d, g, x, scale, zp, stat, dt, 128.0, dt)

    def cluster(**kw):
        return nat.absmax_fakequant_cluster(d, x, 1e-10, 128.0, dt, run, 0.1, False, **kw)

    return [
        ('stats, one launch', onepass(True, stats), ['bvq_stats']),
        ('stats, two launches', onepass(False, stats), ['bvq_stats']),
        ('stats, min/max', some(lambda: nat.stats(nat.STAT_MINMAX, x, OUTER, CH, INNER)), ['bvq_stats']),
        ('absmax_scale, one launch', onepass(True, absmax), ['bvq_stats']),
        ('absmax_scale, two launches', onepass(False, absmax), ['bvq_stats']),
        ('absmax_scale, running, one launch', onepass(True, absmax_run), ['bvq_stats']),
        ('absmax_scale, running, two launches', onepass(False, absmax_run), ['bvq_stats']),
        ('fakequant_fwd', some(lambda: nat.fakequant_fwd(d, x, scale, zp)), ['bvq_fakequant_fwd']),
        ('stats_fakequant_fwd', some(lambda: nat.stats_fakequant_fwd(d, x, 1e-10, 128.0, dt)),
         ['bvq_stats_fakequant_fwd']),
        ('cluster forward', some(cluster), ['bvq_stats_fakequant_fwd']),
        ('cluster forward, a given form', some(lambda: cluster(form=nat.CLUSTER_WALK)), ['bvq_stats_fakequant_fwd']),
        ('group_quant_fwd', some(lambda: nat.group_quant_fwd(gd, xg, 1e-10, 7.0)), ['bvq_group_quant_fwd']),
        ('group_quant_bwd', some(lambda: nat.group_quant_bwd(gd, gg, xg, gscale, gstat, None, 1e-10, 7.0)),
         ['bvq_group_quant_bwd']),
        ('group_shifted_fwd', some(lambda: nat.group_shifted_fwd(sd, xg, 1e-10, 15.0)), ['bvq_group_shifted_fwd']),
        ('group_shifted_bwd', some(lambda: nat.group_shifted_bwd(sd, gg, xg, sstat, None, None, 1e-10, 15.0)),
         ['bvq_group_shifted_bwd']),
        ('row_shifted_fwd', some(lambda: nat.row_shifted_fwd(rd, xw, 1e-10, 255.0)), ['bvq_row_shifted_fwd']),
        ('row_shifted_bwd', some(lambda: nat.row_shifted_bwd(rd, gw, xw, rstat, None, None, 1e-10, 255.0)),
         ['bvq_row_shifted_bwd']),
        ('group_mse_fwd', some(lambda: nat.group_mse_fwd(gd, xg, table, 1e-10, 7.0)), ['bvq_group_mse_fwd']),
        ('group_mse_bwd', some(lambda: nat.group_mse_bwd(gd, gg, xg, mstat, midx, None, table, 1e-10, 7.0)),
         ['bvq_group_mse_bwd']),
        ('weight_norm_fwd', some(lambda: nat.weight_norm_fwd(wd, *wn, xw, ws, wg)), ['bvq_weight_norm_fwd']),
        ('weight_norm_bwd', some(lambda: nat.weight_norm_bwd(wd, *wn, gw, xw, ws, wg, wnorm)), ['bvq_weight_norm_bwd']),
        ('mx_quant_fwd', some(lambda: nat.mx_quant_fwd(xg, GSIZE, nat.MX_E4M3, nat.MX_FLOOR)), ['bvq_mx_quant_fwd']),
        ('mx_quant_bwd', some(lambda: nat.mx_quant_bwd(gg, xg, None, GSIZE, nat.MX_E4M3, nat.MX_FLOOR, False)),
         ['bvq_mx_quant_bwd']),
        ('mx_encode', some(lambda: nat.mx_encode(xg, GSIZE, nat.MX_E4M3, nat.MX_FLOOR)), ['bvq_mx_encode']),
        ('mx_decode', some(lambda: nat.mx_decode(codes, e8m0, GSIZE, nat.MX_E4M3, dt)), ['bvq_mx_decode']),
        ('kth_value', some(lambda: nat.kth_value(x, 5, OUTER, CH, INNER, True)), ['bvq_kth_value']),
        ('fakequant_bwd_stats, one launch', onepass(True, bwd_stats, 'ONEPASS_BWD'), ['bvq_fakequant_bwd']),
        ('fakequant_bwd_stats, two launches', onepass(False, bwd_stats, 'ONEPASS_BWD'), ['bvq_fakequant_bwd']),
        ('fakequant_bwd_shard', some(lambda: nat.fakequant_bwd_shard(d, g, x, scale, zp, stat, 0)),
         ['bvq_fakequant_bwd']),
        ('fakequant_bwd_learned', some(lambda: nat.fakequant_bwd_learned(d, g, x, scale, zp, value, 1e-10, 128.0)),
         ['bvq_fakequant_bwd']),
        ('fakequant_bwd', some(lambda: nat.fakequant_bwd(d, g, x, scale, zp, True, False)), ['bvq_fakequant_bwd']),
        ('weight list, forward and backward', weights, ['bvq_weight_quant_list_fwd', 'bvq_weight_quant_list_bwd']),
        ('unary (not bracketed)', some(lambda: nat.unary(nat.OP_ABS, x)), []),
    ]


def test_every_bracketed_wrapper_records_its_name():
    from brevitas_amd import _native as nat
    cases = _cases(nat)
    rec = _Recorder()
    got = []
    nat.set_kernel_timer(rec)
    try:
        for label, fn, _ in cases:
            rec.names = []
            fn()
            got.append((label, rec.names))
    finally:
        nat.set_kernel_timer(None)
    torch.cuda.synchronize()
    want = [(label, [pair for n in names for pair in (('before', n), ('after', n))]) for label, _, names in cases]
    assert got == want


def test_a_call_on_another_device_runs_there_and_leaves_the_current_one():
    from brevitas_amd import _native as nat
    if torch.cuda.device_count() < 2:
        pytest.skip('needs two devices')
    torch.manual_seed(20252)
    x = torch.randn(OUTER * CH * INNER).to(torch.bfloat16).to('cuda:1')

    def both():
        return nat.unary(nat.OP_ABS, x), *nat.absmax_scale(x, OUTER, CH, INNER, 1e-10, 128.0, torch.bfloat16)

    with torch.cuda.device(1):
        want = both()
    torch.cuda.set_device(0)
    got = both()
    assert torch.cuda.current_device() == 0
    for a, b in zip(got, want):
        assert a.device == torch.device('cuda:1') and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))
