"""Every backward, statistic and select entry that carves a workspace runs in a buffer of exactly the queried size, on
each of its routes: the same bits as with a generous buffer, nothing written outside the slice, and a buffer one byte
short of the measured layout refused before any launch (Workspaces)."""
import ctypes
import os
import re

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD, FILL, BIG = 256, 0xA5, 1 << 20
ERR_WORKSPACE = -3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (outer, channels, inner), misaligned x -> the route
ROW_FULL, ROW_RAGGED, COLS_A, COLS_B = (2, 3, 128), (2, 3, 129), (5, 16, 1), (64, 6, 196)
ROUTES = [(ROW_FULL, False), (ROW_RAGGED, False), (ROW_FULL, True), (COLS_A, False), (COLS_B, False)]
ROUTE_IDS = ['row-full', 'row-ragged', 'row-misaligned-x', 'cols-5x16x1', 'cols-64x6x196']


def slack():
    text = open(os.path.join(ROOT, 'brevitas_amd', 'csrc', 'bvq_common.h')).read()
    return int(re.search(r'constexpr int64_t kWorkspaceSlack = (\d+);', text).group(1))


def bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32) if t.element_size() == 4 else t


def tensors(shape, dtype, misaligned):
    """x (one element past a 16-byte boundary if asked), g, with a tie and an arg-max at the very end"""
    outer, ch, inner = shape
    n = outer * ch * inner
    gen = torch.Generator(device='cpu').manual_seed(97531)
    x = (torch.randn(n + 8, generator=gen) * 3).to(dtype).to(DEV)[int(misaligned):int(misaligned) + n]
    g = torch.randn(n, generator=gen).to(dtype).to(DEV)
    xv = x.view(outer, ch, inner)
    if ch > 1:
        xv[:, 1, :] = 0.0
    xv[outer - 1, 0, inner - 1] = 40.0
    assert (x.data_ptr() % 16 != 0) == misaligned
    return x, g


def desc(nat, shape, dtype, **kw):
    code = nat.dtype_code(dtype)
    f = dict(scale_per_channel=1, zp_per_channel=0)
    f.update(kw)
    return nat.QuantDesc(shape[0], shape[1], shape[2], code, code, code, nat.F32, f['scale_per_channel'],
                         f['zp_per_channel'], -128.0, 127.0, 0, 0, 0, nat.OUT_DEQUANT, 0)


def run_both(nat, wsb, call, short_is_refused=False, short=None, big_bytes=BIG):
    """call(ws_ptr, ws_bytes) -> (rc, outputs) with a 1 MiB workspace (big_bytes: a query above that) and with a guarded
    slice of exactly wsb bytes: the same bits, both guards intact; optionally the refusal of wsb - slack - 1 bytes
    (short: of that many instead -- a query without slack, or a layout that is not the query's largest)"""
    assert 0 < wsb <= big_bytes
    big = torch.zeros(big_bytes, dtype=torch.uint8, device=DEV)
    rc, want = call(big.data_ptr(), big_bytes)
    assert rc == 0, nat.last_error()
    buf = torch.full((GUARD + wsb + GUARD,), FILL, dtype=torch.uint8, device=DEV)
    rc, got = call(buf.data_ptr() + GUARD, wsb)
    assert rc == 0, nat.last_error()
    torch.cuda.synchronize()
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(bits(a), bits(b)), 'output %d differs' % i
    assert bool((buf[:GUARD] == FILL).all()) and bool((buf[GUARD + wsb:] == FILL).all())
    if short_is_refused or short is not None:
        # (refused by the entry's size check: nothing launches)
        rc, _ = call(buf.data_ptr() + GUARD, wsb - slack() - 1 if short is None else short)
        assert rc == ERR_WORKSPACE, (rc, nat.last_error())


def scale_zp(nat, x, shape, per_channel=True):
    outer, ch, inner = shape
    stat, scale = nat.absmax_scale(x.clone(), outer, ch if per_channel else 1,
                                   inner if per_channel else ch * inner, 1e-10, 128.0, x.dtype)
    return stat.to(x.dtype).contiguous(), scale, torch.zeros(1, device=DEV)


def case_fakequant_bwd(route, form):
    from brevitas_amd import _native as nat
    shape, mis = route
    dtype = torch.bfloat16
    x, g = tensors(shape, dtype, mis)
    stat, scale, zp = scale_zp(nat, x, shape)
    d = desc(nat, shape, dtype)
    ch = shape[1]
    wsb = int(nat.lib.bvq_fakequant_bwd_workspace_bytes(ctypes.byref(d)))
    bounds = torch.tensor([-100.0, 90.0], device=DEV)
    value = (scale.float() * 128.0).to(dtype)
    st = nat.stream_ptr(torch.device(DEV))
    P = nat.ptr

    def call(ws, n):
        dx = torch.empty_like(x)
        ds = torch.empty(ch, dtype=torch.float32, device=DEV)
        if form == 'dscale' or form == 'dscale+dzp':
            dz = torch.empty(ch, dtype=torch.float32, device=DEV) if form == 'dscale+dzp' else None
            rc = nat.lib.bvq_fakequant_bwd(ctypes.byref(d), P(g), P(x), P(scale), P(zp), P(dx), P(ds), P(dz), None, None,
                                           ws, n, st)
            return rc, [dx, ds] + ([dz] if dz is not None else [])
        if form == 'bounds':
            db = torch.empty(2, ch, dtype=torch.float32, device=DEV)
            rc = nat.lib.bvq_fakequant_bwd_bounds(ctypes.byref(d), P(g), P(x), P(scale), P(zp), P(bounds), P(dx), P(ds),
                                                  P(db), ws, n, st)
            return rc, [dx, ds, db]
        dv = torch.empty(ch, dtype=dtype, device=DEV)
        rc = nat.lib.bvq_fakequant_bwd_learned(ctypes.byref(d), P(g), P(x), P(scale), P(zp), P(dx), P(ds), P(value),
                                               nat.dtype_code(dtype), 1e-10, 1, 128.0, None, P(dv), ws, n, st)
        return rc, [dx, ds, dv]

    return nat, wsb, call, None


def case_fakequant_bwd_stats(route, form):
    from brevitas_amd import _native as nat
    shape, mis = route
    dtype = torch.bfloat16
    x, g = tensors(shape, dtype, mis)
    stat, scale, zp = scale_zp(nat, x, shape)
    d = desc(nat, shape, dtype)
    ch = shape[1]
    wsb = int(nat.lib.bvq_fakequant_bwd_stats_workspace_bytes(ctypes.byref(d)))
    dev = torch.device(DEV)
    st = nat.stream_ptr(dev)
    arrive = nat.arrival_buffer(dev, st, ch)
    code = nat.dtype_code(dtype)
    P = nat.ptr
    onepass = bool(nat.lib.bvq_fakequant_bwd_stats_onepass_supported(ctypes.byref(d)))

    def call(ws, n):
        dx = torch.empty_like(x)
        if form.startswith('shard'):
            msg = torch.empty(2 * ch, dtype=torch.float64, device=DEV)
            pos = torch.empty(ch, dtype=torch.int64, device=DEV)
            arr = arrive if form.endswith('arrive') else None
            rc = nat.lib.bvq_fakequant_bwd_shard(ctypes.byref(d), P(g), P(x), P(scale), P(zp), P(stat), P(dx), P(msg),
                                                 P(pos), 1, ws, n, P(arr), arr.numel() if arr is not None else 0, st)
            return rc, [dx, msg, pos]
        ds = torch.empty(ch, dtype=torch.float32, device=DEV)
        if form == 'one-launch' and onepass:
            rc = nat.lib.bvq_fakequant_bwd_stats_onepass(ctypes.byref(d), P(g), P(x), P(scale), P(zp), P(stat), P(dx),
                                                         P(ds), code, 128.0, code, ws, n, P(arrive), arrive.numel(), st)
        else:  # (column-mapped layouts have the two-launch form only)
            rc = nat.lib.bvq_fakequant_bwd_stats(ctypes.byref(d), P(g), P(x), P(scale), P(zp), P(stat), P(dx), P(ds),
                                                 code, 128.0, code, ws, n, st)
        return rc, [dx, ds]

    return nat, wsb, call, arrive


def case_variant_bwd(route, kind):
    from brevitas_amd import _native as nat
    shape, mis = route
    dtype = torch.bfloat16
    x, g = tensors(shape, dtype, mis)
    stat, scale, zp = scale_zp(nat, x, shape)
    pre = (scale.float() * 1.25).to(scale.dtype)
    code = nat.dtype_code(dtype)
    k = nat.VAR_DECOUPLED if kind == 'decoupled' else nat.VAR_BINARY
    d = nat.VariantDesc(shape[0], shape[1], shape[2], k, code, code, code, nat.F32, 1, 0, 0, 0, -128.0, 127.0, 0.5, 1.0)
    ch = shape[1]
    wsb = int(nat.lib.bvq_variant_bwd_workspace_bytes(ctypes.byref(d)))
    st = nat.stream_ptr(torch.device(DEV))
    P = nat.ptr

    def call(ws, n):
        dx = torch.empty_like(x)
        ds = torch.empty(ch, dtype=torch.float32, device=DEV)
        dp = torch.empty(ch, dtype=torch.float32, device=DEV) if kind == 'decoupled' else None
        rc = nat.lib.bvq_variant_bwd(ctypes.byref(d), P(g), P(x), P(scale), P(pre) if kind == 'decoupled' else None,
                                     None, None, P(dx), P(ds), P(dp), ws, n, st)
        return rc, [dx, ds] + ([dp] if dp is not None else [])

    return nat, wsb, call, None


def case_abs_moments(route, form=None):
    from brevitas_amd import _native as nat
    shape, mis = route
    dtype = torch.bfloat16
    x, _ = tensors(shape, dtype, mis)
    ch = shape[1]
    code = nat.dtype_code(dtype)
    wsb = int(nat.lib.bvq_abs_moments_workspace_bytes(code, *shape))
    st = nat.stream_ptr(torch.device(DEV))

    def call(ws, n):
        sums = torch.empty(3 * ch, dtype=torch.float32, device=DEV)
        rc = nat.lib.bvq_abs_moments(code, nat.ptr(x), shape[0], ch, shape[2], nat.ptr(sums), ws, n, st)
        return rc, [sums]

    return nat, wsb, call, None


CASES = [(case_fakequant_bwd, f) for f in ('dscale', 'dscale+dzp', 'bounds', 'learned')] + \
        [(case_fakequant_bwd_stats, f) for f in ('two-launch', 'one-launch', 'shard-rank1', 'shard-rank1-arrive')] + \
        [(case_variant_bwd, f) for f in ('binary', 'decoupled')] + [(case_abs_moments, None)]
CASE_IDS = ['%s-%s' % (c.__name__[5:], f) for c, f in CASES]


@pytest.mark.parametrize('route', ROUTES, ids=ROUTE_IDS)
@pytest.mark.parametrize('case', CASES, ids=CASE_IDS)
def test_exact_workspace(case, route):
    build, form = case
    nat, wsb, call, arrive = build(route, form)
    # a column-mapped stats layout has that one route: its layout is the query's
    run_both(nat, wsb, call, short_is_refused=build is case_fakequant_bwd_stats and route[0] in (COLS_A, COLS_B))
    if arrive is not None:
        torch.cuda.synchronize()
        assert int(arrive.count_nonzero()) == 0


@pytest.mark.parametrize('case', [(case_fakequant_bwd, 'bounds'), (case_fakequant_bwd_stats, 'two-launch'),
                                  (case_variant_bwd, 'decoupled'), (case_abs_moments, None)],
                         ids=['fakequant_bwd-bounds', 'fakequant_bwd_stats', 'variant_bwd', 'abs_moments'])
def test_short_workspace_is_refused_at_the_larger_width(case):
    """On a shape that only the row-mapped route covers, a query is the larger of the layouts at the two vector widths
    (for bvq_fakequant_bwd: of the call with all three partial arrays, the bound gradients), plus the slack.  Aligned
    tensors take the full width and an x one element off takes width 1, so a buffer one byte short of the query less
    the slack is refused by at least one of the two calls -- by the size check, before anything is launched; the other
    call's layout, if smaller, fits that buffer."""
    build, form = case
    rcs = []
    for mis in (False, True):
        nat, wsb, call, _ = build((ROW_FULL, mis), form)
        buf = torch.full((GUARD + wsb + GUARD,), FILL, dtype=torch.uint8, device=DEV)
        rc, _ = call(buf.data_ptr() + GUARD, wsb - slack() - 1)
        torch.cuda.synchronize()
        assert rc in (0, ERR_WORKSPACE), nat.last_error()
        assert bool((buf[:GUARD] == FILL).all()) and bool((buf[GUARD + wsb - slack() - 1:] == FILL).all())
        rcs.append(rc)
    assert ERR_WORKSPACE in rcs, rcs


@pytest.mark.parametrize('n_items', [1, 16])
def test_weight_quant_list_bwd(n_items):
    from brevitas_amd import _native as nat
    dtype = torch.bfloat16
    sizes = [(64, 576), (128, 1152), (16, 32), (32, 2304)]
    items = (nat.WeightItem * n_items)()
    gen = torch.Generator(device='cpu').manual_seed(24680)
    xs, gs = [], []
    for i in range(n_items):
        c, inner = sizes[i % len(sizes)]
        xs.append(torch.randn(c, inner, generator=gen).to(dtype).to(DEV))
        gs.append(torch.randn(c, inner, generator=gen).to(dtype).to(DEV))
        it = items[i]
        it.x, it.channels, it.inner = xs[i].data_ptr(), c, inner
        it.min_val, it.int_threshold, it.qmin, it.qmax, it.use_min, it.clamp_ste = 1e-10, 127.0, -127.0, 127.0, 1, 0
    assert nat.weight_list_supported(items, 0, n_items, dtype, nat.ROUND)
    ys, stat, scale = nat.weight_quant_list_fwd(items, 0, xs, dtype, nat.ROUND)
    total = sum(int(items[i].channels) for i in range(n_items))
    dev = torch.device(DEV)
    st = nat.stream_ptr(dev)
    arrive = nat.arrival_buffer(dev, st, total)
    code = nat.dtype_code(dtype)
    addr = ctypes.addressof(items)

    def call(ws, n):
        dxs = [torch.empty_like(x) for x in xs]
        ds = torch.empty(total, dtype=torch.float32, device=DEV)
        off = 0
        for i in range(n_items):
            it = items[i]
            it.g, it.dx = gs[i].data_ptr(), dxs[i].data_ptr()
            it.stat = stat.data_ptr() + off * stat.element_size()
            it.scale = scale.data_ptr() + off * scale.element_size()
            it.dscale = ds.data_ptr() + off * 4
            off += int(it.channels)
        rc = nat.lib.bvq_weight_quant_list_bwd(code, code, code, nat.ROUND, n_items, addr, ws, n, nat.ptr(arrive),
                                               arrive.numel(), st)
        return rc, dxs + [ds]

    wsb = int(nat.lib.bvq_weight_quant_list_bwd_workspace_bytes(code, n_items, addr))
    run_both(nat, wsb, call, short_is_refused=True)  # (one route: every item at full width)
    torch.cuda.synchronize()
    assert int(arrive.count_nonzero()) == 0


# ---- the statistic entries ------------------------------------------------------------------------------------------
def const(name):
    """an integer constant of the library's sources"""
    for f in ('bvq_common.hip', 'bvq_stats.hip'):
        m = re.search(r'(?:#define|constexpr int64_t) %s(?: =)? (\d+)' % name,
                      open(os.path.join(ROOT, 'brevitas_amd', 'csrc', f)).read())
        if m:
            return int(m.group(1))
    raise KeyError(name)


def over_one_finish_slice():
    """The smallest 16-byte aligned row length of a 16-bit type that a full-width tiling cuts into more than
    kFinishSlice pieces: pieces are BVQ_PIECE_CHUNKS 16-byte chunks per lane of a 64-lane wave -- 8 * 64 * 8 = 4096
    elements -- so kFinishSlice = 4096 of them and one more chunk, 16777224 elements (32 MiB).  As the rows of (1, 2, N)
    that is 4097 partials per channel, a two-stage finish; as the one row of (1, 1, N) 4097 short units, which the
    whole-tensor abs-max replaces by long ones."""
    return const('kFinishSlice') * const('BVQ_PIECE_CHUNKS') * 64 * 8 + 8


def stat_call(nat, entry, kind, shape, x, out_dtype):
    """(workspace query, call) of one statistic entry on x[shape]"""
    outer, ch, inner = shape
    code, ocode = nat.dtype_code(x.dtype), nat.dtype_code(out_dtype)
    st = nat.stream_ptr(torch.device(DEV))
    P = nat.ptr
    wsb = int(nat.lib.bvq_stats_workspace_bytes(kind, code, *shape))
    running0 = torch.full((ch,), 0.5, dtype=torch.float32, device=DEV)

    def call(ws, n):
        out = torch.empty(ch * (2 if kind == nat.STAT_MINMAX else 1), dtype=out_dtype, device=DEV)
        if entry == 'stats':
            return nat.lib.bvq_stats(kind, code, P(x), outer, ch, inner, ocode, P(out), ws, n, st), [out]
        if entry == 'stats_pre':
            return nat.lib.bvq_stats_pre(kind, nat.PRE_SIGMOID, code, P(x), outer, ch, inner, ocode, P(out), ws, n,
                                         st), [out]
        scale = torch.empty(ch, dtype=torch.float32, device=DEV)
        if entry == 'absmax_scale':
            rc = nat.lib.bvq_absmax_scale(nat.PRE_NONE, code, P(x), outer, ch, inner, P(out), 1e-10, 1, 128.0, nat.F32,
                                          P(scale), ws, n, st)
            return rc, [out, scale]
        running = running0.clone()
        rc = nat.lib.bvq_absmax_scale_running(nat.PRE_NONE, code, P(x), outer, ch, inner, P(out), 1e-10, 1, 128.0,
                                              nat.F32, P(scale), nat.F32, P(running), 0.1, 0, ws, n, st)
        return rc, [out, scale, running]

    return wsb, call


@pytest.mark.parametrize('route', ROUTES, ids=ROUTE_IDS)
@pytest.mark.parametrize('out_f32', [False, True], ids=['out-x-dtype', 'out-f32'])
@pytest.mark.parametrize('kind', ['absmax', 'minmax'])
def test_stats_exact_workspace(kind, out_f32, route):
    """On each of these shapes the route taken has the query's largest layout -- the row-mapped units are as many at
    both widths, and no fewer bytes than the tie words; the column-mapped partial rows are more -- so one byte short of
    the query less the slack is refused."""
    from brevitas_amd import _native as nat
    shape, mis = route
    x, _ = tensors(shape, torch.bfloat16, mis)
    k = nat.STAT_MINMAX if kind == 'minmax' else nat.STAT_ABSMAX
    wsb, call = stat_call(nat, 'stats', k, shape, x, torch.float32 if out_f32 else x.dtype)
    run_both(nat, wsb, call, short_is_refused=True)


@pytest.mark.parametrize('entry,shape', [('stats_pre', ROW_FULL), ('absmax_scale', ROW_FULL), ('absmax_scale', COLS_B),
                                         ('absmax_scale_running', ROW_FULL), ('absmax_scale_running', COLS_B)])
def test_stats_entries_exact_workspace(entry, shape):
    from brevitas_amd import _native as nat
    x, _ = tensors(shape, torch.bfloat16, False)
    wsb, call = stat_call(nat, entry, nat.STAT_ABSMAX, shape, x, x.dtype)
    run_both(nat, wsb, call)


@pytest.mark.parametrize('channels', [2, 1], ids=['two-stage-finish', 'long-units'])
def test_stats_exact_workspace_past_one_finish_slice(channels):
    from brevitas_amd import _native as nat
    shape = (1, channels, over_one_finish_slice())
    x, _ = tensors(shape, torch.bfloat16, False)
    wsb, call = stat_call(nat, 'stats', nat.STAT_ABSMAX, shape, x, x.dtype)
    run_both(nat, wsb, call)


@pytest.mark.parametrize('per_channel', [True, False], ids=['per-channel', 'one-channel-tie'])
def test_stat_bwd_exact_workspace(per_channel):
    """the tie words are all bvq_stat_bwd carves: one byte short of them is refused"""
    from brevitas_amd import _native as nat
    outer, ch, inner = ROW_FULL
    x, g = tensors(ROW_FULL, torch.bfloat16, False)
    if not per_channel:
        x[7] = -40.0  # (a second element attaining the whole tensor's maximum of |x|)
        outer, ch, inner = 1, 1, x.numel()
    code = nat.dtype_code(x.dtype)
    stat = nat.stats(nat.STAT_ABSMAX, x, outer, ch, inner)
    gstat = g[:ch].contiguous()
    st = nat.stream_ptr(torch.device(DEV))
    P = nat.ptr

    def call(ws, n):
        dx = torch.empty_like(x)
        rc = nat.lib.bvq_stat_bwd(0, code, P(x), P(stat), P(gstat), P(dx), outer, ch, inner, 0, ws, n, st)
        return rc, [dx]

    wsb = int(nat.lib.bvq_stats_workspace_bytes(nat.STAT_ABSMAX, code, outer, ch, inner))
    run_both(nat, wsb, call, short=int(nat.lib.bvq_tie_info_bytes(ch)) - 1)


# ---- the select entries: their queries carry no slack -------------------------------------------------------------
WIDE = (1, 1, 1 << 22)


def select_case(nat, shape, dtype):
    outer, ch, inner = shape
    x, _ = tensors(shape, dtype, False)
    code = nat.dtype_code(dtype)
    wsb = int(nat.lib.bvq_kth_workspace_bytes(code, *shape))
    n = outer * inner
    return x, code, wsb, (max(1, n // 3), n)


@pytest.mark.parametrize('entry', ['value', 'pair'])
@pytest.mark.parametrize('shape,dtype,short', [(ROW_FULL, torch.bfloat16, False), (COLS_B, torch.bfloat16, True),
                                               (WIDE, torch.float32, True)],
                         ids=['row-mapped', 'channel-last-copy', 'wide'])
def test_select_exact_workspace(shape, dtype, short, entry):
    from brevitas_amd import _native as nat
    outer, ch, inner = shape
    x, code, wsb, (k1, k2) = select_case(nat, shape, dtype)
    st = nat.stream_ptr(torch.device(DEV))
    P = nat.ptr

    def call(ws, n):
        out = torch.empty((1 if entry == 'value' else 2) * ch, dtype=dtype, device=DEV)
        if entry == 'value':
            return nat.lib.bvq_kth_value(1, code, P(x), outer, ch, inner, k1, P(out), ws, n, st), [out]
        return nat.lib.bvq_kth_pair(1, code, P(x), outer, ch, inner, k1, k2, P(out), ws, n, st), [out]

    run_both(nat, wsb, call, short=wsb - 1 if short else None, big_bytes=max(BIG, 2 * wsb))


@pytest.mark.parametrize('wide', [False, True], ids=['kth-steps', 'kthw-steps'])
def test_select_steps_exact_workspace(wide):
    """the steps in order, in the exact buffer: the one-shot entry's bits"""
    from brevitas_amd import _native as nat
    shape = (1, 1, 1 << 16) if wide else ROW_FULL
    outer, ch, inner = shape
    dtype = torch.float32
    x, code, wsb, (k, _) = select_case(nat, shape, dtype)
    st = nat.stream_ptr(torch.device(DEV))
    P, lib = nat.ptr, nat.lib
    passes = lib.bvq_kthw_plan(0, code, -1, None, None) if wide else lib.bvq_kth_passes(code)

    def call(ws, n):
        out = torch.empty(ch, dtype=dtype, device=DEV)
        rc = lib.bvq_kthw_begin(0, code, ws, n, st) if wide else lib.bvq_kth_begin(code, ch, nat.KTH_EXPLICIT, k, 0.0, ws,
                                                                                    n, st)
        for p in range(passes):
            if wide:
                rc = rc or lib.bvq_kthw_hist(0, code, P(x), x.numel(), p, ws, n, st)
                rc = rc or lib.bvq_kthw_pick(0, code, p, nat.KTH_EXPLICIT, k, 0.0, ws, n, st)
            else:
                rc = rc or lib.bvq_kth_hist(0, code, P(x), outer, ch, inner, p, ws, n, st)
                rc = rc or lib.bvq_kth_pick(code, ch, p, nat.KTH_EXPLICIT, 0.0, ws, n, st)
        rc = rc or (lib.bvq_kthw_finish(0, code, P(out), ws, n, st) if wide else
                    lib.bvq_kth_finish(0, code, ch, P(out), ws, n, st))
        return rc, [out]

    run_both(nat, wsb, call, big_bytes=max(BIG, 2 * wsb))
    buf = torch.zeros(wsb, dtype=torch.uint8, device=DEV)
    rc, (steps,) = call(buf.data_ptr(), wsb)
    assert rc == 0, nat.last_error()
    assert torch.equal(bits(steps), bits(nat.kth_value(x, k, outer, ch, inner, False)))
