"""The workspace queries of the backward, statistic and select entries are their layouts, measured (DESIGN.md,
Workspaces): host-side, no GPU.  Every query keeps its classification -- -1 a bad descriptor, 0 (the stats-scaled
backward only) a layout that is not covered, > 0 a covered one -- and returns no more than before the layouts were
shared with the entries.  The select's published counter offsets are the numbers they were."""
import ctypes

import pytest

from brevitas_amd import _native as nat

DTYPES = {'f32': nat.F32, 'bf16': nat.BF16, 'f16': nat.F16}
# shape -> the route a call with aligned tensors takes
SHAPES = {
    (2, 3, 128): 'row-mapped, full width',
    (2, 3, 129): 'row-mapped, width 1 (ragged rows; outer < 64: not column-mapped)',
    (5, 16, 1): 'column-mapped',
    (64, 6, 196): 'column-mapped',
    (256, 512, 3136): 'the benchmark',
    (1, 2, 20000000): 'more than 4096 row-mapped units per channel',
}
LONG_UNITS, WIDE_SELECT = (1, 1, 20000000), (1, 1, 1 << 22)  # one more shape of the statistics', of the select's table
STAT_KINDS = {'absmax': nat.STAT_ABSMAX, 'minmax': nat.STAT_MINMAX}
TIE_CHANNELS = (1, 2, 3, 520)
SELECT_CHANNELS = (1, 3, 520)
LIST_ITEMS = [(64, 576), (128, 1152), (16, 27), (256, 2304)]  # (channels, inner), repeated up to 16 items


def quant_desc(shape, dt, per_channel):
    code = DTYPES[dt]
    return nat.QuantDesc(shape[0], shape[1], shape[2], code, code, code, nat.F32, int(per_channel), 0, -128.0, 127.0, 0,
                         0, 0, nat.OUT_DEQUANT, 0)


def variant_desc(shape, dt, per_channel, kind):
    code = DTYPES[dt]
    return nat.VariantDesc(shape[0], shape[1], shape[2], kind, code, code, code, nat.F32, int(per_channel), 0, 0, 0,
                           -128.0, 127.0, 0.5, 1.0)


def weight_items(n):
    items = (nat.WeightItem * n)()
    for i in range(n):
        items[i].channels, items[i].inner = LIST_ITEMS[i % len(LIST_ITEMS)]
        items[i].x = 4096  # (a query reads no tensor: any non-null address)
        items[i].qmin, items[i].qmax, items[i].int_threshold = -128.0, 127.0, 127.0
    return items


def measured():
    """{case id: bytes} of every query over the table"""
    out = {}
    for shape in SHAPES:
        sid = 'x'.join(map(str, shape))
        for dt, code in DTYPES.items():
            for pc in (0, 1):
                key = '%s-%s-%s' % (sid, dt, 'pc' if pc else 'pt')
                d = quant_desc(shape, dt, pc)
                out['bwd-' + key] = nat.lib.bvq_fakequant_bwd_workspace_bytes(ctypes.byref(d))
                out['stats-' + key] = nat.lib.bvq_fakequant_bwd_stats_workspace_bytes(ctypes.byref(d))
                for kind in (nat.VAR_BINARY, nat.VAR_DECOUPLED):
                    v = variant_desc(shape, dt, pc, kind)
                    out['variant%d-%s' % (kind, key)] = nat.lib.bvq_variant_bwd_workspace_bytes(ctypes.byref(v))
            out['moments-%s-%s' % (sid, dt)] = nat.lib.bvq_abs_moments_workspace_bytes(code, *shape)
    for dt, code in DTYPES.items():
        for shape in list(SHAPES) + [LONG_UNITS]:
            for kind, k in STAT_KINDS.items():
                out['statws-%s-%s-%s' % ('x'.join(map(str, shape)), dt, kind)] = nat.lib.bvq_stats_workspace_bytes(
                    k, code, *shape)
        for shape in list(SHAPES) + [WIDE_SELECT]:
            out['kth-%s-%s' % ('x'.join(map(str, shape)), dt)] = nat.lib.bvq_kth_workspace_bytes(code, *shape)
    for ch in TIE_CHANNELS:
        out['tie-%d' % ch] = nat.lib.bvq_tie_info_bytes(ch)
    for dt, code in DTYPES.items():
        for n in (1, 16):
            items = weight_items(n)
            out['list%d-%s' % (n, dt)] = nat.lib.bvq_weight_quant_list_bwd_workspace_bytes(code, n,
                                                                                          ctypes.addressof(items))
    return out


# the same table from the library built at the parent commit, 1519979
PARENT = {
    'bwd-1x2x20000000-bf16-pc': 1073112, 'bwd-1x2x20000000-bf16-pt': 1073112, 'bwd-1x2x20000000-f16-pc': 1073112,
    'bwd-1x2x20000000-f16-pt': 1073112, 'bwd-1x2x20000000-f32-pc': 1073112, 'bwd-1x2x20000000-f32-pt': 1073112,
    'bwd-256x512x3136-bf16-pc': 15753488, 'bwd-256x512x3136-bf16-pt': 11024672, 'bwd-256x512x3136-f16-pc': 15753488,
    'bwd-256x512x3136-f16-pt': 11024672, 'bwd-256x512x3136-f32-pc': 15753488, 'bwd-256x512x3136-f32-pt': 11024672,
    'bwd-2x3x128-bf16-pc': 344, 'bwd-2x3x128-bf16-pt': 308, 'bwd-2x3x128-f16-pc': 344, 'bwd-2x3x128-f16-pt': 308,
    'bwd-2x3x128-f32-pc': 344, 'bwd-2x3x128-f32-pt': 308, 'bwd-2x3x129-bf16-pc': 308, 'bwd-2x3x129-bf16-pt': 308,
    'bwd-2x3x129-f16-pc': 308, 'bwd-2x3x129-f16-pt': 308, 'bwd-2x3x129-f32-pc': 308, 'bwd-2x3x129-f32-pt': 308,
    'bwd-5x16x1-bf16-pc': 1344, 'bwd-5x16x1-bf16-pt': 284, 'bwd-5x16x1-f16-pc': 1344, 'bwd-5x16x1-f16-pt': 284,
    'bwd-5x16x1-f32-pc': 1344, 'bwd-5x16x1-f32-pt': 284, 'bwd-64x6x196-bf16-pc': 14368, 'bwd-64x6x196-bf16-pt': 2288,
    'bwd-64x6x196-f16-pc': 9664, 'bwd-64x6x196-f16-pt': 2288, 'bwd-64x6x196-f32-pc': 2576,
    'bwd-64x6x196-f32-pt': 2288, 'list1-bf16': 1024, 'list1-f16': 1024, 'list1-f32': 1024, 'list16-bf16': 22528,
    'list16-f16': 22528, 'list16-f32': 34816, 'moments-1x2x20000000-bf16': 626520, 'moments-1x2x20000000-f16': 626520,
    'moments-1x2x20000000-f32': 626520, 'moments-256x512x3136-bf16': 7356680, 'moments-256x512x3136-f16': 7356680,
    'moments-256x512x3136-f32': 7356680, 'moments-2x3x128-bf16': 312, 'moments-2x3x128-f16': 312,
    'moments-2x3x128-f32': 312, 'moments-2x3x129-bf16': 312, 'moments-2x3x129-f16': 312, 'moments-2x3x129-f32': 312,
    'moments-5x16x1-bf16': 4488, 'moments-5x16x1-f16': 4488, 'moments-5x16x1-f32': 2440,
    'moments-64x6x196-bf16': 47304, 'moments-64x6x196-f16': 47304, 'moments-64x6x196-f32': 3336,
    'stats-1x2x20000000-bf16-pc': 0, 'stats-1x2x20000000-bf16-pt': 0, 'stats-1x2x20000000-f16-pc': 0,
    'stats-1x2x20000000-f16-pt': 0, 'stats-1x2x20000000-f32-pc': 0, 'stats-1x2x20000000-f32-pt': 0,
    'stats-256x512x3136-bf16-pc': 15728896, 'stats-256x512x3136-bf16-pt': 0, 'stats-256x512x3136-f16-pc': 15728896,
    'stats-256x512x3136-f16-pt': 0, 'stats-256x512x3136-f32-pc': 15728896, 'stats-256x512x3136-f32-pt': 0,
    'stats-2x3x128-bf16-pc': 328, 'stats-2x3x128-bf16-pt': 0, 'stats-2x3x128-f16-pc': 328, 'stats-2x3x128-f16-pt': 0,
    'stats-2x3x128-f32-pc': 328, 'stats-2x3x128-f32-pt': 0, 'stats-2x3x129-bf16-pc': 292, 'stats-2x3x129-bf16-pt': 0,
    'stats-2x3x129-f16-pc': 292, 'stats-2x3x129-f16-pt': 0, 'stats-2x3x129-f32-pc': 292, 'stats-2x3x129-f32-pt': 0,
    'stats-5x16x1-bf16-pc': 1472, 'stats-5x16x1-bf16-pt': 0, 'stats-5x16x1-f16-pc': 1472, 'stats-5x16x1-f16-pt': 0,
    'stats-5x16x1-f32-pc': 1472, 'stats-5x16x1-f32-pt': 0, 'stats-64x6x196-bf16-pc': 23776,
    'stats-64x6x196-bf16-pt': 0, 'stats-64x6x196-f16-pc': 19072, 'stats-64x6x196-f16-pt': 0,
    'stats-64x6x196-f32-pc': 2560, 'stats-64x6x196-f32-pt': 0, 'variant0-1x2x20000000-bf16-pc': 715760,
    'variant0-1x2x20000000-bf16-pt': 715760, 'variant0-1x2x20000000-f16-pc': 715760,
    'variant0-1x2x20000000-f16-pt': 715760, 'variant0-1x2x20000000-f32-pc': 715760,
    'variant0-1x2x20000000-f32-pt': 715760, 'variant0-256x512x3136-bf16-pc': 10510400,
    'variant0-256x512x3136-bf16-pt': 7354448, 'variant0-256x512x3136-f16-pc': 10510400,
    'variant0-256x512x3136-f16-pt': 7354448, 'variant0-256x512x3136-f32-pc': 10510400,
    'variant0-256x512x3136-f32-pt': 7354448, 'variant0-2x3x128-bf16-pc': 112, 'variant0-2x3x128-bf16-pt': 88,
    'variant0-2x3x128-f16-pc': 112, 'variant0-2x3x128-f16-pt': 88, 'variant0-2x3x128-f32-pc': 112,
    'variant0-2x3x128-f32-pt': 88, 'variant0-2x3x129-bf16-pc': 88, 'variant0-2x3x129-bf16-pt': 88,
    'variant0-2x3x129-f16-pc': 88, 'variant0-2x3x129-f16-pt': 88, 'variant0-2x3x129-f32-pc': 88,
    'variant0-2x3x129-f32-pt': 88, 'variant0-5x16x1-bf16-pc': 704, 'variant0-5x16x1-bf16-pt': 72,
    'variant0-5x16x1-f16-pc': 704, 'variant0-5x16x1-f16-pt': 72, 'variant0-5x16x1-f32-pc': 704,
    'variant0-5x16x1-f32-pt': 72, 'variant0-64x6x196-bf16-pc': 1600, 'variant0-64x6x196-bf16-pt': 1408,
    'variant0-64x6x196-f16-pc': 1600, 'variant0-64x6x196-f16-pt': 1408, 'variant0-64x6x196-f32-pc': 1600,
    'variant0-64x6x196-f32-pt': 1408, 'variant3-1x2x20000000-bf16-pc': 715760,
    'variant3-1x2x20000000-bf16-pt': 715760, 'variant3-1x2x20000000-f16-pc': 715760,
    'variant3-1x2x20000000-f16-pt': 715760, 'variant3-1x2x20000000-f32-pc': 715760,
    'variant3-1x2x20000000-f32-pt': 715760, 'variant3-256x512x3136-bf16-pc': 10510400,
    'variant3-256x512x3136-bf16-pt': 7354448, 'variant3-256x512x3136-f16-pc': 10510400,
    'variant3-256x512x3136-f16-pt': 7354448, 'variant3-256x512x3136-f32-pc': 10510400,
    'variant3-256x512x3136-f32-pt': 7354448, 'variant3-2x3x128-bf16-pc': 112, 'variant3-2x3x128-bf16-pt': 88,
    'variant3-2x3x128-f16-pc': 112, 'variant3-2x3x128-f16-pt': 88, 'variant3-2x3x128-f32-pc': 112,
    'variant3-2x3x128-f32-pt': 88, 'variant3-2x3x129-bf16-pc': 88, 'variant3-2x3x129-bf16-pt': 88,
    'variant3-2x3x129-f16-pc': 88, 'variant3-2x3x129-f16-pt': 88, 'variant3-2x3x129-f32-pc': 88,
    'variant3-2x3x129-f32-pt': 88, 'variant3-5x16x1-bf16-pc': 704, 'variant3-5x16x1-bf16-pt': 72,
    'variant3-5x16x1-f16-pc': 704, 'variant3-5x16x1-f16-pt': 72, 'variant3-5x16x1-f32-pc': 704,
    'variant3-5x16x1-f32-pt': 72, 'variant3-64x6x196-bf16-pc': 1600, 'variant3-64x6x196-bf16-pt': 1408,
    'variant3-64x6x196-f16-pc': 1600, 'variant3-64x6x196-f16-pt': 1408, 'variant3-64x6x196-f32-pc': 1600,
    'variant3-64x6x196-f32-pt': 1408,
}

# the statistic, select and tie queries from the library built at their parent commit, 2a28927
PARENT_STAT_SELECT = {
    'kth-1x1x4194304-bf16': 1196608, 'kth-1x1x4194304-f16': 1196608, 'kth-1x1x4194304-f32': 1204800,
    'kth-1x2x20000000-bf16': 33280, 'kth-1x2x20000000-f16': 33280, 'kth-1x2x20000000-f32': 49664,
    'kth-256x512x3136-bf16': 8395008, 'kth-256x512x3136-f16': 8395008, 'kth-256x512x3136-f32': 12589312,
    'kth-2x3x128-bf16': 49664, 'kth-2x3x128-f16': 49664, 'kth-2x3x128-f32': 74240, 'kth-2x3x129-bf16': 49664,
    'kth-2x3x129-f16': 49664, 'kth-2x3x129-f32': 74240, 'kth-5x16x1-bf16': 263072, 'kth-5x16x1-f16': 263072,
    'kth-5x16x1-f32': 394304, 'kth-64x6x196-bf16': 249600, 'kth-64x6x196-f16': 249600, 'kth-64x6x196-f32': 147968,
    'statws-1x1x20000000-bf16-absmax': 321048, 'statws-1x1x20000000-bf16-minmax': 321048,
    'statws-1x1x20000000-f16-absmax': 321048, 'statws-1x1x20000000-f16-minmax': 321048,
    'statws-1x1x20000000-f32-absmax': 321048, 'statws-1x1x20000000-f32-minmax': 321048,
    'statws-1x2x20000000-bf16-absmax': 625440, 'statws-1x2x20000000-bf16-minmax': 625440,
    'statws-1x2x20000000-f16-absmax': 625440, 'statws-1x2x20000000-f16-minmax': 625440,
    'statws-1x2x20000000-f32-absmax': 625440, 'statws-1x2x20000000-f32-minmax': 625440,
    'statws-256x512x3136-bf16-absmax': 7348480, 'statws-256x512x3136-bf16-minmax': 7348480,
    'statws-256x512x3136-f16-absmax': 7348480, 'statws-256x512x3136-f16-minmax': 7348480,
    'statws-256x512x3136-f32-absmax': 7348480, 'statws-256x512x3136-f32-minmax': 7348480,
    'statws-2x3x128-bf16-absmax': 352, 'statws-2x3x128-bf16-minmax': 352, 'statws-2x3x128-f16-absmax': 352,
    'statws-2x3x128-f16-minmax': 352, 'statws-2x3x128-f32-absmax': 352, 'statws-2x3x128-f32-minmax': 352,
    'statws-2x3x129-bf16-absmax': 352, 'statws-2x3x129-bf16-minmax': 352, 'statws-2x3x129-f16-absmax': 352,
    'statws-2x3x129-f16-minmax': 352, 'statws-2x3x129-f32-absmax': 352, 'statws-2x3x129-f32-minmax': 352,
    'statws-5x16x1-bf16-absmax': 4608, 'statws-5x16x1-bf16-minmax': 4608, 'statws-5x16x1-f16-absmax': 4608,
    'statws-5x16x1-f16-minmax': 4608, 'statws-5x16x1-f32-absmax': 2560, 'statws-5x16x1-f32-minmax': 2560,
    'statws-64x6x196-bf16-absmax': 47344, 'statws-64x6x196-bf16-minmax': 47344, 'statws-64x6x196-f16-absmax': 47344,
    'statws-64x6x196-f16-minmax': 47344, 'statws-64x6x196-f32-absmax': 3424, 'statws-64x6x196-f32-minmax': 3424,
    'tie-1': 8208, 'tie-2': 16, 'tie-3': 24, 'tie-520': 4160,
}
PARENT.update(PARENT_STAT_SELECT)
# what the select published at that commit: 'hist-<dtype>-<channels>-<pass>': bvq_kth_hist_offset;
# 'wide-<dtype>-<abs_key>-<pass>': bvq_kthw_plan's (offset, words)
PARENT_OFFSETS = {
    'hist-bf16-1-0': 0, 'hist-bf16-1-1': 8192, 'hist-bf16-3-0': 0, 'hist-bf16-3-1': 24576, 'hist-bf16-520-0': 0,
    'hist-bf16-520-1': 4259840, 'hist-f16-1-0': 0, 'hist-f16-1-1': 8192, 'hist-f16-3-0': 0, 'hist-f16-3-1': 24576,
    'hist-f16-520-0': 0, 'hist-f16-520-1': 4259840, 'hist-f32-1-0': 0, 'hist-f32-1-1': 8192, 'hist-f32-1-2': 16384,
    'hist-f32-3-0': 0, 'hist-f32-3-1': 24576, 'hist-f32-3-2': 49152, 'hist-f32-520-0': 0, 'hist-f32-520-1': 4259840,
    'hist-f32-520-2': 8519680, 'wide-bf16-0-0': (16896, 32768), 'wide-bf16-0-1': (147968, 2), 'wide-bf16-1-0':
    (16896, 32768), 'wide-f16-0-0': (16896, 32768), 'wide-f16-0-1': (147968, 2), 'wide-f16-1-0': (16896, 32768),
    'wide-f32-0-0': (25088, 32768), 'wide-f32-0-1': (156160, 131072), 'wide-f32-1-0': (25088, 32768),
    'wide-f32-1-1': (156160, 65536),
}


def test_every_case_has_a_parent_value():
    assert sorted(measured()) == sorted(PARENT)


@pytest.mark.parametrize('key', sorted(PARENT))
def test_query_classifies_as_before_and_is_no_larger(key):
    got, before = measured_once()[key], PARENT[key]
    assert (got > 0) == (before > 0) and (got == 0) == (before == 0), (key, got, before)
    assert got <= before, (key, got, before)


_CACHE = {}


def measured_once():
    if not _CACHE:
        _CACHE.update(measured())
    return _CACHE


def test_the_stats_query_says_not_covered_with_zero():
    for dt in DTYPES:
        # per-tensor scales, and too many units per channel for the one-workgroup finish
        assert measured_once()['stats-2x3x128-%s-pt' % dt] == 0
        assert measured_once()['stats-1x2x20000000-%s-pc' % dt] == 0
        for shape in ('2x3x128', '2x3x129', '5x16x1', '64x6x196', '256x512x3136'):
            assert measured_once()['stats-%s-%s-pc' % (shape, dt)] > 0
    assert all(v > 0 for k, v in measured_once().items() if not k.startswith('stats-'))


def test_bad_descriptors_give_minus_one():
    bad = quant_desc((2, 0, 8), 'bf16', 1)  # no channels
    assert nat.lib.bvq_fakequant_bwd_workspace_bytes(ctypes.byref(bad)) == -1
    assert nat.lib.bvq_fakequant_bwd_stats_workspace_bytes(ctypes.byref(bad)) == -1
    assert nat.lib.bvq_fakequant_bwd_workspace_bytes(None) == -1
    assert nat.lib.bvq_fakequant_bwd_stats_workspace_bytes(None) == -1
    badv = variant_desc((2, 3, 8), 'bf16', 1, 99)
    assert nat.lib.bvq_variant_bwd_workspace_bytes(ctypes.byref(badv)) == -1
    assert nat.lib.bvq_abs_moments_workspace_bytes(7, 2, 3, 8) == -1
    assert nat.lib.bvq_abs_moments_workspace_bytes(nat.BF16, 2, 0, 8) == -1
    items = weight_items(1)
    assert nat.lib.bvq_weight_quant_list_bwd_workspace_bytes(nat.BF16, 0, ctypes.addressof(items)) == -1
    assert nat.lib.bvq_weight_quant_list_bwd_workspace_bytes(nat.BF16, 17, ctypes.addressof(items)) == -1
    items[0].inner = 0
    assert nat.lib.bvq_weight_quant_list_bwd_workspace_bytes(nat.BF16, 1, ctypes.addressof(items)) == -1


def select_offsets():
    out = {}
    for dt, code in DTYPES.items():
        for ch in SELECT_CHANNELS:
            for p in range(nat.lib.bvq_kth_passes(code)):
                out['hist-%s-%d-%d' % (dt, ch, p)] = nat.lib.bvq_kth_hist_offset(code, ch, p)
        for abs_key in (0, 1):
            for p in range(nat.lib.bvq_kthw_plan(abs_key, code, -1, None, None)):
                off, words = ctypes.c_int64(-1), ctypes.c_int64(-1)
                nat.lib.bvq_kthw_plan(abs_key, code, p, ctypes.byref(off), ctypes.byref(words))
                out['wide-%s-%d-%d' % (dt, abs_key, p)] = (off.value, words.value)
    return out


def test_the_select_publishes_the_offsets_it_did():
    """a sharded caller slices its workspace at these for the all-reduce"""
    assert select_offsets() == PARENT_OFFSETS


def test_the_select_counters_lie_inside_the_workspace_and_apart():
    got = select_offsets()
    for dt, code in DTYPES.items():
        for ch in SELECT_CHANNELS:
            need = nat.lib.bvq_kth_workspace_bytes(code, 2, ch, 128)  # (row-mapped: the state alone)
            spans = []
            for p in range(nat.lib.bvq_kth_passes(code)):
                off = got['hist-%s-%d-%d' % (dt, ch, p)]
                spans.append((off, off + ch * 2048 * 4))
            if ch == 1:
                for abs_key in (0, 1):
                    wide = [got[k] for k in sorted(got) if k.startswith('wide-%s-%d-' % (dt, abs_key))]
                    assert len(wide) == nat.lib.bvq_kthw_plan(abs_key, code, -1, None, None)
                    both = spans + [(off, off + 4 * words) for off, words in wide]
                    assert all(words > 0 for _, words in wide)
                    check_spans(both, need, (dt, ch, abs_key))
            else:
                check_spans(spans, need, (dt, ch))


def check_spans(spans, need, what):
    spans = sorted(spans)
    assert spans[0][0] >= 0 and spans[-1][1] <= need, (what, spans, need)
    for (_, end), (start, _) in zip(spans, spans[1:]):
        assert end <= start, (what, spans)


def test_a_select_workspace_off_a_16_byte_boundary_is_refused_on_the_host():
    """the published offsets are those of an aligned base: every launching entry refuses base + 4 before it launches
    anything (no GPU is needed to see it; the addresses are never used)"""
    lib, F32, BASE = nat.lib, nat.F32, 1 << 20
    outer, ch, inner = 2, 3, 128
    need = lib.bvq_kth_workspace_bytes(F32, outer, ch, inner) + 16
    need1 = lib.bvq_kth_workspace_bytes(F32, 1, 1, 1 << 22) + 16
    for ws in (BASE + 4, BASE + 8):
        calls = {
            'bvq_kth_begin': lib.bvq_kth_begin(F32, ch, nat.KTH_EXPLICIT, 1, 0.0, ws, need, None),
            'bvq_kth_hist': lib.bvq_kth_hist(1, F32, BASE, outer, ch, inner, 0, ws, need, None),
            'bvq_kth_pick': lib.bvq_kth_pick(F32, ch, 0, nat.KTH_EXPLICIT, 0.0, ws, need, None),
            'bvq_kth_finish': lib.bvq_kth_finish(1, F32, ch, BASE, ws, need, None),
            'bvq_kthw_begin': lib.bvq_kthw_begin(1, F32, ws, need1, None),
            'bvq_kthw_hist': lib.bvq_kthw_hist(1, F32, BASE, 64, 0, ws, need1, None),
            'bvq_kthw_pick': lib.bvq_kthw_pick(1, F32, 0, nat.KTH_EXPLICIT, 1, 0.0, ws, need1, None),
            'bvq_kthw_finish': lib.bvq_kthw_finish(1, F32, BASE, ws, need1, None),
            'bvq_kth_value': lib.bvq_kth_value(1, F32, BASE, outer, ch, inner, 1, BASE, ws, need, None),
            'bvq_kth_pair': lib.bvq_kth_pair(1, F32, BASE, outer, ch, inner, 1, 2, BASE, ws, need, None),
            'bvq_kth_value/wide': lib.bvq_kth_value(1, F32, BASE, 1, 1, 1 << 22, 1, BASE, ws, need1, None),
        }
        for name, rc in calls.items():
            assert rc == -1, (name, ws, rc)
            assert '16-byte boundary' in nat.last_error()


def test_bad_statistic_and_select_queries_give_minus_one():
    assert nat.lib.bvq_stats_workspace_bytes(nat.STAT_ABSMAX, 7, 2, 3, 8) == -1
    assert nat.lib.bvq_stats_workspace_bytes(nat.STAT_MINMAX, nat.BF16, 2, 0, 8) == -1
    assert nat.lib.bvq_stats_workspace_bytes(nat.STAT_MINMAX, nat.BF16, -1, 3, 8) == -1
    assert nat.lib.bvq_kth_workspace_bytes(7, 2, 3, 8) == -1 and nat.lib.bvq_kth_workspace_bytes(nat.F32, 2, 0, 8) == -1
    assert nat.lib.bvq_tie_info_bytes(0) == -1
