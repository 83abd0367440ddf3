"""The workspace queries of the backward entries are their layouts, measured (Workspaces): host-side, no
GPU.  Every query keeps its classification -- -1 a bad descriptor, 0 (the stats-scaled backward only) a layout that is
not covered, > 0 a covered one -- and returns no more than before the layouts were shared with the entries."""
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
