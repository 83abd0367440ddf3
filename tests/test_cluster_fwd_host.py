"""The cluster forward's C entries (include/bvq.h, bvq_absmax_fakequant_cluster[_supported]) without a GPU: the
coverage predicate is host-side and answers for the headline activation, the entry rejects bad arguments before it
touches a device, and what the headline needs fits the per-stream arrival buffer."""
import pytest
import torch

BASE = 1 << 20  # a 16-byte aligned stand-in address: the predicate only looks at alignment and overlap


def _desc(nat, outer, ch, inner, dt=None, ct=None, scale_pc=1, pre=0, out=0, zp_pc=0, rm=0):
    dt = nat.BF16 if dt is None else dt
    ct = dt if ct is None else ct
    return nat.QuantDesc(outer, ch, inner, dt, ct, dt, nat.F32, scale_pc, zp_pc, -128.0, 127.0, rm, 0, 0, out, pre)


def _words(nat, d, x=BASE, y=None):
    if y is None:
        esize = 4 if d.x_dtype == nat.F32 else 2
        y = x + d.outer * d.channels * d.inner * esize + 4096
    return int(nat.lib.bvq_absmax_fakequant_cluster_supported(d, x, y))


def test_predicate_covers_the_headline_and_fits_the_arrival_buffer():
    from brevitas_amd import _native as nat
    for shape in ((256, 512, 3136), (32, 512, 3136)):
        for dt in (nat.BF16, nat.F16, nat.F32):
            for pre in (nat.PRE_NONE, nat.PRE_RELU):
                for rm in (nat.ROUND, nat.FLOOR, nat.ROUND_TO_ZERO):
                    w = _words(nat, _desc(nat, *shape, dt=dt, pre=pre, rm=rm))
                    assert 0 < w <= nat.ARRIVE_WORDS, (shape, dt, pre, rm, w)
    # the headline: 256 rows of 3136 bf16 = one slice per wave, 16 workgroups of 16 waves per channel
    assert _words(nat, _desc(nat, 256, 512, 3136)) == 512 * (16 + 1)


def test_predicate_rejects_what_it_does_not_cover():
    from brevitas_amd import _native as nat
    head = (256, 512, 3136)
    assert _words(nat, _desc(nat, *head, scale_pc=0)) == 0                    # per-tensor scale
    assert _words(nat, _desc(nat, 256, 1, 3136)) == 0                         # one channel
    assert _words(nat, _desc(nat, *head, dt=nat.BF16, ct=nat.F32)) == 0       # mixed dtypes
    assert _words(nat, _desc(nat, *head, out=nat.OUT_INT)) == 0               # integer output
    assert _words(nat, _desc(nat, *head, zp_pc=1)) == 0                       # per-channel zero-point
    assert _words(nat, _desc(nat, *head), x=BASE + 2) == 0                    # unaligned x
    assert _words(nat, _desc(nat, *head), y=BASE * 4096 + 8) == 0             # unaligned y
    assert _words(nat, _desc(nat, *head), y=BASE + 4096) == 0                 # y overlaps x
    assert _words(nat, _desc(nat, 256, 512, 3135)) == 0                       # ragged rows
    assert _words(nat, _desc(nat, 1100, 8, 3136)) == 0                        # 69 workgroups per channel: above the cap
    assert _words(nat, _desc(nat, 1024, 8, 3136)) > 0                         # 64: at the cap
    assert nat.lib.bvq_absmax_fakequant_cluster_supported(None, BASE, BASE * 4096) == 0


def test_entry_rejects_bad_arguments_without_a_device():
    from brevitas_amd import _native as nat
    lib = nat.lib
    d = _desc(nat, 256, 512, 3136)
    x, y, stat, scale, arr = BASE, BASE * 4096, BASE * 8192, BASE * 8192 + 4096, BASE * 16384

    def call(desc=d, x=x, y=y, stat=stat, scale=scale, arr=arr, words=nat.ARRIVE_WORDS, flags=0, run_dtype=0):
        return lib.bvq_absmax_fakequant_cluster(desc, x, 1e-10, 1, 128.0, stat, scale, run_dtype, None, 0.1, 0, y, arr,
                                                words, flags, None, None)

    assert call(desc=None) != 0
    for kw in (dict(x=None), dict(y=None), dict(stat=None), dict(scale=None), dict(arr=None)):
        assert call(**kw) != 0, kw
        assert b'null pointer' in lib.bvq_last_error(), kw
    assert call(flags=2) != 0 and b'bad argument' in lib.bvq_last_error()
    assert call(desc=_desc(nat, 256, 512, 3136, scale_pc=0)) != 0
    assert b'not covered' in lib.bvq_last_error()
    assert call(words=512 * 17 - 1) != 0
    assert b'arrival buffer' in lib.bvq_last_error()
    bad = _desc(nat, 256, 512, 3136)
    bad.pre_op = 7
    assert call(desc=bad) != 0


def test_entries_are_exported():
    from brevitas_amd import _native as nat
    for name in ('bvq_absmax_fakequant_cluster_supported', 'bvq_absmax_fakequant_cluster'):
        assert name in nat.EXPORTS
        assert hasattr(nat.lib, name)
