"""The edges of the k-th select's shared pieces, against torch.kthvalue on the device (exact):

* the flat walk under bvq_kthw_hist (kth_hist15_kernel, kth_low_kernel): every `head` in front of the first 16-byte
  boundary, element counts around one vector, one workgroup row (1024 chunks) and one loop trip of the first pass
  (1024 * 4 chunks; the low pass's 256 * 4 lies below it), all four widths of the second read (0, 1, 16, 17 bits);
* the pick kernel on both routes, with the rank in the first bins of thread 0 and in the last bin of the last thread;
* the one-shot per-tensor route, its stepwise form and the digit passes giving the same bits;
* the argument checks of every select entry, which return before anything is launched.
"""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
DT = {'bf16': torch.bfloat16, 'f16': torch.float16, 'f32': torch.float32}
KEYS = pytest.mark.parametrize('abs_key', [True, False], ids=['abs', 'signed'])
DTYPES = pytest.mark.parametrize('dn', ['bf16', 'f16', 'f32'])
# return codes of include/bvq.h
OK, ERR_INVALID, ERR_UNSUPPORTED, ERR_WORKSPACE = 0, -1, -2, -3


def _run(steps, first_hist=None):
    steps.begin()
    for p in range(steps.passes):
        h = steps.hist(p)
        if p == 0 and first_hist is not None:
            first_hist.append(h.to(torch.int64).sum())
        steps.pick(p)
    return steps.finish()


def _kth(x, k, abs_key):
    return (x.abs() if abs_key else x).float().kthvalue(k).values


@functools.lru_cache(maxsize=None)
def _randn(dn, n):
    g = torch.Generator(device=DEV).manual_seed(20260 + n)
    buf = torch.empty(n + 16, device=DEV, dtype=DT[dn])
    assert buf.data_ptr() % 16 == 0
    buf.copy_(torch.randn(n + 16, device=DEV, generator=g).clamp_(-4, 4).to(DT[dn]))
    return buf


@DTYPES
@KEYS
def test_flat_walk_edges(dn, abs_key):
    from brevitas_amd import _native as nat
    vec = 16 // DT[dn].itemsize
    sizes = (1, vec - 1, vec, vec + 1, 2 * vec + 1, 1024 * vec - 1, 1024 * vec + 1, 4096 * vec - 1, 4096 * vec + 1)
    src = _randn(dn, max(sizes))
    buf = torch.empty_like(src)
    got, want, counted, expected = [], [], [], []
    for head in range(vec):
        off = (vec - head) % vec  # `head` elements lie between buf[off] and the next 16-byte boundary
        for n in sizes:
            if n <= head:
                continue
            x = buf[off:off + n]
            x.copy_(src[:n])
            x[0] = -9.0 if abs_key else 9.0   # the largest key on the first element ...
            x[n - 1] = 0.0 if abs_key else -9.0   # ... the smallest on the last
            assert (-x.data_ptr() % 16) // x.element_size() == head
            for i, k in enumerate((1, (n + 1) // 2, n)):
                sums = [] if i == 0 else None
                got.append(_run(nat.KthWideSteps(x, abs_key, nat.KTH_EXPLICIT, 0.0, k=k), sums).float().reshape(()))
                want.append(_kth(x, k, abs_key))
                if sums:  # every element counted exactly once: a lucky rank can hide one counted twice or not at all
                    counted += sums
                    expected.append(n)
    assert torch.equal(torch.stack(counted).cpu(), torch.tensor(expected))
    assert torch.equal(torch.stack(got), torch.stack(want))


@DTYPES
@pytest.mark.parametrize('value,abs_key', [(-math.inf, False), (0.0, True), (math.nan, False), (math.nan, True)],
                         ids=['neginf-signed', 'zero-abs', 'nan-signed', 'nan-abs'])
def test_pick_edges(dn, value, abs_key):
    """constant tensors of the smallest and of the largest key: the rank lies in the first bins of thread 0 or in the
    last bin of the last thread, whichever rank is asked"""
    from brevitas_amd import _native as nat
    for outer, ch, inner in ((1, 1, 1000), (4, 5, 250)):
        n = outer * inner
        x = torch.full((outer * ch * inner,), value, device=DEV, dtype=DT[dn])
        want = _kth(x[:n], 1, abs_key).nan_to_num(nan=777.0).expand(ch)
        for k in (1, n):
            routes = [nat.KthSelectSteps(x, outer, ch, inner, abs_key, nat.KTH_EXPLICIT, 0.0, k=k)]
            if ch == 1:
                routes.append(nat.KthWideSteps(x, abs_key, nat.KTH_EXPLICIT, 0.0, k=k))
            for steps in routes:
                assert torch.equal(_run(steps).float().nan_to_num(nan=777.0), want), (type(steps).__name__, ch, k)


def _top15(v, abs_key):
    """the 15-bit first digit of the select's key of a finite value"""
    wide = v.dtype == torch.float32
    bits = 32 if wide else 16
    b = v.view(torch.int32 if wide else torch.int16).to(torch.int64) & ((1 << bits) - 1)
    if abs_key:
        return (b & ((1 << (bits - 1)) - 1)) >> (bits - 1 - 15)
    return torch.where(b >> (bits - 1) == 1, b ^ ((1 << bits) - 1), b ^ (1 << (bits - 1))) >> (bits - 15)


@DTYPES
@KEYS
@pytest.mark.parametrize('n', [1 << 22, (1 << 22) + 3])
def test_one_shot_equals_stepwise_equals_digit_passes(dn, abs_key, n):
    from brevitas_amd import _native as nat
    x = _randn(dn, (1 << 22) + 3)[:n]
    bits = lambda t: t.view(torch.int32 if dn == 'f32' else torch.int16)  # noqa: E731
    for k in (1, n // 3, n):
        one = nat.kth_value(x, k, 1, 1, n, abs_key)
        assert one.float().item() == _kth(x, k, abs_key).item(), k
        wide = _run(nat.KthWideSteps(x, abs_key, nat.KTH_EXPLICIT, 0.0, k=k))
        digits = _run(nat.KthSelectSteps(x, 1, 1, n, abs_key, nat.KTH_EXPLICIT, 0.0, k=k))
        assert torch.equal(bits(one), bits(wide)) and torch.equal(bits(one), bits(digits)), k
    # two ranks from one histogram read: neighbours in one 15-bit bin (values near 1: one sign, one exponent), and
    # equal ranks
    k = int(0.85 * n)
    for k1, k2 in ((k, k + 1), (k, k)):
        both = nat.kth_pair(x, k1, k2, 1, 1, n, abs_key)
        assert torch.equal(_top15(both[0], abs_key), _top15(both[1], abs_key))
        assert torch.equal(bits(both[0]), bits(nat.kth_value(x, k1, 1, 1, n, abs_key))), (k1, k2)
        assert torch.equal(bits(both[1]), bits(nat.kth_value(x, k2, 1, 1, n, abs_key))), (k1, k2)


def test_argument_checks_return_before_any_launch():
    """every refusal below is decided on the host: the pointers are real device buffers, and none is ever used"""
    from brevitas_amd import _native as nat
    lib, F32, BAD = nat.lib, nat.F32, 7
    EXPLICIT, HIGH = nat.KTH_EXPLICIT, nat.KTH_HIGH
    # the queries
    assert lib.bvq_kth_workspace_bytes(BAD, 1, 1, 8) == -1 and lib.bvq_kth_workspace_bytes(F32, -1, 1, 8) == -1
    assert lib.bvq_kth_workspace_bytes(F32, 1, 0, 8) == -1 and lib.bvq_kth_workspace_bytes(F32, 1, 1, -8) == -1
    assert lib.bvq_kth_passes(BAD) == -1 and lib.bvq_kth_passes(-1) == -1
    assert lib.bvq_kth_hist_offset(BAD, 1, 0) == -1 and lib.bvq_kth_hist_offset(F32, 0, 0) == -1
    assert lib.bvq_kth_hist_offset(F32, 1, -1) == -1 and lib.bvq_kth_hist_offset(F32, 1, 3) == -1
    assert lib.bvq_kth_hist_offset(nat.BF16, 1, 2) == -1
    assert lib.bvq_kthw_plan(1, BAD, 0, None, None) == -1 and lib.bvq_kthw_plan(0, -1, -1, None, None) == -1

    # rows of 512 bytes: the row-mapped layout, whose workspace is the select's state alone
    outer, ch, inner = 2, 3, 128
    n = outer * inner
    x = torch.zeros(outer * ch * inner, device=DEV)
    out = torch.zeros(2 * ch, device=DEV)
    need = lib.bvq_kth_workspace_bytes(F32, outer, ch, inner)
    need1 = lib.bvq_kth_workspace_bytes(F32, 1, 1, n)
    ws = torch.zeros(max(need, need1), dtype=torch.uint8, device=DEV)
    X, O, W = x.data_ptr(), out.data_ptr(), ws.data_ptr()

    # one caller per launching entry: dtype, workspace and its size first, what else it can refuse by keyword
    def begin(dt, w, wsb, rule=EXPLICIT, k=1, q=0.0):
        return lib.bvq_kth_begin(dt, ch, rule, k, q, w, wsb, None)

    def hist(dt, w, wsb, p=0):
        return lib.bvq_kth_hist(1, dt, X, outer, ch, inner, p, w, wsb, None)

    def pick(dt, w, wsb, p=0, rule=EXPLICIT):
        return lib.bvq_kth_pick(dt, ch, p, rule, 0.0, w, wsb, None)

    def finish(dt, w, wsb, o=O):
        return lib.bvq_kth_finish(1, dt, ch, o, w, wsb, None)

    def wbegin(dt, w, wsb):
        return lib.bvq_kthw_begin(0, dt, w, wsb, None)

    def whist(dt, w, wsb, p=0, count=n):
        return lib.bvq_kthw_hist(0, dt, X, count, p, w, wsb, None)

    def wpick(dt, w, wsb, p=0, rule=EXPLICIT, k=1, q=0.0, abs_key=0):
        return lib.bvq_kthw_pick(abs_key, dt, p, rule, k, q, w, wsb, None)

    def wfinish(dt, w, wsb, o=O):
        return lib.bvq_kthw_finish(0, dt, o, w, wsb, None)

    def value(dt, w, wsb, k=1, xp=X, o=O):
        return lib.bvq_kth_value(1, dt, xp, outer, ch, inner, k, o, w, wsb, None)

    def pair(dt, w, wsb, k1=1, k2=n, xp=X, o=O):
        return lib.bvq_kth_pair(1, dt, xp, outer, ch, inner, k1, k2, o, w, wsb, None)

    for step, size in ((begin, need), (hist, need), (pick, need), (finish, need),
                       (wbegin, need1), (whist, need1), (wpick, need1), (wfinish, need1)):
        assert step(BAD, W, size) == ERR_INVALID, step.__name__
        assert step(F32, None, size) == ERR_WORKSPACE, step.__name__
        assert step(F32, W, size - 1) == ERR_WORKSPACE, step.__name__
    for entry in (value, pair):
        assert entry(BAD, W, need) == ERR_INVALID, entry.__name__
        assert entry(F32, None, need) == ERR_INVALID, entry.__name__   # ("null pointer", with x and out)
        assert entry(F32, W, need - 1) == ERR_WORKSPACE, entry.__name__
        assert entry(F32, W, need, xp=None) == ERR_INVALID and entry(F32, W, need, o=None) == ERR_INVALID
    # pass
    for step, passes in ((hist, 3), (pick, 3), (whist, 2), (wpick, 2)):
        assert step(F32, W, need1 if step in (whist, wpick) else need, p=-1) == ERR_INVALID, step.__name__
        assert step(F32, W, need1 if step in (whist, wpick) else need, p=passes) == ERR_INVALID, step.__name__
    assert wpick(nat.BF16, W, need1, p=1, abs_key=1) == ERR_INVALID   # |x| of a 16-bit type has one pass
    # rule, percentile and rank
    for rule in (-1, 3):
        assert begin(F32, W, need, rule=rule) == ERR_INVALID and pick(F32, W, need, rule=rule) == ERR_INVALID
        assert wpick(F32, W, need1, rule=rule) == ERR_INVALID and wpick(F32, W, need1, p=1, rule=rule) == ERR_INVALID
    assert begin(F32, W, need, k=0) == ERR_INVALID and wpick(F32, W, need1, k=0) == ERR_INVALID
    for q in (-0.5, 100.5, math.nan):
        assert begin(F32, W, need, rule=HIGH, q=q) == ERR_INVALID
        assert wpick(F32, W, need1, rule=HIGH, q=q) == ERR_INVALID
    assert value(F32, W, need, k=0) == ERR_INVALID and value(F32, W, need, k=n + 1) == ERR_INVALID
    for k1, k2 in ((0, 1), (1, 0), (n + 1, 1), (1, n + 1)):
        assert pair(F32, W, need, k1=k1, k2=k2) == ERR_INVALID, (k1, k2)
    # the other refusals of the entries above
    assert finish(F32, W, need, o=None) == ERR_INVALID and wfinish(F32, W, need1, o=None) == ERR_INVALID
    assert whist(F32, W, need1, count=-1) == ERR_INVALID and whist(F32, W, need1, count=1 << 32) == ERR_UNSUPPORTED
    assert lib.bvq_kth_hist(1, F32, X, -1, ch, inner, 0, W, need, None) == ERR_INVALID
    assert lib.bvq_kth_hist(1, F32, None, outer, ch, inner, 0, W, need, None) == ERR_INVALID
    assert lib.bvq_kth_hist(1, F32, X, 1 << 16, ch, 1 << 16, 0, W, need, None) == ERR_UNSUPPORTED
    assert lib.bvq_kthw_hist(0, F32, None, n, 0, W, need1, None) == ERR_INVALID
    assert lib.bvq_kth_value(1, F32, X, 1 << 16, ch, 1 << 16, 1, O, W, need, None) == ERR_UNSUPPORTED
    # the per-tensor route's own workspace check: 2^22 elements on a 16-byte boundary, one byte short
    big = 1 << 22
    assert X % 16 == 0
    short = lib.bvq_kth_workspace_bytes(F32, 1, 1, big) - 1
    assert lib.bvq_kth_value(1, F32, X, 1, 1, big, 1, O, W, short, None) == ERR_WORKSPACE
    assert lib.bvq_kth_pair(1, F32, X, 1, 1, big, 1, big, O, W, short, None) == ERR_WORKSPACE
