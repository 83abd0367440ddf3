"""WeightQuantGroup and the list entries of the C ABI (include/bvq.h, bvq_weight_quant_list_*) without a GPU: a group
over a CPU model changes nothing, the new entries reject bad arguments before touching a device, and the item struct
of the Python binding has the header's layout."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model():
    import brevitas_amd.quant as Q
    from brevitas_amd.nn import QuantConv2d, QuantLinear

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.c1 = QuantConv2d(3, 8, 3, padding=1, weight_quant=Q.Int8WeightPerChannelFloat)
            self.c2 = QuantConv2d(8, 8, 1, weight_quant=Q.Int4WeightPerChannelFloat)
            self.c3 = QuantConv2d(8, 8, 3, padding=1, weight_quant=Q.Int8WeightPerTensorFloat)
            self.fc = QuantLinear(8, 5, weight_quant=Q.Int8WeightPerChannelFloat)

        def forward(self, x):
            x = self.c3(self.c2(self.c1(x)))
            return self.fc(x.mean((2, 3)))

    return Net()


def _step(model, x, group=None):
    model.zero_grad(set_to_none=True)
    if group is not None:
        with group:
            out = model(x)
    else:
        out = model(x)
    out.sum().backward()
    return out.detach(), {n: p.grad.clone() for n, p in model.named_parameters()}


def test_group_over_a_cpu_model_changes_nothing():
    from brevitas_amd import WeightQuantGroup
    torch.manual_seed(0)
    model = _model()
    keys = list(model.state_dict().keys())
    x = torch.randn(2, 3, 8, 8)
    out0, g0 = _step(model, x)
    group = WeightQuantGroup(model)
    assert group.covered == []
    reasons = dict(group.uncovered)
    assert reasons['c1.weight_quant'] == 'weight on the CPU'
    assert reasons['c3.weight_quant'] == 'per-tensor scale'
    out1, g1 = _step(model, x, group)
    assert torch.equal(out0, out1)
    assert g0.keys() == g1.keys() and all(torch.equal(g0[k], g1[k]) for k in g0)
    assert list(model.state_dict().keys()) == keys
    # the block leaves nothing behind
    from brevitas_amd.core.quant import int as qint
    assert qint._ACTIVE_GROUP is None and group._results is None


def test_list_entries_reject_bad_arguments_without_a_device():
    from brevitas_amd import _native as nat
    lib = nat.lib
    items = (nat.WeightItem * (nat.WEIGHT_LIST_MAX + 1))()
    buf = torch.empty(1024, dtype=torch.float32)  # host memory: nothing may read it
    for it in items:
        it.x = it.y = it.stat = it.scale = it.g = it.dx = it.dscale = buf.data_ptr()
        it.channels, it.inner, it.qmin, it.qmax = 4, 8, -128.0, 127.0
    addr = ctypes.addressof(items)
    fwd = lambda dt, n, a: lib.bvq_weight_quant_list_fwd(dt, nat.F32, nat.ROUND, n, a, None)  # noqa: E731
    bwd = lambda dt, n, a: lib.bvq_weight_quant_list_bwd(dt, nat.F32, nat.F32, nat.ROUND, n, a,  # noqa: E731
                                                         buf.data_ptr(), 4096, buf.data_ptr(), 1024, None)
    for call in (fwd, bwd):
        for dt, n, a, msg in ((nat.F32, 0, addr, 'items'), (nat.F32, nat.WEIGHT_LIST_MAX + 1, addr, 'items'),
                              (nat.F32, 1, None, 'null'), (7, 1, addr, 'bad dtype'), (-1, 1, addr, 'bad dtype')):
            assert call(dt, n, a) == -1, (call, dt, n, a)
            assert msg in nat.last_error()
    items[0].y = None
    assert fwd(nat.F32, 1, addr) == -1 and 'null pointer' in nat.last_error()
    items[1].g = None
    assert bwd(nat.F32, 2, addr) == -1 and 'null pointer' in nat.last_error()
    assert lib.bvq_weight_quant_list_bwd(nat.F32, nat.F32, 9, nat.ROUND, 1, addr, buf.data_ptr(), 4096, buf.data_ptr(),
                                         1024, None) == -1
    assert lib.bvq_weight_quant_list_bwd_workspace_bytes(nat.F32, 0, addr) == -1
    assert lib.bvq_weight_quant_list_bwd_workspace_bytes(9, 1, addr) == -1
    assert lib.bvq_weight_list_supported(nat.F32, nat.ROUND, 0, addr, 0) == 0
    assert lib.bvq_weight_list_supported(nat.F32, nat.ROUND, nat.WEIGHT_LIST_MAX + 1, addr, 0) == 0
    assert lib.bvq_weight_list_supported(5, nat.ROUND, 1, addr, 0) == 0
    assert lib.bvq_weight_list_supported(nat.F32, nat.ROUND, 1, None, 0) == 0


def test_list_coverage_rules():
    """host-side coverage (no device is touched: the pointers are only checked for alignment)"""
    from brevitas_amd import _native as nat
    items = (nat.WeightItem * 3)()
    for it, (c, inner) in zip(items, ((256, 1024), (64, 576), (1000, 2048))):
        it.x, it.channels, it.inner, it.qmin, it.qmax = 1 << 20, c, inner, -128.0, 127.0
    addr = ctypes.addressof(items)
    for dt in (nat.F32, nat.BF16, nat.F16):
        assert nat.lib.bvq_weight_list_supported(dt, nat.ROUND, 3, addr, 0) == 1, dt
    assert nat.lib.bvq_weight_list_supported(nat.F32, nat.FLOOR, 3, addr, 0) == 0      # no one-launch backward
    assert nat.lib.bvq_weight_list_supported(nat.F32, nat.ROUND, 3, addr, 1000) == 0   # arrival buffer too small
    items[1].x = (1 << 20) + 4                                                         # misaligned
    assert nat.lib.bvq_weight_list_supported(nat.F32, nat.ROUND, 3, addr, 0) == 0
    items[1].x, items[1].inner = 1 << 20, 147                                          # ragged rows ([64,3,7,7])
    assert nat.lib.bvq_weight_list_supported(nat.F32, nat.ROUND, 3, addr, 0) == 0
    items[1].inner, items[1].channels = 1 << 20, 4                                     # a channel beyond 8 waves
    assert nat.lib.bvq_weight_list_supported(nat.F32, nat.ROUND, 3, addr, 0) == 0
    assert nat.lib.bvq_weight_quant_list_bwd_workspace_bytes(nat.F32, 1, addr) > 256


def _header_struct_fields(name):
    text = open(os.path.join(ROOT, 'include', 'bvq.h')).read()
    body = re.search(r'typedef struct %s \{(.*?)\} %s;' % (name, name), text, flags=re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = []
    for decl in body.split(';'):
        decl = decl.strip()
        if decl:
            m = re.match(r'(.*?)([A-Za-z_][A-Za-z0-9_]*)$', decl)
            fields.append((m.group(2), re.sub(r'\s+', ' ', m.group(1).strip())))
    return fields


def test_weight_item_layout_matches_header(tmp_path):
    """the ctypes struct has the header's fields in the header's order and kinds, and the C compiler agrees on every
    offset and the size"""
    from brevitas_amd import _native as nat
    fields = _header_struct_fields('bvq_weight_item')
    assert [n for n, _ in fields] == [n for n, _ in nat.WeightItem._fields_]
    kinds = {'int64_t': ctypes.c_int64, 'int32_t': ctypes.c_int32, 'double': ctypes.c_double, 'float': ctypes.c_float}
    for (name, ctype), (pname, ptype) in zip(fields, nat.WeightItem._fields_):
        want = ctypes.c_void_p if ctype.endswith('*') else kinds[ctype]
        assert ptype is want, (name, ctype, ptype)
    src = tmp_path / 'layout.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bvq.h"\nint main(void) {\n'
                   '  printf("%zu\\n", sizeof(bvq_weight_item));\n' +
                   ''.join('  printf("%%zu\\n", offsetof(bvq_weight_item, %s));\n' % n for n, _ in fields) +
                   '  printf("%d\\n", BVQ_WEIGHT_LIST_MAX);\n  return 0;\n}\n')
    exe = tmp_path / 'layout'
    cc = next((c for c in ('cc', 'gcc', 'clang') if subprocess.run(['which', c], capture_output=True).returncode == 0),
              None)
    if cc is None:
        pytest.skip('no C compiler')
    subprocess.run([cc, '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == ctypes.sizeof(nat.WeightItem)
    assert got[1:-1] == [getattr(nat.WeightItem, n).offset for n, _ in fields]
    assert got[-1] == nat.WEIGHT_LIST_MAX


def test_chunks_respect_the_list_size_and_the_arrival_buffer():
    """a chunk (one list call each way) holds at most WEIGHT_LIST_MAX weights whose channels fit one arrival buffer"""
    from types import SimpleNamespace
    from brevitas_amd import _native as nat
    from brevitas_amd.core.quant import _fused
    from brevitas_amd.core.quant.weight_group import _Entry, _WeightList

    def entries(channels):
        quant = SimpleNamespace(int_scaling_impl=lambda bw: bw)
        tmpl = SimpleNamespace(qmin=-128.0, qmax=127.0, round_mode=nat.ROUND, clamp_ste=True)
        return [_Entry(None, quant, torch.empty(c, 8), _fused.StatsPlan(1, c, 8, (c, 1), 1e-8, 127.0), tmpl,
                       torch.tensor(8.0)) for c in channels]

    wl = _WeightList(entries([64] * 40))
    assert wl.chunks == [(0, 16), (16, 32), (32, 40)]
    big = nat.ARRIVE_WORDS // 4 + 1   # four of them overflow one arrival buffer
    wl = _WeightList(entries([big] * 10 + [8] * 3))
    assert wl.chunks == [(0, 3), (3, 6), (6, 9), (9, 13)]
    for lo, hi in wl.chunks:
        assert sum(wl.channels[lo:hi]) <= nat.ARRIVE_WORDS and hi - lo <= nat.WEIGHT_LIST_MAX
        assert [wl.chunk_of[i] for i in range(lo, hi)] == [wl.chunks.index((lo, hi))] * (hi - lo)
        assert wl.offsets[lo:hi] == [sum(wl.channels[lo:i]) for i in range(lo, hi)]
