"""The host layer of the per-unit families (brevitas_amd._native.UNIT_FAMILIES) against stand-ins, no GPU.

The binding: the public wrappers <stem>_supported / _fwd / _bwd, through unit_fwd / unit_bwd, hand every entry exactly
the arguments of its _SIG row in the header's order, the stream last, and allocate the outputs the family's record names.
The Functions of core/quant/_fused.py: with the two wrappers replaced by recording stand-ins, they shape the outputs,
save and hand back the tensors the record names, and prepare the gradients as the record says."""
import ctypes
import inspect

import pytest
import torch

STREAM = 0x5EED
MIN_VAL = 1e-10
DT = torch.bfloat16
STEMS = ['group_quant', 'group_mse', 'group_shifted', 'row_shifted']
families = pytest.mark.parametrize('stem', STEMS)
# what each Function hands on after y, and which of it flat and non-differentiable
FUNCTION = {'group_quant': ('GroupStatsFakeQuantFn', ('scale',), ()),
            'group_mse': ('GroupMSEFakeQuantFn', ('scale', 'idx'), ('idx',)),
            'group_shifted': ('GroupShiftedFakeQuantFn', ('scale', 'zp'), ()),
            'row_shifted': ('RowShiftedFakeQuantFn', ('scale', 'zp'), ())}


class _Lib:
    """every entry records its arguments and succeeds"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith('bvq_'):
            raise AttributeError(name)
        return lambda *args: self.calls.append((name, args)) or 0


@pytest.fixture
def nat(monkeypatch):
    from brevitas_amd import _native
    monkeypatch.setattr(_native, 'lib', _Lib())
    monkeypatch.setattr(_native, 'stream_ptr', lambda dev: STREAM)
    monkeypatch.setattr(_native, '_timer', None)
    monkeypatch.setattr(_native, 'require_device', lambda *tensors: torch.device('cpu'))  # no index: no guard
    return _native


def _family(nat, stem):
    fam = getattr(nat, stem.upper())
    assert (fam.supported, fam.fwd, fam.bwd) == tuple('bvq_%s_%s' % (stem, way) for way in ('supported', 'fwd', 'bwd'))
    return fam


def _x(stem):
    """[4, 64] in groups of 32 for the group families, [3, 136] for the row family -> (x, unit length, units)"""
    if stem.startswith('row'):
        return torch.randn(3, 136).to(DT), 136, 3
    return torch.randn(4, 64).to(DT), 32, 8


def _desc(fam, x, unit_len):
    from brevitas_amd.core.quant import _fused
    qmax = 15.0 if fam.zp_per_unit else 7.0
    return _fused.unit_call(x, unit_len, fam.zp_per_unit, qmax, 0.0 if fam.zp_per_unit else -qmax, qmax, True)


def _public_extra(nat, fam):
    """what the public wrappers take for the record's extra host arguments, and what the entry must receive"""
    if not fam.extra:
        return (), ()
    assert fam.extra == ('ratios', 'n_ratios')
    table = nat.mse_ratio_table([1.0, 0.5])
    return (table,), (ctypes.addressof(table), 2)


def test_the_table_names_the_four_families_and_their_wrappers(nat):
    assert [f.fwd for f in nat.UNIT_FAMILIES] == ['bvq_%s_fwd' % s for s in STEMS]
    for stem in STEMS:
        fam = _family(nat, stem)
        names = [o.name for o in fam.outs]
        assert set(fam.saved) <= set(names) and len(fam.side) <= len(FUNCTION[stem][1])
        for entry in (fam.supported, fam.fwd, fam.bwd):
            assert entry in nat._SIG and callable(getattr(nat, entry[4:]))


@families
@pytest.mark.parametrize('min_val, use_min', [(None, 0), (0, 0), (0.0, 0), (MIN_VAL, 1)])
def test_forward_arguments_follow_the_header(nat, stem, min_val, use_min):
    fam = _family(nat, stem)
    x, unit_len, units = _x(stem)
    desc, thr = _desc(fam, x, unit_len)
    pub, raw = _public_extra(nat, fam)
    y, *outs = getattr(nat, stem + '_fwd')(desc, x, *pub, min_val, thr)
    (name, args), = nat.lib.calls
    assert name == fam.fwd
    assert len(args) == len(nat._SIG[name][1]) and args[-1] == STREAM
    assert args[0]._obj is desc and args[1] == x.data_ptr()
    assert args[2:2 + len(raw)] == raw
    assert args[2 + len(raw):5 + len(raw)] == (float(min_val or 0.0), use_min, float(thr))
    assert args[5 + len(raw):-1] == tuple(t.data_ptr() for t in [y] + outs)
    assert y.shape == x.shape and y.dtype == x.dtype and y.data_ptr() != x.data_ptr()
    assert len(outs) == len(fam.outs)
    for o, t in zip(fam.outs, outs):
        assert t.shape == (o.per_unit * units,) and t.dtype == (o.dtype or x.dtype), o.name


@families
@pytest.mark.parametrize('min_val, use_min', [(None, 0), (0, 0), (MIN_VAL, 1)])
def test_backward_arguments_follow_the_header(nat, stem, min_val, use_min):
    fam = _family(nat, stem)
    x, unit_len, units = _x(stem)
    desc, thr = _desc(fam, x, unit_len)
    pub, raw = _public_extra(nat, fam)
    out = dict(zip([o.name for o in fam.outs], nat.unit_fwd(fam, desc, x, *raw, min_val, thr)[1:]))
    saved = [out[n] for n in fam.saved]
    side = [torch.zeros(units, dtype=DT)] + [None] * (len(fam.side) - 1)
    g = torch.ones_like(x)
    nat.lib.calls.clear()
    dx = getattr(nat, stem + '_bwd')(desc, g, x, *saved, *side, *pub, min_val, thr)
    (name, args), = nat.lib.calls
    assert name == fam.bwd
    assert len(args) == len(nat._SIG[name][1]) and args[-1] == STREAM
    assert args[0]._obj is desc and args[1:3] == (g.data_ptr(), x.data_ptr())
    k = 3 + len(saved)
    assert args[3:k] == tuple(t.data_ptr() for t in saved)
    assert args[k:k + len(side)] == tuple(None if s is None else s.data_ptr() for s in side)
    k += len(side)
    assert args[k:k + len(raw)] == raw
    k += len(raw)
    assert args[k:-1] == (float(min_val or 0.0), use_min, float(thr), dx.data_ptr())
    assert dx.shape == x.shape and dx.dtype == x.dtype


@families
def test_supported_hands_on_descriptor_tensor_and_extras(nat, stem):
    fam = _family(nat, stem)
    x, unit_len, _ = _x(stem)
    desc, _ = _desc(fam, x, unit_len)
    extra = (2,) if fam.extra else ()  # group_mse_supported takes the candidate count alone
    assert getattr(nat, stem + '_supported')(desc, x, *extra) is False  # the stand-in answers 0
    (name, args), = nat.lib.calls
    assert name == fam.supported and len(args) == len(nat._SIG[name][1])
    assert args[0]._obj is desc and args[1:] == (x.data_ptr(),) + extra


def test_the_wrappers_keep_their_asserts(nat):
    x, unit_len, units = _x('group_mse')
    desc, thr = _desc(nat.GROUP_MSE, x, unit_len)
    table = nat.mse_ratio_table([1.0, 0.5])
    stat, gs = torch.zeros(units, dtype=DT), torch.zeros(2 * units, dtype=DT)[::2]
    with pytest.raises(AssertionError):
        nat.group_quant_fwd(desc, x.t(), MIN_VAL, thr)
    with pytest.raises(AssertionError):  # idx must be uint8
        nat.group_mse_bwd(desc, x, x, stat, torch.zeros(units, dtype=torch.int32), None, table, MIN_VAL, thr)
    with pytest.raises(AssertionError):  # a strided side gradient
        nat.group_quant_bwd(desc, x, x, stat, stat, gs, MIN_VAL, thr)
    with pytest.raises(AssertionError):  # a strided saved tensor
        nat.group_shifted_bwd(desc, x, x, torch.zeros(4 * units, dtype=DT)[::2], None, None, MIN_VAL, thr)
    with pytest.raises(AssertionError):  # a strided gradient
        nat.row_shifted_bwd(desc, x.t(), x, torch.zeros(2 * units, dtype=DT), None, None, MIN_VAL, thr)
    with pytest.raises(AssertionError):  # an argument short
        nat.group_shifted_bwd(desc, x, x, torch.zeros(2 * units, dtype=DT), None, MIN_VAL, thr)
    assert nat.lib.calls == []


# ---- the Functions ------------------------------------------------------------------------------------------------

def _function(stem):
    from brevitas_amd.core.quant import _fused
    return getattr(_fused, FUNCTION[stem][0])


class _Wrappers:
    """recording stand-ins of a family's two wrappers, returning CPU tensors shaped as the record says"""

    def __init__(self, monkeypatch, nat, stem, units):
        self.fam, self.units, self.fwd_calls, self.bwd_calls, self.outs = _family(nat, stem), units, [], [], None
        monkeypatch.setattr(nat, stem + '_fwd', self.fwd)
        monkeypatch.setattr(nat, stem + '_bwd', self.bwd)

    def fwd(self, desc, x, *rest):
        self.fwd_calls.append((desc, x) + rest)
        self.outs = {o.name: torch.full((o.per_unit * self.units,), 2, dtype=o.dtype or x.dtype) for o in self.fam.outs}
        return (x * 2, *self.outs.values())

    def bwd(self, desc, g, x, *rest):
        self.bwd_calls.append((desc, g, x) + rest)
        return torch.full_like(x, 3)


def _apply(nat, stem, x, unit_len):
    """-> (the Function's outputs, what the wrappers must see behind x / the side gradients)"""
    fam = _family(nat, stem)
    qmax = 15.0 if fam.zp_per_unit else 7.0
    args = (MIN_VAL, qmax, 0.0 if fam.zp_per_unit else -qmax, qmax, True)
    if not stem.startswith('row'):
        args = (unit_len,) + args
    extra = (nat.mse_ratio_table([1.0, 0.5]),) if fam.extra else ()
    return _function(stem).apply(x, *args, *extra), extra


def _misaligned(units):
    """a [units, 1] gradient whose memory is 2 bytes past a 16-byte boundary"""
    base = torch.ones(units + 16, dtype=DT)
    off = next(i for i in range(16) if base[i:].data_ptr() % 16 == 2)
    return base[off:off + units].view(-1, 1)


@families
def test_function_forward_shapes_its_outputs(nat, monkeypatch, stem):
    x, unit_len, units = _x(stem)
    w = _Wrappers(monkeypatch, nat, stem, units)
    x.requires_grad_(True)
    (y, *ret), extra = _apply(nat, stem, x, unit_len)
    (call,) = w.fwd_calls
    desc, thr = _desc(w.fam, x, unit_len)
    assert bytes(call[0]) == bytes(desc) and call[1] is x and call[2:] == extra + (MIN_VAL, thr)
    _, returns, nondiff = FUNCTION[stem]
    assert y.shape == x.shape and y.requires_grad and len(ret) == len(returns)
    for name, t in zip(returns, ret):
        assert t.data_ptr() == w.outs[name].data_ptr(), name
        if name in nondiff:
            assert t.shape == (units,) and not t.requires_grad, name
        else:
            assert t.shape == (units, 1) and t.requires_grad, name


@families
def test_function_backward_hands_back_what_the_record_saves(nat, monkeypatch, stem):
    x, unit_len, units = _x(stem)
    w = _Wrappers(monkeypatch, nat, stem, units)
    x.requires_grad_(True)
    (y, *ret), extra = _apply(nat, stem, x, unit_len)
    g = torch.randn(x.shape).to(DT)
    y.backward(g)  # a wrong number of returned values would raise here
    (call,) = w.bwd_calls
    desc, thr = _desc(w.fam, x, unit_len)
    assert bytes(call[0]) == bytes(desc) and torch.equal(call[1], g) and call[2].data_ptr() == x.data_ptr()
    k = 3 + len(w.fam.saved)
    assert [t.data_ptr() for t in call[3:k]] == [w.outs[n].data_ptr() for n in w.fam.saved]
    assert call[k:] == (None,) * len(w.fam.side) + extra + (MIN_VAL, thr)
    assert torch.equal(x.grad, torch.full_like(x, 3))


@families
def test_function_backward_without_gy_and_with_a_misaligned_side_gradient(nat, monkeypatch, stem):
    x, unit_len, units = _x(stem)
    w = _Wrappers(monkeypatch, nat, stem, units)
    fam = w.fam
    x.requires_grad_(True)
    (y, *ret), extra = _apply(nat, stem, x, unit_len)
    gside = _misaligned(units)
    last = len(fam.side) - 1  # the last side output alone: scale for one, zero-point for two
    torch.autograd.backward([ret[last]], [gside])
    (call,) = w.bwd_calls
    gy = call[1]
    assert gy.shape == x.shape and gy.dtype == x.dtype and not gy.any() and gy.data_ptr() % 16 == 0
    k = 3 + len(fam.saved)
    side = call[k:k + len(fam.side)]
    assert all(s is None for s in side[:last])
    got = side[last]
    assert got.shape == (units,) and got.dtype == x.dtype and got.is_contiguous() and torch.equal(got, gside.view(-1))
    if fam.align_side:
        assert got.data_ptr() % 16 == 0
    else:
        assert got.data_ptr() == gside.data_ptr()
    assert call[k + len(fam.side):] == extra + (MIN_VAL, _desc(fam, x, unit_len)[1])


@families
def test_function_backward_returns_one_value_per_forward_input(nat, monkeypatch, stem):
    x, unit_len, units = _x(stem)
    w = _Wrappers(monkeypatch, nat, stem, units)
    fn = _function(stem)
    n_in = len(inspect.signature(fn.forward).parameters) - 1

    class Ctx:
        saved_tensors = (x,) + tuple(torch.zeros(units, dtype=DT) for _ in w.fam.saved)
        desc, min_val, thr_div, table = None, MIN_VAL, 1.0, None

    nothing = (None,) * len(FUNCTION[stem][1])
    assert fn.backward(Ctx, None, *nothing) == (None,) * n_in and not w.bwd_calls
    out = fn.backward(Ctx, torch.ones_like(x), *nothing)
    assert len(out) == n_in and out[1:] == (None,) * (n_in - 1) and torch.equal(out[0], torch.full_like(x, 3))


def test_the_functions_look_the_wrappers_up_when_called(nat, monkeypatch):
    """tests count launches by patching nat.<stem>_fwd after import: a Function must not hold the function object"""
    x, unit_len, units = _x('group_quant')
    w = _Wrappers(monkeypatch, nat, 'group_quant', units)
    count = []
    monkeypatch.setattr(nat, 'group_quant_fwd', lambda *a: count.append(1) or w.fwd(*a))
    _apply(nat, 'group_quant', x, unit_len)
    assert count == [1]
