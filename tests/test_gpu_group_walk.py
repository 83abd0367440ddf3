"""The sub-wave group walk (csrc/bvq_group_walk.h) where it can go wrong: one group below, on and one group above every
load, window and workgroup boundary of each L = g * sizeof(T) / 16; every NT = true instantiation through the forced-NT
build of the library (brevitas_amd/libbvq_nt0.so, made by __graft_entry__.build()); and the backward branches of the
two autograd Functions that no other test reaches on a device.  The six entry points are called through their
brevitas_amd._native wrappers: group_quant_fwd / bwd, mx_quant_fwd / bwd, mx_encode, mx_decode; the asymmetric kernels
(group_shifted_fwd / bwd) through their quantizer module.

No bar of its own.  MX: y and scale bit for bit against the numpy oracle, dx by assert_dx of test_mx_quant_host.py; codes
and scale bytes byte for byte against the numpy encoder of test_mx_pack_host.py, the decoder against the device forward.
Group-wise integer: y and scale bit for bit against the CPU oracle and the per-channel route on the regrouped weight, dw
by assert_dw of test_gpu_group_quant.py with its derived deposit_ulps.  Asymmetric: y, scale and zp bit for bit against
the per-channel route on the regrouped weight, dw by compare of test_gpu_group_shifted.py.
"""
import functools

import pytest
import torch

import golden_util as G
import test_gpu_group_quant as GQ
import test_gpu_group_shifted as GS
import test_mx_pack_host as P
import test_mx_quant_host as H
from test_group_walk_host import FWD_DEPTH, LANES, NT_BYTES, WAVES, edge_counts, lanes_per_group, nt0_path
from test_gpu_mx_quant import untie
from test_mx_quant_host import DT

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NT_GROUPS = 517       # odd, ragged in every L, several windows
dtypes = pytest.mark.parametrize('dn', ['f32', 'bf16', 'f16'])
edge_sizes = pytest.mark.parametrize('g', [16, 64, 256])      # L = 2, 8, 32 for 16-bit types, 4, 16, 64 for float32
all_sizes = pytest.mark.parametrize('g', [16, 32, 64, 128, 256])
MODES = (('floor', True), ('ceil', False))                     # (scale rule, clamp-STE)
PACK_FORMATS = ['e4m3', 'e2m3', 'e2m1']                        # the code widths 8, 6 and 4


def nat():
    from brevitas_amd import _native
    return _native


def bits_equal(a, b):
    """two device tensors of one dtype hold the same bits"""
    it = {4: torch.int32, 2: torch.int16, 1: torch.uint8}[a.element_size()]
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(a.view(it), b.view(it)))


# ---- the forced-NT variant ------------------------------------------------------------------------------------------

@functools.lru_cache(None)
def _nt0_lib():
    return nat()._load(nt0_path())


@pytest.fixture
def use_nt0(monkeypatch):
    """-> a function that switches brevitas_amd._native to the forced-NT library for the rest of the test"""
    lib = _nt0_lib()

    def switch():
        monkeypatch.setattr(nat(), 'lib', lib)
        assert nat().lib.bvq_nt_threshold_bytes() == 0, 'libbvq_nt0.so was not built with -DBVQ_NT_BYTES=0'
    return switch


@pytest.fixture
def launches(monkeypatch):
    """counts the launches of the six wrappers by name; 'grad_ptrs': the addresses of the gradients handed to the two
    backward wrappers (gy, then gscale or None), call by call"""
    n = nat()
    calls = {'grad_ptrs': []}

    def count(name):
        real = getattr(n, name)
        calls[name] = 0

        def counted(*a, **k):
            calls[name] += 1
            if name == 'mx_quant_bwd':      # (g, x, gscale, ...)
                calls['grad_ptrs'].append((a[0].data_ptr(), None if a[2] is None else a[2].data_ptr()))
            if name == 'group_quant_bwd':   # (desc, g, x, scale, stat, gscale, ...)
                calls['grad_ptrs'].append((a[1].data_ptr(), None if a[5] is None else a[5].data_ptr()))
            return real(*a, **k)
        monkeypatch.setattr(n, name, counted)
    for name in ('group_quant_fwd', 'group_quant_bwd', 'mx_quant_fwd', 'mx_quant_bwd', 'mx_encode', 'mx_decode',
                 'group_shifted_fwd', 'group_shifted_bwd'):
        count(name)
    return calls


# ---- MX: inputs, the device step, the bars --------------------------------------------------------------------------

@functools.lru_cache(None)
def mx_inputs(dn, g, groups):
    """(x, grad, gscale) on the CPU: randn * 3 without abs-max ties in any group, shared and left unchanged"""
    x, grad, gen = H.make_weight((groups * g,), dn)
    return untie(x, g), grad, torch.randn(groups, generator=gen)


def mx_code(fmt):
    from brevitas_amd.core.quant.mx import MX_FORMATS
    return MX_FORMATS[fmt].code


def mx_rule(rule):
    return {'floor': nat().MX_FLOOR, 'ceil': nat().MX_CEIL}[rule]


def mx_step(x, grad, gs, g, fmt, rule, ste):
    """forward and backward through the wrappers on device tensors -> (y, scale, dx)"""
    y, scale = nat().mx_quant_fwd(x, g, mx_code(fmt), mx_rule(rule))
    dx = nat().mx_quant_bwd(grad, x, gs, g, mx_code(fmt), mx_rule(rule), ste)
    return y, scale, dx


def check_mx(out, x, grad, gs, g, fmt, rule, ste, dn):
    """the bars of test_mx_quant_host.py on (y, scale, dx) -> the worst deposit difference in ulps"""
    y, scale, dx = (t.cpu() for t in out)
    H.check_forward(y, scale, H.oracle(x, g, fmt, rule))
    return H.assert_dx(dx, x, grad, gs, g, fmt, rule, ste, dn)


def pack_step(x, g, fmt, rule):
    """encode into outputs with 64 guard bytes behind each, decode them -> (code buffer, scale buffer, decoded)"""
    n = x.numel()
    nbytes, groups = n * P.BITS[fmt] // 8, n // g
    cbuf = torch.full((nbytes + 64,), 0xa5, dtype=torch.uint8, device=DEV)
    sbuf = torch.full((groups + 64,), 0xa5, dtype=torch.uint8, device=DEV)
    assert cbuf.data_ptr() % 16 == 0 and sbuf.data_ptr() % 16 == 0
    nat().mx_encode(x, g, mx_code(fmt), mx_rule(rule), codes=cbuf[:nbytes], scale_e8m0=sbuf[:groups])
    back = nat().mx_decode(cbuf[:nbytes], sbuf[:groups], g, mx_code(fmt), x.dtype)
    return cbuf, sbuf, back


def check_pack(out, x, y, g, fmt, rule):
    """guards untouched, bytes of the numpy encoder, the decoder gives the device forward's y"""
    cbuf, sbuf, back = (t.cpu() for t in out)
    n = x.numel()
    nbytes, groups = n * P.BITS[fmt] // 8, n // g
    assert bool((cbuf[nbytes:] == 0xa5).all()), torch.nonzero(cbuf[nbytes:] != 0xa5).reshape(-1).tolist()
    assert bool((sbuf[groups:] == 0xa5).all()), torch.nonzero(sbuf[groups:] != 0xa5).reshape(-1).tolist()
    codes, scale = P.numpy_encode(x, g, fmt, rule)
    P.assert_bytes(sbuf[:groups], scale, 'scale bytes')
    P.assert_bytes(cbuf[:nbytes], codes, 'codes')
    P.assert_round_trip(back, y.cpu(), fmt)


# ---- group-wise integer: inputs, the device step, the bars ----------------------------------------------------------

@functools.lru_cache(None)
def group_inputs(dn, g, groups):
    """(w [groups, g], grad, gscale) on the CPU: the first groups of the weight of test_gpu_group_quant.py, whose second
    group is all zero and whose third holds its abs-max twice"""
    w, grad, gscale = GQ.make_weight((max(groups, 3), g), g, dn)
    return w[:groups].contiguous(), grad[:groups].contiguous(), gscale[:groups].contiguous()


@functools.lru_cache(None)
def group_template(bits):
    """(min_val, int_threshold, qmin, qmax) that Int8WeightPerGroupFloat hands to its one-kernel route"""
    import brevitas_amd.quant as Q
    q = Q.Int8WeightPerGroupFloat(torch.nn.Parameter(torch.zeros(2, 64)), group_size=64, bit_width=bits)
    t = q._group_template(q.msb_clamp_bit_width_impl())
    thr = 2.0 ** (bits - 1) - 1
    assert t is not None and (t.int_thr, t.qmin, t.qmax) == (thr, -thr, thr), t
    return t.min_val, t.int_thr, t.qmin, t.qmax


def group_step(w, grad, gscale, g, bits, ste):
    """forward and backward through the wrappers on device tensors -> (y, scale, dw)"""
    from brevitas_amd.core.quant._fused import group_quant_call
    n = nat()
    min_val, int_thr, qmin, qmax = group_template(bits)
    desc, thr_div = group_quant_call(w, g, int_thr, qmin, qmax, ste)   # as GroupStatsFakeQuantFn builds them
    y, scale, stat = n.group_quant_fwd(desc, w, min_val, thr_div)
    dw = n.group_quant_bwd(desc, grad, w, scale, stat, gscale, min_val, thr_div)
    return y, scale, dw


def check_group_forward(y, scale, w, grad, g, bits, ste, dn):
    """y and scale against the CPU oracle, as test_forward_matches_the_oracle of test_gpu_group_quant.py"""
    import oracle as O
    min_val, thr, qmin, qmax = group_template(bits)
    xn, code = O.from_torch(w.reshape(-1))
    gn, _ = O.from_torch(grad.reshape(-1))
    d = O.make_desc(1, w.numel() // g, g, code, code, code, O.F32, scale_per_channel=True, qmin=qmin, qmax=qmax,
                    clamp_ste=ste)
    y_o, _, scale_o, _, _ = O.step_stats_scaled(d, xn, gn, min_val, thr)
    assert G.same_bits(O.from_torch(y.reshape(-1))[0], y_o, dn), 'y against the oracle'
    assert G.same_bits(O.from_torch(scale.reshape(-1))[0], scale_o, dn), 'scale against the oracle'


def check_group(out, ref, w, grad, g, bits, ste, dn):
    """the bars of test_gpu_group_quant.py on (y, scale, dw); ref: (y, scale, dw) of the per-channel route on the
    regrouped weight (GQ.per_channel_step) -> the worst deposit difference in ulps"""
    y, scale, dw = out
    y_r, scale_r, dw_r = ref
    GQ.assert_same_bits(y, y_r, dn, 'y')
    GQ.assert_same_bits(scale, scale_r, dn, 'scale')
    check_group_forward(y.cpu(), scale.cpu(), w, grad, g, bits, ste, dn)
    return GQ.assert_dw(dw, dw_r, w, grad, g, bits, dn)


# ---- asymmetric group-wise integer: inputs, the device steps with their bar --------------------------------------------

SHIFTED_BITS = 4      # the format's own width (unsigned 4-bit codes with a zero-point per group)


@functools.lru_cache(None)
def shifted_inputs(dn, g, groups):
    """(w [groups, g], grad, gscale, gzp) on the CPU: the first groups of the weight of test_gpu_group_shifted.py, whose
    groups 0 .. 9 are planted -- those of them that exist"""
    w, grad, gscale, gzp = GS.make_weight((max(groups, 10), g), g, dn)
    return tuple(t[:groups].contiguous() for t in (w, grad, gscale, gzp))


def shifted_steps(dn, g, groups, ste):
    """-> (device inputs, (y, scale, zp, dw) of the one-kernel route, the same of the per-channel route on the regrouped
    weight).  A single group is a weight of ONE channel there, the planted group 0 all ties: its statistics are reduced
    along a dim, so the per-channel route too puts the gradient of a tied extremum on the first tie (torch.max(x, dim)),
    whatever the channel count (tests/test_gpu_tie_routes.py)."""
    dev = tuple(t.to(DEV) for t in shifted_inputs(dn, g, groups))
    wd, gd, gsd, gzd = dev
    ref = GS.per_channel_step(wd, g, SHIFTED_BITS, ste, gd, gsd, gzd)
    return dev, GS.grouped_step(wd, g, SHIFTED_BITS, ste, gd, gsd, gzd), ref


def check_shifted(out, ref, dev, dn, g):
    """the bar of test_gpu_group_shifted.py on the device inputs `dev` -> the worst deposit difference in ulps"""
    wd, gd, gsd, gzd = dev
    return GS.compare(out, ref, wd, gd, g, SHIFTED_BITS, dn, gsd, gzd)


# ---- a: one group below, on and above every boundary ----------------------------------------------------------------

@dtypes
@edge_sizes
@pytest.mark.parametrize('fmt', ['e4m3', 'e2m1', 'int8'])
def test_mx_quant_at_the_edges(dn, g, fmt):
    worst = 0.0
    for groups in edge_counts(dn, g):
        x, grad, gs = mx_inputs(dn, g, groups)
        xd, gd, gsd = x.to(DEV), grad.to(DEV), gs.to(DEV)
        for rule, ste in MODES:
            try:
                worst = max(worst, check_mx(mx_step(xd, gd, gsd, g, fmt, rule, ste), x, grad, gs, g, fmt, rule, ste,
                                            dn))
            except AssertionError as e:
                raise AssertionError('%d groups, %s, ste=%d: %s' % (groups, rule, ste, e)) from e
    print('GROUP_WALK_EDGE_MX_DEPOSIT_ULPS %s %s g=%d worst=%.3f' % (dn, fmt, g, worst))


@dtypes
@edge_sizes
@pytest.mark.parametrize('fmt', PACK_FORMATS)
def test_mx_pack_at_the_edges(dn, g, fmt):
    for groups in edge_counts(dn, g):
        x, _, _ = mx_inputs(dn, g, groups)
        xd = x.to(DEV)
        for rule in H.RULES:
            y, _ = nat().mx_quant_fwd(xd, g, mx_code(fmt), mx_rule(rule))
            try:
                check_pack(pack_step(xd, g, fmt, rule), x, y, g, fmt, rule)
            except AssertionError as e:
                raise AssertionError('%d groups, %s: %s' % (groups, rule, e)) from e


@dtypes
@edge_sizes
@pytest.mark.parametrize('bits', [4, 8])
def test_group_quant_at_the_edges(dn, g, bits):
    worst = 0.0
    for groups in edge_counts(dn, g):
        w, grad, gs = group_inputs(dn, g, groups)
        wd, gd, gsd = w.to(DEV), grad.to(DEV), gs.to(DEV)
        for ste in (True, False):
            try:
                ref = GQ.per_channel_step(wd, g, bits, ste, gd, gsd)
                worst = max(worst, check_group(group_step(wd, gd, gsd, g, bits, ste), ref, w, grad, g, bits, ste, dn))
            except AssertionError as e:
                raise AssertionError('%d groups, ste=%d: %s' % (groups, ste, e)) from e
    print('GROUP_WALK_EDGE_INT_DEPOSIT_ULPS %s g=%d bits=%d worst=%.3f' % (dn, g, bits, worst))


@dtypes
@edge_sizes
def test_group_shifted_at_the_edges(dn, g, launches):
    worst, steps = 0.0, 0
    for groups in edge_counts(dn, g):
        for ste in (True, False):
            try:
                dev, out, ref = shifted_steps(dn, g, groups, ste)
                worst = max(worst, check_shifted(out, ref, dev, dn, g))
            except AssertionError as e:
                raise AssertionError('%d groups, ste=%d: %s' % (groups, ste, e)) from e
            steps += 1
    assert launches['group_shifted_fwd'] == launches['group_shifted_bwd'] == steps
    print('GROUP_WALK_EDGE_SHIFTED_DEPOSIT_ULPS %s g=%d worst=%.3f' % (dn, g, worst))


# ---- c: every NT = true instantiation -------------------------------------------------------------------------------

def test_the_two_libraries_report_their_thresholds(use_nt0):
    assert nat().lib.bvq_nt_threshold_bytes() == NT_BYTES
    use_nt0()
    assert nat().lib.bvq_nt_threshold_bytes() == 0
    assert nat().lib.bvq_abi_version() == nat().ABI_VERSION


@dtypes
@all_sizes
@H.formats
def test_mx_quant_nt(dn, g, fmt, use_nt0):
    x, grad, gs = mx_inputs(dn, g, NT_GROUPS)
    xd, gd, gsd = x.to(DEV), grad.to(DEV), gs.to(DEV)
    assert nat().lib.bvq_nt_threshold_bytes() == NT_BYTES
    plain = [mx_step(xd, gd, gsd, g, fmt, rule, ste) for rule, ste in MODES]
    use_nt0()
    worst = 0.0
    for (rule, ste), want in zip(MODES, plain):
        out = mx_step(xd, gd, gsd, g, fmt, rule, ste)
        for a, b, what in zip(out, want, ('y', 'scale', 'dx')):
            assert bits_equal(a, b), '%s of the NT kernel differs from the default library (%s)' % (what, rule)
        worst = max(worst, check_mx(out, x, grad, gs, g, fmt, rule, ste, dn))
    print('GROUP_WALK_NT_MX_DEPOSIT_ULPS %s %s g=%d worst=%.3f' % (dn, fmt, g, worst))


@dtypes
@all_sizes
@pytest.mark.parametrize('fmt', PACK_FORMATS)
def test_mx_pack_nt(dn, g, fmt, use_nt0):
    x, _, _ = mx_inputs(dn, g, NT_GROUPS)
    xd = x.to(DEV)
    assert nat().lib.bvq_nt_threshold_bytes() == NT_BYTES
    plain = [pack_step(xd, g, fmt, rule) for rule in H.RULES]
    ys = [nat().mx_quant_fwd(xd, g, mx_code(fmt), mx_rule(rule))[0] for rule in H.RULES]
    use_nt0()
    for rule, want, y in zip(H.RULES, plain, ys):
        out = pack_step(xd, g, fmt, rule)
        for a, b, what in zip(out, want, ('codes', 'scale bytes', 'decoded values')):
            assert bits_equal(a, b), '%s of the NT kernel differ from the default library (%s)' % (what, rule)
        check_pack(out, x, y, g, fmt, rule)


@dtypes
@all_sizes
@pytest.mark.parametrize('bits', [4, 8])
def test_group_quant_nt(dn, g, bits, use_nt0):
    w, grad, gs = group_inputs(dn, g, NT_GROUPS)
    wd, gd, gsd = w.to(DEV), grad.to(DEV), gs.to(DEV)
    assert nat().lib.bvq_nt_threshold_bytes() == NT_BYTES
    plain = [group_step(wd, gd, gsd, g, bits, ste) for ste in (True, False)]
    # the reference route runs on the default library: the per-channel kernels' NT variants are not the subject
    refs = [GQ.per_channel_step(wd, g, bits, ste, gd, gsd) for ste in (True, False)]
    use_nt0()
    worst = 0.0
    for ste, want, ref in zip((True, False), plain, refs):
        out = group_step(wd, gd, gsd, g, bits, ste)
        for a, b, what in zip(out, want, ('y', 'scale', 'dw')):
            assert bits_equal(a, b), '%s of the NT kernel differs from the default library (ste=%d)' % (what, ste)
        worst = max(worst, check_group(out, ref, w, grad, g, bits, ste, dn))
    print('GROUP_WALK_NT_INT_DEPOSIT_ULPS %s g=%d bits=%d worst=%.3f' % (dn, g, bits, worst))


@dtypes
@pytest.mark.parametrize('g', [16, 256])
def test_group_shifted_nt(dn, g, use_nt0, launches):
    """one workgroup's forward window, one group less and one group more"""
    window = LANES // lanes_per_group(dn, g) * FWD_DEPTH * WAVES
    assert nat().lib.bvq_nt_threshold_bytes() == NT_BYTES
    cases = [(groups, ste) for groups in (window - 1, window + 1) for ste in (True, False)]
    # the reference route runs on the default library: the per-channel kernels' NT variants are not the subject
    plain = [shifted_steps(dn, g, groups, ste) for groups, ste in cases]
    use_nt0()
    worst = 0.0
    for (groups, ste), (dev, want, ref) in zip(cases, plain):
        wd, gd, gsd, gzd = dev
        out = GS.grouped_step(wd, g, SHIFTED_BITS, ste, gd, gsd, gzd)
        for a, b, what in zip(out, want, ('y', 'scale', 'zp', 'dw')):
            assert bits_equal(a, b), '%s of the NT kernel differs from the default library (%d groups, ste=%d)' \
                % (what, groups, ste)
        worst = max(worst, check_shifted(out, ref, dev, dn, g))
    assert launches['group_shifted_fwd'] == launches['group_shifted_bwd'] == 2 * len(cases)
    print('GROUP_WALK_NT_SHIFTED_DEPOSIT_ULPS %s g=%d worst=%.3f' % (dn, g, worst))


# ---- d: backward branches of the autograd Functions -----------------------------------------------------------------

class _OffBoundary(torch.autograd.Function):
    """the identity, whose gradient comes back as a contiguous view that starts one element off a 16-byte boundary;
    its address is appended to `seen`"""

    @staticmethod
    def forward(ctx, t, seen):
        ctx.seen = seen
        return t.view_as(t)

    @staticmethod
    def backward(ctx, g):
        base = torch.empty(g.numel() + 16, dtype=g.dtype, device=g.device)
        assert base.data_ptr() % 16 == 0
        v = base[1:1 + g.numel()].view(g.shape)
        v.copy_(g)
        assert v.is_contiguous() and v.data_ptr() % 16 == g.element_size()
        ctx.seen.append(v.data_ptr())
        return v, None


@pytest.fixture
def clones(monkeypatch):
    """the addresses of the tensors whose .clone() was called, in order"""
    made = []
    real = torch.Tensor.clone

    def clone(self, *a, **k):
        made.append(self.data_ptr())
        return real(self, *a, **k)
    monkeypatch.setattr(torch.Tensor, 'clone', clone)
    return made


def assert_took_the_clone(seen, clones, launches, which, off):
    """the Function received the gradient at the address _OffBoundary made, `off` bytes off a 16-byte boundary, cloned
    exactly that tensor, and handed the backward wrapper an aligned copy"""
    assert len(seen) == 1 and seen[0] % 16 == off
    assert clones.count(seen[0]) == 1
    handed = launches['grad_ptrs'][-1][0 if which == 'gy' else 1]
    assert handed != seen[0] and handed % 16 == 0


BRANCH_SHAPE, BRANCH_G = (9, 192), 64


def mx_module_step(q, x, grad, gs, wrap_y=None, wrap_scale=None):
    """wrap_y / wrap_scale: a list -- that output's gradient arrives through _OffBoundary, which appends to it"""
    leaf = x.detach().clone().requires_grad_(True)
    y, scale, _, _ = q(leaf)
    if wrap_y is not None:
        y = _OffBoundary.apply(y, wrap_y)
    if wrap_scale is not None:
        scale = _OffBoundary.apply(scale, wrap_scale)
    outs = [t for t, g in ((y, grad), (scale, gs)) if g is not None]
    grads = [g.view(t.shape) for t, g in ((y, grad), (scale, gs)) if g is not None]
    torch.autograd.backward(outs, grads)
    return leaf.grad.detach()


@dtypes
@pytest.mark.parametrize('fmt', ['e4m3', 'e2m1'])
def test_mx_backward_when_only_the_scale_is_used(dn, fmt, launches):
    g = BRANCH_G
    x, _, gs = mx_inputs(dn, g, 27)
    x = x.view(BRANCH_SHAPE)
    for rule, ste in MODES:
        before = launches['mx_quant_bwd']
        dx = mx_module_step(H.mx(fmt, g, rule, ste).to(DEV), x.to(DEV), None, gs.to(DEV)).cpu()
        assert launches['mx_quant_bwd'] == before + 1
        H.assert_dx(dx, x, torch.zeros_like(x), gs, g, fmt, rule, ste, dn)
        moved = (dx.view(-1, g) != 0).sum(dim=1)
        assert bool((moved <= 1).all()) and int(moved.sum()) > 0   # one element per group at most, and some


@dtypes
@pytest.mark.parametrize('which', ['gy', 'gscale'])
def test_mx_backward_with_a_gradient_off_a_16_byte_boundary(dn, which, launches, clones):
    g, fmt = BRANCH_G, 'e4m3'
    x, grad, gs = mx_inputs(dn, g, 27)
    xd, gd, gsd = x.view(BRANCH_SHAPE).to(DEV), grad.view(BRANCH_SHAPE).to(DEV), gs.to(DEV)
    q = H.mx(fmt, g, 'floor', True).to(DEV)
    want = mx_module_step(q, xd, gd, gsd)
    seen = []
    del clones[:]
    got = mx_module_step(q, xd, gd, gsd, wrap_y=seen if which == 'gy' else None,
                         wrap_scale=seen if which == 'gscale' else None)
    assert_took_the_clone(seen, clones, launches, which, 2 if (which == 'gy' and dn != 'f32') else 4)
    assert launches['mx_quant_fwd'] == 2 and launches['mx_quant_bwd'] == 2
    assert bits_equal(got, want)
    H.assert_dx(got.cpu(), x, grad, gs, g, fmt, 'floor', True, dn)


def group_module_step(w0, g, bits, ste, grad, gscale, wrap_y=None):
    import brevitas_amd.quant as Q
    w = torch.nn.Parameter(w0.clone())
    q = GQ.set_clamp(Q.Int8WeightPerGroupFloat(w, group_size=g, bit_width=bits).to(w.device), ste)
    y, scale, _, _ = q(w)
    if wrap_y is not None:
        y = _OffBoundary.apply(y, wrap_y)
    outs = [t for t, g_ in ((y, grad), (scale, gscale)) if g_ is not None]
    grads = [g_.view(t.shape) for t, g_ in ((y, grad), (scale, gscale)) if g_ is not None]
    torch.autograd.backward(outs, grads)
    return w.grad.detach().clone()


@dtypes
@pytest.mark.parametrize('ste', [True, False], ids=['clamp_ste', 'clamp'])
def test_group_backward_when_only_the_scale_is_used(dn, ste, launches):
    g, bits = BRANCH_G, 4
    w, _, gs = GQ.make_weight(BRANCH_SHAPE, g, dn)
    wd, gsd = w.to(DEV), gs.to(DEV)
    dw = group_module_step(wd, g, bits, ste, None, gsd)
    assert launches['group_quant_fwd'] == 1 and launches['group_quant_bwd'] == 1
    zero = torch.zeros_like(wd)
    _, _, dw_r = GQ.per_channel_step(wd, g, bits, ste, zero, gsd)
    GQ.assert_dw(dw, dw_r, w, zero, g, bits, dn)
    # one element per group at most, and some.  Not the all-zero group: in float16 its scale, clamp_min(0, 1e-10) / 7,
    # rounds to zero and both routes give 0 / 0 for every element of it (assert_dw above compared them)
    live = (w.view(-1, g).float().abs().amax(dim=1) > 0).to(DEV)
    moved = (dw.view(-1, g) != 0).sum(dim=1)[live]
    assert int(live.sum()) == w.numel() // g - 1 and bool((moved <= 1).all()) and int(moved.sum()) > 0


@dtypes
def test_group_backward_with_a_gradient_off_a_16_byte_boundary(dn, launches, clones):
    g, bits = BRANCH_G, 4
    w, grad, gs = GQ.make_weight(BRANCH_SHAPE, g, dn)
    wd, gd, gsd = w.to(DEV), grad.to(DEV), gs.to(DEV)
    want = group_module_step(wd, g, bits, True, gd, gsd)
    seen = []
    del clones[:]
    got = group_module_step(wd, g, bits, True, gd, gsd, wrap_y=seen)
    assert_took_the_clone(seen, clones, launches, 'gy', 2 if dn != 'f32' else 4)
    assert launches['group_quant_fwd'] == 2 and launches['group_quant_bwd'] == 2
    assert bits_equal(got, want)
    _, _, dw_r = GQ.per_channel_step(wd, g, bits, True, gd, gsd)
    GQ.assert_dw(got, dw_r, w, grad, g, bits, dn)
