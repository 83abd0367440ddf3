"""MX block-scaled quantizers on the device: the one-kernel route (csrc/bvq_mx_quant.hip) against the composed route on
the CPU and against the numpy oracle of test_mx_quant_host.py; the routes that refuse, graph capture, a layer step.

Bars (test_mx_quant_host.py): y and scale are bit-exact; dx is bit-equal to gy * mask except at the first arg-max of each
group, where it lies within the derived tolerance of the float64 autograd reference.
"""
import functools

import pytest
import torch

import test_mx_quant_host as H
from test_mx_quant_host import DT, formats, rules

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
# the shapes of test_gpu_group_quant.py: less than one wave load in every dtype; a whole wave per float32 group with a
# ragged last wave; a number of groups that is no multiple of the groups per load; several workgroups at full depth;
# and groups along the last dimension of an activation
SHAPES = [((3, 64), 16, 'flat'), ((5, 512), 256, 'flat'), ((7, 96), 32, 'flat'), ((64, 4096), 128, 'flat'),
          ((2, 5, 64), 32, 'last'), ((9, 192), 64, 'flat')]     # and 27 groups of 64, ragged in every dtype
shapes = pytest.mark.parametrize('shape,g,axis', SHAPES,
                                 ids=['3x64-g16', '5x512-g256', '7x96-g32', '64x4096-g128', '2x5x64-g32-last',
                                      '9x192-g64'])
dtypes = pytest.mark.parametrize('dn', ['f32', 'bf16', 'f16'])


@pytest.fixture
def fused_calls(monkeypatch):
    """counts the launches of the MX kernels' wrappers: [forward, backward]"""
    from brevitas_amd import _native as nat
    calls = [0, 0]
    real_fwd, real_bwd = nat.mx_quant_fwd, nat.mx_quant_bwd

    def fwd(*a, **k):
        calls[0] += 1
        return real_fwd(*a, **k)

    def bwd(*a, **k):
        calls[1] += 1
        return real_bwd(*a, **k)
    monkeypatch.setattr(nat, 'mx_quant_fwd', fwd)
    monkeypatch.setattr(nat, 'mx_quant_bwd', bwd)
    return calls


def untie(x, g):
    """the first abs-max of every group made 1.25 times larger: no ties for the abs-max, whatever the dtype"""
    x2 = x.clone().view(-1, g)
    k = x2.float().abs().argmax(dim=1, keepdim=True)
    x2.scatter_(1, k, (x2.gather(1, k).float() * 1.25).to(x.dtype))
    return x2.view(x.shape)


@functools.lru_cache(None)
def inputs(shape, g, dn):
    """(x, grad, gscale) on the CPU: randn * 3 without abs-max ties, shared by the tests and left unchanged"""
    x, grad, gen = H.make_weight(shape, dn)
    x = untie(x, g)
    gscale = torch.randn(x.numel() // g, generator=gen)
    return x, grad, gscale


def device_step(q, x, grad, gscale=None):
    y, scale, dx = H.step(q.to(DEV), x.to(DEV), grad.to(DEV), None if gscale is None else gscale.to(DEV))
    torch.cuda.synchronize()
    return y.cpu(), scale.cpu(), dx.cpu()


# ---- the fused route against the oracle and the composed route -----------------------------------------------------

@shapes
@dtypes
@formats
@rules
def test_fused_route(shape, g, axis, dn, fmt, rule, fused_calls):
    x, grad, gscale = inputs(shape, g, dn)
    ste = rule == 'floor'       # both clamp modes over the sweep
    y, scale, dx = device_step(H.mx(fmt, g, rule, ste, axis), x, grad, gscale)
    assert fused_calls == [1, 1]
    H.check_forward(y, scale, H.oracle(x, g, fmt, rule))
    y_c, scale_c, _ = H.step(H.mx(fmt, g, rule, ste, axis), x, grad, gscale)
    assert H.same_bits(y, y_c) and H.same_bits(scale, scale_c)
    want = (shape[0], x.numel() // shape[0] // g, 1) if axis == 'flat' else shape[:-1] + (shape[-1] // g, 1)
    assert tuple(scale.shape) == want and scale.dtype == torch.float32 and y.shape == x.shape
    worst = H.assert_dx(dx, x, grad, gscale, g, fmt, rule, ste, dn)
    print('MX_QUANT_DEPOSIT_ULPS %s %s %s g=%d ste=%d worst=%.3f' % (dn, fmt, rule, g, ste, worst))


@dtypes
@formats
def test_without_a_gradient_through_the_scale(dn, fmt, fused_calls):
    x, grad, _ = inputs((7, 96), 32, dn)
    _, _, dx = device_step(H.mx(fmt, 32, 'floor', False), x, grad)
    assert fused_calls == [1, 1]
    H.assert_dx(dx, x, grad, None, 32, fmt, 'floor', False, dn)


@formats
@dtypes
def test_bf16_sweep(fmt, dn, fused_calls):
    x = H.bf16_sweep(dn)
    y, scale, _, _ = H.mx(fmt, 32).to(DEV)(x.to(DEV))
    assert fused_calls == [1, 0]
    H.check_forward(y.cpu(), scale.cpu(), H.oracle(x, 32, fmt, 'floor'))


@formats
@rules
@dtypes
def test_midpoints(fmt, rule, dn, fused_calls):
    x = H.midpoint_input(fmt, dn)
    y, scale, _, _ = H.mx(fmt, 32, rule).to(DEV)(x.to(DEV))
    assert fused_calls == [1, 0]
    H.check_forward(y.cpu(), scale.cpu(), H.oracle(x, 32, fmt, rule))


# ---- edge groups ----------------------------------------------------------------------------------------------------

def edge_input(dn):
    """[8, 32]: an all-zero group with signed zeros, a NaN, an Inf, the exponent clamp, tiny values, a tie for the
    abs-max across two 16-byte chunks, the largest finite values, and a plain group"""
    x, grad, _ = H.make_weight((8, 32), dn)
    x[0] = H.edge_all_zero(dn)[0]
    x[1, 9] = float('nan')
    x[2, 31] = float('-inf')
    x[3] = 0.0
    if dn == 'f16':
        x[3] = (torch.arange(-16, 16, dtype=torch.float32) * 2.0 ** -24).to(torch.float16)   # subnormals
    else:
        x[3, 5], x[3, 6] = 2.0 ** -120, -2.0 ** -123
    x[4] = H.tie_input(dn)[0][2]
    big = float(torch.finfo(DT[dn]).max)
    x[5] = 0.0
    x[5, 0], x[5, 1] = big, -big
    x[6] = (x[6].float() * 2.0 ** -130).to(DT[dn]) if dn != 'f16' else (x[6].float() * 2.0 ** -20).to(DT[dn])
    return x, grad


@formats
@rules
@dtypes
def test_edge_groups(fmt, rule, dn, fused_calls):
    x, grad = edge_input(dn)
    gs = torch.full((8,), 3.0)
    y, scale, dx = device_step(H.mx(fmt, 32, rule, True), x, grad, gs)
    assert fused_calls == [1, 1]
    ref = H.oracle(x, 32, fmt, rule)
    H.check_forward(y, scale, ref)
    assert bool(torch.isnan(scale.reshape(-1)[1])) and bool(torch.isnan(scale.reshape(-1)[2]))
    assert bool(torch.isnan(y[1]).all()) and bool(torch.isnan(y[2]).all()) and int(torch.isnan(scale).sum()) == 2
    assert float(scale.reshape(-1)[0]) == 2.0 ** -126 and H.same_bits(y[0], x[0])
    y_c, scale_c, dx_c = H.step(H.mx(fmt, 32, rule, True), x, grad, gs)
    assert H.same_bits(y, y_c) and H.same_bits(scale, scale_c)
    it = H.INT_VIEW[dn]
    for row in range(8):          # no deposit where nothing flows through a; one, on the first arg-max, elsewhere
        moved = torch.nonzero(dx[row].view(it) != grad[row].view(it)).reshape(-1).tolist()
        moved_c = torch.nonzero(dx_c[row].view(it) != grad[row].view(it)).reshape(-1).tolist()
        assert moved == moved_c, (row, moved, moved_c)
        if row in (0, 1, 2) or ref['clamped'][row]:
            assert moved == [], (row, moved)
    assert torch.nonzero(dx[4].view(it) != grad[4].view(it)).reshape(-1).tolist() == [1]
    if dn == 'f16' and fmt == 'e2m1' and rule == 'ceil':
        assert float(y[5, 0]) == float('inf') and float(y[5, 1]) == float('-inf')   # 4 * 2^14, by the definition


# ---- the composed route on the device -------------------------------------------------------------------------------

@pytest.mark.parametrize('kind', ['fused_paths_off', 'g48', 'misaligned'])
@pytest.mark.parametrize('fmt', ['e4m3', 'e2m1', 'int8'])
def test_the_composed_route_on_the_device(kind, fmt, fused_calls, monkeypatch):
    import brevitas_amd.config as config
    dn, g = 'bf16', 32
    gen = torch.Generator().manual_seed(7)
    if kind == 'g48':
        g = 48
    x = (torch.randn(8, 96, generator=gen) * 3).to(DT[dn])
    grad = torch.randn(8, 96, generator=gen).to(DT[dn])
    gs = torch.randn(8 * 96 // g, generator=gen)
    xd = x.to(DEV)
    if kind == 'fused_paths_off':
        monkeypatch.setattr(config, 'FUSED_PATHS', False)
    elif kind == 'misaligned':       # a view starting 2 bytes off a 16-byte boundary
        base = torch.zeros(8 * 96 + 8, dtype=DT[dn], device=DEV)
        base[1:1 + 8 * 96] = xd.reshape(-1)
        xd = base[1:1 + 8 * 96].view(8, 96)
        assert xd.data_ptr() % 16 == 2 and xd.is_contiguous()
    q = H.mx(fmt, g, 'floor', True)
    y, scale, dx = H.step(q.to(DEV), xd, grad.to(DEV), gs.to(DEV), clone=kind != 'misaligned')
    assert fused_calls == [0, 0]
    y_c, scale_c, dx_c = H.step(H.mx(fmt, g, 'floor', True), x, grad, gs)
    assert H.same_bits(y.cpu(), y_c) and H.same_bits(scale.cpu(), scale_c)
    assert H.same_bits(dx.cpu(), dx_c), H.first_mismatch(dx.cpu(), dx_c)
    H.check_forward(y.cpu(), scale.cpu(), H.oracle(x, g, fmt, 'floor'))


def test_a_non_contiguous_input_is_made_contiguous(fused_calls):
    x, grad, _ = inputs((7, 96), 32, 'bf16')
    xt = x.to(DEV).t().contiguous().t()
    assert not xt.is_contiguous()
    y, scale, _, _ = H.mx('e4m3', 32).to(DEV)(xt)
    assert fused_calls == [1, 0]
    H.check_forward(y.cpu(), scale.cpu(), H.oracle(x, 32, 'e4m3', 'floor'))


# ---- graph capture --------------------------------------------------------------------------------------------------

def test_step_in_a_graph(fused_calls):
    """one stream, no parallel branches: a forward + backward captured and replayed gives the eager bits"""
    torch.manual_seed(123456)
    w = torch.nn.Parameter((torch.randn(32, 256, device=DEV) * 3).to(torch.bfloat16))
    g = torch.randn(32, 256, device=DEV).to(torch.bfloat16)
    q = H.mx('e2m1', 32, 'floor', True).to(DEV)

    def one():
        w.grad = None
        y, scale, _, _ = q(w)
        y.backward(g)
        return y, scale, w.grad

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            one()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y_s, scale_s, dw_s = one()
    assert fused_calls == [4, 4]
    with torch.no_grad():
        w.mul_(1.5).add_(0.01)  # new values in the captured input
    graph.replay()
    torch.cuda.synchronize()
    got = (y_s.clone(), scale_s.clone(), dw_s.clone())
    y, scale, dw = one()
    assert torch.equal(got[0], y) and torch.equal(got[1], scale) and torch.equal(got[2], dw)


# ---- a layer --------------------------------------------------------------------------------------------------------

def test_quant_linear_step_matches_the_cpu(fused_calls):
    """[16, 128] -> 64 with MX weight and input quantizers: the quantizers' outputs are the CPU's bits, the float op
    is exactly F.linear on them (the bar of the existing layer tests), and the two quantizer backwards, fed the
    device's own gradients of the float op, meet the bars of the composed route"""
    import brevitas_amd.quant as Q
    from brevitas_amd.nn import QuantLinear, QuantReLU
    torch.manual_seed(0)
    bf = torch.bfloat16
    cpu = QuantLinear(128, 64, weight_quant=Q.MXFloat4e2m1Weight, input_quant=Q.MXFloat8e4m3Act(), dtype=bf)
    with torch.no_grad():
        cpu.weight.copy_(untie((torch.randn(64, 128) * 0.3).to(bf), 32))
    dev = QuantLinear(128, 64, weight_quant=Q.MXFloat4e2m1Weight, input_quant=Q.MXFloat8e4m3Act(), dtype=bf)
    dev.load_state_dict(cpu.state_dict())
    dev = dev.to(DEV)
    x = untie((torch.randn(16, 128) * 3).to(bf), 32)
    gout = torch.randn(16, 64).to(bf)
    # the layer, end to end
    xi = x.to(DEV).requires_grad_(True)
    out = dev(xi)
    out.backward(gout.to(DEV))
    assert fused_calls == [2, 2]
    # the same step with the quantized operands in hand
    xj = x.to(DEV).requires_grad_(True)
    xq, in_scale, _, _ = dev.input_quant(xj)
    wq, w_scale, _, _ = dev.quant_weight()
    xq.retain_grad()
    wq.retain_grad()
    dw_layer, db_layer = dev.weight.grad.clone(), dev.bias.grad.clone()
    dev.weight.grad = dev.bias.grad = None
    out2 = torch.nn.functional.linear(xq, wq, dev.bias)
    assert torch.equal(out, out2)
    out2.backward(gout.to(DEV))
    assert torch.equal(xi.grad, xj.grad) and torch.equal(dw_layer, dev.weight.grad) and torch.equal(db_layer, dev.bias.grad)
    assert tuple(in_scale.shape) == (16, 4, 1) and tuple(w_scale.shape) == (64, 4, 1)
    # against the CPU: the quantizers bit for bit, their backwards by the bars
    xq_c, is_c, _, _ = cpu.input_quant(x)
    wq_c, ws_c, _, _ = cpu.quant_weight()
    assert H.same_bits(xq.cpu(), xq_c) and H.same_bits(in_scale.cpu(), is_c)
    assert H.same_bits(wq.cpu(), wq_c) and H.same_bits(w_scale.cpu(), ws_c)
    H.assert_dx(xj.grad.cpu(), x, xq.grad.cpu(), None, 32, 'e4m3', 'floor', False, 'bf16')
    H.assert_dx(dev.weight.grad.cpu(), cpu.weight.detach(), wq.grad.cpu(), None, 32, 'e2m1', 'floor', True, 'bf16')
    # the bias gradient is a sum of 16 bfloat16 terms, rounded once
    db = gout.double().sum(0)
    assert bool(((dev.bias.grad.cpu().double() - db).abs() <= 2.0 ** -7 * gout.double().abs().sum(0)).all())
    # a fused activation in front of an MX quantizer: the activation is applied, then the one-kernel route
    n = fused_calls[0]
    act = QuantReLU(act_quant=Q.MXFloat8e4m3Act()).to(DEV)
    ya = act(x.to(DEV))
    assert fused_calls[0] == n + 1
    y_ref, _, _, _ = Q.MXFloat8e4m3Act()(torch.relu(x))
    assert H.same_bits(ya.cpu(), y_ref)
