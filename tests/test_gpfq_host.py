"""GPFQ on the host: the reduction to round-to-nearest, the composed float32 route against a float64 implementation of the
textbook recurrence in sample space, a dead column, the refusals and shape checks, gpfq_mode on a CPU model (the pairs
that enter H and D, the original weights the float pass sees, what __exit__ leaves) and the host-side argument checks of
bvq_gpfq_block.  No device is touched."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from brevitas_amd import quant as Q
from brevitas_amd.graph import GPFQResult, gpfq_mode, gpfq_quantize_weight
from brevitas_amd.graph import gpfq as P
from brevitas_amd.nn import QuantConv2d, QuantLinear


def _correlated(n, k, gen):
    return torch.randn(n, k, generator=gen) @ (torch.eye(k) + 2 * torch.randn(k, k, generator=gen) / k ** 0.5)


def _stats(x, xq):
    """H and D of one batch, with the weighting of gpfq_mode"""
    return (2.0 / x.shape[0]) * (xq.t() @ xq), (2.0 / x.shape[0]) * ((x - xq).t() @ xq)


# ---- D = 0 and a diagonal H: nothing is fed forward, every column is rounded to nearest ------------------------------

_RTN = {
    'sym4_g16': lambda w: Q.Int4WeightPerGroupFloat(w, 16),
    'asym4_g16': lambda w: Q.ShiftedUint4WeightPerGroupFloat(w, 16),
    'sym8_channel': lambda w: Q.Int8WeightPerChannelFloat(w),
    'asym8_tensor': lambda w: Q.ShiftedUint8WeightPerTensorFloat(w),
}


# (a per-tensor scale is a float32 scalar whatever the weight's dtype; the loop, like GPTQ's, rounds it to the weight's
# dtype, so for a 16-bit weight its codes are those of the rounded scale, which is what it hands back)
_RTN_CASES = [(c, dt) for c in sorted(_RTN) for dt in ('f32', 'bf16') if (c, dt) != ('asym8_tensor', 'bf16')]


@pytest.mark.parametrize('case,dn', _RTN_CASES, ids=['%s-%s' % c for c in _RTN_CASES])
def test_no_drift_and_a_diagonal_gram_matrix_is_round_to_nearest(case, dn):
    dtype = {'f32': torch.float32, 'bf16': torch.bfloat16}[dn]
    gen = torch.Generator().manual_seed(1)
    k = 160  # two blocks, the second ragged
    weight = torch.nn.Parameter((0.05 * torch.randn(24, k, generator=gen)).to(dtype))
    quant = _RTN[case](weight)
    h = torch.diag(0.5 + torch.rand(k, generator=gen))
    res = gpfq_quantize_weight(weight, h, torch.zeros(k, k), quant)
    want, scale, zp, bw = quant(weight)
    assert isinstance(res, GPFQResult) and res.q.dtype == dtype and res.q.shape == weight.shape
    assert torch.equal(res.q, want.detach())
    assert torch.equal(res.scale.to(dtype), scale.detach().to(dtype)) and torch.equal(res.zero_point, zp.detach())
    assert float(res.bit_width) == float(bw)


# ---- the textbook recurrence in sample space, float64 ----------------------------------------------------------------

def _sample_space_gpfq(w, x, xq, scale, zp, qmin, qmax):
    """u <- u + w_t X_t - q_t X~_t, q_t = Q(<X~_t, u + w_t X_t> / |X~_t|^2), all rows at once in float64
    -> (Q [R, K], the smallest distance of any step's code value to a rounding tie, per row, in code units)"""
    w, x, xq, scale, zp = w.double(), x.double(), xq.double(), scale.double(), zp.double()
    rows, k = w.shape
    u = torch.zeros(rows, x.shape[0], dtype=torch.float64)
    q = torch.empty(rows, k, dtype=torch.float64)
    margin = torch.full((rows,), float('inf'), dtype=torch.float64)
    for t in range(k):
        target = u + w[:, t:t + 1] * x[:, t]
        v = (target @ xq[:, t]) / xq[:, t].dot(xq[:, t])
        code = v / scale[:, t] + zp[:, t]
        margin = torch.minimum(margin, ((code - torch.floor(code)) - 0.5).abs())
        q[:, t] = (torch.clamp(torch.round(code), qmin, qmax) - zp[:, t]) * scale[:, t]
        u = target - q[:, t:t + 1] * xq[:, t]
    return q, margin


_SAMPLE = {
    # name -> (factory, group size or None: one group per row, qmin, qmax)
    'sym4_g16': (lambda w: Q.Int4WeightPerGroupFloat(w, 16), 16, -7.0, 7.0),
    'asym4_g16': (lambda w: Q.ShiftedUint4WeightPerGroupFloat(w, 16), 16, 0.0, 15.0),
    'sym8_channel': (lambda w: Q.Int8WeightPerChannelFloat(w), None, -127.0, 127.0),
}
# chosen on the CPU from the float64 route alone: it leaves out 0, 1 and 0 of the 64 rows of the three cases, and no
# row's margin lies between 5e-5 and 2e-4, so the count does not hang on the last bits of a float64 sum
SAMPLE_SEED = 16


@pytest.mark.parametrize('case', sorted(_SAMPLE))
def test_composed_route_follows_the_sample_space_recurrence(case):
    """R = 64, K = 48, N = 256, X~ = X + small noise: the codes of the composed float32 route are those of the float64
    recurrence on every row whose float64 trajectory stays 1e-4 code units away from a rounding tie at every step; at
    most 5 % of the rows may be left out"""
    make, g, qmin, qmax = _SAMPLE[case]
    rows, k, n = 64, 48, 256
    gen = torch.Generator().manual_seed(SAMPLE_SEED)
    w = 0.05 * torch.randn(rows, k, generator=gen)
    x = _correlated(n, k, gen)
    xq = x + 0.02 * torch.randn(n, k, generator=gen)
    weight = torch.nn.Parameter(w.clone())
    h, d = _stats(x, xq)
    res = gpfq_quantize_weight(weight, h, d, make(weight))
    g = g or k
    scale = res.scale.reshape(rows, -1).repeat_interleave(g, dim=1)
    zp = res.zero_point.reshape(-1, 1).expand(rows, k) if res.zero_point.numel() == 1 else \
        res.zero_point.reshape(rows, -1).repeat_interleave(g, dim=1)
    want, margin = _sample_space_gpfq(w, x, xq, scale, zp, qmin, qmax)
    keep = margin >= 1e-4
    left_out = int((~keep).sum())
    print('%s: %d of %d rows left out' % (case, left_out, rows))
    assert left_out <= 0.05 * rows
    got_codes = torch.round(res.q.double() / scale.double() + zp.double())
    want_codes = torch.round(want / scale.double() + zp.double())
    assert torch.equal(got_codes[keep], want_codes[keep])
    assert torch.equal(weight.detach(), w)  # nothing is changed in place


# ---- a column whose input never fired --------------------------------------------------------------------------------

@pytest.mark.parametrize('case', ['sym8_channel', 'asym4_g16'])
def test_dead_column_is_rounded_to_nearest_and_feeds_nothing_forward(case):
    rows, k, n, dead = 16, 48, 128, 21
    gen = torch.Generator().manual_seed(3)
    w = 0.05 * torch.randn(rows, k, generator=gen)
    w[:, dead] *= 0.1  # never the extremum its scale comes from
    x = _correlated(n, k, gen)
    xq = x + 0.02 * torch.randn(n, k, generator=gen)
    x[:, dead] = 0.0
    xq[:, dead] = 0.0
    h, d = _stats(x, xq)
    assert float(h[dead, dead]) == 0.0 and not h[dead].any() and not h[:, dead].any()
    weight = torch.nn.Parameter(w.clone())
    quant = _RTN[case](weight)
    res = gpfq_quantize_weight(weight, h, d, quant)
    assert torch.equal(res.q[:, dead], quant(weight)[0].detach()[:, dead])
    # without it: the same layer with nothing in that column
    w0 = w.clone()
    w0[:, dead] = 0.0
    weight0 = torch.nn.Parameter(w0)
    res0 = gpfq_quantize_weight(weight0, h, d, _RTN[case](weight0))
    others = [c for c in range(k) if c != dead]
    assert torch.equal(res.scale, res0.scale)
    assert torch.equal(res.q[:, others], res0.q[:, others])
    assert (res.q[:, others] != quant(weight)[0].detach()[:, others]).any()  # the other columns do feed forward


# ---- refusals and shapes ---------------------------------------------------------------------------------------------

def test_refusals_and_shape_errors():
    from brevitas_amd.core.bit_width import BitWidthParameter
    w = torch.nn.Parameter(torch.randn(8, 64))
    h = torch.eye(64)
    d = torch.zeros(64, 64)
    with pytest.raises(TypeError, match='gpfq.*GroupwiseMSEIntQuant'):
        gpfq_quantize_weight(w, h, d, Q.Int4WeightPerGroupFloatMSE(w, 32))
    with pytest.raises(TypeError, match='gpfq.*GroupwiseHQOIntQuant'):
        gpfq_quantize_weight(w, h, d, Q.ShiftedUint4WeightPerGroupFloatHQO(w, 32))
    with pytest.raises(TypeError, match='MXQuant'):
        gpfq_quantize_weight(w, h, d, Q.MXInt8Weight(w, 32))
    learned = Q.Int8WeightPerChannelFloat(w)
    learned.msb_clamp_bit_width_impl = BitWidthParameter(4)
    with pytest.raises(TypeError, match='learned bit width'):
        gpfq_quantize_weight(w, h, d, learned)
    quant = Q.Int8WeightPerChannelFloat(w)
    with pytest.raises(ValueError, match=r'H of shape \(32, 32\).*64'):
        gpfq_quantize_weight(w, torch.eye(32), d, quant)
    with pytest.raises(ValueError, match=r'D of shape \(64, 32\).*64'):
        gpfq_quantize_weight(w, h, torch.zeros(64, 32), quant)
    with pytest.raises(ValueError, match='no whole groups'):
        gpfq_quantize_weight(w, h, d, Q.Int4WeightPerGroupFloat(torch.nn.Parameter(torch.randn(8, 96)), 48))
    model = torch.nn.Sequential(QuantConv2d(8, 8, 3, groups=2, weight_quant=Q.Int8WeightPerChannelFloat))
    with pytest.raises(NotImplementedError, match=r"gpfq_mode.*'0'.*groups=2"):
        gpfq_mode(model).__enter__()
    for make in (Q.Int4WeightPerGroupFloatMSE, Q.ShiftedUint4WeightPerGroupFloatHQO):
        model = torch.nn.Sequential(QuantLinear(64, 8, weight_quant=functools.partial(make, group_size=32)))
        with pytest.raises(TypeError, match='Groupwise(MSE|HQO)IntQuant'):
            gpfq_mode(model).__enter__()


# ---- gpfq_mode on a CPU model ----------------------------------------------------------------------------------------

def _mlp():
    torch.manual_seed(3)
    return torch.nn.Sequential(
        QuantLinear(32, 48, weight_quant=functools.partial(Q.Int4WeightPerGroupFloat, group_size=16)),
        torch.nn.ReLU(),
        QuantLinear(48, 16, weight_quant=Q.Int8WeightPerChannelFloat))


def test_gpfq_mode_on_a_cpu_mlp():
    model = _mlp().eval()
    gen = torch.Generator().manual_seed(4)
    batches = [_correlated(40, 32, gen) for _ in range(3)]
    w1, b1 = model[0].weight.detach().clone(), model[0].bias.detach().clone()
    w2 = model[2].weight.detach().clone()
    with gpfq_mode(model) as gpfq:
        assert gpfq.num_layers == 2 and [name for name, _ in gpfq.layers] == ['0', '2']
        for b in batches:
            assert gpfq.model(b) is None  # both forwards stop behind the current layer
        # the first layer sees the same rows on both paths: no drift
        x = torch.cat(batches)
        torch.testing.assert_close(gpfq._h, (2.0 / 120) * (x.t() @ x), rtol=1e-4, atol=1e-5)
        assert gpfq._d.shape == (32, 32) and not gpfq._d.any()
        r1 = gpfq.update()
        assert torch.equal(model[0].weight.detach(), r1.q) and not torch.equal(r1.q, w1)
        assert torch.equal(model[0].frozen_weight_scale, r1.scale)
        assert torch.equal(gpfq._originals[model[0]], w1)  # kept for the float pass
        for b in batches:
            gpfq.model(b)
            # the float pass leaves nothing behind: the codes are back, the quantizers are on, eval mode stays
            assert torch.equal(model[0].weight.detach(), r1.q) and not model[0].bvq_disable_weight_quant
            assert not any(m.training for m in model.modules())
        # the second layer: X from a float copy of the model, X~ from the frozen first layer, entering as pairs
        want_h, want_d, n = torch.zeros(48, 48), torch.zeros(48, 48), 0
        for b in batches:
            xf = F.relu(F.linear(b, w1, b1))
            xq = F.relu(F.linear(b, r1.q, b1))
            want_h = want_h * (n / (n + 40)) + (2.0 / (n + 40)) * (xq.t() @ xq)
            want_d = want_d * (n / (n + 40)) + (2.0 / (n + 40)) * ((xf - xq).t() @ xq)
            n += 40
        assert torch.equal(gpfq._h, want_h)
        assert torch.equal(gpfq._d, want_d) and gpfq._d.any()
        r2 = gpfq.update()
        assert torch.equal(r2.q, gpfq_quantize_weight(torch.nn.Parameter(w2), want_h, want_d,
                                                      Q.Int8WeightPerChannelFloat(torch.nn.Parameter(w2))).q)
        assert set(gpfq._originals) == {model[0], model[2]}
        with pytest.raises(RuntimeError, match='every layer'):
            gpfq.update()
    assert gpfq._originals == {}  # released
    assert 'forward' not in model[0].__dict__ and 'forward' not in model[2].__dict__
    assert {'0.frozen_weight_scale', '0.frozen_weight_zero_point', '2.frozen_weight_scale',
            '2.frozen_weight_zero_point'} <= set(model.state_dict())
    y = model(batches[0])
    assert torch.equal(y, F.linear(F.relu(F.linear(batches[0], r1.q, model[0].bias)), r2.q, model[2].bias))
    # the second layer follows the float model's output more closely than round-to-nearest of the same weight does
    with torch.no_grad():
        x = torch.cat(batches)
        xq = F.relu(F.linear(x, r1.q, b1))
        want = F.linear(F.relu(F.linear(x, w1, b1)), w2)
        rtn = Q.Int8WeightPerChannelFloat(torch.nn.Parameter(w2))(w2)[0]
        err_gpfq, err_rtn = float((F.linear(xq, r2.q) - want).norm()), float((F.linear(xq, rtn) - want).norm())
    print('second layer: output error gpfq %.5f, round-to-nearest %.5f' % (err_gpfq, err_rtn))
    assert err_gpfq < err_rtn


def test_gpfq_mode_leaves_an_interrupted_model_clean():
    """an exception inside the with-block: every forward is restored and the saved weights are dropped"""
    model = _mlp().eval()
    x = torch.randn(8, 32)
    with pytest.raises(KeyError):
        with gpfq_mode(model) as gpfq:
            gpfq.model(x)
            gpfq.update()
            gpfq.model(x)
            raise KeyError('interrupted')
    assert gpfq._originals == {}
    assert 'forward' not in model[0].__dict__ and 'forward' not in model[2].__dict__
    assert not model[0].bvq_disable_weight_quant and not model[2].bvq_disable_weight_quant


def test_gpfq_mode_on_a_cpu_conv_layer():
    torch.manual_seed(7)
    model = torch.nn.Sequential(
        QuantConv2d(4, 8, 3, padding=1, weight_quant=functools.partial(Q.Int4WeightPerGroupFloat, group_size=12))).eval()
    x = torch.randn(2, 4, 6, 6)
    with gpfq_mode(model) as gpfq:
        gpfq.model(x)
        assert gpfq._h.shape == (36, 36)
        res = gpfq.update()
    assert res.q.shape == model[0].weight.shape and res.scale.shape == (8, 3, 1)
    with torch.no_grad():
        assert torch.equal(model(x), F.conv2d(x, model[0].weight, model[0].bias, padding=1))


# ---- host-side refusals of bvq_gpfq_block ----------------------------------------------------------------------------

def test_block_entry_refuses_before_the_device():
    from brevitas_amd import _native as nat
    lib = nat.lib
    ok = ctypes.c_void_p(4096)
    rows, cols = 8, 256

    def desc(g, zp=0, dt=nat.F32):
        return nat.QuantDesc(1, rows * cols // g, g, dt, dt, dt, dt if zp else nat.F32, 1, zp, -7.0, 7.0, nat.ROUND, 0, 1,
                             nat.OUT_DEQUANT, nat.PRE_NONE)

    def call(d, wf=ok, c=ok, h=ok, col0=0, bc=128, q=ok, err=ok, scale=ok, zp=None):
        return lib.bvq_gpfq_block(ctypes.byref(d) if d is not None else None, wf, c, h, rows, cols, col0, bc, q, err,
                                  scale, zp, None)

    assert call(None) == -1 and 'descriptor' in nat.last_error()
    for name in ('wf', 'c', 'h', 'q', 'err', 'scale'):
        assert call(desc(32), **{name: None}) == -1 and 'null pointer' in nat.last_error(), name
    assert call(desc(32, zp=1)) == -1 and 'zp' in nat.last_error()  # an asymmetric quantizer needs zp
    for name in ('wf', 'c', 'h', 'q', 'err'):
        assert call(desc(32), **{name: ctypes.c_void_p(4100)}) == -2 and '16-byte' in nat.last_error(), name
    assert call(desc(32), bc=129) == -1 and 'block_cols 129' in nat.last_error()
    assert call(desc(32), bc=0) == -1 and 'block_cols 0' in nat.last_error()
    assert call(desc(32), col0=192, bc=128) == -1 and 'columns 192' in nat.last_error()
    assert call(desc(48)) == -1 and 'groups of 48' in nat.last_error()  # 48 does not divide 256
    d = desc(32)
    d.round_mode = nat.FLOOR
    assert call(d) == -2 and 'half-even' in nat.last_error()
    # any group size that divides the columns, at any column offset
    assert lib.bvq_gpfq_block_supported(ctypes.byref(desc(256)), rows, cols, 128, 128, ok, ok, ok, ok) == 1
    assert lib.bvq_gpfq_block_supported(ctypes.byref(desc(32)), rows, cols, 16, 72, ok, ok, ok, ok) == 1
    assert lib.bvq_gpfq_block_supported(ctypes.byref(desc(32)), rows, cols, 0, 128, ok, ctypes.c_void_p(4100), ok, ok) == 0
    assert P.BLOCK == nat.COLUMN_BLOCK == 128
