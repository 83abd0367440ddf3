"""Loader of tests/golden/dynamic_act.npz (tests/golden/make_golden_dynamic_act.py) and what the CPU and the device
tests of the dynamic activation quantizers share: the cases as golden_util.Case objects whose x, g, y and dx are decoded
from the compact forms the generator stores (its docstring names them), the quantizer of a case, one training step, and
the bars of a case -- the helpers of tests/test_group_shifted_golden.py (asymmetric) and tests/test_group_quant_golden.py
(symmetric) with a row, or the whole tensor, in a group's place."""
import numpy as np
import torch

import golden_util as G
import test_group_quant_golden as SYM
import test_group_shifted_golden as SH

DT = SH.DT


def _to_np(t):
    return SH.to_np(t).copy()


class DynCase(G.Case):

    def has(self, name):
        return name in ('x', 'g', 'y', 'dx') or super().has(name)

    def arr(self, name):
        key = ('dyn', self._idx, name)
        if key in self._arrays:
            return self._arrays[key]
        dt = DT[self['dtype']]
        if name in ('x', 'g'):
            out = _to_np(torch.from_numpy(self._arrays['%s_%s' % (self['inputs'], name)].copy()).to(dt))
        elif name == 'y':
            q = torch.from_numpy(super().arr('q').astype(np.float32)).to(dt)
            scale, zp = self.torch('scale'), self.torch('zp')
            g = self['group_size']
            q2 = q.reshape(-1, g) if g else q
            scale2 = scale.reshape(-1, 1) if scale.dim() else scale
            zp2 = zp.reshape(-1, 1) if zp.dim() else zp
            y = ((q2 - zp2) * scale2).reshape(-1)   # the last two ops of the reference's forward
            y[torch.from_numpy(super().arr('nz').astype(np.int64))] = -0.0
            out = _to_np(y.reshape(q.shape))
        elif name == 'dx':
            gb = self.arr('g')
            out = super().arr('dxg') ^ (gb.view(np.uint32) if gb.dtype == np.float32 else gb)
            out = out.view(np.float32) if self['dtype'] == 'f32' else out
        else:
            return super().arr(name)
        self._arrays[key] = out
        return out


def load():
    cases = G.load('dynamic_act')
    return [DynCase(dict(c), c._arrays, c._idx) for c in cases]


CASES = load()
IDS = G.ids(CASES, ['quantizer', 'shape', 'bit_width', 'dtype'])


def quantizer(c):
    import brevitas_amd.quant as Q
    kw = dict(bit_width=c['bit_width'])
    if c['granularity'] == 'group':
        kw['group_size'] = c['group_size']
    return getattr(Q, c['quantizer'])(**kw)


def run_case(c, device, shape=None):
    """one training step on the golden input -> (y, scale, zero_point, dx); shape: x reshaped to it (same rows)"""
    x = c.torch('x', device)
    g = c.torch('g', device)
    if shape is not None:
        x, g = x.reshape(shape), g.reshape(shape)
    x = x.clone().requires_grad_(True)
    q = quantizer(c).to(device)
    y, scale, zp, bw = q(x)
    assert float(bw) == c['bit_width']
    y.backward(g)
    return y, scale, zp, x.grad


def stat_unit(c):
    """elements sharing one pair of statistics: the group, the row, or the whole tensor"""
    rows, h = c['shape']
    return {'tensor': rows * h, 'row': h, 'group': c['group_size']}[c['granularity']]


def tensor_positions(x, shifted):
    """a whole-tensor max / min hands its gradient to EVERY element attaining it (torch.max / torch.min without a dim)"""
    a = x.detach().float().cpu().reshape(-1)
    if shifted:
        hit = (a == a.max()) | (a == a.min())
    else:
        hit = a.abs() == a.abs().max()
    return set(torch.nonzero(hit).reshape(-1).tolist())


def check_case(c, y, scale, zp, dx):
    """y, scale and zp bit-exact, dx bit-exact except at the deposit positions -> the worst deposit difference in ulps
    (asymmetric cases; None for the symmetric ones, whose helper returns nothing)"""
    rows, h = c['shape']
    unit, dt = stat_unit(c), DT[c['dtype']]
    sshape = {'tensor': (), 'row': (rows, 1), 'group': (rows, h // unit, 1)}[c['granularity']]
    assert tuple(y.shape) == (rows, h) and y.dtype == dt
    assert tuple(scale.shape) == sshape and scale.dtype == DT[c['dtypes']['scale']]
    SH.assert_bits(y, c, 'y')
    SH.assert_bits(scale, c, 'scale')
    x = c.torch('x')
    if not c['shifted']:
        assert zp.dim() == 0 and float(zp) == 0.0
        pos = tensor_positions(x, False) if c['granularity'] == 'tensor' else SYM.first_argmax_positions(x, unit)
        SYM.assert_dx(dx, c, pos)
        return None
    assert tuple(zp.shape) == sshape and zp.dtype == DT[c['dtypes']['zp']]
    zf = zp.detach().float().cpu()
    assert bool((zf == zf.round()).all()) and float(zf.min()) >= 0 and float(zf.max()) <= 2 ** c['bit_width'] - 1
    SH.assert_bits(zp, c, 'zp')
    if c['granularity'] != 'tensor':
        return SH.assert_dx(dx, c.torch('dx'), x, c.torch('g'), c.torch('scale'), c.torch('zp'), unit, c['bit_width'],
                            c['dtype'])
    return assert_dx_tensor(dx, c.torch('dx'), x, c.torch('g'), c.torch('scale'), c.torch('zp'), c['bit_width'], c['dtype'])


def assert_dx_tensor(got, want, x, grad, scale, zp, bits, dn):
    """SH.assert_dx for ONE pair of statistics over the whole tensor, where every attaining element is a deposit
    position: bit-equal away from them, within SH.deposit_ulps(dn, numel) there -> the worst ulps seen"""
    unit = x.numel()
    view = np.uint32 if dn == 'f32' else np.uint16
    gotb, wantb = SH.to_np(got).reshape(-1).view(view), SH.to_np(want).reshape(-1).view(view)
    gotf = got.detach().float().cpu().numpy().reshape(-1).astype(np.float64)
    wantf = want.detach().float().cpu().numpy().reshape(-1).astype(np.float64)
    bad = np.nonzero(gotb != wantb)[0].tolist()
    assert set(bad) <= tensor_positions(x, True), sorted(bad)[:8]
    mag0 = float(SH.deposit_magnitude(x, grad, scale, zp, unit, bits)[0])
    worst = 0.0
    for i in bad:
        n = abs(gotf[i] - wantf[i]) / SH.ulp(max(abs(gotf[i]), abs(wantf[i]), mag0), dn)
        assert n <= SH.deposit_ulps(dn, unit), (i, gotf[i], wantf[i], n)
        worst = max(worst, n)
    return worst
