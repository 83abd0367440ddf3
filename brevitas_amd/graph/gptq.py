"""GPTQ weight quantization (Frantar et al., 2022; `gptq_mode` of later Brevitas releases, no reference counterpart).

GPTQ quantizes a weight [R, K] one input column at a time and pushes each column's error onto the columns not yet
quantized, through the upper Cholesky factor U of the damped inverse Hessian of the layer's inputs.  DESIGN.md §9 and
include/bvq.h ("GPTQ") state the definition; two routes compute it with the same bits:

  * fused: one bvq_gptq_block launch per block of 128 columns (csrc/bvq_gptq.hip: one wave per row, the block in
    registers) -- device tensors, config.FUSED_PATHS, scale and zero-point given or computed for groups of 16, 32, 64
    or 128;
  * composed: plain torch ops per column, written from the quantizer's own sub-modules -- CPU tensors, other group
    sizes, misaligned tensors, config.FUSED_PATHS off.

Both share the Hessian preparation and the float32 update of the columns right of a block.

    with gptq_mode(model) as gptq:
        for _ in range(gptq.num_layers):
            for batch in loader:
                gptq.model(batch)
            gptq.update()

Re-running a stats-scaled quantizer on the GPTQ codes does not reproduce the GPTQ scales (the abs-max of a group of Q is
in general not the one its scale came from), so `update()` writes Q into `layer.weight.data` and FREEZES the layer:
buffers `frozen_weight_scale` / `frozen_weight_zero_point`, from which `quant_weight()` answers without running the
quantizer.  `freeze_weight_quant` / `unfreeze_weight_quant` do the same by hand (loading a checkpoint into a fresh model,
resuming QAT)."""
from typing import NamedTuple, Optional

import torch
import torch.nn.functional as F
from torch import Tensor

import brevitas_amd.config as config
from brevitas_amd import _native as nat
from brevitas_amd.core.quant import _fused
from brevitas_amd.core.quant._recognise import GROUP_SIZES, clamp_ste_of, round_mode_of
from brevitas_amd.core.quant.int import (GroupwiseHQOIntQuant, GroupwiseMSEIntQuant, GroupwiseRescalingIntQuant,
                                         RescalingIntQuant)
from brevitas_amd.core.quant.int_base import IntQuant
from brevitas_amd.core.scaling.runtime import StatsFromParameterScaling
from brevitas_amd.core.zero_point import StatsFromParameterZeroPoint, ZeroZeroPoint
from brevitas_amd.function.ops import int_range_host

__all__ = ['gptq_mode', 'gptq_quantize_weight', 'GPTQResult', 'freeze_weight_quant', 'unfreeze_weight_quant']

BLOCK = nat.COLUMN_BLOCK
_FUSED_GROUPS = tuple(g for g in GROUP_SIZES if g <= BLOCK)  # a group never straddles a block


class GPTQResult(NamedTuple):
    q: Tensor            # the dequantized codes, shaped and typed like the weight
    scale: Tensor        # shaped as the quantizer returns it
    zero_point: Tensor
    bit_width: Tensor


class _Plan(NamedTuple):
    quant: RescalingIntQuant
    group: int        # columns that share a scale: the group size, or K
    computed: bool    # scale and zero-point are computed in the loop, at each group start
    shifted: bool     # one zero-point per group (asymmetric)
    bit_width: Tensor
    qmin: float
    qmax: float


def _plan(quantizer, k: int, static_groups: bool, who: str = 'gptq') -> _Plan:
    """what the loop needs to know of `quantizer`, or the TypeError naming what is refused; who: the caller the error
    speaks for (graph/awq.py plans its composed route with this one)"""
    name = type(quantizer).__name__
    if isinstance(quantizer, GroupwiseMSEIntQuant):
        raise TypeError('%s: the clip-search quantizer %s is not covered (its threshold is searched on the finished '
                        'group, which the column loop does not have)' % (who, name))
    if isinstance(quantizer, GroupwiseHQOIntQuant):
        raise TypeError('%s: the zero-point-search quantizer %s is not covered (its zero-point is searched on the '
                        'finished group, which the column loop does not have)' % (who, name))
    if type(quantizer) not in (RescalingIntQuant, GroupwiseRescalingIntQuant):
        raise TypeError('%s: the quantizer %s is not covered (integer weight quantizers per tensor, per channel or '
                        'per group only)' % (who, name))
    iq, zpi = quantizer.int_quant, quantizer.zero_point_impl
    bw = quantizer.msb_clamp_bit_width_impl()
    host_bw = getattr(bw, 'bvq_host_value', None)
    if host_bw is None:
        raise TypeError('%s: %s with a learned bit width is not covered' % (who, name))
    if type(iq) is not IntQuant or round_mode_of(iq.float_to_int_impl) != nat.ROUND:
        raise TypeError('%s: %s with the integer quantizer %s is not covered (IntQuant with half-even rounding only)'
                        % (who, name, type(iq).__name__))
    if type(zpi) not in (ZeroZeroPoint, StatsFromParameterZeroPoint):
        raise TypeError('%s: %s with the zero-point %s is not covered' % (who, name, type(zpi).__name__))
    shifted = type(zpi) is StatsFromParameterZeroPoint
    grouped = isinstance(quantizer, GroupwiseRescalingIntQuant)
    if grouped and not static_groups and type(quantizer.scaling_impl) is not StatsFromParameterScaling:
        raise TypeError('%s: %s with the scaling %s is not covered where the scales are computed in the loop (a '
                        'statistic of the group only; static_groups=True takes the quantizer\'s own scales)'
                        % (who, name, type(quantizer.scaling_impl).__name__))
    group = quantizer.group_size if grouped else k
    if k % group:
        raise ValueError('%s: %d input columns are no whole groups of %d' % (who, k, group))
    qmin, qmax = int_range_host(iq.signed, iq.narrow_range, host_bw)
    return _Plan(quantizer, group, grouped and not static_groups, shifted, bw, qmin, qmax)


# ---- what both routes share ------------------------------------------------------------------------------------------

_DEVICE_LINALG = {}


def _device_linalg_ok(device) -> bool:
    """torch.linalg's Cholesky routines work on this device in this torch build (asked once, on a 2 x 2 matrix)"""
    ok = _DEVICE_LINALG.get(device)
    if ok is None:
        try:
            eye = torch.eye(2, dtype=torch.float32, device=device)
            torch.linalg.cholesky(torch.cholesky_inverse(torch.linalg.cholesky(eye)), upper=True)
            ok = True
        except RuntimeError:
            ok = False
        _DEVICE_LINALG[device] = ok
    return ok


def prepare_hessian(hessian: Tensor, wf: Tensor, percdamp: float, name: str = '') -> Tensor:
    """H [K, K] -> U float32 [K, K] on wf's device, the upper Cholesky factor of the damped inverse Hessian; the columns
    of wf (the float32 working copy, changed in place) whose input never fired are zeroed.  The factorisation is
    plumbing: torch.linalg on the device where that works (float32), else on the host in float64."""
    h = hessian.detach().to(device=wf.device, dtype=torch.float32).clone()
    k = wf.shape[1]
    if h.shape != (k, k):
        raise ValueError('gptq: a Hessian of shape %s for %d input columns' % (tuple(h.shape), k))
    diag = torch.diagonal(h)
    dead = diag == 0
    diag[dead] = 1.0
    wf[:, dead] = 0.0
    diag += percdamp * diag.mean()
    on_device = wf.is_cuda and _device_linalg_ok(wf.device)
    work = h if on_device else h.to(device='cpu', dtype=torch.float64)
    try:
        u = torch.linalg.cholesky(torch.cholesky_inverse(torch.linalg.cholesky(work)), upper=True)
    except RuntimeError as exc:  # (torch.linalg.LinAlgError is one)
        raise RuntimeError('gptq: the Hessian of layer %r could not be factorised with percdamp=%g (%s); collect more '
                           'calibration data or raise percdamp' % (name, percdamp, str(exc).splitlines()[0])) from exc
    return u.to(device=wf.device, dtype=torch.float32).contiguous()


def tail_update(wf: Tensor, err: Tensor, u: Tensor, c0: int, c1: int) -> None:
    """Wf[:, c1:] -= E @ U[c0:c1, c1:], one float32 matrix product"""
    if c1 < wf.shape[1]:
        wf[:, c1:] -= torch.matmul(err, u[c0:c1, c1:])


def _given_params(plan: _Plan, weight: Tensor):
    """(scale, zero-point or None) as [R, K / group] arrays of the weight's dtype, and the quantizer's own outputs, from
    one run of the quantizer on the original weight"""
    _, scale, zero_point, _ = plan.quant(weight)
    rows = weight.shape[0]
    groups = (weight.numel() // rows) // plan.group

    def table(t):
        t = t.detach().to(weight.dtype)
        return (t.reshape(rows, groups) if t.numel() == rows * groups else t.reshape(-1, 1).expand(rows, groups)).contiguous()
    # what is handed back is what the loop used: a 0-dim float32 scale of a 16-bit weight rounded to the weight's dtype
    used = scale.detach().to(weight.dtype).to(scale.dtype)
    return table(scale), table(zero_point) if plan.shifted else None, used, zero_point.detach()


def _group_params(plan: _Plan, xg: Tensor):
    """scale [R, 1] and zero-point of the groups xg [R, g], from the quantizer's own sub-modules: the statistic of xg
    in place of the tracked weight's, then the quantizer's own maps"""
    q = plan.quant
    sc, zpi = q.scaling_impl, q.zero_point_impl
    stat = sc.parameter_list_stats.stats.stats_impl(xg).reshape(-1, 1)
    scale = sc.stats_scaling_impl(stat) / q.int_scaling_impl(plan.bit_width)
    if not plan.shifted:
        return scale, zpi(xg, scale, plan.bit_width)
    zstat = zpi.parameter_list_stats.stats.stats_impl(xg).reshape(-1, 1)
    return scale, zpi.scale_shift_zero_point(-zstat, scale, plan.bit_width)


# ---- the column loop, as GPTQ and GPFQ (graph/gpfq.py) share it ---------------------------------------------------------

class _ComposedBlock:
    """the bookkeeping of the block [c0, c1) in plain torch ops: which scale and zero-point apply at a column, the
    buffer E [R, c1 - c0] and the stores.  The arithmetic of a step is the algorithm's own."""

    def __init__(self, plan: _Plan, wf: Tensor, c0: int, c1: int, q: Tensor, scale: Tensor, zp: Optional[Tensor]):
        self.plan, self.wf, self.c0, self.q, self.scale, self.zp = plan, wf, c0, q, scale, zp
        self.err = torch.empty(wf.shape[0], c1 - c0, dtype=torch.float32, device=wf.device)

    def columns(self):
        """(i, col, s, z) for each column of the block.  Computed parameters come from the group in wf as it stands
        when its first column is reached, and are stored; given ones are read at a group start and at the block's
        first column, where a group may have begun in an earlier block."""
        plan, g, wf, scale, zp = self.plan, self.plan.group, self.wf, self.scale, self.zp
        zero = None if plan.shifted else plan.quant.zero_point_impl(wf, scale, plan.bit_width)
        s = z = None
        for i in range(self.err.shape[1]):
            col = self.c0 + i
            if plan.computed and col % g == 0:
                # the whole group: its columns beyond the block hold the tail updates of earlier blocks only
                s, z = _group_params(plan, wf[:, col:col + g].to(self.q.dtype).contiguous())
                scale[:, col // g] = s[:, 0]
                if plan.shifted:
                    zp[:, col // g] = z[:, 0]
            elif col % g == 0 or i == 0:
                s = scale[:, col // g].reshape(-1, 1).contiguous()
                z = zp[:, col // g].reshape(-1, 1).contiguous() if plan.shifted else zero
            yield i, col, s, z

    def store(self, i: int, qc: Tensor, e: Tensor) -> None:
        self.q[:, self.c0 + i] = qc
        self.err[:, i] = e


def walk_blocks(k: int, supported, fused, composed, tail) -> None:
    """the blocks [c0, c1) of k columns in order: the block step, fused(c0, c1) or composed(c0, c1) -> E, then
    tail(E, c0, c1), the update of the columns right of the block.  fused: None where the route is out; it is taken for
    every block if supported(c0, c1) holds for the first (the tensors' alignment: one answer serves all blocks)."""
    if fused is not None and not supported(0, min(BLOCK, k)):
        fused = None
    for c0 in range(0, k, BLOCK):
        c1 = min(c0 + BLOCK, k)
        tail((fused or composed)(c0, c1), c0, c1)


# ---- GPTQ's own ------------------------------------------------------------------------------------------------------

def composed_block(plan: _Plan, wf: Tensor, u: Tensor, c0: int, c1: int, q: Tensor, scale: Tensor,
                   zp: Optional[Tensor]) -> Tensor:
    """the column loop of the block [c0, c1) in plain torch ops: the block's columns of wf (float32, updated in place)
    -> the block's columns of q, the entries of scale / zp of the groups that start in the block where they are computed,
    and E [R, c1 - c0].  A group may cross the block's end (group sizes that do not divide 128, or 256): its parameters
    are computed once, at its first column, and read back in the blocks it continues in."""
    block = _ComposedBlock(plan, wf, c0, c1, q, scale, zp)
    wb = wf[:, c0:c1]
    for i, col, s, z in block.columns():
        x = wb[:, i:i + 1].to(q.dtype).contiguous()
        qc = plan.quant.int_quant(s, z, plan.bit_width, x)[:, 0]
        e = (wb[:, i] - qc.float()) / u[col, col]
        block.store(i, qc, e)
        if i + 1 < c1 - c0:
            # the product rounded, then the difference: two ops, no fused multiply-add
            wb[:, i + 1:] -= e.reshape(-1, 1) * u[col, col + 1:c1].reshape(1, -1)
    return block.err


class _FusedArgs(NamedTuple):
    desc: 'nat.QuantDesc'
    min_val: Optional[float]
    thr_div: float


def fused_block_args(plan: _Plan, rows: int, k: int, dtype: torch.dtype) -> Optional[_FusedArgs]:
    """the descriptor and scale arguments of bvq_gptq_block for a weight [rows, k] of `dtype`, or None: the quantizer's
    graph, the group size or the configuration is not what the kernel covers (tensors apart)"""
    if not config.FUSED_PATHS or dtype not in _fused._FLOATS:
        return None
    groups = rows * (k // plan.group)
    min_val, thr_div = None, 1.0
    clamp_ste = clamp_ste_of(plan.quant.int_quant.tensor_clamp_impl)
    if clamp_ste is None:
        return None
    if plan.computed:
        # the loop computes what the one-kernel route of the group-wise quantizer computes: the same recognised graph
        tmpl = plan.quant._group_template(plan.bit_width)
        if tmpl is None or plan.group not in _FUSED_GROUPS or tmpl.shifted != plan.shifted:
            return None
        min_val, thr_div = tmpl.min_val, _fused.scale_rule(dtype, (groups, 1), tmpl.int_thr).thr_div
    desc = _fused.channel_desc(1, groups, plan.group, dtype, plan.qmin, plan.qmax, nat.ROUND,
                               bool(clamp_ste), zp_dtype=dtype if plan.shifted else torch.float32, zp_pc=plan.shifted)
    return _FusedArgs(desc, min_val, thr_div)


def fused_block(args: _FusedArgs, plan: _Plan, wf: Tensor, u: Tensor, c0: int, c1: int, q: Tensor, scale: Tensor,
                zp: Optional[Tensor]) -> Tensor:
    """composed_block as one bvq_gptq_block launch (wf is read only: the block's columns are finished)"""
    return nat.gptq_block(args.desc, wf, u, c0, c1 - c0, plan.computed, args.min_val, args.thr_div, q, scale, zp)


def gptq_quantize_weight(weight: Tensor, hessian: Tensor, quantizer, *, percdamp: float = 0.01,
                         static_groups: bool = False, name: str = '') -> GPTQResult:
    """GPTQ of `weight` ([R, ...], flattened to [R, K]) under `hessian` ([K, K], accumulated as gptq_mode does) with the
    codes, scales and zero-points of `quantizer`, the weight's own weight quantizer.  Nothing is changed in place.
    static_groups: a group-wise quantizer's scales and zero-points are computed once from the original weight, instead of
    at each group start of the loop.  name: the layer's, for the error of a failing factorisation."""
    with torch.no_grad():
        rows = weight.shape[0]
        w2 = weight.detach().reshape(rows, -1)
        k = w2.shape[1]
        plan = _plan(quantizer, k, static_groups)
        groups = k // plan.group
        if plan.computed:
            scale = torch.empty(rows, groups, dtype=weight.dtype, device=weight.device)
            zp = torch.empty_like(scale) if plan.shifted else None
        else:
            scale, zp, scale_out, zp_out = _given_params(plan, weight)
        wf = w2.float().clone()
        u = prepare_hessian(hessian, wf, percdamp, name)
        q = torch.empty(rows, k, dtype=weight.dtype, device=weight.device)

        fa = fused_block_args(plan, rows, k, weight.dtype) if weight.is_cuda else None
        walk_blocks(k, lambda c0, c1: nat.gptq_block_supported(fa.desc, wf, u, q, c0, c1 - c0, plan.computed),
                    None if fa is None else lambda c0, c1: fused_block(fa, plan, wf, u, c0, c1, q, scale, zp),
                    lambda c0, c1: composed_block(plan, wf, u, c0, c1, q, scale, zp),
                    lambda err, c0, c1: tail_update(wf, err, u, c0, c1))
        if plan.computed:
            scale_out = scale.reshape(rows, groups, 1)
            zp_out = zp.reshape(rows, groups, 1) if plan.shifted else quantizer.zero_point_impl(weight, scale_out,
                                                                                                plan.bit_width)
        return GPTQResult(q.reshape(weight.shape), scale_out, zp_out, plan.bit_width)


# ---- frozen layers ---------------------------------------------------------------------------------------------------

def freeze_weight_quant(layer, scale: Tensor, zero_point: Tensor) -> None:
    """`layer.weight` holds dequantized codes already: from now on quant_weight() returns (weight, scale, zero_point,
    bit_width) from the buffers `frozen_weight_scale` / `frozen_weight_zero_point` without running the quantizer"""
    if getattr(layer, 'weight_quant', None) is None:
        raise TypeError('freeze_weight_quant: %s has no weight quantizer' % type(layer).__name__)
    if not hasattr(layer.weight_quant, 'msb_clamp_bit_width_impl'):
        raise TypeError('freeze_weight_quant: the weight quantizer %s has no bit-width module '
                        '(msb_clamp_bit_width_impl) for the frozen quant_weight() to report'
                        % type(layer.weight_quant).__name__)
    for key, t in (('frozen_weight_scale', scale), ('frozen_weight_zero_point', zero_point)):
        t = t.detach().clone().to(layer.weight.device)
        if key in layer._buffers:
            layer._buffers[key] = t
        else:
            layer.register_buffer(key, t)


def unfreeze_weight_quant(layer) -> None:
    """the layer's own weight quantizer runs again (the buffers and their state-dict keys go)"""
    for key in ('frozen_weight_scale', 'frozen_weight_zero_point'):
        if key in layer._buffers:
            del layer._buffers[key]


# ---- the context manager ---------------------------------------------------------------------------------------------

class _StopForward(Exception):
    """raised by the current layer once it has seen its input: nothing behind it is needed"""


class gptq_mode:
    """with gptq_mode(model) as gptq: per layer, calibration forwards through `gptq.model(batch)` then `gptq.update()`.

    Layers: every QuantLinear, and QuantConv2d with groups == 1 (through F.unfold), that has a weight quantizer and is
    not frozen, in module order.  Only the current layer accumulates its Hessian
    H = H * N / (N + n) + 2 / (N + n) * X^T X per batch X [n, K] of float32 rows -- from the tensor its float op consumes,
    after `input_quant` where there is one -- and each forward stops behind it.  update() quantizes the current layer's
    weight (gptq_quantize_weight), writes Q into `layer.weight.data`, freezes the layer and moves on: the next layer
    calibrates on the output of the frozen ones."""

    def __init__(self, model: torch.nn.Module, percdamp: float = 0.01, static_groups: bool = False):
        self._model = model
        self.percdamp = float(percdamp)
        self.static_groups = bool(static_groups)
        self.layers = []
        self.current = 0
        self._h = None
        self._n = 0

    @property
    def num_layers(self) -> int:
        return len(self.layers)

    who = 'gptq'  # the algorithm the refusals speak for (gpfq_mode: 'gpfq', with this _admit)

    # What a mode with the same protocol (graph/awq.py) states for itself: _admit, _reset, _accumulate, _quantize and
    # _freeze.
    def _admit(self, name: str, m) -> None:
        """the refusal of a layer that has a weight quantizer and is not frozen, or nothing"""
        from brevitas_amd.nn import QuantConv2d, QuantLinear
        if not isinstance(m, (QuantLinear, QuantConv2d)) or (isinstance(m, QuantConv2d) and m.groups != 1):
            raise NotImplementedError('%s_mode: layer %r (%s%s) is not covered: QuantLinear, and QuantConv2d with '
                                      'groups == 1' % (self.who, name, type(m).__name__,
                                                       ', groups=%d' % m.groups if hasattr(m, 'groups') else ''))
        _plan(m.weight_quant, m.weight.numel() // m.weight.shape[0], self.static_groups, who=self.who)

    def _reset(self) -> None:
        """nothing collected for the current layer yet"""
        self._h, self._n = None, 0

    def _accumulate(self, rows: Tensor) -> None:
        """one batch of float32 input rows [n, K] of the current layer"""
        n = rows.shape[0]
        if self._h is None:
            self._h = torch.zeros(rows.shape[1], rows.shape[1], dtype=torch.float32, device=rows.device)
        total = self._n + n
        self._h = self._h * (self._n / total) + (2.0 / total) * torch.matmul(rows.t(), rows)
        self._n = total

    def __enter__(self):
        from brevitas_amd.nn import _QuantWeightMixin
        self.layers = []
        for name, m in self._model.named_modules():
            if not isinstance(m, _QuantWeightMixin) or m.weight_quant is None or \
                    getattr(m, 'frozen_weight_scale', None) is not None:
                continue
            self._admit(name, m)  # refusals, before any work
            self.layers.append((name, m))
        self.current = 0
        self._arm()
        return self

    def __exit__(self, *exc):
        self._disarm()
        return False

    # the current layer's forward is replaced by one that accumulates H and stops
    def _arm(self):
        self._reset()
        if self.current < len(self.layers):
            self.layers[self.current][1].forward = self._capture

    def _disarm(self):
        if self.current < len(self.layers):
            self.layers[self.current][1].__dict__.pop('forward', None)

    def _capture(self, x):
        layer = self.layers[self.current][1]
        if layer.input_quant is not None and not getattr(layer, 'bvq_disable_input_quant', False):
            x = layer.input_quant(x)[0]
        with torch.no_grad():
            x = x.detach()
            if isinstance(layer, torch.nn.Conv2d):
                cols = F.unfold(x, layer.kernel_size, dilation=layer.dilation, padding=layer.padding,
                                stride=layer.stride)                       # [N, K, L], K = in * kh * kw
                rows = cols.transpose(1, 2).reshape(-1, cols.shape[1])
            else:
                rows = x.reshape(-1, x.shape[-1])
            self._accumulate(rows.float())
        raise _StopForward()

    def model(self, *args, **kwargs):
        """one calibration forward: runs the model up to the current layer"""
        try:
            return self._model(*args, **kwargs)
        except _StopForward:
            return None

    def update(self):
        """quantize the current layer from the Hessian collected so far, freeze it, move to the next"""
        who = type(self).__name__
        if self.current >= len(self.layers):
            raise RuntimeError('%s.update: every layer has been quantized already' % who)
        name, layer = self.layers[self.current]
        if self._h is None:
            raise RuntimeError('%s.update: layer %r has seen no calibration batch' % (who, name))
        res = self._quantize(name, layer)
        self._disarm()
        layer.weight.data.copy_(res.q)
        self._freeze(layer, res)
        self.current += 1
        self._arm()
        return res

    def _quantize(self, name: str, layer):
        """the current layer's result from what was collected: q, scale and zero_point at least"""
        return gptq_quantize_weight(layer.weight, self._h.to(layer.weight.device), layer.weight_quant,
                                    percdamp=self.percdamp, static_groups=self.static_groups, name=name)

    def _freeze(self, layer, res) -> None:
        freeze_weight_quant(layer, res.scale, res.zero_point)
