"""AWQ activation-aware weight scaling (Lin et al., 2023; no reference counterpart).

Before a group-wise quantizer rounds a linear weight w [R, K], AWQ multiplies every input column by a factor s [K] that
grows with the size of that input channel's activations, and divides the factor out again afterwards: columns that
matter lose less to the rounding.  s = act_mean^ratio, normalised, and the ratio is found by a grid search of n_grid
candidates under the layer's output error tr(dW H dW^T), H the input Hessian gptq_mode accumulates.  DESIGN.md §9 and
include/bvq.h ("AWQ") state the definition; two routes compute a candidate with the same bits:

  * fused: every candidate of a step in one bvq_group_awq_fwd launch (csrc/bvq_group_awq.hip: the weight is read once
    and stays in registers) -- device tensors, config.FUSED_PATHS, the quantizer graph the group kernels recognise;
  * composed: per candidate torch.mul, the quantizer's own sub-modules on the regrouped tensor (as GPTQ computes the
    groups of its loop), torch.div -- CPU tensors, misaligned tensors, config.FUSED_PATHS off.

Both hand their candidates to the same loss function.

    with awq_mode(model) as awq:
        for _ in range(awq.num_layers):
            for batch in loader:
                awq.model(batch)
            awq.update()

update() writes the dequantized codes Q into `layer.weight.data`, freezes the layer as GPTQ does and registers the
buffer `awq_input_scale` [K]: the integer codes of the layer are round(weight * awq_input_scale / scale + zero_point).

AWQ's second stage, the activation-aware clip search (`auto_clip` of the paper's code), is awq_clip_weight, and
awq_mode(model, clip=True) runs it behind the column-factor search: per group of the scaled weight the threshold
abs-max * ratio_i whose output error d^T H_jj d under the calibration activations is smallest ("AWQ clip
search"), all candidates of all groups in one bvq_group_clip_fwd launch (csrc/bvq_group_clip.hip) or composed from the
quantizer's sub-modules and one einsum per candidate.  Symmetric group-wise quantizers only.

Folding 1 / s into a preceding layer, a clip search for asymmetric groups, convolutions and a backward are out of
scope."""
from typing import Iterator, NamedTuple, Optional, Tuple

import torch
from torch import Tensor

import brevitas_amd.config as config
from brevitas_amd import _aten
from brevitas_amd import _native as nat
from brevitas_amd.core.quant import _fused
from brevitas_amd.core.quant.int import (GroupwiseHQOIntQuant, GroupwiseMSEIntQuant, GroupwiseRescalingIntQuant,
                                         RescalingIntQuant, check_mse_ratios)
from brevitas_amd.graph import gptq

__all__ = ['awq_mode', 'awq_scale_weight', 'awq_candidates', 'awq_losses', 'awq_table', 'AWQResult',
           'freeze_awq_weight', 'awq_clip_weight', 'awq_clip_ratios', 'hessian_blocks', 'AWQClipResult']


class AWQResult(NamedTuple):
    q: Tensor            # the dequantized codes with the column factor divided out, shaped and typed like the weight
    scale: Tensor        # shaped as the quantizer returns it; the scale of weight * input_scale
    zero_point: Tensor
    bit_width: Tensor
    input_scale: Tensor  # [K] in the weight's dtype: the kept column factor
    index: int           # the kept candidate
    losses: Tensor       # float32 [n_grid]


class AWQClipResult(NamedTuple):
    q: Tensor            # the dequantized codes with the column factor divided out, shaped and typed like the weight
    scale: Tensor        # [R, K / g, 1]: the scale of weight * input_scale at the kept threshold
    zero_point: Tensor
    bit_width: Tensor
    index: Tensor        # uint8 [R, K / g]: the kept candidate of every group
    losses: Tensor       # float32 [R, K / g, n]: every candidate's output error, of the scaled weight


def _plan(quantizer, k: int) -> 'gptq._Plan':
    """what the composed route needs to know of `quantizer` (GPTQ's plan of a group-wise quantizer whose parameters are
    computed from the groups at hand), or the TypeError naming what is refused"""
    name = type(quantizer).__name__
    if isinstance(quantizer, (GroupwiseMSEIntQuant, GroupwiseHQOIntQuant)):
        raise TypeError('awq: the searching quantizer %s is not covered (its search per group and the search of the '
                        'column factor would have to be one search)' % name)
    if type(quantizer) is RescalingIntQuant:
        raise TypeError('awq: the per-tensor or per-channel quantizer %s is not covered (a scale shared by a whole row '
                        'does not survive a factor per column; group-wise quantizers only)' % name)
    if type(quantizer) is not GroupwiseRescalingIntQuant:
        raise TypeError('awq: the quantizer %s is not covered (group-wise integer weight quantizers only)' % name)
    return gptq._plan(quantizer, k, False, who='awq')


def awq_table(act_mean: Tensor, n_grid: int, dtype: torch.dtype) -> Tensor:
    """the candidate column factors [n_grid, K] in `dtype`, on act_mean's device: row i is act_mean^(i / n_grid),
    bounded below by 1e-4 and divided by sqrt(max * min), as the AWQ reference implementation forms it.  Computed on the
    host in float32, so that every device searches the same table; row 0 is exactly ones."""
    if int(n_grid) < 1:
        raise ValueError('awq: n_grid must be positive, got %r' % (n_grid,))
    am = act_mean.detach().to(device='cpu', dtype=torch.float32).reshape(-1)
    rows = []
    for i in range(int(n_grid)):
        s = am.pow(i / int(n_grid)).clamp(min=1e-4)
        rows.append(s / (s.max() * s.min()).sqrt())
    return torch.stack(rows).to(device=act_mean.device, dtype=dtype)


def _fused_args(plan: 'gptq._Plan', w2: Tensor, table: Tensor):
    """(descriptor, min_val, thr_div) of bvq_group_awq_fwd, or None: the configuration, the quantizer's graph or the
    tensors are not what the kernel covers"""
    if not (w2.is_cuda and config.FUSED_PATHS and w2.dtype in _fused._FLOATS):
        return None
    tmpl = plan.quant._group_template(plan.bit_width)
    if tmpl is None or tmpl.shifted != plan.shifted:
        return None
    desc, thr_div = _fused.unit_call(w2, plan.group, tmpl.shifted, tmpl.int_thr, tmpl.qmin, tmpl.qmax, tmpl.clamp_ste)
    if not nat.group_awq_supported(desc, w2, table):
        return None
    return desc, tmpl.min_val, thr_div


def _composed(plan: 'gptq._Plan', w2: Tensor, factors: Tensor):
    """one candidate in plain torch ops and the quantizer's own sub-modules
    -> (y [R, K], scale [groups, 1], zero-point)"""
    xg = (w2 * factors).reshape(-1, plan.group)
    scale, zp = gptq._group_params(plan, xg)
    yq = plan.quant.int_quant(scale, zp, plan.bit_width, xg)
    return yq.reshape(w2.shape) / factors, scale, zp


def _steps(weight: Tensor, table: Tensor, quantizer) -> Iterator[Tuple[int, Tensor, Tensor, Tensor]]:
    """The candidates of `table` in steps of as many as fit config.AWQ_CANDIDATE_BYTES (one at least): yields
    (index of the step's first candidate, y [m, R, K], scale [m, R, K / g, 1], zero_point likewise -- or the quantizer's
    own zero where it has no zero-point per group).  A step is one launch on the fused route."""
    rows = weight.shape[0]
    w2 = weight.detach().reshape(rows, -1).contiguous()
    k = w2.shape[1]
    if table.dim() != 2 or table.shape[1] != k or table.dtype != w2.dtype or table.device != w2.device:
        raise ValueError('awq: a table of shape %s, %s on %s for a weight with %d input columns, %s on %s'
                         % (tuple(table.shape), table.dtype, table.device, k, w2.dtype, w2.device))
    plan = _plan(quantizer, k)
    table = table.detach()
    per = max(1, min(nat.AWQ_MAX_CANDIDATES, config.AWQ_CANDIDATE_BYTES // max(w2.numel() * w2.element_size(), 1)))
    shape = (-1, rows, k // plan.group, 1)
    for i0 in range(0, table.shape[0], per):
        tab = table[i0:i0 + per]
        fa = _fused_args(plan, w2, tab)
        if fa is not None:
            y, scale, zp = nat.group_awq_fwd(fa[0], w2, tab, fa[1], fa[2])
        else:
            ys, scales, zps = zip(*[_composed(plan, w2, tab[i]) for i in range(tab.shape[0])])
            y, scale = torch.stack(ys), torch.stack(scales)
            zp = torch.stack(zps) if plan.shifted else None
        scale = scale.reshape(shape)
        zp = zp.reshape(shape) if plan.shifted else quantizer.zero_point_impl(w2, scale, plan.bit_width)
        yield i0, y, scale, zp


def awq_candidates(weight: Tensor, table: Tensor, quantizer) -> Tuple[Tensor, Tensor, Tensor]:
    """Every candidate of `table` [n, K] (column factors in the weight's dtype, on its device) for `weight` ([R, ...],
    flattened to [R, K]) under `quantizer`, the weight's own group-wise weight quantizer: -> (y [n, R, K], scale
    [n, R, K / g, 1], zero_point likewise, or the quantizer's own zero where it has none per group).  y[i] is the weight
    with its columns multiplied by table[i], quantized, and the factors divided out again."""
    with torch.no_grad():
        steps = list(_steps(weight, table, quantizer))
        if len(steps) == 1:
            return steps[0][1:]
        shifted = steps[0][3].dim() == 4
        return (torch.cat([s[1] for s in steps]), torch.cat([s[2] for s in steps]),
                torch.cat([s[3] for s in steps]) if shifted else steps[0][3])


def awq_losses(y: Tensor, weight: Tensor, hessian: Tensor) -> Tensor:
    """float32 [n]: tr(d_i H d_i^T) = ||d_i X||^2 up to H's constant, d_i = y[i] - weight in float32, H [K, K] as
    gptq_mode accumulates it.  One candidate at a time, so that a candidate's loss does not depend on its neighbours."""
    with torch.no_grad():
        wf = weight.detach().reshape(y.shape[1:]).float()
        h = hessian.detach().to(device=y.device, dtype=torch.float32)
        out = torch.empty(y.shape[0], dtype=torch.float32, device=y.device)
        for i in range(y.shape[0]):
            d = y[i].float() - wf
            out[i] = (torch.matmul(d, h) * d).sum()
        return out


def awq_scale_weight(weight: Tensor, hessian: Tensor, act_mean: Tensor, quantizer, *, n_grid: int = 20,
                     name: str = '') -> AWQResult:
    """The AWQ search for `weight` ([R, ...], flattened to [R, K]) under `hessian` ([K, K]) and `act_mean` ([K]: the
    mean of |x| per input column), both as awq_mode accumulates them, with the codes of `quantizer`, the weight's own
    group-wise weight quantizer.  Keeps the first candidate with the smallest finite loss.  Nothing is changed in place.
    name: the layer's, for the error of a search without a finite loss."""
    with torch.no_grad():
        k = weight.numel() // weight.shape[0]
        if act_mean.numel() != k or tuple(hessian.shape) != (k, k):
            raise ValueError('awq: act_mean of %d entries and a Hessian of shape %s for %d input columns'
                             % (act_mean.numel(), tuple(hessian.shape), k))
        table = awq_table(act_mean, n_grid, weight.dtype).to(weight.device)
        best, best_loss, losses = None, None, []
        for i0, y, scale, zp in _steps(weight, table, quantizer):
            step = awq_losses(y, weight, hessian)
            losses.append(step)
            host = step.cpu()
            host = torch.where(torch.isfinite(host), host, torch.full_like(host, float('inf')))
            j = int(torch.argmin(host))  # the first of equal minima
            if torch.isfinite(host[j]) and (best is None or float(host[j]) < best_loss):
                best_loss = float(host[j])
                best = (i0 + j, y[j].clone(), scale[j].clone(), zp[j].clone() if zp.dim() == 4 else zp)
        if best is None:
            raise RuntimeError('awq: no candidate of layer %r has a finite loss; check the calibration data (act_mean, '
                               'Hessian) and the weight for NaN or inf' % name)
        index, q, scale, zp = best
        bit_width = quantizer.msb_clamp_bit_width_impl()
        return AWQResult(q.reshape(weight.shape), scale, zp, bit_width, table[index].clone(), index, torch.cat(losses))


# ---- the clip search -------------------------------------------------------------------------------------------------

def awq_clip_ratios(n_grid: int = 20, max_shrink: float = 0.5) -> Tensor:
    """the candidate ratios of the clip search, float32 on the host: 1 - i / n_grid for i < int(max_shrink * n_grid), as
    the AWQ reference implementation walks them; formed in float32 so that every device searches the same thresholds.
    At least one, at most 16 (the kernel's candidate count)."""
    if int(n_grid) < 1:
        raise ValueError('awq: n_grid must be positive, got %r' % (n_grid,))
    n = int(float(max_shrink) * int(n_grid))
    if n > nat.CLIP_MAX_CANDIDATES:
        raise ValueError('awq: %d clip ratios (max_shrink=%r of n_grid=%r); at most %d'
                         % (n, max_shrink, n_grid, nat.CLIP_MAX_CANDIDATES))
    ratios = 1.0 - torch.arange(n, dtype=torch.float32) / torch.tensor(float(n_grid), dtype=torch.float32)
    check_mse_ratios(ratios.tolist())
    return ratios


def hessian_blocks(hessian: Tensor, g: int, input_scale: Optional[Tensor] = None) -> Tensor:
    """float32 [K / g, g, g], contiguous: block j is hessian[j g:(j + 1) g, j g:(j + 1) g], what the output error of a
    change inside group j depends on.  input_scale [K]: the blocks for a weight whose columns were multiplied by it --
    entry (a, b) divided by s_a * s_b in float32, so that d^T block d is the error of d / s."""
    k = hessian.shape[0]
    if hessian.dim() != 2 or hessian.shape[1] != k or int(g) < 1 or k % int(g):
        raise ValueError('awq: a Hessian of shape %s has no diagonal blocks of %r columns' % (tuple(hessian.shape), g))
    nj = k // int(g)
    j = torch.arange(nj, device=hessian.device)
    hb = hessian.detach().float().reshape(nj, g, nj, g)[j, :, j, :]
    if input_scale is not None:
        s = input_scale.detach().to(device=hb.device, dtype=torch.float32).reshape(nj, g)
        hb = hb / (s[:, :, None] * s[:, None, :])
    return hb.contiguous()


def _clip_fused_args(plan: 'gptq._Plan', x: Tensor, hb: Tensor, n: int):
    """(descriptor, min_val, thr_div) of bvq_group_clip_fwd, or None: the configuration, the quantizer's graph or the
    tensors are not what the kernel covers"""
    if not (x.is_cuda and config.FUSED_PATHS and x.dtype in _fused._FLOATS):
        return None
    tmpl = plan.quant._group_template(plan.bit_width)
    if tmpl is None or tmpl.shifted:
        return None
    desc, thr_div = _fused.unit_call(x, plan.group, False, tmpl.int_thr, tmpl.qmin, tmpl.qmax, tmpl.clamp_ste)
    if not nat.group_clip_supported(desc, x, hb, n):
        return None
    return desc, tmpl.min_val, thr_div


def awq_clip_weight(weight: Tensor, hessian: Tensor, quantizer, *, ratios=None, input_scale: Optional[Tensor] = None,
                    name: str = '') -> AWQClipResult:
    """AWQ's clip search for `weight` ([R, ...], flattened to [R, K]) under `hessian` ([K, K], as awq_mode accumulates
    it) with the codes of `quantizer`, the weight's own symmetric group-wise quantizer.  Per row and group of
    x = weight * input_scale (one torch.mul in the weight's dtype; the weight itself without a factor) the threshold
    abs-max * ratios[i] is kept whose loss d^T hb d is the first strict minimum, d = y_i - x in float32 and hb =
    hessian_blocks(hessian, g, input_scale): the loss is that of the SCALED weight under the blocks divided by the
    factors, which is the output error of q = y / input_scale.  ratios: awq_clip_ratios() unless given (float32, the
    first 1, at most 16).  Nothing is changed in place.  name: the layer's, for the errors."""
    with torch.no_grad():
        rows = weight.shape[0]
        w2 = weight.detach().reshape(rows, -1).contiguous()
        k = w2.shape[1]
        plan = _plan(quantizer, k)
        if plan.shifted:
            raise TypeError('awq: the clip search of layer %r does not cover the asymmetric quantizer %s (its zero-point '
                            'moves with the threshold; symmetric group-wise quantizers only)'
                            % (name, type(quantizer).__name__))
        if tuple(hessian.shape) != (k, k) or (input_scale is not None and input_scale.numel() != k):
            raise ValueError('awq: a Hessian of shape %s%s for %d input columns'
                             % (tuple(hessian.shape), '' if input_scale is None else
                                ' and an input_scale of %d entries' % input_scale.numel(), k))
        ratios = awq_clip_ratios() if ratios is None else torch.as_tensor(ratios, dtype=torch.float32).cpu()
        table = check_mse_ratios(ratios.tolist())
        if len(table) > nat.CLIP_MAX_CANDIDATES:
            raise ValueError('awq: %d clip ratios; at most %d' % (len(table), nat.CLIP_MAX_CANDIDATES))
        g, q = plan.group, plan.quant
        if input_scale is not None:
            input_scale = input_scale.detach().to(device=w2.device, dtype=w2.dtype).reshape(k)
        x = w2 if input_scale is None else w2 * input_scale
        hb = hessian_blocks(hessian.to(w2.device), g, input_scale)
        fa = _clip_fused_args(plan, x, hb, len(table))
        if fa is not None:
            y, scale, _, index, losses = nat.group_clip_fwd(fa[0], x, hb, nat.mse_ratio_table(table), fa[1], fa[2])
        else:
            xg = x.reshape(-1, g)
            sc = q.scaling_impl
            stat = sc.parameter_list_stats.stats.stats_impl(xg).reshape(-1, 1)  # of the groups at hand (gptq._group_params)
            int_threshold = q.int_scaling_impl(plan.bit_width)

            def scale_of(threshold):
                return sc.stats_scaling_impl(threshold) / int_threshold

            def quantize(s):
                return q.int_quant(s, q.zero_point_impl(xg, s, plan.bit_width), plan.bit_width, xg)
            index, losses = _aten.group_clip_index(xg, hb, table, stat, scale_of, quantize)
            y, scale = _aten.group_mse_quantize_at(table, index.reshape(-1), stat, scale_of, quantize)
        y = y.reshape(rows, k)
        scale = scale.reshape(rows, k // g, 1)
        return AWQClipResult((y if input_scale is None else y / input_scale).reshape(weight.shape), scale,
                             q.zero_point_impl(w2, scale, plan.bit_width), plan.bit_width, index.reshape(rows, k // g),
                             losses)


def freeze_awq_weight(layer, scale: Tensor, zero_point: Tensor, input_scale: Tensor) -> None:
    """freeze_weight_quant, and the buffer `awq_input_scale` [K] that says which column factor the codes were taken
    under: codes = round(weight * awq_input_scale / scale + zero_point).  (By hand: to load a checkpoint of a searched
    model into a fresh one.)"""
    gptq.freeze_weight_quant(layer, scale, zero_point)
    t = input_scale.detach().clone().to(layer.weight.device)
    if 'awq_input_scale' in layer._buffers:
        layer._buffers['awq_input_scale'] = t
    else:
        layer.register_buffer('awq_input_scale', t)


class awq_mode(gptq.gptq_mode):
    """with awq_mode(model) as awq: per layer, calibration forwards through `awq.model(batch)` then `awq.update()`:
    gptq_mode's protocol and its capture of the current layer's input.

    Layers: every QuantLinear with a GroupwiseRescalingIntQuant weight quantizer (symmetric or asymmetric, constant bit
    width, half-even rounding) that is not frozen, in module order; anything else with a weight quantizer is refused on
    entry.  Next to the Hessian the current layer accumulates the mean of |x| per input column, from the same rows.
    update() searches the column factor (awq_scale_weight), writes Q into `layer.weight.data`, freezes the layer
    (freeze_awq_weight) and moves on: the next layer calibrates on the output of the frozen ones.

    clip=True: behind the column-factor search update() runs the clip search on the kept factor (awq_clip_weight with
    awq_clip_ratios(n_grid, max_shrink)) and freezes the layer from its q and scale; the AWQClipResult of the last
    layer is `last_clip`.  Symmetric quantizers only then: an asymmetric one is refused on entry."""

    def __init__(self, model: torch.nn.Module, n_grid: int = 20, clip: bool = False, max_shrink: float = 0.5):
        super().__init__(model)
        if int(n_grid) < 1:
            raise ValueError('awq_mode: n_grid must be positive, got %r' % (n_grid,))
        self.n_grid = int(n_grid)
        self.clip = bool(clip)
        self.clip_ratios = awq_clip_ratios(n_grid, max_shrink) if self.clip else None
        self.last_clip = None
        self._abs = None

    def _admit(self, name: str, m) -> None:
        from brevitas_amd.nn import QuantLinear
        if not isinstance(m, QuantLinear):
            raise NotImplementedError('awq_mode: layer %r (%s with the weight quantizer %s) is not covered: '
                                      'QuantLinear only' % (name, type(m).__name__, type(m.weight_quant).__name__))
        if _plan(m.weight_quant, m.weight.shape[1]).shifted and self.clip:
            raise TypeError('awq_mode: layer %r: the clip search does not cover the asymmetric quantizer %s'
                            % (name, type(m.weight_quant).__name__))

    def _reset(self) -> None:
        super()._reset()
        self._abs = None

    def _accumulate(self, rows: Tensor) -> None:
        super()._accumulate(rows)
        s = rows.abs().sum(0)
        self._abs = s if self._abs is None else self._abs + s

    @property
    def act_mean(self) -> Optional[Tensor]:
        """float32 [K]: the mean of |x| per input column over the rows the current layer has seen"""
        return None if self._abs is None else self._abs / self._n

    def _quantize(self, name: str, layer) -> AWQResult:
        dev = layer.weight.device
        res = awq_scale_weight(layer.weight, self._h.to(dev), self.act_mean.to(dev), layer.weight_quant,
                               n_grid=self.n_grid, name=name)
        if not self.clip:
            return res
        self.last_clip = awq_clip_weight(layer.weight, self._h.to(dev), layer.weight_quant, ratios=self.clip_ratios,
                                         input_scale=res.input_scale, name=name)
        return res._replace(q=self.last_clip.q, scale=self.last_clip.scale, zero_point=self.last_clip.zero_point)

    def _freeze(self, layer, res: AWQResult) -> None:
        freeze_awq_weight(layer, res.scale, res.zero_point, res.input_scale)
