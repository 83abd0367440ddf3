"""GPFQ weight quantization: greedy path-following quantization (Lybrand & Saab, 2021; Zhang, Zhou & Saab, 2023;
`gpfq_mode` of later Brevitas releases, no reference counterpart).

Once the layers in front of a layer are quantized, the input X~ that the layer sees on the quantized path is no longer
the input X the float model would have fed it.  GPTQ and AWQ measure their error on X~ alone; GPFQ picks each input
column's code so that X~ Q^T follows X W^T, the float layer on the float input.  It needs two statistics [K, K], the Gram
matrix H = mean X~^T X~ and the drift D = mean (X - X~)^T X~, and no factorisation, so a singular H is no failure: a
column whose input never fired is rounded to nearest.  Scale, zero-point and bit width are the quantizer's own, taken
once from the original weight, which is never changed.  DESIGN.md §9 and include/bvq.h ("GPFQ") state the definition;
two routes compute it with the same bits:

  * fused: one bvq_gpfq_block launch per block of 128 columns (csrc/bvq_gpfq.hip: one wave per row, the block's weight
    and running correction in registers) -- device tensors, config.FUSED_PATHS, 16-byte aligned, any group size;
  * composed: plain torch ops per column, written from the quantizer's own IntQuant -- CPU tensors, tensors the kernel
    refuses, config.FUSED_PATHS off.

Both share the product Wf @ triu(D) that starts the running correction and its float32 update right of a block.

    with gpfq_mode(model) as gpfq:
        for _ in range(gpfq.num_layers):
            for batch in loader:
                gpfq.model(batch)      # two forwards up to the current layer: a float one, then a quantized one
            gpfq.update()

update() writes Q into `layer.weight.data` and freezes the layer exactly as gptq_mode does.  The accumulator-aware
variant (GPFA2Q), act_order and the subsampling of the calibration rows are out of scope; the searching quantizers (MSE
clip, HQO) are refused as in GPTQ."""
from typing import NamedTuple, Optional

import torch
from torch import Tensor

from brevitas_amd import _native as nat
from brevitas_amd.graph import gptq
from brevitas_amd.graph.calibrate import DisableEnableQuantization

__all__ = ['gpfq_mode', 'gpfq_quantize_weight', 'GPFQResult']

BLOCK = gptq.BLOCK


class GPFQResult(NamedTuple):
    q: Tensor            # the dequantized codes, shaped and typed like the weight
    scale: Tensor        # as the quantizer returns them on the original weight
    zero_point: Tensor
    bit_width: Tensor


def _plan(quantizer, k: int) -> 'gptq._Plan':
    """GPTQ's plan with given parameters (there is nothing to compute in the loop: the weight the statistics come from
    never changes), or the error naming what is refused"""
    return gptq._plan(quantizer, k, True, who='gpfq')


def initial_correction(wf: Tensor, d: Tensor) -> Tensor:
    """C = Wf @ triu(D), diagonal included: one float32 matrix product, the working copy [R, K]"""
    return torch.matmul(wf, torch.triu(d))


def tail_update(c: Tensor, err: Tensor, h: Tensor, c0: int, c1: int) -> None:
    """C[:, c1:] += E @ H[c0:c1, c1:], one float32 matrix product"""
    if c1 < c.shape[1]:
        c[:, c1:] += torch.matmul(err, h[c0:c1, c1:])


def composed_block(plan: 'gptq._Plan', wf: Tensor, c: Tensor, h: Tensor, c0: int, c1: int, q: Tensor, scale: Tensor,
                   zp: Optional[Tensor]) -> Tensor:
    """the column loop of the block [c0, c1) in plain torch ops: wf (float32, read only), the block's columns of c
    (float32, updated in place) -> the block's columns of q, and E [R, c1 - c0].  A group may have begun before the
    block: its parameters are read at the block's first column."""
    block = gptq._ComposedBlock(plan, wf, c0, c1, q, scale, zp)
    cb = c[:, c0:c1]
    for i, col, s, z in block.columns():
        w = wf[:, col]
        hd = h[col, col]  # a tensor on wf's device: the division below is IEEE's, no product with a reciprocal
        # the quotient rounded, then the sum; a column whose input never fired is rounded to nearest
        v = torch.where(hd > 0, w + cb[:, i] / hd, w)
        qc = plan.quant.int_quant(s, z, plan.bit_width, v.to(q.dtype).reshape(-1, 1).contiguous())[:, 0]
        e = w - qc.float()  # against the original weight, not v
        block.store(i, qc, e)
        if i + 1 < c1 - c0:
            # the product rounded, then the sum: two ops, no fused multiply-add
            cb[:, i + 1:] += e.reshape(-1, 1) * h[col, col + 1:c1].reshape(1, -1)
    return block.err


def fused_block_desc(plan: 'gptq._Plan', rows: int, k: int, dtype: torch.dtype) -> Optional['nat.QuantDesc']:
    """the descriptor of bvq_gpfq_block for a weight [rows, k] of `dtype` (that of bvq_gptq_block with given
    parameters), or None: the quantizer's graph or the configuration is not what the kernel covers (tensors apart)"""
    fa = gptq.fused_block_args(plan, rows, k, dtype)
    return None if fa is None else fa.desc


def fused_block(desc, wf: Tensor, c: Tensor, h: Tensor, c0: int, c1: int, q: Tensor, scale: Tensor,
                zp: Optional[Tensor]) -> Tensor:
    """composed_block as one bvq_gpfq_block launch (c is read only: the block's columns are finished)"""
    return nat.gpfq_block(desc, wf, c, h, c0, c1 - c0, q, scale, zp)


def gpfq_quantize_weight(weight: Tensor, h: Tensor, d: Tensor, quantizer, *, name: str = '') -> GPFQResult:
    """GPFQ of `weight` ([R, ...], flattened to [R, K]) under the statistics `h` and `d` ([K, K] each, accumulated as
    gpfq_mode does: H = mean X~^T X~, D = mean (X - X~)^T X~ with one weighting) with the codes, scales and zero-points
    of `quantizer`, the weight's own weight quantizer.  Nothing is changed in place.  name: the layer's, for errors."""
    with torch.no_grad():
        rows = weight.shape[0]
        w2 = weight.detach().reshape(rows, -1)
        k = w2.shape[1]
        plan = _plan(quantizer, k)
        for what, t in (('H', h), ('D', d)):
            if tuple(t.shape) != (k, k):
                raise ValueError('gpfq: %s of shape %s for the %d input columns of layer %r'
                                 % (what, tuple(t.shape), k, name))
        scale, zp, scale_out, zp_out = gptq._given_params(plan, weight)
        wf = w2.float().contiguous()
        hf = h.detach().to(device=wf.device, dtype=torch.float32).contiguous()
        c = initial_correction(wf, d.detach().to(device=wf.device, dtype=torch.float32))
        q = torch.empty(rows, k, dtype=weight.dtype, device=weight.device)

        desc = fused_block_desc(plan, rows, k, weight.dtype) if weight.is_cuda else None
        gptq.walk_blocks(k, lambda c0, c1: nat.gpfq_block_supported(desc, wf, c, hf, q, c0, c1 - c0),
                         None if desc is None else lambda c0, c1: fused_block(desc, wf, c, hf, c0, c1, q, scale, zp),
                         lambda c0, c1: composed_block(plan, wf, c, hf, c0, c1, q, scale, zp),
                         lambda err, c0, c1: tail_update(c, err, hf, c0, c1))
        return GPFQResult(q.reshape(weight.shape), scale_out, zp_out, plan.bit_width)


class gpfq_mode(gptq.gptq_mode):
    """with gpfq_mode(model) as gpfq: per layer, calibration forwards through `gpfq.model(batch)` then `gpfq.update()`:
    gptq_mode's protocol, layers (QuantLinear, and QuantConv2d with groups == 1 through F.unfold) and freezing.

    One `gpfq.model(batch)` call runs the model twice up to the current layer.  First a float pass: every quantizer off
    (DisableEnableQuantization, in eval mode, so that no statistic moves) and the ORIGINAL weights of the layers this
    mode has finished swapped in for its duration -- update() keeps each finished layer's original weight, and __exit__
    releases them all.  Then a quantized pass, the model as it stands.  The current layer's input rows of the two passes,
    X and X~ [n, K] in float32, enter the statistics as a pair, with gptq_mode's running-mean weighting for both:
        H = H * N / (N + n) + 2 / (N + n) * X~^T X~,    D = D * N / (N + n) + 2 / (N + n) * (X - X~)^T X~.
    A layer that was frozen before the mode was entered has no original weight left: it runs as it stands in both
    passes, and the float path is then float only from that layer on."""

    who = 'gpfq'

    def __init__(self, model: torch.nn.Module):
        super().__init__(model, static_groups=True)  # given parameters, which is also what gptq_mode._admit plans with
        self._d = None
        self._float_rows = None
        self._float_pass = False
        self._originals = {}  # finished layer -> its original weight
        self._switch = DisableEnableQuantization()

    def _reset(self) -> None:
        super()._reset()
        self._d, self._float_rows = None, None

    def _accumulate(self, rows: Tensor) -> None:
        """the float pass leaves its rows X; the quantized pass brings X~ and both enter H and D"""
        if self._float_pass:
            self._float_rows = rows
            return
        x, self._float_rows = self._float_rows, None
        if x is None or x.shape != rows.shape:
            raise RuntimeError('gpfq_mode: the float pass left %s input rows for layer %r and the quantized pass %s; '
                               'calibrate through gpfq.model(batch)'
                               % ('no' if x is None else tuple(x.shape), self.layers[self.current][0],
                                  tuple(rows.shape)))
        n = rows.shape[0]
        if self._d is None:
            self._d = torch.zeros(rows.shape[1], rows.shape[1], dtype=torch.float32, device=rows.device)
        total = self._n + n
        self._d = self._d * (self._n / total) + (2.0 / total) * torch.matmul((x - rows).t(), rows)
        super()._accumulate(rows)

    def model(self, *args, **kwargs):
        """one calibration step: the float pass, then the quantized pass, each up to the current layer"""
        modes = [(m, m.training) for m in self._model.modules()]
        kept = []
        self._float_rows = None
        self._float_pass = True
        try:
            self._switch.apply(self._model, is_training=False, quantization_enabled=False)
            for layer, original in self._originals.items():
                kept.append((layer, layer.weight.data))
                layer.weight.data = original
            with torch.no_grad():
                super().model(*args, **kwargs)
        finally:
            self._float_pass = False
            for layer, data in kept:
                layer.weight.data = data
            self._switch.apply(self._model, is_training=False, quantization_enabled=True)
            for m, training in modes:
                m.training = training
        return super().model(*args, **kwargs)

    def _quantize(self, name: str, layer) -> GPFQResult:
        dev = layer.weight.device
        res = gpfq_quantize_weight(layer.weight, self._h.to(dev), self._d.to(dev), layer.weight_quant, name=name)
        self._originals[layer] = layer.weight.detach().clone()  # update() overwrites weight.data next
        return res

    def __exit__(self, *exc):
        self._originals.clear()
        return super().__exit__(*exc)
