"""WeightQuantGroup: every per-channel weight of a model quantized in one forward and one backward launch.

In QAT each layer re-quantizes its weight on every forward (proxy.tensor_quant(w) -> RescalingIntQuant.forward,
B/proxy/parameter_quant.py:83-89, B/core/quant/int.py:155-163): one statistic + quantizer launch, one backward launch and
one autograd node per weight, 50-100 us of host time each (profiles/r03_host_cost.txt).  Inside a group's block the first
weight quantizer that runs quantizes ALL the group's covered weights at once (_fused.WeightListFakeQuantFn: one
bvq_weight_quant_list_fwd launch per 16 weights, one node), and every member then returns its own slice of that result:

    group = WeightQuantGroup(model)
    for x, t in loader:
        with group:
            loss = criterion(model(x), t)
        loss.backward()
        opt.step()

Each weight gets the bits its own forward and backward give it.  The one difference: a layer called twice in one block
gets the same y, and its two gradients are summed by autograd before the one backward (equal to the two per-layer
backwards up to the order of that summation).

A member falls back to its own per-layer forward, unchanged, when the tensor it is handed is not its tracked weight
(identity, data_ptr, shape, stride), the weight changed in place since the group quantized it (`_version`), the grad mode
differs from the one the group quantized under (the first member call of the block decides), the weight is not covered
(`group.uncovered` says why), or its layer is calibrating (`bvq_disable_weight_quant`, `bvq_collect_only`).  A weight
that needs no gradient gets a y that needs none.  A captured step (HIP graph) runs the list backward when it is
captured on the stream its eager warm-up ran on; on another stream the backward takes the per-tensor route.
The group owns no parameters or buffers: state dicts are unchanged.
"""
from typing import List, NamedTuple, Optional, Tuple

import torch

from brevitas_amd import _native as nat
from brevitas_amd.core.function_wrapper.learned_round import LearnedRoundSte
from brevitas_amd.core.quant import _fused
from brevitas_amd.core.quant import int as _int
from brevitas_amd.core.quant.int import GroupwiseRescalingIntQuant, RescalingIntQuant

__all__ = ['WeightQuantGroup']


class _Member(NamedTuple):
    quant: RescalingIntQuant
    layer: Optional[torch.nn.Module]  # the module whose `weight` the quantizer tracks (calibration flags live there)


class _WeightList:
    """the static description of one (device, dtype, rounding) list of covered weights: the item array of include/bvq.h
    and what the per-tensor backward needs for each weight.  Rebuilt when a weight's storage, shape or dtype, a member
    or a member's template (bit width, integer range, clamp, statistic -> scale map) changes."""

    def __init__(self, entries):
        n = len(entries)
        self.items = (nat.WeightItem * n)()
        self.channels = [e.sp.channels for e in entries]
        self.shapes = [tuple(e.sp.scaling_shape) for e in entries]
        self.offsets = []
        self.descs = []
        self.sps = []
        # the int_threshold tensors (the per-tensor backward of a weight whose scale has a gradient reads them), taken
        # now: IntScaling creates its cached tensor on first use, which a capturing stream would not allow
        self.int_thresholds = [e.quant.int_scaling_impl(e.bit_width) for e in entries]
        w0 = entries[0].weight
        self.scale_dtype = w0.dtype  # a dimensioned scale keeps the weight's dtype (_fused.stats_scale)
        self.round_mode = entries[0].tmpl.round_mode
        # chunks: one list call each way, at most WEIGHT_LIST_MAX weights whose channels fit one arrival buffer
        self.chunks, self.chunk_of = [], []
        lo, off = 0, 0
        for i, e in enumerate(entries):
            if i > lo and (i - lo == nat.WEIGHT_LIST_MAX or off + e.sp.channels > nat.ARRIVE_WORDS):
                self.chunks.append((lo, i))
                lo, off = i, 0
            self.chunk_of.append(len(self.chunks))
            sp, t = e.sp, e.tmpl
            it = self.items[i]
            it.x = e.weight.data_ptr()
            it.channels = sp.channels
            it.inner = sp.inner
            it.min_val = float(sp.min_val or 0.0)
            it.use_min = int(bool(sp.min_val))
            it.int_threshold = _fused.scale_rule(w0.dtype, sp.scaling_shape, sp.int_threshold).thr_div
            it.qmin, it.qmax = t.qmin, t.qmax
            it.clamp_ste = int(t.clamp_ste)
            self.offsets.append(off)
            off += sp.channels
            self.descs.append(_fused.channel_desc(sp.outer, sp.channels, sp.inner, w0.dtype, t.qmin, t.qmax,
                                                  t.round_mode, t.clamp_ste))
            self.sps.append(_fused._SpLike(sp.outer, sp.channels, sp.inner, sp.int_threshold))
        self.chunks.append((lo, n))


class _Entry(NamedTuple):
    key: tuple
    quant: RescalingIntQuant
    weight: torch.Tensor
    sp: '_fused.StatsPlan'
    tmpl: tuple   # _recognise.StatsTemplate
    bit_width: torch.Tensor


def _weight_key(w):
    return (w.data_ptr(), tuple(w.shape), w.stride(), w.dtype, w.device)


class WeightQuantGroup:
    """Quantizes every covered per-output-channel weight of `module` in one launch each way, inside `with group:`.

    Members: every RescalingIntQuant of module.modules() whose recognised graph is a plain stats-scaled per-output-channel
    weight (AbsMax statistic of exactly the weight it quantizes, plain clamp_min -> / int_threshold, no shared quantizer).
    `covered` / `uncovered`: (name, reason) of each member right now."""

    def __init__(self, module: torch.nn.Module):
        names = {id(m): n for n, m in module.named_modules()}
        owners = {}
        for m in module.modules():
            w = m._parameters.get('weight') if hasattr(m, '_parameters') else None
            if w is not None:
                owners.setdefault(id(w), m)
        self._members: List[_Member] = []
        self._names = []
        for m in module.modules():
            # (a group-wise quantizer is no member: it keeps its own one-kernel route)
            if isinstance(m, RescalingIntQuant) and not isinstance(m, GroupwiseRescalingIntQuant):
                tmpl = m._stats_template(m.msb_clamp_bit_width_impl())
                w = tmpl.weight if tmpl is not None else None
                self._members.append(_Member(m, owners.get(id(w)) if w is not None else None))
                self._names.append(names.get(id(m), ''))
        self._lists = {}        # (device, dtype, round mode) -> (weights' keys, quantizers, _WeightList, covered mask)
        self._plans = {}        # id(quantizer) -> (template, weight key, StatsPlan or None)
        self._ids = {id(m.quant) for m in self._members}
        self._results = None    # id(quantizer) -> (y, scale, bit_width, weight, weight version, weight key)
        self._grad_mode = None  # torch.is_grad_enabled() when the results were made
        self._saved = None

    # ---- coverage -------------------------------------------------------------------------------------------------
    def _entry(self, mem: _Member) -> Tuple[Optional[_Entry], str]:
        q = mem.quant
        if getattr(q, 'bvq_collect_only', False) or (mem.layer is not None and
                                                     getattr(mem.layer, 'bvq_disable_weight_quant', False)):
            return None, 'calibrating'
        if mem.layer is not None and mem.layer._buffers.get('frozen_weight_scale') is not None:
            return None, 'frozen weight (graph/gptq.py: freeze_weight_quant)'
        if isinstance(getattr(q.int_quant, 'float_to_int_impl', None), LearnedRoundSte):
            return None, 'learned rounding (graph/learned_round.py: learned_round_mode): the layer quantizes it on its own'
        bw = q.msb_clamp_bit_width_impl()
        tmpl = q._stats_template(bw)
        if tmpl is None:
            return None, 'not a recognised stats-scaled graph (learned scale, another statistic, no host bit width...)'
        if tmpl.runtime is not None:
            return None, 'activation quantizer'
        if tmpl.shared is not None:
            return None, 'quantizer shared by several weights'
        if tmpl.post is not None:
            return None, 'statistic -> scale map is not a plain lower bound'
        if not tmpl.per_channel:
            return None, 'per-tensor scale'
        w = tmpl.weight
        if w is None:
            return None, 'no tracked weight'
        if not w.is_cuda:
            return None, 'weight on the CPU'
        if w.dtype not in _fused._FLOATS:
            return None, 'weight dtype %s' % w.dtype
        key = _weight_key(w)
        cached = self._plans.get(id(q))
        if cached is not None and cached[0] is tmpl and cached[1] == key:
            sp = cached[2]
        else:
            plan = q._stats_plan(w, bw)
            sp = plan[0] if plan is not None and plan[0].outer == 1 and not plan[0].nhwc and w.is_contiguous() else None
            self._plans[id(q)] = (tmpl, key, sp)
        if sp is None:
            return None, 'weight layout not per output channel'
        return _Entry(key, q, w, sp, tmpl, bw), ''

    def _coverage(self):
        """-> ([(name, entry)], [(name, reason)]) right now"""
        cov, unc = [], []
        for name, mem in zip(self._names, self._members):
            e, why = self._entry(mem)
            if e is not None:
                one = _WeightList([e])
                if not nat.weight_list_supported(one.items, 0, 1, e.weight.dtype, one.round_mode):
                    e, why = None, 'channel too large for one workgroup, ragged rows or no one-launch backward'
            (cov if e is not None else unc).append((name, e) if e is not None else (name, why))
        return cov, unc

    @property
    def covered(self) -> List[Tuple[str, str]]:
        return [(name, 'weight %s %s' % (tuple(e.weight.shape), e.weight.dtype)) for name, e in self._coverage()[0]]

    @property
    def uncovered(self) -> List[Tuple[str, str]]:
        return self._coverage()[1]

    # ---- the block ------------------------------------------------------------------------------------------------
    def __enter__(self):
        self._saved = _int._ACTIVE_GROUP
        self._results = None
        _int._ACTIVE_GROUP = self
        return self

    def __exit__(self, *exc):
        _int._ACTIVE_GROUP = self._saved
        self._saved = None
        self._results = None
        self._grad_mode = None
        return False

    def _quantize_all(self):
        groups = {}
        for mem in self._members:
            e, _ = self._entry(mem)
            if e is not None:
                groups.setdefault((e.weight.device, e.weight.dtype, e.tmpl.round_mode), []).append(e)
        results = {}
        for gkey, entries in groups.items():
            keys, quants, tmpls = [e.key for e in entries], [e.quant for e in entries], [e.tmpl for e in entries]
            cached = self._lists.get(gkey)
            # a member's template is a new object whenever what it describes changed (RescalingIntQuant._stats_template)
            if cached is None or cached[0] != keys or cached[1] != quants or \
                    any(a is not b for a, b in zip(cached[2], tmpls)):
                one = _WeightList(entries)
                ok = [nat.weight_list_supported(one.items, i, 1, e.weight.dtype, one.round_mode)
                      for i, e in enumerate(entries)]
                # uncovered weights stay out of the list: their layers quantize them on their own
                kept = [e for e, k in zip(entries, ok) if k]
                cached = self._lists[gkey] = (keys, quants, tmpls, _WeightList(kept) if kept else None, ok)
            wl, ok = cached[3], cached[4]
            if wl is None:
                continue
            entries = [e for e, k in zip(entries, ok) if k]
            out = _fused.WeightListFakeQuantFn.apply(wl, *[e.weight for e in entries])
            n = len(entries)
            for i, e in enumerate(entries):
                results[id(e.quant)] = (out[i], out[n + i], e.bit_width, e.weight, e.weight._version, e.key)
        self._results = results
        self._grad_mode = torch.is_grad_enabled()

    def _member_forward(self, q: RescalingIntQuant, x: torch.Tensor):
        """RescalingIntQuant.forward inside the block: the member's slice of the group's result, or None (the member's
        own forward runs)"""
        if self._results is None:
            if id(q) not in self._ids:
                return None
            self._quantize_all()
        r = self._results.get(id(q))
        if r is None:
            return None
        y, scale, bit_width, w, version, key = r
        # not the tracked weight itself (a detached alias has no path to it), changed in place, calibrating, or another
        # grad mode than the one the results were made under (a no_grad teacher pass inside a training block)
        if x is not w or _weight_key(x) != key or x._version != version or getattr(q, 'bvq_collect_only', False) or \
                torch.is_grad_enabled() != self._grad_mode:
            return None
        return y, scale, q.zero_point_impl(x, scale, bit_width), bit_width
