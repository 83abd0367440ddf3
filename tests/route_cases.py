"""The case matrix and the signature function of tests/test_gpu_quantizer_routes.py.

A quantizer's route is observable without instrumentation: the chain of autograd node names from y.grad_fn back to the
leaf x names the Function (or C++ node) the forward reached, and a Sigmoid / Tanh / Relu backward node under it says the
pre-op was materialised.  The signature adds whether the scale comes out of the same node as y and, for an activation
quantizer, whether its running statistic saw its first batch.

Only the public factories of brevitas_amd.quant and forward / bvq_forward_pre are used, so the same file records
tests/golden/quantizer_routes.json on the commit before a change of the module layer and checks it after.  One graph has
no factory: a statistic -> scale map under IntScaling that is no plain lower bound (affine rescaling; the fixed-point
factories pair their power-of-two map with PowerOfTwoIntScaling, which the fused routes leave to the generic one).  The
'affine' cases build it from the public core modules, the way tests/test_affine_golden.py does.
"""
import itertools

import torch

import brevitas_amd.config as config
import brevitas_amd.quant as Q
from brevitas_amd import _native as nat

from brevitas_amd.core.bit_width import BitWidthConst
from brevitas_amd.core.function_wrapper import OverOutputChannelView, RoundSte, TensorClamp, TensorClampSte
from brevitas_amd.core.quant import IntQuant, RescalingIntQuant
from brevitas_amd.core.restrict_val import FloatRestrictValue
from brevitas_amd.core.scaling import IntScaling, RuntimeStatsScaling, StatsFromParameterScaling
from brevitas_amd.core.stats import AbsMax
from brevitas_amd.core.zero_point import ZeroZeroPoint

DEV = 'cuda:0'
DTYPES = {'f32': torch.float32, 'bf16': torch.bfloat16}
PRE_OPS = {'none': nat.PRE_NONE, 'relu': nat.PRE_RELU, 'sigmoid': nat.PRE_SIGMOID}



def _affine_weight(w):
    return RescalingIntQuant(
        IntQuant(narrow_range=True, signed=True, float_to_int_impl=RoundSte(), tensor_clamp_impl=TensorClampSte()),
        StatsFromParameterScaling(AbsMax(1), OverOutputChannelView(None), 1, [w], FloatRestrictValue(),
                                  (w.shape[0],) + (1,) * (w.dim() - 1), affine_rescaling=True, scaling_min_val=1e-10),
        IntScaling(signed=True, narrow_range=True), ZeroZeroPoint(), BitWidthConst(8))


def _affine_act(channels):
    return RescalingIntQuant(
        IntQuant(narrow_range=False, signed=True, float_to_int_impl=RoundSte(), tensor_clamp_impl=TensorClamp()),
        RuntimeStatsScaling(AbsMax(1), OverOutputChannelView((1, 0, 2, 3)), FloatRestrictValue(), (1, channels, 1, 1),
                            affine_rescaling=True, scaling_stats_momentum=0.1, scaling_min_val=1e-10),
        IntScaling(signed=True, narrow_range=False), ZeroZeroPoint(), BitWidthConst(8))


WEIGHT_SHAPES = ((4, 3, 3, 3), (4, 32), (1, 32))
WEIGHTS = {
    'per_tensor': lambda w: Q.Int8WeightPerTensorFloat(w),
    'per_channel': lambda w: Q.Int8WeightPerChannelFloat(w),
    'shared2': lambda w: Q.Int8WeightPerChannelFloat([w, torch.nn.Parameter(w.detach().flip(0) * 0.5)]),
    'fixed_point': lambda w: Q.Int8WeightPerChannelFixedPoint(w),
    'affine': _affine_weight,
    'shifted': lambda w: Q.ShiftedUint8WeightPerChannelFloat(w),
    'group16': lambda w: Q.Int8WeightPerGroupFloat(w, group_size=16),
    'shifted_group16': lambda w: Q.ShiftedUint8WeightPerGroupFloat(w, group_size=16),
    'mse': lambda w: Q.Int8WeightPerGroupFloatMSE(w, group_size=16, mse_iters=4),
    'weight_norm_l2': lambda w: Q.Int8WeightNormL2PerChannelFloat(w),
    'a2q': lambda w: Q.Int8AccumulatorAwareWeightQuant(w),
}

# (name, shape, how the leaf lies in memory)
ACT_INPUTS = (('nchw', (2, 3, 4, 4), 'contiguous'), ('nhwc', (2, 3, 4, 4), 'channels_last'),
              ('one_channel', (2, 1, 4, 4), 'contiguous'), ('misaligned', (2, 3, 4, 4), 'misaligned'))
ACTS = {   # name -> (factory(channels), training forwards run before the case)
    'per_channel_stats': (lambda c: Q.Int8ActPerChannelFloat(c, 'stats'), 0),
    'from_stats_collecting': (lambda c: Q.Int8ActPerTensorFloat('parameter_from_stats', 2, scaling_stats_op='max'), 0),
    'from_stats_learned': (lambda c: Q.Int8ActPerTensorFloat('parameter_from_stats', 2, scaling_stats_op='max'), 2),
    'affine_stats': (_affine_act, 0),
    'min_max_init': (lambda c: Q.Int8ActPerTensorFloatMinMaxInit(-1.0, 1.0), 0),
    'fixed_point': (lambda c: Q.Int8ActPerTensorFixedPoint(collect_stats_steps=2), 0),
}

DYNAMIC_SHAPES = ((3, 32), (3, 40), (1, 40))
DYNAMICS = {
    'tensor': lambda: Q.Int8DynamicActPerTensorFloat(),
    'row': lambda: Q.Int8DynamicActPerRowFloat(),
    'group': lambda: Q.Int8DynamicActPerGroupFloat(group_size=8),
    'group32': lambda: Q.Int8DynamicActPerGroupFloat(group_size=32),
    'shifted_tensor': lambda: Q.ShiftedUint8DynamicActPerTensorFloat(),
    'shifted_row': lambda: Q.ShiftedUint8DynamicActPerRowFloat(),
    'shifted_group': lambda: Q.ShiftedUint8DynamicActPerGroupFloat(group_size=8),
    'shifted_group32': lambda: Q.ShiftedUint8DynamicActPerGroupFloat(group_size=32),
}

FLAGS = tuple(itertools.product(('train', 'eval'), (False, True), (True, False)))  # mode, collect_only, FUSED_PATHS


def _values(shape, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * 0.5).to(dtype)


def _leaf(shape, dtype, layout):
    v = _values(shape, dtype).to(DEV)
    if layout == 'channels_last':
        v = v.contiguous(memory_format=torch.channels_last)
    elif layout == 'misaligned':
        base = torch.empty(v.numel() + 1, dtype=dtype, device=DEV)
        base[1:].copy_(v.reshape(-1))
        v = base[1:].view(shape)
        assert v.data_ptr() % 16 != 0
    return v.detach().requires_grad_()


def _chain(fn, leaf):
    """the names of the autograd nodes on the first path (depth first, inputs in order) from `fn` to `leaf`, or None"""
    seen = set()

    def walk(node):
        if node is None or node in seen:
            return None
        seen.add(node)
        if getattr(node, 'variable', None) is leaf:
            return []
        for nxt, _ in node.next_functions:
            tail = walk(nxt)
            if tail is not None:
                return [type(node).__name__] + tail
        return None
    return walk(fn)


def _runtime(q):
    sc = getattr(q, 'scaling_impl', None)
    for name in ('runtime_stats', 'stats'):
        r = getattr(sc, name, None)
        if hasattr(r, 'first_batch'):
            return r
    return None


def signature(q, x, pre_op):
    """run one forward of `q` on the leaf `x` -> the observable route, a JSON-able dict"""
    runtime = _runtime(q)
    before = runtime.first_batch if runtime is not None else None
    if pre_op == nat.PRE_NONE:
        y, scale, zero_point, bit_width = q(x)
    else:
        y, scale, zero_point, bit_width = q.bvq_forward_pre(x, pre_op)
    sig = {'chain': _chain(y.grad_fn, x) if y.grad_fn is not None else None,
           'y_is_x': y is x,
           'scale_node': type(scale.grad_fn).__name__ if scale is not None and scale.grad_fn is not None else None,
           'scale_from_y_node': scale is not None and scale.grad_fn is not None and scale.grad_fn is y.grad_fn}
    if runtime is not None:
        sig['first_batch'] = [bool(before), bool(runtime.first_batch)]
    return sig


def _learned_bit_width(q):
    from brevitas_amd.core.bit_width import BitWidthParameter
    q.msb_clamp_bit_width_impl = BitWidthParameter(8).to(DEV)
    return q


def _prepare(q, mode, collect_only):
    q = q.to(DEV)
    q.train(mode == 'train')
    if collect_only:
        q.bvq_collect_only = True
    return q


def cases():
    """-> [(case id, thunk)]: thunk() builds the quantizer and its leaf and returns (q, x, pre_op); a thunk whose factory
    or forward rejects the combination raises, and the combination is dropped (recorded as {'rejected': error type})"""
    out = []
    for (fname, factory), shape, (dn, dtype), (pn, pre_op), (mode, collect, fused) in itertools.product(
            WEIGHTS.items(), WEIGHT_SHAPES, DTYPES.items(), PRE_OPS.items(), FLAGS):
        def weight_case(factory=factory, shape=shape, dtype=dtype, pre_op=pre_op, mode=mode, collect=collect, lbw=False):
            w = torch.nn.Parameter(_values(shape, dtype).to(DEV))
            q = factory(w)
            if pre_op != nat.PRE_NONE and not hasattr(q, 'bvq_forward_pre'):
                raise TypeError('no pre-op')
            return _prepare(_learned_bit_width(q) if lbw else q, mode, collect), w, pre_op
        cid = 'weight/%s/%s/%s/%s/%s/collect%d/fused%d' % (fname, 'x'.join(map(str, shape)), dn, pn, mode, collect, fused)
        out.append((cid, fused, weight_case))
        if (shape, dn, pn, mode, collect, fused) == ((4, 32), 'f32', 'none', 'train', False, True):
            out.append((cid + '/learned_bit_width', fused, lambda c=weight_case: c(lbw=True)))
    for (fname, (factory, warm)), (iname, shape, layout), (dn, dtype), (pn, pre_op), (mode, collect, fused) in \
            itertools.product(ACTS.items(), ACT_INPUTS, DTYPES.items(), PRE_OPS.items(), FLAGS):
        def act_case(factory=factory, warm=warm, shape=shape, layout=layout, dtype=dtype, pre_op=pre_op, mode=mode,
                     collect=collect, lbw=False):
            q = factory(shape[1]).to(DEV)
            if lbw:
                _learned_bit_width(q)
            q.train()
            for _ in range(warm):
                q(_values(shape, dtype, seed=1).to(DEV))
            return _prepare(q, mode, collect), _leaf(shape, dtype, layout), pre_op
        cid = 'act/%s/%s/%s/%s/%s/collect%d/fused%d' % (fname, iname, dn, pn, mode, collect, fused)
        out.append((cid, fused, act_case))
        if (iname, dn, pn, mode, collect, fused) == ('nchw', 'f32', 'none', 'train', False, True):
            out.append((cid + '/learned_bit_width', fused, lambda c=act_case: c(lbw=True)))
    for (fname, factory), shape, (dn, dtype), (mode, collect, fused) in itertools.product(
            DYNAMICS.items(), DYNAMIC_SHAPES, DTYPES.items(), FLAGS):
        def dynamic_case(factory=factory, shape=shape, dtype=dtype, mode=mode, collect=collect, lbw=False):
            q = factory()
            return _prepare(_learned_bit_width(q) if lbw else q, mode, collect), _leaf(shape, dtype, 'contiguous'), \
                nat.PRE_NONE
        cid = 'dynamic/%s/%s/%s/%s/collect%d/fused%d' % (fname, 'x'.join(map(str, shape)), dn, mode, collect, fused)
        out.append((cid, fused, dynamic_case))
        if (fname, shape, dn, mode, collect, fused) == ('row', (3, 40), 'f32', 'train', False, True):
            out.append((cid + '/learned_bit_width', fused, lambda c=dynamic_case: c(lbw=True)))
    return out


def run(observe=None):
    """every case -> {case id: signature or {'rejected': ...}}; observe(case id, q) may wrap q before its forward"""
    table = {}
    saved = config.FUSED_PATHS
    try:
        for cid, fused, thunk in cases():
            config.FUSED_PATHS = fused
            try:
                q, x, pre_op = thunk()
                if observe is not None:
                    observe(cid, q)
                table[cid] = signature(q, x, pre_op)
            except (TypeError, ValueError, NotImplementedError, nat.BvqError) as e:
                table[cid] = {'rejected': type(e).__name__}
    finally:
        config.FUSED_PATHS = saved
    return table
