"""Developer tool: the weight quantizers of a model, per layer against WeightQuantGroup (run on the GPU box).

    python tools/weight_group_bench.py [--steps N] [--only resnet50|layer3] [--dtype f32|bf16] [--profile-step]

Two weight sets, each Int8 per-output-channel (Int8WeightPerChannelFloat) weights as QuantConv2d / QuantLinear layers:
  resnet50  the 54 weights of ResNet-50: 53 convolutions and the fc layer (listed below; no torchvision needed) -- the
            [64,3,7,7] stem has ragged rows and stays outside the group
  layer3    config 4's three layer-3 bottleneck weights ([256,1024,1,1], [256,256,3,3], [1024,256,1,1])
For f32 and bf16, per-step time (device-synchronised wall clock over --steps steps after a warm-up) of
  eager     quant_weight() of every layer, one random upstream gradient each, backward
  no_grad   the forward alone under torch.no_grad()
  graph     the eager step captured in a HIP graph, replayed
with and without the group, and whether the results are bit-identical.  --profile-step: 10 eager group steps, then 10
eager per-layer steps of the ResNet-50 set in bf16, nothing else -- for a `rocprofv3 --kernel-trace --stats` run."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # the repository root
import brevitas_amd.quant as Q  # noqa: E402
from brevitas_amd import WeightQuantGroup  # noqa: E402
from brevitas_amd.nn import QuantConv2d, QuantLinear  # noqa: E402


def resnet50_shapes():
    """[Cout, Cin, kh, kw] of ResNet-50's convolutions in order (projection shortcuts included), then the fc layer"""
    shapes = [(64, 3, 7, 7)]
    cin = 64
    for width, blocks in ((64, 3), (128, 4), (256, 6), (512, 3)):
        for b in range(blocks):
            shapes += [(width, cin, 1, 1), (width, width, 3, 3), (width * 4, width, 1, 1)]
            if b == 0:
                shapes.append((width * 4, cin, 1, 1))
            cin = width * 4
    shapes.append((1000, 2048))
    assert len(shapes) == 54, len(shapes)  # 53 convolutions and the fc layer
    return shapes


LAYER3 = [(256, 1024, 1, 1), (256, 256, 3, 3), (1024, 256, 1, 1)]


def build(shapes, dtype, dev):
    layers = torch.nn.ModuleList()
    for s in shapes:
        if len(s) == 2:
            layers.append(QuantLinear(s[1], s[0], bias=False, weight_quant=Q.Int8WeightPerChannelFloat, device=dev,
                                      dtype=dtype))
        else:
            layers.append(QuantConv2d(s[1], s[0], s[2], bias=False, weight_quant=Q.Int8WeightPerChannelFloat,
                                      device=dev, dtype=dtype))
    with torch.no_grad():
        for p in layers.parameters():
            p.mul_(0.05)
    return layers


class _Null:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


def make_step(layers, group, grads):
    ctx = group if group is not None else _Null()

    def step():
        for p in layers.parameters():
            p.grad = None
        with ctx:
            ys = [m.quant_weight()[0] for m in layers]
        torch.autograd.backward(ys, grads)
        # detached: an output kept alive keeps the weights' AccumulateGrad nodes bound to this stream, and a later
        # capture on another stream would then have to wait on it
        return [y.detach() for y in ys], [p.grad for p in layers.parameters()]

    def fwd():
        with torch.no_grad(), ctx:
            return [m.quant_weight()[0] for m in layers]
    return step, fwd


def per_step(fn, steps, warmup=20):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e6


def graphed(step):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):  # (the warm-up's stream: its arrival buffer exists, see _native.arrival_buffer)
        out = step()
    return g, out


def same(a, b):
    return all(torch.equal(u.view(torch.uint8), v.view(torch.uint8)) for u, v in zip(a, b))


def run(name, shapes, dtype, steps):
    dev = 'cuda:0'
    torch.manual_seed(0)
    layers = build(shapes, dtype, dev)
    group = WeightQuantGroup(layers)
    grads = [torch.randn(m.weight.shape, device=dev).to(dtype) for m in layers]
    row = dict(set=name, dtype=str(dtype).split('.')[-1], weights=len(shapes), covered=len(group.covered),
               uncovered=[r for _, r in group.uncovered])
    step_l, fwd_l = make_step(layers, None, grads)
    step_g, fwd_g = make_step(layers, group, grads)
    ys_l, dw_l = step_l()
    ys_l, dw_l = [t.clone() for t in ys_l], [t.clone() for t in dw_l]
    ys_g, dw_g = step_g()
    row['bit_identical'] = same(ys_l, ys_g) and same(dw_l, dw_g)
    for _ in range(2):  # alternate the two routes: the host's speed drifts
        for tag, fn in (('eager_per_layer_us', step_l), ('eager_group_us', step_g),
                        ('no_grad_per_layer_us', fwd_l), ('no_grad_group_us', fwd_g)):
            t = per_step(fn, steps)
            row[tag] = round(min(t, row.get(tag, t)), 1)
    from brevitas_amd import _native as nat
    bwd, calls = nat.weight_quant_list_bwd, []

    def counted(*a, **k):
        out = bwd(*a, **k)
        calls.append(out is not None)
        return out
    nat.weight_quant_list_bwd = counted
    for tag, st in (('graph_per_layer_us', step_l), ('graph_group_us', step_g)):
        calls.clear()
        g, out = graphed(st)
        if tag == 'graph_group_us':  # list backward launches of the warm-up and the capture (False: per-tensor route)
            row['graph_group_list_bwd_calls'] = [sum(calls), len(calls)]
        row[tag] = round(per_step(g.replay, steps), 1)
        g.replay()
        torch.cuda.synchronize()
        if tag == 'graph_group_us':
            row['graph_bit_identical'] = same(out[0], ys_l) and same(out[1], dw_l)
        del g
    nat.weight_quant_list_bwd = bwd
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--only', choices=('resnet50', 'layer3'))
    ap.add_argument('--dtype', choices=('f32', 'bf16'))
    ap.add_argument('--profile-step', action='store_true')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'weight_group_bench.py measures on the GPU'
    if a.profile_step:
        torch.manual_seed(0)
        layers = build(resnet50_shapes(), torch.bfloat16, 'cuda:0')
        grads = [torch.randn(m.weight.shape, device='cuda:0').to(torch.bfloat16) for m in layers]
        for group in (WeightQuantGroup(layers), None):  # group steps, then per-layer steps, each 10 times
            step, _ = make_step(layers, group, grads)
            for _ in range(10):
                step()
            torch.cuda.synchronize()
        return
    sets = {'resnet50': resnet50_shapes(), 'layer3': LAYER3}
    for name, shapes in sets.items():
        if a.only and a.only != name:
            continue
        for dt in (torch.float32, torch.bfloat16):
            if a.dtype and {'f32': torch.float32, 'bf16': torch.bfloat16}[a.dtype] != dt:
                continue
            run(name, shapes, dt, a.steps)


if __name__ == '__main__':
    main()
