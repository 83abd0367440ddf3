#!/usr/bin/env python
"""Fused against materialised steady-state step (forward + backward) of QuantSigmoid and QuantTanh: the activation
folded into the quantizer kernels (csrc/bvq_act.h) against q(torch.sigmoid(x)) / q(torch.tanh(x)) and its autograd.
The quantizers are in their steady state, a learned per-tensor scale (LearnedScaleFakeQuantFn: the route of the default
Uint8ActPerTensorFloat / Int8ActPerTensorFloat after collection).  One process; the two routes alternate, `--runs`
runs each of `--steps` timed steps (HIP events around the whole run), medians reported with the fused / materialised
ratio.  The fused route of a (dtype, activation) pair the library leaves materialised (16-bit tanh) is the
materialised one: its line says so.

    python tools/act_fused_bench.py [--shape 256,512,56,56] [--dtypes bf16,f16,f32] [--runs 3] [--steps 20]
"""
import argparse
import json
import statistics
import sys

import torch

sys.path.insert(0, '.')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', default='256,512,56,56')
    ap.add_argument('--dtypes', default='bf16,f16,f32')
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    args = ap.parse_args()
    import brevitas_amd.quant as bq
    from brevitas_amd.core.quant import _fused
    from brevitas_amd.proxy import FusedActivationQuantProxy
    dev = torch.device('cuda', 0)
    shape = tuple(int(v) for v in args.shape.split(','))
    for dn in args.dtypes.split(','):
        dt = {'bf16': torch.bfloat16, 'f16': torch.float16, 'f32': torch.float32}[dn]
        torch.manual_seed(1)
        x = (torch.randn(shape, device=dev) * 3).to(dt).requires_grad_(True)
        g = torch.randn(shape, device=dev).to(dt)
        for name, f, mod, qf in (('sigmoid', torch.sigmoid, torch.nn.Sigmoid,
                                  lambda: bq.Uint8ActPerTensorFloatMaxInit(1.0)),
                                 ('tanh', torch.tanh, torch.nn.Tanh,
                                  lambda: bq.Int8ActPerTensorFloatMinMaxInit(-1.0, 1.0))):
            fused = FusedActivationQuantProxy(mod(), qf()).to(dev).to(dt)
            ref = qf().to(dev).to(dt)
            routes = {'fused': lambda: fused(x)[0], 'materialised': lambda: ref(f(x))[0]}

            def run(fn, steps):
                for _ in range(steps):
                    x.grad = None
                    fn().backward(g)

            for fn in routes.values():
                run(fn, args.warmup)
            times = {k: [] for k in routes}
            for _ in range(args.runs):
                for k, fn in routes.items():  # alternate the routes
                    torch.cuda.synchronize()
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()
                    run(fn, args.steps)
                    t1.record()
                    torch.cuda.synchronize()
                    times[k].append(t0.elapsed_time(t1) / args.steps)
            med = {k: statistics.median(v) for k, v in times.items()}
            print(json.dumps({'act': name, 'dtype': dn, 'shape': list(shape),
                              'fused_in_kernels': _fused.act_dtype_ok(x, _fused.nat.PRE_SIGMOID if name == 'sigmoid'
                                                                      else _fused.nat.PRE_TANH),
                              'ms_per_step': {k: [round(t, 4) for t in v] for k, v in times.items()},
                              'median_ms': {k: round(v, 4) for k, v in med.items()},
                              'fused_over_materialised': round(med['fused'] / med['materialised'], 4)}), flush=True)
            del fused, ref
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
