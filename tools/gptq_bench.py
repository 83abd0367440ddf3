"""GPTQ weight quantization on the device: the fused route (one bvq_gptq_block launch per block of 128 columns) against
the composed torch route, and the column-loop kernel alone.

    python tools/gptq_bench.py [--shapes 4096x4096,11008x4096] [--reps 5] [--composed-reps 5] [--group 128]

Per shape (bf16 weight, 4-bit, group-wise): medians over --reps runs (the composed route: --composed-reps) after one
warm-up run each, HIP events on the current stream,
  prep_ms      the Hessian preparation both routes share (damping, the three factorisation calls)
  fused_ms     gptq_quantize_weight, fused route, everything included
  composed_ms  gptq_quantize_weight with config.FUSED_PATHS off: what a user would otherwise run on the same device
  kernel_ms    the K / 128 launches of the column-loop kernel alone, back to back (no tail updates between them)
One JSON line per shape.  profiles/gptq.md holds the measured values."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def timed(fn, reps, warmup=1):
    """median milliseconds of fn() between two HIP events"""
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='4096x4096,11008x4096')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--composed-reps', type=int, default=5)
    ap.add_argument('--group', type=int, default=128)
    ap.add_argument('--asym', action='store_true')
    args = ap.parse_args()

    import brevitas_amd.config as config
    from brevitas_amd import quant as Q
    from brevitas_amd.graph import gptq as G

    dev = torch.device('cuda', 0)
    for shape in args.shapes.split(','):
        rows, k = (int(v) for v in shape.split('x'))
        torch.manual_seed(0)
        w = torch.nn.Parameter((0.05 * torch.randn(rows, k, device=dev)).to(torch.bfloat16))
        x = torch.randn(2 * k, k, device=dev)
        x = x + 0.5 * x.roll(1, dims=1)
        h = (2.0 / x.shape[0]) * (x.t() @ x)
        del x
        make = Q.ShiftedUint4WeightPerGroupFloat if args.asym else Q.Int4WeightPerGroupFloat
        quant = make(w, args.group).to(dev)
        plan = G._plan(quant, k, False)

        prep_ms = timed(lambda: G.prepare_hessian(h, torch.zeros(1, k, device=dev), 0.01), args.reps)
        fused_ms = timed(lambda: G.gptq_quantize_weight(w, h, quant), args.reps)

        # the kernel alone: every block's launch on the same working copy, nothing between them
        wf = w.detach().float()
        u = G.prepare_hessian(h, wf, 0.01)
        q = torch.empty_like(w)
        scale = torch.empty(rows, k // args.group, dtype=w.dtype, device=dev)
        zp = torch.empty_like(scale) if plan.shifted else None
        fa = G.fused_block_args(plan, rows, k, w.dtype)
        assert fa is not None, 'the fused route does not cover this quantizer'

        def blocks():
            for c0 in range(0, k, G.BLOCK):
                G.fused_block(fa, plan, wf, u, c0, min(c0 + G.BLOCK, k), q, scale, zp)
        kernel_ms = timed(blocks, args.reps)

        composed_ms = None
        if args.composed_reps > 0:
            config.FUSED_PATHS = False
            try:
                composed_ms = timed(lambda: G.gptq_quantize_weight(w, h, quant), args.composed_reps)
            finally:
                config.FUSED_PATHS = True
        print(json.dumps(dict(shape=[rows, k], dtype='bf16', bits=4, group=args.group, asym=args.asym,
                              prep_ms=round(prep_ms, 3), fused_ms=round(fused_ms, 3),
                              composed_ms=None if composed_ms is None else round(composed_ms, 1),
                              kernel_ms=round(kernel_ms, 3), launches=(k + G.BLOCK - 1) // G.BLOCK,
                              device_linalg=G._device_linalg_ok(dev))), flush=True)


if __name__ == '__main__':
    main()
