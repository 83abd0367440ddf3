"""GPFQ weight quantization on the device: the fused route (one bvq_gpfq_block launch per block of 128 columns) against
the composed torch route, and the column-loop kernel alone.

    python tools/gpfq_bench.py [--shapes 4096x4096,11008x4096] [--reps 5] [--composed-reps 5] [--group 128]

Per shape (bf16 weight, 4-bit, group-wise): medians over --reps runs (the composed route: --composed-reps) after one
warm-up run each, HIP events on the current stream,
  first_ms     the product Wf @ triu(D) both routes share
  fused_ms     gpfq_quantize_weight, fused route, everything included
  composed_ms  gpfq_quantize_weight with config.FUSED_PATHS off: what a user would otherwise run on the same device
  kernel_ms    the K / 128 launches of the column-loop kernel alone, back to back (no tail updates between them)
The two routes' codes are compared bit for bit before anything is timed.  One JSON line per shape.  profiles/gpfq.md
holds the measured values."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from gptq_bench import timed  # noqa: E402


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
    from brevitas_amd.graph import gpfq as P
    from brevitas_amd.graph import gptq as G

    dev = torch.device('cuda', 0)
    for shape in args.shapes.split(','):
        rows, k = (int(v) for v in shape.split('x'))
        torch.manual_seed(0)
        w = torch.nn.Parameter((0.05 * torch.randn(rows, k, device=dev)).to(torch.bfloat16))
        x = torch.randn(2 * k, k, device=dev)
        x = x + 0.5 * x.roll(1, dims=1)
        xq = x + 0.05 * torch.randn(2 * k, k, device=dev)
        h = (2.0 / x.shape[0]) * (xq.t() @ xq)
        d = (2.0 / x.shape[0]) * ((x - xq).t() @ xq)
        del x, xq
        make = Q.ShiftedUint4WeightPerGroupFloat if args.asym else Q.Int4WeightPerGroupFloat
        quant = make(w, args.group).to(dev)
        plan = P._plan(quant, k)

        fused = P.gpfq_quantize_weight(w, h, d, quant)
        same = None
        if args.composed_reps > 0:
            config.FUSED_PATHS = False
            try:
                same = bool(torch.equal(P.gpfq_quantize_weight(w, h, d, quant).q, fused.q))
            finally:
                config.FUSED_PATHS = True

        wf = w.detach().float()
        first_ms = timed(lambda: P.initial_correction(wf, d), args.reps)
        fused_ms = timed(lambda: P.gpfq_quantize_weight(w, h, d, quant), args.reps)

        # the kernel alone: every block's launch on the same correction, nothing between them
        c = P.initial_correction(wf, d)
        q = torch.empty_like(w)
        scale, zp, _, _ = G._given_params(plan, w)
        desc = P.fused_block_desc(plan, rows, k, w.dtype)
        assert desc is not None, 'the fused route does not cover this quantizer'

        def blocks():
            for c0 in range(0, k, P.BLOCK):
                P.fused_block(desc, wf, c, h, c0, min(c0 + P.BLOCK, k), q, scale, zp)
        kernel_ms = timed(blocks, args.reps)

        composed_ms = None
        if args.composed_reps > 0:
            config.FUSED_PATHS = False
            try:
                composed_ms = timed(lambda: P.gpfq_quantize_weight(w, h, d, quant), args.composed_reps)
            finally:
                config.FUSED_PATHS = True
        print(json.dumps(dict(shape=[rows, k], dtype='bf16', bits=4, group=args.group, asym=args.asym,
                              routes_bit_identical=same, first_ms=round(first_ms, 3), fused_ms=round(fused_ms, 3),
                              composed_ms=None if composed_ms is None else round(composed_ms, 1),
                              kernel_ms=round(kernel_ms, 3), launches=(k + P.BLOCK - 1) // P.BLOCK)), flush=True)


if __name__ == '__main__':
    main()
