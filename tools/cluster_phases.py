#!/usr/bin/env python
"""Where a round of the cluster forward goes: per-phase medians from the clock stamps of a developer build.

Needs a library built with -DBVQ_CLUSTER_STAMPS (never the product library):

    python -m brevitas_amd.csrc.build -DBVQ_CLUSTER_STAMPS --out=build/variants/libbvq_stamps.so
    BREVITAS_AMD_LIB=build/variants/libbvq_stamps.so python tools/cluster_phases.py [--shape 256,512,3136] [--dtype bf16]

Wave 0 of every workgroup stamps s_memrealtime (100 MHz) at the start of a round and at five points of it; one line of
JSON per form with the median over all (channel, member) rounds of each phase, in microseconds.
"""
import argparse
import json
import sys

import torch

sys.path.insert(0, '.')

PHASES = ('wait_for_loads', 'fold_and_publish', 'sweep', 'quantize_and_issue_stores', 'hand_back')
TICK_US = 0.01


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', default='256,512,3136')
    ap.add_argument('--dtype', default='bf16')
    ap.add_argument('--launches', type=int, default=5, help='launches before the one whose stamps are read')
    args = ap.parse_args()
    from brevitas_amd import _native as nat
    dt = {'bf16': torch.bfloat16, 'f16': torch.float16, 'f32': torch.float32}[args.dtype]
    dev = torch.device('cuda', 0)
    outer, ch, inner = (int(v) for v in args.shape.split(','))
    torch.manual_seed(1)
    x = torch.randn(outer * ch * inner, device=dev, dtype=dt)
    code = nat.dtype_code(dt)
    d = nat.QuantDesc(outer, ch, inner, code, code, code, nat.F32, 1, 0, -128.0, 127.0, 0, 0, 0, nat.OUT_DEQUANT, 0)
    words = int(nat.lib.bvq_absmax_fakequant_cluster_supported(d, x.data_ptr(), x.data_ptr() + 2 * x.numel() * x.element_size()))
    members = words // ch - 1
    run = torch.ones(ch, device=dev, dtype=dt)
    fb = torch.zeros(1, dtype=torch.int32, device=dev)
    for name, form in (('walk', nat.CLUSTER_WALK), ('oneshot', nat.CLUSTER_ONESHOT)):
        stamps = torch.zeros(ch * members * 6, dtype=torch.int64, device=dev)
        for _ in range(args.launches + 1):
            nat.absmax_fakequant_cluster(d, x, 1e-10, 128.0, dt, run, 0.1, False, 0, fb, form=form, stamps=stamps)
        torch.cuda.synchronize()
        t = stamps.view(ch * members, 6).double()
        phases = (t[:, 1:] - t[:, :-1]) * TICK_US
        med = phases.median(dim=0).values.tolist()
        print(json.dumps({
            'form': name, 'shape': [outer, ch, inner], 'dtype': args.dtype, 'members': members,
            'median_us': {k: round(v, 2) for k, v in zip(PHASES, med)},
            'round_us': round(float(((t[:, 5] - t[:, 0]) * TICK_US).median()), 2),
            'kernel_us': round(float((t[:, 5].max() - t[:, 0].min()) * TICK_US), 1),
            'fallbacks': int(fb.item())}), flush=True)


if __name__ == '__main__':
    main()
