#!/usr/bin/env python
"""Interleaved A/B rounds, one process: the cluster forward (bvq_absmax_fakequant_cluster: statistic, scale, running
statistic and quantizer in one launch, x read once) against statistic + quantizer (bvq_absmax_scale_onepass +
bvq_fakequant_fwd), on the headline tensor and a few other shapes.  HIP events around each call, medians over rounds;
reports the fallbacks the cluster kernel took (0 expected).  'cluster' is the form the library chooses for the shape
(cluster_plan); --forms adds every named form of bvq_absmax_fakequant_cluster_form to the same rounds, which is how
the plan's rule is decided.

    python tools/cluster_ab.py [--shapes 256,512,3136;32,512,3136] [--rounds 10] [--iters 20] [--dtype bf16]
                               [--forms walk,oneshot]
"""
import argparse
import json
import statistics
import sys

import torch

sys.path.insert(0, '.')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='256,512,3136;32,512,3136;256,64,3136;40,24,3136')
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--dtype', default='bf16')
    ap.add_argument('--label', default='', help='free text carried into the JSON line (e.g. the -D flags of the build)')
    ap.add_argument('--forms', default='', help='comma list of walk, oneshot: timed next to the plan\'s choice')
    args = ap.parse_args()
    from brevitas_amd import _native as nat
    form_codes = {'walk': nat.CLUSTER_WALK, 'oneshot': nat.CLUSTER_ONESHOT}
    forms = [f for f in args.forms.split(',') if f]
    dt = {'bf16': torch.bfloat16, 'f16': torch.float16, 'f32': torch.float32}[args.dtype]
    dev = torch.device('cuda', 0)
    esize = torch.tensor([], dtype=dt).element_size()
    for spec in args.shapes.split(';'):
        outer, ch, inner = (int(v) for v in spec.split(','))
        torch.manual_seed(1)
        x = torch.randn(outer * ch * inner, device=dev, dtype=dt)
        code = nat.dtype_code(dt)
        d = nat.QuantDesc(outer, ch, inner, code, code, code, nat.F32, 1, 0, -128.0, 127.0, 0, 0, 0, nat.OUT_DEQUANT, 0)
        zp = torch.zeros(1, device=dev)
        run_a = torch.ones(ch, device=dev, dtype=dt)
        run_b = run_a.clone()
        fb = torch.zeros(1, dtype=torch.int32, device=dev)

        def cluster(form=0):
            return nat.absmax_fakequant_cluster(d, x, 1e-10, 128.0, dt, run_a, 0.1, False, 0, fb, form=form)

        def two():
            _, scale = nat.absmax_scale(x, outer, ch, inner, 1e-10, 128.0, dt, 0, running=run_b, momentum=0.1,
                                        first_batch=False)
            nat.fakequant_fwd(d, x, scale, zp)

        if cluster() is None:
            print(json.dumps({'shape': [outer, ch, inner], 'covered': False}))
            continue

        def timed(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            fn()
            a.record()
            for _ in range(args.iters):
                fn()
            b.record()
            torch.cuda.synchronize()
            return a.elapsed_time(b) / args.iters

        runs = {'cluster': cluster, 'statistic+quantizer': two}
        for f in forms:
            runs[f] = (lambda code: lambda: cluster(code))(form_codes[f])
        for _ in range(3):  # settle
            for fn in runs.values():
                fn()
        res = {k: [] for k in runs}
        for _ in range(args.rounds):
            for k, fn in runs.items():
                res[k].append(timed(fn))
        torch.cuda.synchronize()
        med = {k: statistics.median(v) for k, v in res.items()}
        nbytes = 2 * outer * ch * inner * esize  # read x, write y
        words = int(nat.lib.bvq_absmax_fakequant_cluster_supported(d, x.data_ptr(), x.data_ptr() + nbytes + 4096))
        print(json.dumps({
            'shape': [outer, ch, inner], 'dtype': args.dtype, 'label': args.label,
            'workgroups_per_channel': words // ch - 1,
            'ms': {k: round(v, 4) for k, v in med.items()},
            'spread_ms': {k: [round(min(v), 4), round(max(v), 4)] for k, v in res.items()},
            'cluster_GBps': round(nbytes / med['cluster'] / 1e6, 1),
            'speedup': round(med['statistic+quantizer'] / med['cluster'], 3),
            'fallbacks': int(fb.item())}), flush=True)


if __name__ == '__main__':
    main()
