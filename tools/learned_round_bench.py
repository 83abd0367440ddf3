"""One learned-rounding step on the device: the fused route (one bvq_learned_round_fwd and one bvq_learned_round_bwd launch
behind the quantizer's own scale computation) against the composed route, and the two kernels alone.

    python tools/learned_round_bench.py [--shapes 4096x4096,11008x4096] [--dtypes bf16,f32] [--reps 7] [--group 128]

Per shape, dtype and layout (per-channel, groups of --group): a QuantLinear weight in learned_round_mode, frozen weights;
one step is quant_weight() forward plus backward to `value`.  The two routes alternate in one process
(config.FUSED_PATHS on / off: the composed route is what a user would otherwise run on the same device), each warmed up,
timed with HIP events on the current stream, median of --reps (at least 5):
  fused_ms / composed_ms    the step, everything included (scale computation, autograd)
  fused_launches / composed_launches   device kernels per step (torch.profiler)
  fwd_ms / bwd_ms / bwd_dx_ms          the kernels alone through their brevitas_amd._native wrappers
  *_tbs, *_share                        algorithmic bytes per second (forward: x, value, y; backward: g, x, value, dvalue,
                                        plus dx) in TB/s and as a share of 8 TB/s
One JSON line per case.  profiles/learned_round.md holds the measured values."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

PEAK_TBS = 8.0
DT = {'bf16': torch.bfloat16, 'f32': torch.float32, 'f16': torch.float16}


def timed(fn, reps, warmup=3):
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


def count_launches(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if str(e.device_type).endswith('CUDA'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='4096x4096,11008x4096')
    ap.add_argument('--dtypes', default='bf16,f32')
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--group', type=int, default=128)
    ap.add_argument('--no-launch-count', action='store_true')
    args = ap.parse_args()
    reps = max(args.reps, 5)

    import brevitas_amd.config as config
    from brevitas_amd import _native as nat
    from brevitas_amd import quant as Q
    from brevitas_amd.core.quant import _fused
    from brevitas_amd.graph import learned_round_mode
    from brevitas_amd.nn import QuantLinear

    dev = torch.device('cuda', 0)
    for shape in args.shapes.split(','):
        rows, k = (int(v) for v in shape.split('x'))
        for dn in args.dtypes.split(','):
            for layout in ('per_channel', 'g%d' % args.group):
                torch.manual_seed(0)
                make = Q.Int4WeightPerChannelFloat if layout == 'per_channel' else \
                    (lambda w: Q.Int4WeightPerGroupFloat(w, args.group))
                layer = QuantLinear(k, rows, bias=False, weight_quant=make, device=dev, dtype=DT[dn])
                g = torch.randn_like(layer.weight)
                res = dict(shape=[rows, k], dtype=dn, layout=layout)
                with learned_round_mode(layer) as lr:
                    value = lr.parameters()[0]

                    def step():
                        value.grad = None
                        layer.quant_weight()[0].backward(g)

                    times = {True: [], False: []}
                    for on in (True, False):          # warm both routes up, then alternate
                        config.FUSED_PATHS = on
                        for _ in range(3):
                            step()
                    for _ in range(reps):
                        for on in (True, False):
                            config.FUSED_PATHS = on
                            times[on].append(timed(step, 1, warmup=0))
                    res['fused_ms'] = statistics.median(times[True])
                    res['composed_ms'] = statistics.median(times[False])
                    if not args.no_launch_count:
                        for on, key in ((True, 'fused_launches'), (False, 'composed_launches')):
                            config.FUSED_PATHS = on
                            res[key] = count_launches(step)
                    config.FUSED_PATHS = True

                    # the kernels alone, on the operands IntQuant hands them
                    q = layer.weight_quant
                    with torch.no_grad():
                        _, scale, zp, _ = q(layer.weight)
                    x = layer.weight.detach()
                    if layout != 'per_channel':
                        x, scale = x.reshape(-1, args.group), scale.reshape(-1, 1)
                    p = _fused.plan(x, scale, zp)
                    sc, zc = scale.reshape(-1).contiguous(), zp.reshape(-1).contiguous()
                    desc = _fused.make_desc(p, x, sc, zc, -8.0, 7.0, nat.FLOOR, True, nat.OUT_DEQUANT)
                    assert nat.learned_round_supported(desc, x, value), nat.last_error()
                    impl = q.int_quant.float_to_int_impl.learned_round_impl
                    kind, consts = impl.bvq_learned_round_kind, impl.bvq_constants()
                    v = value.detach()
                    nbytes = x.numel() * x.element_size()
                    for key, streams, fn in (
                            ('fwd', 3, lambda: nat.learned_round_fwd(desc, x, v, sc, zc, kind, consts, False)),
                            ('bwd', 4, lambda: nat.learned_round_bwd(desc, g, x, v, sc, zc, kind, consts, False)),
                            ('bwd_dx', 5, lambda: nat.learned_round_bwd(desc, g, x, v, sc, zc, kind, consts, True))):
                        ms = timed(fn, reps)
                        res[key + '_ms'] = ms
                        res[key + '_tbs'] = streams * nbytes / (ms * 1e-3) / 1e12
                        res[key + '_share'] = res[key + '_tbs'] / PEAK_TBS
                print(json.dumps(res), flush=True)
                del layer, g


if __name__ == '__main__':
    main()
