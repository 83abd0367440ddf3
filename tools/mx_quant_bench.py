"""Developer tool: the MX block-scaled quantizer kernels next to the composed route, the integer group kernels and the
chip's ceiling.

    python tools/yardstick.py build      # here (no GPU): build/tools/libyardstick.so
    python tools/mx_quant_bench.py       # on the GPU box

An [8192, 8192] tensor in bf16 and f16, groups of 32, formats e4m3 and e2m1, forward and backward of
  (a) the MX kernels (bvq_mx_quant_fwd / bvq_mx_quant_bwd: one launch each);
  (b) the composed route on the device (core/quant/mx.py, MXComposedFn: plain torch ops);
  (c) the integer group kernels at g = 32 (bvq_group_quant_fwd / bvq_group_quant_bwd): the same bytes +- the scale words;
  (d) tools/yardstick.hip: the same bytes with no arithmetic, read + write and two reads + write, best of a small sweep.
Interleaved rounds in one process, one warm call in front of every timed call (the queue is never empty when the timed
launch starts), HIP events on the launching stream, median / min / max over the rounds."""
import statistics
import sys

import rounds
from rounds import ROOT, ev

ROUNDS = 9
COMPOSED_ROUNDS = 3   # (b) is tens of times slower: fewer rounds, same protocol


def main():
    import torch
    sys.path.insert(0, ROOT)
    from brevitas_amd import _native as nat
    from brevitas_amd.core.quant.mx import MX_FORMATS, MXComposedFn
    dev = 'cuda:0'
    out_f, k, gs = 8192, 8192, 32

    print('# tools/mx_quant_bench.py: [%d, %d], groups of %d, one MI355X; median / min / max ms over %d interleaved '
          'rounds (%d for the composed route)' % (out_f, k, gs, ROUNDS, COMPOSED_ROUNDS))
    for dn, dt in (('bf16', torch.bfloat16), ('f16', torch.float16)):
        torch.manual_seed(0)
        x = (torch.randn(out_f, k, device=dev) * 0.02).to(dt).reshape(-1)
        g = torch.randn(out_f, k, device=dev).to(dt).reshape(-1)
        o = torch.empty_like(x)
        nbytes = x.numel() * x.element_size()
        code = nat.dtype_code(dt)

        cands = {}
        for fmt in ('e4m3', 'e2m1'):
            f = MX_FORMATS[fmt]
            assert nat.mx_quant_supported(x, gs, f.code)
            cands['(a) MX kernels %s fwd' % fmt] = lambda f=f: nat.mx_quant_fwd(x, gs, f.code, nat.MX_FLOOR)
            cands['(a) MX kernels %s bwd' % fmt] = lambda f=f: nat.mx_quant_bwd(g, x, None, gs, f.code, nat.MX_FLOOR, 1)

            def composed_fwd(f=f):
                return MXComposedFn.apply(x, gs, f, False, True)

            def composed_bwd(f=f):
                leaf = x.detach().requires_grad_(True)
                y, _ = MXComposedFn.apply(leaf, gs, f, False, True)
                a = ev()
                y.backward(g)
                return a
            cands['(b) composed route %s fwd' % fmt] = composed_fwd
            cands['(b) composed route %s bwd' % fmt] = composed_bwd
        d = nat.QuantDesc(1, x.numel() // gs, gs, code, code, code, nat.F32, 1, 0, -7.0, 7.0, nat.ROUND, 0, 1,
                          nat.OUT_DEQUANT, nat.PRE_NONE)
        assert nat.group_quant_supported(d, x)
        _, scale_g, stat_g = nat.group_quant_fwd(d, x, 1e-10, 7.0)
        cands['(c) int4 group kernels g=32 fwd'] = lambda: nat.group_quant_fwd(d, x, 1e-10, 7.0)
        cands['(c) int4 group kernels g=32 bwd'] = lambda: nat.group_quant_bwd(d, g, x, scale_g, stat_g, None, 1e-10, 7.0)
        cands.update(rounds.yardstick_cands(rounds.yardstick(x, g, o)))

        for name, fn in cands.items():   # warm-up
            if not name.startswith('(b)'):
                fn()
        torch.cuda.synchronize()
        res = {name: [] for name in cands}
        for rnd in range(ROUNDS):
            pairs = []
            for name, fn in cands.items():
                if name.startswith('(b)'):
                    if rnd >= COMPOSED_ROUNDS:
                        continue
                    out = fn()                       # warm
                    torch.cuda.synchronize()         # (its temporaries are many times the tensor)
                    del out
                    a = ev()
                    out = fn()
                    if name.endswith('bwd'):
                        a = out                      # the event recorded between its forward and its backward
                    pairs.append((name, a, ev()))
                    del out
                    torch.cuda.synchronize()
                    continue
                fn()
                a = ev()
                out = fn()
                pairs.append((name, a, ev()))
                del out
            torch.cuda.synchronize()
            for name, a, b_ in pairs:
                res[name].append(a.elapsed_time(b_))
            torch.cuda.empty_cache()
        print('== %s (%d MiB per tensor)' % (dn, nbytes >> 20))
        med = {name: statistics.median(ts) for name, ts in res.items()}
        best = {}
        for name, ts in res.items():
            passes = 3 if ('bwd' in name or 'triad' in name) else 2
            print('%-46s %8.4f / %8.4f / %8.4f ms  %5.2f TB/s' % (name, med[name], min(ts), max(ts),
                                                                  passes * nbytes / med[name] / 1e9))
            if name.startswith('(d)'):
                kind = name.split(' ')[1]
                if kind not in best or med[name] < best[kind]:
                    best[kind] = med[name]
        for way, kind in (('fwd', 'copy'), ('bwd', 'triad')):
            c = res['(c) int4 group kernels g=32 %s' % way]
            for fmt in ('e4m3', 'e2m1'):
                a = med['(a) MX kernels %s %s' % (fmt, way)]
                b_ = med['(b) composed route %s %s' % (fmt, way)]
                print('%s %s: (a) %.4f ms | (b)/(a) %.1f | (a)/(c) %.3f, (c) max/min %.3f | (a)/(d) %.3f (ceiling %s %.4f ms)'
                      % (fmt, way, a, b_ / a, a / statistics.median(c), max(c) / min(c), a / best[kind], kind, best[kind]))
        del x, g, o, cands
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
