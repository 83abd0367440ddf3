"""Developer tool: a forward + backward step of the accumulator-aware weight quantizer next to the per-channel weight
quantizer and the chip's ceiling.

    python tools/yardstick.py build        # here (no GPU): build/tools/libyardstick.so
    python tools/weight_norm_bench.py      # on the GPU box

Weights [512, 512, 3, 3] and [4096, 4096] in bf16 and f32, 8 bits:
  (a)  Int8AccumulatorAwareWeightQuant through the module: the step a layer pays -- the restriction of s and g (four
       scale-shaped launches each way), one kernel each way (csrc/bvq_weight_norm.hip), autograd;
  (a') its two kernels alone, through their wrappers (bvq_weight_norm_fwd / bvq_weight_norm_bwd);
  (b)  Int8WeightPerChannelFloat through the module, the same tensors: code this quantizer does not touch;
  (c)  tools/yardstick.hip: the same bytes with no arithmetic -- read + write (2 x 16 bytes per chunk, the forward) and
       two reads + write (3 x 16, the backward), best of a small sweep.
Steps: host clock around STEPS steps that end in a device synchronise, 50 warm-up steps in front, (a) and (b)
alternating, median / min over the rounds.  Kernels: HIP events, one warm call in front of every timed call."""
import statistics
import sys
import time

import rounds
from rounds import ROOT

ROUNDS, STEPS, WARMUP = 7, 100, 50
SHAPES = ((512, 512, 3, 3), (4096, 4096))


def main():
    import torch
    sys.path.insert(0, ROOT)
    from brevitas_amd import _native as nat
    import brevitas_amd.quant as Q
    from brevitas_amd.core.quant import _fused
    dev = 'cuda:0'

    print('# tools/weight_norm_bench.py: 8-bit weights, one MI355X; median / min over %d rounds; steps: ms per step over '
          '%d steps behind %d warm-up steps' % (ROUNDS, STEPS, WARMUP))
    for shape in SHAPES:
        for dn, dt in (('bf16', torch.bfloat16), ('f32', torch.float32)):
            torch.manual_seed(0)
            w0 = (torch.randn(shape, device=dev) * 0.03).to(dt)
            g = torch.randn(shape, device=dev).to(dt)
            o = torch.empty_like(w0)
            nbytes = w0.numel() * w0.element_size()

            def stepper(make):
                w = torch.nn.Parameter(w0.clone())
                q = make(w).to(dev)
                params = [w] + list(q.parameters())

                def step():
                    for p in params:
                        p.grad = None
                    q(w)[0].backward(g)
                return step

            steps = {'(a) A2Q module step': stepper(Q.Int8AccumulatorAwareWeightQuant),
                     '(b) per-channel module step': stepper(Q.Int8WeightPerChannelFloat)}
            for fn in steps.values():
                for _ in range(WARMUP):
                    fn()
            torch.cuda.synchronize()
            res = {name: [] for name in steps}
            for _ in range(ROUNDS):
                for name, fn in steps.items():
                    t0 = time.perf_counter()
                    for _ in range(STEPS):
                        fn()
                    torch.cuda.synchronize()
                    res[name].append((time.perf_counter() - t0) * 1e3 / STEPS)

            rows = shape[0]
            desc = _fused.weight_norm_call(w0, 127.0, nat.ROUND_TO_ZERO, True)
            T, nmin = 2.0 ** 23 / 256, 1e-10
            assert nat.weight_norm_supported(desc, nat.NORM_L1, T, nmin, w0)
            v = w0.reshape(rows, -1).float()
            s = (v.abs().max(1).values / 127).contiguous()
            gp = v.abs().sum(1).contiguous()
            n = nat.weight_norm_fwd(desc, nat.NORM_L1, T, nmin, w0, s, gp)[1]
            kern = {"(a') A2Q kernel fwd": lambda: nat.weight_norm_fwd(desc, nat.NORM_L1, T, nmin, w0, s, gp),
                    "(a') A2Q kernel bwd": lambda: nat.weight_norm_bwd(desc, nat.NORM_L1, T, nmin, g, w0, s, gp, n)}
            kern.update(rounds.yardstick_cands(rounds.yardstick(w0, g, o), '(c)', persistent=False))
            kres = rounds.timed_rounds(kern, ROUNDS, warmup=WARMUP)
            print('== %s %s (%.1f MiB)' % ('x'.join(map(str, shape)), dn, nbytes / 2 ** 20))
            for name, ts in res.items():
                print('%-34s %8.4f / %8.4f ms per step' % (name, statistics.median(ts), min(ts)))
            kmed, best = rounds.report(kres, nbytes, 34, '(c)')
            a = statistics.median(res['(a) A2Q module step'])
            b = statistics.median(res['(b) per-channel module step'])
            kf, kb = (kmed["(a') A2Q kernel %s" % way] for way in ('fwd', 'bwd'))
            print('%s %s: step (a) %.4f ms (b) %.4f ms (a)/(b) %.2f | kernels fwd %.4f ms = %.2f x copy %.4f, bwd %.4f ms '
                  '= %.2f x triad %.4f | kernels / step %.2f'
                  % ('x'.join(map(str, shape)), dn, a, b, a / b, kf, kf / best['copy'], best['copy'], kb,
                     kb / best['triad'], best['triad'], (kf + kb) / a))
            del w0, g, o, steps, kern
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
