"""Developer tool: the asymmetric group-wise weight quantizer kernels next to the route they replace, the symmetric group
kernels and the chip's ceiling.

    python tools/yardstick.py build        # here (no GPU): build/tools/libyardstick.so
    python tools/group_shifted_bench.py    # on the GPU box

An [8192, 8192] weight in bf16 and f16, 4 bits, group sizes 128 and 32, forward and backward of
  (a)  the asymmetric group kernels (bvq_group_shifted_fwd / bvq_group_shifted_bwd: one launch each);
  (a') the same through the module, ShiftedUint4WeightPerGroupFloat: what a layer pays, autograd included;
  (b)  the route without them: ShiftedUint8WeightPerChannelFloat on w.view(-1, g), through the module -- two statistic
       passes, scale-shaped torch ops for scale and zero-point, the per-channel quantizer kernels, two deposit passes;
  (c)  the symmetric group kernels (bvq_group_quant_fwd / bvq_group_quant_bwd);
  (d)  tools/yardstick.hip: the same bytes with no arithmetic, read + write and two reads + write, best of a small sweep.
Interleaved rounds in one process, one warm call in front of every timed call (the queue is never empty when the timed
launch starts), HIP events on the launching stream, median / min over the rounds."""
import sys

import rounds
from rounds import ROOT

ROUNDS = 7


def main():
    import torch
    sys.path.insert(0, ROOT)
    from brevitas_amd import _native as nat
    import brevitas_amd.quant as Q
    from brevitas_amd.core.quant import _fused
    dev = 'cuda:0'
    out_f, k = 8192, 8192
    bits, min_val = 4, 1e-10

    print('# tools/group_shifted_bench.py: [%d, %d] weight, %d bits, one MI355X; median / min ms over %d interleaved '
          'rounds' % (out_f, k, bits, ROUNDS))
    for dn, dt in (('bf16', torch.bfloat16), ('f16', torch.float16)):
        torch.manual_seed(0)
        x = (torch.randn(out_f, k, device=dev) * 0.02).to(dt).reshape(-1)
        g = torch.randn(out_f, k, device=dev).to(dt).reshape(-1)
        o = torch.empty_like(x)
        nbytes = x.numel() * x.element_size()

        cands = {}
        for gs in (128, 32):
            ds, thr_s = _fused.group_shifted_call(x, gs, 2.0 ** bits - 1, 0.0, 2.0 ** bits - 1, True)
            assert nat.group_shifted_supported(ds, x)
            stat_s = nat.group_shifted_fwd(ds, x, min_val, thr_s)[3]
            cands['(a) shifted group kernels g=%d fwd' % gs] = \
                lambda d=ds, t=thr_s: nat.group_shifted_fwd(d, x, min_val, t)
            cands['(a) shifted group kernels g=%d bwd' % gs] = \
                lambda d=ds, t=thr_s, s=stat_s: nat.group_shifted_bwd(d, g, x, s, None, None, min_val, t)
            wg = torch.nn.Parameter(x.view(out_f, k))
            f, b = rounds.module_pair(Q.ShiftedUint4WeightPerGroupFloat(wg, group_size=gs).to(dev), wg, g.view(out_f, k))
            cands["(a') shifted group module g=%d fwd" % gs] = f
            cands["(a') shifted group module g=%d bwd" % gs] = b
            wc = torch.nn.Parameter(x.view(-1, gs))
            f, b = rounds.module_pair(Q.ShiftedUint8WeightPerChannelFloat(wc, bit_width=bits).to(dev), wc, g.view(-1, gs))
            cands['(b) per-channel module on view(-1, %d) fwd' % gs] = f
            cands['(b) per-channel module on view(-1, %d) bwd' % gs] = b
            dq, thr_q = _fused.group_quant_call(x, gs, 2.0 ** (bits - 1) - 1, -(2.0 ** (bits - 1) - 1),
                                                2.0 ** (bits - 1) - 1, True)
            _, scale_q, stat_q = nat.group_quant_fwd(dq, x, min_val, thr_q)
            cands['(c) symmetric group kernels g=%d fwd' % gs] = \
                lambda d=dq, t=thr_q: nat.group_quant_fwd(d, x, min_val, t)
            cands['(c) symmetric group kernels g=%d bwd' % gs] = \
                lambda d=dq, t=thr_q, s=scale_q, st=stat_q: nat.group_quant_bwd(d, g, x, s, st, None, min_val, t)
        cands.update(rounds.yardstick_cands(rounds.yardstick(x, g, o)))
        res = rounds.timed_rounds(cands, ROUNDS)
        print('== %s (%d MiB per tensor)' % (dn, nbytes >> 20))
        med, best = rounds.report(res, nbytes, 48)
        for gs in (128, 32):
            for way, kind in (('fwd', 'copy'), ('bwd', 'triad')):
                a = med['(a) shifted group kernels g=%d %s' % (gs, way)]
                am = med["(a') shifted group module g=%d %s" % (gs, way)]
                b_ = med['(b) per-channel module on view(-1, %d) %s' % (gs, way)]
                c = med['(c) symmetric group kernels g=%d %s' % (gs, way)]
                print("g=%-3d %s: (a) %.4f ms (a') %.4f ms | (b)/(a) %.2f (b)/(a') %.2f | (a)/(c) %.3f | (a)/(d) %.3f "
                      '(ceiling %s %.4f ms)' % (gs, way, a, am, b_ / a, b_ / am, a / c, a / best[kind], kind, best[kind]))
        del x, g, o, cands, wg, wc
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
