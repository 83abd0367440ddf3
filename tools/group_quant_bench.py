"""Developer tool: the group-wise weight quantizer kernels next to the routes they replace and to the chip's ceiling.

    python tools/yardstick.py build      # here (no GPU): build/tools/libyardstick.so
    python tools/group_quant_bench.py    # on the GPU box

An [8192, 8192] weight in bf16 and f16, group sizes 128 and 32, forward and backward of
  (a) the group kernels (bvq_group_quant_fwd / bvq_group_quant_bwd: one launch each);
  (b) the per-channel kernels on the weight regrouped as [groups, g] -- what a per-channel quantizer on w.view(-1, g)
      runs: bvq_stats_fakequant_fwd, bvq_fakequant_bwd_stats;
  (c) the per-channel kernels on the weight as it is, [8192, 8192]: the same bytes, 8192 scales;
  (d) tools/yardstick.hip: the same bytes with no arithmetic, read + write and two reads + write, best of a small sweep.
Interleaved rounds in one process, one warm call in front of every timed call (the queue is never empty when the timed
launch starts), HIP events on the launching stream, median / min over the rounds."""
import sys

import rounds
from rounds import ROOT

ROUNDS = 9


def main():
    import torch
    sys.path.insert(0, ROOT)
    from brevitas_amd import _native as nat
    dev = 'cuda:0'
    out_f, k = 8192, 8192
    bits, thr, min_val = 4, 7.0, 1e-10
    qmax = float(2 ** (bits - 1) - 1)
    zp = torch.zeros(1, device=dev)

    print('# tools/group_quant_bench.py: [%d, %d] weight, int%d, one MI355X; median / min ms over %d interleaved rounds'
          % (out_f, k, bits, ROUNDS))
    for dn, dt in (('bf16', torch.bfloat16), ('f16', torch.float16)):
        torch.manual_seed(0)
        x = (torch.randn(out_f, k, device=dev) * 0.02).to(dt).reshape(-1)
        g = torch.randn(out_f, k, device=dev).to(dt).reshape(-1)
        o = torch.empty_like(x)
        nbytes = x.numel() * x.element_size()
        code = nat.dtype_code(dt)

        def desc(channels, inner):
            return nat.QuantDesc(1, channels, inner, code, code, code, nat.F32, 1, 0, -qmax, qmax, nat.ROUND, 0, 1,
                                 nat.OUT_DEQUANT, nat.PRE_NONE)

        def per_channel(channels, inner):
            """forward / backward of the per-channel route on [channels, inner], as StatsFakeQuantFn calls them"""
            d = desc(channels, inner)

            def fwd():
                r = nat.stats_fakequant_fwd(d, x, min_val, thr, dt)
                if r is None:
                    r = nat.absmax_fakequant_cluster(d, x, min_val, thr, dt)
                if r is None:
                    stat, scale = nat.absmax_scale(x, 1, channels, inner, min_val, thr, dt)
                    return stat, scale, nat.fakequant_fwd(d, x, scale, zp)
                return r
            stat, scale, _ = fwd()

            def bwd():
                dx = nat.fakequant_bwd_stats(d, g, x, scale, zp, stat, dt, thr, dt)
                assert dx is not None
                return dx
            return fwd, bwd

        cands = {}
        for gs in (128, 32):
            d = desc(x.numel() // gs, gs)
            assert nat.group_quant_supported(d, x)
            _, scale_g, stat_g = nat.group_quant_fwd(d, x, min_val, thr)
            cands['(a) group kernels g=%d fwd' % gs] = lambda d=d: nat.group_quant_fwd(d, x, min_val, thr)
            cands['(a) group kernels g=%d bwd' % gs] = \
                lambda d=d, s=scale_g, t=stat_g: nat.group_quant_bwd(d, g, x, s, t, None, min_val, thr)
            f, b = per_channel(x.numel() // gs, gs)
            cands['(b) per-channel on view(-1, %d) fwd' % gs] = f
            cands['(b) per-channel on view(-1, %d) bwd' % gs] = b
        f, b = per_channel(out_f, k)
        cands['(c) per-channel [8192, 8192] fwd'] = f
        cands['(c) per-channel [8192, 8192] bwd'] = b
        cands.update(rounds.yardstick_cands(rounds.yardstick(x, g, o)))
        res = rounds.timed_rounds(cands, ROUNDS)
        print('== %s (%d MiB per tensor)' % (dn, nbytes >> 20))
        med, best = rounds.report(res, nbytes, 46)
        for gs in (128, 32):
            for way, kind in (('fwd', 'copy'), ('bwd', 'triad')):
                a = med['(a) group kernels g=%d %s' % (gs, way)]
                b_ = med['(b) per-channel on view(-1, %d) %s' % (gs, way)]
                c = med['(c) per-channel [8192, 8192] %s' % way]
                print('g=%-3d %s: (a) %.4f ms | (b)/(a) %.2f | (c)/(a) %.2f | (a)/(d) %.3f (ceiling %s %.4f ms)'
                      % (gs, way, a, b_ / a, c / a, a / best[kind], kind, best[kind]))
        del x, g, o, cands
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
