"""Developer tool: the asymmetric per-row (per-token) activation quantizer kernels next to the route they replace, the
symmetric per-row quantizer and the chip's ceiling.

    python tools/yardstick.py build        # here (no GPU): build/tools/libyardstick.so
    python tools/row_shifted_bench.py      # on the GPU box

[tokens, hidden] activations of [8192, 4096], [8192, 11008] and [32768, 1024] in bf16 and f16, 8 bits, forward and
backward of
  (a)  the row kernels (bvq_row_shifted_fwd / bvq_row_shifted_bwd: one launch each) through their wrappers;
  (a') the same through the module, ShiftedUint8DynamicActPerRowFloat: what a layer pays, autograd included;
  (b)  the route without them: ShiftedUint8WeightPerChannelFloat on the same [tokens, hidden] tensor with the plain clamp,
       through the module -- two statistic passes, scale-shaped torch ops for scale and zero-point, the per-channel
       quantizer kernels, deposit passes through dense temporaries;
  (c)  Int8DynamicActPerRowFloat, the symmetric per-row quantizer on the existing per-channel kernels, through the module;
  (d)  tools/yardstick.hip: the same bytes with no arithmetic, read + write and two reads + write, best of a small sweep.
Interleaved rounds in one process, one warm call in front of every timed call (the queue is never empty when the timed
launch starts), HIP events on the launching stream, median / min over the rounds."""
import sys

import rounds
from rounds import ROOT

ROUNDS = 7
SHAPES = ((8192, 4096), (8192, 11008), (32768, 1024))


def main():
    import torch
    sys.path.insert(0, ROOT)
    from brevitas_amd import _native as nat
    import brevitas_amd.quant as Q
    from brevitas_amd.core.function_wrapper import TensorClamp
    from brevitas_amd.core.quant import _fused
    dev = 'cuda:0'
    bits, min_val = 8, 1e-10
    qmax = 2.0 ** bits - 1

    print('# tools/row_shifted_bench.py: [tokens, hidden] activations, %d bits, one MI355X; median / min ms over %d '
          'interleaved rounds' % (bits, ROUNDS))
    for rows, h in SHAPES:
        for dn, dt in (('bf16', torch.bfloat16), ('f16', torch.float16)):
            torch.manual_seed(0)
            x = (torch.randn(rows, h, device=dev) * 0.5).to(dt)
            g = torch.randn(rows, h, device=dev).to(dt)
            o = torch.empty_like(x)
            nbytes = x.numel() * x.element_size()

            cands = {}
            desc, thr = _fused.row_shifted_call(x, qmax, 0.0, qmax, False)
            assert nat.row_shifted_supported(desc, x)
            stat = nat.row_shifted_fwd(desc, x, min_val, thr)[3]
            cands['(a) row kernels fwd'] = lambda: nat.row_shifted_fwd(desc, x, min_val, thr)
            cands['(a) row kernels bwd'] = lambda: nat.row_shifted_bwd(desc, g, x, stat, None, None, min_val, thr)
            xa = x.clone().requires_grad_(True)
            f, b = rounds.module_pair(Q.ShiftedUint8DynamicActPerRowFloat(bit_width=bits).to(dev), xa, g)
            cands["(a') row module fwd"], cands["(a') row module bwd"] = f, b
            wc = torch.nn.Parameter(x.clone())
            qb = Q.ShiftedUint8WeightPerChannelFloat(wc, bit_width=bits).to(dev)
            qb.int_quant.tensor_clamp_impl = TensorClamp()
            f, b = rounds.module_pair(qb, wc, g)
            cands['(b) per-channel module fwd'], cands['(b) per-channel module bwd'] = f, b
            xc = x.clone().requires_grad_(True)
            f, b = rounds.module_pair(Q.Int8DynamicActPerRowFloat(bit_width=bits).to(dev), xc, g)
            cands['(c) symmetric row module fwd'], cands['(c) symmetric row module bwd'] = f, b
            cands.update(rounds.yardstick_cands(rounds.yardstick(x, g, o)))
            res = rounds.timed_rounds(cands, ROUNDS)
            print('== [%d, %d] %s (%d MiB per tensor)' % (rows, h, dn, nbytes >> 20))
            med, best = rounds.report(res, nbytes, 44)
            for way, kind in (('fwd', 'copy'), ('bwd', 'triad')):
                a = med['(a) row kernels %s' % way]
                am = med["(a') row module %s" % way]
                b_ = med['(b) per-channel module %s' % way]
                c = med['(c) symmetric row module %s' % way]
                print("[%d, %d] %s %s: (a) %.4f ms (a') %.4f ms | (b)/(a) %.2f (b)/(a') %.2f | (a)/(c) %.3f | (a)/(d) "
                      '%.3f (ceiling %s %.4f ms)' % (rows, h, dn, way, a, am, b_ / a, b_ / am, a / c, a / best[kind], kind,
                                                    best[kind]))
            del x, g, o, cands, xa, wc, xc, stat
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
