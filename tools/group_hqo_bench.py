"""Developer tool: the HQO zero-point group kernels next to the composed route they replace and to the plain asymmetric
group kernels.

    python tools/group_hqo_bench.py [--out FILE]    # on the GPU box

A [4096, 4096] weight (randn * 0.05, every 37th column times 6), bf16 and f32, g = 64 and 128, 4 bits, the default search
(20 iterations, beta 10, kappa 1.01, p = 0.5), forward and backward of
  (a) the HQO kernels (bvq_group_hqo_fwd / bvq_group_hqo_bwd: one launch each);
  (b) the composed route on the same device tensors -- GroupwiseHQOIntQuant with config.FUSED_PATHS off: the search and
      the quantization at the kept zero-points from the module's sub-modules on torch ops, differentiated by autograd
      (its backward is timed as a whole step, forward + backward);
  (c) the plain asymmetric group kernels (bvq_group_shifted_fwd / bvq_group_shifted_bwd): the same bytes, no search.
Then the forward (a) at 0, 1, 2, 4, 8, 20 and 63 iterations on the same weight (a wave load stops once none of its
groups is live, so the later counts cost what the data makes them cost).
Interleaved rounds in one process, one warm call in front of every timed call (the queue is never empty when the timed
launch starts), HIP events on the launching stream, median / min over the rounds.  The launches of a call are counted
with torch.profiler in a pass of their own, after the timing.  Before anything is timed, (a) is held against (b): every
output bit."""
import os
import statistics
import sys

import rounds
from group_mse_bench import kernel_launches
from rounds import ROOT

ROUNDS = 9
SWEEP = (0, 1, 2, 4, 8, 20, 63)


def main():
    import torch
    sys.path.insert(0, ROOT)
    import brevitas_amd.config as config
    import brevitas_amd.quant as Q
    from brevitas_amd import _native as nat
    from brevitas_amd.core.quant import _fused
    from brevitas_amd.csrc import build
    out_path = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    dev = 'cuda:0'
    out_f, k, bits, iters, beta, kappa, p = 4096, 4096, 4, 20, 10.0, 1.01, 0.5
    qmax, min_val, lp = float(2 ** bits - 1), 1e-10, nat.HQO_LP[p]
    say('# tools/group_hqo_bench.py: [%d, %d] weight, uint%d, %d iterations, beta %g, kappa %g, p %g, one MI355X'
        % (out_f, k, bits, iters, beta, kappa, p))
    say('# build digest %s' % build.source_digest())
    for dt, dn in ((torch.bfloat16, 'bf16'), (torch.float32, 'f32')):
        for gs in (64, 128):
            torch.manual_seed(0)
            w0 = torch.randn(out_f, k, device=dev) * 0.05
            w0[:, ::37] *= 6
            w = torch.nn.Parameter(w0.to(dt))
            g = torch.randn(out_f, k, device=dev).to(dt)
            x, gf = w.detach().reshape(-1), g.reshape(-1)
            d, thr_div = _fused.group_shifted_call(x, gs, qmax, 0.0, qmax, True)
            assert nat.group_hqo_supported(d, x, iters, lp) and nat.group_shifted_supported(d, x)
            table = nat.hqo_beta_table(beta, kappa, iters)
            q = Q.ShiftedUint4WeightPerGroupFloatHQO(w, group_size=gs, hqo_iters=iters, hqo_beta=beta, hqo_kappa=kappa,
                                                     hqo_lp_norm=p).to(dev)
            y_a, scale_a, zp_a, stat_a, idx_a = nat.group_hqo_fwd(d, x, table, lp, min_val, thr_div)
            _, _, _, stat_c = nat.group_shifted_fwd(d, x, min_val, thr_div)
            state = {}

            def composed_fwd():
                config.FUSED_PATHS = False
                try:
                    w.grad = None
                    state['y'], state['scale'], state['zp'], _ = q(w)
                finally:
                    config.FUSED_PATHS = True
                return state['y']

            def composed_step():
                composed_fwd().backward(g)
                return w.grad

            # (a) against (b) before anything is timed
            y_b = composed_fwd().detach().reshape(-1)
            it = torch.int16 if dt == torch.bfloat16 else torch.int32
            same = torch.equal(y_a.view(it), y_b.view(it)) and torch.equal(zp_a.view(it), state['zp'].reshape(-1).view(it)) \
                and torch.equal(idx_a, q.last_hqo_index.reshape(-1))
            say('## %s, g = %d (%d MiB, %d groups)' % (dn, gs, x.numel() * x.element_size() >> 20, x.numel() // gs))
            say('(a) vs (b): y, zero-point and index bit-equal: %s; groups that kept k > 0: %.1f %%, mean k %.2f, max k %d'
                % (same, 100.0 * float((idx_a > 0).float().mean()), float(idx_a.float().mean()), int(idx_a.max())))
            assert same
            cands = {
                '(a) HQO kernels fwd': lambda: nat.group_hqo_fwd(d, x, table, lp, min_val, thr_div),
                '(a) HQO kernels bwd': lambda: nat.group_hqo_bwd(d, gf, x, stat_a, zp_a, None, min_val, thr_div),
                '(b) composed route fwd': composed_fwd,
                '(b) composed route fwd + bwd': composed_step,
                '(c) plain asymmetric kernels fwd': lambda: nat.group_shifted_fwd(d, x, min_val, thr_div),
                '(c) plain asymmetric kernels bwd': lambda: nat.group_shifted_bwd(d, gf, x, stat_c, None, None, min_val,
                                                                                  thr_div),
            }
            # the forward at other iteration counts.  A wave load stops once none of its groups is live, so beyond the
            # first few counts the time follows the data, not n: the first steps, where nearly every group is still
            # live, give the cost of a candidate
            tables = {n: nat.hqo_beta_table(beta, kappa, n) for n in SWEEP}
            for n in SWEEP:
                cands['(a) fwd, %2d iterations' % n] = lambda n=n: nat.group_hqo_fwd(d, x, tables[n], lp, min_val, thr_div)
            res = rounds.timed_rounds(cands, ROUNDS)
            med = {name: statistics.median(ts) for name, ts in res.items()}
            launches = {name: kernel_launches(fn) for name, fn in cands.items() if name[:3] in ('(a)', '(b)', '(c)')
                        and 'iterations' not in name}
            nbytes = x.numel() * x.element_size()
            say('%-44s %10s %10s %9s %s' % ('', 'median ms', 'min ms', 'launches', 'x-sized passes / median'))
            for name, ts in res.items():
                passes = 5 if 'fwd + bwd' in name else 3 if 'bwd' in name else 2
                say('%-44s %10.4f %10.4f %9s %6.2f TB/s' % (name, med[name], min(ts), launches.get(name, ''),
                                                              passes * nbytes / med[name] / 1e9))
            a_f, a_b = med['(a) HQO kernels fwd'], med['(a) HQO kernels bwd']
            b_f, b_s = med['(b) composed route fwd'], med['(b) composed route fwd + bwd']
            c_f, c_b = med['(c) plain asymmetric kernels fwd'], med['(c) plain asymmetric kernels bwd']
            say('fwd      : (a) %.4f ms | (b)/(a) %.2f | (a)/(c) %.2f' % (a_f, b_f / a_f, a_f / c_f))
            say('bwd      : (a) %.4f ms | (b) fwd + bwd minus fwd %.4f ms, /(a) %.2f | (a)/(c) %.2f'
                % (a_b, b_s - b_f, (b_s - b_f) / a_b, a_b / c_b))
            say('fwd + bwd: (a) %.4f ms | (b)/(a) %.2f | (a)/(c) %.2f'
                % (a_f + a_b, b_s / (a_f + a_b), (a_f + a_b) / (c_f + c_b)))
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
