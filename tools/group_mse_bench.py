"""Developer tool: the clip-search group kernels next to the composed route they replace and to the plain group kernels.

    python tools/group_mse_bench.py [--out FILE]    # on the GPU box

An [8192, 8192] bf16 weight, g = 128, 4 bits, 20 candidates (1 - i * 0.025), forward and backward of
  (a) the clip-search kernels (bvq_group_mse_fwd / bvq_group_mse_bwd: one launch each);
  (b) the composed route on the same device tensors -- GroupwiseMSEIntQuant with config.FUSED_PATHS off: the search and
      the quantization at the chosen candidates from the module's sub-modules on torch ops, differentiated by autograd
      (its backward is timed as a whole step, forward + backward);
  (c) the plain group kernels (bvq_group_quant_fwd / bvq_group_quant_bwd): the same bytes, no search.
Interleaved rounds in one process, one warm call in front of every timed call (the queue is never empty when the timed
launch starts), HIP events on the launching stream, median / min over the rounds.  The launches of a call are counted
with torch.profiler in a pass of their own, after the timing.  Before anything is timed, (a) is held against (b): the
chosen candidates, and y at the groups that chose the same one."""
import os
import statistics
import sys

import rounds
from rounds import ROOT

ROUNDS = 9


def kernel_launches(fn):
    """device kernels one call of fn launches (torch.profiler, in a pass of its own)"""
    import torch
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(e.count for e in prof.key_averages() if e.device_type.name == 'CUDA' and 'Memcpy' not in e.key
               and 'Memset' not in e.key)


def main():
    import torch
    sys.path.insert(0, ROOT)
    import brevitas_amd.config as config
    import brevitas_amd.quant as Q
    from brevitas_amd import _native as nat
    from brevitas_amd.csrc import build
    out_path = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    dev = 'cuda:0'
    out_f, k, gs, bits, n_ratios, step = 8192, 8192, 128, 4, 20, 0.025
    thr, min_val = float(2 ** (bits - 1) - 1), 1e-10
    ratios = [1.0 - i * step for i in range(n_ratios)]
    table = nat.mse_ratio_table(ratios)
    torch.manual_seed(0)
    w = torch.nn.Parameter((torch.randn(out_f, k, device=dev) * 0.02).to(torch.bfloat16))
    g = torch.randn(out_f, k, device=dev).to(torch.bfloat16)
    x = w.detach().reshape(-1)
    gf = g.reshape(-1)
    code = nat.dtype_code(torch.bfloat16)
    d = nat.QuantDesc(1, x.numel() // gs, gs, code, code, code, nat.F32, 1, 0, -thr, thr, nat.ROUND, 0, 1,
                      nat.OUT_DEQUANT, nat.PRE_NONE)
    assert nat.group_mse_supported(d, x, n_ratios) and nat.group_quant_supported(d, x)
    q = Q.Int4WeightPerGroupFloatMSE(w, group_size=gs, mse_ratios=ratios).to(dev)

    y_a, scale_a, stat_a, idx_a = nat.group_mse_fwd(d, x, table, min_val, thr)
    _, scale_c, stat_c = nat.group_quant_fwd(d, x, min_val, thr)

    state = {}

    def composed_fwd():
        config.FUSED_PATHS = False
        try:
            w.grad = None
            state['y'], state['scale'], _, _ = q(w)
        finally:
            config.FUSED_PATHS = True
        return state['y']

    def composed_step():
        composed_fwd().backward(g)
        return w.grad

    # (a) against (b) before anything is timed
    y_b = composed_fwd().detach()
    idx_b = q.last_mse_index.reshape(-1)
    agree = idx_a == idx_b
    same = torch.equal(y_a.reshape(-1, gs)[agree].view(torch.int16), y_b.reshape(-1, gs)[agree].view(torch.int16))
    say('# tools/group_mse_bench.py: [%d, %d] bf16 weight, g = %d, int%d, %d candidates, one MI355X' %
        (out_f, k, gs, bits, n_ratios))
    say('# build digest %s' % build.source_digest())
    say('(a) vs (b): %d of %d groups chose the same candidate; y bit-equal at those groups: %s; groups below their '
        'abs-max: %.1f %%' % (int(agree.sum()), agree.numel(), same, 100.0 * float((idx_a > 0).float().mean())))
    assert same and float(agree.float().mean()) >= 0.99

    cands = {
        '(a) clip-search kernels fwd': lambda: nat.group_mse_fwd(d, x, table, min_val, thr),
        '(a) clip-search kernels bwd': lambda: nat.group_mse_bwd(d, gf, x, stat_a, idx_a, None, table, min_val, thr),
        '(b) composed route fwd': composed_fwd,
        '(b) composed route fwd + bwd': composed_step,
        '(c) plain group kernels fwd': lambda: nat.group_quant_fwd(d, x, min_val, thr),
        '(c) plain group kernels bwd': lambda: nat.group_quant_bwd(d, gf, x, scale_c, stat_c, None, min_val, thr),
    }

    res = rounds.timed_rounds(cands, ROUNDS)
    med = {name: statistics.median(ts) for name, ts in res.items()}
    launches = {name: kernel_launches(fn) for name, fn in cands.items()}
    nbytes = x.numel() * x.element_size()
    say('%-32s %10s %10s %9s %s' % ('', 'median ms', 'min ms', 'launches', 'x-sized passes / median'))
    for name, ts in res.items():
        passes = 5 if 'fwd + bwd' in name else 3 if 'bwd' in name else 2
        say('%-32s %10.4f %10.4f %9d %6.2f TB/s' % (name, med[name], min(ts), launches[name],
                                                      passes * nbytes / med[name] / 1e9))
    a_f, a_b = med['(a) clip-search kernels fwd'], med['(a) clip-search kernels bwd']
    b_f, b_s = med['(b) composed route fwd'], med['(b) composed route fwd + bwd']
    c_f, c_b = med['(c) plain group kernels fwd'], med['(c) plain group kernels bwd']
    say('fwd      : (a) %.4f ms | (b)/(a) %.2f | (a)/(c) %.2f' % (a_f, b_f / a_f, a_f / c_f))
    say('bwd      : (a) %.4f ms | (b) fwd + bwd minus fwd %.4f ms, /(a) %.2f | (a)/(c) %.2f'
        % (a_b, b_s - b_f, (b_s - b_f) / a_b, a_b / c_b))
    say('fwd + bwd: (a) %.4f ms | (b)/(a) %.2f | (a)/(c) %.2f' % (a_f + a_b, b_s / (a_f + a_b), (a_f + a_b) / (c_f + c_b)))
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
