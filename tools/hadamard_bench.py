"""Developer tool: the Hadamard transform kernel next to what else could compute it.

    python tools/hadamard_bench.py [--out FILE]    # on the GPU box

bf16 [8192, 8192] with b = 8192, [8192, 14336] with b = 2048 and [65536, 4096] with b = 32 (randn):
  (a) the kernel, bvq_hadamard: one launch, x read once and y written once;
  (b) the composed route on the device (brevitas_amd._aten.hadamard): log2 b float32 stages of torch ops;
  (c) the dense route the reference's layer takes, x.view(-1, b) @ H_b in bf16 (the +-1 matrix, unscaled: the scale
      would be one more pass), O(b) multiply-adds per element;
  (d) out.copy_(x): the same bytes read and written with no arithmetic, the floor of a one-read one-write kernel.
Interleaved rounds in one process, one warm call in front of every timed call, HIP events on the launching stream,
median / min over the rounds (tools/rounds.py).  Before anything is timed (a) is held against (b), every bit."""
import os
import statistics
import sys

import rounds
from rounds import ROOT

ROUNDS = 9
CASES = ((8192, 8192, 8192), (8192, 14336, 2048), (65536, 4096, 32))


def main():
    import torch
    sys.path.insert(0, ROOT)
    from brevitas_amd import _aten
    from brevitas_amd import _native as nat
    from brevitas_amd.csrc import build
    from brevitas_amd.function.hadamard import _row_view, hadamard_matrix
    out_path = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    dev, dt = 'cuda:0', torch.bfloat16
    say('# tools/hadamard_bench.py: bf16, one MI355X, %d rounds' % ROUNDS)
    say('# build digest %s' % build.source_digest())
    for rows, cols, b in CASES:
        torch.manual_seed(0)
        x = torch.randn(rows, cols, device=dev).to(dt)
        out = torch.empty_like(x)
        scale = b ** -0.5
        c = _row_view(cols, b, x.element_size())
        r = x.numel() // c
        assert nat.hadamard_supported(x, r, c, b, out)
        h = hadamard_matrix(b, dt, dev)

        def kernel():
            return nat.hadamard(x, r, c, b, scale, out=out)

        def composed():
            return _aten.hadamard(x, b, scale)

        def dense():
            return torch.matmul(x.view(-1, b), h)

        def copy():
            return out.copy_(x)

        same = torch.equal(kernel().view(torch.int16), composed().view(torch.int16))
        nbytes = x.numel() * x.element_size()
        say('## [%d, %d], b = %d (%d MiB; the kernel sees [%d, %d])' % (rows, cols, b, nbytes >> 20, r, c))
        say('(a) vs (b): every bit equal: %s' % same)
        assert same
        cands = {'(a) kernel': kernel, '(b) composed torch ops, float32 stages': composed,
                 '(c) dense x @ H_b, bf16': dense, '(d) out.copy_(x)': copy}
        res = rounds.timed_rounds(cands, ROUNDS)
        med = {name: statistics.median(ts) for name, ts in res.items()}
        say('%-42s %10s %10s  %s' % ('', 'median ms', 'min ms', 'TB/s of x read + y written at the median'))
        for name, ts in res.items():
            say('%-42s %10.4f %10.4f  %5.2f' % (name, med[name], min(ts), 2 * nbytes / med[name] / 1e9))
        a, bb, cc, d = (med[name] for name in cands)
        say('(a) / (d) %.2f, (b) / (a) %.1f, (c) / (a) %.1f' % (a / d, bb / a, cc / a))
        del x, out, h
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
