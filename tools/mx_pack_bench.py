"""Developer tool: the MX wire-format kernels (bvq_mx_encode, bvq_mx_decode) next to the fake-quantizer's forward.

    python tools/mx_pack_bench.py        # on the GPU box

An [8192, 8192] bfloat16 tensor, groups of 32, formats e4m3, e2m3 and e2m1 (8, 6 and 4 bits per element):
  fwd     bvq_mx_quant_fwd: reads x, writes y (2 B/elem) and a float32 scale per group -- the yardstick: the same x, more
          bytes written;
  encode  bvq_mx_encode: reads x, writes bits / 8 B/elem of codes and one scale byte per group;
  decode  bvq_mx_decode: reads those, writes y.
All three through the C ABI on preallocated buffers, in one process, in interleaved rounds, one warm call in front of
every timed call (the queue is never empty when the timed launch starts), HIP events on the launching stream; median /
min / max over the rounds, the bytes each call has to move computed from the shapes, and bytes / median as TB/s.  The
encoder's codes are checked against the composed route on a slice first, and the decoder against the forward's y."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUNDS = 15


def main():
    import torch
    sys.path.insert(0, ROOT)
    from brevitas_amd import _native as nat
    from brevitas_amd.core.quant.mx import MX_FORMATS, MXQuant
    dev = 'cuda:0'
    rows, k, gs = 8192, 8192, 32
    dt = torch.bfloat16
    torch.manual_seed(0)
    x = (torch.randn(rows, k, device=dev) * 0.02).to(dt).reshape(-1)
    n, groups = x.numel(), x.numel() // gs
    y = torch.empty_like(x)
    scale = torch.empty(groups, dtype=torch.float32, device=dev)
    code = nat.dtype_code(dt)
    stream = torch.cuda.current_stream().cuda_stream
    lib = nat.lib

    def ev():
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    cands, moved, bufs = {}, {}, {}
    for fmt in ('e4m3', 'e2m3', 'e2m1'):
        f = MX_FORMATS[fmt]
        cbytes = n * f.bit_width // 8
        codes = torch.empty(cbytes, dtype=torch.uint8, device=dev)
        sbytes = torch.empty(groups, dtype=torch.uint8, device=dev)
        bufs[fmt] = (codes, sbytes)

        def fwd(f=f):
            nat.check(lib.bvq_mx_quant_fwd(code, groups, gs, f.code, nat.MX_FLOOR, x.data_ptr(), y.data_ptr(),
                                           scale.data_ptr(), stream), 'bvq_mx_quant_fwd')

        def encode(f=f, codes=codes, sbytes=sbytes):
            nat.check(lib.bvq_mx_encode(code, groups, gs, f.code, nat.MX_FLOOR, x.data_ptr(), codes.data_ptr(),
                                        sbytes.data_ptr(), stream), 'bvq_mx_encode')

        def decode(f=f, codes=codes, sbytes=sbytes):
            nat.check(lib.bvq_mx_decode(code, groups, gs, f.code, codes.data_ptr(), sbytes.data_ptr(), y.data_ptr(),
                                        stream), 'bvq_mx_decode')
        cands['%s fwd' % fmt], moved['%s fwd' % fmt] = fwd, 2 * n + 2 * n + 4 * groups
        cands['%s encode' % fmt], moved['%s encode' % fmt] = encode, 2 * n + cbytes + groups
        cands['%s decode' % fmt], moved['%s decode' % fmt] = decode, cbytes + groups + 2 * n
        # the results, before anything is timed: a slice against the composed route, the decoder against the forward
        encode()
        q = MXQuant(fmt, gs)
        part = q.to_mx_codes(x[:1 << 20].reshape(32, -1).cpu())
        assert torch.equal(codes[:part.codes.numel()].cpu(), part.codes.reshape(-1)), fmt
        assert torch.equal(sbytes[:part.scale_e8m0.numel()].cpu(), part.scale_e8m0.reshape(-1)), fmt
        fwd()
        want = y.clone()
        y.zero_()
        decode()
        assert torch.equal(y.view(torch.int16), want.view(torch.int16)), fmt
        del want

    for fn in cands.values():
        fn()
    torch.cuda.synchronize()
    res = {name: [] for name in cands}
    for rnd in range(ROUNDS):
        pairs = []
        for name, fn in cands.items():
            fn()
            a = ev()
            fn()
            pairs.append((name, a, ev()))
        torch.cuda.synchronize()
        for name, a, b in pairs:
            res[name].append(a.elapsed_time(b))
    print('# tools/mx_pack_bench.py: [%d, %d] bfloat16, groups of %d, one MI355X; median / min / max ms over %d '
          'interleaved rounds' % (rows, k, gs, ROUNDS))
    print('| call | median / min / max ms | max / min | MiB moved | TB/s | time / fwd |')
    print('|---|---|---|---|---|---|')
    for name, ts in res.items():
        med = statistics.median(ts)
        ref = statistics.median(res[name.split(' ')[0] + ' fwd'])
        print('| %s | %.4f / %.4f / %.4f | %.3f | %.1f | %.2f | %.3f |'
              % (name, med, min(ts), max(ts), max(ts) / min(ts), moved[name] / 2 ** 20, moved[name] / med / 1e9,
                 med / ref))


if __name__ == '__main__':
    main()
