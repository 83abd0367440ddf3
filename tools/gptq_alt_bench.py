"""The rejected shape of the GPTQ column-loop kernel against the one the library ships (profiles/gptq.md).

    python tools/gptq_alt_bench.py build    # no GPU needed: hipcc tools/gptq_lane_per_row.hip -> build/tools/
    python tools/gptq_alt_bench.py run [--shapes 4096x4096,11008x4096] [--reps 5]

tools/gptq_lane_per_row.hip: one lane per row on a transposed float32 working copy, U read wave-uniformly.  `run` first
holds its codes and errors of block 0 against bvq_gptq_block's, bit for bit, then times the K / 128 launches of each
kernel back to back (HIP events, medians; bf16, 4-bit symmetric, group size 128).  The transposition the rejected shape
needs before and after is timed on its own and not charged to it.  One JSON line per shape."""
import argparse
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SO = os.path.join(ROOT, 'build', 'tools', 'libgptq_lane_per_row.so')


def build():
    os.makedirs(os.path.dirname(SO), exist_ok=True)
    subprocess.check_call(['hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off',
                           '-fno-fast-math', '-I' + os.path.join(ROOT, 'include'),
                           os.path.join(ROOT, 'tools', 'gptq_lane_per_row.hip'), '-o', SO])
    print(SO)


def run(args):
    import torch
    from brevitas_amd import _native as nat
    from brevitas_amd import quant as Q
    from brevitas_amd.graph import gptq as G
    from gptq_bench import timed

    lib = ctypes.CDLL(SO)
    fn = lib.gptq_lane_per_row_block
    vp, i64, f32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_float
    fn.argtypes = [vp, vp, vp, vp, i64, i64, i64, f32, f32, f32, f32, vp]
    fn.restype = ctypes.c_int
    dev = torch.device('cuda', 0)
    for shape in args.shapes.split(','):
        rows, k = (int(v) for v in shape.split('x'))
        torch.manual_seed(0)
        w = torch.nn.Parameter((0.05 * torch.randn(rows, k, device=dev)).to(torch.bfloat16))
        x = torch.randn(2 * k, k, device=dev)
        x = x + 0.5 * x.roll(1, dims=1)
        h = (2.0 / x.shape[0]) * (x.t() @ x)
        del x
        quant = Q.Int4WeightPerGroupFloat(w, 128).to(dev)
        plan = G._plan(quant, k, False)
        fa = G.fused_block_args(plan, rows, k, w.dtype)
        wf = w.detach().float()
        u = G.prepare_hessian(h, wf, 0.01)
        q = torch.zeros_like(w)
        scale = torch.empty(rows, k // 128, dtype=w.dtype, device=dev)

        transpose_ms = timed(lambda: wf.t().contiguous(), args.reps)
        wft = wf.t().contiguous()
        qt = torch.zeros(k, rows, dtype=w.dtype, device=dev)
        et = torch.zeros(128, rows, dtype=torch.float32, device=dev)
        stream = nat.stream_ptr(dev)

        def alt_block(c0):
            rc = fn(wft.data_ptr(), u.data_ptr(), qt.data_ptr(), et.data_ptr(), rows, k, c0, plan.qmin, plan.qmax,
                    fa.min_val, fa.thr_div, stream)
            assert rc == 0, rc

        # block 0 of both, bit for bit
        err = G.fused_block(fa, plan, wf, u, 0, 128, q, scale, None)
        alt_block(0)
        torch.cuda.synchronize()
        same_q = bool(torch.equal(qt[:128].t().contiguous().view(torch.int16), q[:, :128].contiguous().view(torch.int16)))
        same_e = bool(torch.equal(et.t().contiguous().view(torch.int32), err.view(torch.int32)))

        def shipped():
            for c0 in range(0, k, 128):
                G.fused_block(fa, plan, wf, u, c0, c0 + 128, q, scale, None)

        def rejected():
            for c0 in range(0, k, 128):
                alt_block(c0)
        print(json.dumps(dict(shape=[rows, k], same_codes=same_q, same_errors=same_e,
                              wave_per_row_ms=round(timed(shipped, args.reps), 3),
                              lane_per_row_ms=round(timed(rejected, args.reps), 3),
                              transpose_ms=round(transpose_ms, 3), launches=k // 128)), flush=True)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('cmd', choices=['build', 'run'])
    ap.add_argument('--shapes', default='4096x4096,11008x4096')
    ap.add_argument('--reps', type=int, default=5)
    a = ap.parse_args()
    build() if a.cmd == 'build' else run(a)
