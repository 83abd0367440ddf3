"""bench.py --dump-outputs on the device: the arrays written after the timed steps are what the last step computed,
checked against the CPU oracle the way smoke() checks the quantizer (y and scale bit-exact, dx away from the arg-max
deposits), and a sampled dump holds those values at its documented positions."""
import numpy as np
import pytest
import torch

import bench

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
SHAPE = (4, 16, 7, 8)


def _job():
    job = bench.Job('act_pc', torch.bfloat16, DEV, None, 0, act_shape=SHAPE)
    bench.timed_run(job, 3, 1, 0, 1, DEV, keep_last=True)
    return job


def test_dump_is_the_last_step_against_the_oracle(tmp_path, oracle):
    O = oracle
    job = _job()
    meta = bench.dump_outputs(job, str(tmp_path))
    assert all(m['sampled'] is None for m in meta.values())
    x, g, _ = job.acts[0]
    n, c, h, w = SHAPE
    xn, code = O.from_torch(x.detach().cpu().reshape(-1))
    gn, _ = O.from_torch(g.cpu().reshape(-1))
    d = O.make_desc(n, c, h * w, code, code, code, O.F32, scale_per_channel=True, qmin=-128.0, qmax=127.0)
    y_o, dx_o, scale_o, _, _ = O.step_stats_scaled(d, xn, gn, 1e-10, 128.0)

    def widen(bits):   # bf16 bit patterns -> float32 values
        return (bits.astype(np.uint32) << 16).view(np.float32)

    y = np.load(tmp_path / 'act0_y.npy')
    assert y.dtype == np.float32 and y.shape == SHAPE
    assert np.array_equal(y.reshape(-1), widen(y_o))
    scale = np.load(tmp_path / 'act0_scale.npy')
    assert np.array_equal(scale.reshape(-1), widen(scale_o))
    dx = np.load(tmp_path / 'act0_grad.npy').reshape(-1)
    assert np.nonzero(dx != widen(dx_o))[0].size <= c
    assert float(np.load(tmp_path / 'act0_bit_width.npy')) == 8.0


def test_sampled_dump_on_the_device(tmp_path):
    job = _job()
    meta = bench.dump_outputs(job, str(tmp_path), limit=4096)
    y = job.last[0][0].detach().reshape(-1).float().cpu()
    k = meta['act0_y']['sampled']
    assert k and k < y.numel()
    stride = y.numel() // k
    gen = torch.Generator().manual_seed(bench.DUMP_SEED)
    idx = torch.arange(k) * stride + torch.randint(0, stride, (k,), generator=gen)
    assert np.array_equal(np.load(tmp_path / 'act0_y.npy'), y[idx].numpy())
