"""bench.py --dump-outputs: what the last timed step returned, written as .npy files the same way on every run, within
the size limit; and --steps is the number of timed steps.  Checked on the CPU route (--device cpu: CPU tensors through
the package's pure-torch route, no kernels, not a measurement)."""
import json
import os
import subprocess
import sys

import numpy as np
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (4, 16, 7, 8)


def _bench(*flags, timeout=240):
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    return subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + list(flags), capture_output=True, text=True,
                          timeout=timeout, env=env, cwd=ROOT)


def test_two_runs_dump_the_same_arrays(tmp_path):
    dumps = []
    for run in ('a', 'b'):
        d = tmp_path / run
        r = _bench('--device', 'cpu', '--act-shape', ','.join(map(str, SHAPE)), '--steps', '3', '--warmup', '1',
                   '--dump-outputs', str(d))
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
        assert len(lines) == 1, r.stdout
        out = json.loads(lines[0])
        assert out['steps'] == 3 and out['ms_per_step'] > 0
        assert out['outputs']['dir'] == str(d)
        dumps.append(d)
    names = sorted(os.listdir(dumps[0]))
    assert names == sorted(n + '.npy' for n in ('act0_y', 'act0_scale', 'act0_zero_point', 'act0_bit_width', 'act0_grad'))
    assert sorted(os.listdir(dumps[1])) == names
    for n in names:
        a, b = np.load(dumps[0] / n), np.load(dumps[1] / n)
        assert a.dtype == np.float32 and a.dtype == b.dtype and a.shape == b.shape
        assert np.array_equal(a, b), n
    assert np.load(dumps[0] / 'act0_y.npy').shape == SHAPE
    assert np.load(dumps[0] / 'act0_grad.npy').shape == SHAPE
    assert np.load(dumps[0] / 'act0_scale.npy').shape == (1, SHAPE[1], 1, 1)


def test_steps_must_be_positive():
    r = _bench('--device', 'cpu', '--act-shape', ','.join(map(str, SHAPE)), '--steps', '0')
    assert r.returncode != 0 and not r.stdout.strip()


class _CountingJob:
    def __init__(self):
        self.calls = []

    def step(self):
        self.calls.append(False)

    def kept_step(self):
        self.calls.append(True)


def test_timed_run_runs_steps_timed_steps_and_keeps_only_the_last():
    job = _CountingJob()
    bench.timed_run(job, 7, 2, 3, 1, torch.device('cpu'), on_gpu=False, keep_last=True)
    assert len(job.calls) == 3 + 2 + 7
    assert job.calls == [False] * 11 + [True]
    job = _CountingJob()
    bench.timed_run(job, 5, 0, 0, 1, torch.device('cpu'), on_gpu=False)
    assert job.calls == [False] * 5


def _job():
    job = bench.Job('act_pc', torch.float32, torch.device('cpu'), None, 0, act_shape=SHAPE)
    bench.timed_run(job, 2, 1, 0, 1, torch.device('cpu'), on_gpu=False, keep_last=True)
    return job


def test_kept_outputs_hold_no_autograd_graph():
    """a kept graph would keep the weight's AccumulateGrad node (and its stream) alive into the steps that follow the
    timed ones, e.g. the HIP-graph capture of a weight workload"""
    job = bench.Job('weight_conv', torch.float32, torch.device('cpu'), None, 0)
    bench.timed_run(job, 1, 0, 0, 1, torch.device('cpu'), on_gpu=False, keep_last=True)
    assert len(job.last) == 1 and len(job.last[0]) == 4
    assert all(t.grad_fn is None and not t.requires_grad for t in job.last[0])


def test_dump_holds_the_last_step_whole_when_it_fits(tmp_path):
    job = _job()
    meta = bench.dump_outputs(job, str(tmp_path))
    y, scale, zp, bw = job.last[0]
    x = job.acts[0][0]
    assert all(m['sampled'] is None for m in meta.values())
    assert np.array_equal(np.load(tmp_path / 'act0_y.npy'), y.detach().numpy())
    assert np.array_equal(np.load(tmp_path / 'act0_scale.npy'), scale.detach().numpy())
    assert np.array_equal(np.load(tmp_path / 'act0_grad.npy'), x.grad.numpy())
    assert float(np.load(tmp_path / 'act0_bit_width.npy')) == float(bw)
    assert float(np.load(tmp_path / 'act0_zero_point.npy')) == float(zp)


def test_larger_arrays_are_a_fixed_seeded_sample_within_the_limit(tmp_path):
    job = _job()
    limit = 4096   # bytes: y and grad (14336 bytes each) must be sampled, scale (64 bytes) stays whole
    meta = bench.dump_outputs(job, str(tmp_path), limit=limit)
    assert sum(os.path.getsize(tmp_path / (n + '.npy')) for n in meta) <= limit
    assert meta['act0_scale']['sampled'] is None
    y, x = job.last[0][0].detach().reshape(-1), job.acts[0][0].grad.reshape(-1)
    for name, full in (('act0_y', y), ('act0_grad', x)):
        k = meta[name]['sampled']
        assert k and k < full.numel()
        got = np.load(tmp_path / (name + '.npy'))
        assert got.shape == (k,)
        # the documented positions: one element at a seeded offset in each of k equal blocks
        stride = full.numel() // k
        gen = torch.Generator().manual_seed(bench.DUMP_SEED)
        idx = torch.arange(k) * stride + torch.randint(0, stride, (k,), generator=gen)
        assert np.array_equal(got, full[idx].numpy())
    again = tmp_path / 'again'
    bench.dump_outputs(job, str(again), limit=limit)
    for name in meta:
        assert np.array_equal(np.load(tmp_path / (name + '.npy')), np.load(again / (name + '.npy')))


class _FakeJob:
    """one large activation and two weights of different sizes (the shape of config 4's step), outputs kept"""

    def __init__(self, sizes):
        g = torch.Generator().manual_seed(7)
        self.acts, self.weights, self.last = [], [], []
        for i, n in enumerate(sizes):
            x = torch.zeros(n)
            x.grad = torch.randn(n, generator=g)
            (self.acts if i == 0 else self.weights).append((x, None, None))
            self.last.append((torch.randn(n, generator=g).to(torch.bfloat16), torch.rand(4, generator=g),
                              torch.tensor(0.0), torch.tensor(8.0)))


def test_arrays_within_their_share_are_written_whole(tmp_path):
    """the arrays share the limit smallest first: a weight larger than a small fixed fraction of the limit, but within
    its share, is written whole; only the activation's arrays are sampled"""
    job = _FakeJob([100000, 3000, 500])
    limit = 200000
    meta = bench.dump_outputs(job, str(tmp_path), limit=limit)
    assert sum(os.path.getsize(tmp_path / (n + '.npy')) for n in meta) <= limit
    assert meta['act0_y']['sampled'] and meta['act0_grad']['sampled']
    for name, m in meta.items():
        if not name.startswith('act0_'):
            assert m['sampled'] is None, name
    assert np.array_equal(np.load(tmp_path / 'weight0_grad.npy'), job.weights[0][0].grad.numpy())
    assert np.array_equal(np.load(tmp_path / 'weight1_y.npy'), job.last[2][0].float().numpy())
    # the activation's two arrays got the rest of the limit between them
    used_whole = sum(os.path.getsize(tmp_path / (n + '.npy')) for n in meta if not n.startswith('act0_'))
    assert meta['act0_y']['sampled'] * 4 * 2 > 0.9 * (limit - used_whole - 2 * 256)
