"""bench.py's command line on CPU: --dump-outputs writes float32 .npy files within 64 MB, the same sample for the same
output, and the options that cannot hold are refused before any work."""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_whole_and_sampled(tmp_path):
    import bench
    small = torch.arange(2 * 3 * 8 * 8, dtype=torch.float32).reshape(2, 3, 8, 8)
    big = torch.randn(bench.DUMP_WHOLE_BYTES // 4 + 1, generator=torch.Generator().manual_seed(0))
    for d in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / d), {'small': small, 'image': big})
    a = np.load(tmp_path / 'a' / 'small.npy')
    assert a.dtype == np.float32 and a.shape == (2, 3, 8, 8)
    np.testing.assert_array_equal(a, small.numpy())
    s = np.load(tmp_path / 'a' / 'image_sample.npy')
    assert s.dtype == np.float32 and s.shape == (bench.DUMP_SAMPLE,)
    assert not os.path.exists(tmp_path / 'a' / 'image.npy')
    np.testing.assert_array_equal(s, np.load(tmp_path / 'b' / 'image_sample.npy'))
    # the sample is made of the output's own values, drawn from all of it
    idx = torch.randperm(big.numel(), generator=torch.Generator().manual_seed(bench.DUMP_SEED))[:bench.DUMP_SAMPLE]
    np.testing.assert_array_equal(s, big[idx.sort().values].numpy())
    assert idx.max() > 0.99 * big.numel() and idx.min() < 0.01 * big.numel()
    # the flagship's image [8, 3, 1024, 1024] is dumped within the 64 MB bound
    assert min(8 * 3 * 1024 * 1024, bench.DUMP_SAMPLE) * 4 <= 64e6
    total = sum(os.path.getsize(tmp_path / 'a' / f) for f in os.listdir(tmp_path / 'a'))
    assert total <= 64e6


def _bench(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), *args], capture_output=True, text=True,
                          timeout=120, cwd=ROOT)


def test_refused_before_any_work(tmp_path):
    pr = _bench('--gpus', '1', '--steps', '0', '--warmup', '0')
    assert pr.returncode != 0 and '--steps must be at least 1' in pr.stderr
    pr = _bench('--gpus', '1', '--workload', 'train256', '--dump-outputs', str(tmp_path / 'd'))
    assert pr.returncode != 0 and '--dump-outputs' in pr.stderr and not os.path.exists(tmp_path / 'd')
    assert not [ln for ln in pr.stdout.splitlines() if ln.startswith('{')]


def test_full_is_an_option():
    pr = _bench('--help')
    assert pr.returncode == 0 and '--full' in pr.stdout and '--dump-outputs' in pr.stdout
