"""bench.py's --dump-outputs on host arrays: every column while the dump fits, otherwise the same seeded columns of every array with
all their rows, in the order asked for, within the budget and the same from run to run; and the arguments the bench refuses."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO


@pytest.fixture
def bench(monkeypatch):
    # bench.py sets this variable for the HIP runtime when it is imported; keep it out of the rest of the session
    monkeypatch.setenv('HSA_ENABLE_IPC_MODE_LEGACY', os.environ.get('HSA_ENABLE_IPC_MODE_LEGACY', '0'))
    import bench
    return bench


def test_dump_outputs_whole_when_it_fits(tmp_path, bench):
    q = torch.rand(1000, dtype=torch.float64)
    out = torch.rand(8, 1000, dtype=torch.float32)
    order = (100 - 8 + np.arange(8)) % 8      # step t in sink row t % 8: the last 8 of 100 steps in step order
    bench.dump_outputs(str(tmp_path), [('final_state', q, None), ('discharge', out, order)])
    assert sorted(os.listdir(tmp_path)) == ['discharge.npy', 'final_state.npy']
    assert np.array_equal(np.load(tmp_path / 'final_state.npy'), q.numpy())
    d = np.load(tmp_path / 'discharge.npy')
    assert d.dtype == np.float32 and np.array_equal(d, out.numpy()[order])


def test_dump_outputs_samples_the_same_columns_within_the_budget(tmp_path, bench, monkeypatch):
    monkeypatch.setattr(bench, 'DUMP_BYTES', 1 << 20)
    n, R = 100_000, 64
    q = torch.arange(n, dtype=torch.float64)      # each value its own column index
    out = torch.arange(R * n, dtype=torch.float64).reshape(R, n)
    order = np.arange(R)[::-1].copy()
    for run in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / run), [('final_state', q, None), ('discharge', out, order)])
    cols = np.load(tmp_path / 'a' / 'final_state.npy').astype(np.int64)
    assert 0 < cols.size < n and np.all(np.diff(cols) > 0)
    assert np.array_equal(np.load(tmp_path / 'a' / 'discharge.npy'), out.numpy()[order][:, cols])
    assert sum(np.load(tmp_path / 'a' / f).nbytes for f in os.listdir(tmp_path / 'a')) <= 1 << 20
    for f in os.listdir(tmp_path / 'a'):
        assert np.array_equal(np.load(tmp_path / 'a' / f), np.load(tmp_path / 'b' / f)), f


@pytest.mark.parametrize('args', [['--steps', '0'], ['--warmup', '-1'], ['--dump-outputs', 'd', '--workload', 'dropin'],
                                  ['--dump-outputs', 'd', '--sequential-parts', '8']])
def test_bench_refuses_before_it_starts(args):
    r = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and 'bench.py: error:' in r.stderr, r.stderr[-2000:]
