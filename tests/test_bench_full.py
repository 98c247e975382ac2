"""bench.py's plain run against `--full`: a plain run times the headline and prints its line, nothing more (no oracle, no copy probe,
no secondary lines); `--full` adds the CPU baseline, the parity gate, the copy probe and, at the headline's size, the secondary lines."""
import json
import os
import subprocess
import sys

import pytest

from conftest import REPO


@pytest.fixture
def bench(monkeypatch):
    # bench.py sets this variable for the HIP runtime when it is imported; keep it out of the rest of the session
    monkeypatch.setenv('HSA_ENABLE_IPC_MODE_LEGACY', os.environ.get('HSA_ENABLE_IPC_MODE_LEGACY', '0'))
    import bench
    return bench


@pytest.mark.parametrize('argv, full, oracle, secondary', [
    ([], False, False, False),
    (['--no-cpu-baseline', '--no-secondary'], False, False, False),
    (['--full'], True, True, True),
    (['--full', '--no-secondary'], True, True, False),
    (['--full', '--no-cpu-baseline'], True, False, True),
])
def test_what_a_run_does_beyond_the_headline(bench, monkeypatch, argv, full, oracle, secondary):
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '1', '--steps', '3', '--warmup', '1', *argv])
    a = bench.parse_args()
    assert (a.full, not a.no_cpu_baseline, a.secondary) == (full, oracle, secondary)
    assert (a.steps, a.warmup, a.reaches, a.runoff_steps) == (3, 1, 1_000_000, 35_040)


@pytest.mark.parametrize('args', [['--secondary'], ['--workload', 'dropin']])
def test_bench_refuses_full_only_parts_in_a_plain_run(args):
    r = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and 'bench.py: error:' in r.stderr and '--full' in r.stderr, r.stderr[-2000:]


def _lines(args):
    r = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--reaches', '100000', '--runoff-steps', '2000', '--steps', '1',
                        '--warmup', '1', *args], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith('{')]


@pytest.mark.gpu
def test_plain_run_and_full_run():
    plain = _lines([])
    assert len(plain) == 1
    p = plain[0]
    assert p['value'] > 0 and p['ms_per_step'] > 0 and p['unit'] == 'reach-steps/s' and p['dtype'] == 'f64' and p['higher_is_better']
    assert p['cpu_baseline'] is None
    assert p['roofline']['avg_launch_us'] > 0 and p['roofline']['peak_measured_copy'] is None

    full = _lines(['--full', '--cpu-replicas', '0', '--cpu-baseline-seconds', '1'])
    assert len(full) == 1      # the secondary lines belong to the headline's size only
    f = full[0]
    assert f['config'] == p['config']
    assert f['cpu_baseline']['value'] > 0 and 'oracle' in f['cpu_baseline']['parity_gate']
    assert f['roofline']['peak_measured_copy'] > 0
