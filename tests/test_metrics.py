"""rr.metrics on the host: the reference's nine names (river_route/metrics.py), their 1-D results against what the
reference computed (tests/golden/metrics.npz, tests/golden/make_golden_metrics.py), and an import that needs no library."""
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

from conftest import GOLDEN, REPO
import river_route_amd as rr

FUNCTIONS = ('mean_error', 'mean_absolute_error', 'mean_square_error', 'pearson_r', 'kling_gupta_efficiency_2012',
             'me', 'mae', 'mse', 'kge2012')
CASES = ('correlated', 'correlated_weak', 'negative', 'perfect', 'zero_true', 'const_true_1', 'const_pred_2.5', 'const_both',
         'one_nan', 'T1', 'T2')


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(GOLDEN, 'metrics.npz'))


def test_module_and_aliases():
    assert 'metrics' in rr.__all__
    m = rr.metrics
    for name in FUNCTIONS:
        assert callable(getattr(m, name)), name
    assert m.me is m.mean_error
    assert m.mae is m.mean_absolute_error
    assert m.mse is m.mean_square_error
    assert m.kge2012 is m.kling_gupta_efficiency_2012
    assert m.SCORES == ('me', 'mae', 'mse', 'pearson_r', 'kge2012')


def test_golden_covers_every_case(golden):
    assert {k.split('/')[0] for k in golden.files} == set(CASES)


@pytest.mark.parametrize('case', CASES)
@pytest.mark.parametrize('name', FUNCTIONS)
def test_1d_equals_reference(golden, case, name):
    """Bit for bit: the same numpy operations in the same order (NaN where the reference gives NaN)."""
    y_true, y_pred = golden[f'{case}/y_true'], golden[f'{case}/y_pred']
    with warnings.catch_warnings(), np.errstate(all='ignore'):
        warnings.simplefilter('ignore')
        got = getattr(rr.metrics, name)(y_true, y_pred)
    assert np.ndim(got) == 0 and isinstance(got, (np.floating, float)), type(got)
    np.testing.assert_array_equal(np.float64(got), golden[f'{case}/{name}'], err_msg=f'{case} {name}')


def test_reference_quirks_are_kept():
    m = rr.metrics
    y = np.array([1.0, 2.0, 4.0, 8.0])
    p = 3.0 * y
    # gamma is (mean_pred / std_pred) / (mean_true / std_true): a scaled series has the same CV, so gamma == 1 and only beta counts
    np.testing.assert_allclose(m.kge2012(y, p), 1.0 - 2.0, rtol=1e-15)
    # std with ddof 0 and the inverse CV ratio of the reference
    q = y + 5.0
    beta = q.mean() / y.mean()
    gamma = (q.mean() / q.std()) / (y.mean() / y.std())
    np.testing.assert_allclose(m.kge2012(y, q), 1 - np.sqrt((beta - 1) ** 2 + (gamma - 1) ** 2), rtol=1e-14)
    with np.errstate(all='ignore'), warnings.catch_warnings():
        warnings.simplefilter('ignore')
        assert np.isnan(m.pearson_r(np.ones(5), y[:4].tolist() + [3.0]))
        assert np.isnan(m.me(np.array([]), np.array([])))
    assert m.pearson_r(y, -y) == -1.0


def test_package_imports_without_the_library(tmp_path):
    """`import river_route_amd` and 1-D scoring load no librr_hip.so (and need none)."""
    code = ('import sys, numpy as np; sys.path.insert(0, sys.argv[1]); import river_route_amd as rr; '
            'from river_route_amd import _lib; '
            'v = rr.metrics.kge2012(np.arange(1.0, 9.0), np.arange(1.0, 9.0) * 1.1); '
            'assert _lib._lib is None; '
            'assert "librr_hip" not in open("/proc/self/maps").read(); print(float(v))')
    env = dict(os.environ, RR_LIB_PATH=str(tmp_path / 'absent' / 'librr_hip.so'))
    out = subprocess.run([sys.executable, '-c', code, REPO], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert abs(float(out.stdout.split()[-1]) - 0.9) < 1e-12
