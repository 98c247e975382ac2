"""
Generates tests/golden/metrics.npz by RUNNING THE REFERENCE's skill scores (river_route/metrics.py, read-only at
/root/reference) on small seeded series.

Runs only in the build container: it refuses to start where /root/reference is absent (the GPU box).  The module needs
numpy only, so it is loaded by file path as it is; the reference's source never enters this repository -- only the
inputs and the outputs it produced are written.

Cases (tests/test_metrics.py CASES): correlated random series, a negative correlation, perfect agreement, an all-zero
observed series (mean_true == 0), constant series of 1.0 and 2.5 (numpy's standard deviation of either is exactly 0),
one NaN, and series of one and of two steps.

    python tests/golden/make_golden_metrics.py
"""
import importlib.util
import os
import sys
import warnings

import numpy as np

REF = '/root/reference'
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
FUNCTIONS = ('mean_error', 'mean_absolute_error', 'mean_square_error', 'pearson_r', 'kling_gupta_efficiency_2012',
             'me', 'mae', 'mse', 'kge2012')


def load_reference_metrics():
    path = os.path.join(REF, 'river_route', 'metrics.py')
    if not os.path.isfile(path):
        raise SystemExit('make_golden_metrics.py: /root/reference is not present; golden vectors can only be '
                         'regenerated in the build container')
    spec = importlib.util.spec_from_file_location('_reference_metrics', path)
    mod = importlib.util.module_from_spec(spec)
    sys.dont_write_bytecode = True
    spec.loader.exec_module(mod)
    return mod


def cases():
    rng = np.random.default_rng(20261015)
    T = 730
    obs = 40.0 + 15.0 * np.sin(np.arange(T) * 2 * np.pi / 365.0) + rng.gamma(2.0, 4.0, T)
    out = {
        'correlated': (obs, 0.9 * obs + 3.0 + rng.normal(0.0, 4.0, T)),
        'correlated_weak': (rng.normal(1.0, 2.0, 500), None),
        'negative': (obs, 120.0 - obs + rng.normal(0.0, 2.0, T)),
        'perfect': (obs, obs.copy()),
        'zero_true': (np.zeros(200), rng.normal(0.5, 1.0, 200)),
        'const_true_1': (np.full(300, 1.0), rng.normal(1.0, 0.3, 300)),
        'const_pred_2.5': (rng.normal(2.0, 0.5, 300), np.full(300, 2.5)),
        'const_both': (np.full(64, 1.0), np.full(64, 2.5)),
        'one_nan': (obs.copy(), 1.1 * obs),
        'T1': (np.array([3.0]), np.array([2.5])),
        'T2': (np.array([3.0, 5.0]), np.array([2.0, 7.5])),
    }
    a, _ = out['correlated_weak']
    out['correlated_weak'] = (a, 0.3 * a + rng.normal(0.0, 2.0, a.size))
    out['one_nan'][0][17] = np.nan
    return out


def main():
    ref = load_reference_metrics()
    out = {}
    with warnings.catch_warnings(), np.errstate(all='ignore'):
        warnings.simplefilter('ignore')
        for tag, (y_true, y_pred) in cases().items():
            out[f'{tag}/y_true'] = y_true
            out[f'{tag}/y_pred'] = y_pred
            for name in FUNCTIONS:
                out[f'{tag}/{name}'] = np.float64(getattr(ref, name)(y_true, y_pred))
    np.savez_compressed(os.path.join(HERE, 'metrics.npz'), **out)
    print('wrote metrics.npz:', {k: float(v) for k, v in out.items() if k.endswith('/kge2012')})


if __name__ == '__main__':
    main()
