"""skip_missing= on the host: the five 1-D functions of rr.metrics (and their aliases) drop the pairs whose y_true is NaN and then
make the reference's own numpy calls, so they equal the same function on the filtered arrays bit for bit, a gap-free series gives
the bits of the default call, and the default call is what it was.  Data: the reference-generated cases of
tests/golden/metrics.npz with NaNs put at the first, a middle and the last position of y_true.  Also: the argument checks of
rr.grad.scores(..., skip_missing=True), which need no GPU and no library."""
import inspect
import os
import warnings

import numpy as np
import pytest

from conftest import GOLDEN
import river_route_amd as rr

FUNCTIONS = ('mean_error', 'mean_absolute_error', 'mean_square_error', 'pearson_r', 'kling_gupta_efficiency_2012',
             'me', 'mae', 'mse', 'kge2012')
CASES = ('correlated', 'correlated_weak', 'negative', 'perfect', 'zero_true', 'const_true_1', 'const_pred_2.5', 'const_both',
         'one_nan', 'T1', 'T2')


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(GOLDEN, 'metrics.npz'))


def quiet(f, *args, **kw):
    with warnings.catch_warnings(), np.errstate(all='ignore'):
        warnings.simplefilter('ignore')
        return f(*args, **kw)


def with_gaps(y_true):
    """y_true with NaN at the first, a middle and the last position (as many of them as the series has)."""
    t = np.array(y_true, dtype=np.float64)
    t[sorted({0, len(t) // 2, len(t) - 1})] = np.nan
    return t


def test_every_function_takes_the_keyword_and_defaults_to_off():
    for name in FUNCTIONS + ('scores',):
        assert inspect.signature(getattr(rr.metrics, name)).parameters['skip_missing'].default is False, name
    assert inspect.signature(rr.metrics.Accumulator.__init__).parameters['skip_missing'].default is False
    assert inspect.signature(rr.grad.scores).parameters['skip_missing'].default is False
    assert rr.metrics.SCORES == ('me', 'mae', 'mse', 'pearson_r', 'kge2012')
    from river_route_amd import _lib, engine
    for name in ('metrics_update_missing_dev', 'metrics_adjoint_missing_dev'):
        assert name in engine.__all__ and callable(getattr(engine, name)) and 'rr_' + name in _lib.EXPORTS


@pytest.mark.parametrize('case', CASES)
@pytest.mark.parametrize('name', FUNCTIONS)
def test_1d_equals_the_function_on_the_kept_pairs(golden, case, name):
    f = getattr(rr.metrics, name)
    y_true, y_pred = with_gaps(golden[f'{case}/y_true']), golden[f'{case}/y_pred']
    keep = ~np.isnan(y_true)
    got = quiet(f, y_true, y_pred, skip_missing=True)
    assert np.ndim(got) == 0 and isinstance(got, (np.floating, float)), type(got)
    if not keep.any():
        assert np.isnan(got)
        return
    want = quiet(f, y_true[keep], y_pred[keep])
    np.testing.assert_array_equal(np.float64(got), np.float64(want), err_msg=f'{case} {name}')
    # a NaN simulated at a skipped position is never looked at
    poisoned = y_pred.copy()
    poisoned[~keep] = np.nan
    np.testing.assert_array_equal(np.float64(quiet(f, y_true, poisoned, skip_missing=True)), np.float64(want))


@pytest.mark.parametrize('name', FUNCTIONS)
def test_one_nan_case_becomes_finite(golden, name):
    y_true, y_pred = golden['one_nan/y_true'], golden['one_nan/y_pred']
    assert np.isnan(y_true).sum() == 1 and not np.isnan(y_pred).any() and np.isnan(golden[f'one_nan/{name}'])
    assert np.isfinite(quiet(getattr(rr.metrics, name), y_true, y_pred, skip_missing=True)), name


@pytest.mark.parametrize('case', [c for c in CASES if c != 'one_nan'])
@pytest.mark.parametrize('name', FUNCTIONS)
def test_gap_free_series_gives_the_default_bits(golden, case, name):
    y_true, y_pred = golden[f'{case}/y_true'], golden[f'{case}/y_pred']
    assert not np.isnan(y_true).any()
    got = quiet(getattr(rr.metrics, name), y_true, y_pred, skip_missing=True)
    np.testing.assert_array_equal(np.float64(got), golden[f'{case}/{name}'], err_msg=f'{case} {name}')
    got = quiet(getattr(rr.metrics, name), list(y_true), list(y_pred), skip_missing=True)      # sequences as the default takes them
    np.testing.assert_array_equal(np.float64(got), golden[f'{case}/{name}'], err_msg=f'{case} {name} (lists)')


@pytest.mark.parametrize('name', FUNCTIONS)
def test_all_missing_gives_nan_and_the_default_is_unchanged(golden, name):
    f = getattr(rr.metrics, name)
    y_pred = golden['correlated/y_pred']
    with warnings.catch_warnings():
        warnings.simplefilter('error')      # no "mean of empty slice" on the way
        got = f(np.full(len(y_pred), np.nan), y_pred, skip_missing=True)
    assert np.isnan(got) and np.ndim(got) == 0
    assert np.isnan(quiet(f, np.array([np.nan]), np.array([1.0]), skip_missing=True))
    # inf is not missing
    t = golden['correlated/y_true'].copy()
    t[3] = np.inf
    assert not np.isfinite(quiet(f, t, y_pred, skip_missing=True))
    # the default call on data with NaN: NaN, with or without the keyword spelled out
    gappy = with_gaps(golden['correlated/y_true'])
    assert np.isnan(quiet(f, gappy, y_pred)) and np.isnan(quiet(f, gappy, y_pred, skip_missing=False))
    y_true, y_pred = golden['one_nan/y_true'], golden['one_nan/y_pred']
    np.testing.assert_array_equal(np.float64(quiet(f, y_true, y_pred)), golden[f'one_nan/{name}'])


def test_single_kept_pair_and_length_mismatch():
    m = rr.metrics
    t, p = np.array([np.nan, 3.0, np.nan]), np.array([np.nan, 5.0, 1.0])
    assert m.me(t, p, skip_missing=True) == -2.0 and m.mae(t, p, skip_missing=True) == 2.0 and m.mse(t, p, skip_missing=True) == 4.0
    assert np.isnan(quiet(m.pearson_r, t, p, skip_missing=True)) and np.isnan(quiet(m.kge2012, t, p, skip_missing=True))
    with pytest.raises(ValueError, match='one length'):
        m.me(t, p[:2], skip_missing=True)


def test_grad_scores_argument_checks_need_no_gpu():
    """The checks of tests/test_grad_scores.py::test_argument_checks_need_no_gpu, with skip_missing=True: each raises before any
    device call (these are CPU tensors, and the device is looked at last)."""
    import torch
    T, n, m = 6, 3, 5
    t, p = torch.ones(T, n, dtype=torch.float64), torch.ones(T, n, dtype=torch.float64, requires_grad=True)
    t[2, 1] = float('nan')
    wide = torch.ones(T, m, dtype=torch.float64)

    def S(*args, **kw):
        return rr.grad.scores(*args, skip_missing=True, **kw)

    with pytest.raises(TypeError, match='y_true must be a torch tensor'):
        S(t.numpy(), p)
    with pytest.raises(TypeError, match='y_pred must be a torch tensor'):
        S(t, p.detach().numpy())
    with pytest.raises(TypeError, match='float32 or float64'):
        S(t.to(torch.float16), p)
    with pytest.raises(ValueError, match='1-D .* or 2-D'):
        S(t.reshape(T, n, 1), p)
    with pytest.raises(ValueError, match='must not require grad'):
        S(t.clone().requires_grad_(), p)
    with pytest.raises(ValueError, match='y_true has 6 rows, y_pred 5'):
        S(t, p[:5])
    with pytest.raises(ValueError, match='no rows'):
        S(t[:0], p[:0])
    with pytest.raises(ValueError, match='y_pred has 5 columns, expected 3'):
        S(t, wide)
    with pytest.raises(ValueError, match='1-D integer array of length 3'):
        S(t, wide, columns=[0, 1])
    with pytest.raises(ValueError, match='refers to column 5 of y_pred, which has 5 columns'):
        S(t, wide, columns=[0, 5, 1])
    with pytest.raises(ValueError, match='refers to column -1'):
        S(t, wide, columns=np.array([0, -1, 1]))
    with pytest.raises(ValueError, match='y_true must be on the GPU'):
        S(t, p)
    with pytest.raises(ValueError, match='y_true must be on the GPU'):
        S(t, wide, columns=[4, 4, 0])
