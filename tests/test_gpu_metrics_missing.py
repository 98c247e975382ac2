"""rr.metrics.scores(..., skip_missing=True) on the GPU (k_metrics_partial<MISSING> through rr_metrics_update_missing_dev; merge and
finish are the unmasked path's kernels): per-column scores over each column's kept pairs against numpy on those pairs (the host
1-D path on the filtered float64 columns), by the rule of tests/test_gpu_metrics.py::check: equal NaN pattern, rtol 1e-10; 'count'
exact.  Every shape carries the gap pattern of missing_helpers.gap_mask: 30 % at random, a gap-free column, whole chunks (at n = 7
whole row splits) missing, every chunk's pivot row missing, the tail row missing, one pair kept, nothing kept.  Also: gap-free
data against the unmasked path, NaN simulated at skipped and at kept rows, a column map whose repeat has two different gap
patterns, row-pitched views, Accumulator row blocks with a block that is entirely missing for a column, repeat runs, and the
ABI's refusals."""
import functools

import numpy as np
import pytest

import river_route_amd as rr
from missing_helpers import SCORES, gap_mask, host_scores_kept, with_gaps
from river_route_amd import _lib, engine
from test_gpu_metrics import bits, check, numpy_of, series

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64


@functools.lru_cache(maxsize=None)
def case(T, n, dt=F64, dp=F64):
    """(y_true with gaps, y_pred, numpy on the kept pairs) of one shape, computed once; nobody writes to them."""
    y_true, y_pred = series(np.random.default_rng(T * 7 + n), T, n, dt, dp)
    y_true = with_gaps(y_true, gap_mask(T, n, seed=T + n))
    want = host_scores_kept(y_true, y_pred)
    for a in (y_true, y_pred, *want.values()):
        a.setflags(write=False)
    return y_true, y_pred, want


def check_missing(got, want, what):
    assert set(got) == set(SCORES) | {'count'}, sorted(got)
    np.testing.assert_array_equal(numpy_of(got['count']), want['count'], err_msg=f'{what}: count')
    check(got, want, what=what)


@pytest.mark.parametrize('T,n,dt,dp', [(2, 3, F64, F64), (33, 300, F64, F64), (3000, 7, F64, F64), (700, 300, F64, F64), (3504, 1000, F64, F64),
                                       (33, 300, F32, F32), (33, 300, F32, F64), (33, 300, F64, F32),
                                       (700, 300, F32, F32), (700, 300, F32, F64), (700, 300, F64, F32)])
def test_numpy_columns_vs_host_on_kept_pairs(T, n, dt, dp):
    y_true, y_pred, want = case(T, n, dt, dp)
    assert y_true.dtype == dt and y_pred.dtype == dp
    if (T, n) != (2, 3):      # every pattern column is there, and every other column has a score
        ordinary = np.ones(n, dtype=bool)
        ordinary[4:6] = False
        assert all(np.isfinite(want[k][ordinary]).all() for k in SCORES)
        assert want['count'][4] == 1 and want['count'][5] == 0 and want['count'][0] == T
    got = rr.metrics.scores(y_true, y_pred, skip_missing=True)
    assert all(isinstance(v, np.ndarray) and v.shape == (n,) and v.dtype == F64 for v in got.values())
    check_missing(got, want, f'{T}x{n} {dt.__name__}/{dp.__name__}')
    if n > 5:
        assert all(np.isnan(got[k][5]) for k in SCORES)                                               # N = 0
        assert all(np.isfinite(got[k][4]) for k in SCORES[:3]) and np.isnan(got['pearson_r'][4]) and np.isnan(got['kge2012'][4])   # N = 1
    # the five 2-D functions are the rows of scores()
    np.testing.assert_array_equal(rr.metrics.kge2012(y_true, y_pred, skip_missing=True), got['kge2012'])
    np.testing.assert_array_equal(rr.metrics.me(y_true, y_pred, skip_missing=True), got['me'])
    # without the keyword: what it was, and no 'count'
    plain = rr.metrics.scores(y_true, y_pred)
    assert set(plain) == set(SCORES)
    gappy = np.isnan(y_true).any(0)
    assert all(np.isnan(plain[k][gappy]).all() for k in SCORES)


def test_one_row_one_column_kept_and_missing():
    got = rr.metrics.scores(np.array([[3.0]]), np.array([[5.0]]), skip_missing=True)
    assert got['count'][0] == 1 and got['me'][0] == -2.0 and got['mae'][0] == 2.0 and got['mse'][0] == 4.0
    assert np.isnan(got['pearson_r'][0]) and np.isnan(got['kge2012'][0])
    got = rr.metrics.scores(np.array([[np.nan]]), np.array([[5.0]]), skip_missing=True)
    assert got['count'][0] == 0 and all(np.isnan(got[k][0]) for k in SCORES)
    check_missing(got, host_scores_kept(np.array([[np.nan]]), np.array([[5.0]])), '1x1 missing')


def test_inf_is_kept():
    y_true, y_pred, _ = case(33, 300)
    t = y_true.copy()
    t[7, 0] = np.inf
    got = rr.metrics.scores(t, y_pred, skip_missing=True)
    assert got['count'][0] == 33 and not np.isfinite(got['mae'][0])


@pytest.mark.parametrize('T,n,dt,dp', [(700, 300, F64, F64), (3000, 7, F64, F64), (33, 300, F32, F32), (3504, 1000, F64, F32)])
def test_gap_free_data_against_the_unmasked_path(T, n, dt, dp):
    """A gap-free column's pivot is its first row, as in k_metrics_partial: within 1e-12 relative, the bound Accumulator documents
    for regrouped sums (in fact the same operations; whether the bits come out equal is printed)."""
    y_true, y_pred = series(np.random.default_rng(T + n), T, n, dt, dp)
    masked, plain = rr.metrics.scores(y_true, y_pred, skip_missing=True), rr.metrics.scores(y_true, y_pred)
    np.testing.assert_array_equal(masked['count'], float(T))
    same = all(np.array_equal(masked[k], plain[k], equal_nan=True) for k in SCORES)
    print(f'gap-free {T}x{n} {dt.__name__}/{dp.__name__}: bits equal to the unmasked path: {same}')
    check(masked, plain, rtol=1e-12, what=f'gap-free {T}x{n}')


def test_nan_simulated_at_a_skipped_row_and_at_a_kept_row():
    T, n = 700, 300
    y_true, y_pred, want = case(T, n)
    miss = np.isnan(y_true)
    first = rr.metrics.scores(y_true, y_pred, skip_missing=True)
    p = y_pred.copy()
    p[miss] = np.nan                                  # every skipped element, pivot rows of column 2 among them
    assert bits(rr.metrics.scores(y_true, p, skip_missing=True)) == bits(first)
    p = y_pred.copy()
    kept_rows = {j: int(np.flatnonzero(~miss[:, j])[k]) for j, k in ((0, 0), (1, 40), (2, 0), (7, -1))}
    for j, r in kept_rows.items():
        p[r, j] = np.nan
    got = rr.metrics.scores(y_true, p, skip_missing=True)
    for j in kept_rows:
        assert all(np.isnan(got[k][j]) for k in SCORES), j
    np.testing.assert_array_equal(got['count'], want['count'])
    others = np.setdiff1d(np.arange(n), list(kept_rows))
    assert all(np.array_equal(got[k][others], first[k][others], equal_nan=True) for k in SCORES)


def test_columns_map_with_a_repeat_of_different_gaps():
    import torch
    rng = np.random.default_rng(11)
    T, m, n = 700, 40, 64
    _, y_pred = series(rng, T, m)
    columns = rng.integers(0, m, n)
    columns[:4] = [7, 7, m - 1, 0]                    # pattern columns 0 (gap-free) and 1 (rows 32..127 missing) share column 7
    columns[20], columns[21] = columns[10], columns[10]      # and three columns with random gaps of their own share another
    y_true = with_gaps(y_pred[:, columns] * rng.uniform(0.5, 1.5, n) + rng.normal(0, 1.0, (T, n)), gap_mask(T, n, seed=5))
    want = host_scores_kept(y_true, y_pred, columns)
    assert want['count'][0] == T and want['count'][1] == T - 96
    got = rr.metrics.scores(y_true, y_pred, columns=columns, skip_missing=True)
    check_missing(got, want, 'columns')
    assert bits(got) == bits(rr.metrics.scores(y_true, np.ascontiguousarray(y_pred[:, columns]), skip_missing=True))
    # torch in: device tensors out, 'count' among them
    t, p = torch.tensor(y_true).cuda(), torch.tensor(y_pred).cuda()
    dev = rr.metrics.scores(t, p, columns=columns, skip_missing=True)
    assert all(torch.is_tensor(v) and v.is_cuda and v.dtype == torch.float64 and v.shape == (n,) for v in dev.values())
    assert not dev['count'].requires_grad and bits(dev) == bits(got)


def test_row_pitched_views_are_read_in_place():
    import torch
    T, n, extra = 700, 300, 37
    y_true, y_pred, want = case(T, n, F64, F32)
    dev = torch.device('cuda', 0)
    bt = torch.full((T, n + extra), float('nan'), dtype=torch.float64, device=dev)      # NaN beside the view: never read
    bp = torch.full((T, n + 2 * extra), float('nan'), dtype=torch.float32, device=dev)
    bt[:, 5:5 + n] = torch.tensor(y_true).to(dev)
    bp[:, extra:extra + n] = torch.tensor(y_pred).to(dev)
    vt, vp = bt[:, 5:5 + n], bp[:, extra:extra + n]
    assert vt.stride() == (n + extra, 1) and not vt.is_contiguous()
    got = rr.metrics.scores(vt, vp, skip_missing=True)
    assert bits(got) == bits(rr.metrics.scores(vt.contiguous(), vp.contiguous(), skip_missing=True))
    check_missing(got, want, 'pitched')


@pytest.mark.parametrize('kind', ['numpy', 'torch'])
def test_accumulator_row_blocks_match_one_pass(kind):
    T, n = 700, 300
    y_true, y_pred, want = case(T, n, F64, F32)
    cuts = [0, 1, 32, 65, 128, 333, 640, T]          # rows 32..64 and 65..127: blocks entirely missing for column 1
    assert np.isnan(y_true[32:65, 1]).all() and np.isnan(y_true[65:128, 1]).all()
    if kind == 'torch':
        import torch
        y_true, y_pred = torch.tensor(y_true).cuda(), torch.tensor(y_pred).cuda()
    acc = rr.metrics.Accumulator(n, skip_missing=True)
    assert acc.skip_missing and not rr.metrics.Accumulator(n).skip_missing
    for a, b in zip(cuts[:-1], cuts[1:]):
        acc.update(y_true[a:b], y_pred[a:b])
    assert acc.rows == T                              # the rows seen, missing or not
    chunked, one = acc.result(), rr.metrics.scores(y_true, y_pred, skip_missing=True)
    if kind == 'torch':
        assert all(v.is_cuda for v in chunked.values())
    np.testing.assert_array_equal(numpy_of(chunked['count']), want['count'])
    check(chunked, {k: numpy_of(v) for k, v in one.items()}, rtol=1e-12, what='row blocks')
    acc2 = rr.metrics.Accumulator(n, skip_missing=True)
    for a, b in zip(cuts[:-1], cuts[1:]):
        acc2.update(y_true[a:b], y_pred[a:b])
    assert bits(acc2.result()) == bits(chunked)
    check_missing(one, want, 'one pass')


def test_repeat_calls_bit_identical():
    import torch
    y_true, y_pred, _ = case(3504, 1000)
    t, p = torch.tensor(y_true).cuda(), torch.tensor(y_pred).cuda()
    first = bits(rr.metrics.scores(t, p, skip_missing=True))
    for _ in range(3):
        assert bits(rr.metrics.scores(t, p, skip_missing=True)) == first
    assert bits(rr.metrics.scores(y_true, y_pred, skip_missing=True)) == first


def test_abi_refusals():
    L = _lib.lib()
    n, T = 300, 100
    need = engine.metrics_work_bytes(n, T)
    rows = np.ones((T, n))
    rows[10:20, 3] = np.nan
    t = engine.DeviceBuffer(T * n * 8).upload(rows)
    p = engine.DeviceBuffer(T * n * 8).upload(np.ones((T, n)))
    state = engine.DeviceBuffer(engine.METRICS_STATE * n * 8).upload(np.zeros(engine.METRICS_STATE * n))
    work = engine.DeviceBuffer(need)
    args = lambda **kw: [kw.get('device', 0), kw.get('n', n), kw.get('rows', T), kw.get('yt', t.address), 0, kw.get('tp', n),      # noqa: E731
                         kw.get('yp', p.address), 0, kw.get('pp', n), None, kw.get('state', state.address), kw.get('work', work.address),
                         kw.get('wb', need), None]
    assert L.rr_metrics_update_missing_dev(*args()) == _lib.RR_OK
    for bad in (dict(yt=None), dict(yp=None), dict(state=None), dict(work=None), dict(wb=need - 8), dict(tp=n - 1),
                dict(pp=n - 1), dict(n=-1), dict(rows=-2)):
        assert L.rr_metrics_update_missing_dev(*args(**bad)) == _lib.RR_E_INVALID, bad
        assert b'rr_metrics' in L.rr_last_error()
    assert L.rr_metrics_update_missing_dev(*args(device=-1)) == _lib.RR_E_NO_DEVICE
    assert L.rr_metrics_update_missing_dev(*args(rows=0)) == _lib.RR_OK
    assert L.rr_metrics_finish_dev(0, n, state.address, work.address, None) == _lib.RR_OK
    engine.synchronize(0)
    res = work.download(np.float64, (5, n))
    np.testing.assert_array_equal(res[:3], 0.0)                 # ones against ones: no error, and r / KGE undefined
    assert np.isnan(res[3:]).all()
    count = state.download(np.float64, (engine.METRICS_STATE, n))[0]
    assert count[3] == T - 10 and (np.delete(count, 3) == T).all()
    # an update with and one without the rule on one state: the count is the sum, and the plain update's NaN poisons its column
    assert L.rr_metrics_update_dev(*args()) == _lib.RR_OK
    assert L.rr_metrics_finish_dev(0, n, state.address, work.address, None) == _lib.RR_OK
    engine.synchronize(0)
    count = state.download(np.float64, (engine.METRICS_STATE, n))[0]
    res = work.download(np.float64, (5, n))
    assert count[3] == 2 * T - 10 and np.isnan(res[:, 3]).all() and (res[:3, :3] == 0.0).all()
