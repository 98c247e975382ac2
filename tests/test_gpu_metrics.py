"""rr.metrics on the GPU (k_metrics_partial / k_metrics_merge / k_metrics_finish through rr_metrics_update_dev and
rr_metrics_finish_dev): per-column scores of (T, n) arrays against the host 1-D path run on each column of the float64
data (float32 data widened), rtol 1e-10 (me: also 1e-10 x mae; pearson_r and kge2012: the project's 1e-10 x max|want|).
Shapes from one row or one column up to a year of 15-minute steps, all four dtype pairs, row pitches wider than the
row, column maps with repeats, NaN / all-zero / constant columns, row blocks against one pass, repeat runs, torch
tensors in and out, and the ABI's refusals."""
import ctypes as C
import warnings

import numpy as np
import pytest

import river_route_amd as rr
from river_route_amd import _lib, engine

pytestmark = pytest.mark.gpu

SCORES = rr.metrics.SCORES
F32, F64 = np.float32, np.float64


def series(rng, T, n, dtype_t=F64, dtype_p=F64):
    """Hydrograph-like observed columns (positive, seasonal, column scales over four decades) and simulations that are
    scaled, shifted and noisy copies of them, some anti-correlated."""
    scale = 10.0 ** rng.uniform(-1, 3, n)
    phase = rng.uniform(0, 2 * np.pi, n)
    tt = np.arange(T)[:, None]
    obs = scale * (2.0 + np.sin(tt * 2 * np.pi / 35040.0 * 4 + phase) + rng.gamma(2.0, 0.3, (T, n)))
    a = rng.uniform(-0.5, 1.5, n)
    sim = a * obs + scale * rng.uniform(-0.5, 0.5, n) + scale * rng.normal(0.0, 0.4, (T, n))
    return obs.astype(dtype_t), sim.astype(dtype_p)


def host_scores(y_true, y_pred, columns=None):
    """The host 1-D path (rr.metrics on numpy 1-D series) on every column of the float64 data."""
    t = np.ascontiguousarray(np.asarray(y_true, dtype=F64).T)
    p = np.asarray(y_pred, dtype=F64)
    p = np.ascontiguousarray((p[:, columns] if columns is not None else p).T)
    fns = [rr.metrics.me, rr.metrics.mae, rr.metrics.mse, rr.metrics.pearson_r, rr.metrics.kge2012]
    out = {k: np.empty(t.shape[0]) for k in SCORES}
    with warnings.catch_warnings(), np.errstate(all='ignore'):
        warnings.simplefilter('ignore')
        for j in range(t.shape[0]):
            for k, f in zip(SCORES, fns):
                out[k][j] = f(t[j], p[j])
    return out


def numpy_of(v):
    return v.detach().cpu().numpy() if hasattr(v, 'detach') else np.asarray(v)


def check(got, want, rtol=1e-10, what=''):
    got = {k: numpy_of(v) for k, v in got.items()}
    for k in SCORES:
        g, w = got[k], np.asarray(want[k])
        assert g.shape == w.shape, f'{what} {k}: shape {g.shape} != {w.shape}'
        np.testing.assert_array_equal(np.isnan(g), np.isnan(w), err_msg=f'{what} {k}: NaN pattern')
        ok = ~np.isnan(w)
        if k == 'me':
            atol = rtol * np.abs(np.asarray(want['mae']))[ok]
        elif k in ('pearson_r', 'kge2012'):
            atol = rtol * (np.abs(w[ok]).max() if ok.any() else 0.0)
        else:
            atol = 0.0
        err = np.abs(g[ok] - w[ok])
        bad = err > rtol * np.abs(w[ok]) + atol
        assert not bad.any(), f'{what} {k}: {int(bad.sum())} columns off, worst got {g[ok][bad][:3]} want {w[ok][bad][:3]}'


def torch_ref(t, p):
    """Two-pass float64 scores of every column on the device (for shapes too wide for a per-column host loop)."""
    import torch
    t, p = t.double(), p.double()
    N = t.shape[0]
    d = t - p
    at, ap = t - t.mean(0), p - p.mean(0)
    m2t, m2p, c = (at * at).sum(0), (ap * ap).sum(0), (at * ap).sum(0)
    nan = torch.full_like(m2t, float('nan'))
    r = torch.where((m2t > 0) & (m2p > 0), (c / m2t.sqrt() / m2p.sqrt()).clamp(-1.0, 1.0), nan)
    mt, mp = t.mean(0), p.mean(0)
    st, sp = (m2t / N).sqrt(), (m2p / N).sqrt()
    kge = 1 - ((r - 1) ** 2 + (mp / mt - 1) ** 2 + ((mp / sp) / (mt / st) - 1) ** 2).sqrt()
    kge = torch.where((st == 0) | (sp == 0) | (mt == 0), nan, kge)
    return {'me': d.mean(0), 'mae': d.abs().mean(0), 'mse': (d * d).mean(0), 'pearson_r': r, 'kge2012': kge}


def bits(res):
    return {k: numpy_of(v).tobytes() for k, v in res.items()}


@pytest.mark.parametrize('dt,dp', [(F64, F64), (F32, F32), (F32, F64), (F64, F32)])
@pytest.mark.parametrize('T,n', [(1, 1), (1, 37), (2, 7), (33, 300), (35040, 1000)])
def test_numpy_columns_vs_host(T, n, dt, dp):
    rng = np.random.default_rng(T * 7 + n)
    y_true, y_pred = series(rng, T, n, dt, dp)
    got = rr.metrics.scores(y_true, y_pred)
    assert all(isinstance(v, np.ndarray) and v.shape == (n,) and v.dtype == F64 for v in got.values())
    check(got, host_scores(y_true, y_pred), what=f'{T}x{n} {dt.__name__}/{dp.__name__}')
    # the five 2-D functions are the rows of scores()
    np.testing.assert_array_equal(rr.metrics.kge2012(y_true, y_pred), got['kge2012'])
    np.testing.assert_array_equal(rr.metrics.me(y_true, y_pred), got['me'])


@pytest.mark.parametrize('T,n,dt,dp', [(8, 1_000_000, F64, F64), (3504, 100_000, F64, F64), (3504, 100_000, F32, F64)])
def test_wide_torch_vs_reference(T, n, dt, dp):
    import torch
    dev = torch.device('cuda', 0)
    g = torch.Generator(device=dev).manual_seed(T + n)
    scale = 10.0 ** (torch.rand(n, generator=g, device=dev, dtype=torch.float64) * 4 - 1)
    obs = scale * (1.0 + torch.rand((T, n), generator=g, device=dev, dtype=torch.float64))
    sim = (0.8 * obs + scale * torch.randn((T, n), generator=g, device=dev, dtype=torch.float64) * 0.3)
    tdt = torch.float32 if dt == F32 else torch.float64
    tdp = torch.float32 if dp == F32 else torch.float64
    obs, sim = obs.to(tdt), sim.to(tdp)
    got = rr.metrics.scores(obs, sim)
    assert all(torch.is_tensor(v) and v.device == dev and v.dtype == torch.float64 and v.shape == (n,) for v in got.values())
    check(got, {k: numpy_of(v) for k, v in torch_ref(obs, sim).items()}, what=f'{T}x{n} torch ref')
    cols = np.sort(np.random.default_rng(1).choice(n, 48, replace=False))
    want = host_scores(obs[:, cols].cpu().numpy(), sim[:, cols].cpu().numpy())
    check({k: numpy_of(v)[cols] for k, v in got.items()}, want, what=f'{T}x{n} sampled host')


def test_row_pitch_wider_than_row():
    import torch
    rng = np.random.default_rng(5)
    T, n, extra = 1000, 513, 37
    y_true, y_pred = series(rng, T, n)
    dev = torch.device('cuda', 0)
    bt = torch.zeros((T, n + extra), dtype=torch.float64, device=dev)
    bp = torch.zeros((T, n + 2 * extra), dtype=torch.float32, device=dev)
    bt[:, 5:5 + n] = torch.from_numpy(y_true).to(dev)
    bp[:, extra:extra + n] = torch.from_numpy(y_pred.astype(F32)).to(dev)
    vt, vp = bt[:, 5:5 + n], bp[:, extra:extra + n]
    assert vt.stride() == (n + extra, 1) and not vt.is_contiguous()
    got = rr.metrics.scores(vt, vp)
    assert bits(got) == bits(rr.metrics.scores(vt.contiguous(), vp.contiguous()))
    check(got, host_scores(y_true, y_pred.astype(F32)), what='pitched')


def test_columns_map_with_repeats():
    rng = np.random.default_rng(11)
    T, m, n = 2000, 300, 500
    _, y_pred = series(rng, T, m)
    columns = rng.integers(0, m, n)
    columns[:4] = [0, m - 1, 7, 7]
    y_true = y_pred[:, columns] * rng.uniform(0.5, 1.5, n) + rng.normal(0, 1.0, (T, n))
    got = rr.metrics.scores(y_true, y_pred, columns=columns)
    check(got, host_scores(y_true, y_pred, columns), what='columns')
    assert bits(got) == bits(rr.metrics.scores(y_true, np.ascontiguousarray(y_pred[:, columns])))
    with pytest.raises(ValueError, match='refers to column'):
        rr.metrics.scores(y_true, y_pred, columns=np.where(columns == 7, m, columns))
    with pytest.raises(ValueError, match='negative'):
        rr.metrics.scores(y_true, y_pred, columns=np.where(columns == 7, -1, columns))
    with pytest.raises(ValueError, match='length'):
        rr.metrics.scores(y_true, y_pred, columns=columns[:-1])
    with pytest.raises(ValueError, match='columns'):
        rr.metrics.scores(y_true, y_pred)                     # 500 true columns against 300 predicted ones


def test_nan_zero_and_constant_columns():
    rng = np.random.default_rng(3)
    T, n = 35040, 64
    y_true, y_pred = series(rng, T, n)
    y_true[1234, 0] = np.nan                # one NaN observed
    y_pred[0, 1] = np.nan                   # one NaN simulated (in the pivot row of the first chunk)
    y_true[:, 2] = 0.0                      # all-zero observed: mean_true == 0
    y_true[:, 3] = 1.0                      # constant observed
    y_pred[:, 4] = 2.5                      # constant simulated
    y_true[:, 5], y_pred[:, 5] = 1.0, 2.5   # both constant
    y_pred[:, 6] = y_true[:, 6]             # perfect agreement
    got = rr.metrics.scores(y_true, y_pred)
    want = host_scores(y_true, y_pred)
    check(got, want, what='special columns')
    for j in (0, 1):
        assert all(np.isnan(got[k][j]) for k in SCORES), j
    for j in (2, 3, 4, 5):
        assert np.isnan(got['kge2012'][j]), j
    for j in (2, 3, 4, 5):
        assert np.isnan(got['pearson_r'][j]), j
    assert got['mse'][6] == 0.0 and got['pearson_r'][6] == pytest.approx(1.0, abs=1e-15)
    assert np.isfinite(got['kge2012'][7:]).all()


def test_no_rows_gives_nan():
    res = rr.metrics.Accumulator(3).result()
    assert all(np.isnan(v).all() and v.shape == (3,) for v in res.values())
    res = rr.metrics.scores(np.zeros((0, 4)), np.zeros((0, 4)))
    assert all(np.isnan(v).all() for v in res.values())


@pytest.mark.parametrize('kind', ['numpy', 'torch'])
def test_accumulator_row_blocks_match_one_pass(kind):
    rng = np.random.default_rng(21)
    T, n = 5000, 700
    y_true, y_pred = series(rng, T, n, F64, F32)
    cuts = [0, 1, 32, 65, 1000, 1001, 4096, T]
    if kind == 'torch':
        import torch
        y_true, y_pred = torch.from_numpy(y_true).cuda(), torch.from_numpy(y_pred).cuda()
    acc = rr.metrics.Accumulator(n)
    for a, b in zip(cuts[:-1], cuts[1:]):
        acc.update(y_true[a:b], y_pred[a:b])
    assert acc.rows == T
    chunked, one = acc.result(), rr.metrics.scores(y_true, y_pred)
    if kind == 'torch':
        assert all(v.is_cuda for v in chunked.values())
    check(chunked, {k: numpy_of(v) for k, v in one.items()}, rtol=1e-12, what='row blocks')
    # the same blocks again: bit-identical
    acc2 = rr.metrics.Accumulator(n)
    for a, b in zip(cuts[:-1], cuts[1:]):
        acc2.update(y_true[a:b], y_pred[a:b])
    assert bits(acc2.result()) == bits(chunked)
    check(one, host_scores(numpy_of(y_true), numpy_of(y_pred)), what='one pass')


def test_repeat_calls_bit_identical():
    import torch
    rng = np.random.default_rng(8)
    y_true, y_pred = series(rng, 35040, 1000)
    t, p = torch.from_numpy(y_true).cuda(), torch.from_numpy(y_pred).cuda()
    first = bits(rr.metrics.scores(t, p))
    for _ in range(3):
        assert bits(rr.metrics.scores(t, p)) == first
    assert bits(rr.metrics.scores(y_true, y_pred)) == first


def test_torch_in_torch_out_and_1d():
    import torch
    rng = np.random.default_rng(2)
    y_true, y_pred = series(rng, 300, 1)
    t, p = torch.from_numpy(y_true[:, 0]).cuda(), torch.from_numpy(y_pred[:, 0]).cuda()
    got = rr.metrics.kge2012(t, p)
    assert torch.is_tensor(got) and got.is_cuda and got.shape == (1,)
    want = rr.metrics.kge2012(y_true[:, 0], y_pred[:, 0])
    assert abs(float(got[0]) - want) <= 1e-10 * abs(want)
    res = rr.metrics.scores(t.reshape(-1, 1), y_pred)           # torch and numpy together: device tensors out
    assert all(torch.is_tensor(v) for v in res.values())
    with pytest.raises(ValueError, match='on the GPU'):
        rr.metrics.scores(t.cpu().reshape(-1, 1), y_pred)


def test_abi_refusals():
    L = _lib.lib()
    out = C.c_int64(-1)
    assert L.rr_metrics_work_bytes(-1, 5, C.byref(out)) == _lib.RR_E_INVALID
    assert L.rr_metrics_work_bytes(5, 5, None) == _lib.RR_E_INVALID
    assert L.rr_metrics_work_bytes(5, 0, C.byref(out)) == _lib.RR_OK and out.value == 0
    n, T = 300, 100
    need = engine.metrics_work_bytes(n, T)
    assert need >= engine.METRICS_STATE * n * 8
    t = engine.DeviceBuffer(T * n * 8).upload(np.ones((T, n)))
    state = engine.DeviceBuffer(engine.METRICS_STATE * n * 8).upload(np.zeros(engine.METRICS_STATE * n))
    work = engine.DeviceBuffer(need)
    args = lambda **kw: [kw.get('device', 0), kw.get('n', n), kw.get('rows', T), kw.get('yt', t.address), 0, kw.get('tp', n),
                         kw.get('yp', t.address), 0, kw.get('pp', n), None, kw.get('state', state.address), kw.get('work', work.address),
                         kw.get('wb', need), None]
    assert L.rr_metrics_update_dev(*args()) == _lib.RR_OK
    for bad in (dict(yt=None), dict(yp=None), dict(state=None), dict(work=None), dict(wb=need - 8), dict(tp=n - 1),
                dict(pp=n - 1), dict(n=-1), dict(rows=-2)):
        assert L.rr_metrics_update_dev(*args(**bad)) == _lib.RR_E_INVALID, bad
        assert L.rr_last_error()
    assert L.rr_metrics_update_dev(*args(device=-1)) == _lib.RR_E_NO_DEVICE
    assert L.rr_metrics_finish_dev(0, n, None, work.address, None) == _lib.RR_E_INVALID
    assert L.rr_metrics_finish_dev(0, -1, state.address, work.address, None) == _lib.RR_E_INVALID
    assert L.rr_metrics_finish_dev(0, n, state.address, work.address, None) == _lib.RR_OK
    engine.synchronize(0)
    res = work.download(np.float64, (5, n))
    np.testing.assert_array_equal(res[:3], 0.0)                 # ones against ones: no error, and r / KGE undefined
    assert np.isnan(res[3:]).all()


def test_broadcast_and_overlapping_rows_are_read_as_their_values():
    """Views whose row stride is below their width (broadcast rows, overlapping rows) are scored as the values they show:
    the kernel addresses whole rows, so these are copied into whole rows first and never read with a widened pitch."""
    import torch
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(17)
    T, n = 256, 300
    y_true, _ = series(rng, T, n)
    baseline = rng.integers(1, 40, n) * 0.5                     # 256 copies of each sum exactly: numpy's std is 0 as well
    t = torch.from_numpy(y_true).to(dev)
    b = torch.from_numpy(baseline).to(dev).expand(T, n)
    assert b.stride() == (0, 1)
    got = rr.metrics.scores(t, b)
    check(got, host_scores(y_true, np.broadcast_to(baseline, (T, n))), what='broadcast baseline')
    assert np.isnan(numpy_of(got['kge2012'])).all()             # a constant simulation has no KGE
    base = torch.from_numpy(rng.normal(5.0, 1.0, T + n - 1)).to(dev)
    lagged = base.as_strided((T, n), (1, 1))                    # column c is the series shifted by c steps
    got = rr.metrics.scores(t, lagged)
    check(got, host_scores(y_true, lagged.cpu().numpy()), what='overlapping rows')
    one = torch.tensor(2.5, dtype=torch.float64, device=dev).expand(T)
    got = rr.metrics.scores(t[:, :1].reshape(-1), one)
    check(got, host_scores(y_true[:, :1], np.full((T, 1), 2.5)), what='broadcast 1-D')


def test_result_on_another_stream_follows_the_updates():
    import torch
    rng = np.random.default_rng(29)
    y_true, y_pred = series(rng, 4096, 700)
    t, p = torch.from_numpy(y_true).cuda(), torch.from_numpy(y_pred).cuda()
    side = torch.cuda.Stream()
    acc = rr.metrics.Accumulator(700)
    with torch.cuda.stream(side):
        acc.update(t[:2048], p[:2048])
        acc.update(t[2048:], p[2048:])
    res = acc.result()                                          # on the default stream
    again = rr.metrics.Accumulator(700).update(t[:2048], p[:2048]).update(t[2048:], p[2048:]).result()
    assert bits(res) == bits(again)
