"""Scores of an ensemble's members on the GPU (k_metrics_partial with several members through rr_metrics_update_members_dev, rr.metrics.scores_members,
rr.metrics.MemberAccumulator, Plan.rapid_route_members_scores): member m of a members call equals rr.metrics.scores on member m alone
-- bit for bit wherever members x ceil(G / 256) x ceil(rows / 32) <= 2048, where both calls cut the rows into the same 32-row ranges,
and within the project's row-split tolerance (rtol 1e-12) beyond -- for every dtype pairing, shared and per-member observations,
column maps, gaps, wide pitches, members more than 2^31 elements apart and row blocks; the ABI's refusals; and the routing driver
against the arrays Plan.rapid_route_members returns."""
import ctypes as C
import warnings

import numpy as np
import pytest

import river_route_amd as rr
from oracle import oracle
from river_route_amd import _lib, engine
from river_route_amd.engine import DeviceBuffer, Plan

pytestmark = pytest.mark.gpu

SCORES = rr.metrics.SCORES
F32, F64 = np.float32, np.float64
PAIRS = [(F64, F64), (F32, F32), (F32, F64), (F64, F32)]


def series(rng, T, n):
    """Hydrograph-like observed columns (positive, seasonal, column scales over four decades) and simulations that are scaled, shifted
    and noisy copies of them, some anti-correlated."""
    scale = 10.0 ** rng.uniform(-1, 3, n)
    phase = rng.uniform(0, 2 * np.pi, n)
    tt = np.arange(T)[:, None]
    obs = scale * (2.0 + np.sin(tt * 2 * np.pi / 35040.0 * 4 + phase) + rng.gamma(2.0, 0.3, (T, n)))
    a = rng.uniform(-0.5, 1.5, n)
    sim = a * obs + scale * rng.uniform(-0.5, 0.5, n) + scale * rng.normal(0.0, 0.4, (T, n))
    return obs, sim


def members_case(rng, M, T, G, extra=37):
    """obs (M, T, G); pred (M, T, G + extra) with the simulations of obs's columns at `columns` (unsorted, with repeats among the
    gauges' own columns where G > 2) and unrelated values elsewhere."""
    W = G + extra
    columns = rng.permutation(W)[:G]
    if G > 2:
        columns[G // 2] = columns[0]
    obs = np.empty((M, T, G))
    pred = rng.normal(3.0, 1.0, (M, T, W))
    for m in range(M):
        o, s = series(rng, T, G)
        obs[m] = o
        pred[m][:, columns] = s      # (a repeated column keeps the later simulation: still a fair pair)
    return obs, pred, columns


def numpy_of(v):
    return v.detach().cpu().numpy() if hasattr(v, 'detach') else np.asarray(v)


def bits(res):
    return {k: numpy_of(v).tobytes() for k, v in res.items()}


def member(res, m):
    return {k: numpy_of(v)[m] for k, v in res.items()}


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


def same_cut(M, G, rows):
    """Both calls cut the rows into the same 32-row ranges (metrics_split)."""
    return M * -(-G // 256) * -(-rows // 32) <= 2048


def assert_members_equal_single_calls(y_true, y_pred, columns=None, skip_missing=False, exact=True, what=''):
    """y_true (T, G) shared or (M, T, G); numpy or torch."""
    got = rr.metrics.scores_members(y_true, y_pred, columns=columns, skip_missing=skip_missing)
    M, G = y_pred.shape[0], y_true.shape[-1]
    keys = SCORES + (('count',) if skip_missing else ())
    assert tuple(got) == keys and all(tuple(v.shape) == (M, G) for v in got.values()), what
    for m in range(M):
        t_m = y_true if y_true.ndim == 2 else y_true[m]
        want = rr.metrics.scores(t_m, y_pred[m], columns=columns, skip_missing=skip_missing)
        if exact:
            assert bits(member(got, m)) == bits(want), f'{what}: member {m}'
        else:
            check(member(got, m), {k: numpy_of(v) for k, v in want.items()}, rtol=1e-12, what=f'{what}: member {m}')
            if skip_missing:
                np.testing.assert_array_equal(numpy_of(got['count'])[m], numpy_of(want['count']))
    return got


# ---- 1. against single calls ----

@pytest.mark.parametrize('rows', [1, 31, 32, 33, 100, 1000])
@pytest.mark.parametrize('G', [1, 255, 300])
@pytest.mark.parametrize('M', [1, 3])
def test_members_equal_single_calls_bit_for_bit(M, G, rows):
    assert same_cut(M, G, rows)
    rng = np.random.default_rng(1000 * M + 10 * G + rows)
    obs, pred, columns = members_case(rng, M, rows, G)
    direct = np.ascontiguousarray(pred[:, :, columns])      # the gathered columns: scored without a map
    for dt, dp in PAIRS:
        for shared in (True, False):
            y_true = (obs[0] if shared else obs).astype(dt)
            what = f'M={M} G={G} rows={rows} {dt.__name__}/{dp.__name__} {"shared" if shared else "per member"}'
            mapped = assert_members_equal_single_calls(y_true, pred.astype(dp), columns, what=what + ' mapped')
            plain = assert_members_equal_single_calls(y_true, direct.astype(dp), what=what)
            assert bits(mapped) == bits(plain), what


def test_beyond_the_common_cut_members_equal_single_calls_to_the_row_split_tolerance():
    M, G, rows = 8, 300, 8000
    assert not same_cut(M, G, rows)
    rng = np.random.default_rng(88)
    obs, sim = series(rng, rows, G)
    pred = np.stack([(sim * (1.0 + 0.05 * m) + 0.1 * m).astype(F32) for m in range(M)])
    assert_members_equal_single_calls(obs, pred, exact=False, what='8 x 300 x 8000')


# ---- 2. against the host path ----

def test_every_member_and_column_against_the_host_path():
    M, G, rows = 3, 40, 500
    obs, pred, columns = members_case(np.random.default_rng(7), M, rows, G)
    got = rr.metrics.scores_members(obs, pred, columns=columns)
    assert all(isinstance(v, np.ndarray) and v.dtype == F64 and v.shape == (M, G) for v in got.values())
    for m in range(M):
        check(member(got, m), host_scores(obs[m], pred[m], columns), what=f'host path, member {m}')
    shared = rr.metrics.scores_members(obs[1], pred, columns=columns)
    for m in range(M):
        check(member(shared, m), host_scores(obs[1], pred[m], columns), what=f'host path, shared observations, member {m}')


# ---- 3. skip_missing ----

@pytest.mark.parametrize('shared', [True, False], ids=['shared', 'per_member'])
@pytest.mark.parametrize('dt,dp', PAIRS)
def test_skip_missing(dt, dp, shared):
    M, G, rows = 3, 300, 100
    assert same_cut(M, G, rows)
    rng = np.random.default_rng(31)
    obs, pred, columns = members_case(rng, M, rows, G)
    obs, pred = obs.astype(dt), pred.astype(dp)
    clean_true = obs[0].copy() if shared else obs.copy()
    # gap-free data: the bits of skip_missing=False
    free = rr.metrics.scores_members(clean_true, pred, columns=columns, skip_missing=True)
    plain = rr.metrics.scores_members(clean_true, pred, columns=columns)
    assert bits({k: free[k] for k in SCORES}) == bits(plain)
    assert free['count'].shape == (M, G) and (free['count'] == rows).all()
    # gaps
    y_true = clean_true.copy()
    y_true[rng.random(y_true.shape) < 0.2] = np.nan
    y_true[..., 0] = np.nan                                  # column 0: nothing kept
    y_true[..., 1] = np.nan
    y_true[..., 40, 1] = clean_true[..., 40, 1]              # column 1: one kept pair
    y_true[..., 10, 5], y_true[..., 11, 6] = clean_true[..., 10, 5], np.nan
    bad = pred.copy()
    bad[1, 10, columns[5]] = np.nan                          # member 1, a kept row of column 5: poisons that member's column
    bad[2, 11, columns[6]] = np.nan                          # member 2, a missing row of column 6: never looked at
    others = [j for j in range(G) if columns[j] in (columns[5], columns[6]) and j not in (5, 6)]      # (a repeat of either column)
    assert not others
    got = assert_members_equal_single_calls(y_true, bad, columns, skip_missing=True, what='gaps')
    ref = rr.metrics.scores_members(y_true, pred, columns=columns, skip_missing=True)
    assert got['count'].shape == (M, G)
    assert (got['count'][:, 0] == 0).all() and all(np.isnan(got[k][:, 0]).all() for k in SCORES)
    assert (got['count'][:, 1] == 1).all() and np.isfinite(got['mse'][:, 1]).all() and np.isnan(got['kge2012'][:, 1]).all()
    assert all(np.isnan(got[k][1, 5]) for k in SCORES)
    poisoned = np.zeros((M, G), bool)
    poisoned[1, 5] = True
    for k in SCORES:      # everything but member 1's column 5 is what the clean simulations give, bit for bit
        assert np.array_equal(got[k][~poisoned].view(np.int64), ref[k][~poisoned].view(np.int64)), k
    assert np.isfinite(got['kge2012'][2, 6]) and np.isfinite(got['kge2012'][0, 5]) and np.isfinite(got['kge2012'][2, 5])
    np.testing.assert_array_equal(got['count'], np.broadcast_to((~np.isnan(y_true)).sum(axis=-2), (M, G)))


# ---- 4. wide pitches, read in place ----

def test_wide_pitches_are_read_in_place():
    import torch
    dev = torch.device('cuda', 0)
    M, G, rows, extra = 3, 300, 100, 37
    obs, pred, columns = members_case(np.random.default_rng(41), M, rows, G, extra)
    W = G + extra
    nan = float('nan')
    bp = torch.full((M, rows + 5, W + 11), nan, dtype=torch.float32, device=dev)
    bt = torch.full((M, rows + 9, G + 3), nan, dtype=torch.float64, device=dev)
    vp, vt = bp[:, 2:2 + rows, 3:3 + W], bt[:, 4:4 + rows, 1:1 + G]
    vp.copy_(torch.from_numpy(pred.astype(F32)).to(dev))
    vt.copy_(torch.from_numpy(obs).to(dev))
    assert vp.stride() == ((rows + 5) * (W + 11), W + 11, 1) and vp.stride(0) > rows * vp.stride(1) and not vp.is_contiguous()
    for v in (vp, vt, vt[1]):      # used where they lie
        r = rr.metrics._MemberRows(v, 'view', shared_ok=True)
        assert r.tensor.data_ptr() == v.data_ptr() and r.pitch == v.stride(-2) and r.member_pitch == (v.stride(0) if v.dim() == 3 else 0)
    for y_true in (vt, vt[1]):
        for cols in (columns, None):
            p = vp if cols is not None else vp[:, :, :G]
            got = rr.metrics.scores_members(y_true, p, columns=cols)
            assert all(torch.is_tensor(v) and v.is_cuda and v.dtype == torch.float64 and tuple(v.shape) == (M, G) for v in got.values())
            assert not any(torch.isnan(v).any() for v in got.values())      # a wrong offset would read the NaN fill
            assert bits(got) == bits(rr.metrics.scores_members(y_true.contiguous(), p.contiguous(), columns=cols))
            for m in range(M):
                t_m = y_true if y_true.dim() == 2 else y_true[m]
                assert bits(member(got, m)) == bits(rr.metrics.scores(t_m.contiguous(), p[m].contiguous(), columns=cols))
    # views the kernel's addressing cannot read are copied first: members that share their rows, columns that are not adjacent
    one = vp[0].contiguous()
    got = rr.metrics.scores_members(vt, one.expand(M, rows, W), columns=columns)
    for m in range(M):
        assert bits(member(got, m)) == bits(rr.metrics.scores(vt[m].contiguous(), one, columns=columns))
    tp = vp.contiguous().permute(0, 2, 1).contiguous().permute(0, 2, 1)      # (M, rows, W) with column stride rows
    assert tp.stride(2) != 1
    assert bits(rr.metrics.scores_members(vt, tp, columns=columns)) == bits(rr.metrics.scores_members(vt, vp, columns=columns))


# ---- 5. members more than 2^31 elements apart ----

def test_member_offset_beyond_2_to_the_31():
    import torch
    dev = torch.device('cuda', 0)
    M, rows, G = 2, 40, 300
    member_pitch = (1 << 31) + 4096
    try:
        buf = torch.empty(member_pitch + rows * G, dtype=torch.float32, device=dev)      # about 8.6 GB, never filled
    except RuntimeError as e:      # (torch.cuda.OutOfMemoryError is one)
        pytest.skip(f'cannot allocate {4 * (member_pitch + rows * G) / 1e9:.1f} GB in one block on this device: {e}')
    obs, pred, _ = members_case(np.random.default_rng(53), M, rows, G, extra=0)
    view = buf.as_strided((M, rows, G), (member_pitch, G, 1))
    for m in range(M):      # only the two members' rows are written
        view[m].copy_(torch.from_numpy(pred[m].astype(F32)).to(dev))
    y_true = torch.from_numpy(obs[0]).to(dev)
    r = rr.metrics._MemberRows(view, 'view')
    assert r.tensor.data_ptr() == buf.data_ptr() and r.member_pitch == member_pitch > 1 << 31
    got = rr.metrics.scores_members(y_true, view)
    for m in range(M):
        assert bits(member(got, m)) == bits(rr.metrics.scores(y_true, view[m]))
    assert bits(member(got, 0)) != bits(member(got, 1))
    del view, buf
    torch.cuda.empty_cache()


# ---- 6. row blocks, repeats, streams ----

@pytest.mark.parametrize('kind', ['numpy', 'torch'])
@pytest.mark.parametrize('cuts', [(0, 500, 1000), (0, 33, 640, 1000)], ids=['two', 'three'])
def test_row_blocks_match_one_pass(cuts, kind):
    M, G, rows = 3, 300, 1000
    obs, pred, columns = members_case(np.random.default_rng(61), M, rows, G)
    pred = pred.astype(F32)
    if kind == 'torch':
        import torch
        obs, pred = torch.from_numpy(obs).cuda(), torch.from_numpy(pred).cuda()

    def blocks(skip_missing=False):
        acc = rr.metrics.MemberAccumulator(G, M, columns=columns, skip_missing=skip_missing)
        for a, b in zip(cuts[:-1], cuts[1:]):
            assert acc.update(obs[:, a:b], pred[:, a:b]) is acc
        assert acc.rows == rows
        return acc.result()
    chunked, one = blocks(), rr.metrics.scores_members(obs, pred, columns=columns)
    if kind == 'torch':
        assert all(v.is_cuda for v in chunked.values())
    for m in range(M):
        check(member(chunked, m), member(one, m), rtol=1e-12, what=f'row blocks, member {m}')
    assert bits(blocks()) == bits(chunked)                  # the same blocks again: bit-identical
    assert bits(rr.metrics.scores_members(obs, pred, columns=columns)) == bits(one)
    gaps = blocks(skip_missing=True)                        # gap-free blocks with the rule: the same bits, and every pair counted
    assert bits({k: gaps[k] for k in SCORES}) == bits(chunked) and (numpy_of(gaps['count']) == rows).all()


def test_no_rows_gives_nan():
    res = rr.metrics.MemberAccumulator(3, 2).result()
    assert all(np.isnan(v).all() and v.shape == (2, 3) for v in res.values())
    res = rr.metrics.scores_members(np.zeros((0, 4)), np.zeros((2, 0, 4)), skip_missing=True)
    assert all(np.isnan(res[k]).all() for k in SCORES) and (res['count'] == 0).all()


def test_result_on_another_stream_follows_the_updates():
    import torch
    M, G, rows = 3, 300, 1000
    obs, pred, _ = members_case(np.random.default_rng(67), M, rows, G, extra=0)
    t, p = torch.from_numpy(obs).cuda(), torch.from_numpy(pred).cuda()
    side = torch.cuda.Stream()
    acc = rr.metrics.MemberAccumulator(G, M)
    with torch.cuda.stream(side):
        acc.update(t[:, :512], p[:, :512])
        acc.update(t[:, 512:], p[:, 512:])
    res = acc.result()                                          # on the default stream
    again = rr.metrics.MemberAccumulator(G, M).update(t[:, :512], p[:, :512]).update(t[:, 512:], p[:, 512:]).result()
    assert bits(res) == bits(again)


# ---- 7. the ABI's refusals: each with its code, the state left as it was ----

def test_abi_refusals_leave_the_state_untouched():
    L = _lib.lib()
    n, M, T = 300, 2, 100
    need = engine.metrics_members_work_bytes(n, M, T)
    assert need == 4 * engine.METRICS_STATE * M * n * 8
    rows = DeviceBuffer(M * T * n * 8).upload(np.ones((M, T, n)))
    mark = np.full(engine.METRICS_STATE * M * n, 7.0)
    state = DeviceBuffer(mark.nbytes).upload(mark)
    work = DeviceBuffer(need)

    def args(**kw):
        return [kw.get('device', 0), kw.get('n', n), kw.get('members', M), kw.get('rows', T), kw.get('yt', rows.address), 0, kw.get('tp', n),
                kw.get('tmp', T * n), kw.get('yp', rows.address), 0, kw.get('pp', n), kw.get('pmp', T * n), kw.get('cols', None), 0,
                kw.get('state', state.address), kw.get('work', work.address), kw.get('wb', need), None]
    refused = [dict(yt=None), dict(yp=None), dict(state=None), dict(work=None), dict(wb=need - 8), dict(tp=n - 1), dict(pp=n - 1),
               dict(n=-1), dict(rows=-2), dict(members=0), dict(members=-3), dict(members=(1 << 31) // n + 1),
               dict(pmp=(T - 1) * n + n - 1), dict(pmp=0), dict(tmp=(T - 1) * n + n - 1), dict(tmp=-1),
               dict(pp=n + 5, pmp=(T - 1) * (n + 5) + n - 1), dict(tp=n + 5, tmp=(T - 1) * (n + 5) + n - 1)]
    for bad in refused:
        assert L.rr_metrics_update_members_dev(*args(**bad)) == _lib.RR_E_INVALID, bad
        assert L.rr_last_error()
    assert L.rr_metrics_update_members_dev(*args(device=-1)) == _lib.RR_E_NO_DEVICE
    # with a column map one column is read: a member pitch of (rows - 1) * pitch + 1 passes, one less does not
    cols = DeviceBuffer(n * 4).upload(np.zeros(n, np.int32))
    assert L.rr_metrics_update_members_dev(*args(cols=cols.address, pp=1, pmp=T - 1)) == _lib.RR_E_INVALID
    engine.synchronize(0)
    np.testing.assert_array_equal(state.download(F64, mark.shape), mark)
    # the calls that pass: the shortest member pitches, shared observations, no rows
    state.upload(np.zeros_like(mark))
    assert L.rr_metrics_update_members_dev(*args(rows=0, yt=None, yp=None, work=None, wb=0)) == _lib.RR_OK
    assert L.rr_metrics_update_members_dev(*args(pmp=(T - 1) * n + n, tmp=0)) == _lib.RR_OK
    assert L.rr_metrics_update_members_dev(*args(cols=cols.address, pp=1, pmp=T)) == _lib.RR_OK
    out = DeviceBuffer(5 * M * n * 8)
    assert L.rr_metrics_finish_dev(0, M * n, state.address, out.address, None) == _lib.RR_OK
    engine.synchronize(0)
    res = out.download(F64, (5, M, n))
    np.testing.assert_array_equal(res[:3], 0.0)                 # ones against ones: no error, and r / KGE undefined
    assert np.isnan(res[3:]).all()
    assert (state.download(F64, (M, n)) == 2 * T).all()         # row 0 of the state: the pairs of both updates, per member and column


def test_one_member_gives_the_bits_of_the_single_call_through_the_abi():
    n, T = 300, 1000
    rng = np.random.default_rng(71)
    obs, sim = series(rng, T, n)
    obs[rng.random(obs.shape) < 0.1] = np.nan
    d_t, d_p = DeviceBuffer(obs.nbytes).upload(obs), DeviceBuffer(sim.nbytes).upload(sim)
    assert engine.metrics_members_work_bytes(n, 1, T) == engine.metrics_work_bytes(n, T)
    work = DeviceBuffer(engine.metrics_work_bytes(n, T))
    zeros = np.zeros(engine.METRICS_STATE * n)
    for missing in (False, True):
        a, b = DeviceBuffer(zeros.nbytes).upload(zeros), DeviceBuffer(zeros.nbytes).upload(zeros)
        single = engine.metrics_update_missing_dev if missing else engine.metrics_update_dev
        single(n, T, d_t, False, n, d_p, False, n, None, a, work, work.nbytes)
        engine.metrics_update_members_dev(n, 1, T, d_t, False, n, 0, d_p, False, n, 0, None, missing, b, work, work.nbytes)
        engine.synchronize(0)
        assert a.download(F64, zeros.shape).tobytes() == b.download(F64, zeros.shape).tobytes(), missing


# ---- 8. Plan.rapid_route_members_scores against the arrays Plan.rapid_route_members returns ----

DT, NSUB, T_ROUTE, M_ROUTE, G_ROUTE = 3600.0, 2, 96, 5, 40


def member_sets(k, x, indices, M, nsub, dt=DT):
    """Coefficient set m: the network's k stretched by 15 % and its x shifted by 0.02 per member.  (lhs (M, E), c2, c3, c4 (M, n))"""
    lhs, c2, c3, c4 = [], [], [], []
    for m in range(M):
        a1, a2, a3 = oracle.muskingum_coefficients(k * (1 + 0.15 * m), np.clip(x + 0.02 * m, 0.0, 0.45), dt / nsub)
        lhs.append(-a1[indices]); c2.append(a2); c3.append(a3); c4.append((a1 + a2) / dt)
    return [np.ascontiguousarray(np.stack(a)) for a in (lhs, c2, c3, c4)]


@pytest.fixture(scope='module')
def routed(golden_kernels):
    """tree1k, five coefficient sets, 96 rows x 2 sub-steps: the plan, and per (dtype, shared forcing) the inputs and what
    rapid_route_members returns for them, computed once and left unchanged."""
    g, case = golden_kernels, 'tree1k'
    indptr, indices = g[f'{case}/indptr'].astype(np.int32), g[f'{case}/indices'].astype(np.int32)
    n = len(indptr) - 1
    sets = member_sets(g[f'{case}/k'], g[f'{case}/x'], indices, M_ROUTE, NSUB)
    base = np.ascontiguousarray(np.tile(g[f'{case}/qlateral'], (T_ROUTE // g[f'{case}/qlateral'].shape[0] + 1, 1))[:T_ROUTE])
    base = base * (1.0 + 0.5 * np.sin(np.arange(T_ROUTE) / 7.0))[:, None]      # rows that differ, so that scores are defined
    q0 = np.stack([g[f'{case}/q0'] * (m + 1) for m in range(M_ROUTE)])
    rng = np.random.default_rng(97)
    gauges = rng.choice(n, G_ROUTE, replace=False)
    gauges[17] = gauges[3]                                                    # one reach gauged twice
    plan = Plan(indptr, indices)
    plan.set_member_coeffs(*sets)
    cases = {}
    for dtype, factor in ((F32, 4), (F64, 1)):
        for shared in (True, False):
            ql = base if shared else np.stack([base * (1.0 + 0.1 * m) for m in range(M_ROUTE)])
            out = np.empty((M_ROUTE, T_ROUTE // factor, n), dtype)
            states = plan.rapid_route_members(q0, ql, out, NSUB, factor=factor)
            rows = out.shape[1]
            observed = (out[2][:, gauges].astype(F64) * rng.uniform(0.7, 1.3, G_ROUTE) + rng.normal(0.0, 0.05, (rows, G_ROUTE))).astype(dtype)
            gappy = observed.copy()
            gappy[rng.random(gappy.shape) < 0.15] = np.nan
            for a in (out, states, observed, gappy):
                a.setflags(write=False)
            cases[dtype, shared] = dict(ql=ql, factor=factor, out=out, states=states, observed=observed, gappy=gappy)
    yield dict(plan=plan, q0=q0, gauges=gauges, n=n, cases=cases)
    plan.close()


def assert_scores_of_the_returned_rows(scores, c, gauges, skip, skip_missing):
    observed = c['gappy'] if skip_missing else c['observed']
    assert tuple(scores) == SCORES + (('count',) if skip_missing else ())
    for m in range(M_ROUTE):
        want = rr.metrics.scores(observed[skip:], c['out'][m][skip:], columns=gauges, skip_missing=skip_missing)
        assert bits(member(scores, m)) == bits(want), f'member {m}'
    assert all(isinstance(v, np.ndarray) and v.dtype == F64 and v.shape == (M_ROUTE, G_ROUTE) for v in scores.values())
    assert np.isfinite(scores['kge2012']).mean() > 0.5      # (scores, not NaN against NaN)


@pytest.mark.parametrize('skip_missing', [False, True], ids=['plain', 'gaps'])
@pytest.mark.parametrize('skip', [0, 3])
@pytest.mark.parametrize('shared', [True, False], ids=['shared', 'per_member'])
@pytest.mark.parametrize('dtype', [F32, F64], ids=['f32_factor4', 'f64'])
def test_routed_scores_equal_the_scores_of_the_routed_rows(routed, dtype, shared, skip, skip_missing):
    c, plan = routed['cases'][dtype, shared], routed['plan']
    assert same_cut(M_ROUTE, G_ROUTE, c['out'].shape[1])
    observed = c['gappy'] if skip_missing else c['observed']
    scores, q_final = plan.rapid_route_members_scores(routed['q0'], c['ql'], observed, routed['gauges'], NSUB, factor=c['factor'],
                                                      skip_missing=skip_missing, skip_rows=skip, dtype=dtype)
    assert plan.last_kernel() == 'tile_ensemble'
    assert_scores_of_the_returned_rows(scores, c, routed['gauges'], skip, skip_missing)
    assert q_final.shape == c['states'].shape and np.array_equal(q_final.view(np.int64), c['states'].view(np.int64))


@pytest.mark.parametrize('shared', [True, False], ids=['shared', 'per_member'])
def test_routed_scores_in_groups_without_a_discharge_download(routed, monkeypatch, shared):
    c, plan, n = routed['cases'][F32, shared], routed['plan'], routed['n']
    real, routed_groups, downloads = Plan.reserve_ensemble, [], []
    monkeypatch.setattr(Plan, 'reserve_ensemble', lambda self, members, *a, **kw: dict(real(self, members, *a, **kw), members_max=2))
    real_dev = Plan.rapid_route_members_dev
    monkeypatch.setattr(Plan, 'rapid_route_members_dev', lambda self, members, *a, **kw: (routed_groups.append(members), real_dev(self, members, *a, **kw))[1])
    real_download = DeviceBuffer.download
    monkeypatch.setattr(DeviceBuffer, 'download', lambda self, dtype, shape, offset=0: (downloads.append(tuple(shape)), real_download(self, dtype, shape, offset))[1])
    scores, q_final = plan.rapid_route_members_scores(routed['q0'], c['ql'], c['gappy'], routed['gauges'], NSUB, factor=c['factor'], skip_missing=True,
                                                      skip_rows=3)
    came_back = sorted(set(downloads))
    assert routed_groups == [2, 2, 1]
    assert_scores_of_the_returned_rows(scores, c, routed['gauges'], 3, True)
    assert np.array_equal(q_final.view(np.int64), c['states'].view(np.int64))
    # only scores (5, m, G), counts (m, G) and final states (m, n) came back: never a (m, rows, n) block
    assert came_back == sorted({(5, 2, G_ROUTE), (5, 1, G_ROUTE), (2, G_ROUTE), (1, G_ROUTE), (2, n), (1, n)})
    # and with the downloads counted the existing call still brings its blocks back, the same as before
    downloads.clear()
    out = np.empty(c['out'].shape, F32)
    states = plan.rapid_route_members(routed['q0'], c['ql'], out, NSUB, factor=c['factor'])
    assert (2, c['out'].shape[1], n) in downloads
    assert np.array_equal(out.view(np.int32), c['out'].view(np.int32)) and np.array_equal(states.view(np.int64), c['states'].view(np.int64))


def test_the_existing_members_call_is_unchanged_afterwards(routed):
    plan = routed['plan']
    for (dtype, shared), c in routed['cases'].items():
        out = np.empty(c['out'].shape, dtype)
        states = plan.rapid_route_members(routed['q0'], c['ql'], out, NSUB, factor=c['factor'])
        assert out.tobytes() == c['out'].tobytes() and states.tobytes() == c['states'].tobytes(), (dtype, shared)
