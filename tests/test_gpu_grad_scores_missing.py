"""rr.grad.scores(..., skip_missing=True) on the GPU (rr_metrics_update_missing_dev forward, rr_metrics_adjoint_missing_dev backward:
k_metrics_adjoint_coef as it is, then k_metrics_adjoint_rows<MISSING>): the forward is rr.metrics.scores(..., skip_missing=True)
bit for bit, 'count' included; dL/dy_pred agrees with torch autograd on the CPU through the masked float64 restatement
(missing_helpers.dense_scores_missing: torch.where on the mask, N = mask.sum(0)) within the assert_grad of
tests/test_gpu_grad_scores.py, and is exactly 0.0 at every skipped element.  Every shape carries the gap pattern of
missing_helpers.gap_mask and runs every loss of test_grad_scores.weights.

Which columns are compared: a column that keeps fewer than two pairs (pattern column 4, one pair; column 5, none; and at T = 2
column 2, whose row 0 is the pivot row the pattern removes) has no r and no KGE, and the reference gradient of a loss that
weights either is NaN there by 0 / 0.  Such columns are compared under the losses of me, mae and mse alone, and left out of the
comparison (their skipped elements are still held to exactly 0) under a loss that weights r or the KGE.  As in
tests/test_gpu_grad_scores.py, two rows are always perfectly correlated, so a loss of r alone is not run at T = 2.  The reference
gradient is asserted finite everywhere it is compared."""
import numpy as np
import pytest
import torch

import river_route_amd as rr
import test_grad as route_cpu
import test_grad_scores as cpu
from missing_helpers import dense_scores_missing, gap_mask, with_gaps
from river_route_amd import _lib, engine
from river_route_amd.engine import DeviceBuffer, Plan
from test_gpu_grad_scores import DEV, assert_grad, loss_of, series

pytestmark = pytest.mark.gpu
SCORES = rr.metrics.SCORES
F32, F64 = torch.float32, torch.float64


def gappy(T, n, seed, m=None):
    obs, sim, columns = series(T, n, seed, m=m)
    return with_gaps(obs, gap_mask(T, n, seed=seed + 1)), sim, columns


def gpu_grad(t, p, G, columns=None, dt=F64, dp=F64, skip_missing=True):
    """(scores with 'count', dL/dy_pred) of rr.grad.scores for L = sum G * scores, as numpy."""
    tt = torch.tensor(t, device=DEV, dtype=dt)
    pt = torch.tensor(p, device=DEV, dtype=dp, requires_grad=True)
    s = rr.grad.scores(tt, pt, columns=columns, skip_missing=skip_missing)
    loss_of(s, G, DEV).backward()
    assert pt.grad.dtype == dp and pt.grad.shape == pt.shape
    return {k: v.detach().cpu().numpy() for k, v in s.items()}, pt.grad.cpu().numpy()


def want_grad(t, p, G, columns=None, dt=F64, dp=F64):
    """The same through the masked restatement on the CPU, on the data as the GPU saw it, widened to float64."""
    tt = torch.tensor(t, dtype=dt).double()
    pt = torch.tensor(p, dtype=dp).double().requires_grad_()
    s = dense_scores_missing(tt, pt if columns is None else pt[:, torch.as_tensor(np.asarray(columns))])
    loss_of(s, G, 'cpu').backward()
    return pt.grad.numpy()


def compared_columns(t, G):
    """Columns of y_true whose reference gradient is defined under G (module docstring)."""
    kept = (~np.isnan(t)).sum(0)
    return np.ones(t.shape[1], dtype=bool) if not (G[3].any() or G[4].any()) else kept >= 2


def skipped_are_zero(got, t, what):
    miss = np.isnan(t)
    assert not np.isnan(got[miss]).any() and (got[miss] == 0.0).all(), f'{what}: a skipped element is not exactly 0'


def compare(got, want, cols, what, f32=False):
    assert np.isfinite(want[:, cols]).all(), f'{what}: the reference gradient itself is not finite'
    assert_grad(got[:, cols], want[:, cols], what, f32=f32)


# ---- forward ----

@pytest.mark.parametrize('dt,dp', [(F64, F64), (F64, F32), (F32, F64), (F32, F32)])
@pytest.mark.parametrize('mapped', [False, True])
def test_forward_bit_equal_to_metrics_scores(dt, dp, mapped):
    T, n = 700, 300
    obs, sim, columns = gappy(T, n, seed=3, m=1000 if mapped else None)
    if mapped:
        columns[5] = columns[9]      # a repeat
    t, p = torch.tensor(obs, device=DEV, dtype=dt), torch.tensor(sim, device=DEV, dtype=dp)
    want = rr.metrics.scores(t, p, columns=columns, skip_missing=True)
    got = rr.grad.scores(t, p.clone().requires_grad_(), columns=columns, skip_missing=True)
    assert set(got) == set(SCORES) | {'count'} and set(rr.grad.scores(t, p.clone().requires_grad_(), columns=columns)) == set(SCORES)
    for k in SCORES:
        assert got[k].dtype == F64 and got[k].shape == (n,) and got[k].requires_grad
        assert torch.equal(got[k].detach().nan_to_num(nan=-7.0), want[k].nan_to_num(nan=-7.0)), k
        assert torch.equal(got[k].isnan(), want[k].isnan()), k
    assert not got['count'].requires_grad and got['count'].grad_fn is None and got['count'].dtype == F64
    assert torch.equal(got['count'], want['count'])
    np.testing.assert_array_equal(got['count'].cpu().numpy(), (~np.isnan(obs)).sum(0))


# ---- gradients ----

SHAPES = [(3, 2), (7, 33), (256, 64), (257, 100), (7, 3000), (300, 700)]


@pytest.mark.parametrize('n,T', SHAPES)
def test_gradients_match_masked_restatement(n, T):
    obs, sim, _ = gappy(T, n, seed=n + T)
    losses = cpu.weights(n, seed=n)
    if T == 2:
        losses = [l for l in losses if l[0] != 'pearson_r']      # module docstring
    for what, G in losses:
        _, got = gpu_grad(obs, sim, G)
        skipped_are_zero(got, obs, what)
        compare(got, want_grad(obs, sim, G), compared_columns(obs, G), f'n={n} T={T} {what}')
        if n > 5:
            assert not got[:, 5].any()      # nothing kept: zeros, whatever the loss


@pytest.mark.parametrize('dt,dp', [(F64, F32), (F32, F64), (F32, F32)])
def test_gradients_float32_inputs(dt, dp):
    n, T = 130, 500
    obs, sim, _ = gappy(T, n, seed=8)
    for what, G in cpu.weights(n, seed=2):
        _, got = gpu_grad(obs, sim, G, dt=dt, dp=dp)
        skipped_are_zero(got, obs, what)
        compare(got, want_grad(obs, sim, G, dt=dt, dp=dp), compared_columns(obs, G), f'{dt} {dp} {what}', f32=dp == F32)


def test_gauge_columns_of_a_wide_array_with_repeats():
    T, m = 200, 40
    rng = np.random.default_rng(5)
    columns = np.array([3, 3, 0, 7, 12, 39, 7, 21, 0, 3, 3])      # pattern columns 4 and 5 have columns 12 and 39 to themselves
    n = len(columns)
    wide = 2.0 + rng.gamma(2.0, 0.5, (T, m))
    obs = with_gaps(wide[:, columns] * rng.uniform(0.7, 1.3, n) + rng.normal(0.0, 0.3, (T, n)), gap_mask(T, n, seed=6))
    miss = np.isnan(obs)
    unscored = np.setdiff1d(np.arange(m), columns)
    for what, G in cpu.weights(n, seed=4):
        _, got = gpu_grad(obs, wide, G, columns=columns)
        assert not got[:, unscored].any()
        pred_cols = np.zeros(m, dtype=bool)
        pred_cols[columns[compared_columns(obs, G)]] = True
        compare(got, want_grad(obs, wide, G, columns=columns), pred_cols, f'repeats {what}')
        # a row where every share of a column is skipped: exactly 0
        for c in np.unique(columns):
            rows = miss[:, columns == c].all(1)
            assert (got[rows, c] == 0.0).all(), (what, c)
    # column 3 of y_pred is scored by y_true columns 0 (gap-free) and 1 (rows 32..127 missing), 9 and 10 (random gaps): with only the
    # first two weighted, rows 32..127 get column 0's share alone, bit for bit what scoring column 0 by itself gives there
    G = np.zeros((5, n))
    G[:, :2] = np.random.default_rng(7).standard_normal((5, 2))
    _, both = gpu_grad(obs, wide, G, columns=columns)
    _, alone = gpu_grad(obs[:, :1], wide, G[:, :1], columns=columns[:1])
    assert np.array_equal(both[32:128, 3], alone[32:128, 3]) and alone[32:128, 3].all()
    assert not np.array_equal(both[:32, 3], alone[:32, 3])
    # the same through a tensor of columns on the device and an odd number of rows left over after the batches
    _, a = gpu_grad(obs[:37], wide[:37], G, columns=torch.tensor(columns, device=DEV))
    pred_cols = np.zeros(m, dtype=bool)
    pred_cols[columns[compared_columns(obs[:37], G)]] = True
    compare(a, want_grad(obs[:37], wide[:37], G, columns=columns), pred_cols, 'repeats, 37 rows')
    assert (a[32:37, 3] == gpu_grad(obs[:37, :1], wide[:37], G[:, :1], columns=columns[:1])[1][32:37, 3]).all()


def test_nan_rules_hold_at_the_kept_rows():
    """One pair kept: finite under me / mae / mse, and under r or the KGE NaN at the kept row only.  A NaN simulated at a skipped
    element changes no bit of the gradient elsewhere and gets 0 itself."""
    T, n = 90, 8
    obs, sim, _ = gappy(T, n, seed=11)
    for k in range(5):
        G = np.zeros((5, n))
        G[k] = 1.0
        _, got = gpu_grad(obs, sim, G)
        skipped_are_zero(got, obs, SCORES[k])
        assert np.isnan(got[5, 4]) == (k >= 3) and np.isfinite(np.delete(got, 4, axis=1)).all(), SCORES[k]
        poisoned = sim.copy()
        poisoned[np.isnan(obs)] = np.nan
        _, again = gpu_grad(obs, poisoned, G)
        assert np.array_equal(got, again, equal_nan=True), SCORES[k]


def test_gap_free_gradient_equals_the_unmasked_gradient():
    n, T = 257, 100
    obs, sim, _ = series(T, n, seed=n + T)
    for what, G in cpu.weights(n, seed=n):
        s, got = gpu_grad(obs, sim, G)
        _, plain = gpu_grad(obs, sim, G, skip_missing=False)
        np.testing.assert_array_equal(s['count'], float(T))
        print(f'gap-free {what}: gradient bits equal to the unmasked path: {np.array_equal(got, plain)}')
        assert np.isfinite(plain).all()
        assert_grad(got, plain, f'gap-free {what}')


def test_two_backward_passes_bit_identical():
    obs, wide, columns = gappy(300, 700, seed=14, m=5000)
    columns[10:20] = columns[30]
    G = np.random.default_rng(2).standard_normal((5, 700))
    for cols, p in ((None, wide[:, :700]), (columns, wide)):
        a, b = gpu_grad(obs, p, G, columns=cols), gpu_grad(obs, p, G, columns=cols)
        assert np.array_equal(a[1], b[1], equal_nan=True) and all(np.array_equal(a[0][k], b[0][k], equal_nan=True) for k in a[0])
    # one graph, two passes
    pt = torch.tensor(wide, device=DEV, requires_grad=True)
    loss = loss_of(rr.grad.scores(torch.tensor(obs, device=DEV), pt, columns=columns, skip_missing=True), G, DEV)
    g1, = torch.autograd.grad(loss, pt, retain_graph=True)
    g2, = torch.autograd.grad(loss, pt)
    assert torch.equal(g1.isnan(), g2.isnan()) and torch.equal(g1.nan_to_num(nan=0.0), g2.nan_to_num(nan=0.0))


def test_gradcheck():
    T, n = 9, 4
    obs, wide, columns = series(T, n, seed=3, m=6)
    obs = with_gaps(obs, gap_mask(T, n, seed=4))
    obs[4, 1] = np.nan                                  # the pattern leaves column 1 gap-free at nine rows
    assert np.isnan(obs).sum(0).tolist() == [0, 1, 1, 1]
    columns[3] = columns[0]
    t = torch.tensor(obs, device=DEV)

    def f(p, cols=None):
        s = rr.grad.scores(t, p, columns=cols, skip_missing=True)
        return tuple(s[k] for k in SCORES)

    assert torch.autograd.gradcheck(lambda p: f(p, columns), (torch.tensor(wide, device=DEV, requires_grad=True),), eps=1e-6, atol=1e-6, rtol=1e-5)
    assert torch.autograd.gradcheck(f, (torch.tensor(wide[:, :4], device=DEV, requires_grad=True),), eps=1e-6, atol=1e-6, rtol=1e-5)


def test_route_score_backward_end_to_end():
    """rapid_route(gauges=) -> scores(skip_missing=True) -> the mean of 1 - KGE over the gauges with count >= 2 -> backward(), on the
    network of tests/test_gpu_grad_scores.py::test_route_score_backward_end_to_end with a gappy observation tensor."""
    n, T, nsub, dt_runoff, n_gauges = 2000, 24, 1, 3600.0, 60
    dt = dt_runoff / nsub
    down, k, x = route_cpu.network('tree', n, seed=7)
    rng = np.random.default_rng(8)
    ql = rng.uniform(0.2, 2.0, (T, n)) * 3600.0 * (1.0 + np.sin(np.arange(T) / 4.0))[:, None]
    q0 = rng.uniform(0.5, 3.0, n)
    gauges = np.sort(rng.choice(n, n_gauges, replace=False))
    truth, _ = route_cpu.oracle_route(down, q0, ql, k * rng.uniform(0.7, 1.3, n), x, dt, dt_runoff)
    obs = truth[:, gauges] * rng.uniform(0.8, 1.2, n_gauges) * (1.0 + rng.normal(0.0, 0.2, (T, n_gauges)))
    obs = with_gaps(obs, gap_mask(T, n_gauges, seed=9))
    usable = (~np.isnan(obs)).sum(0) >= 2
    assert not usable[4] and not usable[5] and usable.sum() >= n_gauges - 4

    indptr, indices = route_cpu.csc_from_down(down)
    plan = Plan(indptr, indices)
    kt, xt = torch.tensor(k, requires_grad=True), torch.tensor(x, requires_grad=True)
    Qg, _ = rr.grad.rapid_route(plan, torch.tensor(q0, device=DEV), torch.tensor(ql, device=DEV), kt, xt, dt, dt_runoff, gauges=gauges)
    assert Qg.shape == (T, n_gauges)
    s = rr.grad.scores(torch.tensor(obs, device=DEV), Qg, skip_missing=True)
    ok = s['count'] >= 2
    assert ok.cpu().numpy().tolist() == usable.tolist()
    kge = s['kge2012'][ok]
    (1.0 - kge).mean().backward()

    kw, xw = torch.tensor(k, requires_grad=True), torch.tensor(x, requires_grad=True)
    c1, c2, c3 = rr.grad.muskingum_coefficients(kw, xw, dt)
    Qw, _ = route_cpu.dense_route(down, torch.tensor(q0), torch.tensor(ql), c1, c2, c3, (c1 + c2) / dt_runoff, nsub)
    kge_w = dense_scores_missing(torch.tensor(obs[:, usable]), Qw[:, torch.as_tensor(gauges[usable])])['kge2012']
    (1.0 - kge_w).mean().backward()
    assert np.isfinite(kt.grad.numpy()).all() and np.isfinite(xt.grad.numpy()).all() and kt.grad.abs().max() > 0
    assert np.isfinite(kw.grad.numpy()).all() and np.isfinite(xw.grad.numpy()).all()
    np.testing.assert_allclose(kge.detach().cpu().numpy(), kge_w.detach().numpy(), rtol=1e-9)
    for got, want, what in ((kt.grad, kw.grad, 'k'), (xt.grad, xw.grad, 'x')):
        assert_grad(got.numpy(), want.numpy(), f'route -> kge over gauges with count >= 2 -> backward: d/d{what}')


# ---- the raw ABI ----

def test_abi_refusals():
    n, T = 40, 16
    buf = lambda count: DeviceBuffer(max(count, 1) * 8)     # noqa: E731
    yt, yp, grad, state, g = buf(T * n), buf(T * n), buf(T * n), buf(9 * n), buf(5 * n)
    maps = DeviceBuffer(4 * (3 * n + 1))
    need = engine.metrics_adjoint_work_bytes(n)
    work = DeviceBuffer(need)

    def code(*args):
        with pytest.raises(_lib.RRError) as e:
            engine.metrics_adjoint_missing_dev(*args)
        return e.value.code, e.value.message

    ok = [n, T, yt, False, n, yp, False, n, state, g, n, None, None, None, grad, n, work, need]

    def but(**kw):
        names = ('n', 'rows', 'y_true', 'true_is_f32', 'true_pitch', 'y_pred', 'pred_is_f32', 'pred_pitch', 'state', 'grad_scores',
                 'n_distinct', 'order', 'distinct_columns', 'segments', 'grad_pred', 'grad_pitch', 'work', 'work_bytes')
        args = dict(zip(names, ok))
        args.update(kw)
        return [args[k] for k in names]

    for name in ('y_true', 'y_pred', 'state', 'grad_scores', 'grad_pred'):
        assert code(*but(**{name: None}))[0] == _lib.RR_E_INVALID, name
    c, msg = code(*but(work=None, work_bytes=0))
    assert c == _lib.RR_E_INVALID and str(need) in msg and 'rr_metrics_adjoint_missing_dev' in msg
    assert code(*but(work_bytes=need - 8))[0] == _lib.RR_E_INVALID
    assert code(*but(true_pitch=n - 1))[0] == _lib.RR_E_INVALID
    assert code(*but(pred_pitch=n - 1))[0] == _lib.RR_E_INVALID
    assert code(*but(grad_pitch=n - 1))[0] == _lib.RR_E_INVALID
    assert code(*but(n_distinct=n - 1))[0] == _lib.RR_E_INVALID                      # no map: every column is its own
    assert code(*but(order=maps))[0] == _lib.RR_E_INVALID                            # a map comes whole
    assert code(*but(order=maps, distinct_columns=maps, segments=maps, n_distinct=n + 1))[0] == _lib.RR_E_INVALID
    assert code(*but(order=maps, distinct_columns=maps, segments=maps, n_distinct=0))[0] == _lib.RR_E_INVALID
    assert code(*but(rows=-1))[0] == _lib.RR_E_INVALID
    assert code(*but(n=-1))[0] == _lib.RR_E_INVALID
    assert code(*ok, 99)[0] == _lib.RR_E_NO_DEVICE
    engine.metrics_adjoint_missing_dev(*but(rows=0))      # nothing to do
    # accepted as it stands: y_true all NaN and an all-zero state, so every element of grad is written as 0
    yt.upload(np.full(T * n, np.nan))
    for b in (yp, state, g):
        b.upload(np.zeros(b.nbytes // 8))
    grad.upload(np.full(T * n, 7.0))
    engine.metrics_adjoint_missing_dev(*ok)
    _lib.lib().rr_dev_synchronize(0)
    assert not grad.download(np.float64, (T, n)).any()
