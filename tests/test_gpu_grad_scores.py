"""rr.grad.scores on the GPU (rr_metrics_adjoint_dev: k_metrics_adjoint_coef, k_metrics_adjoint_rows): the forward is
rr.metrics.scores bit for bit; dL/dy_pred agrees with torch autograd through the pure-torch restatement of
tests/test_grad_scores.py (checked there against the reference's values) on the widened float64 data to rtol 1e-9 and
atol 1e-9 x max|want|, the tolerance of tests/test_gpu_grad.py (float32 y_pred: 2^-23 more on rtol, the one rounding of the
store); column maps with repeats; NaN scores; repeat runs bit-identical; gradcheck; route -> score -> backward against the two
restatements chained; and the ABI's refusals.

Inputs are sim = a obs + noise, so r stays away from +-1 and E from 0, and every reference gradient is checked to be finite.
Every shape runs every loss: each score alone, a random weighting of all five, and (1 - kge).mean().  One exception: two rows are
always perfectly correlated, so at T = 2 the derivative of r is 0 and what either side computes for a loss of r alone is its own
rounding, with no max|want| to hold it to; r's share is still in the T = 2 runs of kge2012 alone and of the two mixed losses."""
import numpy as np
import pytest
import torch

import river_route_amd as rr
import test_grad as route_cpu
import test_grad_scores as cpu
from river_route_amd import _lib, engine
from river_route_amd.engine import DeviceBuffer, Plan

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
SCORES = rr.metrics.SCORES
F32, F64 = torch.float32, torch.float64


def series(T, n, seed, m=None):
    """(obs[T, n], sim[T, m or n], columns or None): positive hydrograph-like columns over three decades of scale, simulations
    a obs + noise of the columns they are scored against (other columns of sim: noise of the same kind)."""
    rng = np.random.default_rng(seed)
    scale = 10.0 ** rng.uniform(-1, 2, n)
    obs = scale * (1.0 + rng.gamma(2.0, 0.5, (T, n)))
    a = rng.uniform(0.6, 1.4, n)
    sim = a * obs + scale * rng.uniform(0.05, 0.3, n) + scale * rng.normal(0.0, 0.35, (T, n))
    if m is None:
        return obs, sim, None
    columns = rng.choice(m, n, replace=False)
    wide = 1.0 + rng.gamma(2.0, 0.5, (T, m))
    wide[:, columns] = sim
    return obs, wide, columns


def loss_of(s, G, device):
    return sum((torch.as_tensor(G[k], device=device) * s[name]).sum() for k, name in enumerate(SCORES) if np.any(G[k] != 0))


def gpu_grad(t, p, G, columns=None, dt=F64, dp=F64):
    """(scores, dL/dy_pred) of rr.grad.scores for L = sum G * scores, as numpy."""
    tt = torch.tensor(t, device=DEV, dtype=dt)
    pt = torch.tensor(p, device=DEV, dtype=dp, requires_grad=True)
    s = rr.grad.scores(tt, pt, columns=columns)
    loss_of(s, G, DEV).backward()
    assert pt.grad.dtype == dp and pt.grad.shape == pt.shape
    return {k: v.detach().cpu().numpy() for k, v in s.items()}, pt.grad.cpu().numpy()


def want_grad(t, p, G, columns=None, dt=F64, dp=F64):
    """The same through the restatement on the CPU, on the data as the GPU saw it, widened to float64."""
    tt = torch.tensor(t, dtype=dt).double()
    pt = torch.tensor(p, dtype=dp).double().requires_grad_()
    s = cpu.dense_scores(tt, pt if columns is None else pt[:, torch.as_tensor(np.asarray(columns))])
    loss_of(s, G, 'cpu').backward()
    want = pt.grad.numpy()
    assert np.isfinite(want).all(), 'the reference gradient itself is not finite'
    return want


def assert_grad(got, want, what, f32=False):
    rtol = 1e-9 + (2.0 ** -23 if f32 else 0.0)
    scale = max(float(np.abs(want).max()), 1e-300)
    err = np.abs(got - want)
    print(f'{what}: worst |got - want| / max|want| = {err.max() / scale:.3g}')
    np.testing.assert_allclose(got, want, rtol=rtol, atol=1e-9 * scale, err_msg=what)


# ---- forward ----

@pytest.mark.parametrize('dt,dp', [(F64, F64), (F64, F32), (F32, F64), (F32, F32)])
@pytest.mark.parametrize('mapped', [False, True])
def test_forward_bit_equal_to_metrics_scores(dt, dp, mapped):
    T, n = 700, 300
    obs, sim, columns = series(T, n, seed=3, m=1000 if mapped else None)
    if mapped:
        columns[5] = columns[9]      # a repeat
    t, p = torch.tensor(obs, device=DEV, dtype=dt), torch.tensor(sim, device=DEV, dtype=dp)
    want = rr.metrics.scores(t, p, columns=columns)
    got = rr.grad.scores(t, p.clone().requires_grad_(), columns=columns)
    for k in SCORES:
        assert got[k].dtype == F64 and got[k].shape == (n,) and got[k].requires_grad
        assert torch.equal(got[k].detach(), want[k]), k


def test_forward_and_gradient_of_a_strided_row_view():
    T, n = 130, 70
    obs, sim, _ = series(T, n, seed=4)
    base_t = torch.zeros((T, n + 9), device=DEV, dtype=F64)
    base_t[:, 3:3 + n] = torch.tensor(obs, device=DEV)
    base_p = torch.full((T, 2 * n), 7.0, device=DEV, dtype=F64)
    base_p[:, :n] = torch.tensor(sim, device=DEV)
    base_p.requires_grad_()
    t, p = base_t[:, 3:3 + n], base_p[:, :n]
    assert not p.is_contiguous()
    want = rr.metrics.scores(t, p.detach())
    got = rr.grad.scores(t, p)
    for k in SCORES:
        assert torch.equal(got[k].detach(), want[k]), k
    G = np.random.default_rng(1).standard_normal((5, n))
    loss_of(got, G, DEV).backward()
    g = base_p.grad.cpu().numpy()
    assert not g[:, n:].any()
    assert_grad(g[:, :n], want_grad(obs, sim, G), 'strided rows')
    # one series each
    got = rr.grad.scores(base_t[:, 3], base_p[:, 0])
    want = rr.metrics.scores(base_t[:, 3], base_p[:, 0].detach())
    assert all(torch.equal(got[k].detach(), want[k]) and got[k].shape == (1,) for k in SCORES)


# ---- gradients ----

SHAPES = [(1, 2), (3, 2), (1, 35_040), (2, 3), (7, 33), (256, 64), (257, 100), (300, 3000), (1000, 31), (5000, 300)]


@pytest.mark.parametrize('n,T', SHAPES)
def test_gradients_match_restatement(n, T):
    obs, sim, _ = series(T, n, seed=n + T)
    losses = cpu.weights(n, seed=n)
    if T == 2:
        losses = [l for l in losses if l[0] != 'pearson_r']      # module docstring
    for what, G in losses:
        _, got = gpu_grad(obs, sim, G)
        assert_grad(got, want_grad(obs, sim, G), f'n={n} T={T} {what}')


@pytest.mark.parametrize('dt,dp', [(F64, F32), (F32, F64), (F32, F32)])
def test_gradients_float32_inputs(dt, dp):
    n, T = 130, 500
    obs, sim, _ = series(T, n, seed=8)
    for what, G in cpu.weights(n, seed=2):
        _, got = gpu_grad(obs, sim, G, dt=dt, dp=dp)
        assert_grad(got, want_grad(obs, sim, G, dt=dt, dp=dp), f'{dt} {dp} {what}', f32=dp == F32)


@pytest.mark.parametrize('dp', [F64, F32])
def test_gauge_columns_of_a_wide_array(dp):
    n, m, T = 2000, 100_000, 40
    obs, wide, columns = series(T, n, seed=6, m=m)
    for what, G in cpu.weights(n, seed=3):
        _, got = gpu_grad(obs, wide, G, columns=columns, dp=dp)
        unscored = np.ones(m, dtype=bool)
        unscored[columns] = False
        assert not got[:, unscored].any()
        assert_grad(got, want_grad(obs, wide, G, columns=columns, dp=dp), f'gauges {dp} {what}', f32=dp == F32)


def test_repeated_columns_sum_and_unscored_columns_are_zero():
    T, m = 200, 40
    rng = np.random.default_rng(5)
    columns = np.array([3, 3, 0, 7, 3, 39, 7, 12, 0, 3, 21])
    n = len(columns)
    wide = 2.0 + rng.gamma(2.0, 0.5, (T, m))
    obs = wide[:, columns] * rng.uniform(0.7, 1.3, n) + rng.normal(0.0, 0.3, (T, n))
    for what, G in cpu.weights(n, seed=4):
        _, got = gpu_grad(obs, wide, G, columns=columns)
        unscored = np.setdiff1d(np.arange(m), columns)
        assert not got[:, unscored].any() and (got[:, np.unique(columns)] != 0).any(0).all()
        assert_grad(got, want_grad(obs, wide, G, columns=columns), f'repeats {what}')
    # the same through a tensor of columns on the device and an odd number of rows left over after the batches
    _, a = gpu_grad(obs[:37], wide[:37], G, columns=torch.tensor(columns, device=DEV))
    assert_grad(a, want_grad(obs[:37], wide[:37], G, columns=columns), 'repeats, 37 rows')


def test_constant_column_nan_rules():
    T, n = 90, 5
    obs, sim, _ = series(T, n, seed=11)
    sim[:, 1] = 2.5
    G = np.zeros((5, n))
    G[2] = np.random.default_rng(0).uniform(0.5, 2.0, n)
    s, got = gpu_grad(obs, sim, G)
    assert np.isnan(s['pearson_r'][1]) and np.isnan(s['kge2012'][1])
    assert np.isfinite(got).all()
    assert_grad(got, want_grad(obs, sim, G), 'constant column under mse')
    for k in (3, 4):
        G = np.zeros((5, n))
        G[k] = 1.0
        _, got = gpu_grad(obs, sim, G)
        tt, pt = torch.tensor(obs), torch.tensor(sim, requires_grad=True)
        cpu.dense_scores(tt, pt)[SCORES[k]].sum().backward()
        want = pt.grad.numpy()
        assert np.array_equal(np.isfinite(got), np.isfinite(want)), SCORES[k]
        assert not np.isfinite(got[:, 1]).any() and np.isfinite(got[:, [0, 2, 3, 4]]).all()
        assert_grad(got[:, [0, 2, 3, 4]], want[:, [0, 2, 3, 4]], f'beside a NaN column: {SCORES[k]}')


def test_two_backward_passes_bit_identical():
    obs, wide, columns = series(300, 700, seed=14, m=5000)
    columns[10:20] = columns[30]
    G = np.random.default_rng(2).standard_normal((5, 700))
    for cols, p in ((None, wide[:, :700]), (columns, wide)):
        a, b = gpu_grad(obs, p, G, columns=cols), gpu_grad(obs, p, G, columns=cols)
        assert np.array_equal(a[1], b[1]) and all(np.array_equal(a[0][k], b[0][k]) for k in SCORES)
    # one graph, two passes
    pt = torch.tensor(wide, device=DEV, requires_grad=True)
    loss = loss_of(rr.grad.scores(torch.tensor(obs, device=DEV), pt, columns=columns), G, DEV)
    g1, = torch.autograd.grad(loss, pt, retain_graph=True)
    g2, = torch.autograd.grad(loss, pt)
    assert torch.equal(g1, g2)


def test_gradcheck():
    obs, wide, columns = series(12, 4, seed=3, m=6)
    columns[3] = columns[0]
    t = torch.tensor(obs, device=DEV)

    def f(p):
        return tuple(rr.grad.scores(t, p, columns=columns).values())

    assert torch.autograd.gradcheck(f, (torch.tensor(wide, device=DEV, requires_grad=True),), eps=1e-6, atol=1e-6, rtol=1e-5)
    assert torch.autograd.gradcheck(lambda p: tuple(rr.grad.scores(t, p).values()),
                                    (torch.tensor(wide[:, :4], device=DEV, requires_grad=True),), eps=1e-6, atol=1e-6, rtol=1e-5)


def test_route_score_backward_end_to_end():
    n, T, nsub, dt_runoff, n_gauges = 2000, 24, 1, 3600.0, 60
    dt = dt_runoff / nsub
    down, k, x = route_cpu.network('tree', n, seed=7)
    rng = np.random.default_rng(8)
    ql = rng.uniform(0.2, 2.0, (T, n)) * 3600.0 * (1.0 + np.sin(np.arange(T) / 4.0))[:, None]
    q0 = rng.uniform(0.5, 3.0, n)
    gauges = np.sort(rng.choice(n, n_gauges, replace=False))
    truth, _ = route_cpu.oracle_route(down, q0, ql, k * rng.uniform(0.7, 1.3, n), x, dt, dt_runoff)
    obs = truth[:, gauges] * rng.uniform(0.8, 1.2, n_gauges) * (1.0 + rng.normal(0.0, 0.2, (T, n_gauges)))

    indptr, indices = route_cpu.csc_from_down(down)
    plan = Plan(indptr, indices)
    kt, xt = torch.tensor(k, requires_grad=True), torch.tensor(x, requires_grad=True)
    Q, _ = rr.grad.rapid_route(plan, torch.tensor(q0, device=DEV), torch.tensor(ql, device=DEV), kt, xt, dt, dt_runoff)
    kge = rr.grad.scores(torch.tensor(obs, device=DEV), Q, columns=gauges)['kge2012']
    (1.0 - kge).mean().backward()

    kw, xw = torch.tensor(k, requires_grad=True), torch.tensor(x, requires_grad=True)
    c1, c2, c3 = rr.grad.muskingum_coefficients(kw, xw, dt)
    Qw, _ = route_cpu.dense_route(down, torch.tensor(q0), torch.tensor(ql), c1, c2, c3, (c1 + c2) / dt_runoff, nsub)
    kge_w = cpu.dense_scores(torch.tensor(obs), Qw[:, torch.as_tensor(gauges)])['kge2012']
    (1.0 - kge_w).mean().backward()
    assert np.isfinite(kw.grad.numpy()).all() and np.isfinite(xw.grad.numpy()).all() and kw.grad.abs().max() > 0
    np.testing.assert_allclose(kge.detach().cpu().numpy(), kge_w.detach().numpy(), rtol=1e-9)
    for got, want, what in ((kt.grad, kw.grad, 'k'), (xt.grad, xw.grad, 'x')):
        assert_grad(got.numpy(), want.numpy(), f'route -> kge -> backward: d/d{what}')


# ---- the raw ABI ----

def test_abi_refusals():
    n, T = 40, 16
    buf = lambda count: DeviceBuffer(max(count, 1) * 8)     # noqa: E731
    yt, yp, grad, state, g = buf(T * n), buf(T * n), buf(T * n), buf(9 * n), buf(5 * n)
    maps = DeviceBuffer(4 * (3 * n + 1))
    need = engine.metrics_adjoint_work_bytes(n)
    assert need == 6 * 8 * n and engine.metrics_adjoint_work_bytes(0) == 0
    work = DeviceBuffer(need)

    def code(*args):
        with pytest.raises(_lib.RRError) as e:
            engine.metrics_adjoint_dev(*args)
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
    assert c == _lib.RR_E_INVALID and str(need) in msg
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
    with pytest.raises(_lib.RRError) as e:
        _lib.check(_lib.lib().rr_metrics_adjoint_work_bytes(n, None))
    assert e.value.code == _lib.RR_E_INVALID
    assert code(*ok, 99)[0] == _lib.RR_E_NO_DEVICE
    engine.metrics_adjoint_dev(*but(rows=0))      # nothing to do
    # accepted as it stands: an all-zero state scores no rows, so the call only has to run
    for b in (yt, yp, state, g):
        b.upload(np.zeros(b.nbytes // 8))
    engine.metrics_adjoint_dev(*ok)
    _lib.lib().rr_dev_synchronize(0)
