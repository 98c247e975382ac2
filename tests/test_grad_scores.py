"""rr.grad.scores without a GPU: the pure-torch dense restatement of the five scores that the GPU test differentiates
(dense_scores: against the reference-generated values of tests/golden/metrics.npz), the closed form of dL/dy_pred that the
kernels evaluate (closed_form_grad, DESIGN.md section 12c: against autograd through the restatement), and every argument check
of rr.grad.scores.

The restatement against the golden values: tests/test_metrics.py holds the host path, the reference's own numpy calls, to the
reference's bits.  A restatement in torch cannot repeat numpy's order of summation (pairwise blocks in np.mean, a BLAS product
in np.corrcoef), so it is held to what a different order of summation of T float64 terms can move a score by, 4 T 2^-53 of the
sum of the terms' magnitudes (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2: (T - 1) u for any order,
twice for two orders, twice again for the two moments a ratio combines): relative for mae and mse, whose terms have one sign,
times mae for me, and absolute for pearson_r and kge2012, which are built from ratios of such sums.  For the longest golden
series, T = 730, that is 3.3e-13.  NaN scores must be NaN."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import river_route_amd as rr

SCORES = rr.metrics.SCORES
CASES = ('correlated', 'correlated_weak', 'negative', 'perfect', 'zero_true', 'const_true_1', 'const_pred_2.5', 'const_both',
         'one_nan', 'T1', 'T2')
U = 2.0 ** -53


def dense_scores(t, p):
    """The five scores of every column of t[T, n] against p[T, n] (float64 torch tensors) as rr_metrics_finish_dev defines them
    (river_route/metrics.py): two-pass centred moments, r clipped to [-1, 1], standard deviations with ddof 0, the reference's
    gamma = (mean_pred / std_pred) / (mean_true / std_true).  A column whose r or KGE the reference leaves undefined (zero
    variance, zero mean of y_true) comes out NaN through 0 / 0, and so does its gradient."""
    N = t.shape[0]
    d = t - p
    mt, mp = t.mean(0), p.mean(0)
    a, b = t - mt, p - mp
    m2t, m2p, c = (a * a).sum(0), (b * b).sum(0), (a * b).sum(0)
    r = (c / m2t.sqrt() / m2p.sqrt()).clamp(-1.0, 1.0)
    st, sp = (m2t / N).sqrt(), (m2p / N).sqrt()
    beta, gamma = mp / mt, (mp / sp) / (mt / st)
    kge = 1.0 - ((r - 1.0) ** 2 + (beta - 1.0) ** 2 + (gamma - 1.0) ** 2).sqrt()
    undefined = (st == 0) | (sp == 0) | (mt == 0)
    kge = kge + torch.where(undefined, torch.full_like(kge, float('nan')), torch.zeros_like(kge))
    return {'me': d.mean(0), 'mae': d.abs().mean(0), 'mse': (d * d).mean(0), 'pearson_r': r, 'kge2012': kge}


def closed_form_grad(t, p, G, coefficients=False, dtype=np.float64):
    """dL/dp[T, n] in numpy from G[5, n] = dL/d(me, mae, mse, pearson_r, kge2012): what k_metrics_adjoint_coef and
    k_metrics_adjoint_rows compute, from two-pass moments.  coefficients: (A, B, P, S, mt, mp) instead.
    dtype: the precision of every operation (np.longdouble: the arbiter of test_offset_series_against_extended_precision)."""
    t, p, G = (np.asarray(v, dtype=dtype) for v in (t, p, G))
    N = t.shape[0]
    mt, mp = t.mean(0), p.mean(0)
    a, b = t - mt, p - mp
    m2t, m2p, c = (a * a).sum(0), (b * b).sum(0), (a * b).sum(0)
    g_me, g_mae, g_mse, g_r, g_kge = G
    with np.errstate(all='ignore'):
        r_raw = c / np.sqrt(m2t) / np.sqrt(m2p)
        inside = ~((r_raw > 1.0) | (r_raw < -1.0))
        r = np.clip(r_raw, -1.0, 1.0)
        r_B = np.where(inside, 1.0 / (np.sqrt(m2t) * np.sqrt(m2p)), 0.0)
        r_P = np.where(inside, -r_raw / m2p, 0.0)
        st, sp = np.sqrt(m2t / N), np.sqrt(m2p / N)
        beta, gamma = mp / mt, (mp / sp) / (mt / st)
        E = np.sqrt((r - 1.0) ** 2 + (beta - 1.0) ** 2 + (gamma - 1.0) ** 2)
        gamma_P, gamma_A, beta_A = -(st / mt) * mp / (N * sp ** 3), (st / mt) / (N * sp), 1.0 / (N * mt)
        zero = np.zeros_like(mt)
        # a score whose gradient is exactly 0 adds nothing, whatever its value
        B = -2.0 * g_mse / N + np.where(g_r != 0, g_r * r_B, zero) + np.where(g_kge != 0, -g_kge * (r - 1.0) * r_B / E, zero)
        P = 2.0 * g_mse / N + np.where(g_r != 0, g_r * r_P, zero) + np.where(g_kge != 0, -g_kge * ((r - 1.0) * r_P + (gamma - 1.0) * gamma_P) / E, zero)
        A = -g_me / N - (2.0 * g_mse / N) * (mt - mp) + np.where(g_kge != 0, -g_kge * ((beta - 1.0) * beta_A + (gamma - 1.0) * gamma_A) / E, zero)
        A = np.where((g_r != 0) & ~((m2t > 0) & (m2p > 0)), np.nan, A)
        A = np.where((g_kge != 0) & ((st == 0) | (sp == 0) | (mt == 0)), np.nan, A)
        S = -g_mae / N
        if coefficients:
            return A, B, P, S, mt, mp
        return A + B * a + P * b + S * np.sign(t - p)


def autograd_grad(t, p, G):
    """dL/dp for L = sum_k sum_j G[k, j] score_k[j] by autograd through the restatement; rows of G that are all zero stay out of
    the loss, as a score nobody uses stays out of the graph."""
    pt = torch.tensor(np.asarray(p, dtype=np.float64), requires_grad=True)
    s = dense_scores(torch.tensor(np.asarray(t, dtype=np.float64)), pt)
    loss = sum((torch.tensor(G[k]) * s[name]).sum() for k, name in enumerate(SCORES) if np.any(G[k] != 0))
    loss.backward()
    return pt.grad.numpy()


def series(kind, T, n, seed):
    rng = np.random.default_rng(seed)
    obs = 2.0 + rng.gamma(2.0, 0.5, (T, n))
    if kind == 'offset':
        obs = 1e6 + 50.0 * obs
    slope = rng.uniform(-1.2, -0.4, n) if kind == 'negative' else rng.uniform(0.5, 1.5, n)
    sim = slope * obs + rng.uniform(0.1, 0.5, n) + rng.normal(0.0, 0.3, (T, n))
    if kind == 'negative':
        sim = sim + 1.5 * obs.mean(0)
    return obs, sim


def weights(n, seed):
    """One G per loss: each score alone, a random weighting of all five, and (1 - kge).mean()."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(5):
        G = np.zeros((5, n))
        G[k] = rng.uniform(0.5, 2.0, n) * rng.choice([-1.0, 1.0], n)
        out.append((SCORES[k], G))
    out.append(('all five', rng.standard_normal((5, n))))
    G = np.zeros((5, n))
    G[4] = -1.0 / n
    out.append(('(1 - kge).mean()', G))
    return out


@pytest.mark.parametrize('case', CASES)
def test_restatement_reproduces_the_reference(case):
    golden = np.load(os.path.join(GOLDEN, 'metrics.npz'))
    y_true, y_pred = golden[f'{case}/y_true'], golden[f'{case}/y_pred']
    T = y_true.shape[0]
    got = {k: float(v[0]) for k, v in dense_scores(torch.tensor(y_true).reshape(-1, 1), torch.tensor(y_pred).reshape(-1, 1)).items()}
    want = {k: float(golden[f'{case}/{k}']) for k in SCORES}
    bound = 4 * T * U
    for k in SCORES:
        print(f'{case} {k}: got {got[k]!r} want {want[k]!r} bound {bound:.3g}')
    for k in SCORES:
        if np.isnan(want[k]):
            assert np.isnan(got[k]), f'{case} {k}: want NaN, got {got[k]}'
            continue
        scale = {'me': abs(want['mae']), 'mae': abs(want['mae']), 'mse': abs(want['mse']), 'pearson_r': 1.0, 'kge2012': 1.0}[k]
        assert abs(got[k] - want[k]) <= bound * scale, f'{case} {k}: got {got[k]!r}, want {want[k]!r}'


@pytest.mark.parametrize('kind,T,n', [('random', 50, 7), ('random', 400, 3), ('offset', 300, 5), ('negative', 200, 6)])
def test_closed_form_equals_autograd(kind, T, n):
    t, p = series(kind, T, n, seed=T + n)
    if kind == 'negative':
        assert (dense_scores(torch.tensor(t), torch.tensor(p))['pearson_r'] < -0.3).all()
    # rtol 1e-10 of every element.  The offset series alone gets an absolute term, for the float64 means the closed form centres on
    # (test_offset_series_against_extended_precision has the reasoning and the arbiter): 21 u (|B mt| + |P mp|) per column, which
    # must stay below 1e-5 of the column's largest gradient
    for what, G in weights(n, seed=T):
        want = autograd_grad(t, p, G)
        assert np.isfinite(want).all(), what
        got = closed_form_grad(t, p, G)
        atol = 0.0
        if kind == 'offset':
            _, B, P, _, mt, mp = closed_form_grad(t, p, G, coefficients=True)
            atol = 21 * U * (np.abs(B * mt) + np.abs(P * mp))
            assert (atol <= 1e-5 * np.abs(want).max(0)).all()
        print(f'{kind} {what}: worst |got - want| / max|want| = {np.abs(got - want).max() / np.abs(want).max():.3g}')
        assert (np.abs(got - want) <= 1e-10 * np.abs(want) + atol).all(), f'{kind}: {what}'


def test_offset_series_against_extended_precision():
    """Which side of test_closed_form_equals_autograd's offset case is the accurate one: the closed form again in np.longdouble
    (64-bit mantissa on x86) is the arbiter, and it is autograd.  Its graph differentiates the moments as computed, so the rounding
    of its means cancels to second order (it is the closer of the two to the arbiter in every loss, asserted below), while the closed
    form centres on means that float64 cannot hold closer than u |mean| and that reach every element of a column through B and P as
    one constant.  numpy sums 300 same-signed terms in blocks of 128 with eight running sums each: a term passes at most 16
    additions in its running sum, 3 that join the eight and 2 that join the blocks, so a mean is within 21 u |mean|, and the closed
    form is held to rtol 1e-10 plus 21 u (|B mt| + |P mp|).  For r, where B (t - mt) and P (p - mp) nearly cancel, that constant
    is up to 1e-9 of the column's largest gradient at offset 1e6 and standard deviation 35: the price of a closed form on
    float64 means, inside the 1e-9 x max|want| the GPU path is held to."""
    T, n = 300, 5
    t, p = series('offset', T, n, seed=T + n)
    for what, G in weights(n, seed=T):
        exact = np.asarray(closed_form_grad(t, p, G, dtype=np.longdouble), dtype=np.float64)
        got, auto = closed_form_grad(t, p, G), autograd_grad(t, p, G)
        _, B, P, _, mt, mp = closed_form_grad(t, p, G, coefficients=True)
        err, err_auto = np.abs(got - exact), np.abs(auto - exact)
        scale = np.abs(exact).max()
        print(f'offset {what}: closed form {err.max() / scale:.3g}, autograd {err_auto.max() / scale:.3g} of max|exact|')
        assert (err <= 1e-10 * np.abs(exact) + 21 * U * (np.abs(B * mt) + np.abs(P * mp))).all(), what
        assert err_auto.max() <= err.max() + 1e-14 * scale, what


def test_closed_form_with_r_clipped():
    """Two rows are perfectly correlated, and rounding leaves these two columns' unclipped r at +-1.0000000000000002: r passes no
    gradient, in its own score and inside the KGE (torch.clamp's rule), while beta and gamma still do."""
    t = np.array([[1.0 + 1.0 / 7.0], [2.0 + 5.0 / 3.0]]) * np.ones((1, 2))
    p = np.stack([1.5 * t[:, 0] + 0.3, -0.7 * t[:, 1] + 9.0], axis=1)
    a, b = t - t.mean(0), p - p.mean(0)
    r_raw = (a * b).sum(0) / np.sqrt((a * a).sum(0)) / np.sqrt((b * b).sum(0))
    assert r_raw[0] > 1.0 and r_raw[1] < -1.0
    assert dense_scores(torch.tensor(t), torch.tensor(p))['pearson_r'].tolist() == [1.0, -1.0]
    for what, G in weights(2, seed=1):
        want = autograd_grad(t, p, G)
        assert np.isfinite(want).all(), what
        np.testing.assert_allclose(closed_form_grad(t, p, G), want, rtol=1e-10, atol=0.0, err_msg=what)
    G = np.zeros((5, 2))
    G[3] = 1.0
    assert not closed_form_grad(t, p, G).any()


def test_constant_column_gradients():
    """A constant simulated column: finite under an mse-only loss, NaN (that column only) as soon as r or the KGE counts."""
    t, p = series('random', 40, 3, seed=2)
    p[:, 1] = 2.5
    G = np.zeros((5, 3))
    G[2] = 1.0
    got, want = closed_form_grad(t, p, G), autograd_grad(t, p, G)
    assert np.isfinite(want).all()
    np.testing.assert_allclose(got, want, rtol=1e-10, atol=0.0)
    for k in (3, 4):
        G = np.zeros((5, 3))
        G[k] = 1.0
        got, want = closed_form_grad(t, p, G), autograd_grad(t, p, G)
        assert np.array_equal(np.isfinite(got), np.isfinite(want))
        assert not np.isfinite(got[:, 1]).any() and np.isfinite(got[:, [0, 2]]).all()


def test_public_names():
    assert 'scores' in rr.grad.__all__ and 'Scores' in rr.grad.__all__
    assert issubclass(rr.grad.Scores, torch.autograd.Function)


def test_argument_checks_need_no_gpu():
    T, n, m = 6, 3, 5
    t, p = torch.ones(T, n, dtype=torch.float64), torch.ones(T, n, dtype=torch.float64, requires_grad=True)
    wide = torch.ones(T, m, dtype=torch.float64)
    S = rr.grad.scores
    with pytest.raises(TypeError, match='y_true must be a torch tensor'):
        S(t.numpy(), p)
    with pytest.raises(TypeError, match='y_pred must be a torch tensor'):
        S(t, p.detach().numpy())
    with pytest.raises(TypeError, match='float32 or float64'):
        S(t.to(torch.int64), p)
    with pytest.raises(TypeError, match='float32 or float64'):
        S(t, p.detach().to(torch.float16))
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
    with pytest.raises(ValueError, match='1-D integer array of length 3'):
        S(t, wide, columns=[0.0, 1.0, 2.0])
    with pytest.raises(ValueError, match='refers to column 5 of y_pred, which has 5 columns'):
        S(t, wide, columns=[0, 5, 1])
    with pytest.raises(ValueError, match='refers to column -1'):
        S(t, wide, columns=np.array([0, -1, 1]))
    # everything else in order: the device comes last
    with pytest.raises(ValueError, match='y_true must be on the GPU'):
        S(t, p)
    with pytest.raises(ValueError, match='y_true must be on the GPU'):
        S(t, wide, columns=[4, 4, 0])
    with pytest.raises(ValueError, match='y_true must be on the GPU'):
        S(t[:, 0], p[:, 0])
