"""The per-column rule of the skill scores and their gradient without a GPU (tests/per_column.py): the arbiter
(oracle/rr_oracle_scores.c) against the reference's values and against exact rational arithmetic, every regime's named property,
the sanity of the rule's unit, the measurement that the committed constants come from, and the rule biting: four wrong variants of
the kernels' algorithm that the existing checks (rtol 1e-10 on series() data; atol 1e-9 x max|want| over a whole gradient) let pass."""
import math
import os
from fractions import Fraction

import numpy as np
import pytest

from conftest import GOLDEN
import missing_helpers
import per_column as pc
import test_gpu_grad_scores as old_grad
import test_gpu_metrics as old_scores
import test_grad_scores as cpu
from oracle import oracle

SCORES, U = pc.SCORES, pc.U
GOLDEN_CASES = cpu.CASES
MEASURE_SHAPES = ((2000, False), (300, False), (2000, True), (300, True), (33, False), (33, True), (100, True))      # (T, gaps) the constants are measured on


def regime_array(T, gaps=False, regimes=pc.REGIMES, repeats=3):
    """One array holding every regime (x gap pattern) `repeats` times."""
    n = len(regimes) * (len(pc.GAPS) if gaps else repeats)
    return pc.arrays(T, n, gaps, regimes)[0]


# ------------------------------------------------------------------------------------------------ the arbiter

def test_arbiter_against_the_reference_values():
    """The arbiter against what the reference itself returned (tests/golden/metrics.npz, which rr.metrics' host path repeats bit for
    bit): the NaN patterns agree, and the difference -- E_host of these cases -- is within what numpy's float64 sums of T terms can
    err by, 4 T u of a score's scale (the bound of tests/test_grad_scores.py, Higham section 4.2), not within a picked number."""
    golden = np.load(os.path.join(GOLDEN, 'metrics.npz'))
    worst = 0.0
    for case in GOLDEN_CASES:
        t, p = golden[f'{case}/y_true'].reshape(-1, 1), golden[f'{case}/y_pred'].reshape(-1, 1)
        arb = oracle.scores_ld(t, p)
        want = {k: np.array([float(golden[f'{case}/{k}'])]) for k in SCORES}
        for k in SCORES:
            assert np.isnan(want[k][0]) == np.isnan(arb[k][0]), f'{case} {k}: reference {want[k][0]}, arbiter {arb[k][0]}'
        err = pc.score_errors(want, arb)
        e = max(float(err[k][0]) for k in SCORES)
        print(f'{case}: E_host = {e / U:.2f} u (T = {t.shape[0]}, allowed {4 * t.shape[0]} u)')
        assert e <= 4 * t.shape[0] * U, case
        worst = max(worst, e)
        assert arb['count'][0] == t.shape[0]
    assert worst <= 1e-12


def _exact_column(t, p):
    """me, mae, mse, r^2 with r's sign, both means of one column in exact rational arithmetic, each rounded to double once."""
    ft, fp = [Fraction(float(v)) for v in t], [Fraction(float(v)) for v in p]
    N = len(ft)
    d = [a - b for a, b in zip(ft, fp)]
    mt, mp = sum(ft) / N, sum(fp) / N
    m2t, m2p = sum((a - mt) ** 2 for a in ft), sum((b - mp) ** 2 for b in fp)
    c = sum((a - mt) * (b - mp) for a, b in zip(ft, fp))
    r = math.copysign(math.sqrt(float(c * c / (m2t * m2p))), float(c)) if m2t > 0 and m2p > 0 else math.nan
    return {'me': float(sum(d) / N), 'mae': float(sum(abs(v) for v in d) / N), 'mse': float(sum(v * v for v in d) / N), 'pearson_r': r,
            'mt': float(mt), 'mp': float(mp), 'std_t': math.sqrt(float(m2t / N)), 'std_p': math.sqrt(float(m2p / N))}


@pytest.mark.parametrize('gaps', [False, True])
def test_arbiter_sums_against_exact_arithmetic(gaps):
    """One column per regime (with gaps: a different gap pattern each): the arbiter's means against math.fsum, and its me, mae, mse, r
    and standard deviations against exact rationals -- within 2 u of the value (me: of mae), the roundings of forming the two doubles
    compared (the square root of r^2 among them)."""
    T = 300
    arr = regime_array(T, gaps)
    arb = oracle.scores_ld(arr.t, arr.p, None, gaps)
    for i, regime in enumerate(pc.REGIMES):
        j = (i % 5 if gaps else 0) * len(pc.REGIMES) + i      # the first five gap patterns keep at least two pairs
        assert arr.regimes[j] == regime and arr.gaps[j] == (pc.GAPS[i % 5] if gaps else 'none')
        keep = ~np.isnan(arr.t[:, j])
        t, p = arr.t[keep, j], arr.p[keep, j]
        assert abs(math.fsum(t) / len(t) - arb['mt'][j]) <= 2 * U * abs(arb['mt'][j]), regime
        assert abs(math.fsum(p) / len(p) - arb['mp'][j]) <= 2 * U * abs(arb['mp'][j]), regime
        ex = _exact_column(t, p)
        assert abs(ex['me'] - arb['me'][j]) <= 2 * U * ex['mae'], regime
        for k in ('mae', 'mse', 'mt', 'mp'):
            assert abs(ex[k] - arb[k][j]) <= 2 * U * abs(ex[k]), f'{regime} {k}'
        if math.isnan(ex['pearson_r']):
            assert np.isnan(arb['pearson_r'][j]) and np.isnan(arb['r_raw'][j]), regime
        else:
            assert abs(ex['pearson_r'] - arb['r_raw'][j]) <= 2 * U, f"{regime}: r {ex['pearson_r']!r} against {arb['r_raw'][j]!r}"
            for k, s in (('kappa_t', abs(ex['mt']) / ex['std_t']), ('kappa_p', abs(ex['mp']) / ex['std_p'])):
                assert abs(s - arb[k][j]) <= 4 * U * s, f'{regime} {k}'


def test_arbiter_gradient_is_the_derivative_of_its_scores():
    """The gradient arbiter against central differences of the scores arbiter (both long double inside): a closed form that dropped or
    mis-signed a term would show at 1e-6 of an element's scale; repeated columns add, and skipped elements are exactly 0."""
    T, n = 9, 4
    rng = np.random.default_rng(3)
    t = 2.0 + rng.gamma(2.0, 0.5, (T, n))
    p = np.concatenate([0.8 * t + 0.3 + rng.normal(0, 0.3, (T, n)), 2.0 + rng.gamma(2.0, 0.5, (T, 2))], axis=1)
    cols = np.array([0, 5, 2, 0])
    t[2, 1] = t[5, 3] = np.nan
    G = rng.standard_normal((5, n))
    a = oracle.scores_grad_ld(t, p, G, cols, True)

    def loss(q):
        s = oracle.scores_ld(t, q, cols, True)
        return sum(float((G[k] * s[name]).sum()) for k, name in enumerate(SCORES))

    for r in range(T):
        for c in range(p.shape[1]):
            h = 1e-6 * max(abs(p[r, c]), 1.0)
            up, dn = p.copy(), p.copy()
            up[r, c] += h
            dn[r, c] -= h
            fd = (loss(up) - loss(dn)) / (2 * h)
            assert abs(fd - a.grad[r, c]) <= 1e-6 * max(a.scale[r, c], 1e-300) + 1e-9, (r, c, fd, a.grad[r, c])
    assert not a.grad[:, [1, 3, 4]].any() and not a.scale[:, [1, 3, 4]].any()      # unscored columns
    assert a.grad[2, 5] == 0.0 and a.scale[2, 5] == 0.0                            # the only share of (2, 5) is skipped
    assert a.grad[5, 0] != 0.0                                                      # column 0 keeps its other share at row 5


# ------------------------------------------------------------------------------------------------ the regimes

@pytest.mark.parametrize('T', [300, 2000])
def test_every_regime_has_its_named_property(T):
    """Each regime's property, from the arbiter's outputs alone."""
    arr = regime_array(T, repeats=12)
    arb = oracle.scores_ld(arr.t, arr.p)
    cols = {regime: [j for j, r in enumerate(arr.regimes) if r == regime] for regime in pc.REGIMES}
    assert all(len(v) == 12 for v in cols.values())
    finite = lambda k, j: np.isfinite(arb[k][j]).all()      # noqa: E731
    j = cols['benign']
    assert ((arb['kappa_t'][j] > 1) & (arb['kappa_t'][j] < 30)).all() and finite('kge2012', j)
    for regime in pc.OFFSET_REGIMES:
        j, want = cols[regime], math.log10(float(regime.split()[1]))
        for k in ('kappa_t', 'kappa_p'):
            assert (np.abs(np.log10(arb[k][j]) - want) <= 0.5).all(), f'{regime} {k}: {arb[k][j]}'
    j = cols['twenty decades']
    decades = np.log10(np.abs(arb['mt'][j]))
    assert decades.min() >= -13 and decades.max() <= 9 and decades.max() - decades.min() >= 12, decades
    j = cols['near-perfect']
    assert arb['mse'][j[0]] == 0.0 and arb['mae'][j[0]] == 0.0 and arb['pearson_r'][j[0]] == 1.0 and arb['kge2012'][j[0]] == 1.0
    rel = np.sqrt(arb['mse'][j[1:]]) / np.abs(arb['mt'][j[1:]])
    assert ((rel > 1e-10) & (rel < 1e-8)).all() and (arb['pearson_r'][j[1:]] >= 1.0 - 2 * U).all()
    assert (arb['pearson_r'][cols['anti-correlated']] < -0.99).all()
    j = cols['spike pivots']
    rest = arr.t[:, j].copy()
    rest[0::pc.CHUNK] = np.nan
    quiet = oracle.scores_ld(rest, arr.p[:, j], None, True)
    sigma = np.abs(quiet['mt']) / quiet['kappa_t']
    assert ((arr.t[0::pc.CHUNK, j] - quiet['mt']) >= 0.999e6 * sigma).all()
    j = cols['step']
    half = oracle.scores_ld(arr.t[:T // 2, j], arr.p[:T // 2, j])
    whole_std, half_std = np.abs(arb['mt'][j]) / arb['kappa_t'][j], np.abs(half['mt']) / half['kappa_t']
    assert (whole_std >= 30 * half_std).all()      # a jump of 100 sigma: the two halves' means carry the variance
    for regime in ('constant true', 'constant pred', 'all-zero true'):
        j = cols[regime]
        assert np.isnan(arb['pearson_r'][j]).all() and np.isnan(arb['kge2012'][j]).all(), regime
        assert finite('me', j) and finite('mae', j) and finite('mse', j), regime
    assert (arb['mt'][cols['all-zero true']] == 0.0).all() and (arb['mt'][cols['constant true']] != 0.0).all()
    j = cols['chunk-constant']
    assert finite('pearson_r', j) and finite('kge2012', j)
    for q in range(0, T - pc.CHUNK + 1, pc.CHUNK * 3):
        inside = oracle.scores_ld(arr.t[q:q + pc.CHUNK, j], arr.p[q:q + pc.CHUNK, j])
        assert np.isnan(inside['pearson_r']).all() and (inside['count'] == pc.CHUNK).all()
    # no column has a mean that is zero by cancellation: mean_true is 0 in the all-zero columns only
    assert (np.flatnonzero(arb['mt'] == 0.0) == np.array(cols['all-zero true'])).all()


@pytest.mark.parametrize('T,gaps', MEASURE_SHAPES + ((2, False), (1, False)))
def test_the_unit_is_sane(T, gaps):
    """E_host, the reference implementation's own error that the rule is stated in, is a rounding error on every regime: at most
    1e-12 (measured: 2 to 34 u; the chunk-constant columns' np.corrcoef carries the 16 to 34)."""
    arr = regime_array(T, gaps)
    ref = pc.ScoreRef(arr.t, arr.p, None, gaps, arr.regimes)
    err = pc.score_errors(ref.host, ref.arb)
    for regime in pc.REGIMES:
        j = [i for i, r in enumerate(arr.regimes) if r == regime]
        print(f'T {T} gaps {gaps} {regime}: ' + ', '.join(f'{k} {err[k][j].max() / U:.1f} u' for k in SCORES))
    assert ref.e_host <= 1e-12
    # the host path has a value wherever the arbiter has one; the other way round only on the documented divergence (DESIGN.md section
    # 9): an exactly constant series, whose numpy standard deviation can come out a rounding above zero
    for k in SCORES:
        for j in np.flatnonzero(np.isnan(ref.host[k]) != np.isnan(ref.arb[k])):
            keep = ~np.isnan(arr.t[:, j])
            assert np.isnan(ref.arb[k][j]) and (np.ptp(arr.t[keep, j]) == 0 or np.ptp(arr.p[keep, j]) == 0), (k, j, arr.regimes[j])
    assert np.array_equal(ref.host['count'], ref.arb['count'])


# ------------------------------------------------------------------------------------------------ the constants

def _pow2_with_margin(worst):
    return 2.0 ** math.ceil(math.log2(4.0 * worst))


@pytest.fixture(scope='module')
def measured():
    """The restatement over every regime, configuration and measurement shape: the worst ratios the constants come from."""
    c_worst, mean_worst, score_runs, grad_runs = 0.0, 0.0, [], []
    small = [shape for shape in pc.GPU_SHAPES if shape[0] <= 100]
    cases = [(T, gaps, regime_array(T, gaps), [regime_array(T, gaps, group) for group in (pc.GRAD_MODERATE, pc.GRAD_OFFSET)])
             for T, gaps in MEASURE_SHAPES]
    # and the very arrays of the GPU file's small shapes, whose few columns make E_host and E_auto small
    for T, n in small:
        for gaps in (False, True):
            garrs = [g for group in (pc.GRAD_MODERATE, pc.GRAD_OFFSET) for g in pc.arrays(T, n, gaps, group)] if (T, n) in pc.GRAD_SHAPES else []
            for a, arr in enumerate(pc.arrays(T, n, gaps)):
                cases.append((T, gaps, arr, garrs if a == 0 else []))
    for T, gaps, arr, garrs in cases:
        ref = pc.ScoreRef(arr.t, arr.p, None, gaps, arr.regimes)
        off = np.array([r in pc.OFFSET_REGIMES for r in arr.regimes]) & (arr.T >= 300)
        grefs = [[(what, G, pc.GradRef(g.t, g.p, G, None, gaps)) for what, G in cpu.weights(g.n, seed=T)] for g in garrs]
        for cfg in pc.CONFIGS:
            state = pc.restatement(arr.t, arr.p, *cfg, skip=gaps)
            got = pc.finish(state)
            for k in SCORES:
                assert np.array_equal(np.isnan(got[k]), np.isnan(ref.arb[k])), (T, gaps, cfg, k)
            assert np.array_equal(got['count'], ref.arb['count'])
            err = pc.score_errors(got, ref.arb)
            with np.errstate(invalid='ignore', divide='ignore'):
                for k in ('pearson_r', 'kge2012'):
                    c_worst = max(c_worst, float(np.nanmax(err[k][off] / (U * ref.kappa[off]), initial=0.0)))
                for a, b in ((state['mt'], ref.arb['mt']), (state['mp'], ref.arb['mp'])):
                    mean_worst = max(mean_worst, float(np.nanmax(np.abs(a - b)[off] / (U * np.abs(b[off])), initial=0.0)))
            score_runs.append((T, gaps, cfg, got, ref))
            for g, refs in zip(garrs, grefs):
                gstate = pc.restatement(g.t, g.p, *cfg, skip=gaps)
                for what, G, gref in refs:
                    grad_runs.append((T, gaps, cfg, what, g, pc.restatement_grad(gstate, g.t, g.p, G, gaps), gref))
    c = _pow2_with_margin(c_worst)
    c_m = _pow2_with_margin(mean_worst)
    by_regime, k_worst = {}, 0.0
    for T, gaps, cfg, got, ref in score_runs:
        ratios = pc.score_ratios(got, ref, c)
        for k in SCORES:
            for j, regime in enumerate(ref.regimes):
                by_regime[regime] = max(by_regime.get(regime, 0.0), float(ratios[k][j]))
        k_worst = max(k_worst, max(float(ratios[k].max()) for k in SCORES))
    grad_by_regime, kg_worst, e_auto = {}, 0.0, {}
    for T, gaps, cfg, what, g, got, gref in grad_runs:
        assert np.array_equal(np.isnan(got), np.isnan(gref.exact)), (T, gaps, cfg, what)
        ratio = pc.grad_ratio(got, gref, c_m)
        for j, regime in enumerate(g.regimes):
            grad_by_regime[regime] = max(grad_by_regime.get(regime, 0.0), float(ratio[:, j].max()))
        kg_worst = max(kg_worst, float(ratio.max()))
        e_auto[what] = max(e_auto.get(what, 0.0), gref.e_auto)
    print(f'c: worst r / kge error over the offset regimes {c_worst:.3g} u (kappa_t + kappa_p) S -> C_KAPPA = {c:g}')
    print(f'c_m: worst error of a mean over the offset regimes {mean_worst:.3g} u |mean| -> C_MEAN = {c_m:g}')
    print(f'K: worst ratio {k_worst:.3g} -> K = {_pow2_with_margin(k_worst):g}; per regime: ' + ', '.join(f'{r} {v:.2f}' for r, v in by_regime.items()))
    print(f'K_GRAD: worst ratio {kg_worst:.3g} -> K_GRAD = {_pow2_with_margin(kg_worst):g}; per regime: '
          + ', '.join(f'{r} {v:.2f}' for r, v in grad_by_regime.items()))
    print('E_auto per loss: ' + ', '.join(f'{w} {v / U:.3g} u' for w, v in e_auto.items()))
    return {'c': c, 'c_m': c_m, 'K': _pow2_with_margin(k_worst), 'K_GRAD': _pow2_with_margin(kg_worst)}


def test_constants_are_the_measured_ones(measured):
    """K, C_KAPPA, K_GRAD and C_MEAN of tests/per_column.py are the worst ratios of the restatement (chunks of 8, 32 and 64 rows; row
    splits of 32, 96 and all rows; both fold orders; every regime; with and without gaps; T = 33 to 2,000, and the arrays of the GPU
    file's shapes up to 100 rows) times 4, rounded up to a power of two -- the margin for a correctly rounded kernel that fuses its
    multiply-adds and folds in another order."""
    assert (pc.C_KAPPA, pc.C_MEAN, pc.K, pc.K_GRAD) == (measured['c'], measured['c_m'], measured['K'], measured['K_GRAD'])


@pytest.mark.parametrize('T,n', list(pc.GPU_SHAPES))
def test_the_restatement_passes_the_rule_on_the_gpu_arrays(T, n):
    """The arrays tests/test_gpu_scores_per_column.py runs, through the restatement cut as metrics_split cuts them: whatever that file
    finds beyond this is the kernels' own."""
    splits, rps = pc.metrics_splits(n, T)
    assert splits == pc.GPU_SHAPES[(T, n)]
    worst = 0.0
    for gaps in (False, True):
        for a, arr in enumerate(pc.arrays(T, n, gaps)):
            ref = pc.ScoreRef(arr.t, arr.p, None, gaps, arr.regimes)
            got = pc.finish(pc.restatement(arr.t, arr.p, rows_per_split=rps, skip=gaps))
            worst = max(worst, max(pc.assert_per_column(got, ref, f'{T}x{n} array {a} gaps {gaps}').values()))
    print(f'{T}x{n}: worst ratio {worst:.2f} of {pc.K:g}')
    for group in (pc.GRAD_MODERATE, pc.GRAD_OFFSET) if (T, n) in pc.GRAD_SHAPES else ():
        for gaps in (False, True):
            for a, arr in enumerate(pc.arrays(T, n, gaps, group)):
                state = pc.restatement(arr.t, arr.p, rows_per_split=rps, skip=gaps)
                for what, G in cpu.weights(n, seed=T):
                    ref = pc.GradRef(arr.t, arr.p, G, None, gaps)
                    pc.assert_grad_per_element(pc.restatement_grad(state, arr.t, arr.p, G, gaps), ref, f'{T}x{n} array {a} gaps {gaps} {what}')


# ------------------------------------------------------------------------------------------------ the rule bites

def _old_check_passes(variant, skip):
    """check() of tests/test_gpu_metrics.py at rtol 1e-10 on series() data, as the existing GPU tests apply it (with gaps: the mask and
    the reference of tests/missing_helpers.py, as tests/test_gpu_metrics_missing.py applies it)."""
    T, n = 35040, 16
    t, p = old_scores.series(np.random.default_rng(T * 7 + n), T, n)
    if skip:
        t = missing_helpers.with_gaps(t, missing_helpers.gap_mask(T, n, seed=5))
        want = missing_helpers.host_scores_kept(t, p)
    else:
        want = old_scores.host_scores(t, p)
    got = pc.finish(pc.restatement(t, p, rows_per_split=96, skip=skip, variant=variant))
    old_scores.check(got, want, what=str(variant))
    if skip:
        assert np.array_equal(got['count'], want['count'])


@pytest.mark.parametrize('variant,skip', [('unshifted', False), ('pivot row 0', True), ('float32 mean', False)])
def test_the_rule_catches_what_the_old_check_lets_pass(variant, skip):
    """Three wrong kernels: sums without a pivot; a MISSING pivot taken only when the chunk's first row is kept; one chunk's means
    rounded through float32.  Each passes today's check on today's data and fails the per-column rule on the regimes; the
    restatement as it stands passes both."""
    _old_check_passes(None, skip)
    _old_check_passes(variant, skip)
    T = 2000
    arr = regime_array(T, skip)
    ref = pc.ScoreRef(arr.t, arr.p, None, skip, arr.regimes)
    splits, rps = pc.metrics_splits(arr.n, T)
    pc.assert_per_column(pc.finish(pc.restatement(arr.t, arr.p, rows_per_split=rps, skip=skip)), ref, 'the restatement')
    wrong = pc.finish(pc.restatement(arr.t, arr.p, rows_per_split=rps, skip=skip, variant=variant))
    ratios = pc.score_ratios(wrong, ref)
    worst = {k: float(ratios[k].max()) for k in SCORES}
    k = max(worst, key=worst.get)
    j = int(np.argmax(ratios[k]))
    print(f'{variant}: worst {k} in column {j} ({arr.regimes[j]}, gaps: {arr.gaps[j]}), {worst[k] / pc.K:.3g} x the allowance')
    assert worst[k] > 100 * pc.K
    with pytest.raises(AssertionError, match='allowance'):
        pc.assert_per_column(wrong, ref, variant)


def test_the_gradient_rule_catches_what_a_whole_array_scale_lets_pass():
    """The smallest-gradient column of a gradient scaled by 1 + 1e-7: within atol 1e-9 x max|want| of the whole array (assert_grad of
    tests/test_gpu_grad_scores.py, on its data), a hundred thousand allowances off at its own elements."""
    T, n = 300, 40
    obs, sim, _ = old_grad.series(T, n, seed=n + T)
    G = np.zeros((5, n))
    G[4] = -1.0 / n
    ref = pc.GradRef(obs, sim, G)
    state = pc.restatement(obs, sim, rows_per_split=pc.metrics_splits(n, T)[1])
    good = pc.restatement_grad(state, obs, sim, G)
    j = int(np.argmin(np.abs(ref.exact).max(0)))
    assert np.abs(ref.exact[:, j]).max() * 1e-7 < 0.5e-9 * np.abs(ref.exact).max()
    wrong = good.copy()
    wrong[:, j] *= 1.0 + 1e-7
    for got in (good, wrong):
        old_grad.assert_grad(got, ref.auto, 'whole-array scale')
    pc.assert_grad_per_element(good, ref, 'the restatement')
    factor = pc.grad_ratio(wrong, ref).max() / pc.K_GRAD
    print(f'column {j} x (1 + 1e-7): {factor:.3g} x the per-element allowance')
    assert factor > 100
    with pytest.raises(AssertionError, match='autograd'):
        pc.assert_grad_per_element(wrong, ref, 'scaled column')
