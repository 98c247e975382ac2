"""Test-only helpers of the per-column parity tests of the skill scores and their gradient (test_per_column.py on the CPU,
test_gpu_scores_per_column.py on the GPU box): the column regimes and gap patterns, the references of an array
(the scores arbiter oracle/rr_oracle_scores.c and the host 1-D path), the two rules, and a float64 numpy restatement of the kernels'
class of algorithm that the rules' constants are measured with.

The rule for the scores (assert_per_column).  u = 2^-53.  `exact` is the arbiter's value of a score in column j, S its scale:
mae for me; the value itself for mae and mse; 1 for pearson_r; |r| + |beta| + |gamma| for kge2012.  E_host is the worst, over all
columns and scores of the array, of |host - exact| / S, host being rr.metrics' 1-D path (the reference's own numpy calls) on each
column -- the reference implementation's rounding error on this very data, recomputed for every array and never taken from the
code under test.  With unit = max(E_host, 2^-52) a result passes when, in every column,
    me, mae, mse:       |got - exact| <= K unit S
    pearson_r, kge2012: |got - exact| <= K (unit + C_KAPPA u (kappa_t + kappa_p)) S,   kappa = |mean| / std from the arbiter,
its NaNs are where the arbiter's are and `count` is the arbiter's.  The kappa term is the price of a state that holds each chunk's
mean in one double (DESIGN.md section 9 "Accuracy"); where mae or mse is 0 (p = t) the bound is 0, so they are exactly 0.

The rule for the gradient (assert_grad_per_element).  The arbiter returns dL/dy_pred, per element the sum of the absolute values of
the terms added into it (`scale`) and per column bm = |B mt| + |P mp|.  E_auto is the worst |autograd - exact| / scale, autograd being
torch on the CPU through test_grad_scores.dense_scores in float64.  An element passes when
    |got - exact| <= K_GRAD max(E_auto, 2^-52) scale + C_MEAN u bm_j     (+ 2^-24 |exact| for float32 y_pred),
summed over the shares of a repeated column; a skipped element and an element of an unscored column are exactly 0; NaNs are where
the arbiter's are.

K, C_KAPPA, K_GRAD and C_MEAN are measured, not chosen: test_per_column.py runs `restatement` (pivoted chunk sums, Chan merges) over
every regime at three chunk lengths, three row splits and both fold orders, takes the worst ratios, gives each a factor 4 and rounds
up to a power of two, and asserts that the constants below are those numbers."""
import functools
import os
import sys
import warnings

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

SCORES = ('me', 'mae', 'mse', 'pearson_r', 'kge2012')
U = 2.0 ** -53
EPS = 2.0 ** -52
CHUNK = 32                 # rr_kernels_metrics.hpp: kMetricsChunk
TARGET_BLOCKS, BLOCK = 2048, 256      # kMetricsTargetBlocks; rr_common.hpp: kBlock

# measured by test_per_column.test_constants_are_the_measured_ones (DESIGN.md section 2d has the table)
K = 128.0
C_KAPPA = 0.25
K_GRAD = 256.0
C_MEAN = 64.0


# ------------------------------------------------------------------------------------------------ regimes and gaps

REGIMES = ('benign', 'offset 1e2', 'offset 1e4', 'offset 1e6', 'twenty decades', 'near-perfect', 'anti-correlated', 'spike pivots',
           'step', 'constant true', 'constant pred', 'all-zero true', 'chunk-constant')
OFFSET_REGIMES = ('offset 1e2', 'offset 1e4', 'offset 1e6')
GAPS = ('none', 'row 0 of every chunk', 'whole chunks', 'alternate rows', 'all but two pairs', 'all but one pair', 'all pairs')
# the gradient of the KGE is 1 / E times bounded terms and E -> 0 where p -> t: its condition number there (1e9) is no property of
# a kernel, and through E_auto it would loosen the bound of every other column, so the gradient arrays leave that regime out
GRAD_REGIMES = tuple(r for r in REGIMES if r != 'near-perfect')
# E_auto is one number per array and autograd's own error grows like u kappa (29,000 u at offset 1e6), so the gradient arrays come in
# two groups: the regimes of moderate kappa, which a large offset next to them must not loosen, and the offsets on their own
GRAD_MODERATE = tuple(r for r in GRAD_REGIMES if r not in ('offset 1e4', 'offset 1e6'))
GRAD_OFFSET = ('benign',) + OFFSET_REGIMES


def _unit_noise(rng, T):
    """A skewed series of mean 0 and standard deviation 1 (a centred gamma, as a hydrograph's noise is)."""
    return (rng.gamma(2.0, 0.5, T) - 1.0) / np.sqrt(0.5)


def regime_column(regime, T, seed, exact_copy=False):
    """(t, p): one observed and one simulated float64 series of T rows in the named regime."""
    from test_gpu_metrics import series
    rng = np.random.default_rng([seed, REGIMES.index(regime)])
    if regime in ('benign', 'twenty decades', 'constant true', 'constant pred', 'all-zero true'):
        t, p = (v[:, 0].copy() for v in series(rng, T, 1))
        if regime == 'twenty decades':
            s = 10.0 ** rng.uniform(-12.0, 8.0) / max(np.abs(t).mean(), 1e-300)
            t, p = t * s, p * s
        elif regime == 'constant true':
            t[:] = 1.0 + rng.integers(1, 40) * 0.5
        elif regime == 'constant pred':
            p[:] = 2.5
        elif regime == 'all-zero true':
            t[:] = 0.0
        return t, p
    sigma = 10.0 ** rng.uniform(-1.0, 1.0)
    x = _unit_noise(rng, T)
    a, noise = rng.uniform(0.6, 1.4), rng.normal(0.0, 0.3, T)
    if regime in OFFSET_REGIMES:
        kappa = float(regime.split()[1])
        return sigma * (kappa + x), sigma * (kappa * rng.uniform(0.8, 1.2) + a * x + noise)
    if regime == 'near-perfect':
        t = sigma * (3.0 + x)
        return t, (t.copy() if exact_copy else t * (1.0 + 1e-9 * rng.standard_normal(T)))
    if regime == 'anti-correlated':
        t = sigma * (3.0 + x)
        return t, a * (2.0 * t.mean() - t) + sigma * 0.05 * noise
    if regime == 'spike pivots':
        t = sigma * (3.0 + x)
        rest = np.delete(t, np.s_[0::CHUNK]) if T > 1 else t
        t[0::CHUNK] = rest.mean() + (1e6 * max(rest.std(), sigma)) * (1.0 + 0.1 * rng.random(t[0::CHUNK].size))
        return t, a * t + sigma * noise
    if regime == 'step':
        t = sigma * (3.0 + x)
        t[T // 2:] += 100.0 * sigma
        return t, a * t + sigma * noise
    if regime == 'chunk-constant':
        v = sigma * (3.0 + _unit_noise(rng, -(-T // CHUNK)))
        w = a * v + sigma * rng.normal(0.0, 0.3, v.size)
        return np.repeat(v, CHUNK)[:T].copy(), np.repeat(w, CHUNK)[:T].copy()
    raise ValueError(regime)


def gap_rows(gap, T):
    """missing[T] of a gap pattern."""
    r = np.arange(T)
    if gap == 'none':
        return np.zeros(T, dtype=bool)
    if gap == 'row 0 of every chunk':
        return r % CHUNK == 0
    if gap == 'whole chunks':
        return (r // CHUNK) % 2 == 1
    if gap == 'alternate rows':
        return r % 2 == 1
    keep = {'all but two pairs': [T // 3, T - 1], 'all but one pair': [T // 2], 'all pairs': []}[gap]
    miss = np.ones(T, dtype=bool)
    miss[keep] = False
    return miss


class Array:
    """One test array: t, p (T, n) float64 (read-only), the regime and the gap pattern of every column."""

    def __init__(self, t, p, regimes, gaps):
        for a in (t, p):
            a.flags.writeable = False
        self.t, self.p, self.regimes, self.gaps = t, p, tuple(regimes), tuple(gaps)
        self.T, self.n = t.shape


@functools.lru_cache(maxsize=None)
def arrays(T, n, gaps=False, regimes=REGIMES, seed=0):
    """The arrays of a shape: column j of array a is combination a n + j of the regimes (cycled fastest, so neighbouring lanes carry
    different regimes) and, with gaps=True, of the gap patterns (NaN in t); as many arrays as it takes to hold every combination
    once.  The first 'near-perfect' column of every array has p = t exactly."""
    combos = len(regimes) * (len(GAPS) if gaps else 1)
    out = []
    for a in range(-(-combos // n)):
        t, p, names, gnames, exact = np.empty((T, n)), np.empty((T, n)), [], [], True
        for j in range(n):
            idx = a * n + j
            regime, gap = regimes[idx % len(regimes)], GAPS[(idx // len(regimes)) % len(GAPS)] if gaps else 'none'
            t[:, j], p[:, j] = regime_column(regime, T, seed * 100_003 + idx, exact_copy=exact and regime == 'near-perfect')
            exact = exact and regime != 'near-perfect'
            t[gap_rows(gap, T), j] = np.nan
            names.append(regime)
            gnames.append(gap)
        out.append(Array(t, p, names, gnames))
    return tuple(out)


def with_map(arr):
    """(t, wide, columns, regimes) of an Array for the column-map paths: `wide` (T, n + 2) holds p in its columns 1 .. n, a copy of p's
    last column in its first and of p's first column in its last; column 0 of t is scored against the LAST column of wide, column
    n - 1 against the FIRST, column j otherwise against j + 1 -- and column 1 of t becomes a rescaled noisy copy of column 0 scored
    against the same column of wide as column 0 (a repeat; its regime and gaps are column 0's)."""
    T, n = arr.t.shape
    t, regimes = arr.t.copy(), list(arr.regimes)
    wide = np.empty((T, n + 2))
    wide[:, 1:n + 1], wide[:, 0], wide[:, n + 1] = arr.p, arr.p[:, n - 1], arr.p[:, 0]
    columns = np.arange(1, n + 1)
    columns[0], columns[n - 1] = n + 1, 0
    if n >= 3:
        rng = np.random.default_rng(n * 1000 + T)
        with np.errstate(invalid='ignore'):
            spread = np.nanstd(t[:, 0]) if np.isfinite(t[:, 0]).any() else 0.0
        t[:, 1] = 1.1 * t[:, 0] + 0.05 * spread * rng.standard_normal(T)
        columns[1], regimes[1] = columns[0], regimes[0]
    for a in (t, wide, columns):
        a.flags.writeable = False
    return t, wide, columns, tuple(regimes)


# (T, n): the expected row splits of rr.metrics.scores -- the smallest shapes at which the kernels take each of their paths
GPU_SHAPES = {(1, 3): 1, (2, 5): 1, (31, 7): 1, (33, 7): 2, (100, 7): 4, (2000, 300): 63, (4100, 64): 129}
GRAD_SHAPES = ((2, 5), (33, 7), (100, 7), (2000, 300))


def metrics_splits(n, rows, members=1):
    """(splits, rows_per_split) of an update: metrics_split's documented function (rr_kernels_metrics.hpp), restated."""
    col_blocks = members * -(-n // BLOCK)
    chunks = -(-rows // CHUNK)
    want = max(1, -(-TARGET_BLOCKS // col_blocks))
    splits = max(1, min(want, chunks))
    rps = -(-chunks // splits) * CHUNK
    return max(1, -(-rows // rps)), rps


# ------------------------------------------------------------------------------------------------ references

def widen(a, dtype):
    """The doubles the GPU computes with when `a` is handed over in `dtype`."""
    return np.asarray(a).astype(dtype).astype(np.float64)


def host_scores(t, p, columns=None, skip=False):
    """rr.metrics' host 1-D path on every column (its kept pairs with skip) of float64 data: {score: (n,)} and 'count'."""
    import river_route_amd as rr
    t, p = np.asarray(t, dtype=np.float64), np.asarray(p, dtype=np.float64)
    p = p[:, columns] if columns is not None else p
    fns = [rr.metrics.me, rr.metrics.mae, rr.metrics.mse, rr.metrics.pearson_r, rr.metrics.kge2012]
    out = {k: np.full(t.shape[1], np.nan) for k in SCORES}
    keep = ~np.isnan(t) if skip else np.ones(t.shape, dtype=bool)
    with warnings.catch_warnings(), np.errstate(all='ignore'):
        warnings.simplefilter('ignore')
        for j in range(t.shape[1]):
            if keep[:, j].any():
                tj, pj = np.ascontiguousarray(t[keep[:, j], j]), np.ascontiguousarray(p[keep[:, j], j])
                for k, f in zip(SCORES, fns):
                    out[k][j] = f(tj, pj)
    out['count'] = keep.sum(0).astype(np.float64)
    return out


def score_scales(arb):
    """S of the rule, per score, from the arbiter's outputs."""
    with np.errstate(invalid='ignore'):
        return {'me': arb['mae'], 'mae': np.abs(arb['mae']), 'mse': np.abs(arb['mse']), 'pearson_r': np.ones_like(arb['mae']),
                'kge2012': np.abs(arb['pearson_r']) + np.abs(arb['beta']) + np.abs(arb['gamma'])}


def score_errors(got, arb):
    """{score: |got - exact| / S per column}, 0 where both are 0 and where the arbiter has a NaN (compared separately)."""
    S = score_scales(arb)
    out = {}
    for k in SCORES:
        with np.errstate(invalid='ignore', divide='ignore'):
            e = np.abs(np.asarray(got[k], dtype=np.float64) - arb[k])
            q = np.where(e == 0, 0.0, e / S[k])
        out[k] = np.where(np.isnan(arb[k]), 0.0, q)
    return out


class ScoreRef:
    """The references of one scores call, computed once: `arb` the arbiter's outputs, `host` the host 1-D path's, E_host."""

    def __init__(self, t, p, columns=None, skip=False, regimes=None):
        from oracle import oracle
        self.arb = oracle.scores_ld(t, p, columns, skip)
        self.host = host_scores(t, p, columns, skip)
        self.skip = skip
        self.regimes = tuple(regimes) if regimes is not None else ('',) * np.asarray(t).shape[1]
        err = score_errors(self.host, self.arb)
        self.e_host = float(max(np.nanmax(err[k], initial=0.0) for k in SCORES))
        self.unit = max(self.e_host, EPS)
        with np.errstate(invalid='ignore'):
            self.kappa = self.arb['kappa_t'] + self.arb['kappa_p']


def score_ratios(got, ref, c=C_KAPPA):
    """{score: |got - exact| / (allowance / K) per column}: what K has to cover."""
    err = score_errors(got, ref.arb)
    out = {}
    for k in SCORES:
        allow = np.full(err[k].shape, ref.unit)
        if k in ('pearson_r', 'kge2012'):
            with np.errstate(invalid='ignore'):
                allow = allow + np.where(np.isfinite(ref.kappa), c * U * ref.kappa, 0.0)
        out[k] = err[k] / allow
    return out


def assert_per_column(got, ref, what, K=K, c=C_KAPPA):
    """The scores rule of the module docstring for got = {score: (n,)[, 'count']} against a ScoreRef.  Returns {regime: worst ratio},
    the ratio in units of the allowance at K = 1 (so a value up to K passes)."""
    got = {k: (v.detach().cpu().numpy() if hasattr(v, 'detach') else np.asarray(v)) for k, v in got.items()}
    n = ref.arb['me'].shape[0]
    for k in SCORES:
        assert got[k].shape == (n,) and got[k].dtype == np.float64, f'{what} {k}: {got[k].dtype} {got[k].shape}'
        bad = np.flatnonzero(np.isnan(got[k]) != np.isnan(ref.arb[k]))
        assert bad.size == 0, (f'{what} {k}: NaN pattern differs from the arbiter\'s in columns {bad[:5]} '
                               f'({[ref.regimes[j] for j in bad[:5]]}): got {got[k][bad[:5]]}, exact {ref.arb[k][bad[:5]]}')
    if ref.skip or 'count' in got:
        assert np.array_equal(got['count'], ref.arb['count']), f'{what}: count differs from the arbiter\'s'
    ratios = score_ratios(got, ref, c)
    worst = {}
    for k in SCORES:
        j = int(np.argmax(ratios[k]))
        assert ratios[k][j] <= K, (f'{what} {k}: column {j} ({ref.regimes[j]}) is off by {ratios[k][j]:.3g} x its allowance at K = 1 (got '
                                   f'{got[k][j]:.17g}, exact {ref.arb[k][j]:.17g}, E_host {ref.e_host:.3g}, kappa_t + kappa_p '
                                   f'{ref.kappa[j]:.3g}; allowed {K:g} x)')
        for j, reg in enumerate(ref.regimes):
            worst[reg] = max(worst.get(reg, 0.0), float(ratios[k][j]))
    return worst


# ------------------------------------------------------------------------------------------------ the gradient rule

def autograd_grad(t, p, G, columns=None, skip=False):
    """dL/dp for L = sum G * scores by torch autograd on the CPU through the dense float64 restatement of tests/test_grad_scores.py
    (its masked form of tests/missing_helpers.py with skip); NaN columns are left as autograd leaves them."""
    import torch
    from missing_helpers import dense_scores_missing
    from test_grad_scores import dense_scores
    tt = torch.tensor(np.asarray(t, dtype=np.float64))
    pt = torch.tensor(np.asarray(p, dtype=np.float64), requires_grad=True)
    ps = pt if columns is None else pt[:, torch.as_tensor(np.array(columns, dtype=np.int64))]
    s = dense_scores_missing(tt, ps) if skip else dense_scores(tt, ps)
    loss = sum((torch.tensor(G[k]) * s[name]).sum() for k, name in enumerate(SCORES) if np.any(G[k] != 0))
    loss.backward()
    return pt.grad.numpy()


class GradRef:
    """The references of one gradient call: `exact`, `scale`, `bm` from the arbiter, `auto` from autograd, E_auto; `allow_mean` is the
    per-element sum of bm over the columns scored against it, `scored` marks the elements some kept pair reaches."""

    def __init__(self, t, p, G, columns=None, skip=False):
        from oracle import oracle
        t, p = np.asarray(t, dtype=np.float64), np.asarray(p, dtype=np.float64)
        a = oracle.scores_grad_ld(t, p, G, columns, skip)
        self.exact, self.scale, self.bm = a.grad, a.scale, a.bm
        self.auto = autograd_grad(t, p, G, columns, skip)
        cols = np.arange(t.shape[1]) if columns is None else np.asarray(columns)
        keep = ~np.isnan(t) if skip else np.ones(t.shape, dtype=bool)
        self.allow_mean = np.zeros(p.shape)
        self.scored = np.zeros(p.shape, dtype=bool)
        for j, c in enumerate(cols):
            self.allow_mean[:, c] += np.where(keep[:, j], np.nan_to_num(self.bm[j], nan=0.0, posinf=0.0), 0.0)
            self.scored[:, c] |= keep[:, j]
        live = self.scored & np.isfinite(self.exact) & np.isfinite(self.auto) & (self.scale > 0)
        with np.errstate(invalid='ignore', divide='ignore'):
            self.e_auto = float(np.max(np.abs(self.auto - self.exact)[live] / self.scale[live], initial=0.0))
        self.unit = max(self.e_auto, EPS)
        self.live = self.scored & np.isfinite(self.exact)


def grad_ratio(got, ref, c_m=C_MEAN, f32=False):
    """Per live element, what K_GRAD has to cover: (|got - exact| - C_MEAN u bm - [f32] 2^-24 |exact|) / (unit scale), floored at 0."""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref.exact)
    rest = err - c_m * U * ref.allow_mean - (2.0 ** -24 * np.abs(ref.exact) if f32 else 0.0)
    out = np.zeros(err.shape)
    with np.errstate(invalid='ignore', divide='ignore'):
        out[ref.live] = np.where(rest[ref.live] <= 0, 0.0, rest[ref.live] / (ref.unit * ref.scale[ref.live]))
    return out


def assert_grad_per_element(got, ref, what, K=K_GRAD, c_m=C_MEAN, f32=False):
    """The gradient rule of the module docstring for got (T, m) against a GradRef.  Returns the worst ratio (up to K passes)."""
    got = np.asarray(got)
    assert got.shape == ref.exact.shape, f'{what}: shape {got.shape} != {ref.exact.shape}'
    assert not got[~ref.scored].any(), f'{what}: {int(np.count_nonzero(got[~ref.scored]))} nonzero values at skipped or unscored elements'
    bad = np.isnan(got) != np.isnan(ref.exact)
    assert not bad.any(), f'{what}: NaN pattern differs from the arbiter\'s, first at {tuple(int(v) for v in np.argwhere(bad)[0])}'
    ratio = grad_ratio(got, ref, c_m, f32)
    at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    assert ratio[at] <= K, (f'{what}: element {tuple(int(v) for v in at)} is off by {ratio[at]:.3g} x autograd\'s own error at the element\'s '
                            f'scale beyond the mean term (got {float(got[at]):.17g}, exact {ref.exact[at]:.17g}, scale {ref.scale[at]:.3g}, '
                            f'E_auto {ref.e_auto:.3g}; allowed {K:g} x)')
    return float(ratio[at])


# ------------------------------------------------------------------------------------------------ the restatement
# The kernels' class of algorithm in float64 numpy, every column at once: the rows of an update are cut into row splits, a split into
# chunks; a chunk's sums are shifted by its pivot (its first kept pair) and added row by row; chunks merge into their split's state
# and the splits into the result by Chan, Golub & LeVeque's pairwise update.  No fused multiply-adds (numpy has none).

FIELDS = ('cnt', 'mt', 'mp', 'm2t', 'm2p', 'c', 'sd', 'sad', 'sd2')


def _merge(a, b):
    """mstat_merge: a <- a merged with b, an empty side skipped or copied as it is."""
    with np.errstate(invalid='ignore', divide='ignore'):
        nn = a['cnt'] + b['cnt']
        f = b['cnt'] / nn
        w = a['cnt'] * f
        dt, dp = b['mt'] - a['mt'], b['mp'] - a['mp']
        m = {'cnt': nn, 'mt': a['mt'] + dt * f, 'mp': a['mp'] + dp * f, 'm2t': a['m2t'] + (b['m2t'] + dt * dt * w),
             'm2p': a['m2p'] + (b['m2p'] + dp * dp * w), 'c': a['c'] + (b['c'] + dt * dp * w), 'sd': a['sd'] + b['sd'],
             'sad': a['sad'] + b['sad'], 'sd2': a['sd2'] + b['sd2']}
    eb, ea = b['cnt'] == 0, a['cnt'] == 0
    return {k: np.where(eb, a[k], np.where(ea, b[k], m[k])) for k in FIELDS}


def restatement(t, p, chunk=CHUNK, rows_per_split=None, reverse=False, skip=False, variant=None):
    """The per-column state {field: (n,)} of (T, n) float64 t, p.  rows_per_split None: one split.  reverse: the splits fold last to
    first.  variant (the rule must catch each, test_per_column.py): 'unshifted' -- pivot 0; 'pivot row 0' -- the pivot is the chunk's
    row 0 where that pair is kept, else 0; 'float32 mean' -- the second chunk's means (the first's, of a single chunk) are rounded
    through float32 before the merge."""
    t, p = np.asarray(t, dtype=np.float64), np.asarray(p, dtype=np.float64)
    T, n = t.shape
    rps = T if rows_per_split is None else int(rows_per_split)
    ok_all = ~np.isnan(t) if skip else np.ones((T, n), dtype=bool)
    zero = {k: np.zeros(n) for k in FIELDS}
    states, chunk_no = [], 0
    for r0 in range(0, T, rps):
        s = dict(zero)
        for q0 in range(r0, min(T, r0 + rps), chunk):
            q1 = min(T, r0 + rps, q0 + chunk)
            kt, kp, kept = np.zeros(n), np.zeros(n), np.zeros(n)
            if variant == 'pivot row 0':
                kt, kp = np.where(ok_all[q0], t[q0], 0.0), np.where(ok_all[q0], p[q0], 0.0)
            acc = {k: np.zeros(n) for k in ('st', 'sp', 'stt', 'spp', 'stp', 'sd', 'sad', 'sd2')}
            for r in range(q0, q1):
                ok = ok_all[r]
                if variant is None or variant == 'float32 mean':
                    first = ok & (kept == 0)
                    kt, kp = np.where(first, t[r], kt), np.where(first, p[r], kp)
                kept = kept + ok
                with np.errstate(invalid='ignore'):
                    a, b, d = np.where(ok, t[r] - kt, 0.0), np.where(ok, p[r] - kp, 0.0), np.where(ok, t[r] - p[r], 0.0)
                acc['st'] = acc['st'] + a
                acc['sp'] = acc['sp'] + b
                acc['stt'] = acc['stt'] + a * a
                acc['spp'] = acc['spp'] + b * b
                acc['stp'] = acc['stp'] + a * b
                acc['sd'] = acc['sd'] + d
                acc['sad'] = acc['sad'] + np.abs(d)
                acc['sd2'] = acc['sd2'] + d * d
            with np.errstate(invalid='ignore', divide='ignore'):
                inv = np.where(kept > 0, 1.0 / np.where(kept > 0, kept, 1.0), 0.0)
                b = {'cnt': kept, 'mt': kt + acc['st'] * inv, 'mp': kp + acc['sp'] * inv,
                     'm2t': acc['stt'] - acc['st'] * inv * acc['st'], 'm2p': acc['spp'] - acc['sp'] * inv * acc['sp'],
                     'c': acc['stp'] - acc['st'] * inv * acc['sp'], 'sd': acc['sd'], 'sad': acc['sad'], 'sd2': acc['sd2']}
                b['m2t'] = np.where(b['m2t'] < 0, 0.0, b['m2t'])
                b['m2p'] = np.where(b['m2p'] < 0, 0.0, b['m2p'])
            if variant == 'float32 mean' and chunk_no == (1 if T > chunk else 0):
                b['mt'], b['mp'] = widen(b['mt'], np.float32), widen(b['mp'], np.float32)
            chunk_no += 1
            s = _merge(s, b)
        states.append(s)
    if reverse:
        states = states[::-1]
    acc = states[0]
    for s in states[1:]:
        acc = _merge(s, acc) if reverse else _merge(acc, s)
    return _merge(dict(zero), acc)


def finish(s):
    """k_metrics_finish: the state -> {score: (n,)} and 'count', with the reference's rules."""
    with np.errstate(invalid='ignore', divide='ignore'):
        N = s['cnt']
        r = np.where((s['m2t'] > 0) & (s['m2p'] > 0), s['c'] / np.sqrt(s['m2t']) / np.sqrt(s['m2p']), np.nan)
        r = np.where(r > 1, 1.0, np.where(r < -1, -1.0, r))
        st, sp = np.sqrt(s['m2t'] / N), np.sqrt(s['m2p'] / N)
        beta, gamma = s['mp'] / s['mt'], (s['mp'] / sp) / (s['mt'] / st)
        kge = 1.0 - np.sqrt((r - 1.0) ** 2 + (beta - 1.0) ** 2 + (gamma - 1.0) ** 2)
        kge = np.where((st == 0) | (sp == 0) | (s['mt'] == 0) | (N == 0), np.nan, kge)
        return {'me': s['sd'] / N, 'mae': s['sad'] / N, 'mse': s['sd2'] / N, 'pearson_r': r, 'kge2012': kge, 'count': N.copy()}


def restatement_grad(s, t, p, G, skip=False):
    """k_metrics_adjoint_coef and k_metrics_adjoint_rows in float64 numpy on a restatement state (dense: no column map)."""
    t, p = np.asarray(t, dtype=np.float64), np.asarray(p, dtype=np.float64)
    N, mt, mp, m2t, m2p = s['cnt'], s['mt'], s['mp'], s['m2t'], s['m2p']
    g_me, g_mae, g_mse, g_r, g_kge = G
    zero = np.zeros_like(mt)
    with np.errstate(all='ignore'):
        has_r = (m2t > 0) & (m2p > 0)
        r_raw = np.where(has_r, s['c'] / np.sqrt(m2t) / np.sqrt(m2p), np.nan)
        clipped = (r_raw > 1) | (r_raw < -1)
        r = np.clip(r_raw, -1.0, 1.0)
        r_B = np.where(clipped, 0.0, 1.0 / (np.sqrt(m2t) * np.sqrt(m2p)))
        r_P = np.where(clipped, 0.0, -r_raw / m2p)
        st, sp = np.sqrt(m2t / N), np.sqrt(m2p / N)
        beta, gamma = mp / mt, (mp / sp) / (mt / st)
        E = np.sqrt((r - 1.0) ** 2 + (beta - 1.0) ** 2 + (gamma - 1.0) ** 2)
        cv = st / mt
        gamma_P, gamma_A, beta_A = -cv * mp / (N * sp * sp * sp), cv / (N * sp), 1.0 / (N * mt)
        w = 2.0 * g_mse / N
        wk = -g_kge / E
        no_kge = (st == 0) | (sp == 0) | (mt == 0)
        A = np.where(g_me != 0, -g_me / N, zero) + np.where(g_mse != 0, -w * (mt - mp), zero)
        B = np.where(g_mse != 0, -w, zero) + np.where(g_r != 0, g_r * r_B, zero)
        P = np.where(g_mse != 0, w, zero) + np.where(g_r != 0, g_r * r_P, zero)
        A = np.where((g_r != 0) & ~has_r, np.nan, A)
        live = (g_kge != 0) & ~no_kge
        B = B + np.where(live, wk * ((r - 1.0) * r_B), zero)
        P = P + np.where(live, wk * ((r - 1.0) * r_P + (gamma - 1.0) * gamma_P), zero)
        A = A + np.where(live, wk * ((beta - 1.0) * beta_A + (gamma - 1.0) * gamma_A), zero)
        A = np.where((g_kge != 0) & no_kge, np.nan, A)
        S = np.where(g_mae != 0, -g_mae / N, zero)
        v = A + B * (t - mt) + P * (p - mp) + S * np.sign(t - p)
        return np.where(np.isnan(t), 0.0, v) if skip else v


CONFIGS = tuple((chunk, rps, rev) for chunk in (8, 32, 64) for rps in (32, 96, None) for rev in (False, True))
