"""Per-column parity of the skill scores and their gradient on the GPU: every entry point of rr.metrics and
rr.grad.scores against the long-double arbiter oracle/rr_oracle_scores.c, each column and each gradient element at its own scale, by
the two rules of tests/per_column.py (assert_per_column, assert_grad_per_element), over every regime and gap pattern of that module
cycled along the columns, at the smallest shapes at which the kernels take each of their paths.

Every test prints `TABLE|path|regime|ratio` lines (the worst ratio in units of the rule's allowance at K = 1): DESIGN.md's table."""
import functools

import numpy as np
import pytest
import torch

import per_column as pc
import river_route_amd as rr
import test_grad_scores as cpu
from oracle import oracle
from river_route_amd import engine

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
SCORES = pc.SCORES
F32, F64 = np.float32, np.float64
TORCH = {F32: torch.float32, F64: torch.float64}
SHAPES = list(pc.GPU_SHAPES)
DTYPES = [(F64, F64), (F32, F32), (F32, F64), (F64, F32)]
MEMBERS = 3


def table(path, worst):
    for regime, ratio in worst.items():
        print(f'TABLE|{path}|{regime}|{ratio:.3f}')


def dev(a, dtype=F64):
    return torch.tensor(np.asarray(a), device=DEV, dtype=TORCH[dtype])


@functools.lru_cache(maxsize=64)
def score_ref(T, n, gaps, a, dt=F64, dp=F64, mapped=False, member=None, own_obs=False):
    """(t, p, columns, ScoreRef) of array `a` of a shape as the GPU sees it (float32: rounded, then widened), computed once.  member: the
    predictions (and with own_obs the observations) of member `member` of the ensemble tests."""
    arr = pc.arrays(T, n, gaps)[a]
    t, p, columns, regimes = (arr.t, arr.p, None, arr.regimes) if not mapped else pc.with_map(arr)
    if member is not None:
        p = p * (1.0 + 0.05 * member)
        t = t * (1.0 + 0.03 * member) if own_obs else t
    t, p = pc.widen(t, dt), pc.widen(p, dp)
    for v in (t, p):
        v.flags.writeable = False
    return t, p, columns, pc.ScoreRef(t, p, columns, gaps, regimes)


def n_arrays(T, n, gaps):
    return len(pc.arrays(T, n, gaps))


def merge(worst, more):
    for k, v in more.items():
        worst[k] = max(worst.get(k, 0.0), v)


# ------------------------------------------------------------------------------------------------ forward

@pytest.mark.parametrize('T,n', SHAPES)
def test_row_splits_are_the_documented_ones(T, n):
    """The shapes exercise what their table says: the update's row splits, from the sizer of its work memory (72 bytes per column and
    split) and from metrics_split's documented function."""
    want = pc.GPU_SHAPES[(T, n)]
    assert engine.metrics_work_bytes(n, T) == want * engine.METRICS_STATE * 8 * n
    assert pc.metrics_splits(n, T)[0] == want
    assert engine.metrics_members_work_bytes(n, MEMBERS, T) == pc.metrics_splits(n, T, MEMBERS)[0] * engine.METRICS_STATE * 8 * n * MEMBERS


@pytest.mark.parametrize('kind', ['numpy', 'torch'])
@pytest.mark.parametrize('dt,dp', DTYPES)
@pytest.mark.parametrize('T,n', SHAPES)
def test_scores(T, n, dt, dp, kind):
    worst = {}
    for a in range(n_arrays(T, n, False)):
        t, p, _, ref = score_ref(T, n, False, a, dt, dp)
        if kind == 'numpy':
            got = rr.metrics.scores(t.astype(dt), p.astype(dp))
            assert all(isinstance(v, np.ndarray) for v in got.values())
        else:
            got = rr.metrics.scores(dev(t, dt), dev(p, dp))
            assert all(torch.is_tensor(v) and v.device == DEV for v in got.values())
        merge(worst, pc.assert_per_column(got, ref, f'scores {kind} {T}x{n} {dt.__name__}/{dp.__name__} array {a}'))
    table(f'scores {kind} {dt.__name__}/{dp.__name__}', worst)


@pytest.mark.parametrize('gaps', [False, True])
@pytest.mark.parametrize('T,n', SHAPES)
def test_column_map_with_repeats(T, n, gaps):
    worst = {}
    for a in range(n_arrays(T, n, gaps)):
        t, wide, columns, ref = score_ref(T, n, gaps, a, mapped=True)
        assert columns[0] == wide.shape[1] - 1 and columns[n - 1] == 0 and (n < 3 or columns[1] == columns[0])
        got = rr.metrics.scores(t, wide, columns=columns, skip_missing=gaps)
        merge(worst, pc.assert_per_column(got, ref, f'column map {T}x{n} gaps {gaps} array {a}'))
    table('column map' + (', skip_missing' if gaps else ''), worst)


@pytest.mark.parametrize('T,n', SHAPES)
def test_pitched_views(T, n):
    """Rows wider than the columns read, the true and the predicted pitch unequal (float64 against float32, as a routed array is)."""
    worst = {}
    for a in range(n_arrays(T, n, False)):
        t, p, _, ref = score_ref(T, n, False, a, F64, F32)
        bt = torch.full((T, n + 37), 7.0, dtype=torch.float64, device=DEV)
        bp = torch.full((T, n + 74), -3.0, dtype=torch.float32, device=DEV)
        bt[:, 5:5 + n], bp[:, 37:37 + n] = dev(t), dev(p, F32)
        vt, vp = bt[:, 5:5 + n], bp[:, 37:37 + n]
        assert vt.stride(0) == n + 37 and vp.stride(0) == n + 74
        merge(worst, pc.assert_per_column(rr.metrics.scores(vt, vp), ref, f'pitched {T}x{n} array {a}'))
    table('pitched views', worst)


@pytest.mark.parametrize('gaps', [False, True])
@pytest.mark.parametrize('T,n', SHAPES)
def test_accumulator_row_blocks(T, n, gaps):
    """Row blocks cut at 1, 31, 32, 33, 65 and T - 1: every block restarts the chunks, so a pivot is any row."""
    cuts = sorted({0, T} | {c for c in (1, 31, 32, 33, 65, T - 1) if 0 < c < T})
    worst = {}
    for a in range(n_arrays(T, n, gaps)):
        t, p, _, ref = score_ref(T, n, gaps, a)
        acc = rr.metrics.Accumulator(n, skip_missing=gaps)
        for r0, r1 in zip(cuts[:-1], cuts[1:]):
            acc.update(t[r0:r1], p[r0:r1])
        assert acc.rows == T
        merge(worst, pc.assert_per_column(acc.result(), ref, f'row blocks {T}x{n} gaps {gaps} array {a}'))
    table('Accumulator row blocks' + (', skip_missing' if gaps else ''), worst)


@pytest.mark.parametrize('kind,dt,dp', [('numpy', F64, F64), ('torch', F32, F64), ('torch', F64, F32)])
@pytest.mark.parametrize('T,n', SHAPES)
def test_skip_missing_every_gap_pattern(T, n, kind, dt, dp):
    worst = {}
    for a in range(n_arrays(T, n, True)):
        t, p, _, ref = score_ref(T, n, True, a, dt, dp)
        got = (rr.metrics.scores(t.astype(dt), p.astype(dp), skip_missing=True) if kind == 'numpy' else
               rr.metrics.scores(dev(t, dt), dev(p, dp), skip_missing=True))
        assert 'count' in got
        merge(worst, pc.assert_per_column(got, ref, f'skip_missing {kind} {T}x{n} {dt.__name__}/{dp.__name__} array {a}'))
    table(f'skip_missing {kind} {dt.__name__}/{dp.__name__}', worst)


@pytest.mark.parametrize('own_obs,mapped,gaps', [(False, False, False), (True, False, False), (False, True, False), (False, False, True),
                                                 (True, True, True)])
@pytest.mark.parametrize('T,n', SHAPES)
def test_members(T, n, own_obs, mapped, gaps):
    """Three members in one launch -- one observation block for all or one per member, with a column map, with skip_missing -- each
    member held to its own arbiter call; scores_members in one pass and MemberAccumulator in two row blocks."""
    worst = {}
    for a in range(n_arrays(T, n, gaps)):
        refs = [score_ref(T, n, gaps, a, mapped=mapped, member=m, own_obs=own_obs) for m in range(MEMBERS)]
        columns = refs[0][2]
        pred = np.stack([r[1] for r in refs])
        obs = np.stack([r[0] for r in refs]) if own_obs else refs[0][0]
        got = rr.metrics.scores_members(obs, pred, columns=columns, skip_missing=gaps)
        acc = rr.metrics.MemberAccumulator(n, MEMBERS, columns=columns, skip_missing=gaps)
        cut = min(T - 1, 33) if T > 1 else T
        acc.update(dev(obs[..., :cut, :]), dev(pred[:, :cut]))
        if cut < T:
            acc.update(dev(obs[..., cut:, :]), dev(pred[:, cut:]))
        blocks = acc.result()
        for m in range(MEMBERS):
            for what, res in (('scores_members', got), ('MemberAccumulator', blocks)):
                one = {k: (v[m].cpu().numpy() if torch.is_tensor(v) else v[m]) for k, v in res.items()}
                merge(worst, pc.assert_per_column(one, refs[m][3], f'{what} {T}x{n} member {m} own_obs {own_obs} mapped {mapped} gaps {gaps} array {a}'))
    table('members' + (', own observations' if own_obs else '') + (', column map' if mapped else '') + (', skip_missing' if gaps else ''), worst)


# ------------------------------------------------------------------------------------------------ backward

GROUPS = {'moderate': pc.GRAD_MODERATE, 'offsets': pc.GRAD_OFFSET}
VARIANTS = ('dense', 'column map', 'skip_missing', 'float32 y_pred', 'float32 y_true')


@functools.lru_cache(maxsize=8)
def grad_inputs(T, n, group, variant, a):
    """(t, p, columns, skip, dt, dp, regimes) of one gradient array as the GPU sees it."""
    skip = variant == 'skip_missing'
    arr = pc.arrays(T, n, skip, GROUPS[group])[a]
    t, p, columns, regimes = (arr.t, arr.p, None, arr.regimes) if variant != 'column map' else pc.with_map(arr)
    dt, dp = (F32 if variant == 'float32 y_true' else F64), (F32 if variant == 'float32 y_pred' else F64)
    return pc.widen(t, dt), pc.widen(p, dp), columns, skip, dt, dp, regimes


def gpu_grad(t, p, G, columns, skip, dt, dp):
    pt = dev(p, dp).requires_grad_()
    s = rr.grad.scores(dev(t, dt), pt, columns=columns, skip_missing=skip)
    loss = sum((torch.as_tensor(G[k], device=DEV) * s[name]).sum() for k, name in enumerate(SCORES) if np.any(G[k] != 0))
    loss.backward()
    assert pt.grad.dtype == TORCH[dp] and pt.grad.shape == pt.shape
    return pt.grad.cpu().numpy()


@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('group', list(GROUPS))
@pytest.mark.parametrize('T,n', pc.GRAD_SHAPES)
def test_gradient_per_element(T, n, group, variant):
    """Each score alone, a random weighting of all five and (1 - kge).mean(): every element of dL/dy_pred at its own scale.  The NaN
    rule rides on the arbiter's pattern: a NaN score with a non-zero incoming gradient makes its column's kept rows NaN, and the
    columns beside it are finite and held to the bound."""
    worst = {}
    for a in range(len(pc.arrays(T, n, variant == 'skip_missing', GROUPS[group]))):
        t, p, columns, skip, dt, dp, regimes = grad_inputs(T, n, group, variant, a)
        for what, G in cpu.weights(n, seed=T):
            ref = pc.GradRef(t, p, G, columns, skip)
            got = gpu_grad(t, p, G, columns, skip, dt, dp)
            ratio = pc.assert_grad_per_element(got, ref, f'{variant} {group} {T}x{n} array {a} {what}', f32=dp == F32)
            worst[what] = max(worst.get(what, 0.0), ratio)
            if what in ('pearson_r', 'kge2012') and columns is None:
                # the NaN columns are those whose score is NaN, its gradient not 0 and a pair kept: nothing leaks into a neighbour
                arb = oracle.scores_ld(t, p, None, skip)
                want_nan = np.isnan(arb[what]) & (G[SCORES.index(what)] != 0) & (arb['count'] > 0)
                assert np.array_equal(np.isnan(got).any(0), want_nan), what
    table(f'gradient, {variant}, {group}', worst)


def test_two_backward_passes_bit_identical():
    T, n = 2000, 300
    t, p, columns, skip, dt, dp, _ = grad_inputs(T, n, 'moderate', 'column map', 0)
    G = np.random.default_rng(2).standard_normal((5, n))
    assert np.array_equal(gpu_grad(t, p, G, columns, skip, dt, dp), gpu_grad(t, p, G, columns, skip, dt, dp), equal_nan=True)
