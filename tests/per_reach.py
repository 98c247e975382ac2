"""Test-only helpers of the per-reach parity tests (test_per_reach.py on the CPU, test_gpu_per_reach.py on the GPU box): the
comparison of a routed array with the long-double arbiter (oracle/rr_oracle_ld.c) at every reach's OWN scale, the forcing /
parameter regimes, and the references (fp64 oracle + arbiter) of a case, computed once and shared read-only.

The rule ("Per-reach parity").  Let `raw` be the arbiter's unclamped interval means and `exact` its clamped rows.
For column j:  S_j = max_t |raw[t, j]|  (for a final state: max(S_j, |exact state_j|));  e_j(A) = max_t |A[t, j] - exact[t, j]|;
E_orc = max_j e_j(fp64 oracle) / S_j over the columns with S_j > 0 -- the reference implementation's own rounding error on this
very case, recomputed in every test and never taken from the code under test.  A routed array passes when, in every column,
e_j(got) <= K max(E_orc, 2^-52) S_j with K = 16; where S_j == 0 it holds +0.0 in every row; its NaNs are where the arbiter's are.

K = 16: a correctly rounded loop in another operation order (the same C loop built with fused multiply-adds) stayed within
4.8 x E_orc over 16 cases (6k ... 300k reaches, random and chain-grown networks, 1 and 3 sub-steps); 16 leaves about 3 x for a
kernel that also sums a reach's tributaries in another order."""
import functools
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

K = 16.0
EPS = 2.0 ** -52
DT = 900.0
N = 6000


# ------------------------------------------------------------------------------------------------ the comparison

def scales(raw, floor=None):
    """S_j: a column's own scale, the largest unclamped interval mean (with `floor`, a final state: no smaller than its magnitude)."""
    raw = np.asarray(raw)
    S = np.max(np.abs(raw), axis=0) if raw.shape[0] else np.zeros(raw.shape[1])
    return S if floor is None else np.maximum(S, np.abs(np.asarray(floor)))


def column_error(A, exact):
    """e_j(A) = max_t |A[t, j] - exact[t, j]| (NaNs, compared separately, count as no error)."""
    with np.errstate(invalid='ignore'):
        d = np.abs(np.asarray(A, dtype=np.float64) - exact)
    return np.max(np.where(np.isnan(d), 0.0, d), axis=0) if d.shape[0] else np.zeros(d.shape[1])


def oracle_error(oracle_rows, exact, S):
    """E_orc: the fp64 oracle's worst error against the arbiter, each reach at its own scale."""
    live = S > 0
    return float(np.max(column_error(oracle_rows, exact)[live] / S[live])) if live.any() else 0.0


def _rows(a):
    a = np.asarray(a)
    return a[None, :] if a.ndim == 1 else a


def assert_per_reach(got, oracle_rows, exact, raw, what, K=K, floor=None):
    """The rule of the module docstring.  got, oracle_rows, exact: (T, n) rows, or (n,) for a final state (then pass floor=exact, and
    raw the unclamped means of the call that left the state).  Returns max_j e_j(got) / (max(E_orc, 2^-52) S_j), the measured ratio."""
    got, oracle_rows, exact = _rows(got), _rows(oracle_rows), _rows(exact)
    assert got.shape == exact.shape == oracle_rows.shape, f'{what}: shapes {got.shape}, {oracle_rows.shape}, {exact.shape}'
    assert np.asarray(raw).shape[1] == exact.shape[1], f'{what}: raw has {np.asarray(raw).shape[1]} columns'
    S = scales(raw, floor)
    unit = max(oracle_error(oracle_rows, exact, S), EPS)
    assert np.array_equal(np.isnan(got), np.isnan(exact)), f'{what}: NaN pattern differs from the arbiter\'s'
    dead = S == 0
    if dead.any():
        g = got[:, dead]
        assert not g.any() and not np.signbit(g).any(), \
            f'{what}: {int(np.count_nonzero((g != 0) | np.signbit(g)))} values other than +0.0 in columns that carry nothing'
    live = ~dead
    if not live.any():
        return 0.0
    ratio = column_error(got, exact)[live] / S[live] / unit      # (in this order: unit x S_j underflows where a drained reach is down among the denormals)
    worst = int(np.argmax(ratio))
    j = int(np.flatnonzero(live)[worst])
    assert ratio[worst] <= K, (f'{what}: column {j} is off by {ratio[worst]:.3g} x the fp64 oracle\'s own error at a reach\'s scale '
                               f'(E_orc {unit:.3g}, S_j {S[j]:.3g}, max S {S.max():.3g}; allowed {K:g} x)')
    return float(ratio[worst])


def assert_per_reach_f32(got32, oracle_rows, exact, raw, what, K=K):
    """float32 rows out: per element |got - exact| <= 2^-24 |exact| + K max(E_orc, 2^-52) S_j -- one rounding to float32 of a value
    that keeps the float64 bound.  Returns the worst element's share of its allowance."""
    got = np.asarray(got32)
    assert got.dtype == np.float32 and got.shape == exact.shape, f'{what}: {got.dtype} {got.shape}'
    S = scales(raw)
    unit = max(oracle_error(oracle_rows, exact, S), EPS)
    assert np.array_equal(np.isnan(got), np.isnan(exact)), f'{what}: NaN pattern differs from the arbiter\'s'
    dead = S == 0
    if dead.any():
        assert not got[:, dead].any() and not np.signbit(got[:, dead]).any(), f'{what}: values other than +0.0 in columns that carry nothing'
    err = np.abs(got.astype(np.float64) - exact)
    allow = 2.0 ** -24 * np.abs(exact) + K * unit * S[None, :]
    bad = err > allow
    assert not bad.any(), (f'{what}: {int(bad.sum())} float32 elements beyond one float32 rounding of the float64 bound; the first at '
                           f'{tuple(int(v) for v in np.argwhere(bad)[0])}')
    live = allow > 0
    return float(np.max(err[live] / allow[live])) if live.any() else 0.0


# ------------------------------------------------------------------------------------------------ networks

def csc_from_down(down_index):
    has = down_index >= 0
    indptr = np.concatenate([[0], np.cumsum(has)]).astype(np.int32)
    return indptr, down_index[has].astype(np.int32)


def wide_network(n, seed=5, fan=8):
    """As test_gpu_tiles._wide_network: reach i flows into one of the next `fan` reaches, several per cent have four or more upstream."""
    rng = np.random.default_rng(seed)
    down = np.arange(n) + 1 + rng.integers(0, fan, n)
    down[down >= n] = n - 1
    down[n - 1] = -1
    return down.astype(np.int64)


@functools.lru_cache(maxsize=None)
def network(name):
    """(down_index, k, x) of a named network; k, x are the benign draw (k in [900, 7200] s, x in [0.05, 0.45]) the regimes start from."""
    from river_route_amd import synth
    if name == 'random':
        net = synth.synth_network(N, seed=21)
    elif name == 'postorder':
        net = synth.synth_network(N, seed=21, order='postorder')
    elif name == 'chain97':
        net = synth.synth_network_chain(N, p_chain=0.97, n_outlets=7, p_third=0.3)
    else:
        if name == 'wide':
            down = wide_network(N)
        elif name == 'chain':       # depth = n, every level one reach wide
            down = np.arange(1, 3001, dtype=np.int64)
        elif name == 'comb':        # reaches 0..m-1 are tributaries, m..2m-1 the stem
            m = 1500
            down = np.concatenate([m + np.arange(m), m + 1 + np.arange(m)]).astype(np.int64)
        elif name == 'star':        # one level of 5,000 tributaries into one outlet
            down = np.full(5001, 5000, dtype=np.int64)
        elif name == 'lone':
            down = np.full(777, -1, dtype=np.int64)
        else:
            raise ValueError(name)
        down[-1] = -1
        idx = np.arange(down.size)
        out = (down, 900.0 + 6300.0 * synth.u01(3, idx), 0.05 + 0.4 * synth.u01(4, idx))
        for a in out:
            a.flags.writeable = False
        return out
    out = (net.down_index, net.k, net.x)
    for a in out:
        a.flags.writeable = False
    return out


# ------------------------------------------------------------------------------------------------ regimes

REGIMES = ('synth params', 'short reaches', 'wild k, x', 'ten decades', 'signed', 'signed, ten decades, wild k', 'half dry')
CORE = ('synth params', 'signed, ten decades, wild k', 'half dry')      # what every path runs at least


def regime_inputs(regime, net_name, rows):
    """(k, x, lat, q0) of a regime on a network: lat is (rows, n) lateral volumes per DT (RapidMuskingum divides by DT through
    c4_dt; the Unit tests hand lat / DT over as lateral inflow), q0 the state a lateral-driven run starts from -- zero: a cold
    start, so a reach's scale is its forcing's; the second call of every test starts from the state the first one left."""
    from river_route_amd import synth
    down, k, x = network(net_name)
    n = down.size
    idx = np.arange(n)
    lat = synth.synth_qlateral(n, 0, rows)
    k, x = k.copy(), x.copy()
    if regime == 'short reaches':
        k[::3] = 300.0
    if 'wild k' in regime:
        k = 10.0 ** (1.5 + 4.0 * synth.u01(41, idx))
        x = 0.5 * synth.u01(42, idx)
        x[::7], x[3::7] = 0.0, 0.5
    if 'signed' in regime:
        lat = lat - 300.0
    if 'ten decades' in regime:
        lat = lat * 10.0 ** (-6.0 + 10.0 * synth.u01(43, idx))[None, :]
    if regime == 'half dry':
        lat[:, dry_columns(n)] = 0.0
    assert regime in REGIMES, regime
    return k, x, lat, np.zeros(n)


def dry_columns(n):
    """A random half of the first n / 2 columns."""
    return np.random.default_rng(44).permutation(n // 2)[:n // 4]


def channel_state(regime, net_name):
    """The initial state of a channel-only Muskingum run (no laterals: the state is all the forcing there is), shaped by the regime as
    the laterals are above -- but for 'signed': a state is a discharge, there is no lateral here that could have made it negative, and
    the clamp has work to do all the same (c1 < 0 or c3 < 0 turn a draining reach negative)."""
    from river_route_amd import synth
    n = network(net_name)[0].size
    idx = np.arange(n)
    q0 = 5.0 * synth.u01(99, idx)
    if 'ten decades' in regime:
        q0 *= 10.0 ** (-6.0 + 10.0 * synth.u01(43, idx))
    if regime == 'half dry':
        q0[dry_columns(n)] = 0.0
    return q0


def coefficients(k, x, nsub):
    """(c1, c2, c3) at the routing step DT / nsub -- doubles, handed to the oracle, the arbiter and the GPU alike."""
    from oracle import oracle
    return oracle.muskingum_coefficients(k, x, DT / nsub)


# ------------------------------------------------------------------------------------------------ references, computed once

class Ref:
    """One call's references: `orc` the fp64 oracle's rows, `exact` / `raw` the arbiter's clamped / unclamped rows, `q_orc` / `q_exact`
    the final states (tuples of arrays for UnitMuskingum: q_ch, q_full).  Every array is read-only."""

    def __init__(self, **kw):
        for k_, v in kw.items():
            for a in (v if isinstance(v, tuple) else (v,)):
                if isinstance(a, np.ndarray):
                    a.flags.writeable = False
            setattr(self, k_, v)


@functools.lru_cache(maxsize=12)      # (tests that share a case run side by side)
def rapid_case(net_name, regime, T, nsub, f32_lat=False):
    """RapidMuskingum, two consecutive calls of T rows each with the state handed over (each side hands over its own).
    f32_lat: the lateral rows are float32 values (widened: exact in float64).  Returns (inputs, [Ref, Ref])."""
    from oracle import oracle
    down, _, _ = network(net_name)
    n = down.size
    indptr, indices = csc_from_down(down)
    k, x, lat, q0 = regime_inputs(regime, net_name, 2 * T)
    if f32_lat:
        lat = lat.astype(np.float32).astype(np.float64)
    c1, c2, c3 = coefficients(k, x, nsub)
    lhs, c4_dt = np.ascontiguousarray(-c1[indices]), (c1 + c2) / DT
    q_o, q_e, refs = q0.copy(), q0.copy(), []
    for call in range(2):
        ql = np.ascontiguousarray(lat[call * T:(call + 1) * T])
        orc, exact, raw = np.zeros((T, n)), np.zeros((T, n)), np.zeros((T, n))
        oracle.rapid_route(indptr, indices, lhs, c2, c3, c4_dt, q_o, ql, orc, nsub)
        oracle.rapid_route_ld(indptr, indices, lhs, c2, c3, c4_dt, q_e, ql, exact, raw, nsub)
        refs.append(Ref(orc=orc, exact=exact, raw=raw, q_orc=q_o.copy(), q_exact=q_e.copy(), ql=ql))
    inputs = Ref(n=n, indptr=indptr, indices=indices, lhs=lhs, c1=c1, c2=c2, c3=c3, c4_dt=c4_dt, q0=q0, lat=lat)
    return inputs, refs


@functools.lru_cache(maxsize=12)      # (tests that share a case run side by side)
def muskingum_case(net_name, regime, T, nsub):
    """Channel-only Muskingum, two consecutive calls of T output rows."""
    from oracle import oracle
    down, _, _ = network(net_name)
    n = down.size
    indptr, indices = csc_from_down(down)
    k, x, _, _ = regime_inputs(regime, net_name, 1)
    q0 = channel_state(regime, net_name)
    c1, c2, c3 = coefficients(k, x, nsub)
    lhs = np.ascontiguousarray(-c1[indices])
    q_o, q_e, refs = q0.copy(), q0.copy(), []
    for call in range(2):
        orc, exact, raw = np.zeros((T, n)), np.zeros((T, n)), np.zeros((T, n))
        oracle.muskingum_route(indptr, indices, lhs, c2, c3, q_o, orc, T, nsub)
        oracle.muskingum_route_ld(indptr, indices, lhs, c2, c3, q_e, exact, raw, T, nsub)
        refs.append(Ref(orc=orc, exact=exact, raw=raw, q_orc=q_o.copy(), q_exact=q_e.copy()))
    inputs = Ref(n=n, indptr=indptr, indices=indices, lhs=lhs, c1=c1, c2=c2, c3=c3, q0=q0)
    return inputs, refs


def unit_split(indptr, indices, n):
    """conftest.unit_split (UnitMuskingum._hook_before_route's headwater / inner split) for a helper module."""
    import scipy.sparse
    A = scipy.sparse.csc_matrix((np.ones(len(indices)), indices, indptr), shape=(n, n))
    incoming = np.asarray(A.sum(axis=1)).flatten()
    hw_idx, inner_idx = np.where(incoming == 0)[0], np.where(incoming != 0)[0]
    return hw_idx, inner_idx, A[np.ix_(inner_idx, inner_idx)].tocsc(), A[np.ix_(inner_idx, hw_idx)].tocsc()


@functools.lru_cache(maxsize=12)      # (tests that share a case run side by side)
def unit_case(net_name, regime, T, nsub, n_ks=0, f32_lat=False):
    """UnitMuskingum, two consecutive files of T rows with the router's state hand-off (inner reaches: q_full; q_ch carried).  n_ks = 0: the
    rows of lateral inflow are the regime's lat / DT.  n_ks > 0: they are the unit-hydrograph convolution of lat / DT / 1e4 (a runoff depth
    in the regime's shape) -- the fp64 oracle routes ITS convolved rows, the arbiter ITS OWN (each rounded to double once), as the fused
    GPU call routes its own; Ref.conv_orc / conv_exact hold them, Ref.uh_orc / uh_exact the carried convolution state."""
    from oracle import oracle
    from river_route_amd import synth
    down, _, _ = network(net_name)
    n = down.size
    indptr, indices = csc_from_down(down)
    hw_idx, inner_idx, A_in, A_hw = unit_split(indptr, indices, n)
    k, x, lat, _ = regime_inputs(regime, net_name, 2 * T)
    lat = lat / DT
    kern = None
    if n_ks:
        kern = synth.synth_uh_kernel(n, n_ks)
        lat = lat / 1e4
    if f32_lat:
        lat = lat.astype(np.float32).astype(np.float64)
    c1, c2, c3 = coefficients(k, x, nsub)
    c1i, c2i, c3i = c1[inner_idx], c2[inner_idx], c3[inner_idx]
    args = (A_in.indptr, A_in.indices, np.ascontiguousarray(-c1i[A_in.indices]), A_in.indptr, A_in.indices, A_in.data,
            A_hw.indptr, A_hw.indices, A_hw.data, c1i, c2i, c3i, hw_idx, inner_idx)
    ni = inner_idx.size
    qc_o, qf_o, qc_e, qf_e = (np.zeros(ni) for _ in range(4))
    uh_o = oracle.UnitHydrograph(kern) if n_ks else None
    uh_e = np.zeros_like(kern) if n_ks else None
    refs = []
    for call in range(2):
        rows = np.ascontiguousarray(lat[call * T:(call + 1) * T])
        conv_o = uh_o.convolve(rows) if n_ks else rows
        conv_e = oracle.uh_convolve_ld(kern, uh_e, rows) if n_ks else rows
        orc, exact, raw = np.zeros((T, n)), np.zeros((T, n)), np.zeros((T, n))
        oracle.unit_route(*args, qc_o, qf_o, conv_o, orc, nsub)
        oracle.unit_route_ld(*args, qc_e, qf_e, conv_e, exact, raw, nsub)
        refs.append(Ref(orc=orc, exact=exact, raw=raw, q_orc=(qc_o.copy(), qf_o.copy()), q_exact=(qc_e.copy(), qf_e.copy()), rows=rows,
                        conv_orc=conv_o, conv_exact=conv_e, uh_orc=uh_o.state.copy() if n_ks else None, uh_exact=uh_e.copy() if n_ks else None))
        # UnitMuskingum._router: the next file's channel state is this one's full discharge (q_ch = q_full = state[inner])
        qc_o, qc_e = qf_o.copy(), qf_e.copy()
    inputs = Ref(n=n, indptr=indptr, indices=indices, c1=c1, c2=c2, c3=c3, hw_idx=hw_idx, inner_idx=inner_idx, ni=ni, kern=kern, lat=lat, args=args)
    return inputs, refs
