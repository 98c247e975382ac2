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
kernel that also sums a reach's tributaries in another order.

The second half of the module is the same for the routing gradients (test_adjoint_oracle.py on the CPU, test_gpu_grad_per_reach.py on
the GPU box): the per-element rule against the adjoint arbiter (oracle/rr_oracle_adj.c), the chain to dL/dk and
dL/dx, and the one table of cases both files run."""
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
    elif name == 'synth20k':
        net = synth.synth_network(20_000, seed=23)
    elif name == 'synth524544':      # 2,049 column blocks of 256: the adjoint's reduction has one sub-step range
        net = synth.synth_network(524_544, seed=25)
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
        elif name == 'y3':          # two reaches into one
            down = np.array([2, 2, -1], dtype=np.int64)
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


# ------------------------------------------------------------------------------------------------ gradients
# The routing adjoints against the adjoint arbiter (oracle/rr_oracle_adj.c), every output element at ITS OWN scale: the arbiter
# returns, next to each gradient, the sum of the absolute values of the terms that were added to make it.  With `exact` the
# long-double result, `scale` that array and `orc` the fp64 build of the same loops:  E_orc = max |orc - exact| / scale over
# scale > 0, recomputed in every test;  got passes when |got - exact| <= K_ADJ max(E_orc, 2^-52) scale at every element, is 0 where
# scale == 0 and has its NaNs where the arbiter has them.  K_ADJ is measured, not chosen: test_adjoint_oracle.py builds the fp64 loops
# a second time in the reverse summation order with fused multiply-adds and asserts that K_ADJ follows from the worst ratio by the
# rule of section 2c.

K_ADJ = 32.0
DT_RUNOFF = 3600.0
ADJ_TARGET_BLOCKS, ADJ_BLOCK = 2048, 256      # rr_adjoint.hpp: kAdjTargetBlocks; rr_common.hpp: kBlock


def element_error(orc, exact, scale):
    """E_orc of the rule above for one output array."""
    live = scale > 0
    if not live.any():
        return 0.0
    with np.errstate(invalid='ignore'):
        r = np.abs(np.asarray(orc)[live] - exact[live]) / scale[live]
    return float(np.nanmax(r, initial=0.0))


def assert_per_element(got, orc, exact, scale, what, K=K_ADJ):
    """The rule of DESIGN.md section 2c.  Returns the worst |got - exact| / (max(E_orc, 2^-52) scale)."""
    got, orc, exact, scale = (np.asarray(a, dtype=np.float64) for a in (got, orc, exact, scale))
    assert got.shape == orc.shape == exact.shape == scale.shape, f'{what}: shapes {got.shape}, {orc.shape}, {exact.shape}, {scale.shape}'
    unit = max(element_error(orc, exact, scale), EPS)
    assert np.array_equal(np.isnan(got), np.isnan(exact)), f'{what}: NaN pattern differs from the arbiter\'s'
    dead = scale == 0
    assert not got[dead].any(), f'{what}: {int(np.count_nonzero(got[dead]))} nonzero values where the gradient is structurally zero'
    live = ~dead & ~np.isnan(exact)
    if not live.any():
        return 0.0
    ratio = np.abs(got[live] - exact[live]) / scale[live] / unit
    w = int(np.argmax(ratio))
    at = tuple(int(v[w]) for v in np.nonzero(live))
    assert ratio[w] <= K, (f'{what}: element {at} is off by {ratio[w]:.3g} x the fp64 arbiter\'s own error at the element\'s scale '
                           f'(got {got[at]:.17g}, exact {exact[at]:.17g}, scale {scale[at]:.3g}, E_orc {unit:.3g}; allowed {K:g} x)')
    return float(ratio[w])


def coefficient_jacobian(k, x, dt, with_c4=True, dt_runoff=DT_RUNOFF):
    """(dc/dk, dc/dx), each [4 or 3, n]: the derivatives of c1, c2, c3 (and c4dt = (c1 + c2) / dt_runoff) of a reach by its own k, x,
    from rr.grad.muskingum_coefficients under torch autograd on the host."""
    import torch
    import river_route_amd as rr
    rows_k, rows_x = [], []
    for j in range(4 if with_c4 else 3):
        kt, xt = torch.tensor(np.asarray(k), requires_grad=True), torch.tensor(np.asarray(x), requires_grad=True)
        c = rr.grad.muskingum_coefficients(kt, xt, dt)
        cj = (c[0] + c[1]) / dt_runoff if j == 3 else c[j]
        gk, gx = torch.autograd.grad(cj.sum(), (kt, xt))
        rows_k.append(gk.numpy())
        rows_x.append(gx.numpy())
    return np.stack(rows_k), np.stack(rows_x)


def chain_to_kx(jac, grad_coef, scale_coef):
    """dL/dk (or dL/dx) = sum_j dL/dc_j dc_j/dk and its scale sum_j scale_cj |dc_j/dk|."""
    return (grad_coef * jac).sum(axis=0), (scale_coef * np.abs(jac)).sum(axis=0)


def adjoint_splits(n, T, nsub, members=1):
    """(splits, steps_per_split) of the adjoints' reduction: the arithmetic of adjoint_layout (rr_adjoint.hpp), restated."""
    S = T * nsub
    col_blocks = -(-n // ADJ_BLOCK) * members
    want = max(1, -(-ADJ_TARGET_BLOCKS // col_blocks))
    splits = max(1, min(want, S))
    steps = -(-S // splits)
    return -(-S // steps), steps


# name: (network, T, nsub, members, (splits, steps_per_split) expected, regimes)
ADJ_CASES = {
    'ragged ranges': ('random', 353, 1, 1, (71, 5), ('benign', 'clamp')),
    'ranges across rows': ('chain', 500, 3, 1, (167, 9), ('benign', 'clamp')),
    'one range': ('synth524544', 6, 1, 1, (1, 6), ('benign', 'clamp')),
    'fan-in star': ('star', 40, 2, 1, (80, 1), ('benign', 'clamp')),
    'fan-in comb': ('comb', 40, 2, 1, (80, 1), ('benign', 'clamp')),
    'fan-in wide': ('wide', 40, 2, 1, (80, 1), ('benign', 'clamp')),
    'no edges': ('lone', 40, 2, 1, (80, 1), ('benign',)),
    'long record': ('y3', 65_552, 1, 1, (1987, 33), ('benign',)),      # the smallest T above 65,535 + 16
    'batch': ('synth20k', 48, 2, 4, (7, 14), ('benign',)),
    'partial losses': ('random', 2, 3, 1, (6, 1), ('benign',)),      # run with the losses 'channel', 'final', 'outlet' only
}


def adjoint_inputs(case, regime, member=0, loss='both'):
    """(k, x, ql, q0, G, Gf) of a case: the draws of test_gpu_grad.py (lateral volumes per DT_RUNOFF from `low` upward, a state in
    [0, 3], standard-normal cotangents); 'clamp' is its clamp / negative-c3 draw (k[::3] = 300, lateral from -1.5) with a zero-mean lateral."""
    net_name, T, nsub, _, _, _ = ADJ_CASES[case]
    down, k, x = network(net_name)
    n = down.size
    k = k.copy()
    low, high = 0.0, 2.0
    if regime == 'clamp':      # (up to 1.5, not 2: with a positive mean the inflow that gathers along a chain keeps all but its head above zero)
        k[::3] = 300.0
        low, high = -1.5, 1.5
    else:
        assert regime == 'benign', regime
    seed = sum(map(ord, case)) * 7 + (1 if regime == 'clamp' else 0) + 1000 * member
    rng = np.random.default_rng(seed)
    ql = rng.uniform(low, high, (T, n)) * DT_RUNOFF
    q0 = rng.uniform(0.0, 3.0, n)
    G, Gf = rng.standard_normal((T, n)), rng.standard_normal(n)
    return k, x, ql, q0, G, Gf


class AdjRef(Ref):
    pass


def rapid_adjoint_refs(indptr, indices, c, q0, ql, G, Gf, nsub, T=None):
    """(orc, exact) of one RapidMuskingum adjoint call: the fp64 and the long-double run of the arbiter."""
    from oracle import oracle
    args = (indptr, indices, c[0], c[1], c[2], c[3], q0, ql, G, Gf, nsub, T)
    return oracle.rapid_adjoint(*args), oracle.rapid_adjoint_ld(*args)


N_GAUGES = 37


def gauge_columns(case):
    """37 gauged reaches of a case, in no order: headwaters and inner reaches among them, the outlet (the last reach) the first."""
    down = network(ADJ_CASES[case][0])[0]
    n = down.size
    inner = inner_reaches(down)
    hw = np.setdiff1d(np.arange(n), inner)
    rng = np.random.default_rng(37)
    g = np.concatenate([[n - 1], rng.choice(hw, 12, replace=False), rng.choice(inner[inner != n - 1], N_GAUGES - 13, replace=False)])
    assert np.unique(g).size == N_GAUGES
    g[1:] = rng.permutation(g[1:])
    return g.astype(np.int32)


def gauge_cotangent(case, G):
    """dL/ddischarge of a gauge loss at full width: zero off the gauge columns."""
    G0 = np.zeros_like(G)
    g = gauge_columns(case)
    G0[:, g] = G[:, g]
    return G0


@functools.lru_cache(maxsize=6)
def rapid_adjoint_case(case, regime, member=0, loss='both', shared=False):
    """Inputs and references of a RapidMuskingum case, computed once.  loss: 'both' (dL/ddischarge and dL/dq_final), 'final' (dL/dq_final
    alone), 'outlet' (dL/ddischarge in the last row at the last reach alone), 'channel' (no laterals), 'gauges' (dL/ddischarge at
    gauge_columns alone, and dL/dq_final).  shared: the member starts from member 0's state."""
    net_name, T, nsub, _, _, _ = ADJ_CASES[case]
    down = network(net_name)[0]
    indptr, indices = csc_from_down(down)
    k, x, ql, q0, G, Gf = adjoint_inputs(case, regime, member)
    if shared:
        q0 = adjoint_inputs(case, regime, 0)[3]
    if loss == 'gauges':
        G = gauge_cotangent(case, G)
    if loss == 'final':
        G = None
    elif loss == 'outlet':
        G0 = np.zeros_like(G)
        G0[-1, -1] = G[-1, -1]
        G, Gf = G0, None
    elif loss == 'channel':
        ql = None
    c1, c2, c3 = coefficients_at(k, x, DT_RUNOFF / nsub)
    c = np.stack([c1, c2, c3, (c1 + c2) / DT_RUNOFF])
    orc, exact = rapid_adjoint_refs(indptr, indices, c, q0, ql, G, Gf, nsub, T)
    return AdjRef(n=down.size, T=T, nsub=nsub, indptr=indptr, indices=indices, k=k, x=x, c=c, ql=ql, q0=q0, G=G, Gf=Gf, orc=orc, exact=exact)


def coefficients_at(k, x, dt):
    from oracle import oracle
    return oracle.muskingum_coefficients(k, x, dt)


def rapid_outputs(r):
    """[(name, orc, exact, scale)] of a rapid_adjoint_case."""
    out = [(f'dL/dc{j + 1}' if j < 3 else 'dL/dc4dt', r.orc.grad_coef[j], r.exact.grad_coef[j], r.exact.scale_coef[j]) for j in range(4)]
    out.append(('dL/dq0', r.orc.grad_q0, r.exact.grad_q0, r.exact.scale_q0))
    if r.ql is not None:
        out.append(('dL/dlateral', r.orc.grad_lateral, r.exact.grad_lateral, r.exact.scale_lateral))
    return out


def forward_margin(orc_raw, exact_raw):
    """The clamp condition of section 2c: the number of elements whose unclamped mean sits within the forward rule's bound of zero without
    being zero, 0 < |raw| <= K E_orc,fwd S_j (K = 16, the forward rule's), and the share of elements the clamp is active on."""
    S = scales(exact_raw)
    e_fwd = max(oracle_error(orc_raw, exact_raw, S), EPS)
    near = (np.abs(exact_raw) > 0) & (np.abs(exact_raw) <= K * e_fwd * S[None, :])
    return int(near.sum()), float((exact_raw <= 0).mean())


def inner_reaches(down):
    """The inner reaches (those with tributaries) in ascending params order: the index of UnitMuskingum's states."""
    has_up = np.zeros(down.size, dtype=bool)
    has_up[down[down >= 0]] = True
    return np.flatnonzero(has_up)


def unit_adjoint_inputs(case, regime, member=0):
    """(k, x, lat, q_ch0, q_full0, G, Gc, Gf) of a case: the draws of test_grad_unit.unit_inputs (lateral inflow from `low` x 50 upward,
    states in [0, 80] and [0, 120], standard-normal cotangents) in the regimes of adjoint_inputs."""
    net_name, T, nsub, _, _, _ = ADJ_CASES[case]
    down, k, x = network(net_name)
    n, ni = down.size, inner_reaches(down).size
    k = k.copy()
    low, high = 0.0, 2.0
    if regime == 'clamp':
        k[::3] = 300.0
        low, high = -1.5, 1.5
    else:
        assert regime == 'benign', regime
    rng = np.random.default_rng(sum(map(ord, case)) * 11 + (1 if regime == 'clamp' else 0) + 1000 * member + 5)
    return (k, x, rng.uniform(low, high, (T, n)) * 50.0, rng.uniform(0.0, 80.0, ni), rng.uniform(0.0, 120.0, ni),
            rng.standard_normal((T, n)), rng.standard_normal(ni), rng.standard_normal(ni))


@functools.lru_cache(maxsize=6)
def unit_adjoint_case(case, regime, member=0, loss='both', shared=False):
    """Inputs and references of a UnitMuskingum case, computed once.  loss: 'both' (all three cotangents), 'final' (those of the final
    states alone), 'outlet' (dL/ddischarge in the last row at the last reach alone), 'gauges' (dL/ddischarge at gauge_columns alone, and
    those of the final states).  shared: the member starts from member 0's states."""
    from oracle import oracle
    net_name, T, nsub, _, _, _ = ADJ_CASES[case]
    down = network(net_name)[0]
    indptr, indices = csc_from_down(down)
    k, x, lat, qc0, qf0, G, Gc, Gf = unit_adjoint_inputs(case, regime, member)
    if shared:
        qc0, qf0 = unit_adjoint_inputs(case, regime, 0)[3:5]
    if loss == 'gauges':
        G = gauge_cotangent(case, G)
    if loss == 'final':
        G = None
    elif loss == 'outlet':
        G0 = np.zeros_like(G)
        G0[-1, -1] = G[-1, -1]
        G, Gc, Gf = G0, None, None
    c = np.stack(coefficients_at(k, x, DT_RUNOFF / nsub))
    args = (indptr, indices, c[0], c[1], c[2], qc0, qf0, lat, G, Gc, Gf, nsub)
    return AdjRef(n=down.size, ni=qc0.size, inner=inner_reaches(down), T=T, nsub=nsub, indptr=indptr, indices=indices, k=k, x=x, c=c, lat=lat,
                  q_ch0=qc0, q_full0=qf0, G=G, Gc=Gc, Gf=Gf, orc=oracle.unit_adjoint(*args), exact=oracle.unit_adjoint_ld(*args))


def unit_outputs(r):
    """[(name, orc, exact, scale)] of a unit_adjoint_case."""
    out = [(f'dL/dc{j + 1}', r.orc.grad_coef[j], r.exact.grad_coef[j], r.exact.scale_coef[j]) for j in range(3)]
    return out + [('dL/dq_ch0', r.orc.grad_qch0, r.exact.grad_qch0, r.exact.scale_qch0),
                  ('dL/dq_full0', r.orc.grad_qfull0, r.exact.grad_qfull0, r.exact.scale_qfull0),
                  ('dL/dlateral', r.orc.grad_lateral, r.exact.grad_lateral, r.exact.scale_lateral)]


def member_sum(rows):
    """The members' coefficient rows summed in member order in long double, rounded once."""
    acc = np.zeros(rows[0].shape, dtype=np.longdouble)
    for r in rows:
        acc = acc + r
    return acc.astype(np.float64)


def every_case():
    """(case, regime, member, loss, shared) of every definition of the table: each case in its regimes (a batch: every member, with its
    own state and with the shared one), the gauge losses on the ragged-ranges case and the partial losses on the fan-in comb."""
    out = []
    for case, (_, _, _, members, _, regimes) in ADJ_CASES.items():
        for regime in regimes if case != PARTIAL_CASE else ():
            for m in range(members):
                out.append((case, regime, m, 'both', False))
                if members > 1 and m:
                    out.append((case, regime, m, 'both', True))
    out += [('ragged ranges', 'benign', m, 'gauges', False) for m in range(3)]
    out += [(PARTIAL_CASE, 'benign', 0, loss, False) for loss in ('channel', 'final', 'outlet')]
    return out


PARTIAL_CASE = 'partial losses'


def adjoint_work_bytes(n, depth, T, nsub, router, members=1, n_gauges=0, grad_rows=True):
    """What the sizers of the adjoint calls return (include/rr_hip.h), from adjoint_splits: a sizer that answers this number laid its
    reduction out in the sub-step ranges the case table says."""
    S = T * nsub
    splits, _ = adjoint_splits(n, T, nsub, members)
    slab_rows, scratch_rows = (4, 2) if router == 'rapid' else (3, 6)
    per_member = 2 * S + 2 * depth + (2 if grad_rows else 1) * T + slab_rows * splits + scratch_rows
    return 8 * (n * members * per_member + max(n * min(T, 16), members * T * n_gauges))
