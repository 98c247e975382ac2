"""The per-reach comparison and its arbiter, on the CPU ("Per-reach parity"; helpers in per_reach.py):
  - the long-double arbiter (oracle/rr_oracle_ld.c) is the same algorithm as the fp64 oracle: within 1e-13 of it, every reach at its
    own scale, on the golden cases of the reference and on every forcing regime of the GPU tests;
  - the regimes are what they are named for, asserted from the arbiter alone;
  - the comparison bites where conftest.assert_close does not: two planted errors at small reaches pass the whole-array tolerance
    and fail the per-reach one."""
import os
import subprocess

import numpy as np
import pytest

import per_reach as pr
from conftest import assert_close, unit_split
from oracle import oracle

PIN = 1e-13      # arbiter against fp64 oracle, per reach at the reach's own scale: the same algorithm, not merely a close one
SHAPES = [(48, 1), (24, 3)]


def test_a_platform_without_extended_precision_fails_the_build():
    """Where long double is double the arbiter would repeat the oracle and every GPU test would pass against itself: the source refuses
    to compile (gcc -mlong-double-64 makes x86 such a platform)."""
    src = os.path.join(os.path.dirname(oracle.__file__), 'rr_oracle_ld.c')
    ok = subprocess.run(['gcc', '-std=c11', '-fsyntax-only', src], capture_output=True, text=True)
    assert ok.returncode == 0, ok.stderr
    narrow = subprocess.run(['gcc', '-std=c11', '-mlong-double-64', '-fsyntax-only', src], capture_output=True, text=True)
    assert narrow.returncode != 0 and 'long double' in narrow.stderr


# ------------------------------------------------------------------------------------------------ the arbiter is the oracle's algorithm

def _pin(orc, exact, raw, what, floor=None):
    S = pr.scales(raw, floor)
    e = pr.oracle_error(pr._rows(orc), pr._rows(exact), S)
    assert e <= PIN, f'{what}: arbiter and fp64 oracle differ by {e:.3g} at a reach\'s own scale'
    return e


@pytest.mark.parametrize('tag,nsubs,n_ks_list', [('docs9', (1, 4), (1, 3)), ('tree1k', (1, 4), (3,)), ('forest30', (1, 3), (48,))])
def test_arbiter_on_the_golden_cases(golden_kernels, tag, nsubs, n_ks_list):
    """The inputs the reference itself was run on (tests/golden/kernels.npz): all three routers in long double against the fp64 oracle,
    and the clamped rows against the reference's own output at the whole-array tolerance the oracle is pinned with."""
    g = golden_kernels
    args = [g[f'{tag}/{k}'] for k in ('indptr', 'indices', 'lhs_off', 'c2', 'c3')]
    ql = g[f'{tag}/qlateral']
    T, n = ql.shape
    for nsub in nsubs:
        c4_dt = g[f'{tag}/rapid{nsub}/c4_dt']
        q_o, q_e = g[f'{tag}/q0'].copy(), g[f'{tag}/q0'].copy()
        orc, exact, raw = np.zeros((T, n)), np.zeros((T, n)), np.zeros((T, n))
        oracle.rapid_route(*args, c4_dt, q_o, ql, orc, nsub)
        oracle.rapid_route_ld(*args, c4_dt, q_e, ql, exact, raw, nsub)
        _pin(orc, exact, raw, f'{tag} rapid{nsub} discharge')
        _pin(q_o, q_e, raw, f'{tag} rapid{nsub} q_t', floor=q_e)
        assert_close(exact, g[f'{tag}/rapid{nsub}/discharge'], f'{tag} rapid{nsub} vs the reference')
        np.testing.assert_array_equal(exact, np.maximum(raw, 0.0))
        n_out = max(T // 4, 1)
        q_o, q_e = g[f'{tag}/q0'].copy(), g[f'{tag}/q0'].copy()
        orc, exact, raw = np.zeros((n_out, n)), np.zeros((n_out, n)), np.zeros((n_out, n))
        oracle.muskingum_route(*args, q_o, orc, n_out, nsub)
        oracle.muskingum_route_ld(*args, q_e, exact, raw, n_out, nsub)
        _pin(orc, exact, raw, f'{tag} musk{nsub} discharge')
        _pin(q_o, q_e, raw, f'{tag} musk{nsub} q_t', floor=q_e)
        assert_close(exact, g[f'{tag}/musk{nsub}/discharge'], f'{tag} musk{nsub} vs the reference')
    indptr, indices = g[f'{tag}/indptr'], g[f'{tag}/indices']
    hw_idx, inner_idx, A_in, A_hw = unit_split(indptr, indices, n)
    c1i, c2i, c3i = (g[f'{tag}/{c}'][inner_idx] for c in ('c1', 'c2', 'c3'))
    uargs = (A_in.indptr, A_in.indices, np.ascontiguousarray(-c1i[A_in.indices]), A_in.indptr, A_in.indices, A_in.data,
             A_hw.indptr, A_hw.indices, A_hw.data, c1i, c2i, c3i, hw_idx, inner_idx)
    for n_ks in n_ks_list:
        p = f'{tag}/unit_ks{n_ks}'
        uh = oracle.UnitHydrograph(g[f'{p}/kernel'])
        uh.state = g[f'{p}/state0'].copy()
        st_e = g[f'{p}/state0'].copy()
        conv_o = uh.convolve(g[f'{p}/depth'])
        conv_e = oracle.uh_convolve_ld(g[f'{p}/kernel'], st_e, g[f'{p}/depth'])
        _pin(conv_o, conv_e, conv_e, f'{p} convolved')
        _pin(uh.state, st_e, np.vstack([conv_e, st_e]), f'{p} convolution state')
        conv = g[f'{p}/convolved']
        for nsub in nsubs:
            qc_o, qf_o, qc_e, qf_e = (g[f'{tag}/q0'][inner_idx].copy() for _ in range(4))
            orc, exact, raw = np.zeros_like(conv), np.zeros_like(conv), np.zeros_like(conv)
            oracle.unit_route(*uargs, qc_o, qf_o, conv, orc, nsub)
            oracle.unit_route_ld(*uargs, qc_e, qf_e, conv, exact, raw, nsub)
            _pin(orc, exact, raw, f'{p} nsub{nsub} discharge')
            _pin(qc_o, qc_e, raw[:, inner_idx], f'{p} nsub{nsub} q_ch', floor=qc_e)
            _pin(qf_o, qf_e, raw[:, inner_idx], f'{p} nsub{nsub} q_full', floor=qf_e)
            np.testing.assert_array_equal(exact[:, hw_idx], conv[:, hw_idx])      # headwaters: the lateral rows as they are
            assert_close(exact, g[f'{p}/nsub{nsub}/discharge'], f'{p} nsub{nsub} vs the reference')


@pytest.mark.parametrize('ci', range(5))
def test_arbiter_convolution_on_the_golden_cases(golden_kernels, ci):
    """UnitHydrograph.convolve incl. T < n_ks, n_ks = 1 and the state carried across two calls."""
    g = golden_kernels
    uh = oracle.UnitHydrograph(g[f'conv{ci}/kernel'])
    uh.state = g[f'conv{ci}/state0'].copy()
    st_e = g[f'conv{ci}/state0'].copy()
    for leg in 'ab':
        out_o = uh.convolve(g[f'conv{ci}/lat_{leg}'])
        out_e = oracle.uh_convolve_ld(g[f'conv{ci}/kernel'], st_e, g[f'conv{ci}/lat_{leg}'])
        _pin(out_o, out_e, out_e, f'conv{ci} {leg} rows')
        _pin(uh.state, st_e, np.vstack([out_e, st_e]), f'conv{ci} {leg} state')
        np.testing.assert_allclose(out_e, g[f'conv{ci}/out_{leg}'], rtol=0, atol=1e-12)
        np.testing.assert_allclose(st_e, g[f'conv{ci}/state_{leg}'], rtol=0, atol=1e-12)


# ------------------------------------------------------------------------------------------------ the regimes

@pytest.mark.parametrize('T,nsub', SHAPES)
@pytest.mark.parametrize('regime', pr.REGIMES)
def test_regimes_are_what_they_claim(regime, T, nsub):
    """n = 6,000 reaches in random order, 48 rows at one sub-step and 24 at three, a cold start: each regime's named property from the
    arbiter's first call alone; in both calls the fp64 oracle stays within 1e-13 of the arbiter per reach (the same algorithm) and
    E_orc -- the unit of every GPU bound -- below 1e-11, so the bound never drifts towards the old whole-array one."""
    inp, refs = pr.rapid_case('random', regime, T, nsub)
    r = refs[0]
    S = pr.scales(r.raw)
    live = S > 0
    neg_c3 = float(np.mean(inp.c3 < 0))
    clamped = float(np.mean(r.raw < 0))
    span = float(S[live].max() / S[live].min())
    print(f'{regime}, T {T} x {nsub}: c3 < 0 at {neg_c3:.3f} of reaches, {clamped:.4f} of elements clamped, scale span {span:.3g}, '
          f'{int((~live).sum())} dry columns, E_orc {pr.oracle_error(r.orc, r.exact, S):.3g}')
    np.testing.assert_array_equal(r.exact, np.maximum(r.raw, 0.0) + 0.0)
    if regime == 'synth params':
        assert neg_c3 == 0.0 and clamped < 0.01 and span < 1e3      # the benign regime every other test draws from
    elif regime == 'short reaches':
        if nsub == 1:
            assert neg_c3 >= 0.30 and clamped >= 0.01
        else:      # DT / 3 = 300 s = k: c3 >= 0 at every reach
            assert neg_c3 == 0.0 and clamped > 0.0
    elif regime == 'wild k, x':
        assert neg_c3 >= 0.15
    elif regime == 'ten decades':
        assert span >= 1e6
    elif regime == 'signed':
        assert 0.01 <= clamped <= 0.50
    elif regime == 'signed, ten decades, wild k':
        assert span >= 1e9 and 0.10 <= clamped <= 0.50
    elif regime == 'half dry':
        assert int((~live).sum()) >= 1000
        assert not r.exact[:, ~live].any() and not np.signbit(r.exact[:, ~live]).any()
    for call, r in enumerate(refs):
        e = _pin(r.orc, r.exact, r.raw, f'{regime} call {call} discharge')
        _pin(r.q_orc, r.q_exact, r.raw, f'{regime} call {call} q_t', floor=r.q_exact)
        assert e <= 1e-11


@pytest.mark.parametrize('T,nsub', SHAPES)
@pytest.mark.parametrize('regime', pr.REGIMES)
def test_arbiter_on_the_regimes_muskingum_and_unit(regime, T, nsub):
    """The other three loops on the same regimes: channel-only Muskingum, UnitMuskingum on rows of lateral inflow, and the
    unit-hydrograph convolution (12 steps) with UnitMuskingum behind it."""
    for what, (inp, refs) in (('muskingum', pr.muskingum_case('random', regime, T, nsub)), ('unit', pr.unit_case('random', regime, T, nsub)),
                              ('unit after convolution', pr.unit_case('random', regime, T, nsub, n_ks=12))):
        for call, r in enumerate(refs):
            S = pr.scales(r.raw)
            assert _pin(r.orc, r.exact, r.raw, f'{what}, {regime}, call {call} discharge') <= 1e-11
            if what == 'muskingum':
                _pin(r.q_orc, r.q_exact, r.raw, f'{what}, {regime}, call {call} q_t', floor=r.q_exact)
            else:
                for nm, qo, qe in zip(('q_ch', 'q_full'), r.q_orc, r.q_exact):
                    _pin(qo, qe, r.raw[:, inp.inner_idx], f'{what}, {regime}, call {call} {nm}', floor=qe)
                np.testing.assert_array_equal(r.exact[:, inp.hw_idx], r.conv_exact[:, inp.hw_idx])
            if what == 'unit after convolution':
                _pin(r.conv_orc, r.conv_exact, r.conv_exact, f'{regime}, call {call} convolved rows')
                _pin(r.uh_orc, r.uh_exact, np.vstack([r.conv_exact, r.uh_exact]), f'{regime}, call {call} convolution state')
            assert S.shape == (inp.n,)


# ------------------------------------------------------------------------------------------------ the comparison bites

@pytest.fixture(scope='module')
def filled():
    """The benign regime once the outlet has filled (1,500 rows of spin-up: the outlet carries the basin's whole inflow, ~3,000 against a
    headwater's ~0.5), then 48 rows: fp64 oracle, arbiter, and what the planted errors need."""
    from river_route_amd import synth
    inp, _ = pr.rapid_case('random', 'synth params', 48, 1)
    n, T, spin = inp.n, 48, 1500
    a = (inp.indptr, inp.indices, inp.lhs, inp.c2, inp.c3, inp.c4_dt)
    q0 = np.zeros(n)
    oracle.rapid_route(*a, q0, synth.synth_qlateral(n, 1000, 1000 + spin), np.zeros((spin, n)), 1)
    ql = synth.synth_qlateral(n, 0, T)
    q_o, q_e = q0.copy(), q0.copy()
    orc, exact, raw = np.zeros((T, n)), np.zeros((T, n)), np.zeros((T, n))
    oracle.rapid_route(*a, q_o, ql, orc, 1)
    oracle.rapid_route_ld(*a, q_e, ql, exact, raw, 1)
    return dict(a=a, c4_dt=inp.c4_dt, q0=q0, ql=ql, orc=orc, exact=exact, raw=raw, S=pr.scales(raw))


def test_the_oracle_passes_its_own_bound(filled):
    f = filled
    assert f['S'].max() / f['S'].min() > 1e3
    assert pr.assert_per_reach(f['orc'], f['orc'], f['exact'], f['raw'], 'the oracle itself') <= 1.0
    assert pr.assert_per_reach(f['exact'], f['orc'], f['exact'], f['raw'], 'the arbiter itself') == 0.0


def test_one_small_column_off_by_1e_9_passes_assert_close_and_fails_per_reach(filled):
    f = filled
    bad = f['orc'].copy()
    bad[:, int(np.argmin(f['S']))] *= 1.0 + 1e-9
    assert_close(bad, f['orc'], 'whole-array tolerance')
    with pytest.raises(AssertionError, match='x the fp64 oracle\'s own error'):
        pr.assert_per_reach(bad, f['orc'], f['exact'], f['raw'], 'planted: smallest column x (1 + 1e-9)')


def test_a_float32_lateral_term_at_small_reaches_passes_assert_close_and_fails_per_reach(filled):
    """c4_dt ql rounded through float32 at the reaches whose scale is below 1 % of the largest: what a kernel that takes one value through
    float32 somewhere does to its small reaches.  (Planted through the input: ql' = float32(c4_dt ql) / c4_dt, the same term to an ulp.)"""
    f = filled
    small = f['S'] < 0.01 * f['S'].max()
    assert 0.5 < small.mean() < 1.0
    term32 = (f['c4_dt'][None, :] * f['ql']).astype(np.float32).astype(np.float64)
    ql = f['ql'].copy()
    ql[:, small] = (term32 / f['c4_dt'][None, :])[:, small]
    q, bad = f['q0'].copy(), np.zeros_like(f['orc'])
    oracle.rapid_route(*f['a'], q, ql, bad, 1)
    assert_close(bad, f['orc'], 'whole-array tolerance')
    with pytest.raises(AssertionError, match='x the fp64 oracle\'s own error'):
        pr.assert_per_reach(bad, f['orc'], f['exact'], f['raw'], 'planted: float32 lateral term at small reaches')


def test_dry_columns_nans_and_float32_rows():
    """The other clauses of the rule: a column that carries nothing holds +0.0 (not -0.0, not 1e-300); NaNs where the arbiter's are and
    nowhere else; a float32 row may be one float32 rounding away from the float64 bound and no more."""
    _, refs = pr.rapid_case('random', 'half dry', 24, 3)
    r = refs[0]
    S = pr.scales(r.raw)
    dry = int(np.flatnonzero(S == 0)[0])
    assert pr.assert_per_reach(r.orc, r.orc, r.exact, r.raw, 'oracle') <= 1.0
    for v in (-0.0, 1e-300):
        bad = r.orc.copy()
        bad[3, dry] = v
        with pytest.raises(AssertionError, match='other than \\+0.0'):
            pr.assert_per_reach(bad, r.orc, r.exact, r.raw, 'dry column')
    bad = r.orc.copy()
    bad[5, 17] = np.nan
    with pytest.raises(AssertionError, match='NaN pattern'):
        pr.assert_per_reach(bad, r.orc, r.exact, r.raw, 'a NaN')
    got32 = r.orc.astype(np.float32)
    assert pr.assert_per_reach_f32(got32, r.orc, r.exact, r.raw, 'float32 rows') <= 1.0
    wet = int(np.argmax(S))
    off = got32.copy()
    off[7, wet] = np.nextafter(np.nextafter(off[7, wet], np.float32(np.inf)), np.float32(np.inf))      # two float32 ulps: more than one rounding
    with pytest.raises(AssertionError, match='float32 elements beyond'):
        pr.assert_per_reach_f32(off, r.orc, r.exact, r.raw, 'float32 rows, one value two ulps off')
    with pytest.raises(AssertionError, match='other than \\+0.0'):
        z = got32.copy()
        z[0, dry] = -0.0
        pr.assert_per_reach_f32(z, r.orc, r.exact, r.raw, 'float32 dry column')
