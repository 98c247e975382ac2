"""Per-reach parity of every routing path ("Per-reach parity"; the rule and the references are in per_reach.py): each
GPU path against the long-double arbiter with every reach at its OWN scale, in units of the fp64 oracle's own error on the same case
(K = 16), where the other GPU tests allow 1e-10 of the largest river.  Small networks that still have many tiles and levels
(6,000 reaches; degenerate shapes of 777 ... 5,001), at most 48 rows, one and three sub-steps, two consecutive calls with the state
handed over.  Every case forces its path with the RR_* knobs (read when a plan is made), asserts the kernel that ran, and prints
its ratio: `pytest -s` shows the table DESIGN.md holds."""
import numpy as np
import pytest

import per_reach as pr
from river_route_amd.engine import DeviceBuffer, Plan, uh_convolve

pytestmark = pytest.mark.gpu

KNOBS = ('RR_WAVE', 'RR_WAVE_K', 'RR_TILE_BLOCK', 'RR_TILE_LEAN', 'RR_UH_PAIRS', 'RR_DIRECT', 'RR_HW_INPASS', 'RR_REC_BATCHES')
SHAPES = [(48, 1), (24, 3)]
HOST_PATHS = {'k_tick': {'RR_WAVE': '0'}, 'k_tile': {'RR_WAVE': '1'}, 'k_tile block 64 K 16': {'RR_WAVE': '1', 'RR_TILE_BLOCK': '64', 'RR_WAVE_K': '16'},
              'k_tile general tick': {'RR_WAVE': '1', 'RR_TILE_LEAN': '0'}, 'k_tile short tick': {'RR_WAVE': '1', 'RR_TILE_LEAN': '1'}}
MUSK_REGIMES = tuple(r for r in pr.REGIMES if r != 'signed')      # (without laterals 'signed' is 'synth params': per_reach.channel_state)


def set_env(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def host_cases(regimes=pr.REGIMES):
    """Every regime on the streaming kernel and on default k_tile, the core three on the other shapes of k_tile (the paths of one
    case side by side: they share its references)."""
    return [(path, regime, T, nsub) for regime in regimes for T, nsub in SHAPES for path in HOST_PATHS
            if path in ('k_tick', 'k_tile') or regime in pr.CORE]


def report(path, mode, net, regime, T, nsub, ratios):
    print(f'\nper-reach ratio | {path} | {mode} | {net} | {regime} | T {T} x {nsub} | ' + ' '.join(f'{k} {v:.2f}' for k, v in ratios.items()))


def check_rapid(got_rows, got_q, r, what, ratios, call):
    ratios[f'rows{call}'] = pr.assert_per_reach(got_rows, r.orc, r.exact, r.raw, f'{what}, call {call}: discharge')
    ratios[f'q{call}'] = pr.assert_per_reach(got_q, r.q_orc, r.q_exact, r.raw, f'{what}, call {call}: q_t', floor=r.q_exact)


def check_unit(got_rows, got_qc, got_qf, inp, r, conv_rows, what, ratios, call):
    """Headwater columns are the lateral rows bit for bit (unclamped, un-averaged); inner columns and both states per reach."""
    np.testing.assert_array_equal(got_rows[:, inp.hw_idx], conv_rows[:, inp.hw_idx], err_msg=f'{what}, call {call}: headwater columns')
    ii = inp.inner_idx
    ratios[f'rows{call}'] = pr.assert_per_reach(got_rows[:, ii], r.orc[:, ii], r.exact[:, ii], r.raw[:, ii], f'{what}, call {call}: inner discharge')
    ratios[f'qch{call}'] = pr.assert_per_reach(got_qc, r.q_orc[0], r.q_exact[0], r.raw[:, ii], f'{what}, call {call}: q_ch', floor=r.q_exact[0])
    ratios[f'qfull{call}'] = pr.assert_per_reach(got_qf, r.q_orc[1], r.q_exact[1], r.raw[:, ii], f'{what}, call {call}: q_full', floor=r.q_exact[1])


def expected_host_kernel(plan, env):
    """RR_WAVE=1 takes the time-tiled kernel wherever the network tiles (a reach with more tributaries than a tile holds does not)."""
    return 'tile' if env.get('RR_WAVE') == '1' and plan.tile_info()['ok'] else 'tick'


# ------------------------------------------------------------------------------------------------ host entry points: k_tick, k_tile

def _host_rapid(monkeypatch, path, net, regime, T, nsub, tiled=None):
    env = HOST_PATHS[path]
    set_env(monkeypatch, env)
    inp, refs = pr.rapid_case(net, regime, T, nsub)
    ratios = {}
    with Plan(inp.indptr, inp.indices) as plan:
        plan.set_coeffs(inp.lhs, inp.c2, inp.c3, inp.c4_dt)
        want = expected_host_kernel(plan, env)
        if tiled is not None:
            assert (want == 'tile') == tiled, f'{net}: tile_info {plan.tile_info()}'
        q = inp.q0.copy()
        for call, r in enumerate(refs):
            d = np.full((T, inp.n), -1.0)
            plan.rapid_route(q, r.ql, d, nsub)
            assert plan.last_kernel() == want
            check_rapid(d, q, r, f'{path}, {net}, {regime}', ratios, call)
    report(path, 'rapid', net, regime, T, nsub, ratios)


@pytest.mark.parametrize('path,regime,T,nsub', host_cases())
def test_rapid_host(monkeypatch, path, regime, T, nsub):
    _host_rapid(monkeypatch, path, 'random', regime, T, nsub, tiled=path != 'k_tick')


@pytest.mark.parametrize('path', ['k_tick', 'k_tile'])
@pytest.mark.parametrize('T,nsub', SHAPES)
@pytest.mark.parametrize('regime', pr.CORE)
@pytest.mark.parametrize('net,tiles', [('chain97', True), ('wide', True), ('chain', True), ('comb', True), ('star', False), ('lone', True)])
def test_rapid_host_other_networks(monkeypatch, net, tiles, path, regime, T, nsub):
    """Chain-grown (long in-degree-1 runs, three-way confluences, seven outlets), fan-8 (confluences of four and more: the general
    kernel's companion launch), and the extremes: one chain of 3,000, a comb of 2 x 1,500, a star of 5,000 tributaries (more than a tile
    holds: it streams whatever RR_WAVE says), 777 unconnected reaches."""
    _host_rapid(monkeypatch, path, net, regime, T, nsub, tiled=tiles and path != 'k_tick')


@pytest.mark.parametrize('path,regime,T,nsub', host_cases(MUSK_REGIMES))
def test_muskingum_host(monkeypatch, path, regime, T, nsub):
    env = HOST_PATHS[path]
    set_env(monkeypatch, env)
    inp, refs = pr.muskingum_case('random', regime, T, nsub)
    ratios = {}
    with Plan(inp.indptr, inp.indices) as plan:
        plan.set_coeffs(inp.lhs, inp.c2, inp.c3, None)
        q = inp.q0.copy()
        for call, r in enumerate(refs):
            d = np.full((T, inp.n), -1.0)
            plan.muskingum_route(q, d, T, nsub)
            assert plan.last_kernel() == ('tick' if path == 'k_tick' else 'tile')
            check_rapid(d, q, r, f'{path}, muskingum, {regime}', ratios, call)
    report(path, 'muskingum', 'random', regime, T, nsub, ratios)


@pytest.mark.parametrize('path,regime,T,nsub', host_cases())
def test_unit_host(monkeypatch, path, regime, T, nsub):
    env = HOST_PATHS[path]
    set_env(monkeypatch, env)
    inp, refs = pr.unit_case('random', regime, T, nsub)
    ratios = {}
    with Plan(inp.indptr, inp.indices) as plan:
        plan.set_coeffs(np.ascontiguousarray(-inp.c1[inp.indices]), inp.c2, inp.c3, None)
        qc, qf = np.zeros(inp.ni), np.zeros(inp.ni)
        for call, r in enumerate(refs):
            d = np.full((T, inp.n), -1.0)
            plan.unit_route(qc, qf, r.rows, d, nsub)
            assert plan.last_kernel() == ('tick' if path == 'k_tick' else 'tile')
            check_unit(d, qc, qf, inp, r, r.rows, f'{path}, unit, {regime}', ratios, call)
            qc = qf.copy()      # UnitMuskingum._router's hand-off
    report(path, 'unit', 'random', regime, T, nsub, ratios)


# ------------------------------------------------------------------------------------------------ device entry points: records, direct rows

def _dev_rapid(plan, inp, refs, T, nsub, want_kernel, what, f32_in=False, f32_out=False):
    """Two rr_rapid_route*_dev calls; returns (ratios, [rows per call], [state per call])."""
    n = inp.n
    ratios, rows, states = {}, [], []
    d_q = DeviceBuffer(n * 8).upload(inp.q0)
    d_ql, d_out = DeviceBuffer(T * n * (4 if f32_in else 8)), DeviceBuffer(T * n * (4 if f32_out else 8))
    for call, r in enumerate(refs):
        d_ql.upload(r.ql.astype(np.float32) if f32_in else r.ql)
        d_out.upload(np.full((T, n), -1.0, dtype=np.float32 if f32_out else np.float64))
        if f32_in:
            plan.rapid_route_f32in_dev(d_q, d_ql, T, T, nsub, **(dict(discharge32=d_out, factor=1) if f32_out else dict(discharge=d_out, out_rows=T)))
        elif f32_out:
            plan.rapid_route_f32_dev(d_q, d_ql, T, d_out, T, nsub, 1)
        else:
            plan.rapid_route_dev(d_q, d_ql, T, d_out, T, T, nsub)
        assert plan.last_kernel() == want_kernel, f'{what}: ran {plan.last_kernel()}'
        d, q = d_out.download(np.float32 if f32_out else np.float64, (T, n)), d_q.download(np.float64, (n,))
        if f32_out:
            ratios[f'rows32_{call}'] = pr.assert_per_reach_f32(d, r.orc, r.exact, r.raw, f'{what}, call {call}: float32 discharge')
            ratios[f'q{call}'] = pr.assert_per_reach(q, r.q_orc, r.q_exact, r.raw, f'{what}, call {call}: q_t', floor=r.q_exact)
        else:
            check_rapid(d, q, r, what, ratios, call)
        rows.append(d)
        states.append(q)
    for b in (d_q, d_ql, d_out):
        b.free()
    return ratios, rows, states


def _dev_muskingum(plan, inp, refs, T, nsub, want_kernel, what):
    n = inp.n
    ratios, rows, states = {}, [], []
    d_q, d_out = DeviceBuffer(n * 8).upload(inp.q0), DeviceBuffer(T * n * 8)
    for call, r in enumerate(refs):
        d_out.upload(np.full((T, n), -1.0))
        plan.muskingum_route_dev(d_q, d_out, T, T, nsub)
        assert plan.last_kernel() == want_kernel, f'{what}: ran {plan.last_kernel()}'
        d, q = d_out.download(np.float64, (T, n)), d_q.download(np.float64, (n,))
        check_rapid(d, q, r, what, ratios, call)
        rows.append(d)
        states.append(q)
    d_q.free(); d_out.free()
    return ratios, rows, states


def _dev_unit(plan, inp, refs, T, nsub, want_kernel, what):
    n, ni = inp.n, inp.ni
    ratios, rows, states = {}, [], []
    d_qc, d_qf = DeviceBuffer(ni * 8).upload(np.zeros(ni)), DeviceBuffer(ni * 8).upload(np.zeros(ni))
    d_conv, d_out = DeviceBuffer(T * n * 8), DeviceBuffer(T * n * 8)
    for call, r in enumerate(refs):
        d_conv.upload(r.rows)
        d_out.upload(np.full((T, n), -1.0))
        plan.unit_route_dev(d_qc, d_qf, d_conv, T, d_out, T, T, nsub)
        assert plan.last_kernel() == want_kernel, f'{what}: ran {plan.last_kernel()}'
        d, qc, qf = d_out.download(np.float64, (T, n)), d_qc.download(np.float64, (ni,)), d_qf.download(np.float64, (ni,))
        check_unit(d, qc, qf, inp, r, r.rows, what, ratios, call)
        d_qc.upload(qf)      # UnitMuskingum._router's hand-off
        rows.append(d)
        states.append(qf)
    for b in (d_qc, d_qf, d_conv, d_out):
        b.free()
    return ratios, rows, states


def _dev_case(mode, net, regime, T, nsub):
    return {'rapid': pr.rapid_case, 'muskingum': pr.muskingum_case, 'unit': pr.unit_case}[mode](net, regime, T, nsub)


def _dev_route(mode, plan, inp, refs, T, nsub, want_kernel, what):
    if mode == 'rapid':
        plan.set_coeffs(inp.lhs, inp.c2, inp.c3, inp.c4_dt)
        return _dev_rapid(plan, inp, refs, T, nsub, want_kernel, what)
    if mode == 'muskingum':
        plan.set_coeffs(inp.lhs, inp.c2, inp.c3, None)
        return _dev_muskingum(plan, inp, refs, T, nsub, want_kernel, what)
    plan.set_coeffs(np.ascontiguousarray(-inp.c1[inp.indices]), inp.c2, inp.c3, None)
    return _dev_unit(plan, inp, refs, T, nsub, want_kernel, what)


@pytest.mark.parametrize('batches', ['1', '4'])
@pytest.mark.parametrize('inpass', ['0', '1'])
@pytest.mark.parametrize('T,nsub', SHAPES + [(48, 3)])      # 144 ticks: two record batches
@pytest.mark.parametrize('regime', pr.CORE)
@pytest.mark.parametrize('mode', ['rapid', 'muskingum', 'unit'])
def test_record_path(monkeypatch, mode, inpass, batches, regime, T, nsub):
    """k_rec_in, k_tile, k_rec_out through the device entry points on the random order: headwaters routed by the in-pass or by k_tile,
    one or four record batches per launch of the passes."""
    set_env(monkeypatch, {'RR_WAVE': '1', 'RR_HW_INPASS': inpass, 'RR_REC_BATCHES': batches})
    inp, refs = _dev_case(mode, 'random', regime, T, nsub)
    with Plan(inp.indptr, inp.indices) as plan:
        info = plan.inpass_info()
        assert info['enabled'] == (inpass == '1') and plan.tile_info()['ok'] and not plan.direct_info()['ok']
        what = f'records in-pass {inpass} batches {batches}, {mode}, {regime}'
        ratios, _, _ = _dev_route(mode, plan, inp, refs, T, nsub, 'tile', what)
        assert plan.inpass_info()['eligible'] > 0      # (with the coefficients set: the headwaters k_rec_in may route)
    report(f'records in-pass {inpass} batches {batches}', mode, 'random', regime, T, nsub, ratios)


@pytest.mark.parametrize('T,nsub', SHAPES)
@pytest.mark.parametrize('regime', pr.CORE)
@pytest.mark.parametrize('mode', ['rapid', 'muskingum', 'unit'])
def test_direct_rows(monkeypatch, mode, regime, T, nsub):
    """k_direct on the post-order numbering of the same network, and the record path on it (RR_DIRECT=0): each per reach against the
    arbiter, and the two bit for bit, as test_direct.py has them."""
    inp, refs = _dev_case(mode, 'postorder', regime, T, nsub)
    got = {}
    for direct in ('1', '0'):
        set_env(monkeypatch, {'RR_DIRECT': direct, 'RR_WAVE': '1'})
        with Plan(inp.indptr, inp.indices) as plan:
            assert plan.direct_info()['ok'], plan.direct_info()['why']
            kernel = 'direct' if direct == '1' else 'tile'
            ratios, rows, states = _dev_route(mode, plan, inp, refs, T, nsub, kernel, f'{kernel} on post-order, {mode}, {regime}')
            got[direct] = rows + states
        report('k_direct' if direct == '1' else 'records on post-order', mode, 'postorder', regime, T, nsub, ratios)
    for a, b in zip(got['1'], got['0']):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize('regime', pr.CORE)
@pytest.mark.parametrize('net,kernel', [('random', 'tile'), ('postorder', 'direct')])
@pytest.mark.parametrize('f32_in,f32_out,T,nsub', [(True, False, 48, 1), (True, False, 24, 3), (False, True, 48, 1), (False, True, 24, 2),
                                                   (True, True, 48, 1), (True, True, 24, 2)])
def test_float32_rows(monkeypatch, f32_in, f32_out, T, nsub, net, kernel, regime):
    """float32 lateral rows in: the arbiter runs on the widened values, the bound is the float64 one.  float32 rows out: one rounding to
    float32 on top of it, per element (two sub-steps there, not three: sub-steps x factor must divide a record batch's 128 rows)."""
    set_env(monkeypatch, {'RR_WAVE': '1'})
    inp, refs = pr.rapid_case(net, regime, T, nsub, f32_lat=f32_in)
    what = f'float32 {"in" if f32_in else ""}{"+" if f32_in and f32_out else ""}{"out" if f32_out else ""}'
    with Plan(inp.indptr, inp.indices) as plan:
        plan.set_coeffs(inp.lhs, inp.c2, inp.c3, inp.c4_dt)
        ratios, _, _ = _dev_rapid(plan, inp, refs, T, nsub, kernel, f'{what}, {kernel}, {regime}', f32_in=f32_in, f32_out=f32_out)
    report(f'{what} ({kernel})', 'rapid', net, regime, T, nsub, ratios)


# ------------------------------------------------------------------------------------------------ the unit-hydrograph convolution

@pytest.mark.parametrize('regime', pr.REGIMES)
@pytest.mark.parametrize('n_ks', [5, 48])
def test_uh_convolve_per_column(n_ks, regime):
    """rr_uh_convolve, two consecutive files of 48 rows with the carried state: rows and state, every column at its own scale."""
    inp, refs = pr.unit_case('random', regime, 48, 1, n_ks=n_ks)
    st = np.zeros_like(inp.kern)
    ratios = {}
    for call, r in enumerate(refs):
        conv = uh_convolve(inp.kern, st, r.rows)
        ratios[f'rows{call}'] = pr.assert_per_reach(conv, r.conv_orc, r.conv_exact, r.conv_exact, f'uh_convolve n_ks {n_ks}, {regime}, call {call}: rows')
        ratios[f'state{call}'] = pr.assert_per_reach(st, r.uh_orc, r.uh_exact, np.vstack([r.conv_exact, r.uh_exact]), f'uh_convolve n_ks {n_ks}, {regime}, call {call}: state')
    report(f'uh_convolve n_ks {n_ks}', 'uh', 'random', regime, 48, 1, ratios)


@pytest.mark.parametrize('T,nsub', SHAPES)
@pytest.mark.parametrize('regime', pr.CORE)
@pytest.mark.parametrize('n_ks', [5, 48])
def test_unit_route_fused_convolution(monkeypatch, n_ks, regime, T, nsub):
    """rr_unit_route_uh_dev: the convolution fused into the in-pass (k_rec_in_uh), k_tile behind it.  Headwater columns are, bit for
    bit, the rows rr_uh_convolve makes of the same depths and state; inner columns, q_ch, the router's state and the convolution's
    carried state per reach against the arbiter, which routes its own convolved rows as the fused call does."""
    set_env(monkeypatch, {'RR_WAVE': '1'})
    inp, refs = pr.unit_case('random', regime, T, nsub, n_ks=n_ks)
    n, ni = inp.n, inp.ni
    ratios = {}
    st_alone = np.zeros_like(inp.kern)
    with Plan(inp.indptr, inp.indices) as plan:
        plan.set_coeffs(np.ascontiguousarray(-inp.c1[inp.indices]), inp.c2, inp.c3, None)
        d_kern, d_state = DeviceBuffer(inp.kern.nbytes).upload(inp.kern), DeviceBuffer(inp.kern.nbytes).upload(np.zeros_like(inp.kern))
        d_depth, d_out, d_fin = DeviceBuffer(T * n * 8), DeviceBuffer(T * n * 8), DeviceBuffer(n * 8)
        d_qc, d_qf = DeviceBuffer(ni * 8).upload(np.zeros(ni)), DeviceBuffer(ni * 8).upload(np.zeros(ni))
        for call, r in enumerate(refs):
            what = f'fused convolution n_ks {n_ks}, {regime}, call {call}'
            conv_alone = uh_convolve(inp.kern, st_alone, r.rows)
            d_depth.upload(r.rows)
            d_out.upload(np.full((T, n), -1.0))
            plan.unit_route_uh_dev(d_qc, d_qf, d_fin, d_kern, d_state, n_ks, d_depth, T, nsub, discharge=d_out)
            assert plan.last_kernel() == 'tile'
            d, qc, qf = d_out.download(np.float64, (T, n)), d_qc.download(np.float64, (ni,)), d_qf.download(np.float64, (ni,))
            fin, st = d_fin.download(np.float64, (n,)), d_state.download(np.float64, inp.kern.shape)
            check_unit(d, qc, qf, inp, r, conv_alone, what, ratios, call)
            np.testing.assert_array_equal(fin[inp.inner_idx], qf, err_msg=f'{what}: router state, inner reaches')
            np.testing.assert_array_equal(fin[inp.hw_idx], conv_alone[-1, inp.hw_idx], err_msg=f'{what}: router state, headwaters')
            ratios[f'uh{call}'] = pr.assert_per_reach(st, r.uh_orc, r.uh_exact, np.vstack([r.conv_exact, r.uh_exact]), f'{what}: convolution state')
            d_qc.upload(qf)
        for b in (d_kern, d_state, d_depth, d_out, d_fin, d_qc, d_qf):
            b.free()
    report(f'fused convolution n_ks {n_ks}', 'unit', 'random', regime, T, nsub, ratios)
