"""Ensembles on the time-tiled kernel (rr_rapid_route_ensemble_dev, Plan.rapid_route_ensemble*): member m of a batched call equals a
single-member call with member m's rows on the same plan, bit for bit -- discharge rows, float32 means and final states -- and the
call refuses what it does not take."""
import numpy as np
import pytest

from oracle import oracle
from river_route_amd import synth
from river_route_amd._lib import RR_E_INVALID, RR_E_STATE, RR_E_UNSUPPORTED, RRError
from river_route_amd.engine import DeviceBuffer, Plan

pytestmark = pytest.mark.gpu
KNOBS = ('RR_WAVE', 'RR_WAVE_K', 'RR_TILE_BLOCK', 'RR_TILE_LEAN', 'RR_UH_PAIRS', 'RR_DIRECT')


@pytest.fixture(autouse=True)
def _records_for_every_call(monkeypatch):
    """Single-member calls on records too (a post-order network would take the direct row path), so both sides run k_tile."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv('RR_DIRECT', '0')


def csc_from_down(down_index):
    has = down_index >= 0
    indptr = np.concatenate([[0], np.cumsum(has)]).astype(np.int32)
    return indptr, down_index[has].astype(np.int32)


def make_plan(down, k, x, dt, nsub):
    indptr, indices = csc_from_down(down)
    c1, c2, c3 = oracle.muskingum_coefficients(k, x, dt / nsub)
    plan = Plan(indptr, indices)
    c4 = (c1 + c2) / dt
    plan.set_coeffs(-c1[indices], c2, c3, c4)
    return plan, (indptr, indices, -c1[indices], c2, c3, c4)


def synth_case(n, M, T, seed=3, order='random'):
    net = synth.synth_network(n, seed=seed, order=order)
    ql = np.stack([synth.synth_qlateral(n, 0, T, seed=100 + m, dt=3600.0) * 3600.0 for m in range(M)])
    q0 = np.stack([2.0 * synth.u01(50 + m, np.arange(n)) for m in range(M)])
    return net.down_index, net.k, net.x, ql, q0


def single_loop(plan, ql, q0, nsub, factor=None):
    """Member by member through rr_rapid_route_dev / _f32_dev / _f32in_dev: (states, discharge)."""
    M, T, n = ql.shape
    f32_in = ql.dtype == np.float32
    rows = T if factor is None else T // factor
    d_ql, d_q = DeviceBuffer(T * n * ql.itemsize), DeviceBuffer(n * 8)
    d_out = DeviceBuffer(rows * n * (8 if factor is None else 4))
    states, out = np.empty((M, n)), np.empty((M, rows, n), np.float64 if factor is None else np.float32)
    for m in range(M):
        d_ql.upload(ql[m]); d_q.upload(q0[m])
        if f32_in and factor is None:
            plan.rapid_route_f32in_dev(d_q, d_ql, T, T, nsub, discharge=d_out, out_rows=T)
        elif f32_in:
            plan.rapid_route_f32in_dev(d_q, d_ql, T, T, nsub, discharge32=d_out, factor=factor)
        elif factor is None:
            plan.rapid_route_dev(d_q, d_ql, T, d_out, T, T, nsub)
        else:
            plan.rapid_route_f32_dev(d_q, d_ql, T, d_out, T, nsub, factor)
        assert plan.last_kernel() == 'tile'
        out[m] = d_out.download(out.dtype, (rows, n))
        states[m] = d_q.download(np.float64, (n,))
    for b in (d_ql, d_q, d_out):
        b.free()
    return states, out


def batched(plan, ql, q0, nsub, factor=None):
    M, T, n = ql.shape
    out = np.empty((M, T, n)) if factor is None else np.empty((M, T // factor, n), np.float32)
    states = plan.rapid_route_ensemble(q0, ql, out, nsub, factor=1 if factor is None else factor)
    assert plan.last_kernel() == 'tile_ensemble'
    return states, out


def assert_members_equal(plan, ql, q0, nsub, factor=None):
    s1, d1 = single_loop(plan, ql, q0, nsub, factor)
    s2, d2 = batched(plan, ql, q0, nsub, factor)
    assert np.array_equal(d1.view(np.int64 if d1.dtype == np.float64 else np.int32), d2.view(np.int64 if d2.dtype == np.float64 else np.int32))      # bit patterns: a zero's sign too
    assert np.array_equal(s1.view(np.int64), s2.view(np.int64))


# factor None: float64 rows out; else float32 means of `factor` rows, which need factor x nsub to divide 128 (as the single-member calls do)
@pytest.mark.parametrize('n,M,T,nsub,f32_in,factor', [
    (100_000, 2, 32, 1, False, None), (100_000, 7, 120, 12, True, None), (100_000, 51, 120, 12, True, None), (100_000, 1, 744, 1, False, None),
    (100_000, 7, 744, 4, False, 1), (100_000, 7, 120, 1, True, 8), (100_000, 2, 744, 4, True, 8), (100_000, 7, 120, 1, False, 2),
    (30_000, 51, 32, 4, False, None)])
def test_batched_equals_single_member_calls(n, M, T, nsub, f32_in, factor):
    down, k, x, ql, q0 = synth_case(n, M, T)
    if f32_in:
        ql = ql.astype(np.float32)
    plan, _ = make_plan(down, k, x, 3600.0, nsub)
    with plan:
        assert_members_equal(plan, ql, q0, nsub, factor)


def test_batched_equals_single_member_calls_on_a_1m_slice():
    down, k, x, ql, q0 = synth_case(1_000_000, 2, 120, seed=8)
    plan, _ = make_plan(down, k, x, 3600.0, 12)
    with plan:
        assert_members_equal(plan, ql.astype(np.float32), q0, 12)


@pytest.mark.parametrize('case', ['docs9', 'forest30', 'tree1k'])
def test_golden_network_members(golden_kernels, case):
    g = golden_kernels
    indptr, indices = g[f'{case}/indptr'].astype(np.int32), g[f'{case}/indices'].astype(np.int32)
    nsub, dt = 2, 3600.0
    c1, c2, c3 = oracle.muskingum_coefficients(g[f'{case}/k'], g[f'{case}/x'], dt / nsub)
    ql = np.stack([np.tile(g[f'{case}/qlateral'], (4, 1)) * (1 + m) for m in range(3)])      # 48 rows
    q0 = np.stack([g[f'{case}/q0'] * (m + 1) for m in range(3)])
    with Plan(indptr, indices) as plan:
        plan.set_coeffs(-c1[indices], c2, c3, (c1 + c2) / dt)
        assert_members_equal(plan, ql, q0, nsub)


def test_two_members_against_the_oracle():
    down, k, x, ql, q0 = synth_case(20_000, 2, 64)
    nsub = 3
    plan, args = make_plan(down, k, x, 3600.0, nsub)
    with plan:
        states, out = batched(plan, ql, q0, nsub)
    for m in range(2):
        q, d = q0[m].copy(), np.zeros((64, 20_000))
        oracle.rapid_route(*args, q, ql[m], d, nsub)
        np.testing.assert_allclose(out[m], d, rtol=1e-10, atol=1e-10 * np.abs(d).max())
        np.testing.assert_allclose(states[m], q, rtol=1e-10, atol=1e-10 * np.abs(d).max())


def test_groups_equal_one_group_and_shared_initial_state():
    down, k, x, ql, q0 = synth_case(30_000, 51, 40)
    plan, _ = make_plan(down, k, x, 3600.0, 4)
    with plan:
        out1 = np.empty((51, 40, 30_000))
        s1 = plan.rapid_route_ensemble(q0[0], ql, out1, 4)           # one group, every member from the same state
        out2, s2 = np.empty_like(out1), np.empty((51, 30_000))
        for g0 in range(0, 51, 16):
            s2[g0:g0 + 16] = plan.rapid_route_ensemble(q0[0], ql[g0:g0 + 16], out2[g0:g0 + 16], 4)
        assert np.array_equal(out1, out2) and np.array_equal(s1, s2)
        assert not np.array_equal(s1[0], s1[1])


def test_wide_pitches_and_a_caller_stream():
    torch = pytest.importorskip('torch')
    n, M, T, nsub = 40_000, 3, 64, 2
    down, k, x, ql, q0 = synth_case(n, M, T)
    plan, _ = make_plan(down, k, x, 3600.0, nsub)
    with plan:
        s_ref, d_ref = single_loop(plan, ql, q0, nsub)
        dev = torch.device('cuda:0')
        lp, op, qp = T * n + 777, T * n + 129, n + 5
        lat = torch.zeros(M * lp, dtype=torch.float64, device=dev)
        out = torch.full((M * op,), -1.0, dtype=torch.float64, device=dev)
        q = torch.zeros(M * qp, dtype=torch.float64, device=dev)
        for m in range(M):
            lat[m * lp:m * lp + T * n] = torch.from_numpy(ql[m].ravel()).to(dev)
            q[m * qp:m * qp + n] = torch.from_numpy(q0[m]).to(dev)
        plan.reserve_ensemble(M, T, nsub)
        stream = torch.cuda.Stream(device=dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            plan.rapid_route_ensemble_dev(M, q, qp, lat, False, lp, out, False, op, 1, T, nsub, stream=stream.cuda_stream)
        stream.synchronize()
        for m in range(M):
            assert np.array_equal(out[m * op:m * op + T * n].cpu().numpy().reshape(T, n), d_ref[m])
            assert np.array_equal(q[m * qp:m * qp + n].cpu().numpy(), s_ref[m])
            assert float(out[m * op + T * n:(m + 1) * op].max()) == -1.0      # the gap between two members is not written


def _refusal(plan, code, **kw):
    from river_route_amd import _lib
    a = dict(members=2, q=DeviceBuffer(2 * plan.n * 8), q_pitch=plan.n, lat=DeviceBuffer(2 * 64 * plan.n * 8), lat_pitch=64 * plan.n,
             out=DeviceBuffer(2 * 64 * plan.n * 8), out_pitch=64 * plan.n, T=64, nsub=1)
    a.update(kw)
    with pytest.raises(RRError) as e:
        _lib.check(_lib.lib().rr_rapid_route_ensemble_dev(plan._h, a['members'], _lib.ptr(a['q']), a['q_pitch'], _lib.ptr(a['lat']), 0, a['lat_pitch'],
                                                          _lib.ptr(a['out']), 0, a['out_pitch'], 1, a['T'], a['nsub'], None))
    assert e.value.code == code, e.value.message
    return e.value.message


def test_refusals():
    down, k, x, _, _ = synth_case(5_000, 1, 1)
    plan, args = make_plan(down, k, x, 3600.0, 1)
    with plan:
        n = plan.n
        _refusal(plan, RR_E_INVALID, members=0)
        _refusal(plan, RR_E_INVALID, q=None)
        _refusal(plan, RR_E_INVALID, q_pitch=n - 1)
        _refusal(plan, RR_E_INVALID, lat_pitch=64 * n - 1)
        _refusal(plan, RR_E_INVALID, out_pitch=64 * n - 1)
        _refusal(plan, RR_E_UNSUPPORTED, T=31)
        assert 'rr_plan_reserve_ensemble(plan, 2, 64, 1' in _refusal(plan, RR_E_STATE)      # nothing reserved yet
        plan.reserve_ensemble(1, 64, 1)
        _refusal(plan, RR_E_STATE)
        with pytest.raises(RRError) as e:
            plan.reserve_ensemble(70_000, 64, 1)
        assert e.value.code == RR_E_INVALID
        indptr, indices, lhs, c2, c3, c4 = args
        lhs2 = lhs.copy()
        rows, counts = np.unique(indices, return_counts=True)
        lhs2[np.flatnonzero(indices == rows[counts >= 2][0])[0]] *= 0.5      # two tributaries of one reach with different weights
        plan.set_coeffs(lhs2, c2, c3, c4)
        assert 'per-edge' in _refusal(plan, RR_E_UNSUPPORTED)
    down, k, x, _, _ = synth_case(5_000, 1, 1, seed=4)
    plan, args = make_plan(down, k, x, 3600.0, 1)
    with plan:
        outlet = int(np.flatnonzero(down < 0)[0])
        plan.set_boundary([], [outlet])
        assert 'boundary' in _refusal(plan, RR_E_UNSUPPORTED)


def test_rapid_muskingum_ensemble_mode_batches_and_matches_the_loop(monkeypatch, tmp_path, golden_routers):
    """RapidMuskingum(runoff_processing_mode='ensemble') on the real engine: members with the same dates go through one group call and
    give what the loop gives, bit for bit (writer calls, member states, channel_state)."""
    import pandas as pd
    import river_route_amd as rr
    g = golden_routers
    params = tmp_path / 'params.parquet'
    pd.DataFrame({'river_id': g['river_ids'], 'downstream_river_id': g['downstream_ids'], 'k': g['k'], 'x': g['x']}).to_parquet(params)
    init = tmp_path / 'init.parquet'
    pd.DataFrame({'Q': g['q0']}).to_parquet(init)
    dates = g['dates0'].astype('datetime64[s]')
    series = [g['vol0'] * (1.0 + 0.25 * m) for m in range(5)]
    files = [str(tmp_path / f'ql{i}.nc') for i in range(5)]
    for f in files:
        open(f, 'w').close()

    def route(batch):
        calls = []

        class InMemory(rr.RapidMuskingum):
            def _qlateral_generator(self):
                yield from zip([dates] * 5, series, self.cfg.qlateral_files, self.cfg.discharge_files)

            def _route_ensemble_group(self, group):
                calls.append(len(group))
                return super()._route_ensemble_group(group)
        if not batch:
            monkeypatch.setattr(InMemory, '_ensemble_batching', lambda self: False)
        got = []
        r = InMemory(params_file=str(params), qlateral_files=files, discharge_dir=str(tmp_path), log=False, channel_state_init_file=str(init),
                     runoff_processing_mode='ensemble', dt_routing=900, dt_discharge=7200)
        r.set_write_discharges(lambda d, q, f, rf='': got.append((np.asarray(d), np.asarray(q), f, rf)))
        r.route()
        return r, got, calls

    r1, got1, calls1 = route(True)
    r2, got2, calls2 = route(False)
    assert calls1 == [5] and calls2 == []
    for (d1, q1, f1, rf1), (d2, q2, f2, rf2) in zip(got1, got2, strict=True):
        assert np.array_equal(d1, d2) and (f1, rf1) == (f2, rf2) and np.array_equal(q1.view(np.int32), q2.view(np.int32))
    for s1, s2 in zip(r1._ensemble_member_states, r2._ensemble_member_states, strict=True):
        assert np.array_equal(s1.view(np.int64), s2.view(np.int64))
    assert np.array_equal(r1.channel_state.view(np.int64), r2.channel_state.view(np.int64))
