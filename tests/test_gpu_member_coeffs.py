"""Parameter ensembles on the time-tiled kernel (rr_plan_set_member_coeffs, rr_rapid_route_members_dev, Plan.set_member_coeffs,
Plan.rapid_route_members*): member m of a members call, routed with coefficient set m, equals -- bit for bit: discharge rows, float32
means and final states -- the existing path with that set: Plan.set_coeffs(member m's arrays) and the one-member
Plan.rapid_route_ensemble on member m's rows and state (both sides run the general tick).  The plan's own coefficient set and what
other calls compute with it stay as they were, and the calls refuse what they do not take."""
import numpy as np
import pytest

from oracle import oracle
from river_route_amd import _lib, synth
from river_route_amd._lib import RR_E_INVALID, RR_E_STATE, RR_E_UNSUPPORTED, RRError
from river_route_amd.engine import DeviceBuffer, Plan

pytestmark = pytest.mark.gpu
KNOBS = ('RR_WAVE', 'RR_WAVE_K', 'RR_TILE_BLOCK', 'RR_TILE_LEAN', 'RR_UH_PAIRS', 'RR_DIRECT', 'RR_HW_INPASS', 'RR_REC_BATCHES')
DT = 3600.0


@pytest.fixture(autouse=True)
def _records_for_every_call(monkeypatch):
    """Single-member calls on records too (a post-order network would take the direct row path), so every call runs k_tile."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv('RR_DIRECT', '0')


def csc_from_down(down_index):
    has = down_index >= 0
    indptr = np.concatenate([[0], np.cumsum(has)]).astype(np.int32)
    return indptr, down_index[has].astype(np.int32)


def member_sets(k, x, indices, M, nsub, dt=DT):
    """Coefficient set m: the network's k stretched by 15 % and its x shifted by 0.02 per member.  (lhs (M, E), c2, c3, c4 (M, n))"""
    lhs, c2, c3, c4 = [], [], [], []
    for m in range(M):
        a1, a2, a3 = oracle.muskingum_coefficients(k * (1 + 0.15 * m), np.clip(x + 0.02 * m, 0.0, 0.45), dt / nsub)
        lhs.append(-a1[indices]); c2.append(a2); c3.append(a3); c4.append((a1 + a2) / dt)
    return [np.ascontiguousarray(np.stack(a)) for a in (lhs, c2, c3, c4)]


def bits(a):
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def rows_out(M, T, n, factor):
    return np.empty((M, T, n)) if factor is None else np.empty((M, T // factor, n), np.float32)


def comparator(plan, sets, m, ql_m, q0_m, nsub, factor=None):
    """The existing path for member m: its arrays as the plan's own coefficients, then the one-member ensemble call."""
    plan.set_coeffs(*(a[m] for a in sets))
    out = rows_out(1, ql_m.shape[0], plan.n, factor)
    state = plan.rapid_route_ensemble(q0_m, ql_m[None], out, nsub, factor=1 if factor is None else factor)
    assert plan.last_kernel() == 'tile_ensemble'
    return state[0], out[0]


def route_members(plan, sets, ql, q0, nsub, factor=None):
    plan.set_member_coeffs(*sets)
    M = sets[1].shape[0]
    out = rows_out(M, ql.shape[-2], plan.n, factor)
    states = plan.rapid_route_members(q0, ql, out, nsub, factor=1 if factor is None else factor)
    assert plan.last_kernel() == 'tile_ensemble'
    return states, out


def assert_members_equal_comparators(plan, sets, ql, q0, nsub, factor=None, members=None):
    """ql (T, n): one forcing for all, or (M, T, n).  The members call first: its tables must survive the comparators' set_coeffs calls."""
    states, out = route_members(plan, sets, ql, q0, nsub, factor)
    for m in (range(sets[1].shape[0]) if members is None else members):
        s_ref, d_ref = comparator(plan, sets, m, ql if ql.ndim == 2 else ql[m], q0[m], nsub, factor)
        assert np.array_equal(bits(out[m]), bits(d_ref)), f'discharge of member {m}'
        assert np.array_equal(bits(states[m]), bits(s_ref)), f'final state of member {m}'
    return states, out


def synth_case(n, M, T, seed=3, order='random'):
    net = synth.synth_network(n, seed=seed, order=order)
    ql = np.stack([synth.synth_qlateral(n, 0, T, seed=100 + m, dt=DT) * DT for m in range(M)])
    q0 = np.stack([2.0 * synth.u01(50 + m, np.arange(n)) for m in range(M)])
    return net.down_index, net.k, net.x, ql, q0


# ---- 1. golden networks: bit-equal to the comparator, and the oracle with member m's coefficients within the parity tolerance ----

@pytest.mark.parametrize('case', ['docs9', 'forest30', 'tree1k'])
def test_golden_network_members(golden_kernels, case):
    g = golden_kernels
    indptr, indices = g[f'{case}/indptr'].astype(np.int32), g[f'{case}/indices'].astype(np.int32)
    M, nsub = 3, 2
    sets = member_sets(g[f'{case}/k'], g[f'{case}/x'], indices, M, nsub)
    ql = np.ascontiguousarray(np.tile(g[f'{case}/qlateral'], (4, 1))[:48])      # 48 rows, shared
    assert ql.shape == (48, len(indptr) - 1)
    q0 = np.stack([g[f'{case}/q0'] * (m + 1) for m in range(M)])
    with Plan(indptr, indices) as plan:
        states, out = assert_members_equal_comparators(plan, sets, ql, q0, nsub)
    for m in range(M):
        q, d = q0[m].copy(), np.zeros_like(ql)
        oracle.rapid_route(indptr, indices, *(a[m] for a in sets), q, ql, d, nsub)
        np.testing.assert_allclose(out[m], d, rtol=1e-10, atol=1e-10 * np.abs(d).max())
        np.testing.assert_allclose(states[m], q, rtol=1e-10, atol=1e-10 * np.abs(d).max())


# ---- 2. synthetic random-order networks: several tiles and levels, a record-batch edge, float32 rows; shared forcing and one per member ----

@pytest.mark.parametrize('shared', [True, False], ids=['shared', 'per_member'])
@pytest.mark.parametrize('M,T,nsub,f32', [(2, 32, 1, False), (7, 40, 4, False), (3, 136, 1, True)])
@pytest.mark.parametrize('n', [5_000, 20_000])
def test_members_equal_their_comparators(n, M, T, nsub, f32, shared):
    down, k, x, ql, q0 = synth_case(n, M, T)
    if f32:
        ql = ql.astype(np.float32)
    indptr, indices = csc_from_down(down)
    sets = member_sets(k, x, indices, M, nsub)
    with Plan(indptr, indices) as plan:
        assert plan.tile_info()['tiles'] > 1 and plan.tile_info()['levels'] > 1
        assert_members_equal_comparators(plan, sets, ql[0] if shared else ql, q0, nsub, 8 if f32 else None)


def test_more_tiles_than_a_members_share_of_the_slots():
    n, M, T = 100_000, 16, 64
    down, k, x, ql, q0 = synth_case(n, 1, T)
    indptr, indices = csc_from_down(down)
    sets = member_sets(k, x, indices, M, 1)
    q0 = q0[0] * (1.0 + 0.25 * np.arange(M))[:, None]
    with Plan(indptr, indices) as plan:
        assert plan.tile_info()['tiles'] > 512 // M
        assert_members_equal_comparators(plan, sets, ql[0], q0, 1)


# ---- 3. M equal sets, all the plan's own: the bits of the forcing ensemble ----

@pytest.mark.parametrize('nsub', [1, 3])
def test_equal_sets_give_the_forcing_ensemble(nsub):
    n, M, T = 5_000, 4, 40
    down, k, x, ql, q0 = synth_case(n, M, T)
    indptr, indices = csc_from_down(down)
    one = member_sets(k, x, indices, 1, nsub)
    sets = [np.ascontiguousarray(np.repeat(a, M, axis=0)) for a in one]
    with Plan(indptr, indices) as plan:
        plan.set_coeffs(*(a[0] for a in one))
        d_ref = np.empty((M, T, n))
        s_ref = plan.rapid_route_ensemble(q0, ql, d_ref, nsub)
        states, out = route_members(plan, sets, ql, q0, nsub)
    assert np.array_equal(bits(out), bits(d_ref)) and np.array_equal(bits(states), bits(s_ref))


# ---- 4. isolation: a NaN in one member's set stays in that member, downstream of its reach ----

def test_a_nan_coefficient_stays_in_its_member_and_downstream_of_its_reach():
    n, M, T, nsub = 5_000, 3, 40, 1
    down, k, x, ql, q0 = synth_case(n, M, T)
    indptr, indices = csc_from_down(down)
    sets = member_sets(k, x, indices, M, nsub)
    # a mid-network reach: reaches upstream of it, and a few downstream
    n_up = np.zeros(n, np.int64)
    for i in range(n):      # params order is upstream-first
        if down[i] >= 0:
            n_up[down[i]] += n_up[i] + 1
    reach = int(np.flatnonzero((n_up >= 20) & (n_up <= 200))[0])
    path = [reach]
    while down[path[-1]] >= 0:
        path.append(int(down[path[-1]]))
    assert len(path) >= 3
    on_path = np.zeros(n, bool)
    on_path[path] = True
    clean = [a.copy() for a in sets]
    sets[2][1, reach] = np.nan
    with Plan(indptr, indices) as plan:
        states, out = assert_members_equal_comparators(plan, sets, ql[0], q0, nsub, members=(0, 2))
        s_nan, d_nan = comparator(plan, sets, 1, ql[0], q0[1], nsub)           # the same NaN through the existing path
        s_clean, d_clean = comparator(plan, clean, 1, ql[0], q0[1], nsub)      # member 1 without it
    assert np.array_equal(bits(out[1]), bits(d_nan)) and np.array_equal(bits(states[1]), bits(s_nan))
    assert np.array_equal(np.isnan(states[1]), on_path)      # the carried discharge: NaN at the reach and downstream of it, nowhere else
    assert not np.isnan(out[1][:, ~on_path]).any()
    assert np.array_equal(bits(out[1][:, ~on_path]), bits(d_clean[:, ~on_path])) and np.array_equal(bits(states[1][~on_path]), bits(s_clean[~on_path]))
    # (a discharge row clamps at zero with !(x > 0): a NaN leaves as 0.0 where the clean run is positive)
    assert not np.array_equal(out[1][:, on_path], d_clean[:, on_path])


# ---- 5. the plan's own coefficient set and what other calls compute with it are untouched ----

def _own_results(plan, ql, q0, nsub, want_kernel):
    T, n = ql.shape[1:]
    d_ql, d_q, d_out = DeviceBuffer(T * n * 8), DeviceBuffer(n * 8), DeviceBuffer(T * n * 8)
    d_ql.upload(ql[0]); d_q.upload(q0[0])
    plan.rapid_route_dev(d_q, d_ql, T, d_out, T, T, nsub)
    assert plan.last_kernel() == want_kernel
    single = (d_out.download(np.float64, (T, n)), d_q.download(np.float64, (n,)))
    for b in (d_ql, d_q, d_out):
        b.free()
    out = np.empty(ql.shape)
    states = plan.rapid_route_ensemble(q0, ql, out, nsub)
    return single + (out, states)


@pytest.mark.parametrize('order,direct', [('random', False), ('postorder', True)])
def test_plan_state_is_untouched(monkeypatch, order, direct):
    if direct:
        monkeypatch.delenv('RR_DIRECT')      # the post-order network's single-member call takes the direct row path
    n, M, T, nsub = 5_000, 3, 40, 1
    down, k, x, ql, q0 = synth_case(n, M, T, order=order)
    indptr, indices = csc_from_down(down)
    own = member_sets(k, x, indices, 1, nsub)
    sets = member_sets(k * 1.3, x, indices, M, nsub)
    with Plan(indptr, indices) as plan:
        plan.set_coeffs(*(a[0] for a in own))
        inpass = plan.inpass_info()
        before = _own_results(plan, ql[:2], q0[:2], nsub, 'direct' if direct else 'tile')
        s_members, d_members = route_members(plan, sets, ql[0], q0, nsub)
        assert plan.inpass_info() == inpass
        after = _own_results(plan, ql[:2], q0[:2], nsub, 'direct' if direct else 'tile')
        for a, b in zip(before, after):
            assert np.array_equal(bits(a), bits(b))
        s_again, d_again = route_members(plan, sets, ql[0], q0, nsub)
        assert np.array_equal(bits(d_members), bits(d_again)) and np.array_equal(bits(s_members), bits(s_again))
    assert not np.array_equal(d_members[0], before[2][0])      # (the members' sets are not the plan's)


def test_a_plan_that_never_saw_set_coeffs_routes_members():
    n, M, T, nsub = 5_000, 3, 40, 2
    down, k, x, ql, q0 = synth_case(n, M, T)
    indptr, indices = csc_from_down(down)
    sets = member_sets(k, x, indices, M, nsub)
    with Plan(indptr, indices) as fresh:
        with pytest.raises(RRError) as e:
            fresh.reserve_ensemble(M, T, nsub)      # neither setter yet
        assert e.value.code == RR_E_STATE
        states, out = route_members(fresh, sets, ql, q0, nsub)
    with Plan(indptr, indices) as plan:
        for m in range(M):
            s_ref, d_ref = comparator(plan, sets, m, ql[m], q0[m], nsub)
            assert np.array_equal(bits(out[m]), bits(d_ref)) and np.array_equal(bits(states[m]), bits(s_ref))


# ---- 6. groups: five sets routed two at a time equal one group of five ----

@pytest.mark.parametrize('shared', [True, False])
def test_groups_equal_one_group(monkeypatch, shared):
    n, M, T, nsub = 5_000, 5, 40, 2
    down, k, x, ql, q0 = synth_case(n, M, T)
    indptr, indices = csc_from_down(down)
    sets = member_sets(k, x, indices, M, nsub)
    forcing = ql[0] if shared else ql
    with Plan(indptr, indices) as plan:
        s1, d1 = route_members(plan, sets, forcing, q0, nsub)
        real, routed = Plan.reserve_ensemble, []

        def two_at_most(self, members, *a, **kw):
            return dict(real(self, members, *a, **kw), members_max=2)
        monkeypatch.setattr(Plan, 'reserve_ensemble', two_at_most)
        real_dev = Plan.rapid_route_members_dev
        monkeypatch.setattr(Plan, 'rapid_route_members_dev', lambda self, members, *a, **kw: (routed.append(members), real_dev(self, members, *a, **kw))[1])
        out = np.empty((M, T, n))
        s2 = plan.rapid_route_members(q0, forcing, out, nsub)
        assert routed == [2, 2, 1]
        assert np.array_equal(bits(d1), bits(out)) and np.array_equal(bits(s1), bits(s2))
        s3 = plan.rapid_route_members(q0, forcing, out, nsub)      # and again: the first group's sets are set anew
        assert np.array_equal(bits(d1), bits(out)) and np.array_equal(bits(s1), bits(s3))


# ---- 7. wide pitches -- the coefficient arrays' too -- and a caller's torch stream ----

def test_wide_pitches_and_a_caller_stream():
    torch = pytest.importorskip('torch')
    n, M, T, nsub = 20_000, 3, 64, 2
    down, k, x, ql, q0 = synth_case(n, M, T)
    indptr, indices = csc_from_down(down)
    sets = member_sets(k, x, indices, M, nsub)
    E = indices.shape[0]
    with Plan(indptr, indices) as plan:
        refs = [comparator(plan, sets, m, ql[m], q0[m], nsub) for m in range(M)]
        wide = [np.full((M, E + 3), np.nan)] + [np.full((M, n + 4), np.nan) for _ in range(3)]      # pitches E + 3 and n + 4, NaN in the gaps
        for w, a in zip(wide, sets):
            w[:, :a.shape[1]] = a
        lib = _lib.lib()
        _lib.check(lib.rr_plan_set_member_coeffs(plan._h, M, _lib.ptr(wide[0]), E + 3, _lib.ptr(wide[1]), _lib.ptr(wide[2]), _lib.ptr(wide[3]), n + 4))
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
            plan.rapid_route_members_dev(M, q, qp, lat, False, lp, out, False, op, 1, T, nsub, stream=stream.cuda_stream)
        stream.synchronize()
        assert plan.last_kernel() == 'tile_ensemble'
        for m in range(M):
            assert np.array_equal(bits(out[m * op:m * op + T * n].cpu().numpy().reshape(T, n)), bits(refs[m][1]))
            assert np.array_equal(bits(q[m * qp:m * qp + n].cpu().numpy()), bits(refs[m][0]))
            assert float(out[m * op + T * n:(m + 1) * op].max()) == -1.0 == float(out[m * op + T * n:(m + 1) * op].min())      # the gap between two members is not written
            assert float(q[m * qp + n:(m + 1) * qp].abs().max()) == 0.0


# ---- 8. refusals, each with its code ----

def _set_refusal(plan, code, sets, **kw):
    a = dict(members=sets[1].shape[0], lhs=sets[0], lhs_pitch=sets[0].shape[1], c2=sets[1], c3=sets[2], c4=sets[3], pitch=plan.n)
    a.update(kw)
    with pytest.raises(RRError) as e:
        _lib.check(_lib.lib().rr_plan_set_member_coeffs(plan._h, a['members'], _lib.ptr(a['lhs']), a['lhs_pitch'], _lib.ptr(a['c2']), _lib.ptr(a['c3']),
                                                        _lib.ptr(a['c4']), a['pitch']))
    assert e.value.code == code, e.value.message
    return e.value.message


def _route_refusal(plan, code, **kw):
    n = plan.n
    a = dict(members=2, q=DeviceBuffer(2 * n * 8), q_pitch=n, lat=DeviceBuffer(2 * 64 * n * 8), lat_pitch=64 * n,
             out=DeviceBuffer(2 * 64 * n * 8), out_pitch=64 * n, T=64, nsub=1)
    a.update(kw)
    with pytest.raises(RRError) as e:
        _lib.check(_lib.lib().rr_rapid_route_members_dev(plan._h, a['members'], _lib.ptr(a['q']), a['q_pitch'], _lib.ptr(a['lat']), 0, a['lat_pitch'],
                                                         _lib.ptr(a['out']), 0, a['out_pitch'], 1, a['T'], a['nsub'], None))
    assert e.value.code == code, e.value.message
    return e.value.message


def test_refusals():
    down, k, x, _, _ = synth_case(5_000, 1, 1)
    indptr, indices = csc_from_down(down)
    sets = member_sets(k, x, indices, 3, 1)
    with Plan(indptr, indices) as plan:
        n = plan.n
        assert 'rr_plan_set_member_coeffs(plan, 2' in _route_refusal(plan, RR_E_STATE)      # routing before the setter
        _set_refusal(plan, RR_E_INVALID, sets, members=0)
        _set_refusal(plan, RR_E_INVALID, sets, members=70_000)
        for name in ('lhs', 'c2', 'c3', 'c4'):
            _set_refusal(plan, RR_E_INVALID, sets, **{name: None})
        _set_refusal(plan, RR_E_INVALID, sets, pitch=n - 1)
        _set_refusal(plan, RR_E_INVALID, sets, lhs_pitch=indices.shape[0] - 1)
        assert 'rr_plan_set_member_coeffs' in _route_refusal(plan, RR_E_STATE)      # none of the refused calls left a set behind
        plan.set_member_coeffs(*sets)
        _route_refusal(plan, RR_E_INVALID, members=0)
        _route_refusal(plan, RR_E_INVALID, members=70_000)
        _route_refusal(plan, RR_E_INVALID, q=None)
        _route_refusal(plan, RR_E_INVALID, lat=None)
        _route_refusal(plan, RR_E_INVALID, out=None)
        _route_refusal(plan, RR_E_INVALID, q_pitch=n - 1)
        _route_refusal(plan, RR_E_INVALID, lat_pitch=64 * n - 1)
        _route_refusal(plan, RR_E_INVALID, out_pitch=64 * n - 1)
        assert 'rr_plan_set_member_coeffs(plan, 4' in _route_refusal(plan, RR_E_STATE, members=4, q=DeviceBuffer(4 * n * 8), lat_pitch=0, out=DeviceBuffer(4 * 64 * n * 8))
        _route_refusal(plan, RR_E_UNSUPPORTED, T=31)
        assert 'rr_plan_reserve_ensemble(plan, 2, 64, 1' in _route_refusal(plan, RR_E_STATE, lat_pitch=0)      # nothing reserved yet
        # member 1 of 3: two tributaries of one reach with different weights
        bad = [a.copy() for a in sets]
        rows, counts = np.unique(indices, return_counts=True)
        bad[0][1, np.flatnonzero(indices == rows[counts >= 2][0])[0]] *= 0.5
        assert 'member 1' in _set_refusal(plan, RR_E_UNSUPPORTED, bad)
    down, k, x, _, _ = synth_case(5_000, 1, 1, seed=4)
    indptr, indices = csc_from_down(down)
    sets = member_sets(k, x, indices, 2, 1)
    with Plan(indptr, indices) as plan:
        plan.set_coeffs(*(a[0] for a in sets))
        plan.set_boundary([], [int(np.flatnonzero(down < 0)[0])])
        plan.set_member_coeffs(*sets)
        assert 'boundary' in _route_refusal(plan, RR_E_UNSUPPORTED)
