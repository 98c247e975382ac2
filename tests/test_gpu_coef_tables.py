"""A second coefficient set replaces every table the first one left (one derivation feeds the lag-order arrays, the
tile-order tables and their masked forms, the skeleton's table, the per-reach tables and the members' tables).  Per routing path: plan A
gets set 1 and routes, gets set 2 (another k, x) and routes again from the same initial state; a fresh plan B gets set 2 only.  A's second
discharge and final state equal B's byte for byte -- a table that a re-set leaves stale shows here -- and A's first result is checked
against the oracle at the tolerance of test_gpu_kernels.py.  60 reaches in post-order, tiles of 32, 40 rows of float64."""
import numpy as np
import pytest

from conftest import assert_close, unit_split
from oracle import oracle
from river_route_amd import synth
from river_route_amd.engine import DeviceBuffer, Plan

pytestmark = pytest.mark.gpu
KNOBS = ('RR_WAVE', 'RR_WAVE_K', 'RR_TILE_BLOCK', 'RR_TILE_LEAN', 'RR_UH_PAIRS', 'RR_DIRECT', 'RR_HW_INPASS', 'RR_REC_BATCHES')
N, T, DT = 60, 40, 900.0
RECORDS = {'RR_DIRECT': '0', 'RR_WAVE': '1', 'RR_TILE_BLOCK': '32'}
PATHS = {      # name: (environment at plan creation, call, last_kernel())
    'streaming': ({'RR_WAVE': '0'}, 'rapid', 'tick'),
    'records_inpass_headwaters': (RECORDS, 'rapid', 'tile'),
    'records_no_inpass_headwaters': (dict(RECORDS, RR_HW_INPASS='0'), 'rapid', 'tile'),
    'direct_rows': ({'RR_TILE_BLOCK': '32'}, 'rapid', 'direct'),
    'unit_on_records': (RECORDS, 'unit', 'tile'),
    'member_sets': (RECORDS, 'members', 'tile_ensemble'),
}


def bits(a):
    return a.view(np.int64)


def network():
    net = synth.synth_network(N, seed=1, order='postorder')
    has = net.down_index >= 0
    return net, np.concatenate([[0], np.cumsum(has)]).astype(np.int32), net.down_index[has].astype(np.int32)


def muskingum(net, s):
    """(c1, c2, c3) of set s: the network's k stretched by 30 % and its x shifted by 0.03 per step."""
    return oracle.muskingum_coefficients(net.k * (1 + 0.3 * s), np.clip(net.x + 0.03 * s, 0.0, 0.45), DT)


def coeff_set(net, indices, s):
    """(lhs_off_data, c2, c3, c4_dt) of set s."""
    c1, c2, c3 = muskingum(net, s)
    return -c1[indices], c2, c3, (c1 + c2) / DT


def rapid(plan, cs, ql, q0, kernel):
    plan.set_coeffs(*cs)
    d_ql, d_q, d_out = DeviceBuffer(ql.nbytes).upload(ql), DeviceBuffer(N * 8).upload(q0), DeviceBuffer(T * N * 8)
    plan.rapid_route_dev(d_q, d_ql, T, d_out, T, T, 1)
    assert plan.last_kernel() == kernel
    got = d_out.download(np.float64, (T, N)), d_q.download(np.float64, (N,))
    for b in (d_ql, d_q, d_out):
        b.free()
    return got


def unit(plan, cs, conv, q0_inner, kernel):
    plan.set_coeffs(*cs[:3], None)
    ni = q0_inner.size
    d_conv, d_qc, d_qf, d_out = DeviceBuffer(conv.nbytes).upload(conv), DeviceBuffer(ni * 8).upload(q0_inner), DeviceBuffer(ni * 8).upload(q0_inner), DeviceBuffer(T * N * 8)
    plan.unit_route_dev(d_qc, d_qf, d_conv, T, d_out, T, T, 1)
    assert plan.last_kernel() == kernel
    got = d_out.download(np.float64, (T, N)), d_qc.download(np.float64, (ni,)), d_qf.download(np.float64, (ni,))
    for b in (d_conv, d_qc, d_qf, d_out):
        b.free()
    return got


@pytest.mark.parametrize('path', list(PATHS))
def test_a_second_set_leaves_no_table_of_the_first(monkeypatch, path):
    env, call, kernel = PATHS[path]
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    net, indptr, indices = network()
    ql = synth.synth_qlateral(N, 0, T, dt=DT)
    q0 = 2.0 * synth.u01(3, np.arange(N))
    if call == 'rapid':
        one, two = coeff_set(net, indices, 0), coeff_set(net, indices, 1)
        with Plan(indptr, indices) as a, Plan(indptr, indices) as b:
            first = rapid(a, one, ql, q0, kernel)
            second = rapid(a, two, ql, q0, kernel)
            fresh = rapid(b, two, ql, q0, kernel)
        q_ref, d_ref = q0.copy(), np.zeros((T, N))
        oracle.rapid_route(indptr, indices, *one, q_ref, ql, d_ref, 1)
        want = (d_ref, q_ref)
    elif call == 'unit':
        one, two = coeff_set(net, indices, 0), coeff_set(net, indices, 1)
        hw_idx, inner_idx, A_in, A_hw = unit_split(indptr, indices, N)
        conv = ql / DT
        with Plan(indptr, indices) as a, Plan(indptr, indices) as b:
            first = unit(a, one, conv, q0[inner_idx].copy(), kernel)
            second = unit(a, two, conv, q0[inner_idx].copy(), kernel)
            fresh = unit(b, two, conv, q0[inner_idx].copy(), kernel)
        c1i, c2i, c3i = (c[inner_idx] for c in muskingum(net, 0))
        qc_ref, qf_ref, d_ref = q0[inner_idx].copy(), q0[inner_idx].copy(), np.zeros((T, N))
        oracle.unit_route(A_in.indptr, A_in.indices, -c1i[A_in.indices], A_in.indptr, A_in.indices, A_in.data, A_hw.indptr, A_hw.indices, A_hw.data,
                          c1i, c2i, c3i, hw_idx, inner_idx, qc_ref, qf_ref, conv, d_ref, 1)
        want = (d_ref, qc_ref, qf_ref)
    else:
        M = 2
        sets = [[np.ascontiguousarray(np.stack(col)) for col in zip(*(coeff_set(net, indices, s0 + m) for m in range(M)))] for s0 in (0, 2)]
        qm = np.stack([q0 * (m + 1) for m in range(M)])
        with Plan(indptr, indices) as a:
            first, second = [], []
            for sets_k, res in zip(sets, (first, second)):
                a.set_member_coeffs(*sets_k)
                out = np.empty((M, T, N))
                states = a.rapid_route_members(qm, ql, out, 1)
                assert a.last_kernel() == kernel
                res += [out, states]
        fresh = [np.empty((M, T, N)), np.empty((M, N))]
        for m in range(M):      # B: the member's set as a fresh plan's own coefficients, the one-member ensemble call (the general tick on both sides)
            with Plan(indptr, indices) as b:
                b.set_coeffs(*(col[m] for col in sets[1]))
                fresh[1][m] = b.rapid_route_ensemble(qm[m], ql[None], fresh[0][m:m + 1], 1)[0]
                assert b.last_kernel() == kernel
        want = [np.zeros((M, T, N)), qm.copy()]
        for m in range(M):
            oracle.rapid_route(indptr, indices, *(col[m] for col in sets[0]), want[1][m], ql, want[0][m], 1)
    for k, (x, y) in enumerate(zip(second, fresh)):
        assert np.array_equal(bits(x), bits(y)), f'{path}: array {k} after the second set differs from a fresh plan\'s'
    assert not np.array_equal(first[0], second[0])      # (the two sets route differently)
    for k, (x, y) in enumerate(zip(first, want)):
        assert_close(x, y, f'{path}: array {k} of the first set against the oracle')
