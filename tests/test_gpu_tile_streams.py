"""k_tile with a cache policy per access stream (rr_kernels_tile.hpp: kTileStreams).  A cache hint cannot change arithmetic; what it could
expose is a value that is not seen across a launch or a call.  So the cases are the places where a store that may carry a hint is read
back by something else: the copy of a record into a ghost's slot, read by another tile one launch later (several tile levels, the ring
gone round); the carried state, read by the tile's next task and by the next call; and every other form that shares the code -- four
sub-steps per row (the 8-byte ghost store per tick), UnitMuskingum's short tick, the general tick, an ensemble, a partitioned network
(exports and boundary ghosts).

Every call runs in a child process (the knobs are read when a plan is made; one child per set of knobs routes its cases and hands the
arrays back in a file): RR_TILE_BLOCK=64 and RR_WAVE_K=32 for all of them -- about fifty tiles on several levels with ghosts between
them, tasks of two record chunks -- with RR_HW_INPASS 1 and 0 and with RR_TILE_LEAN=0.  Networks of about 3,000 reaches in random
order, 300 rows (and once 2,400: the ring gone round twice); against the oracle at the other GPU tests' tolerance (rtol 1e-10, atol 1e-10 max|want|)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle
from river_route_amd import synth

N, T, NSUB, MEMBERS = 3000, 300, 4, 3
T_LONG = 2400      # more than two revolutions of the record ring these knobs give (asserted)
CUTS = (97, 97 + 128, T)      # calls of 97, 128 and 75 rows
HERE = os.path.dirname(os.path.abspath(__file__))
SIDES = {'on': {'RR_HW_INPASS': '1'}, 'off': {'RR_HW_INPASS': '0'}, 'general': {'RR_HW_INPASS': '1', 'RR_TILE_LEAN': '0'}}
KNOBS = ('RR_WAVE_K', 'RR_TILE_BLOCK', 'RR_TILE_LEAN', 'RR_UH_PAIRS', 'RR_REC_BATCHES', 'RR_HW_INPASS', 'RR_WAVE', 'RR_DIRECT')


def csc_from_down(down_index):
    has = down_index >= 0
    indptr = np.concatenate([[0], np.cumsum(has)]).astype(np.int32)
    return indptr, down_index[has].astype(np.int32)


def network():
    net = synth.synth_network(N, seed=23)
    return net, csc_from_down(net.down_index)


def rapid_inputs(nsub=1, rows=T):
    """(indptr, indices, coeffs, lateral rows, a random initial state)"""
    net, (indptr, indices) = network()
    c1, c2, c3 = oracle.muskingum_coefficients(net.k, net.x, 900.0)
    coeffs = (-c1[indices], c2, c3, (c1 + c2) / (900.0 * nsub))
    return indptr, indices, coeffs, synth.synth_qlateral(N, 0, rows, dt=900.0 * nsub), 2.0 * synth.u01(3, np.arange(N))


def member_inputs():
    ql = np.stack([synth.synth_qlateral(N, 0, T, seed=100 + m) for m in range(MEMBERS)])
    q0 = np.stack([2.0 * synth.u01(50 + m, np.arange(N)) for m in range(MEMBERS)])
    return ql, q0


def unit_inputs():
    net, (indptr, indices) = network()
    c1, c2, c3 = oracle.muskingum_coefficients(net.k, net.x, 900.0)
    inner_idx = np.flatnonzero(np.bincount(indices, minlength=N) > 0)
    return indptr, indices, (c1, c2, c3), inner_idx, synth.synth_qlateral(N, 0, T) / 900.0, 5.0 * synth.u01(99, np.arange(N))


def two_part_network():
    """A random network with chain links cut in two (as test_gpu_headwater_inpass.two_part_network, without the moved headwater)."""
    from river_route_amd.engine import partition_forest
    net = synth.synth_network_chain(4000, seed=4, p_chain=0.3)
    part_of, _ = partition_forest(*csc_from_down(net.down_index), 2)
    return net, np.asarray(part_of)


# ------------------------------------------------------------------------------------------------ the child process: one set of knobs

def _rapid(inputs, nsub, info=None):
    from river_route_amd.engine import MODE_RAPID, DeviceBuffer, Plan
    indptr, indices, coeffs, ql, q0 = inputs
    rows = ql.shape[0]
    with Plan(indptr, indices) as plan:
        plan.set_coeffs(*coeffs)
        if info is not None:
            t = plan.tile_info()
            info.append(np.array([t['levels'], t['ghosts'], t['tiles'], plan.reserve(MODE_RAPID, rows, nsub)['ring_chunks']], dtype=np.int64))
        d_ql, d_q, d_out = DeviceBuffer(ql.nbytes).upload(ql), DeviceBuffer(N * 8).upload(q0), DeviceBuffer(rows * N * 8)
        plan.rapid_route_dev(d_q, d_ql, rows, d_out, rows, rows, nsub)
        assert plan.last_kernel() == 'tile'
        got = d_out.download(np.float64, (rows, N)), d_q.download(np.float64, (N,))
        for b in (d_ql, d_q, d_out):
            b.free()
    return got


def _calls(inputs, cuts):
    """One session advanced to each of `cuts` rows in turn: the state crosses tasks, launches and calls."""
    import torch
    from river_route_amd.engine import Plan
    indptr, indices, coeffs, ql, q0 = inputs
    dev = torch.device('cuda:0')
    with Plan(indptr, indices) as plan:
        plan.set_coeffs(*coeffs)
        q, lat = torch.from_numpy(q0.copy()).to(dev), torch.from_numpy(ql).to(dev)
        out = torch.zeros((T, N), dtype=torch.float64, device=dev)
        plan.stream_begin(q, lat, T, out, T, T, 1, stream=torch.cuda.current_stream().cuda_stream)
        for c in cuts:
            plan.stream_advance(c, c)
        plan.stream_end(q)
        torch.cuda.synchronize()
        assert plan.last_kernel() == 'tile'
        return out.cpu().numpy(), q.cpu().numpy()


def _ensemble():
    from river_route_amd.engine import Plan
    indptr, indices, coeffs, _, _ = rapid_inputs()
    ql, q0 = member_inputs()
    out = np.empty((MEMBERS, T, N))
    with Plan(indptr, indices) as plan:
        plan.set_coeffs(*coeffs)
        states = plan.rapid_route_ensemble(q0, ql, out, 1)
        assert plan.last_kernel() == 'tile_ensemble'
    return out, states


def _unit():
    from river_route_amd.engine import DeviceBuffer, Plan
    indptr, indices, (c1, c2, c3), inner_idx, conv, q0 = unit_inputs()
    ni = inner_idx.size
    with Plan(indptr, indices) as plan:
        plan.set_coeffs(-c1[indices], c2, c3, None)
        d_qc, d_qf = DeviceBuffer(ni * 8).upload(0.5 * q0[inner_idx]), DeviceBuffer(ni * 8).upload(q0[inner_idx].copy())
        d_conv, d_out = DeviceBuffer(conv.nbytes).upload(conv), DeviceBuffer(T * N * 8)
        plan.unit_route_dev(d_qc, d_qf, d_conv, T, d_out, T, T, 1)
        assert plan.last_kernel() == 'tile'
        got = d_out.download(np.float64, (T, N)), d_qf.download(np.float64, (ni,)), d_qc.download(np.float64, (ni,))
        for b in (d_qc, d_qf, d_conv, d_out):
            b.free()
    return got


def _parts():
    from river_route_amd.multi_gpu import HipPartEngine, run_sequential, split_network
    net, part_of = two_part_network()
    n = net.n
    c1, c2, c3 = oracle.muskingum_coefficients(net.k, net.x, 900.0)
    q0, ql = 4.0 * synth.u01(8, np.arange(n)), synth.synth_qlateral(n, 0, T)
    specs = [split_network(net.down_index, part_of, p, 2) for p in range(2)]
    q, d = np.zeros(n), np.zeros((T, n))

    def visit(s, e):
        q[s.real_global] = e.final_state()
        d[:, s.real_global] = e.discharge.cpu().numpy()[:, s.n_ghost:]
    run_sequential(specs, lambda s: HipPartEngine(s, c1, c2, c3, (c1 + c2) / 900.0, q0, ql[:, s.real_global], T, 1, 0, out_rows=T), T, 1, visit=visit)
    return d, q, np.array([sum(s.n_ghost for s in specs)], dtype=np.int64)


def worker(path, side):
    os.environ.update(RR_DIRECT='0', RR_WAVE='1', RR_TILE_BLOCK='64', RR_WAVE_K='32', **SIDES[side])
    res = {}

    def put(name, arrays):
        for k, a in enumerate(arrays):
            res[f'{name}.{k}'] = a
    info = []
    put('one_call', _rapid(rapid_inputs(), 1, info))
    res['info'] = info[0]
    if side != 'general':
        put('long', _rapid(rapid_inputs(rows=T_LONG), 1, info))
        res['info_long'] = info[1]
    if side == 'on':
        put('joint', _calls(rapid_inputs(), (T,)))
        put('split', _calls(rapid_inputs(), CUTS))
        put('substeps', _rapid(rapid_inputs(NSUB), NSUB))
        put('unit', _unit())
        put('ensemble', _ensemble())
        put('parts', _parts())
    np.savez(path, **res)


if __name__ == '__main__':
    worker(sys.argv[1], sys.argv[2])
    sys.exit(0)


# ------------------------------------------------------------------------------------------------ the tests

_SIDES = {}


@pytest.fixture(scope='module')
def routed(tmp_path_factory):
    """side -> the arrays its child process routed (each child runs once, when a test first asks for its side)."""
    root = os.path.dirname(HERE)
    tmp = tmp_path_factory.mktemp('tile_streams')

    def get(side):
        if side not in _SIDES:
            path = str(tmp / f'{side}.npz')
            env = dict(os.environ, PYTHONPATH=os.pathsep.join([root, HERE, os.environ.get('PYTHONPATH', '')]))
            for k in KNOBS:
                env.pop(k, None)
            flags = ['-s'] if sys.flags.no_user_site else []
            r = subprocess.run([sys.executable, *flags, os.path.abspath(__file__), path, side], env=env, capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, f'{side}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}'
            _SIDES[side] = dict(np.load(path))
        return _SIDES[side]
    return get


def assert_close(got, want, what):
    scale = max(float(np.abs(want).max()), 1e-300)
    np.testing.assert_allclose(got, want, rtol=1e-10, atol=1e-10 * scale, err_msg=what)


def bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


@pytest.fixture(scope='module')
def rapid_ref():
    """The oracle on the 300-row call, one sub-step per row: shared, read only."""
    indptr, indices, coeffs, ql, q0 = rapid_inputs()
    q, d = q0.copy(), np.zeros((T, N))
    oracle.rapid_route(indptr, indices, *coeffs, q, ql, d, 1)
    return d, q


@pytest.mark.gpu
def test_ghost_copies_across_levels(routed, rapid_ref):
    """Tiles on three levels and more with ghosts between them: a ghost's record is stored by the tile that owns the reach and loaded by
    the ghost's tile one launch later.  Both sides of RR_HW_INPASS (k_tile stores a headwater's record, or never does) agree bit for bit."""
    on, off = routed('on'), routed('off')
    levels, ghosts, tiles, ring_chunks = (int(v) for v in on['info'])
    print(f'tiles {tiles}, levels {levels}, ghosts {ghosts}, ring of {ring_chunks} chunks = {16 * ring_chunks} tick-rows for {T} rows')
    assert levels >= 3 and ghosts > 0
    assert np.array_equal(on['info'], off['info'])
    assert bits_equal(on['one_call.0'], off['one_call.0']), 'discharge: RR_HW_INPASS=1 against 0'
    assert bits_equal(on['one_call.1'], off['one_call.1']), 'final state: RR_HW_INPASS=1 against 0'
    assert_close(on['one_call.0'], rapid_ref[0], 'discharge')
    assert_close(on['one_call.1'], rapid_ref[1], 'final state')


@pytest.mark.gpu
def test_ring_goes_round_twice(routed):
    """The 300-row calls above stay inside one revolution of the ring these knobs give (its length is the deepest lag plus levels x K
    tick-rows plus the batches in flight).  2,400 rows go round it more than twice: a ghost's slot is stored over what an earlier
    revolution left there, and the load one launch later must see the new copy."""
    on, off = routed('on'), routed('off')
    ring_rows = 16 * int(on['info_long'][3])
    print(f'ring of {ring_rows} tick-rows for {T_LONG} rows')
    assert 2 * ring_rows < T_LONG and int(on['info_long'][0]) >= 3 and int(on['info_long'][1]) > 0
    assert bits_equal(on['long.0'], off['long.0']), 'discharge: RR_HW_INPASS=1 against 0'
    assert bits_equal(on['long.1'], off['long.1']), 'final state: RR_HW_INPASS=1 against 0'
    indptr, indices, coeffs, ql, q0 = rapid_inputs(rows=T_LONG)
    q, d = q0.copy(), np.zeros((T_LONG, N))
    oracle.rapid_route(indptr, indices, *coeffs, q, ql, d, 1)
    assert_close(on['long.0'], d, 'discharge')
    assert_close(on['long.1'], q, 'final state')


@pytest.mark.gpu
def test_state_across_tasks_and_calls(routed, rapid_ref):
    """One call of 300 rows against calls of 97, 128 and 75 rows: the carried state is stored at the end of a task and loaded by the
    tile's next task, one launch or one call later.  The same bits."""
    on = routed('on')
    assert bits_equal(on['split.0'], on['joint.0']), 'discharge: three calls against one'
    assert bits_equal(on['split.1'], on['joint.1']), 'final state: three calls against one'
    assert bits_equal(on['joint.0'], on['one_call.0']) and bits_equal(on['joint.1'], on['one_call.1']), 'the session against the single call'
    assert_close(on['split.0'], rapid_ref[0], 'discharge')
    assert_close(on['split.1'], rapid_ref[1], 'final state')


@pytest.mark.gpu
def test_four_substeps_per_row(routed):
    """With sub-steps a mirrored reach sends 8 bytes per tick into its ghost's record, and the interval sum is carried state."""
    indptr, indices, coeffs, ql, q0 = rapid_inputs(NSUB)
    q, d = q0.copy(), np.zeros((T, N))
    oracle.rapid_route(indptr, indices, *coeffs, q, ql, d, NSUB)
    on = routed('on')
    assert_close(on['substeps.0'], d, 'discharge')
    assert_close(on['substeps.1'], q, 'final state')


@pytest.mark.gpu
def test_unit_muskingum_short_tick(routed):
    from conftest import unit_split
    indptr, indices, (c1, c2, c3), inner_idx, conv, q0 = unit_inputs()
    hw_idx, inner, A_in, A_hw = unit_split(indptr, indices, N)
    assert np.array_equal(inner, inner_idx)
    c1i, c2i, c3i = c1[inner_idx], c2[inner_idx], c3[inner_idx]
    qc, qf, d = 0.5 * q0[inner_idx], q0[inner_idx].copy(), np.zeros((T, N))
    oracle.unit_route(A_in.indptr, A_in.indices, -c1i[A_in.indices], A_in.indptr, A_in.indices, A_in.data, A_hw.indptr, A_hw.indices, A_hw.data,
                      c1i, c2i, c3i, hw_idx, inner_idx, qc, qf, conv, d, 1)
    on = routed('on')
    assert_close(on['unit.0'], d, 'discharge')
    assert_close(on['unit.1'], qf, 'q_full')
    assert_close(on['unit.2'], qc, 'q_ch')


@pytest.mark.gpu
def test_general_tick(routed, rapid_ref):
    """RR_TILE_LEAN=0: every tile goes through the general tick."""
    gen = routed('general')
    assert int(gen['info'][0]) >= 3 and int(gen['info'][1]) > 0
    assert_close(gen['one_call.0'], rapid_ref[0], 'discharge')
    assert_close(gen['one_call.1'], rapid_ref[1], 'final state')


@pytest.mark.gpu
def test_ensemble_of_three(routed):
    indptr, indices, coeffs, _, _ = rapid_inputs()
    ql, q0 = member_inputs()
    on = routed('on')
    for m in range(MEMBERS):
        q, d = q0[m].copy(), np.zeros((T, N))
        oracle.rapid_route(indptr, indices, *coeffs, q, ql[m], d, 1)
        assert_close(on['ensemble.0'][m], d, f'member {m}: discharge')
        assert_close(on['ensemble.1'][m], q, f'member {m}: final state')


@pytest.mark.gpu
def test_two_part_network(routed):
    """run_sequential over two parts: the upstream part's exports are the downstream part's boundary ghosts."""
    net, _ = two_part_network()
    n = net.n
    indptr, indices = csc_from_down(net.down_index)
    c1, c2, c3 = oracle.muskingum_coefficients(net.k, net.x, 900.0)
    q, d = 4.0 * synth.u01(8, np.arange(n)), np.zeros((T, n))
    oracle.rapid_route(indptr, indices, -c1[indices], c2, c3, (c1 + c2) / 900.0, q, synth.synth_qlateral(n, 0, T), d, 1)
    on = routed('on')
    assert int(on['parts.2'][0]) > 0, 'no boundary ghost'
    assert_close(on['parts.0'], d, 'discharge')
    assert_close(on['parts.1'], q, 'final state')
