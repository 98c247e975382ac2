"""Headwaters routed by the in-pass (k_rec_in<..., HW>, RR_HW_INPASS): k_tile publishes their records and never
stores them.  Every case is routed twice, with RR_HW_INPASS=1 and =0, each side in a child process of its own (the switch is read when
a plan is made; one child per side routes every case and hands the arrays back in a file), and the two sides must agree exactly:
discharge rows bit for bit (they are clamped: no negative zero), final states value for value.  One side is checked against the
oracle as the other GPU tests are (rtol 1e-10, atol 1e-10 max|want|).  Networks are a few thousand reaches: there is a skeleton, so
there are ghosts, and headwaters that hang directly off skeleton reaches (mirrored: left to k_tile)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle
from river_route_amd import synth
from river_route_amd._lib import RR_DEVICE_NONE
from river_route_amd.engine import Plan

N, T_SHORT, T_LONG = 3000, 300, 1100
HERE = os.path.dirname(os.path.abspath(__file__))


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


def mixed_network(n, confluences=3, fan=5):
    """The random network with a few confluences of seven reaches: some tiles go to the general kernel's companion launch, the others
    stay with the short tick -- in wide_network at this size every tile holds a wide confluence."""
    down = synth.synth_network(n, seed=23).down_index.copy()
    hw = np.flatnonzero(np.bincount(down[down >= 0], minlength=n) == 0)
    rng = np.random.default_rng(7)
    for j in range(confluences):
        t = int(rng.integers(n // 2, n - 1))
        down[hw[hw < t][j * fan:(j + 1) * fan]] = t      # (upstream reaches keep their smaller indices)
    return down


def rapid_inputs(down, T, kind='plain'):
    """(indptr, indices, coeffs, ql, q0): kind 'plain' zero initial state; 'state' a random one; 'zeros' a forcing with exact zeros,
    a headwater column and an inner column of negative laterals, zeros in the initial state."""
    n = down.size
    indptr, indices = csc_from_down(down)
    k, x = 900.0 + 6300.0 * synth.u01(11, np.arange(n)), 0.05 + 0.4 * synth.u01(12, np.arange(n))
    c1, c2, c3 = oracle.muskingum_coefficients(k, x, 900.0)
    coeffs = (-c1[indices], c2, c3, (c1 + c2) / 900.0)
    ql = synth.synth_qlateral(n, 0, T)
    q0 = np.zeros(n) if kind == 'plain' else 2.0 * synth.u01(3, np.arange(n))
    if kind == 'zeros':
        indeg = np.bincount(down[down >= 0], minlength=n)
        hw, inner = np.flatnonzero(indeg == 0), np.flatnonzero(indeg > 0)
        ql[40:170] = 0.0                      # whole rows of zeros, across a batch edge
        ql[:, hw[1::5]] = 0.0                 # headwater columns that never see inflow
        ql[:, hw[2]] = -np.abs(ql[:, hw[2]]) - 1e-3      # negative laterals: the record is unclamped, the rows are clamped
        ql[:, inner[3]] = -np.abs(ql[:, inner[3]]) - 1e-3
        q0[hw[::3]] = 0.0
    return indptr, indices, coeffs, ql, q0


def two_part_network():
    """A random network with chain links cut in two, then one headwater h of the downstream part whose downstream reach has no other upstream reach
    moved into the upstream part: h is a headwater that is an export, and downstream a boundary ghost feeds an otherwise upstream-less
    reach."""
    from river_route_amd.engine import partition_forest
    net = synth.synth_network_chain(4000, seed=4, p_chain=0.3)      # (the plain random network is binary: no reach has one inflow)
    down = net.down_index
    indptr, indices = csc_from_down(down)
    part_of, _ = partition_forest(indptr, indices, 2)
    part_of = np.asarray(part_of).copy()
    indeg = np.bincount(down[down >= 0], minlength=net.n)
    cand = [i for i in np.flatnonzero(indeg == 0) if down[i] >= 0 and indeg[down[i]] == 1 and part_of[i] == 1 and part_of[down[i]] == 1]
    assert cand, 'no headwater with a single-inflow downstream reach in the downstream part'
    part_of[cand[0]] = 0
    return net, part_of, int(cand[0])


# ------------------------------------------------------------------------------------------------ the child process: one side, every case

def _route_dev(inputs, T, f32_in=False):
    from river_route_amd.engine import DeviceBuffer
    indptr, indices, coeffs, ql, q0 = inputs
    n = q0.size
    with Plan(indptr, indices) as plan:
        plan.set_coeffs(*coeffs)
        src = ql.astype(np.float32) if f32_in else ql
        d_ql, d_q, d_out = DeviceBuffer(src.nbytes).upload(src), DeviceBuffer(n * 8).upload(q0), DeviceBuffer(T * n * 8)
        if f32_in:
            plan.rapid_route_f32in_dev(d_q, d_ql, T, T, 1, discharge=d_out, out_rows=T)
        else:
            plan.rapid_route_dev(d_q, d_ql, T, d_out, T, T, 1)
        assert plan.last_kernel() == 'tile'
        out, q = d_out.download(np.float64, (T, n)), d_q.download(np.float64, (n,))
        for b in (d_ql, d_q, d_out):
            b.free()
    return out, q


def _route_stream(inputs, T, cuts):
    import torch
    indptr, indices, coeffs, ql, q0 = inputs
    dev = torch.device('cuda:0')
    with Plan(indptr, indices) as plan:
        plan.set_coeffs(*coeffs)
        q, lat = torch.from_numpy(q0.copy()).to(dev), torch.from_numpy(ql).to(dev)
        out = torch.zeros((T, q0.size), dtype=torch.float64, device=dev)
        plan.stream_begin(q, lat, T, out, T, T, 1, stream=torch.cuda.current_stream().cuda_stream)
        for c in cuts:
            plan.stream_advance(c, c)
        plan.stream_end(q)
        torch.cuda.synchronize()
        assert plan.last_kernel() == 'tile'
        return out.cpu().numpy(), q.cpu().numpy()


def _route_parts():
    from river_route_amd.multi_gpu import HipPartEngine, run_sequential, split_network
    net, part_of, _ = two_part_network()
    n, T = net.n, T_SHORT
    c1, c2, c3 = oracle.muskingum_coefficients(net.k, net.x, 900.0)
    q0, ql = 4.0 * synth.u01(8, np.arange(n)), synth.synth_qlateral(n, 0, T)
    specs = [split_network(net.down_index, part_of, p, 2) for p in range(2)]
    q, d = np.zeros(n), np.zeros((T, n))

    def visit(s, e):
        q[s.real_global] = e.final_state()
        d[:, s.real_global] = e.discharge.cpu().numpy()[:, s.n_ghost:]
    run_sequential(specs, lambda s: HipPartEngine(s, c1, c2, c3, (c1 + c2) / 900.0, q0, ql[:, s.real_global], T, 1, 0, out_rows=T), T, 1, visit=visit)
    return d, q


def _route_unit(n=3000, T=200, n_ks=16):
    from river_route_amd.engine import DeviceBuffer
    net = synth.synth_network(n, seed=23)
    indptr, indices = csc_from_down(net.down_index)
    indeg = np.bincount(indices, minlength=n)
    inner_idx = np.flatnonzero(indeg > 0)
    c1, c2, c3 = oracle.muskingum_coefficients(net.k, net.x, 900.0)
    kern, depth = synth.synth_uh_kernel(n, n_ks), synth.synth_runoff_depth(n, 0, T)
    state, ni = 3.0 * synth.u01(7, np.arange(n)), inner_idx.size
    with Plan(indptr, indices) as plan:
        plan.set_coeffs(-c1[indices], c2, c3, None)
        d_kern, d_state = DeviceBuffer(kern.nbytes).upload(kern), DeviceBuffer(kern.nbytes).upload(np.zeros_like(kern))
        d_depth, d_out, d_fin = DeviceBuffer(T * n * 8).upload(depth), DeviceBuffer(T * n * 8), DeviceBuffer(n * 8)
        d_qc, d_qf = DeviceBuffer(ni * 8).upload(state[inner_idx].copy()), DeviceBuffer(ni * 8).upload(state[inner_idx].copy())
        plan.unit_route_uh_dev(d_qc, d_qf, d_fin, d_kern, d_state, n_ks, d_depth, T, 1, discharge=d_out)
        assert plan.last_kernel() == 'tile'
        got = (d_out.download(np.float64, (T, n)), d_fin.download(np.float64, (n,)), d_qc.download(np.float64, (ni,)))
        for b in (d_kern, d_state, d_depth, d_out, d_fin, d_qc, d_qf):
            b.free()
    return got


def worker(path):
    """Every case on this process's side of the switch (RR_HW_INPASS is in the environment), records for every call."""
    os.environ['RR_DIRECT'] = '0'
    os.environ['RR_WAVE'] = '1'
    down = synth.synth_network(N, seed=23).down_index
    res = {}

    def put(name, arrays):
        for k, a in enumerate(arrays):
            res[f'{name}.{k}'] = a
    put('skeleton', _route_dev(rapid_inputs(down, T_SHORT), T_SHORT))
    for nb in ('4', '1'):
        os.environ['RR_REC_BATCHES'] = nb
        put(f'batches{nb}', _route_dev(rapid_inputs(down, T_LONG, 'state'), T_LONG))
    del os.environ['RR_REC_BATCHES']
    put('state', _route_dev(rapid_inputs(down, T_SHORT, 'state'), T_SHORT))
    put('f32in', _route_dev(rapid_inputs(down, T_SHORT, 'state'), T_SHORT, f32_in=True))
    put('joint', _route_stream(rapid_inputs(down, T_SHORT, 'state'), T_SHORT, (T_SHORT,)))
    put('split', _route_stream(rapid_inputs(down, T_SHORT, 'state'), T_SHORT, (131, T_SHORT)))
    put('zeros', _route_dev(rapid_inputs(down, T_SHORT, 'zeros'), T_SHORT))
    put('wide', _route_dev(rapid_inputs(wide_network(N), T_SHORT, 'state'), T_SHORT))
    put('mixed', _route_dev(rapid_inputs(mixed_network(N), T_SHORT, 'state'), T_SHORT))
    put('parts', _route_parts())
    put('unit', _route_unit())
    np.savez(path, **res)


if __name__ == '__main__':
    worker(sys.argv[1])
    sys.exit(0)


# ------------------------------------------------------------------------------------------------ the tests

@pytest.fixture(scope='module')
def sides(tmp_path_factory):
    """{'1': arrays, '0': arrays}: one child process per side of the switch."""
    out = {}
    root = os.path.dirname(HERE)
    for side in ('1', '0'):
        path = str(tmp_path_factory.mktemp('hw_inpass') / f'side{side}.npz')
        env = dict(os.environ, RR_HW_INPASS=side, PYTHONPATH=os.pathsep.join([root, HERE, os.environ.get('PYTHONPATH', '')]))
        for k in ('RR_WAVE_K', 'RR_TILE_BLOCK', 'RR_TILE_LEAN', 'RR_UH_PAIRS', 'RR_REC_BATCHES'):
            env.pop(k, None)
        flags = ['-s'] if sys.flags.no_user_site else []
        r = subprocess.run([sys.executable, *flags, os.path.abspath(__file__), path], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, f'RR_HW_INPASS={side}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}'
        out[side] = dict(np.load(path))
    return out


def assert_close(got, want, what):
    scale = max(float(np.abs(want).max()), 1e-300)
    np.testing.assert_allclose(got, want, rtol=1e-10, atol=1e-10 * scale, err_msg=what)


def same(sides, name, what=('discharge', 'final state')):
    """Switch on against switch off: discharge rows bit for bit, every other array value for value.  Returns the on side's arrays."""
    on = [sides['1'][f'{name}.{k}'] for k in range(len(what))]
    off = [sides['0'][f'{name}.{k}'] for k in range(len(what))]
    assert on[0].shape == off[0].shape and np.array_equal(on[0].view(np.int64), off[0].view(np.int64)), f'{name}: {what[0]} bits'
    for a, b, w in zip(on[1:], off[1:], what[1:]):
        np.testing.assert_array_equal(a, b, err_msg=f'{name}: {w}')
    return on


def rapid_oracle(inputs, T, f32_in=False):
    indptr, indices, coeffs, ql, q0 = inputs
    q_ref, d_ref = q0.copy(), np.zeros((T, q0.size))
    oracle.rapid_route(indptr, indices, *coeffs, q_ref, ql.astype(np.float32).astype(np.float64) if f32_in else ql, d_ref, 1)
    return d_ref, q_ref


@pytest.fixture(scope='module')
def down():
    return synth.synth_network(N, seed=23).down_index


@pytest.fixture(scope='module')
def state_ref(down):
    """The oracle on the 300-row call with a random initial state: shared, read only."""
    return rapid_oracle(rapid_inputs(down, T_SHORT, 'state'), T_SHORT)


@pytest.mark.gpu
def test_skeleton_present(sides, down):
    """T = 300: no multiple of 128, shorter than depth + levels x K, so the pipeline's fill and drain use the tested tasks."""
    indptr, indices = csc_from_down(down)
    with Plan(indptr, indices, device=RR_DEVICE_NONE) as plan:
        info, hw = plan.tile_info(), plan.inpass_info()
    assert info['levels'] > 1 and info['ghosts'] > 0 and hw['mirrored_or_boundary'] > 0 and hw['eligible'] > 1000
    d, q = same(sides, 'skeleton')
    d_ref, q_ref = rapid_oracle(rapid_inputs(down, T_SHORT), T_SHORT)
    assert_close(d, d_ref, 'discharge')
    assert_close(q, q_ref, 'final state')


@pytest.mark.gpu
def test_multi_batch_walk(sides, down):
    """T = 1,100 is nine batches: the carry crosses batches inside a launch (RR_REC_BATCHES=4) and launches (=1 too)."""
    d4, q4 = same(sides, 'batches4')
    d1, q1 = same(sides, 'batches1')
    assert np.array_equal(d4.view(np.int64), d1.view(np.int64)) and np.array_equal(q4, q1)
    d_ref, q_ref = rapid_oracle(rapid_inputs(down, T_LONG, 'state'), T_LONG)
    assert_close(d4, d_ref, 'discharge')
    assert_close(q4, q_ref, 'final state')


@pytest.mark.gpu
def test_non_zero_initial_state(sides, state_ref):
    d, q = same(sides, 'state')
    assert_close(d, state_ref[0], 'discharge')
    assert_close(q, state_ref[1], 'final state')


@pytest.mark.gpu
def test_float32_rows_in(sides, down):
    d, q = same(sides, 'f32in')
    d_ref, q_ref = rapid_oracle(rapid_inputs(down, T_SHORT, 'state'), T_SHORT, f32_in=True)
    assert_close(d, d_ref, 'discharge')
    assert_close(q, q_ref, 'final state')


@pytest.mark.gpu
def test_split_call(sides, state_ref):
    """The streaming session advanced in two uneven parts (131 + 169 rows) against one advance: the same bits, on both sides."""
    ds, qs = same(sides, 'split')
    dj, qj = same(sides, 'joint')
    assert np.array_equal(ds.view(np.int64), dj.view(np.int64)), 'discharge: split against joint'
    np.testing.assert_array_equal(qs, qj, err_msg='final state: split against joint')
    assert_close(ds, state_ref[0], 'discharge')
    assert_close(qs, state_ref[1], 'final state')


@pytest.mark.gpu
def test_signed_zeros(sides, down):
    d, q = same(sides, 'zeros')
    assert not np.signbit(d).any()      # clamped rows: no negative value, no negative zero
    d_ref, q_ref = rapid_oracle(rapid_inputs(down, T_SHORT, 'zeros'), T_SHORT)
    assert_close(d, d_ref, 'discharge')
    assert_close(q, q_ref, 'final state')


@pytest.mark.gpu
def test_wide_confluence(sides):
    """Tiles with a reach of more than three upstream reaches go to the companion launch of the general kernel: their headwaters stay there."""
    for name, wd in (('wide', wide_network(N)), ('mixed', mixed_network(N))):
        indptr, indices = csc_from_down(wd)
        assert np.bincount(indices, minlength=N).max() > 3
        with Plan(indptr, indices, device=RR_DEVICE_NONE) as plan:
            hw = plan.inpass_info()
        assert hw['wide_tile'] > 0 and (hw['eligible'] > 0 or name == 'wide')      # mixed: tiles of both kinds in one launch
        d, q = same(sides, name)
        d_ref, q_ref = rapid_oracle(rapid_inputs(wd, T_SHORT, 'state'), T_SHORT)
        assert_close(d, d_ref, f'{name}: discharge')
        assert_close(q, q_ref, f'{name}: final state')


@pytest.mark.gpu
def test_partitioned(sides):
    net, part_of, h = two_part_network()
    assert part_of[h] == 0 and part_of[net.down_index[h]] == 1
    d, q = same(sides, 'parts')
    n = net.n
    indptr, indices = csc_from_down(net.down_index)
    c1, c2, c3 = oracle.muskingum_coefficients(net.k, net.x, 900.0)
    q_ref, d_ref = 4.0 * synth.u01(8, np.arange(n)), np.zeros((T_SHORT, n))
    oracle.rapid_route(indptr, indices, -c1[indices], c2, c3, (c1 + c2) / 900.0, q_ref, synth.synth_qlateral(n, 0, T_SHORT), d_ref, 1)
    assert_close(d, d_ref, 'discharge')
    assert_close(q, q_ref, 'final state')


@pytest.mark.gpu
def test_unit_muskingum(sides):
    """UnitMuskingum's short tick drops the store of a headwater's record, which it never changes: switch on against off, exact."""
    same(sides, 'unit', ('discharge', 'router state', 'q_ch'))


def test_eligibility_count():
    """Host side only: the plan's count against the tile layout -- positions that own a reach and have no upstream position, minus the
    mirrored ones (bit 27 of lag) and those in a tile with a reach of more than three upstream positions; boundary ghosts leave too."""
    for down_index in (synth.synth_network(N, seed=23).down_index, wide_network(N), mixed_network(N)):
        indptr, indices = csc_from_down(down_index)
        with Plan(indptr, indices, device=RR_DEVICE_NONE) as plan:
            L, hw = plan.tile_layout(), plan.inpass_info()
            own = (L['lag'] & (1 << 28)) == 0
            head = own & ((L['ccnt'] & 0xFFFF) == 0)
            mirrored = head & ((L['lag'] & (1 << 27)) != 0)
            wide_tiles = np.array([((L['ccnt'][a:b] & 0xFFFF) > 3).any() for a, b in zip(L['tile_ptr'][:-1], L['tile_ptr'][1:])])
            in_wide = np.repeat(wide_tiles, np.diff(L['tile_ptr']))
            indeg = np.bincount(indices, minlength=down_index.size)
            assert hw['headwater_positions'] == head.sum() == (indeg == 0).sum()      # a headwater has no upstream position, a reach with one has
            assert hw['mirrored_or_boundary'] == mirrored.sum()
            assert hw['wide_tile'] == (head & ~mirrored & in_wide).sum()
            assert hw['eligible'] == (head & ~mirrored & ~in_wide).sum() == hw['headwater_positions'] - hw['mirrored_or_boundary'] - hw['wide_tile']
            ghosts = np.flatnonzero(indeg == 0)[:7]      # as boundary ghosts of a partitioned network these headwaters leave
            plan.set_boundary(ghosts, np.array([], dtype=np.int64))
            hb = plan.inpass_info()
            left = (~mirrored[L_inv(L, ghosts)] & ~in_wide[L_inv(L, ghosts)]).sum()
            assert hb['eligible'] == hw['eligible'] - left and hb['headwater_positions'] == hw['headwater_positions']


def L_inv(L, reaches):
    """Positions that own the given reaches."""
    own = np.flatnonzero((L['lag'] & (1 << 28)) == 0)
    pos = np.empty(L['perm'].max() + 1, dtype=np.int64)
    pos[L['perm'][own]] = own
    return pos[reaches]
