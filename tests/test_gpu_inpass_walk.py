"""The batch walk of the in-pass (k_rec_in, plain and <..., HW>; DESIGN.md section 4, "Headwaters routed on the way in") at the smallest
shapes at which it can go wrong: a forest of 70 reaches -- three 32-column tiles, the last one of 6 columns and 26 replicas of column 69,
headwaters in every tile, lags with more than eight different lag % 16 -- over 128 x 5 + 37 rows: with RR_REC_BATCHES=4 four batches share one
workgroup walk and a short walk follows, with 8 one walk takes all six, with 1 every batch is a launch; the call's last rows fall inside a
register block of the headwater walk.  Every case is routed with RR_HW_INPASS=1 and =0, each side in a child process of its own (the switch is read
when a plan is made), and the two sides must agree byte for byte -- discharge rows and final state compared as uint64, so the signs of
zeros count (the headwater walk evaluates fma(c1row, 0.0, fma(c2, 0.0, r)) as r + 0.0: a zero state under zero or negative-zero laterals
is where that could differ).  The on side is checked against the oracle as the other GPU tests are (rtol 1e-10, atol 1e-10 max|want|).
The eligibility rule behind that arithmetic (rr_plan.hpp: mark_inpass_headwaters) is tested without a GPU in test_inpass_eligibility.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle
from river_route_amd import synth

N, T = 70, 128 * 5 + 37
CUT = 300      # the split call's first advance: no multiple of 128
BATCHES = ('1', '4', '8')
HERE = os.path.dirname(os.path.abspath(__file__))


def forest(n=N, seed=71, fan=3):
    """Reach i flows into one of the next `fan` reaches (at most three upstream reaches each: no wide tile), three outlets."""
    rng = np.random.default_rng(seed)
    down = np.arange(n) + 1 + rng.integers(0, fan, n)
    down[down >= n] = -1
    down[[24, 51, n - 1]] = -1
    return down.astype(np.int64)


def csc_from_down(down_index):
    has = down_index >= 0
    indptr = np.concatenate([[0], np.cumsum(has)]).astype(np.int32)
    return indptr, down_index[has].astype(np.int32)


def headwaters(down):
    return np.flatnonzero(np.bincount(down[down >= 0], minlength=down.size) == 0)


def inputs(kind):
    """(indptr, indices, coeffs, ql, q0).  Every forcing has headwater columns of exact 0.0 and of -0.0 (one of each in every column
    tile) and an inner column of each; kind 'state': a random initial state, 'zero': a zero one, 'inf': 'state' with a non-finite c2
    at one headwater (the plan leaves that column to k_tile)."""
    down = forest()
    indptr, indices = csc_from_down(down)
    k, x = 900.0 + 6300.0 * synth.u01(11, np.arange(N)), 0.05 + 0.4 * synth.u01(12, np.arange(N))
    c1, c2, c3 = oracle.muskingum_coefficients(k, x, 900.0)
    hw = headwaters(down)
    c4 = (c1 + c2) / 900.0
    if kind == 'inf':
        c2 = c2.copy()
        c2[hw[3]] = np.inf
    coeffs = (-c1[indices], c2, c3, c4)
    ql = synth.synth_qlateral(N, 0, T)
    ql[200:330] = 0.0      # whole rows of zeros, across a batch edge
    inner = np.setdiff1d(np.arange(N), hw)
    for tile in range(3):
        h = hw[(hw >= 32 * tile) & (hw < 32 * tile + 32)]
        ql[:, h[0]] = 0.0
        ql[:, h[-1]] = -0.0
    ql[:, inner[2]] = 0.0
    ql[:, inner[5]] = -0.0
    q0 = np.zeros(N) if kind == 'zero' else 2.0 * synth.u01(3, np.arange(N))
    return indptr, indices, coeffs, ql, q0


# ------------------------------------------------------------------------------------------------ the child process: one side, every case

def _route_dev(case, f32_in=False, eligible=None):
    from river_route_amd.engine import DeviceBuffer, Plan
    indptr, indices, coeffs, ql, q0 = case
    with Plan(indptr, indices) as plan:
        plan.set_coeffs(*coeffs)
        if eligible is not None:      # (the plan's count is the same on both sides of the switch: 'enabled' says which side this is)
            assert plan.inpass_info()['eligible'] == eligible, plan.inpass_info()
        src = ql.astype(np.float32) if f32_in else ql
        d_ql, d_q, d_out = DeviceBuffer(src.nbytes).upload(src), DeviceBuffer(N * 8).upload(q0), DeviceBuffer(T * N * 8)
        if f32_in:
            plan.rapid_route_f32in_dev(d_q, d_ql, T, T, 1, discharge=d_out, out_rows=T)
        else:
            plan.rapid_route_dev(d_q, d_ql, T, d_out, T, T, 1)
        assert plan.last_kernel() == 'tile'
        out, q = d_out.download(np.float64, (T, N)), d_q.download(np.float64, (N,))
        for b in (d_ql, d_q, d_out):
            b.free()
    return out, q


def _route_stream(case, cuts):
    import torch
    from river_route_amd.engine import Plan
    indptr, indices, coeffs, ql, q0 = case
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


def worker(path):
    """Every case on this process's side of the switch (RR_HW_INPASS is in the environment), the time-tiled kernel on records for every call."""
    os.environ['RR_DIRECT'] = '0'
    os.environ['RR_WAVE'] = '1'
    n_hw = headwaters(forest()).size
    res = {}

    def put(name, arrays):
        for k, a in enumerate(arrays):
            res[f'{name}.{k}'] = a
    for nb in BATCHES:
        os.environ['RR_REC_BATCHES'] = nb
        for kind in ('state', 'zero'):
            put(f'{kind}.f64.{nb}', _route_dev(inputs(kind), eligible=n_hw))
            put(f'{kind}.f32.{nb}', _route_dev(inputs(kind), f32_in=True))
    os.environ['RR_REC_BATCHES'] = '4'
    put('joint', _route_stream(inputs('state'), (T,)))
    put('split', _route_stream(inputs('state'), (CUT, T)))
    put('inf', _route_dev(inputs('inf'), eligible=n_hw - 1))
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
        path = str(tmp_path_factory.mktemp('inpass_walk') / f'side{side}.npz')
        env = dict(os.environ, RR_HW_INPASS=side, PYTHONPATH=os.pathsep.join([root, HERE, os.environ.get('PYTHONPATH', '')]))
        for k in ('RR_WAVE_K', 'RR_TILE_BLOCK', 'RR_TILE_LEAN', 'RR_UH_PAIRS', 'RR_REC_BATCHES'):
            env.pop(k, None)
        flags = ['-s'] if sys.flags.no_user_site else []
        r = subprocess.run([sys.executable, *flags, os.path.abspath(__file__), path], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, f'RR_HW_INPASS={side}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}'
        out[side] = dict(np.load(path))
    return out


@pytest.fixture(scope='module')
def refs():
    """The oracle per (kind, float32 rows): computed once, read only."""
    out = {}
    for kind in ('state', 'zero'):
        indptr, indices, coeffs, ql, q0 = inputs(kind)
        for f32 in (False, True):
            q_ref, d_ref = q0.copy(), np.zeros((T, N))
            oracle.rapid_route(indptr, indices, *coeffs, q_ref, ql.astype(np.float32).astype(np.float64) if f32 else ql, d_ref, 1)
            out[kind, f32] = (d_ref, q_ref)
    return out


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def same(sides, name):
    """Switch on against switch off, byte for byte.  Returns the on side's (discharge, final state)."""
    on, off = [[sides[s][f'{name}.{k}'] for k in range(2)] for s in ('1', '0')]
    for a, b, what in zip(on, off, ('discharge', 'final state')):
        assert a.shape == b.shape and np.array_equal(bits(a), bits(b)), f'{name}: {what} bits, RR_HW_INPASS=1 against 0'
    return on


def assert_close(got, want, what):
    scale = max(float(np.abs(want).max()), 1e-300)
    np.testing.assert_allclose(got, want, rtol=1e-10, atol=1e-10 * scale, err_msg=what)


def test_forest_shape():
    """What the cases rely on: three column tiles with a ragged last one, headwaters in each, several lag % 16, no wide confluence."""
    from river_route_amd._lib import RR_DEVICE_NONE
    from river_route_amd.engine import Plan
    down = forest()
    indptr, indices = csc_from_down(down)
    hw = headwaters(down)
    assert N % 32 not in (0, 1) and all(((hw >= 32 * t) & (hw < 32 * t + 32)).sum() >= 2 for t in range(3))
    assert np.bincount(indices, minlength=N).max() <= 3
    with Plan(indptr, indices, device=RR_DEVICE_NONE) as plan:
        L = plan.tile_layout()
    own = (L['lag'] & (1 << 28)) == 0
    lag = np.empty(N, dtype=np.int64)
    lag[L['perm'][own]] = L['lag'][own] & ((1 << 27) - 1)
    assert np.unique(lag[hw] % 16).size >= 8 and lag.max() >= 16
    assert T % 128 % 8 != 0 and CUT % 128 != 0


@pytest.mark.gpu
@pytest.mark.parametrize('nb', BATCHES)
@pytest.mark.parametrize('rows', ('f64', 'f32'))
@pytest.mark.parametrize('kind', ('state', 'zero'))
def test_walk(sides, refs, kind, rows, nb):
    d, q = same(sides, f'{kind}.{rows}.{nb}')
    d_ref, q_ref = refs[kind, rows == 'f32']
    assert_close(d, d_ref, 'discharge')
    assert_close(q, q_ref, 'final state')
    d4, q4 = (sides['1'][f'{kind}.{rows}.4.{k}'] for k in range(2))      # however many batches a launch walks: the same bytes
    assert np.array_equal(bits(d), bits(d4)) and np.array_equal(bits(q), bits(q4))


@pytest.mark.gpu
def test_zero_state_keeps_positive_zeros(sides):
    """A headwater that starts at zero under a 0.0 or -0.0 lateral column stays at +0.0, on both sides: the sign argument of the walk."""
    down = forest()
    hw = headwaters(down)
    ql = inputs('zero')[3]
    quiet = [h for h in hw if not ql[:, h].any()]
    assert any(np.signbit(ql[:, h]).all() for h in quiet) and any(not np.signbit(ql[:, h]).any() for h in quiet)
    for nb in BATCHES:
        for rows in ('f64', 'f32'):
            d, q = same(sides, f'zero.{rows}.{nb}')
            assert not bits(q[quiet]).any() and not bits(d[:, quiet]).any()


@pytest.mark.gpu
def test_split_call(sides, refs):
    """One call advanced in two parts, 300 + 377 rows, against one advance: the same bytes, on both sides."""
    ds, qs = same(sides, 'split')
    dj, qj = same(sides, 'joint')
    assert np.array_equal(bits(ds), bits(dj)), 'discharge: split against joint'
    assert np.array_equal(bits(qs), bits(qj)), 'final state: split against joint'
    assert_close(ds, refs['state', False][0], 'discharge')
    assert_close(qs, refs['state', False][1], 'final state')


@pytest.mark.gpu
def test_non_finite_c2_stays_with_k_tile(sides):
    """A headwater with a non-finite c2 is not the in-pass's (the worker checks the plan's count: one fewer): the same bytes either way."""
    d, q = same(sides, 'inf')
    assert np.isnan(q).any()      # fma(inf, 0.0, .) is a NaN in the tick: the case is what it claims to be
