"""The record in-pass with the gridded-runoff aggregation fused in (k_rec_in_runoff, rr_rapid_route_runoff_dev) through
Plan.rapid_route_runoff_dev, at the shapes where its own edge logic decides: a record's 16 rows start at
128 batch + 16 k - (lag % 16), the 16-byte gather is taken only for records that lie inside a grid point's row, rows outside
[0, T) become zeros, the row before a record is read for cumulative input only, a call whose length is a multiple of 128 keeps
its last rows in a batch of their own, and the ring slot is chunk mod rec_chunks.

Two references for every call.  The oracle: oracle.runoff_to_qlateral_core, then oracle.rapid_route (rtol 1e-10,
atol 1e-10 max|want|; float32 means: rtol 3e-7 against the float64 means).  And the two-step form on the same plan and device
arrays -- rr_runoff_to_qlateral_dev into (T, n) rows, then the routing call on those rows -- which the kernel's comment says it
repeats ("same gather, same rounding, same post-processing"): discharge rows bit for bit, final state value for value.

The network (3,000 reaches, seed 23) has 7 tiles on 2 levels with 56 mirrored ghost positions and lags up to 112 with every value
of lag % 16; the fixture asserts that, so a planner change cannot take the edges away unnoticed.  The runoff block comes in every
layout the header allows: point-major with rows padded to a multiple of 16 (the padding poisoned with NaN or 1e300, not the zeros
the routers write: the kernel promises not to use those rows), unpadded (stride_p = T), stride_p = T + 5 (also poisoned), and
time-major.

Why these cases bite.  Take `t0 = 128 batch + 16 k - o + 1` in k_rec_in_runoff (one row late at every lag offset).  The kernel
then gathers rows t0 .. t0 + 15 correctly but stores them in the record of ticks one earlier: the slot of row r of every reach
holds the inflow of row r + 1, and the slot of row T - 1 holds zero (row T fails the `t < T` test).  The runoff rows are independent
draws from [-0.3, 1.7] mm over 400 points and the areas 1e5 .. 5e7 m2, so consecutive inflow rows of a reach differ by about
their own size: every reach with a weight row differs from the oracle and from the two-step form in every row of every case, far
outside 1e-10.  Were the slip confined to some lag offsets (o = 5 only, say) the 170 to 220 reaches with that offset would differ
in the same way, and every offset is present.  At T = 128 the rows T - o .. T - 1 of a reach with o > 0 are written by batch 1
(its record k = 0 starts at 128 - o): a kernel that skipped that batch, or zeroed rows from 128 - o on, would leave those rows
without inflow in 2,800 reaches.  A gather that reads one element too far takes its last row from the poison: 1e300 (inf as
float32) survives the NaN fill and the clip and comes out as a discharge of 1e300 or inf; NaN is filled with zero, which is not
the inflow of that row either.  (The `t < T` test where the staged record is written is not covered by any of this and cannot be:
k_tile never reads a record slot of a tick outside the call, so what the in-pass writes there does not reach a result.)"""
import functools

import numpy as np
import pytest

from conftest import assert_close
from test_gpu_tiles import csc_from_down, set_env
from test_runoff import random_weights

from oracle import oracle
from river_route_amd import engine, synth
from river_route_amd._lib import RR_DEVICE_NONE, RR_E_INVALID, RR_E_UNSUPPORTED, RRError
from river_route_amd.engine import MODE_RAPID, DeviceBuffer, Plan

pytestmark = pytest.mark.gpu

N, N_POINTS = 3000, 400
LENGTHS = [(33, False), (128, False), (129, False), (200, False), (300, False), (5, True), (17, True)]      # (T, RR_WAVE=1)
LAYOUTS = ['padded', 'tight', 'plus5', 'time_major']
FLAG_DTYPES = [(cum, clip, dt) for cum in (False, True) for clip in (False, True) for dt in ('float32', 'float64')]
OUTPUTS = [('f64', 1), ('f32', 1), ('f32', 4), ('f32', 8)]


class Inputs:
    """A bag of arrays (hashable by identity: the cached references are keyed on it)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


@pytest.fixture(scope='module')
def net():
    """The network, its coefficients, the weights and areas; shared, read only."""
    sn = synth.synth_network(N, seed=23)
    indptr, indices = csc_from_down(sn.down_index)
    with Plan(indptr, indices, device=RR_DEVICE_NONE) as plan:
        perm, lag, _ = plan.layout()
        info = plan.tile_info()
    assert (info['tiles'], info['levels'], info['ghosts']) == (7, 2, 56)
    assert lag.max() == 112 and sorted(set(lag % 16)) == list(range(16)) and int((lag >= 16).sum()) == 2840
    lag_of = np.empty(N, dtype=np.int64)
    lag_of[perm] = lag
    c1, c2, c3 = oracle.muskingum_coefficients(sn.k, sn.x, 900.0)
    rng = np.random.default_rng(3)
    W = random_weights(rng, N, N_POINTS)
    assert (np.diff(W.indptr) == 0).any()      # empty weight rows
    area = rng.uniform(1e5, 5e7, N)
    return Inputs(indptr=indptr, indices=indices, coeffs=(-c1[indices], c2, c3, (c1 + c2) / 900.0), W=W, area=area,
                  lag=lag_of, q0=2.0 * synth.u01(3, np.arange(N)), w_ptr=W.indptr.astype(np.int32),
                  w_idx=W.indices.astype(np.int32), w_data=W.data.astype(np.float64))


@functools.lru_cache(maxsize=None)
def make_runoff(T, dtype, cumulative, seed=0):
    """As test_gpu_runoff.case, in metres: -0.3 .. 1.7 mm so that clipping matters, a handful of NaNs, the cumulative variant with
    its NaN.  Read only."""
    rng = np.random.default_rng(seed + T)
    runoff = ((rng.random((T, N_POINTS)) * 2.0 - 0.3) * 1e-3).astype(dtype)
    runoff[rng.integers(0, T, 7), rng.integers(0, N_POINTS, 7)] = np.nan
    if cumulative:
        runoff = np.cumsum(np.nan_to_num(runoff), axis=0).astype(dtype)
        runoff[T // 2, 3] = np.nan
    runoff.flags.writeable = False
    return runoff


def oracle_route(net, runoff, cumulative, clip, with_area, q0):
    ql = oracle.runoff_to_qlateral_core(net.W, runoff, net.area if with_area else None, cumulative, clip)
    q_ref, d_ref = q0.copy(), np.zeros((runoff.shape[0], N))
    oracle.rapid_route(net.indptr, net.indices, *net.coeffs, q_ref, ql, d_ref, 1)
    return d_ref, q_ref


@functools.lru_cache(maxsize=None)
def reference(net, T, dtype, cumulative, clip, with_area, state):
    """(discharge rows, final state) of the oracle for one set of inputs: computed once, read only."""
    d_ref, q_ref = oracle_route(net, make_runoff(T, dtype, cumulative), cumulative, clip, with_area, net.q0 if state else np.zeros(N))
    d_ref.flags.writeable = q_ref.flags.writeable = False
    return d_ref, q_ref


def lay_out(runoff, layout, poison=np.nan):
    """(host block, stride_t, stride_p) of the (T, points) runoff in one of the layouts of rr_rapid_route_runoff_dev."""
    T = runoff.shape[0]
    if layout == 'time_major':
        return np.ascontiguousarray(runoff), N_POINTS, 1
    stride_p = {'padded': -(-T // 16) * 16, 'tight': T, 'plus5': T + 5}[layout]
    with np.errstate(over='ignore'):
        block = np.full((N_POINTS, stride_p), poison).astype(runoff.dtype)      # (1e300 is inf as float32)
    block[:, :T] = runoff.T
    return block, 1, stride_p


def flags_of(cumulative, clip):
    return (engine.RUNOFF_CUMULATIVE if cumulative else 0) | (engine.RUNOFF_FORCE_POSITIVE if clip else 0)


def route_both(net, plan, runoff, layout, poison, flags, with_area, out, q0):
    """One fused call and the two-step form on the same plan and device arrays -> (rows, state) of each.  The output arrays start
    as NaN, so a row that is not written shows."""
    T, (kind, factor) = runoff.shape[0], out
    block, stride_t, stride_p = lay_out(runoff, layout, poison)
    f32 = runoff.dtype == np.float32
    out_dtype, rows = (np.float64, T) if kind == 'f64' else (np.float32, T // factor)
    blank = np.full((rows, N), np.nan, dtype=out_dtype)
    up = lambda a: DeviceBuffer(a.nbytes).upload(a)      # noqa: E731
    d_block, d_ptr, d_idx, d_w = up(block), up(net.w_ptr), up(net.w_idx), up(net.w_data)
    d_area = up(net.area) if with_area else None
    d_q, d_q2, d_out, d_out2, d_lat = up(q0), up(q0), up(blank), up(blank), DeviceBuffer(T * N * 8)
    bufs = [b for b in (d_block, d_ptr, d_idx, d_w, d_area, d_q, d_q2, d_out, d_out2, d_lat) if b is not None]
    try:
        kw = dict(discharge=d_out) if kind == 'f64' else dict(discharge32=d_out, factor=factor)
        plan.rapid_route_runoff_dev(d_q, N_POINTS, d_ptr, d_idx, d_w, d_block, f32, stride_t, stride_p, d_area, flags, T, **kw)
        assert plan.last_kernel() == 'tile'
        fused = d_out.download(out_dtype, (rows, N)), d_q.download(np.float64, (N,))
        engine.runoff_to_qlateral_dev(N, N_POINTS, T, d_ptr, d_idx, d_w, d_block, f32, stride_t, stride_p, d_area, flags, d_lat)
        if kind == 'f64':
            plan.rapid_route_dev(d_q2, d_lat, T, d_out2, T, T, 1)
        else:
            plan.rapid_route_f32_dev(d_q2, d_lat, T, d_out2, T, 1, factor)
        assert plan.last_kernel() == 'tile'
        two_step = d_out2.download(out_dtype, (rows, N)), d_q2.download(np.float64, (N,))
    finally:
        for b in bufs:
            b.free()
    return fused, two_step


def check(net, fused, two_step, ref, out, what):
    """The fused call against the oracle (to tolerance) and against the two-step form (exactly)."""
    (d, q), (d2, q2), (d_ref, q_ref), (kind, factor) = fused, two_step, ref, out
    if kind == 'f64':
        assert_close(d, d_ref, f'{what}: discharge')
    else:
        want = d_ref.reshape(d_ref.shape[0] // factor, factor, N).mean(axis=1)
        np.testing.assert_allclose(d, want, rtol=3e-7, atol=1e-10 * np.abs(want).max(), err_msg=f'{what}: float32 means of {factor}')
    assert_close(q, q_ref, f'{what}: final state')
    bits = np.int64 if kind == 'f64' else np.int32
    differ = np.argwhere(d.view(bits) != d2.view(bits))
    if differ.size:
        row, reach = (int(v) for v in differ[0])
        raise AssertionError(f'{what}: {differ.shape[0]} discharge values differ from the two-step form; the first in output row {row}, '
                             f'reach {reach} (lag {net.lag[reach]}, lag % 16 = {net.lag[reach] % 16}): {d[row, reach]!r} against {d2[row, reach]!r}')
    assert (q == q2).all(), f'{what}: final state differs from the two-step form at reaches {np.flatnonzero(q != q2)[:8]}'


def cases():
    """Every (layout, T) pair; the other axes cycle underneath so that every (flags, dtype) pair, both area settings, every output
    form and both initial states appear (test_axes_are_covered)."""
    out = []
    for li, layout in enumerate(LAYOUTS):
        for ti, (T, wave) in enumerate(LENGTHS):
            c = li * len(LENGTHS) + ti
            cumulative, clip, dtype = FLAG_DTYPES[c % 8]
            kind, factor = OUTPUTS[c % 4]
            if T % factor:
                kind, factor = OUTPUTS[(c // 4) % 2]
            poison = 1e300 if ti % 2 else np.nan      # (T = 128 has no padding in the padded layout; 33, 129, 200, 300, 5, 17 have)
            out.append(pytest.param(layout, T, wave, poison, dtype, cumulative, clip, c % 3 != 0, (kind, factor), c % 3 != 1,
                                    id=f'{layout}-T{T}-{dtype}-cum{int(cumulative)}-clip{int(clip)}-area{int(c % 3 != 0)}-{kind}x{factor}-state{int(c % 3 != 1)}'))
    return out


def test_axes_are_covered():
    v = [p.values for p in cases()]
    assert {(a[0], a[1]) for a in v} == {(lay, T) for lay in LAYOUTS for T, _ in LENGTHS}
    assert {(a[5], a[6], a[4]) for a in v} == set(FLAG_DTYPES)
    assert {a[7] for a in v} == {True, False} and {a[8] for a in v} == set(OUTPUTS)
    assert sum(a[9] for a in v) * 2 >= len(v) and not all(a[9] for a in v)
    padded = [(a[1], a[3]) for a in v if a[0] == 'padded' and a[1] % 16]
    assert any(np.isnan(p) for _, p in padded) and any(p == 1e300 for _, p in padded)


@pytest.mark.parametrize('layout,T,wave,poison,dtype,cumulative,clip,with_area,out,state', cases())
def test_fused_call_vs_oracle_and_two_step(monkeypatch, net, layout, T, wave, poison, dtype, cumulative, clip, with_area, out, state):
    """The exact comparison with the two-step form held in every case on the MI355X (no differing value at any shape or lag offset)."""
    set_env(monkeypatch, {'RR_WAVE': '1'} if wave else {})
    runoff = make_runoff(T, dtype, cumulative)
    with Plan(net.indptr, net.indices) as plan:
        plan.set_coeffs(*net.coeffs)
        assert plan.reserve(MODE_RAPID, T, 1, plain_rows=False)['tiled']
        fused, two_step = route_both(net, plan, runoff, layout, poison, flags_of(cumulative, clip), with_area, out,
                                     net.q0 if state else np.zeros(N))
    check(net, fused, two_step, reference(net, T, dtype, cumulative, clip, with_area, state), out, f'{layout} T={T}')


RING_T = 1313      # the smallest: depth 113 and 2 levels of 16-tick tasks keep (112 + 32) // 16 + 4 x 8 = 41 chunks, 41 x 32 = 1,312


def test_the_ring_goes_round(monkeypatch, net):
    """One call more than twice as long as the record ring (RR_WAVE_K=16: the shortest tasks, so the shortest ring): every slot is
    reused, chunk mod rec_chunks with it.  Cumulative float32 runoff, the production layout."""
    set_env(monkeypatch, {'RR_WAVE_K': '16'})
    runoff = make_runoff(RING_T, 'float32', True)
    with Plan(net.indptr, net.indices) as plan:
        plan.set_coeffs(*net.coeffs)
        info = plan.reserve(MODE_RAPID, RING_T, 1, plain_rows=False)
        print(f'T = {RING_T}: {info}')
        assert info['tiled'] and info['ring_chunks'] * 16 * 2 < RING_T, info
        fused, two_step = route_both(net, plan, runoff, 'padded', np.nan, flags_of(True, False), True, ('f64', 1), net.q0)
    check(net, fused, two_step, oracle_route(net, runoff, True, False, True, net.q0), ('f64', 1), f'ring, T={RING_T}')


def test_split_call(net):
    """T = 300 routed as 200 + 100 rows with the state carried in q_t.  The second call's block is rows 200 .. 299 of the same
    cumulative series, and a cumulative block's row 0 is kept as it is: the reference is the oracle on that sub-block, carried
    the same way."""
    runoff = make_runoff(300, 'float64', True)
    flags, q = flags_of(True, True), net.q0
    with Plan(net.indptr, net.indices) as plan:
        plan.set_coeffs(*net.coeffs)
        for part in (runoff[:200], runoff[200:]):
            d_ref, q_ref = oracle_route(net, part, True, True, True, q)
            fused, two_step = route_both(net, plan, part, 'padded', np.nan, flags, True, ('f64', 1), q)
            check(net, fused, two_step, (d_ref, q_ref), ('f64', 1), f'split call, {part.shape[0]} rows')
            q = fused[1]      # the device's own state goes on


@pytest.mark.parametrize('T,factor,code', [(24, 1, RR_E_UNSUPPORTED), (96, 3, RR_E_UNSUPPORTED), (96, 5, RR_E_INVALID)],
                         ids=['24_rows', '128_not_a_multiple_of_3', '96_not_a_multiple_of_5'])
def test_refusals_leave_everything_alone(monkeypatch, net, T, factor, code):
    """Fewer than 32 rows without RR_WAVE, a float32 factor that does not divide a batch of 128, one that does not divide the call:
    RRError with the code the header gives, the state and the output array untouched -- RapidMuskingum's fall-back to the two-step
    form goes on from them."""
    set_env(monkeypatch, {})
    runoff = make_runoff(T, 'float32', False)
    block, stride_t, stride_p = lay_out(runoff, 'padded', 0.0)
    sentinel = np.full((T, N), -12345.0, dtype=np.float32)
    up = lambda a: DeviceBuffer(a.nbytes).upload(a)      # noqa: E731
    with Plan(net.indptr, net.indices) as plan:
        plan.set_coeffs(*net.coeffs)
        bufs = [up(block), up(net.w_ptr), up(net.w_idx), up(net.w_data), up(net.area), up(net.q0), up(sentinel)]
        d_block, d_ptr, d_idx, d_w, d_area, d_q, d_out = bufs
        try:
            with pytest.raises(RRError) as e:
                plan.rapid_route_runoff_dev(d_q, N_POINTS, d_ptr, d_idx, d_w, d_block, True, stride_t, stride_p, d_area, 0, T,
                                            discharge32=d_out, factor=factor)
            assert e.value.code == code
            engine.synchronize()
            np.testing.assert_array_equal(d_q.download(np.float64, (N,)), net.q0)
            np.testing.assert_array_equal(d_out.download(np.float32, (T, N)), sentinel)
        finally:
            for b in bufs:
                b.free()
