"""The record passes with a cache policy per access stream (rr_kernels_rec.hpp: kRecStreams) and up to eight batches per launch, at the
call lengths at which the multi-batch walk is the default (16,384 tick-rows and more): every case is routed with one batch per launch
(RR_REC_BATCHES=1, the reference form) and again on a fresh plan with the default count and with eight forced, and the discharge rows or
float32 means and the final state must be the same bytes.  The first rows are checked against the oracle as the other GPU tests are.

Network: 2,999 reaches -- 94 column tiles, the last one of 23 columns, a row pitch that is no multiple of a 128-byte line, lags of every
offset lag % 16 (test_network_shape).  Rows: 16,384 (128 batches: whole groups of eight), 16,385 (a group that ends one row in) and
16,384 + 8 x 128 + 77 (an odd tail).  Forms: float64 rows in and out; float32 rows in with float32 means out, factor 1 and -- where the
row count is a multiple of it, as the entry point demands -- factor 4; RR_HW_INPASS 0 and 1.  One call split in two through
rr_stream_advance at a row that is no multiple of 128, where the finished batches are no whole group.  One plan whose ring allocation the device refuses once (RR_ALLOC_FAIL_AT): it
takes fewer batches per launch, a shorter ring (Plan.reserve's ring_chunks), and still gives the reference's bytes.

A float32 mean is the float32 rounding of a double that is within 1e-10 (of the largest discharge) of the oracle's: it may differ from
the rounded oracle mean by that plus one float32 unit in the last place, rtol 2^-23."""
import hashlib
import os

import numpy as np
import pytest

from conftest import assert_close
from oracle import oracle
from river_route_amd import synth

N = 2999
ROWS = (16384, 16385, 16384 + 8 * 128 + 77)
T_MAX = max(ROWS)
CUT = 5200      # the split call's first advance: no multiple of 128, and the batches finished by then (37) no multiple of four
HEAD = 256      # rows checked against the oracle
KNOBS = ('RR_WAVE', 'RR_WAVE_K', 'RR_TILE_BLOCK', 'RR_TILE_LEAN', 'RR_UH_PAIRS', 'RR_DIRECT', 'RR_HW_INPASS', 'RR_REC_BATCHES', 'RR_ALLOC_FAIL_AT')
FORMS = {'f64': None, 'f32x1': 1, 'f32x4': 4}      # form -> factor of the float32 means (None: float64 rows in and out)
CASES = [(T, form, hw) for T in ROWS for form in FORMS for hw in ('1', '0') if FORMS[form] is None or T % FORMS[form] == 0]


def csc_from_down(down_index):
    has = down_index >= 0
    indptr = np.concatenate([[0], np.cumsum(has)]).astype(np.int32)
    return indptr, down_index[has].astype(np.int32)


@pytest.fixture(scope='module')
def case():
    """(indptr, indices, coeffs, float64 lateral rows, their float32 copy, initial state): made once, read only."""
    net = synth.synth_network(N, seed=23)
    indptr, indices = csc_from_down(net.down_index)
    c1, c2, c3 = oracle.muskingum_coefficients(net.k, net.x, 900.0)
    coeffs = (-c1[indices], c2, c3, (c1 + c2) / 900.0)
    ql = synth.synth_qlateral(N, 0, T_MAX)
    q0 = 2.0 * synth.u01(3, np.arange(N))
    for a in (ql, q0):
        a.setflags(write=False)
    ql32 = ql.astype(np.float32)
    ql32.setflags(write=False)
    return indptr, indices, coeffs, ql, ql32, q0


@pytest.fixture(scope='module')
def heads(case):
    """The oracle's first HEAD rows per form: float64 rows; float32 means of the rows routed from the float32 laterals."""
    indptr, indices, coeffs, ql, ql32, q0 = case
    out = {}
    q, d = q0.copy(), np.zeros((HEAD, N))
    oracle.rapid_route(indptr, indices, *coeffs, q, np.ascontiguousarray(ql[:HEAD]), d, 1)
    out['f64'] = d
    q, d = q0.copy(), np.zeros((HEAD, N))
    oracle.rapid_route(indptr, indices, *coeffs, q, ql32[:HEAD].astype(np.float64), d, 1)
    for form, factor in FORMS.items():
        if factor is not None:
            out[form] = d.reshape(HEAD // factor, factor, N).mean(axis=1)
    return out


def set_side(monkeypatch, nb, hw):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv('RR_DIRECT', '0')
    monkeypatch.setenv('RR_HW_INPASS', hw)
    if nb != 'default':
        monkeypatch.setenv('RR_REC_BATCHES', nb)


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def arm(k):
    """The k-th device allocation from here on is refused once (0: none): the switch is read by rr_plan_create -- here of a host-only
    plan, which allocates nothing on the device."""
    from river_route_amd._lib import RR_DEVICE_NONE
    from river_route_amd.engine import Plan
    os.environ['RR_ALLOC_FAIL_AT'] = str(k)
    try:
        Plan(np.zeros(2, np.int32), np.zeros(0, np.int32), device=RR_DEVICE_NONE).close()
    finally:
        del os.environ['RR_ALLOC_FAIL_AT']


def route(case, T, form, refuse_ring=False):
    """One call on a fresh plan: (rows or float32 means, final state, Plan.reserve's answer, k_rec_out launches)."""
    from river_route_amd.engine import MODE_RAPID, DeviceBuffer, Plan
    indptr, indices, coeffs, ql, ql32, q0 = case
    factor = FORMS[form]
    with Plan(indptr, indices) as plan:
        plan.set_coeffs(*coeffs)
        plan.set_options(sample_every=128)
        if refuse_ring:      # the next device allocation of the process -- the ring, rr_plan_reserve's first -- is refused once
            arm(1)
        try:
            info = plan.reserve(MODE_RAPID, T, 1, f32_out=factor is not None)
        finally:
            if refuse_ring:
                arm(0)
        src = (ql if factor is None else ql32)[:T]
        rows = T if factor is None else T // factor
        d_ql, d_q = DeviceBuffer(src.nbytes).upload(src), DeviceBuffer(N * 8).upload(q0)
        d_out = DeviceBuffer(rows * N * (8 if factor is None else 4))
        if factor is None:
            plan.rapid_route_dev(d_q, d_ql, T, d_out, T, T, 1)
        else:
            plan.rapid_route_f32in_dev(d_q, d_ql, T, T, 1, discharge32=d_out, factor=factor)
        assert plan.last_kernel() == 'tile'
        launches = plan.profile_aux()['k_rec_out']['launches']
        out = d_out.download(np.float64 if factor is None else np.float32, (rows, N))
        q = d_q.download(np.float64, (N,))
        for b in (d_ql, d_q, d_out):
            b.free()
    return out, q, info, launches


_REFERENCE = {}


def reference(monkeypatch, case, T, form, hw):
    """The call with one batch per launch: digests of its rows and final state, its first rows; routed once per (T, form, hw)."""
    key = (T, form, hw)
    if key not in _REFERENCE:
        set_side(monkeypatch, '1', hw)
        out, q, info, launches = route(case, T, form)
        assert launches == (T + 127) // 128, launches      # one batch per launch
        _REFERENCE[key] = (digest(out), digest(q), out[:HEAD // (FORMS[form] or 1)].copy(), info)
    return _REFERENCE[key]


def check_head(form, got, heads):
    want = heads[form]
    if FORMS[form] is None:
        assert_close(got, want, 'first rows against the oracle')
    else:
        scale = float(np.abs(want).max())
        np.testing.assert_allclose(got.astype(np.float64), want, rtol=2.0 ** -23, atol=1e-10 * scale, err_msg='first float32 means against the oracle')


def test_network_shape():
    """What the cases rely on: a ragged last column tile, a row pitch that shares 128-byte lines between tiles, every lag % 16."""
    from river_route_amd._lib import RR_DEVICE_NONE
    from river_route_amd.engine import Plan
    net = synth.synth_network(N, seed=23)
    indptr, indices = csc_from_down(net.down_index)
    with Plan(indptr, indices, device=RR_DEVICE_NONE) as plan:
        L = plan.tile_layout()
    own = (L['lag'] & (1 << 28)) == 0
    lag = np.empty(N, dtype=np.int64)
    lag[L['perm'][own]] = L['lag'][own] & ((1 << 27) - 1)
    assert N % 32 not in (0, 1) and N % 16 != 0
    assert np.unique(lag % 16).size == 16 and lag.max() >= 16
    assert [T % 128 for T in ROWS] == [0, 1, 77] and ROWS[0] // 128 % 8 == 0 and CUT % 128 != 0 and all(T >= 16384 for T in ROWS)


@pytest.mark.gpu
@pytest.mark.parametrize('nb', ('default', '8'))
@pytest.mark.parametrize('T,form,hw', CASES)
def test_same_bytes_as_one_batch_per_launch(monkeypatch, case, heads, T, form, hw, nb):
    ref_out, ref_q, ref_head, _ = reference(monkeypatch, case, T, form, hw)
    set_side(monkeypatch, nb, hw)
    out, q, info, launches = route(case, T, form)
    assert info['tiled'], info
    assert launches < (T + 127) // 128, launches      # several batches per launch
    if nb == '8':
        assert launches >= ((T + 127) // 128 + 7) // 8
    assert digest(out) == ref_out, f'rows differ from RR_REC_BATCHES=1: first difference in the head {np.argwhere(out[:ref_head.shape[0]] != ref_head)[:1]}'
    assert digest(q) == ref_q, 'final state differs from RR_REC_BATCHES=1'
    check_head(form, out[:ref_head.shape[0]], heads)


def split_route(case, T):
    """The call advanced to CUT rows, then to its end, on a fresh plan: (rows, final state, rows that were out when the first advance returned)."""
    from river_route_amd.engine import DeviceBuffer, Plan, synchronize
    indptr, indices, coeffs, ql, ql32, q0 = case
    with Plan(indptr, indices) as plan:
        plan.set_coeffs(*coeffs)
        d_ql, d_q = DeviceBuffer(T * N * 8).upload(ql[:T]), DeviceBuffer(N * 8).upload(q0)
        d_out = DeviceBuffer(T * N * 8).upload(np.full((T, N), -1.0))      # no discharge is negative: a row of -1 has not been written
        plan.stream_begin(d_q, d_ql, T, d_out, T, T, 1)
        plan.stream_advance(CUT, CUT)
        synchronize()
        first = d_out.download(np.float64, (CUT, N))
        written = (first != -1.0).all(axis=1)
        rows_out = int(written.sum())
        assert written[:rows_out].all() and not (first[rows_out:] != -1.0).any()      # whole rows, in order
        plan.stream_advance(T, T)
        plan.stream_end(d_q)
        synchronize()
        assert plan.last_kernel() == 'tile'
        got, got_q = d_out.download(np.float64, (T, N)), d_q.download(np.float64, (N,))
        for buf in (d_ql, d_q, d_out):
            buf.free()
    return got, got_q, rows_out


_SPLIT_ROWS_OUT = {}


@pytest.mark.gpu
@pytest.mark.parametrize('nb', ('default', '8'))
def test_split_call(monkeypatch, case, heads, nb):
    """rr_stream_begin / advance / end, 5,200 rows then the rest: the first advance returns with every finished row out -- as many as
    with one batch per launch, although fewer than a whole group were left -- and the call gives the bytes of the undivided call with
    one batch per launch."""
    T = ROWS[2]
    ref_out, ref_q, _, _ = reference(monkeypatch, case, T, 'f64', '1')
    if not _SPLIT_ROWS_OUT:
        set_side(monkeypatch, '1', '1')
        _SPLIT_ROWS_OUT['1'] = split_route(case, T)[2]
    set_side(monkeypatch, nb, '1')
    got, got_q, rows_out = split_route(case, T)
    print(f'rows out after the first advance of {CUT}: {rows_out} (one batch per launch: {_SPLIT_ROWS_OUT["1"]})')
    assert rows_out == _SPLIT_ROWS_OUT['1'] and rows_out >= 128 and rows_out % 128 == 0 and rows_out // 128 % 4 != 0
    assert digest(got) == ref_out, 'rows: split call against the undivided call with RR_REC_BATCHES=1'
    assert digest(got_q) == ref_q, 'final state: split call against the undivided call with RR_REC_BATCHES=1'
    check_head('f64', got[:HEAD], heads)


@pytest.mark.gpu
def test_refused_ring_takes_fewer_batches(monkeypatch, case, heads):
    """The ring of the default count does not fit (the device refuses it once): the plan takes half as many batches per launch -- a ring
    shorter by the batches the out-pass no longer holds back, one batch of eight chunks each -- before it would shorten its tasks."""
    T = ROWS[0]
    ref_out, ref_q, _, _ = reference(monkeypatch, case, T, 'f64', '1')
    set_side(monkeypatch, 'default', '1')
    _, _, whole, launches_whole = route(case, T, 'f64')
    out, q, short, launches_short = route(case, T, 'f64', refuse_ring=True)
    print(f'ring as asked for: {whole}, {launches_whole} k_rec_out launches; after one refusal: {short}, {launches_short} launches')
    assert short['tiled'] and short['ticks_per_launch'] == whole['ticks_per_launch'], (whole, short)
    assert short['ring_chunks'] == whole['ring_chunks'] - 8 * 2, (whole, short)      # four batches per launch -> two
    assert launches_short > launches_whole and launches_short >= T // 128 // 2
    assert digest(out) == ref_out and digest(q) == ref_q
    check_head('f64', out[:HEAD], heads)
