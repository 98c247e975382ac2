"""The record passes over several batches per launch (k_rec_in / k_rec_out, RR_REC_BATCHES): a call routed with one batch per launch
and the same call with four -- the knob forces them into calls of any length -- give the same bits: discharge rows, float32 means,
final states.  One case of each group is checked against the oracle too.  The knob is read when a plan is created, so each side
routes on a plan of its own; RR_DIRECT=0 keeps every call on records."""
import numpy as np
import pytest

from conftest import assert_close
from oracle import oracle
from river_route_amd import synth
from river_route_amd.engine import DeviceBuffer, Plan

pytestmark = pytest.mark.gpu
KNOBS = ('RR_WAVE', 'RR_WAVE_K', 'RR_TILE_BLOCK', 'RR_TILE_LEAN', 'RR_UH_PAIRS', 'RR_DIRECT', 'RR_REC_BATCHES')
SIDES = ('1', '4')


def csc_from_down(down_index):
    has = down_index >= 0
    indptr = np.concatenate([[0], np.cumsum(has)]).astype(np.int32)
    return indptr, down_index[has].astype(np.int32)


def set_side(monkeypatch, nb, extra=None):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv('RR_DIRECT', '0')
    monkeypatch.setenv('RR_REC_BATCHES', nb)
    for k, v in (extra or {}).items():
        monkeypatch.setenv(k, v)


def bits(a):
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def assert_same_bits(a, b, what):
    for x, y, w in zip(a, b, what):
        assert x.shape == y.shape and np.array_equal(bits(x), bits(y)), w


def rapid_case(n, T, nsub, seed):
    net = synth.synth_network(n, seed=seed)
    indptr, indices = csc_from_down(net.down_index)
    c1, c2, c3 = oracle.muskingum_coefficients(net.k, net.x, 900.0 / nsub)
    coeffs = (-c1[indices], c2, c3, (c1 + c2) / 900.0)
    ql = synth.synth_qlateral(n, 0, T)
    q0 = 2.0 * synth.u01(3, np.arange(n))
    return indptr, indices, coeffs, ql, q0


def route(case, T, nsub, f32_in=False, big_endian=False, factor=None):
    """One call on a fresh plan: (discharge rows or float32 means, final state, k_rec_in / k_rec_out launches)."""
    indptr, indices, coeffs, ql, q0 = case
    n = q0.size
    with Plan(indptr, indices) as plan:
        plan.set_coeffs(*coeffs)
        plan.set_options(sample_every=128)
        if big_endian:
            plan.set_row_format(in32_big_endian=True)
        src = ql.astype('>f4' if big_endian else np.float32) if f32_in else ql
        d_ql, d_q = DeviceBuffer(src.nbytes).upload(src), DeviceBuffer(n * 8).upload(q0)
        rows = T if factor is None else T // factor
        d_out = DeviceBuffer(rows * n * (8 if factor is None else 4))
        if f32_in and factor is None:
            plan.rapid_route_f32in_dev(d_q, d_ql, T, T, nsub, discharge=d_out, out_rows=T)
        elif f32_in:
            plan.rapid_route_f32in_dev(d_q, d_ql, T, T, nsub, discharge32=d_out, factor=factor)
        elif factor is None:
            plan.rapid_route_dev(d_q, d_ql, T, d_out, T, T, nsub)
        else:
            plan.rapid_route_f32_dev(d_q, d_ql, T, d_out, T, nsub, factor)
        assert plan.last_kernel() == 'tile'
        aux = plan.profile_aux()
        out = d_out.download(np.float64 if factor is None else np.float32, (rows, n))
        q = d_q.download(np.float64, (n,))
        for b in (d_ql, d_q, d_out):
            b.free()
    return out, q, (aux['k_rec_in']['launches'], aux['k_rec_out']['launches'])


# T below one batch, between one and four, not a multiple of four batches; sub-steps 2-4; a last column tile of 7 columns
@pytest.mark.parametrize('n,T,nsub,oracle_check', [(60_000, 1100, 1, True), (60_000, 50, 1, False), (60_000, 300, 1, False),
                                                   (60_007, 700, 1, False), (60_000, 200, 2, True), (60_000, 150, 3, False),
                                                   (60_000, 100, 4, False)])
def test_float64_rows(monkeypatch, n, T, nsub, oracle_check):
    case = rapid_case(n, T, nsub, seed=23)
    got = []
    for nb in SIDES:
        set_side(monkeypatch, nb)
        got.append(route(case, T, nsub))
    (d1, q1, l1), (d4, q4, l4) = got
    assert_same_bits((d1, q1), (d4, q4), ('discharge', 'final state'))
    total = T * nsub
    assert l1 == ((total + 14) // 128 + 1, (total + 127) // 128)      # one batch per launch
    if total > 128:
        assert l4[0] < l1[0] and l4[1] < l1[1], (l1, l4)      # several per launch
    if oracle_check:
        indptr, indices, coeffs, ql, q0 = case
        q_ref, d_ref = q0.copy(), np.zeros((T, q0.size))
        oracle.rapid_route(indptr, indices, *coeffs, q_ref, ql, d_ref, nsub)
        assert_close(d4, d_ref, 'discharge')
        assert_close(q4, q_ref, 'final state')


@pytest.mark.parametrize('n,T,nsub,big_endian', [(60_000, 700, 1, False), (60_000, 700, 1, True), (50_001, 300, 2, True)])
def test_float32_rows_in(monkeypatch, n, T, nsub, big_endian):
    """k_rec_in<..., IN32>: float32 lateral rows, a big-endian file's bytes as they are too; the same bits as the native float32 rows."""
    case = rapid_case(n, T, nsub, seed=41)
    got = []
    for nb in SIDES:
        set_side(monkeypatch, nb)
        got.append(route(case, T, nsub, f32_in=True, big_endian=big_endian))
    assert_same_bits(got[0][:2], got[1][:2], ('discharge', 'final state'))
    native = route(case, T, nsub, f32_in=True)
    assert_same_bits(got[1][:2], native[:2], ('discharge against native float32 rows', 'final state against native float32 rows'))
    if not big_endian:      # the float32 rows are exact in float64: the oracle on their float64 copy
        indptr, indices, coeffs, ql, q0 = case
        q_ref, d_ref = q0.copy(), np.zeros((T, q0.size))
        oracle.rapid_route(indptr, indices, *coeffs, q_ref, ql.astype(np.float32).astype(np.float64), d_ref, nsub)
        assert_close(got[1][0], d_ref, 'discharge')


@pytest.mark.parametrize('n,T,nsub,factor', [(60_000, 1000, 1, 1), (60_000, 1000, 1, 4), (60_000, 1024, 1, 128), (60_000, 600, 2, 4)])
def test_float32_means_out(monkeypatch, n, T, nsub, factor):
    """k_rec_out<..., OUT32>: float32 means of `factor` rows; an output row never spans two batches (128 % (factor x nsub) == 0)."""
    case = rapid_case(n, T, nsub, seed=17)
    got = []
    for nb in SIDES:
        set_side(monkeypatch, nb)
        got.append(route(case, T, nsub, factor=factor))
    assert_same_bits(got[0][:2], got[1][:2], ('float32 means', 'final state'))
    if factor == 4 and nsub == 1:      # the routers' post-processing on the float64 rows
        set_side(monkeypatch, '4')
        d64, q64, _ = route(case, T, nsub)
        want = d64.reshape(T // factor, factor, -1).mean(axis=1).astype(np.float32)
        np.testing.assert_array_equal(got[1][0], want)


@pytest.mark.parametrize('M,T,nsub,f32_in', [(3, 700, 1, False), (2, 120, 12, True)])
def test_ensemble(monkeypatch, M, T, nsub, f32_in):
    """k_rec_in / k_rec_out<..., ENS>: every member's rows in one launch."""
    n = 30_000
    net = synth.synth_network(n, seed=3)
    indptr, indices = csc_from_down(net.down_index)
    c1, c2, c3 = oracle.muskingum_coefficients(net.k, net.x, 3600.0 / nsub)
    c4 = (c1 + c2) / 3600.0
    ql = np.stack([synth.synth_qlateral(n, 0, T, seed=100 + m, dt=3600.0) * 3600.0 for m in range(M)])
    if f32_in:
        ql = ql.astype(np.float32)
    q0 = np.stack([2.0 * synth.u01(50 + m, np.arange(n)) for m in range(M)])
    got = []
    for nb in SIDES:
        set_side(monkeypatch, nb)
        with Plan(indptr, indices) as plan:
            plan.set_coeffs(-c1[indices], c2, c3, c4)
            out = np.empty((M, T, n))
            states = plan.rapid_route_ensemble(q0, ql, out, nsub, factor=1)
            assert plan.last_kernel() == 'tile_ensemble'
            got.append((out, np.asarray(states)))
    assert_same_bits(got[0], got[1], ('discharge', 'final states'))
    q_ref, d_ref = q0[0].copy(), np.zeros((T, n))
    oracle.rapid_route(indptr, indices, -c1[indices], c2, c3, c4, q_ref, ql[0].astype(np.float64), d_ref, nsub)
    assert_close(got[1][0][0], d_ref, 'member 0 discharge')


def test_stream_session_with_a_refilled_lateral_ring_shorter_than_four_batches(monkeypatch):
    """rr_stream_begin / advance / end on records with a 384-row cyclic lateral ring the caller refills 256 rows at a time: the in-pass
    takes what is announced (two batches), the out-pass sends every finished batch out before an advance returns."""
    import torch
    n, T, ring, feed = 60_000, 1000, 384, 256
    case = rapid_case(n, T, 1, seed=43)
    indptr, indices, coeffs, ql, q0 = case
    dev = torch.device('cuda:0')
    got = []
    for nb in SIDES:
        set_side(monkeypatch, nb)
        with Plan(indptr, indices) as plan:
            plan.set_coeffs(*coeffs)
            q = torch.from_numpy(q0.copy()).to(dev)
            lat = torch.zeros((ring, n), dtype=torch.float64, device=dev)
            out = torch.zeros((T, n), dtype=torch.float64, device=dev)
            plan.stream_begin(q, lat, ring, out, T, T, 1, stream=torch.cuda.current_stream().cuda_stream)
            fed = 0
            while fed < T:
                step = min(feed, T - fed)
                lat[torch.arange(fed, fed + step, device=dev) % ring] = torch.from_numpy(ql[fed:fed + step]).to(dev)      # on the call's stream
                fed += step
                plan.stream_advance(fed, fed)
            plan.stream_end(q)
            torch.cuda.synchronize()
            assert plan.last_kernel() == 'tile'
            got.append((out.cpu().numpy(), q.cpu().numpy()))
    assert_same_bits(got[0], got[1], ('discharge', 'final state'))
    q_ref, d_ref = q0.copy(), np.zeros((T, n))
    oracle.rapid_route(indptr, indices, *coeffs, q_ref, ql, d_ref, 1)
    assert_close(got[1][0], d_ref, 'discharge')
    assert_close(got[1][1], q_ref, 'final state')


def test_partitioned_network_with_ghosts_and_exports_on_records(monkeypatch):
    """Eight parts of a cut network through rr_stream_* with their boundary series exchanged in batches, every part on records
    (RR_DIRECT=0): boundary ghosts in, exports out, four batches per launch of the lateral passes -- against the oracle."""
    from test_gpu_tiles import _route_parts_vs_oracle
    set_side(monkeypatch, '4', {'RR_WAVE': '1'})
    specs = _route_parts_vs_oracle(200_000, 8, 700, 64)
    assert sum(s.n_ghost for s in specs) > 50
