"""rr.grad.runoff_to_qlateral on the GPU: the gradients of the gridded-runoff inflow against a numpy restatement
written out in plain loops (the arbiter) and, on NaN-free data, against torch autograd through a dense restatement.

One fixture family throughout: 257 rivers (one past a 256-lane block) over 300 grid points; river 0 has an empty row, river 1 exactly
one point, river 2 only the dry point (runoff 0 at every step, so its value is exactly 0 under the clip), rivers 10 .. 49 share point 7
(a transposed column of 40 pairs and more), and point 299 belongs to no river."""
import functools
import math

import numpy as np
import pytest
import torch

import river_route_amd as rr
import test_grad as route_cpu
import test_grad_scores as scores_cpu
from conftest import assert_close
from river_route_amd import _lib, engine
from test_gpu_grad import DEV, _default_knobs, assert_grad, make_plan  # noqa: F401  (the fixture resets the engine's knobs)

pytestmark = pytest.mark.gpu
N, P = 257, 300
DRY, SHARED, UNUSED = 5, 7, 299
FLAGS = [(False, False), (False, True), (True, False), (True, True)]      # (cumulative, force_positive)
FLAG_IDS = ['plain', 'clip', 'cumulative', 'cumulative-clip']


@functools.lru_cache(maxsize=None)
def table():
    rng = np.random.default_rng(11)
    rows = []
    for r in range(N):
        if r == 0:
            pts = []
        elif r == 1:
            pts = [123]
        elif r == 2:
            pts = [DRY]
        else:
            pts = set(rng.choice(P - 1, size=rng.integers(1, 6), replace=False).tolist()) - {DRY}      # never point 299
            if 10 <= r < 50:
                pts.add(SHARED)
            pts = sorted(pts) or [r % 100 + 20]
        rows.append(pts)
    indptr = np.concatenate(([0], np.cumsum([len(p) for p in rows]))).astype(np.int32)
    indices = np.concatenate([np.asarray(p, dtype=np.int32) for p in rows])
    assert np.count_nonzero(indices == SHARED) >= 40 and not np.any(indices == UNUSED)
    weights = rng.uniform(0.1, 1.0, indices.shape[0])
    area = rng.uniform(0.5, 2.0, N)
    return indptr, indices, weights, area, rr.grad.RunoffMap(indptr, indices, P)


@functools.lru_cache(maxsize=None)
def data(T, nan=False):
    """(runoff[T, P], G[T, N]): signed, so the clip is active with and without the cumulative difference; the dry point is 0."""
    rng = np.random.default_rng(100 + T)
    R, G = rng.standard_normal((T, P)), rng.standard_normal((T, N))
    R[:, DRY] = 0.0
    if nan:
        R[5, SHARED] = np.nan      # mid-chunk, in the long column
        R[15, 123] = np.nan        # a chunk's last row, river 1's only point
    R.setflags(write=False), G.setflags(write=False)
    return R, G


def restate(indptr, indices, w, R, area, G, cumulative, force_positive):
    """The arbiter: forward and adjoint of DESIGN.md section 12h in plain float64 loops.  (qlateral, grad_runoff, grad_weights)."""
    T, n_points = R.shape
    n = len(indptr) - 1
    S, q = np.zeros((T, n)), np.zeros((T, n))
    Gb, Gs = np.zeros((T, n)), np.zeros((T, n))
    river = np.zeros(len(indices), dtype=np.int64)
    for r in range(n):
        for k in range(indptr[r], indptr[r + 1]):
            river[k] = r
            for t in range(T):
                S[t, r] = S[t, r] + w[k] * R[t, indices[k]]
    for r in range(n):
        a = 1.0 if area is None else area[r]
        for t in range(T):
            v = S[t, r] - S[t - 1, r] if cumulative and t > 0 else S[t, r]
            passes = not math.isnan(v) and (not force_positive or v >= 0.0)
            if force_positive and v < 0.0:
                v = 0.0
            if math.isnan(v):
                v = 0.0
            q[t, r] = v * a if area is not None else v
            Gb[t, r] = G[t, r] * a if passes else 0.0
        for t in range(T):
            Gs[t, r] = Gb[t, r] - Gb[t + 1, r] if cumulative and t + 1 < T else Gb[t, r]
    gR, gW = np.zeros((T, n_points)), np.zeros(len(indices))
    for k in range(len(indices)):
        r, p, acc = river[k], indices[k], 0.0
        for t in range(T):
            if Gs[t, r] != 0.0:
                gR[t, p] = gR[t, p] + w[k] * Gs[t, r]
                acc = acc + Gs[t, r] * R[t, p]
        gW[k] = acc
    return q, gR, gW


@functools.lru_cache(maxsize=None)
def arbiter(T, cumulative, force_positive, nan=False, f32=False):
    indptr, indices, w, area, _ = table()
    R, G = data(T, nan)
    if f32:
        R = R.astype(np.float32).astype(np.float64)
    return restate(indptr, indices, w, R, area, G, cumulative, force_positive)


def torch_grads(indptr, indices, w, R, area, G, cumulative, force_positive):
    """The second arbiter (NaN-free data): autograd through index_add of R[:, cols] * w, cat / diff, clamp(min=0), * area."""
    n = len(indptr) - 1
    river = torch.as_tensor(np.repeat(np.arange(n), np.diff(indptr)))
    Rt, wt = torch.tensor(R, requires_grad=True), torch.tensor(w, requires_grad=True)
    S = torch.zeros((R.shape[0], n), dtype=torch.float64).index_add(1, river, Rt[:, torch.as_tensor(indices.astype(np.int64))] * wt)
    V = torch.cat([S[:1], S[1:] - S[:-1]]) if cumulative else S
    if force_positive:
        V = V.clamp(min=0)
    q = V * torch.as_tensor(area) if area is not None else V
    (q * torch.tensor(G)).sum().backward()
    return q.detach().numpy(), Rt.grad.numpy(), wt.grad.numpy()


def on_gpu(a, dtype=None):
    return torch.tensor(np.asarray(a), device=DEV, dtype=dtype)


def gpu_grads(R, G, cumulative, force_positive, *, area=True, want=(True, True), rmap=None, layout=None, dtype=torch.float64,
              tab=None):
    """(qlateral, runoff.grad, weights.grad) as numpy arrays (None where not asked).  layout: a function that lays the (T, P) device
    tensor out differently without changing its values."""
    indptr, indices, w, a, m = tab or table()
    Rt = on_gpu(R, dtype)
    if layout is not None:
        Rt = layout(Rt)
    Rt = Rt.detach().requires_grad_(want[0])
    wt = on_gpu(w).requires_grad_(want[1])
    at = on_gpu(a) if area is True else area
    q = rr.grad.runoff_to_qlateral(rmap or m, Rt, wt, at, cumulative=cumulative, force_positive=force_positive)
    (q * on_gpu(G)).sum().backward()
    host = lambda t: None if t is None else t.detach().cpu().numpy()
    return host(q), host(Rt.grad), host(wt.grad)


# ---- 1, 2. chunk edges against both arbiters ----

@pytest.mark.parametrize('cumulative,force_positive', FLAGS, ids=FLAG_IDS)
@pytest.mark.parametrize('T', [1, 15, 16, 17, 33])
def test_gradients_match_the_arbiter(T, cumulative, force_positive):
    R, G = data(T)
    want_q, want_r, want_w = arbiter(T, cumulative, force_positive)
    q, gr, gw = gpu_grads(R, G, cumulative, force_positive)
    if force_positive:
        assert (want_q == 0).any() and (want_q > 0).any()      # the clip is active
    assert np.abs(want_r).max() > 0 and np.abs(want_w).max() > 0
    assert_close(q, want_q, 'qlateral')
    assert_close(gr, want_r, 'grad_runoff')
    assert_close(gw, want_w, 'grad_weights')


def test_more_rows_than_one_block_of_the_point_pass_walks():
    # a block of the point pass walks 8 chunks (128 rows): 130 rows need a second one, which starts at row 128
    T = 130
    R, G = data(T)
    want_q, want_r, want_w = arbiter(T, True, True)
    q, gr, gw = gpu_grads(R, G, True, True)
    assert_close(q, want_q, 'qlateral')
    assert_close(gr, want_r, 'grad_runoff')
    assert_close(gw, want_w, 'grad_weights')
    assert np.abs(want_r[128:]).max() > 0


@pytest.mark.parametrize('cumulative,force_positive', FLAGS, ids=FLAG_IDS)
@pytest.mark.parametrize('T', [1, 15, 16, 17, 33])
def test_gradients_match_torch_autograd(T, cumulative, force_positive):
    indptr, indices, w, area, _ = table()
    R, G = data(T)
    want_q, want_r, want_w = torch_grads(indptr, indices, w, R, area, G, cumulative, force_positive)
    q, gr, gw = gpu_grads(R, G, cumulative, force_positive)
    assert_close(q, want_q, 'qlateral')
    assert_close(gr, want_r, 'grad_runoff')
    assert_close(gw, want_w, 'grad_weights')


# ---- 3. NaN in the runoff ----

@pytest.mark.parametrize('cumulative', [False, True], ids=['plain', 'cumulative'])
def test_nan_in_the_runoff_poisons_nothing(cumulative):
    T = 33
    indptr, indices, w, area, _ = table()
    R, G = data(T, nan=True)
    assert np.isnan(R).sum() == 2
    want_q, want_r, want_w = arbiter(T, cumulative, True, nan=True)
    q, gr, gw = gpu_grads(R, G, cumulative, True)
    assert np.isfinite(gr).all() and np.isfinite(gw).all() and np.isfinite(q).all()
    assert_close(gr, want_r, 'grad_runoff')
    assert_close(gw, want_w, 'grad_weights')
    flags = engine.RUNOFF_FORCE_POSITIVE | (engine.RUNOFF_CUMULATIVE if cumulative else 0)
    assert np.array_equal(q, engine.runoff_to_qlateral(indptr, indices, w, R, area, flags))


# ---- 4. unused point, empty river ----

def test_unused_point_is_written_zero_and_empty_river_counts_for_nothing():
    T = 17
    indptr, indices, w, area, m = table()
    R, G = data(T)
    wt, at, Rt = on_gpu(w), on_gpu(area), on_gpu(R)
    pointers = m.device_pointers()
    nbytes = engine.runoff_adjoint_work_bytes(N, P, T)
    work = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    out = []
    for g in (G, np.concatenate((np.full((T, 1), 1e30), G[:, 1:]), axis=1)):      # the second: another cotangent for the empty river
        gr = torch.full((T, P), float('nan'), dtype=torch.float64, device=DEV)
        gw = torch.full((m.nnz,), float('nan'), dtype=torch.float64, device=DEV)
        engine.runoff_adjoint_dev(N, P, T, pointers[0], pointers[1], wt, pointers[2], pointers[3], Rt, False, P, 1, at,
                                  engine.RUNOFF_CUMULATIVE | engine.RUNOFF_FORCE_POSITIVE, on_gpu(g), gr, P, gw, work, nbytes,
                                  stream=torch.cuda.current_stream(0).cuda_stream)
        out.append((gr.cpu().numpy(), gw.cpu().numpy()))
    (gr, gw), (gr2, gw2) = out
    assert np.isfinite(gr).all() and np.isfinite(gw).all()
    assert np.all(gr[:, UNUSED] == 0.0) and not np.signbit(gr[:, UNUSED]).any()
    _, want_r, want_w = arbiter(T, True, True)
    assert_close(gr, want_r, 'grad_runoff')
    assert_close(gw, want_w, 'grad_weights')
    assert np.array_equal(gr, gr2) and np.array_equal(gw, gw2)


# ---- 5. float32 runoff ----

@pytest.mark.parametrize('cumulative,force_positive', [(False, False), (True, True)], ids=['plain', 'cumulative-clip'])
def test_float32_runoff(cumulative, force_positive):
    T = 33
    R, G = data(T)
    _, want_r, want_w = arbiter(T, cumulative, force_positive, f32=True)
    _, gr, gw = gpu_grads(R, G, cumulative, force_positive, dtype=torch.float32)
    assert gr.dtype == np.float32 and gw.dtype == np.float64
    np.testing.assert_allclose(gr, want_r.astype(np.float32), rtol=2.0 ** -23, atol=0.0, err_msg='grad_runoff (float32)')
    assert_close(gw, want_w, 'grad_weights')


# ---- 6. strides ----

def column_slice(R):
    wide = torch.zeros((R.shape[0], R.shape[1] + 7), dtype=R.dtype, device=R.device)
    wide[:, 3:3 + R.shape[1]] = R
    return wide[:, 3:3 + R.shape[1]]


def point_major(R):
    return R.t().contiguous().t()      # stride_t = 1, stride_p = T


def point_major_padded(R):
    """Rows of a multiple of 16 elements, allocated in full: the layout the kernels read as 16-byte vectors."""
    T = R.shape[0]
    block = torch.zeros((R.shape[1], -(-T // 16) * 16), dtype=R.dtype, device=R.device)
    block[:, :T] = R.t()
    return block[:, :T].t()


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32], ids=['f64', 'f32'])
@pytest.mark.parametrize('cumulative', [False, True], ids=['plain', 'cumulative'])
@pytest.mark.parametrize('T', [17, 33])
def test_layouts_give_the_same_bits(T, cumulative, dtype):
    R, G = data(T)
    base = gpu_grads(R, G, cumulative, True, dtype=dtype)
    assert np.abs(base[1]).max() > 0
    for layout in (column_slice, point_major, point_major_padded):
        got = gpu_grads(R, G, cumulative, True, dtype=dtype, layout=layout)
        for a, b, name in zip(got, base, ('qlateral', 'grad_runoff', 'grad_weights')):
            assert np.array_equal(a, b), f'{layout.__name__}: {name}'


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32], ids=['f64', 'f32'])
def test_direct_call_on_unpadded_rows_gives_the_same_bits(dtype):
    # rr.grad copies such rows into the vector layout, so only a direct call reaches the kernels' row-by-row path
    T = 33
    indptr, indices, w, area, m = table()
    R, G = data(T, nan=True)
    _, want_r, want_w = gpu_grads(R, G, True, True, dtype=dtype)
    pointers = m.device_pointers()
    nbytes = engine.runoff_adjoint_work_bytes(N, P, T)
    work = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    wt, at, Gt = on_gpu(w), on_gpu(area), on_gpu(G)
    for Rt in (on_gpu(R, dtype), point_major(on_gpu(R, dtype))):      # as read from a file; point-major with rows of 33 elements
        gr = torch.full((T, P), float('nan'), dtype=dtype, device=DEV)
        gw = torch.full((m.nnz,), float('nan'), dtype=torch.float64, device=DEV)
        engine.runoff_adjoint_dev(N, P, T, pointers[0], pointers[1], wt, pointers[2], pointers[3], Rt.data_ptr(), dtype == torch.float32, Rt.stride(0),
                                  Rt.stride(1), at, engine.RUNOFF_CUMULATIVE | engine.RUNOFF_FORCE_POSITIVE, Gt, gr, P, gw, work, nbytes,
                                  stream=torch.cuda.current_stream(0).cuda_stream)
        assert np.array_equal(gr.cpu().numpy(), want_r) and np.array_equal(gw.cpu().numpy(), want_w)


def test_layouts_with_nan_match_the_arbiter():
    # the vector path's own handling of the row before and the row after a chunk, with the mask in play
    T = 33
    R, G = data(T, nan=True)
    _, want_r, want_w = arbiter(T, True, True, nan=True)
    _, gr, gw = gpu_grads(R, G, True, True, layout=point_major_padded)
    assert_close(gr, want_r, 'grad_runoff')
    assert_close(gw, want_w, 'grad_weights')


# ---- 7. determinism ----

def test_two_backward_passes_bit_identical():
    R, G = data(33)
    a, b = gpu_grads(R, G, True, True), gpu_grads(R, G, True, True)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


# ---- 8. only what is asked ----

def test_only_what_is_asked_and_area_none():
    R, G = data(17)
    both = gpu_grads(R, G, True, True)
    _, gr, gw = gpu_grads(R, G, True, True, want=(True, False))
    assert gw is None and np.array_equal(gr, both[1])
    _, gr, gw = gpu_grads(R, G, True, True, want=(False, True))
    assert gr is None and np.array_equal(gw, both[2])
    none = gpu_grads(R, G, True, True, area=None)
    ones = gpu_grads(R, G, True, True, area=torch.ones(N, dtype=torch.float64, device=DEV))
    for x, y in zip(none, ones):
        assert np.array_equal(x, y)
    assert not np.array_equal(none[1], both[1])


# ---- 9. forward parity ----

@pytest.mark.parametrize('dtype', [np.float64, np.float32], ids=['f64', 'f32'])
@pytest.mark.parametrize('cumulative,force_positive', FLAGS, ids=FLAG_IDS)
def test_forward_bit_equal_to_engine(cumulative, force_positive, dtype):
    T = 33
    indptr, indices, w, area, m = table()
    R = data(T)[0].astype(dtype)
    flags = (engine.RUNOFF_CUMULATIVE if cumulative else 0) | (engine.RUNOFF_FORCE_POSITIVE if force_positive else 0)
    for a in (area, None):
        want = engine.runoff_to_qlateral(indptr, indices, w, R, a, flags)
        got = rr.grad.runoff_to_qlateral(m, on_gpu(R), on_gpu(w), None if a is None else on_gpu(a), cumulative=cumulative,
                                         force_positive=force_positive)
        assert got.dtype == torch.float64 and np.array_equal(got.cpu().numpy(), want)


# ---- 10. gradcheck ----

@pytest.mark.parametrize('cumulative', [False, True], ids=['plain', 'cumulative'])
def test_gradcheck(cumulative):
    indptr, indices = np.array([0, 2, 2, 5, 6]), np.array([0, 1, 1, 2, 4, 1])      # T = 3, n = 4, P = 5
    m = rr.grad.RunoffMap(indptr, indices, 5)
    rng = np.random.default_rng(3)
    R = on_gpu(rng.standard_normal((3, 5))).requires_grad_()
    w = on_gpu(rng.uniform(0.1, 1.0, 6)).requires_grad_()
    area = on_gpu(rng.uniform(0.5, 2.0, 4))
    assert torch.autograd.gradcheck(lambda r, ww: rr.grad.runoff_to_qlateral(m, r, ww, area, cumulative=cumulative), (R, w))


# ---- 11. the chain: runoff -> inflow -> routing at gauges -> KGE ----

def test_chain_to_a_score_at_gauges():
    n, T, nsub, n_points, dt_runoff = 60, 24, 2, 40, 3600.0
    down, k, x = route_cpu.network('forest', n, seed=8)
    rng = np.random.default_rng(21)
    rows = [np.sort(rng.choice(n_points, size=rng.integers(1, 4), replace=False)) for _ in range(n)]
    indptr = np.concatenate(([0], np.cumsum([len(r) for r in rows])))
    indices = np.concatenate(rows)
    w = rng.uniform(0.2, 1.0, indices.shape[0])
    area = rng.uniform(1000.0, 5000.0, n)
    R = np.cumsum(rng.uniform(-0.2, 1.0, (T, n_points)), axis=0)      # cumulative input whose increments are sometimes negative
    q0 = rng.uniform(0.0, 3.0, n)
    gauges = np.array([59, 3, 31, 17, 44])
    obs = rng.uniform(0.5, 3.0, (T, gauges.shape[0]))
    river = torch.as_tensor(np.repeat(np.arange(n), np.diff(indptr)))

    # dense restatements of the three stages on the CPU
    Rt, wt = torch.tensor(R, requires_grad=True), torch.tensor(w, requires_grad=True)
    S = torch.zeros((T, n), dtype=torch.float64).index_add(1, river, Rt[:, torch.as_tensor(indices)] * wt)
    ql = torch.cat([S[:1], S[1:] - S[:-1]]).clamp(min=0) * torch.as_tensor(area)
    assert bool((ql == 0).any())      # the clip is active
    c1, c2, c3 = rr.grad.muskingum_coefficients(torch.tensor(k), torch.tensor(x), dt_runoff / nsub)
    d, _ = route_cpu.dense_route(down, torch.tensor(q0), ql, c1, c2, c3, (c1 + c2) / dt_runoff, nsub)
    want_kge = scores_cpu.dense_scores(torch.tensor(obs), d[:, torch.as_tensor(gauges)])['kge2012']
    want_kge.sum().backward()

    m = rr.grad.RunoffMap(indptr, indices, n_points)
    Rg, wg = on_gpu(R).requires_grad_(), on_gpu(w).requires_grad_()
    qlg = rr.grad.runoff_to_qlateral(m, Rg, wg, on_gpu(area), cumulative=True, force_positive=True)
    dg, _ = rr.grad.rapid_route(make_plan(down), on_gpu(q0), qlg, torch.tensor(k), torch.tensor(x), dt_runoff / nsub, dt_runoff, gauges=gauges)
    kge = rr.grad.scores(on_gpu(obs), dg)['kge2012']
    kge.sum().backward()
    assert bool(torch.isfinite(kge).all())
    assert_grad(kge.detach().cpu().numpy(), want_kge.detach().numpy(), 'kge2012')
    assert np.abs(Rt.grad.numpy()).max() > 0 and np.abs(wt.grad.numpy()).max() > 0
    assert_grad(Rg.grad.cpu().numpy(), Rt.grad.numpy(), 'dL/drunoff')
    assert_grad(wg.grad.cpu().numpy(), wt.grad.numpy(), 'dL/dweights')


# ---- 12. a non-default stream ----

def test_non_default_stream():
    T = 33
    indptr, indices, w, area, m = table()
    R, G = data(T)
    want = gpu_grads(R, G, True, True)
    Rt, wt = on_gpu(R).requires_grad_(), on_gpu(w).requires_grad_()
    at, Gt = on_gpu(area), on_gpu(G)
    s = torch.cuda.Stream(device=DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):
        q = rr.grad.runoff_to_qlateral(m, Rt, wt, at, cumulative=True, force_positive=True)
        (q * Gt).sum().backward()
    torch.cuda.synchronize(DEV)
    for got, w_ in zip((q.detach(), Rt.grad, wt.grad), want):
        assert np.array_equal(got.cpu().numpy(), w_)


# ---- the ABI's refusals that need a device ----

def test_work_memory_too_small_is_refused_with_the_byte_count():
    T = 17
    indptr, indices, w, area, m = table()
    pointers = m.device_pointers()
    nbytes = engine.runoff_adjoint_work_bytes(N, P, T)
    work = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    gr = torch.empty((T, P), dtype=torch.float64, device=DEV)
    args = (N, P, T, pointers[0], pointers[1], on_gpu(w), pointers[2], pointers[3], on_gpu(data(T)[0]), False, P, 1, None, 0, on_gpu(data(T)[1]), gr, P,
            None, work)
    with pytest.raises(_lib.RRError) as e:
        engine.runoff_adjoint_dev(*args, nbytes - 1)
    assert e.value.code == _lib.RR_E_STATE and str(nbytes) in e.value.message
    with pytest.raises(_lib.RRError) as e:
        engine.runoff_adjoint_dev(*args[:13], engine.RUNOFF_KEEP_NAN, *args[14:], nbytes)
    assert e.value.code == _lib.RR_E_INVALID
    with pytest.raises(ValueError, match='runoff must be on cuda:0'):
        rr.grad.runoff_to_qlateral(m, torch.tensor(data(T)[0]), on_gpu(w))
    with pytest.raises(ValueError, match='weights must be on cuda:0'):
        rr.grad.runoff_to_qlateral(m, on_gpu(data(T)[0]), torch.tensor(w))
