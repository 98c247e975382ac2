"""rr.grad.runoff_to_qlateral and rr.grad.RunoffMap on the host: every bad argument raises ValueError or TypeError naming the argument,
on CPU tensors, so the check is made before any device call; the map's transposed (CSC) structure is what scipy builds; and the new
ABI entry points exist and refuse what they must without a GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import river_route_amd as rr
from river_route_amd import _lib, engine

F64 = dict(dtype=torch.float64)
# 4 rivers over 5 grid points: river 1 has no pair, point 3 belongs to no river, point 1 is shared by rivers 0, 2 and 3
INDPTR = np.array([0, 2, 2, 5, 6])
INDICES = np.array([0, 1, 1, 2, 4, 1])
N, P, NNZ, T = 4, 5, 6, 3


def rmap():
    return rr.grad.RunoffMap(INDPTR, INDICES, P)


def args():
    return torch.ones((T, P), **F64), torch.ones(NNZ, **F64), torch.ones(N, **F64)


BAD = [
    ('runoff not a tensor', lambda r, w, a: (np.ones((T, P)), w, a), TypeError, 'runoff'),
    ('runoff int', lambda r, w, a: (r.long(), w, a), TypeError, 'runoff'),
    ('runoff half', lambda r, w, a: (r.half(), w, a), TypeError, 'runoff'),
    ('runoff rank 1', lambda r, w, a: (r[0], w, a), ValueError, 'runoff'),
    ('runoff rank 3', lambda r, w, a: (r[None], w, a), ValueError, 'runoff'),
    ('runoff no rows', lambda r, w, a: (r[:0], w, a), ValueError, 'runoff'),
    ('runoff points', lambda r, w, a: (r[:, :P - 1], w, a), ValueError, 'runoff'),
    ('weights not a tensor', lambda r, w, a: (r, [1.0] * NNZ, a), TypeError, 'weights'),
    ('weights float32', lambda r, w, a: (r, w.float(), a), TypeError, 'weights'),
    ('weights short', lambda r, w, a: (r, w[:-1], a), ValueError, 'weights'),
    ('weights rank 2', lambda r, w, a: (r, w[None], a), ValueError, 'weights'),
    ('area not a tensor', lambda r, w, a: (r, w, np.ones(N)), TypeError, 'area'),
    ('area float32', lambda r, w, a: (r, w, a.float()), TypeError, 'area'),
    ('area length', lambda r, w, a: (r, w, a[:-1]), ValueError, 'area'),
    ('area requires grad', lambda r, w, a: (r, w, a.clone().requires_grad_()), ValueError, 'area'),
]


@pytest.mark.parametrize('what,change,error,match', BAD, ids=[b[0] for b in BAD])
def test_bad_arguments_raise_before_a_device(what, change, error, match):
    r, w, a = change(*args())
    with pytest.raises(error, match=match):
        rr.grad.runoff_to_qlateral(rmap(), r, w, a, cumulative=True)


def test_rmap_must_be_a_runoff_map():
    r, w, a = args()
    with pytest.raises(TypeError, match='rmap'):
        rr.grad.runoff_to_qlateral((INDPTR, INDICES), r, w, a)


def test_good_arguments_reach_the_device_check():
    # CPU tensors are refused last, by name: everything else about them was accepted
    r, w, a = args()
    for kw in ({}, dict(cumulative=True), dict(force_positive=True)):
        with pytest.raises(ValueError, match='runoff must be on cuda:0'):
            rr.grad.runoff_to_qlateral(rmap(), r, w, a, **kw)
        with pytest.raises(ValueError, match='runoff must be on cuda:0'):
            rr.grad.runoff_to_qlateral(rmap(), r.float(), w, None, **kw)
        with pytest.raises(ValueError, match='runoff must be on cuda:0'):
            rr.grad.runoff_to_qlateral(rmap(), r.t().contiguous().t(), w.requires_grad_(), None, **kw)


def test_map_refuses_a_structure_that_does_not_fit():
    with pytest.raises(ValueError, match='n_points'):
        rr.grad.RunoffMap(INDPTR, INDICES, 4)      # the largest index is 4
    with pytest.raises(ValueError, match='n_points'):
        rr.grad.RunoffMap(INDPTR, np.array([0, 1, 1, -1, 4, 1]), P)
    with pytest.raises(ValueError, match='indptr'):
        rr.grad.RunoffMap(INDPTR[:-1], INDICES, P)      # ends before len(indices)
    with pytest.raises(ValueError, match='indptr'):
        rr.grad.RunoffMap(np.array([0, 3, 2, 6]), INDICES, P)
    with pytest.raises(ValueError, match='indices'):
        rr.grad.RunoffMap(INDPTR, INDICES.astype(np.float64), P)
    with pytest.raises(ValueError, match='indptr'):
        rr.grad.RunoffMap(INDPTR[None], INDICES, P)


def check_csc(m):
    assert m.t_indptr.dtype == m.t_pairs.dtype == np.int32
    assert m.t_indptr.shape == (m.n_points + 1,) and m.t_pairs.shape == (m.nnz,)
    assert m.t_indptr[0] == 0 and m.t_indptr[-1] == m.nnz and np.all(np.diff(m.t_indptr) >= 0)
    assert np.array_equal(np.sort(m.t_pairs), np.arange(m.nnz))      # every pair once
    for p in range(m.n_points):
        col = m.t_pairs[m.t_indptr[p]:m.t_indptr[p + 1]]
        assert np.all(np.diff(col) > 0), f'pairs of point {p} not ascending'
        assert np.all(m.indices[col] == p)
    for k in range(m.nnz):
        r = m.pair_river[k]
        assert m.indptr[r] <= k < m.indptr[r + 1]


def test_csc_of_the_small_table():
    m = rmap()
    check_csc(m)
    assert (m.n_rivers, m.n_points, m.nnz) == (N, P, NNZ)
    assert m.t_indptr.tolist() == [0, 1, 4, 5, 5, 6]      # point 3 has an empty column
    assert m.t_pairs.tolist() == [0, 1, 2, 5, 3, 4]
    assert m.pair_river.tolist() == [0, 0, 2, 2, 2, 3]


def test_csc_agrees_with_scipy_on_a_random_table():
    import scipy.sparse
    rng = np.random.default_rng(7)
    n, p = 60, 45
    rows = [np.sort(rng.choice(p - 3, size=rng.integers(0, 7), replace=False)) for _ in range(n)]      # the last 3 points: unused
    indptr = np.concatenate(([0], np.cumsum([len(r) for r in rows])))
    indices = np.concatenate(rows)
    m = rr.grad.RunoffMap(indptr, indices, p)
    check_csc(m)
    assert np.all(np.diff(m.t_indptr)[-3:] == 0)
    # the data of the matrix are the pair indices (from 1: scipy drops nothing), so tocsc() carries them to where each pair lands
    csc = scipy.sparse.csr_matrix((np.arange(1, m.nnz + 1, dtype=np.float64), indices, indptr), shape=(n, p)).tocsc()
    assert np.array_equal(csc.indptr, m.t_indptr)
    assert np.array_equal(csc.data.astype(np.int64) - 1, m.t_pairs)
    assert np.array_equal(csc.indices, m.pair_river[m.t_pairs])


def test_map_from_a_runoff_source():
    src = rr.runoff.RunoffSource(np.zeros((T, P), dtype=np.float32), INDPTR.astype(np.int32), INDICES.astype(np.int32), np.ones(NNZ), np.ones(N),
                                 0, np.arange(T), np.arange(N), False, 0)
    m = rr.grad.RunoffMap.from_source(src)
    assert (m.n_rivers, m.n_points, m.nnz, m.device) == (N, P, NNZ, 0)
    assert np.array_equal(m.indices, INDICES) and m.t_pairs.tolist() == [0, 1, 2, 5, 3, 4]


def test_names_are_exported():
    for name in ('RunoffMap', 'runoff_to_qlateral'):
        assert name in rr.grad.__all__
    for name in ('rr_runoff_adjoint_work_bytes', 'rr_runoff_adjoint_dev'):
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name)


def test_work_bytes():
    assert engine.runoff_adjoint_work_bytes(257, 300, 17) == 257 * 32 * 8      # Gs: n rivers by T rounded up to 16 rows
    assert engine.runoff_adjoint_work_bytes(10, 3, 16) == 10 * 16 * 8
    assert engine.runoff_adjoint_work_bytes(0, 3, 16) == 0
    with pytest.raises(_lib.RRError) as e:
        engine.runoff_adjoint_work_bytes(-1, 3, 16)
    assert e.value.code == _lib.RR_E_INVALID
    assert _lib.lib().rr_runoff_adjoint_work_bytes(1, 1, 1, None) == _lib.RR_E_INVALID


def adjoint_rc(device=0, flags=0, grad_runoff=1, grad_weights=1, indptr=1, t_pairs=1, n=N, stride_t=P):
    # addresses are never followed: every refusal here is made before a device is looked for, and the last one is the device's
    L = _lib.lib()
    return L.rr_runoff_adjoint_dev(device, n, P, T, 64 * indptr, 64, 64, 64, 64 * t_pairs, 64, 0, stride_t, 1, None, flags, 64, 64 * grad_runoff or None,
                                   P, 64 * grad_weights or None, 64, 1 << 20, None)


def test_abi_refuses_bad_input_without_a_gpu():
    assert adjoint_rc(flags=engine.RUNOFF_KEEP_NAN) == _lib.RR_E_INVALID
    assert b'KEEP_NAN' in _lib.lib().rr_last_error()
    assert adjoint_rc(flags=engine.RUNOFF_KEEP_NAN | engine.RUNOFF_CUMULATIVE) == _lib.RR_E_INVALID
    assert adjoint_rc(grad_runoff=0, grad_weights=0) == _lib.RR_E_INVALID
    assert adjoint_rc(indptr=0) == _lib.RR_E_INVALID
    assert adjoint_rc(t_pairs=0) == _lib.RR_E_INVALID
    assert adjoint_rc(n=-1) == _lib.RR_E_INVALID
    assert adjoint_rc(stride_t=-1) == _lib.RR_E_INVALID
    assert adjoint_rc(device=-1) == _lib.RR_E_NO_DEVICE
    assert adjoint_rc(device=_lib.device_count()) == _lib.RR_E_NO_DEVICE      # one past the last device; 0 where there is none
    with pytest.raises(_lib.RRError) as e:
        engine.runoff_adjoint_dev(N, P, T, 64, 64, 64, 64, 64, 64, False, P, 1, None, engine.RUNOFF_KEEP_NAN, 64, 64, P, None, 64, 1 << 20)
    assert e.value.code == _lib.RR_E_INVALID
