"""
ctypes front-end of the CPU oracle (oracle/rr_oracle.c) and of its long-double restatement, the per-reach arbiter
(oracle/rr_oracle_ld.c: the *_ld functions), the adjoint arbiter (oracle/rr_oracle_adj.c) and the arbiter of the skill scores and their
gradient (oracle/rr_oracle_scores.c: scores_ld, scores_grad_ld).

TEST INFRASTRUCTURE ONLY: imported by tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg.
Nothing under river_route_amd/ may import this module.

Parity: every function here is pinned to outputs of the reference itself (tests/golden/*.npz; tests/test_oracle.py,
tests/test_runoff.py).

The function signatures mirror the reference call sites so a parity test reads like the reference:
river_route/routers/_numba_kernels.py:9-14, 50-55, 89-99; uhkernels/UnitHydrograph.py:64-107;
routers/Muskingum.py:172-193; tools.py:75-109.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_i32p = np.ctypeslib.ndpointer(np.int32, flags='C_CONTIGUOUS')
_i64p = np.ctypeslib.ndpointer(np.int64, flags='C_CONTIGUOUS')
_f64p = np.ctypeslib.ndpointer(np.float64, flags='C_CONTIGUOUS')
_i64 = C.c_int64

_ERRORS = {
    -1: MemoryError('oracle: allocation failed'),
    -2: ValueError('Muskingum coefficients do not sum to 1, check routing parameters and time step'),
    -3: ValueError('Unknown downstream_river_id'),
    -4: ValueError('params_file must be topologically sorted upstream to downstream'),
}


def build(fast: bool = False, out_dir: str | None = None) -> str:
    """Compile the oracle with gcc if its shared object is missing or stale; returns the .so path."""
    name = 'librr_oracle_fast.so' if fast else 'librr_oracle.so'
    # the parity checker holds the extended-precision arbiters too (rr_oracle_ld.c, rr_oracle_adj.c, rr_oracle_scores.c); the timed
    # baseline is the fp64 loops alone
    srcs = [os.path.join(_HERE, f) for f in (('rr_oracle.c',) if fast else ('rr_oracle.c', 'rr_oracle_ld.c', 'rr_oracle_adj.c',
                                                                            'rr_oracle_scores.c'))]
    out = os.path.join(out_dir or _HERE, name)
    if os.path.exists(out) and os.path.getmtime(out) >= max(os.path.getmtime(src) for src in srcs):
        return out
    flags = ['-O3', '-march=native', '-ffast-math'] if fast else ['-O2', '-fno-fast-math', '-ffp-contract=off']
    subprocess.check_call(['gcc', '-std=c11', *flags, '-fPIC', '-shared', '-o', out, *srcs, '-lm'])
    return out


def _bind(lib: C.CDLL) -> C.CDLL:
    lib.orc_muskingum_route.argtypes = [_i64, _i32p, _i32p, _f64p, _f64p, _f64p, _f64p, _f64p, _i64, _i64]
    lib.orc_rapid_route.argtypes = [_i64, _i32p, _i32p, _f64p, _f64p, _f64p, _f64p, _f64p, _f64p, _f64p, _i64, _i64]
    lib.orc_unit_route.argtypes = [_i64, _i64, _i64, _i32p, _i32p, _f64p, _i32p, _i32p, _f64p, _i32p, _i32p, _f64p,
                                   _f64p, _f64p, _f64p, _i64p, _i64p, _f64p, _f64p, _f64p, _f64p, _i64, _i64]
    lib.orc_muskingum_coefficients.argtypes = [_i64, _f64p, _f64p, C.c_double, _f64p, _f64p, _f64p]
    lib.orc_adjacency_matrix.argtypes = [_i64, _i64p, _i64p, _i32p, _i32p]
    lib.orc_uh_convolve_incrementally.argtypes = [_i64, _i64, _f64p, _f64p, _f64p, _f64p]
    lib.orc_uh_convolve_incrementally.restype = None
    lib.orc_uh_convolve.argtypes = [_i64, _i64, _i64, _f64p, _f64p, _f64p, _f64p]
    for f in ('orc_muskingum_route', 'orc_rapid_route', 'orc_unit_route', 'orc_muskingum_coefficients',
              'orc_adjacency_matrix', 'orc_uh_convolve'):
        getattr(lib, f).restype = C.c_int
    if hasattr(lib, 'orcl_rapid_route'):      # the arbiter (rr_oracle_ld.c): in the parity checker only
        lib.orcl_muskingum_route.argtypes = [_i64, _i32p, _i32p, _f64p, _f64p, _f64p, _f64p, _f64p, _f64p, _i64, _i64]
        lib.orcl_rapid_route.argtypes = [_i64, _i32p, _i32p, _f64p, _f64p, _f64p, _f64p, _f64p, _f64p, _f64p, _f64p, _i64, _i64]
        lib.orcl_unit_route.argtypes = [_i64, _i64, _i64, _i32p, _i32p, _f64p, _i32p, _i32p, _f64p, _i32p, _i32p, _f64p,
                                        _f64p, _f64p, _f64p, _i64p, _i64p, _f64p, _f64p, _f64p, _f64p, _f64p, _i64, _i64]
        lib.orcl_uh_convolve.argtypes = [_i64, _i64, _i64, _f64p, _f64p, _f64p, _f64p]
        for f in ('orcl_muskingum_route', 'orcl_rapid_route', 'orcl_unit_route', 'orcl_uh_convolve'):
            getattr(lib, f).restype = C.c_int
    if hasattr(lib, 'orcl_rapid_adjoint'):    # the adjoint arbiter (rr_oracle_adj.c): in the parity checker only
        _bind_adjoint(lib)
    if hasattr(lib, 'orcl_scores'):           # the scores arbiter (rr_oracle_scores.c): in the parity checker only
        o = C.c_void_p
        lib.orcl_scores.argtypes = [_i64, _i64, _f64p, _f64p, _i64, o, C.c_int, _f64p]
        lib.orcl_scores_grad.argtypes = [_i64, _i64, _f64p, _f64p, _i64, o, C.c_int, _f64p, _f64p, _f64p, _f64p]
        lib.orcl_scores.restype = lib.orcl_scores_grad.restype = C.c_int
    return lib


def _bind_adjoint(lib: C.CDLL) -> C.CDLL:
    o = C.c_void_p      # optional arrays: NULL or the address of a float64 array
    for f in ('orc_rapid_adjoint', 'orcl_rapid_adjoint'):
        getattr(lib, f).argtypes = [_i64, _i32p, _i32p, _f64p, _f64p, _f64p, _f64p, _f64p, o, o, o, _i64, _i64,
                                    _f64p, _f64p, o, _f64p, _f64p, o, _f64p]
        getattr(lib, f).restype = C.c_int
    for f in ('orc_unit_adjoint', 'orcl_unit_adjoint'):
        getattr(lib, f).argtypes = [_i64, _i32p, _i32p, _f64p, _f64p, _f64p, _f64p, _f64p, _f64p, o, o, o, _i64, _i64,
                                    _f64p, _f64p, _f64p, _f64p, _f64p, _f64p, _f64p, _f64p]
        getattr(lib, f).restype = C.c_int
    return lib


def build_adjoint_reordered(out_dir: str) -> C.CDLL:
    """rr_oracle_adj.c alone, its fp64 loops summing the terms of every recursion and the tributaries of every reach in the reverse
    order, with fused multiply-adds: a second correctly rounded evaluation, for measuring what a change of order costs (the K of
    tests/per_reach.assert_per_element).  Built into `out_dir`, never beside the sources."""
    out = os.path.join(out_dir, 'librr_oracle_adj_reordered.so')
    subprocess.check_call(['gcc', '-std=c11', '-O2', '-march=native', '-fno-fast-math', '-ffp-contract=fast', '-DORC_ADJ_REORDER',
                           '-fPIC', '-shared', '-o', out, os.path.join(_HERE, 'rr_oracle_adj.c'), '-lm'])
    return _bind_adjoint(C.CDLL(out))


_LIBS: dict[str, C.CDLL] = {}


def lib(fast: bool = False, out_dir: str | None = None) -> C.CDLL:
    path = build(fast, out_dir)
    if path not in _LIBS:
        _LIBS[path] = _bind(C.CDLL(path))
    return _LIBS[path]


def _check(rc: int) -> None:
    if rc != 0:
        raise _ERRORS.get(rc, RuntimeError(f'oracle error {rc}'))


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


# ---- the three routing kernels, argument-for-argument as in _numba_kernels.py (mutating in place) ----

def muskingum_route(csc_indptr, csc_indices, lhs_off_data, c2, c3, q_t, discharge_array,
                    num_output_steps, num_routing_per_output, *, fast=False, out_dir=None):
    n = q_t.shape[0]
    assert discharge_array.shape == (num_output_steps, n)
    _check(lib(fast, out_dir).orc_muskingum_route(n, _i32(csc_indptr), _i32(csc_indices), _f64(lhs_off_data),
                                                  _f64(c2), _f64(c3), q_t, discharge_array,
                                                  num_output_steps, num_routing_per_output))


def rapid_route(csc_indptr, csc_indices, lhs_off_data, c2, c3, c4_dt, q_t, qlateral, discharge_array,
                num_substeps, *, fast=False, out_dir=None):
    n = q_t.shape[0]
    T = qlateral.shape[0]
    assert qlateral.shape == (T, n) and discharge_array.shape == (T, n)
    _check(lib(fast, out_dir).orc_rapid_route(n, _i32(csc_indptr), _i32(csc_indices), _f64(lhs_off_data),
                                              _f64(c2), _f64(c3), _f64(c4_dt), q_t, _f64(qlateral),
                                              discharge_array, T, num_substeps))


def unit_route(lhs_indptr, lhs_indices, lhs_off_data, a_inner_indptr, a_inner_indices, a_inner_data,
               a_hw_indptr, a_hw_indices, a_hw_data, c1_inner, c2_inner, c3_inner, hw_idx, inner_idx,
               q_ch, q_full, convolved_lateral, discharge_array, num_substeps, *, fast=False, out_dir=None):
    n_in, n_hw = len(inner_idx), len(hw_idx)
    T, n_total = convolved_lateral.shape
    assert discharge_array.shape == (T, n_total)
    _check(lib(fast, out_dir).orc_unit_route(
        n_in, n_hw, n_total, _i32(lhs_indptr), _i32(lhs_indices), _f64(lhs_off_data),
        _i32(a_inner_indptr), _i32(a_inner_indices), _f64(a_inner_data),
        _i32(a_hw_indptr), _i32(a_hw_indices), _f64(a_hw_data),
        _f64(c1_inner), _f64(c2_inner), _f64(c3_inner),
        np.ascontiguousarray(hw_idx, dtype=np.int64), np.ascontiguousarray(inner_idx, dtype=np.int64),
        q_ch, q_full, _f64(convolved_lateral), discharge_array, T, num_substeps))


# ---- the extended-precision arbiter (rr_oracle_ld.c): the same loops in long double ----
# Arguments as the fp64 functions above, plus `raw_array` (the shape of discharge_array) for the UNCLAMPED interval means.  The state
# arrays are updated in place to the final state, rounded to double once.  tests/per_reach.py holds the comparison built on these.

def muskingum_route_ld(csc_indptr, csc_indices, lhs_off_data, c2, c3, q_t, discharge_array, raw_array,
                       num_output_steps, num_routing_per_output):
    n = q_t.shape[0]
    assert discharge_array.shape == raw_array.shape == (num_output_steps, n)
    _check(lib().orcl_muskingum_route(n, _i32(csc_indptr), _i32(csc_indices), _f64(lhs_off_data), _f64(c2), _f64(c3),
                                      q_t, discharge_array, raw_array, num_output_steps, num_routing_per_output))


def rapid_route_ld(csc_indptr, csc_indices, lhs_off_data, c2, c3, c4_dt, q_t, qlateral, discharge_array, raw_array,
                   num_substeps):
    n = q_t.shape[0]
    T = qlateral.shape[0]
    assert qlateral.shape == (T, n) and discharge_array.shape == raw_array.shape == (T, n)
    _check(lib().orcl_rapid_route(n, _i32(csc_indptr), _i32(csc_indices), _f64(lhs_off_data), _f64(c2), _f64(c3),
                                  _f64(c4_dt), q_t, _f64(qlateral), discharge_array, raw_array, T, num_substeps))


def unit_route_ld(lhs_indptr, lhs_indices, lhs_off_data, a_inner_indptr, a_inner_indices, a_inner_data,
                  a_hw_indptr, a_hw_indices, a_hw_data, c1_inner, c2_inner, c3_inner, hw_idx, inner_idx,
                  q_ch, q_full, convolved_lateral, discharge_array, raw_array, num_substeps):
    n_in, n_hw = len(inner_idx), len(hw_idx)
    T, n_total = convolved_lateral.shape
    assert discharge_array.shape == raw_array.shape == (T, n_total)
    _check(lib().orcl_unit_route(
        n_in, n_hw, n_total, _i32(lhs_indptr), _i32(lhs_indices), _f64(lhs_off_data),
        _i32(a_inner_indptr), _i32(a_inner_indices), _f64(a_inner_data),
        _i32(a_hw_indptr), _i32(a_hw_indices), _f64(a_hw_data),
        _f64(c1_inner), _f64(c2_inner), _f64(c3_inner),
        np.ascontiguousarray(hw_idx, dtype=np.int64), np.ascontiguousarray(inner_idx, dtype=np.int64),
        q_ch, q_full, _f64(convolved_lateral), discharge_array, raw_array, T, num_substeps))


class Adjoint:
    """What an adjoint arbiter call returns: each gradient, the scale of each (the sum of the absolute values of the terms that
    were added to make it) and `raw`, the unclamped interval means of the forward it ran."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _opt(a):
    """(the array kept alive, its address or None)"""
    if a is None:
        return None, None
    a = _f64(a)
    return a, a.ctypes.data


def _rapid_adjoint(fn, csc_indptr, csc_indices, c1, c2, c3, c4_dt, q0, qlateral, grad_out, grad_qfinal, T, num_substeps):
    n = q0.shape[0]
    T = int(qlateral.shape[0] if qlateral is not None else T)
    assert T >= 1 and num_substeps >= 1
    ql, ql_p = _opt(qlateral)
    go, go_p = _opt(grad_out)
    gf, gf_p = _opt(grad_qfinal)
    assert (ql is None or ql.shape == (T, n)) and (go is None or go.shape == (T, n)) and (gf is None or gf.shape == (n,))
    r = Adjoint(grad_coef=np.zeros((4, n)), grad_q0=np.zeros(n), grad_lateral=None if ql is None else np.zeros((T, n)),
                scale_coef=np.zeros((4, n)), scale_q0=np.zeros(n), scale_lateral=None if ql is None else np.zeros((T, n)),
                raw=np.zeros((T, n)))
    _check(fn(n, _i32(csc_indptr), _i32(csc_indices), _f64(c1), _f64(c2), _f64(c3), _f64(c4_dt), _f64(q0), ql_p, go_p, gf_p, T,
              num_substeps, r.grad_coef, r.grad_q0, None if ql is None else r.grad_lateral.ctypes.data, r.scale_coef, r.scale_q0,
              None if ql is None else r.scale_lateral.ctypes.data, r.raw))
    return r


def rapid_adjoint(csc_indptr, csc_indices, c1, c2, c3, c4_dt, q0, qlateral, grad_out, grad_qfinal, num_substeps, T=None, *, lib_=None):
    """The gradient of L through rapid_route (per-reach c1: lhs_off_data = -c1[indices]) in fp64, by the plain loops of
    rr_oracle_adj.c.  qlateral None: channel-only routing of T rows.  grad_out (T, n) = dL/ddischarge and grad_qfinal (n) may be
    None.  `lib_`: another build of the same source (build_adjoint_reordered)."""
    return _rapid_adjoint((lib_ or lib()).orc_rapid_adjoint, csc_indptr, csc_indices, c1, c2, c3, c4_dt, q0, qlateral, grad_out,
                          grad_qfinal, T, num_substeps)


def rapid_adjoint_ld(csc_indptr, csc_indices, c1, c2, c3, c4_dt, q0, qlateral, grad_out, grad_qfinal, num_substeps, T=None):
    """rapid_adjoint in long double, every output rounded to double once: the arbiter."""
    return _rapid_adjoint(lib().orcl_rapid_adjoint, csc_indptr, csc_indices, c1, c2, c3, c4_dt, q0, qlateral, grad_out,
                          grad_qfinal, T, num_substeps)


def _unit_adjoint(fn, csc_indptr, csc_indices, c1, c2, c3, q_ch0, q_full0, lateral, grad_out, grad_qch_final, grad_qfull_final,
                  num_substeps):
    lateral = _f64(lateral)
    T, n = lateral.shape
    ni = q_ch0.shape[0]
    assert T >= 1 and num_substeps >= 1 and q_full0.shape == (ni,)
    go, go_p = _opt(grad_out)
    gc, gc_p = _opt(grad_qch_final)
    gf, gf_p = _opt(grad_qfull_final)
    assert (go is None or go.shape == (T, n)) and (gc is None or gc.shape == (ni,)) and (gf is None or gf.shape == (ni,))
    m = max(ni, 1)
    r = Adjoint(grad_coef=np.zeros((3, n)), grad_qch0=np.zeros(m), grad_qfull0=np.zeros(m), grad_lateral=np.zeros((T, n)),
                scale_coef=np.zeros((3, n)), scale_states=np.zeros(2 * m), scale_lateral=np.zeros((T, n)), raw=np.zeros((T, n)))
    _check(fn(n, _i32(csc_indptr), _i32(csc_indices), _f64(c1), _f64(c2), _f64(c3), _f64(np.resize(q_ch0, m) if ni else np.zeros(1)),
              _f64(np.resize(q_full0, m) if ni else np.zeros(1)), lateral, go_p, gc_p, gf_p, T, num_substeps,
              r.grad_coef, r.grad_qch0, r.grad_qfull0, r.grad_lateral, r.scale_coef, r.scale_states, r.scale_lateral, r.raw))
    r.scale_qch0, r.scale_qfull0 = r.scale_states[:ni].copy(), r.scale_states[ni:2 * ni].copy()
    r.grad_qch0, r.grad_qfull0 = r.grad_qch0[:ni], r.grad_qfull0[:ni]
    return r


def unit_adjoint(csc_indptr, csc_indices, c1, c2, c3, q_ch0, q_full0, lateral, grad_out, grad_qch_final, grad_qfull_final,
                 num_substeps, *, lib_=None):
    """The gradient of L through unit_route with the callers' unit edge weights, in fp64 (rr_oracle_adj.c): the CSC arrays and
    the coefficients are the whole network's, in params order; the states and their gradients are indexed by inner reach
    (ascending params order), as Plan.unit_adjoint_dev takes them.  Any of the three cotangents may be None."""
    return _unit_adjoint((lib_ or lib()).orc_unit_adjoint, csc_indptr, csc_indices, c1, c2, c3, q_ch0, q_full0, lateral, grad_out,
                         grad_qch_final, grad_qfull_final, num_substeps)


def unit_adjoint_ld(csc_indptr, csc_indices, c1, c2, c3, q_ch0, q_full0, lateral, grad_out, grad_qch_final, grad_qfull_final,
                    num_substeps):
    """unit_adjoint in long double, every output rounded to double once: the arbiter."""
    return _unit_adjoint(lib().orcl_unit_adjoint, csc_indptr, csc_indices, c1, c2, c3, q_ch0, q_full0, lateral, grad_out,
                         grad_qch_final, grad_qfull_final, num_substeps)


def uh_convolve_ld(kernel, state, lateral):
    """UnitHydrograph.convolve in long double: returns the (T, n) rows -- there is no clamp, they are their own unclamped form --
    and updates `state` (n_ks, n) in place to the carried state, both rounded to double once."""
    kernel, lateral = _f64(kernel), _f64(lateral)
    n_ks, n = kernel.shape
    T = lateral.shape[0]
    assert state.shape == (n_ks, n) and lateral.shape == (T, n)
    out = np.empty((T, n))
    _check(lib().orcl_uh_convolve(T, n_ks, n, kernel, state, lateral, out))
    return out


# ---- the scores arbiter (rr_oracle_scores.c): rr.metrics' five scores and their gradient in compensated long double ----

SCORES_LD_ROWS = ('count', 'me', 'mae', 'mse', 'pearson_r', 'kge2012', 'mt', 'mp', 'kappa_t', 'kappa_p', 'beta', 'gamma', 'r_raw')


def _scores_args(y_true, y_pred, columns):
    t, p = _f64(y_true), _f64(y_pred)
    if t.ndim != 2 or p.ndim != 2 or t.shape[0] != p.shape[0]:
        raise ValueError(f'scores arbiter: (T, n) and (T, m) arrays of one length, got {t.shape} and {p.shape}')
    cols = None if columns is None else _i32(columns)
    if cols is not None and cols.shape != (t.shape[1],):
        raise ValueError('scores arbiter: one column index per column of y_true')
    return t, p, cols, (None if cols is None else cols.ctypes.data)


def scores_ld(y_true, y_pred, columns=None, skip_missing=False) -> dict:
    """The five scores of every column of y_true[T, n] against y_pred[T, m] (column columns[j], or j) as rr.metrics defines them, two-pass
    in compensated long double and rounded to double once: {name: (n,)} for SCORES_LD_ROWS -- the pairs kept, the scores, both means,
    kappa = |mean| / std of both series, KGE's beta and gamma, and the unclipped r.  float32 data: widened here (exactly)."""
    t, p, cols, cols_p = _scores_args(y_true, y_pred, columns)
    out = np.empty((len(SCORES_LD_ROWS), t.shape[1]))
    rc = lib().orcl_scores(t.shape[0], t.shape[1], t, p, p.shape[1], cols_p, int(bool(skip_missing)), out)
    if rc == -5:
        raise ValueError('scores arbiter: a column index outside y_pred (or widths that differ without a map)')
    _check(rc)
    return dict(zip(SCORES_LD_ROWS, out))


def scores_grad_ld(y_true, y_pred, G, columns=None, skip_missing=False) -> Adjoint:
    """dL/dy_pred for G[5, n] = dL/d(me, mae, mse, pearson_r, kge2012) by DESIGN.md section 12c's closed form on the long-double
    moments: Adjoint(grad (T, m), scale (T, m): the sum of the absolute values of the terms added into each element, bm (n,):
    |B mt| + |P mp| of each scored column)."""
    t, p, cols, cols_p = _scores_args(y_true, y_pred, columns)
    G = _f64(G)
    assert G.shape == (5, t.shape[1]), G.shape
    r = Adjoint(grad=np.empty(p.shape), scale=np.empty(p.shape), bm=np.empty(t.shape[1]))
    rc = lib().orcl_scores_grad(t.shape[0], t.shape[1], t, p, p.shape[1], cols_p, int(bool(skip_missing)), G, r.grad, r.scale, r.bm)
    if rc == -5:
        raise ValueError('scores arbiter: a column index outside y_pred (or widths that differ without a map)')
    _check(rc)
    return r


# ---- host prep on the path ----

def muskingum_coefficients(k, x, dt_routing):
    """Muskingum.py:172-185 -> (c1, c2, c3); raises ValueError like the reference when they do not sum to 1."""
    k, x = _f64(k), _f64(x)
    c1, c2, c3 = (np.empty_like(k) for _ in range(3))
    _check(lib().orc_muskingum_coefficients(k.shape[0], k, x, float(dt_routing), c1, c2, c3))
    return c1, c2, c3


def adjacency_csc(river_ids, downstream_ids):
    """tools.py:75-109 -> (indptr int32[n+1], indices int32[nnz]) of A[down, up] = 1 in CSC."""
    rid = np.ascontiguousarray(river_ids, dtype=np.int64)
    did = np.ascontiguousarray(downstream_ids, dtype=np.int64)
    n = rid.shape[0]
    indptr = np.zeros(n + 1, dtype=np.int32)
    indices = np.zeros(max(n, 1), dtype=np.int32)
    _check(lib().orc_adjacency_matrix(n, rid, did, indptr, indices))
    return indptr, indices[:indptr[-1]].copy()


class UnitHydrograph:
    """UnitHydrograph.py:13-107 with the kernel handed over as a dense (n_ks, n) array."""

    def __init__(self, kernel):
        self.kernel = _f64(kernel)
        if self.kernel.ndim != 2:
            raise ValueError('kernel must be a 2D array')
        self.state = np.zeros_like(self.kernel)

    def convolve_incrementally(self, runoff_vector):
        n_ks, n = self.kernel.shape
        out = np.empty(n)
        lib().orc_uh_convolve_incrementally(n_ks, n, self.kernel, self.state, _f64(runoff_vector), out)
        return out

    def convolve(self, lateral):
        lateral = _f64(lateral)
        T = lateral.shape[0]
        n_ks, n = self.kernel.shape
        out = np.empty((T, n))
        _check(lib().orc_uh_convolve(T, n_ks, n, self.kernel, self.state, lateral, out))
        return out


def runoff_to_qlateral_core(weights, runoff_raw, catchment_area=None, cumulative=False, force_positive_runoff=False,
                            keep_nan=False):
    """The arithmetic of river_route/runoff.py:296-330 on arrays already extracted from the files: `weights` is the
    scipy CSR (n_rivers, n_points) of proportion * unit conversion (runoff.py:288-291), `runoff_raw` the (T, n_points)
    block of the runoff variable (float32 or float64).  numpy/scipy restatement, same statements in the same order:
    sparse product (296), cumulative -> incremental from the last row down (307-309), clip (310-311), NaN -> 0
    (327-329), times catchment area for volumes (331-332).  `keep_nan` stops before the fill, where the reference's
    irregular-time-step branch resamples (313-325).

    Pinned to the reference: tests/golden/runoff.npz holds what river_route.runoff.runoff_to_qlateral itself returned
    for five seeded cases (tests/golden/make_golden_runoff.py runs the reference function as written; xarray, absent
    from the image, is replaced there by a file-access stand-in that does no arithmetic).  tests/test_runoff.py checks
    this restatement -- through the host logic of river_route_amd.runoff -- against those outputs, and against an
    independent dense evaluation."""
    q = np.array(np.asarray(weights @ np.asarray(runoff_raw).T).T, dtype=np.float64)      # (time, n_rivers)
    if cumulative:
        for i in range(q.shape[0] - 1, 0, -1):
            q[i] -= q[i - 1]
    if force_positive_runoff:
        np.clip(q, 0, None, out=q)
    if not keep_nan:
        mask = np.isnan(q)
        if mask.any():
            q[mask] = 0.0
    if catchment_area is not None:
        q *= np.asarray(catchment_area, dtype=np.float64)[np.newaxis, :]
    return q
