"""rr.grad on the host: muskingum_coefficients against the routers' numpy coefficients and the oracle (bit for bit, the error
case included); the pure-torch restatement of the routing loop that the GPU tests trust (tests/test_gpu_grad.py), checked
first -- its forward against the oracle, its autograd gradients against central finite differences of the oracle; and the
argument checks, which raise before a device is touched."""
import logging
import types

import numpy as np
import pytest
import scipy.sparse
import torch

import river_route_amd as rr
from oracle import oracle
from river_route_amd import _lib, synth
from river_route_amd.engine import Plan
from river_route_amd.routers import Muskingum


# ---- the restatement (also used by tests/test_gpu_grad.py) ----

def dense_route(down, q0, ql, c1, c2, c3, c4dt, nsub, rows=None):
    """(discharge[T, n], q_final[n]) of river_route/routers/_numba_kernels.py:rapid_route with per-reach coefficients, in torch:
    a dense unit lower-triangular solve per sub-step (n <= 300 or so).  ql None: channel-only, `rows` rows.  down[i]: the
    downstream index of reach i (-1 at outlets), reaches sorted upstream first."""
    n = q0.shape[0]
    idx = np.arange(n)
    has = down >= 0
    A = torch.zeros((n, n), dtype=torch.float64)
    A[torch.as_tensor(down[has]), torch.as_tensor(idx[has])] = 1.0
    M = torch.eye(n, dtype=torch.float64) - c1[:, None] * A
    B = c2[:, None] * A
    T = rows if ql is None else ql.shape[0]
    q, out = q0, []
    inv = 1.0 / nsub
    for t in range(T):
        acc = torch.zeros_like(q0)
        for _ in range(nsub):
            rhs = B @ q + c3 * q
            if ql is not None:
                rhs = rhs + c4dt * ql[t]
            q = torch.linalg.solve_triangular(M, rhs[:, None], upper=False)[:, 0]
            acc = acc + q
        m = acc * inv
        out.append(torch.where(m > 0, m, torch.zeros_like(m)))
    return torch.stack(out), q


def csc_from_down(down):
    has = down >= 0
    indptr = np.concatenate([[0], np.cumsum(has)]).astype(np.int32)
    return indptr, down[has].astype(np.int32)


def oracle_route(down, q0, ql, k, x, dt_routing, dt_runoff):
    """The oracle's rapid_route with the routers' coefficients: (discharge, q_final) as numpy arrays."""
    indptr, indices = csc_from_down(down)
    c1, c2, c3 = oracle.muskingum_coefficients(k, x, dt_routing)
    nsub = int(round(dt_runoff / dt_routing))
    q = np.array(q0, dtype=np.float64)
    d = np.zeros(ql.shape)
    oracle.rapid_route(indptr, indices, -c1[indices], c2, c3, (c1 + c2) / dt_runoff, q, np.ascontiguousarray(ql), d, nsub)
    return d, q


def network(kind, n, seed=3):
    """(down, k, x) of a test network: 'tree' (random topology, random order), 'postorder', 'forest' (several outlets),
    'chain' (one long channel)."""
    if kind == 'chain':
        down = np.append(np.arange(1, n), -1).astype(np.int64)
        idx = np.arange(n)
        return down, 900.0 + 6300.0 * synth.u01(seed, idx), 0.05 + 0.40 * synth.u01(seed + 1, idx)
    if kind == 'forest':
        net = synth.synth_network_chain(n, seed=seed, n_outlets=max(1, n // 20), p_chain=0.3)
    else:
        net = synth.synth_network(n, seed=seed, order='postorder' if kind == 'postorder' else 'random')
    return net.down_index.astype(np.int64), net.k, net.x


def dense_loss_grads(down, k, x, ql, q0, dt_routing, dt_runoff, G, Gf):
    """L = sum(G * discharge) + sum(Gf * q_final) through the restatement: (L, dL/dk, dL/dx, dL/dql, dL/dq0) as numpy."""
    kt, xt = torch.tensor(k, requires_grad=True), torch.tensor(x, requires_grad=True)
    qlt = None if ql is None else torch.tensor(ql, requires_grad=True)
    q0t = torch.tensor(q0, requires_grad=True)
    c1, c2, c3 = rr.grad.muskingum_coefficients(kt, xt, dt_routing)
    nsub = int(round(dt_runoff / dt_routing))
    d, qf = dense_route(down, q0t, qlt, c1, c2, c3, (c1 + c2) / dt_runoff, nsub, rows=G.shape[0])
    L = (d * torch.as_tensor(G)).sum() + (qf * torch.as_tensor(Gf)).sum()
    L.backward()
    return (float(L.detach()), kt.grad.numpy(), xt.grad.numpy(), None if qlt is None else qlt.grad.numpy(), q0t.grad.numpy())


# ---- coefficients ----

def router_coefficients(k, x, dt):
    """The routers' own method on a stand-in object (river_route/routers/Muskingum.py:172-193)."""
    n = k.shape[0]
    me = types.SimpleNamespace(k=k, x=x, logger=logging.getLogger('test_grad'), A=scipy.sparse.csc_matrix((n, n)))
    Muskingum._set_muskingum_coefficients(me, dt)
    return me.c1, me.c2, me.c3


@pytest.mark.parametrize('dt', [60.0, 900.0, 3600.0, 86400.0])
def test_coefficients_bit_equal_to_routers_and_oracle(dt):
    rng = np.random.default_rng(int(dt))
    n = 20000
    k = rng.uniform(100.0, 50000.0, n)
    x = rng.uniform(0.0, 0.5, n)
    got = rr.grad.muskingum_coefficients(torch.tensor(k), torch.tensor(x), dt)
    for want in (router_coefficients(k, x, dt), oracle.muskingum_coefficients(k, x, dt)):
        for g, w in zip(got, want):
            assert g.dtype == torch.float64
            assert np.array_equal(g.numpy(), w)


def test_coefficients_error_case():
    k = np.array([3600.0, 0.0, 7200.0])
    x = np.array([0.2, 0.3, 0.1])
    with pytest.raises(ValueError, match='do not sum to 1'):
        rr.grad.muskingum_coefficients(torch.tensor(k), torch.tensor(x), 900.0)
    with pytest.raises(ValueError):
        router_coefficients(k, x, 900.0)
    with pytest.raises(ValueError):
        oracle.muskingum_coefficients(k, x, 900.0)


# ---- the restatement checked ----

@pytest.mark.parametrize('kind,n,T,nsub', [('tree', 60, 12, 1), ('forest', 80, 9, 2), ('chain', 40, 10, 4), ('postorder', 1, 5, 2),
                                           ('tree', 200, 6, 3)])
def test_restatement_forward_matches_oracle(kind, n, T, nsub):
    down, k, x = network(kind, n, seed=n + T)
    rng = np.random.default_rng(n)
    dt_runoff = 3600.0
    ql = rng.uniform(-0.3, 2.0, (T, n)) * dt_runoff        # some negative rows: the clamp is active in places
    q0 = rng.uniform(0.0, 3.0, n)
    d_ref, q_ref = oracle_route(down, q0, ql, k, x, dt_runoff / nsub, dt_runoff)
    c1, c2, c3 = rr.grad.muskingum_coefficients(torch.tensor(k), torch.tensor(x), dt_runoff / nsub)
    d, q = dense_route(down, torch.tensor(q0), torch.tensor(ql), c1, c2, c3, (c1 + c2) / dt_runoff, nsub)
    scale = np.abs(d_ref).max()
    np.testing.assert_allclose(d.numpy(), d_ref, rtol=1e-12, atol=1e-12 * scale)
    np.testing.assert_allclose(q.numpy(), q_ref, rtol=1e-12, atol=1e-12 * scale)


@pytest.mark.parametrize('kind,nsub', [('tree', 1), ('forest', 2), ('chain', 4)])
def test_restatement_gradients_match_finite_differences(kind, nsub):
    n, T, dt_runoff = 40, 6, 3600.0
    dt = dt_runoff / nsub
    down, k, x = network(kind, n, seed=7)
    rng = np.random.default_rng(11)
    ql = rng.uniform(0.2, 2.0, (T, n)) * dt_runoff       # positive: no clamp kink inside the differences
    q0 = rng.uniform(0.5, 3.0, n)
    G = rng.standard_normal((T, n))
    Gf = rng.standard_normal(n)

    def loss(k_, x_, ql_):
        d, q = oracle_route(down, q0, ql_, k_, x_, dt, dt_runoff)
        return float((G * d).sum() + (Gf * q).sum())

    _, gk, gx, gql, _ = dense_loss_grads(down, k, x, ql, q0, dt, dt_runoff, G, Gf)
    for i in (0, n // 2, n - 1):
        h = 1e-4 * k[i]
        kp, km = k.copy(), k.copy()
        kp[i] += h
        km[i] -= h
        fd = (loss(kp, x, ql) - loss(km, x, ql)) / (2 * h)
        assert abs(fd - gk[i]) <= 1e-6 * max(abs(fd), np.abs(gk).max()), (i, fd, gk[i])
        h = 1e-5
        xp, xm = x.copy(), x.copy()
        xp[i] += h
        xm[i] -= h
        fd = (loss(k, xp, ql) - loss(k, xm, ql)) / (2 * h)
        assert abs(fd - gx[i]) <= 1e-6 * max(abs(fd), np.abs(gx).max()), (i, fd, gx[i])
    for t, i in ((0, 0), (T // 2, n // 3), (T - 1, n - 1)):
        h = 1e-3 * ql[t, i]
        qp, qm = ql.copy(), ql.copy()
        qp[t, i] += h
        qm[t, i] -= h
        fd = (loss(k, x, qp) - loss(k, x, qm)) / (2 * h)
        assert abs(fd - gql[t, i]) <= 1e-6 * max(abs(fd), np.abs(gql).max()), (t, i, fd, gql[t, i])


# ---- arguments ----

def host_only_plan(n=5):
    down = np.append(np.arange(1, n), -1).astype(np.int64)
    indptr, indices = csc_from_down(down)
    return Plan(indptr, indices, device=_lib.RR_DEVICE_NONE)


def test_arguments_checked_before_a_device():
    n = 5
    plan = host_only_plan(n)
    f64 = dict(dtype=torch.float64)
    q0, ql, k, x = torch.ones(n, **f64), torch.ones((4, n), **f64), torch.full((n,), 3600.0, **f64), torch.full((n,), 0.2, **f64)
    g = rr.grad.rapid_route
    with pytest.raises(TypeError, match='Plan'):
        g(object(), q0, ql, k, x, 900.0, 3600.0)
    with pytest.raises(TypeError, match='float64'):
        g(plan, q0.float(), ql, k, x, 900.0, 3600.0)
    with pytest.raises(TypeError, match='float64'):
        g(plan, q0, ql.float(), k, x, 900.0, 3600.0)
    with pytest.raises(ValueError, match='shape'):
        g(plan, torch.ones(n + 1, **f64), ql, k, x, 900.0, 3600.0)
    with pytest.raises(ValueError, match='ensembles'):
        g(plan, q0, torch.ones((2, 4, n), **f64), k, x, 900.0, 3600.0)
    with pytest.raises(ValueError, match='whole number'):
        g(plan, q0, ql, k, x, 900.0, 1000.0)
    with pytest.raises(ValueError, match='positive'):
        g(plan, q0, ql, k, x, 0.0, 3600.0)
    with pytest.raises(ValueError, match='rows'):
        g(plan, q0, None, k, x, 900.0, 3600.0)
    with pytest.raises(ValueError, match='rows_per_window'):
        g(plan, q0, ql, k, x, 900.0, 3600.0, rows_per_window=0)
    with pytest.raises(ValueError, match='shape'):
        g(plan, q0, ql, k[:-1], x, 900.0, 3600.0)
    with pytest.raises(ValueError, match='contiguous'):
        g(plan, q0, torch.ones((n, 4), **f64).t(), k, x, 900.0, 3600.0)
    with pytest.raises(ValueError, match='host-only'):
        g(plan, q0, ql, k, x, 900.0, 3600.0)


def test_host_only_plan_has_no_adjoint():
    plan = host_only_plan()
    with pytest.raises(_lib.RRError) as e:
        plan.rapid_adjoint_work_bytes(4, 1)
    assert e.value.code == _lib.RR_E_UNSUPPORTED
    with pytest.raises(_lib.RRError) as e:
        plan.rapid_adjoint_dev(None, None, 0, None, None, None, None, None, None, None, 0, 4, 1)
    assert e.value.code == _lib.RR_E_UNSUPPORTED
    assert _lib.lib().rr_version() >= 230
