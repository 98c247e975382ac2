"""rr.grad for UnitMuskingum on the host: the pure-torch restatements the GPU tests trust (tests/test_gpu_grad_unit.py) --
dense_unit_route (a dense triangular solve per sub-step over the inner reaches, the reference's statement order) and
dense_uh_convolve (direct form with carried state) -- checked first: forward against the oracle, autograd gradients against
central differences of the oracle; the closed-form adjoint the kernels implement (rr_kernels_adjoint_unit.hpp), written out in
numpy loops, against autograd through the restatement; and the argument checks, which raise before a device is touched."""
import numpy as np
import pytest
import torch

import river_route_amd as rr
import test_grad as cpu
from oracle import oracle
from river_route_amd import _lib
from tests_support import unit_split_arrays


# ---- the restatements (also used by tests/test_gpu_grad_unit.py) ----

def split(down):
    """(hw_idx, inner_idx) of a network given by its downstream indices: reaches without / with upstream reaches, ascending."""
    n = down.shape[0]
    has_up = np.zeros(n, dtype=bool)
    has_up[down[down >= 0]] = True
    return np.flatnonzero(~has_up), np.flatnonzero(has_up)


def dense_unit_route(down, q_ch0, q_full0, lat, c1, c2, c3, nsub):
    """(discharge[T, n], q_ch[n_inner], q_full[n_inner]) of river_route/routers/_numba_kernels.py:unit_route with the callers'
    unit edge weights, in torch.  c1, c2, c3 have n values (the inner reaches' are used)."""
    n = down.shape[0]
    hw, inner = split(down)
    T = lat.shape[0]
    if inner.size == 0:
        return lat + 0.0, q_ch0, q_full0
    kof = -np.ones(n, dtype=np.int64)
    kof[inner] = np.arange(inner.size)
    hof = -np.ones(n, dtype=np.int64)
    hof[hw] = np.arange(hw.size)
    A_in = torch.zeros((inner.size, inner.size), dtype=torch.float64)
    A_hw = torch.zeros((inner.size, hw.size), dtype=torch.float64)
    for i in range(n):
        if down[i] >= 0:
            if kof[i] >= 0:
                A_in[kof[down[i]], kof[i]] = 1.0
            else:
                A_hw[kof[down[i]], hof[i]] = 1.0
    ti, th = torch.as_tensor(inner), torch.as_tensor(hw)
    c1i, c2i, c3i = c1[ti], c2[ti], c3[ti]
    M = torch.eye(inner.size, dtype=torch.float64) - c1i[:, None] * A_in
    q_ch, q_full, rows = q_ch0, q_full0, []
    inv = 1.0 / nsub
    for t in range(T):
        l_hw, l_in = lat[t][th], lat[t][ti]
        hw_sum = A_hw @ l_hw
        c1_a_ql = c1i * (A_in @ l_in + hw_sum)
        acc = torch.zeros_like(l_in)
        for _ in range(nsub):
            rhs = c1_a_ql + c2i * hw_sum + c3i * q_ch + c2i * (A_in @ q_full)
            q_ch = torch.linalg.solve_triangular(M, rhs[:, None], upper=False)[:, 0]
            q_full = q_ch + l_in
            acc = acc + q_full
        m = acc * inv
        row = torch.zeros(n, dtype=torch.float64)
        row = row.index_put((th,), l_hw).index_put((ti,), torch.where(m > 0, m, torch.zeros_like(m)))
        rows.append(row)
    return torch.stack(rows), q_ch, q_full


def dense_uh_convolve(kernel, state, depth):
    """(convolved[T, n], state_out[n_ks, n]) of UnitHydrograph.convolve (river_route/uhkernels/UnitHydrograph.py:93-107), direct form."""
    n_ks, n = kernel.shape
    T = depth.shape[0]
    buf = torch.zeros((T + n_ks - 1, n), dtype=torch.float64)
    for j in range(n_ks):
        buf = buf + torch.nn.functional.pad(kernel[j] * depth, (0, 0, j, n_ks - 1 - j))
    buf = buf + torch.nn.functional.pad(state, (0, 0, 0, T - 1))[:T + n_ks - 1]
    return buf[:T], torch.cat([buf[T:], torch.zeros((1, n), dtype=torch.float64)])


def oracle_unit_route(down, q_ch0, q_full0, lat, k, x, dt_routing, nsub):
    indptr, indices = cpu.csc_from_down(down)
    n = down.shape[0]
    c1, c2, c3 = oracle.muskingum_coefficients(k, x, dt_routing)
    hw_idx, inner_idx, A_in, A_hw = unit_split_arrays(indptr, indices, n)
    c1i, c2i, c3i = c1[inner_idx], c2[inner_idx], c3[inner_idx]
    qc, qf, d = np.array(q_ch0, dtype=np.float64), np.array(q_full0, dtype=np.float64), np.zeros(lat.shape)
    oracle.unit_route(A_in.indptr, A_in.indices, -c1i[A_in.indices], A_in.indptr, A_in.indices, A_in.data, A_hw.indptr, A_hw.indices,
                      A_hw.data, c1i, c2i, c3i, hw_idx, inner_idx, qc, qf, np.ascontiguousarray(lat), d, nsub)
    return d, qc, qf


def oracle_uh_convolve(kernel, state, depth):
    uh = oracle.UnitHydrograph(kernel)
    uh.state[:] = state
    conv = uh.convolve(depth)
    return conv, uh.state.copy()


def unit_inputs(down, T, seed, low=0.0, n_ks=None):
    """Random lateral (or depth) rows, states, loss weights; with n_ks also a kernel and a carried convolution state."""
    n = down.shape[0]
    ni = split(down)[1].size
    rng = np.random.default_rng(seed)
    d = dict(lat=rng.uniform(low, 2.0, (T, n)) * 50.0, q_ch0=rng.uniform(0.0, 80.0, ni), q_full0=rng.uniform(0.0, 120.0, ni),
             G=rng.standard_normal((T, n)), Gc=rng.standard_normal(ni), Gf=rng.standard_normal(ni))
    if n_ks is not None:
        kern = rng.uniform(0.0, 1.0, (n_ks, n))
        d.update(kernel=kern / kern.sum(0), state=rng.uniform(0.0, 20.0, (n_ks, n)), Gs=rng.standard_normal((n_ks, n)))
        d['state'][-1] = 0.0         # what a convolve call leaves; a gradient is asked of the row all the same
    return d


def dense_unit_loss_grads(down, k, x, d, dt_routing, nsub):
    """L = sum(G out) + sum(Gc q_ch) + sum(Gf q_full) through the restatement: gradients as numpy, by name."""
    t = {key: torch.tensor(d[key], requires_grad=True) for key in ('lat', 'q_ch0', 'q_full0')}
    kt, xt = torch.tensor(k, requires_grad=True), torch.tensor(x, requires_grad=True)
    c1, c2, c3 = rr.grad.muskingum_coefficients(kt, xt, dt_routing)
    out, qc, qf = dense_unit_route(down, t['q_ch0'], t['q_full0'], t['lat'], c1, c2, c3, nsub)
    L = (out * torch.as_tensor(d['G'])).sum() + (qc * torch.as_tensor(d['Gc'])).sum() + (qf * torch.as_tensor(d['Gf'])).sum()
    L.backward()
    z = lambda v: (torch.zeros_like(v) if v.grad is None else v.grad).numpy()      # noqa: E731
    return dict(k=z(kt), x=z(xt), lat=z(t['lat']), q_ch0=z(t['q_ch0']), q_full0=z(t['q_full0']), out=out.detach().numpy())


def dense_unit_muskingum_loss_grads(down, k, x, d, dt_routing, nsub, window=None):
    """The same through convolution + routing (d['lat'] holds the runoff depths), with sum(Gs uh_state_out) added."""
    t = {key: torch.tensor(d[key], requires_grad=True) for key in ('lat', 'q_ch0', 'q_full0', 'kernel', 'state')}
    kt, xt = torch.tensor(k, requires_grad=True), torch.tensor(x, requires_grad=True)
    c1, c2, c3 = rr.grad.muskingum_coefficients(kt, xt, dt_routing)
    T = d['lat'].shape[0]
    R = T if window is None else window
    qc, qf, st, rows = t['q_ch0'], t['q_full0'], t['state'], []
    for t0 in range(0, T, R):
        conv, st = dense_uh_convolve(t['kernel'], st, t['lat'][t0:t0 + R])
        out, qc, qf = dense_unit_route(down, qc, qf, conv, c1, c2, c3, nsub)
        rows.append(out)
    out = torch.cat(rows)
    L = ((out * torch.as_tensor(d['G'])).sum() + (qc * torch.as_tensor(d['Gc'])).sum() + (qf * torch.as_tensor(d['Gf'])).sum() +
         (st * torch.as_tensor(d['Gs'])).sum())
    L.backward()
    z = lambda v: (torch.zeros_like(v) if v.grad is None else v.grad).numpy()      # noqa: E731
    return dict(k=z(kt), x=z(xt), depth=z(t['lat']), q_ch0=z(t['q_ch0']), q_full0=z(t['q_full0']), kernel=z(t['kernel']),
                state=z(t['state']), out=out.detach().numpy())


# ---- the closed-form adjoint (what the kernels implement) ----

def closed_form_unit_adjoint(down, q_ch0, q_full0, lat, c1, c2, c3, nsub, G, Gc, Gf):
    """Forward and adjoint recurrences of rr_kernels_adjoint_unit.hpp in plain loops: gradients of lat, q_ch0, q_full0, c1, c2, c3."""
    n, T = down.shape[0], lat.shape[0]
    S = T * nsub
    hw, inner = split(down)
    kof = {int(i): k for k, i in enumerate(inner)}
    ups = [[] for _ in range(n)]
    for i in range(n):
        if down[i] >= 0:
            ups[down[i]].append(i)
    is_hw = np.ones(n, dtype=bool)
    is_hw[inner] = False
    qc, qf = np.zeros((S + 1, n)), np.zeros((S + 1, n))
    qc[0, inner], qf[0, inner] = q_ch0, q_full0
    new, old = np.zeros((S + 1, n)), np.zeros((S + 1, n))
    for s in range(1, S + 1):
        t = (s - 1) // nsub
        for i in inner:      # ascending: upstream first
            a = sum(lat[t, h] for h in ups[i] if is_hw[h])
            new[s, i] = a + sum(qf[s, u] for u in ups[i] if not is_hw[u])
            old[s, i] = a + sum(qf[s - 1, u] for u in ups[i] if not is_hw[u])
            qc[s, i] = c1[i] * new[s, i] + c2[i] * old[s, i] + c3[i] * qc[s - 1, i]
            qf[s, i] = qc[s, i] + lat[t, i]
    out = lat.copy()
    for t in range(T):
        m = qf[t * nsub + 1:(t + 1) * nsub + 1].mean(0)
        out[t, inner] = np.maximum(m[inner], 0.0)
    mu, phi = np.zeros((S + 2, n)), np.zeros((S + 2, n))
    for s in range(S, 0, -1):
        t = (s - 1) // nsub
        for i in inner[::-1]:      # descending: downstream first
            d = down[i]
            p = (G[t, i] / nsub if out[t, i] > 0 else 0.0) + (Gf[kof[i]] if s == S else 0.0)
            if d >= 0:
                p += c1[d] * mu[s, d] + c2[d] * mu[s + 1, d]
            phi[s, i] = p
            mu[s, i] = p + (Gc[kof[i]] if s == S else 0.0) + c3[i] * mu[s + 1, i]
    g = dict(c1=np.zeros(n), c2=np.zeros(n), c3=np.zeros(n), lat=np.zeros((T, n)), q_ch0=np.zeros(inner.size), q_full0=np.zeros(inner.size))
    for i in inner:
        g['c1'][i] = (mu[1:S + 1, i] * new[1:, i]).sum()
        g['c2'][i] = (mu[1:S + 1, i] * old[1:, i]).sum()
        g['c3'][i] = (mu[1:S + 1, i] * qc[:S, i]).sum()
        g['q_ch0'][kof[i]] = c3[i] * mu[1, i]
        d = down[i]
        g['q_full0'][kof[i]] = c2[d] * mu[1, d] if d >= 0 else 0.0
    for t in range(T):
        rows = slice(t * nsub + 1, (t + 1) * nsub + 1)
        for i in range(n):
            if not is_hw[i]:
                g['lat'][t, i] = phi[rows, i].sum()
            else:
                d = down[i]
                g['lat'][t, i] = G[t, i] + ((c1[d] + c2[d]) * mu[rows, d].sum() if d >= 0 else 0.0)
    return g, out


def closed_form_uh_adjoint(kernel, depth, Gconv, Gstate):
    n_ks, n = kernel.shape
    T = depth.shape[0]
    Gb = np.zeros((T + 2 * n_ks, n))
    Gb[:T] = Gconv
    Gb[T:T + n_ks - 1] = Gstate[:n_ks - 1]
    g_depth, g_kernel = np.zeros((T, n)), np.zeros((n_ks, n))
    for t in range(T):
        for j in range(n_ks):
            g_depth[t] += kernel[j] * Gb[t + j]
            g_kernel[j] += depth[t] * Gb[t + j]
    return g_depth, g_kernel, Gb[:n_ks].copy()


def close(got, want, what, rtol):
    scale = max(float(np.abs(want).max()) if want.size else 0.0, 1e-300)
    np.testing.assert_allclose(got, want, rtol=rtol, atol=rtol * scale, err_msg=what)


# ---- the restatements checked ----

@pytest.mark.parametrize('kind,n,T,nsub', [('tree', 60, 12, 1), ('forest', 80, 9, 2), ('chain', 40, 10, 4), ('postorder', 1, 5, 2),
                                           ('tree', 200, 6, 3)])
def test_unit_restatement_forward_matches_oracle(kind, n, T, nsub):
    down, k, x = cpu.network(kind, n, seed=n + T)
    d = unit_inputs(down, T, n, low=-0.3)          # some negative rows: the clamp is active in places, headwaters stay negative
    dt = 3600.0 / nsub
    want = oracle_unit_route(down, d['q_ch0'], d['q_full0'], d['lat'], k, x, dt, nsub)
    c1, c2, c3 = rr.grad.muskingum_coefficients(torch.tensor(k), torch.tensor(x), dt)
    got = dense_unit_route(down, torch.tensor(d['q_ch0']), torch.tensor(d['q_full0']), torch.tensor(d['lat']), c1, c2, c3, nsub)
    scale = np.abs(want[0]).max()
    for g, w in zip(got, want):
        np.testing.assert_allclose(g.numpy(), w, rtol=1e-12, atol=1e-12 * scale)


@pytest.mark.parametrize('n,T,n_ks', [(30, 20, 6), (17, 3, 8), (5, 9, 1), (40, 1, 4), (12, 48, 48)])
def test_uh_restatement_forward_matches_oracle(n, T, n_ks):
    rng = np.random.default_rng(n + T)
    kernel, state, depth = rng.uniform(0, 1, (n_ks, n)), rng.uniform(0, 5, (n_ks, n)), rng.uniform(0, 3, (T, n))
    want = oracle_uh_convolve(kernel, state, depth)
    got = dense_uh_convolve(torch.tensor(kernel), torch.tensor(state), torch.tensor(depth))
    scale = np.abs(want[0]).max()
    for g, w in zip(got, want):
        np.testing.assert_allclose(g.numpy(), w, rtol=1e-12, atol=1e-12 * scale)


@pytest.mark.parametrize('kind,nsub', [('tree', 1), ('forest', 2), ('chain', 4)])
def test_unit_restatement_gradients_match_finite_differences(kind, nsub):
    n, T = 40, 6
    dt = 3600.0 / nsub
    down, k, x = cpu.network(kind, n, seed=7)
    d = unit_inputs(down, T, 11, low=0.2)           # positive: no clamp kink inside the differences
    inner = split(down)[1]

    def loss(k_, x_, lat_):
        out, qc, qf = oracle_unit_route(down, d['q_ch0'], d['q_full0'], lat_, k_, x_, dt, nsub)
        return float((d['G'] * out).sum() + (d['Gc'] * qc).sum() + (d['Gf'] * qf).sum())

    g = dense_unit_loss_grads(down, k, x, d, dt, nsub)
    assert np.abs(g['k'][inner]).min() > 0 and not g['k'][split(down)[0]].any()        # headwaters: never read
    for i in (int(inner[0]), int(inner[inner.size // 2]), int(inner[-1])):
        for name, base, h in (('k', k, 1e-4 * k[i]), ('x', x, 1e-5)):
            vp, vm = base.copy(), base.copy()
            vp[i] += h
            vm[i] -= h
            fd = ((loss(vp, x, d['lat']) - loss(vm, x, d['lat'])) if name == 'k' else (loss(k, vp, d['lat']) - loss(k, vm, d['lat']))) / (2 * h)
            assert abs(fd - g[name][i]) <= 1e-6 * max(abs(fd), np.abs(g[name]).max()), (name, i, fd, g[name][i])
    lat = d['lat']
    for t, i in ((0, 0), (T // 2, n // 3), (T - 1, n - 1), (1, int(split(down)[0][0]))):
        h = 1e-3 * lat[t, i]
        qp, qm = lat.copy(), lat.copy()
        qp[t, i] += h
        qm[t, i] -= h
        fd = (loss(k, x, qp) - loss(k, x, qm)) / (2 * h)
        assert abs(fd - g['lat'][t, i]) <= 1e-6 * max(abs(fd), np.abs(g['lat']).max()), (t, i, fd, g['lat'][t, i])


def test_uh_restatement_gradients_match_finite_differences():
    n, T, n_ks = 9, 7, 4
    rng = np.random.default_rng(2)
    kernel, state, depth = rng.uniform(0, 1, (n_ks, n)), rng.uniform(0, 5, (n_ks, n)), rng.uniform(0, 3, (T, n))
    Gc, Gs = rng.standard_normal((T, n)), rng.standard_normal((n_ks, n))

    def loss(kernel_, state_, depth_):
        conv, st = oracle_uh_convolve(kernel_, state_, depth_)
        return float((Gc * conv).sum() + (Gs * st).sum())

    ts = [torch.tensor(v, requires_grad=True) for v in (kernel, state, depth)]
    conv, st = dense_uh_convolve(*ts)
    ((conv * torch.as_tensor(Gc)).sum() + (st * torch.as_tensor(Gs)).sum()).backward()
    args = [kernel, state, depth]
    for a, (name, idx) in ((0, ('kernel', (0, 0))), (0, ('kernel', (n_ks - 1, 3))), (1, ('state', (1, 2))), (1, ('state', (n_ks - 1, 0))),
                           (2, ('depth', (0, 1))), (2, ('depth', (T - 1, n - 1)))):
        h = 1e-3
        vp, vm = [v.copy() for v in args], [v.copy() for v in args]
        vp[a][idx] += h
        vm[a][idx] -= h
        fd = (loss(*vp) - loss(*vm)) / (2 * h)
        got = float(ts[a].grad[idx])
        assert abs(fd - got) <= 1e-6 * max(abs(fd), float(ts[a].grad.abs().max())), (name, idx, fd, got)


CLOSED = [('tree', 30, 6, 1, 0.2), ('tree', 25, 4, 2, -3.0), ('forest', 40, 5, 4, 0.0), ('chain', 12, 7, 2, -3.0), ('postorder', 1, 3, 2, 0.0),
          ('tree', 2, 3, 1, 0.0), ('forest', 40, 5, 1, -3.0)]


@pytest.mark.parametrize('kind,n,T,nsub,low', CLOSED)
def test_closed_form_unit_adjoint_matches_autograd(kind, n, T, nsub, low):
    down, k, x = cpu.network(kind, n, seed=n + T + nsub)
    d = unit_inputs(down, T, n + 3, low=low)
    c1, c2, c3 = (torch.tensor(c, requires_grad=True) for c in oracle.muskingum_coefficients(k, x, 3600.0 / nsub))
    t = {key: torch.tensor(d[key], requires_grad=True) for key in ('lat', 'q_ch0', 'q_full0')}
    out, qc, qf = dense_unit_route(down, t['q_ch0'], t['q_full0'], t['lat'], c1, c2, c3, nsub)
    L = (out * torch.as_tensor(d['G'])).sum() + (qc * torch.as_tensor(d['Gc'])).sum() + (qf * torch.as_tensor(d['Gf'])).sum()
    L.backward()
    got, out_np = closed_form_unit_adjoint(down, d['q_ch0'], d['q_full0'], d['lat'], c1.detach().numpy(), c2.detach().numpy(),
                                           c3.detach().numpy(), nsub, d['G'], d['Gc'], d['Gf'])
    close(out_np, out.detach().numpy(), 'forward', 1e-12)
    if low < 0 and n > 2:
        inner = split(down)[1]
        assert (out_np[:, inner] == 0).any()          # the clamp is active
    z = lambda v: (torch.zeros_like(v) if v.grad is None else v.grad).numpy()      # noqa: E731
    want = dict(c1=z(c1), c2=z(c2), c3=z(c3), lat=z(t['lat']), q_ch0=z(t['q_ch0']), q_full0=z(t['q_full0']))
    for name in want:
        close(got[name], want[name], f'{kind} n={n} T={T} nsub={nsub}: d/d{name}', 1e-10)


@pytest.mark.parametrize('n,T,n_ks', [(11, 20, 6), (7, 3, 8), (5, 9, 1), (6, 1, 4), (4, 1, 1)])
def test_closed_form_uh_adjoint_matches_autograd(n, T, n_ks):
    rng = np.random.default_rng(n * T)
    kernel, state, depth = rng.uniform(0, 1, (n_ks, n)), rng.uniform(0, 5, (n_ks, n)), rng.uniform(0, 3, (T, n))
    Gc, Gs = rng.standard_normal((T, n)), rng.standard_normal((n_ks, n))
    ts = [torch.tensor(v, requires_grad=True) for v in (kernel, state, depth)]
    conv, st = dense_uh_convolve(*ts)
    ((conv * torch.as_tensor(Gc)).sum() + (st * torch.as_tensor(Gs)).sum()).backward()
    g_depth, g_kernel, g_state = closed_form_uh_adjoint(kernel, depth, Gc, Gs)
    close(g_kernel, ts[0].grad.numpy(), 'kernel', 1e-10)
    close(g_state, ts[1].grad.numpy(), 'state', 1e-10)
    close(g_depth, ts[2].grad.numpy(), 'depth', 1e-10)


# ---- arguments ----

def test_unit_arguments_checked_before_a_device():
    n = 5
    plan = cpu.host_only_plan(n)
    ni = plan.n_inner
    assert ni == n - 1
    f64 = dict(dtype=torch.float64)
    qc, qf, lat = torch.ones(ni, **f64), torch.ones(ni, **f64), torch.ones((4, n), **f64)
    k, x = torch.full((n,), 3600.0, **f64), torch.full((n,), 0.2, **f64)
    kern, st = torch.ones((3, n), **f64), torch.zeros((3, n), **f64)
    g = rr.grad.unit_route
    with pytest.raises(TypeError, match='Plan'):
        g(object(), qc, qf, lat, k, x, 900.0, 3600.0)
    with pytest.raises(TypeError, match='float64'):
        g(plan, qc.float(), qf, lat, k, x, 900.0, 3600.0)
    with pytest.raises(TypeError, match='float64'):
        g(plan, qc, qf, lat.float(), k, x, 900.0, 3600.0)
    with pytest.raises(ValueError, match='shape'):
        g(plan, torch.ones(n, **f64), qf, lat, k, x, 900.0, 3600.0)
    with pytest.raises(ValueError, match='shape'):
        g(plan, qc, qf, torch.ones((4, n + 1), **f64), k, x, 900.0, 3600.0)
    with pytest.raises(ValueError, match='ensembles'):
        g(plan, qc, qf, torch.ones((2, 4, n), **f64), k, x, 900.0, 3600.0)
    with pytest.raises(ValueError, match='whole number'):
        g(plan, qc, qf, lat, k, x, 900.0, 1000.0)
    with pytest.raises(ValueError, match='positive'):
        g(plan, qc, qf, lat, k, x, 0.0, 3600.0)
    with pytest.raises(ValueError, match='rows_per_window'):
        g(plan, qc, qf, lat, k, x, 900.0, 3600.0, rows_per_window=0)
    with pytest.raises(ValueError, match='shape'):
        g(plan, qc, qf, lat, k[:-1], x, 900.0, 3600.0)
    with pytest.raises(ValueError, match='contiguous'):
        g(plan, qc, qf, torch.ones((n, 4), **f64).t(), k, x, 900.0, 3600.0)
    with pytest.raises(ValueError, match='host-only'):
        g(plan, qc, qf, lat, k, x, 900.0, 3600.0)
    m = rr.grad.unit_muskingum
    with pytest.raises(ValueError, match='ensembles'):
        m(plan, qc, qf, torch.ones((2, 4, n), **f64), kern, st, k, x, 900.0, 3600.0)
    with pytest.raises(ValueError, match='uh_kernel'):
        m(plan, qc, qf, lat, kern[0], st, k, x, 900.0, 3600.0)
    with pytest.raises(ValueError, match='shape'):
        m(plan, qc, qf, lat, kern, st[:2], k, x, 900.0, 3600.0)
    with pytest.raises(TypeError, match='float64'):
        m(plan, qc, qf, lat, kern.float(), st, k, x, 900.0, 3600.0)
    with pytest.raises(ValueError, match='host-only'):
        m(plan, qc, qf, lat, kern, st, k, x, 900.0, 3600.0)
    u = rr.grad.uh_convolve
    with pytest.raises(ValueError, match='2-D'):
        u(kern[0], st, lat)
    with pytest.raises(ValueError, match='shape'):
        u(kern, st[:2], lat)
    with pytest.raises(TypeError, match='float64'):
        u(kern, st, lat.float())
    with pytest.raises(ValueError, match='ensembles'):
        u(kern, st, torch.ones((2, 4, n), **f64))
    with pytest.raises(ValueError, match='GPU'):
        u(kern, st, lat)          # host tensors


def test_host_only_plan_has_no_unit_adjoint():
    plan = cpu.host_only_plan()
    with pytest.raises(_lib.RRError) as e:
        plan.unit_adjoint_work_bytes(4, 1)
    assert e.value.code == _lib.RR_E_UNSUPPORTED
    with pytest.raises(_lib.RRError) as e:
        plan.unit_adjoint_dev(None, None, None, 0, None, None, None, None, None, None, None, None, None, 0, 4, 1)
    assert e.value.code == _lib.RR_E_UNSUPPORTED
    assert rr.engine.uh_adjoint_work_bytes(100, 48, 1_000_000) == 0          # enough column blocks: one row range, written in place
    assert rr.engine.uh_adjoint_work_bytes(100, 3, 1000) == 8 * 100 * 3 * 1000
    with pytest.raises(_lib.RRError) as e:
        rr.engine.uh_adjoint_work_bytes(0, 3, 10)
    assert e.value.code == _lib.RR_E_INVALID
