"""gauges= of rr.grad.rapid_route and rr.grad.rapid_route_batch on the GPU (rr_rapid_adjoint_gauges_dev: the slot map kernels, k_adj_mask
over the (T, G) blocks, the gauge form of k_adj_tick in its four instantiations).  The gauge path and the dense path with the loss on
discharge[:, gauges] perform the same floating-point operations on the same values, so every output is compared with np.array_equal;
against the pure-torch restatement of tests/test_grad.py, whose cotangent is scattered to full width, the tolerance is the project's
1e-9.  Windows, members, repeat runs, the work memory and its refusals, the scores on top, and the peak memory of a backward pass."""
import numpy as np
import pytest
import torch

import river_route_amd as rr
import test_grad as cpu
from oracle import oracle
from river_route_amd import _lib, synth
from river_route_amd.engine import DeviceBuffer, Plan
from test_gpu_grad import DEV, _default_knobs, assert_grad, inputs, make_plan  # noqa: F401  (the fixture resets the engine's knobs)

pytestmark = pytest.mark.gpu
DT_RUNOFF = 3600.0
NAMES = ('gauge discharge', 'q_final', 'k.grad', 'x.grad', 'qlateral.grad', 'q0.grad')


def route_grads(plan, k, x, ql, q0, nsub, gauges, W, Gf, use_gauges, rows=None, rows_per_window=None, need_kx=True, need_ql=True):
    """(gauge discharge, q_final, dL/dk, dL/dx, dL/dql, dL/dq0) of L = sum(W discharge[:, gauges]) + sum(Gf q_final): through gauges=
    (use_gauges) or through the dense call and an indexed view of its discharge.  W None: a loss on q_final alone."""
    kt, xt = torch.tensor(k, requires_grad=need_kx), torch.tensor(x, requires_grad=need_kx)
    qlt = None if ql is None else torch.tensor(ql, device=DEV, requires_grad=need_ql)
    q0t = torch.tensor(q0, device=DEV, requires_grad=True)
    kw = dict(rows=rows, rows_per_window=rows_per_window)
    if use_gauges:
        d, qf = rr.grad.rapid_route(plan, q0t, qlt, kt, xt, DT_RUNOFF / nsub, DT_RUNOFF, gauges=gauges, **kw)
    else:
        d, qf = rr.grad.rapid_route(plan, q0t, qlt, kt, xt, DT_RUNOFF / nsub, DT_RUNOFF, **kw)
        d = d[:, torch.as_tensor(np.asarray(gauges), dtype=torch.int64, device=DEV)]
    L = (qf * torch.tensor(Gf, device=DEV)).sum()
    if W is not None:
        L = L + (d * torch.tensor(W, device=DEV)).sum()
    L.backward()
    host = lambda t: None if t is None or t.grad is None else t.grad.cpu().numpy()      # noqa: E731
    return d.detach().cpu().numpy(), qf.detach().cpu().numpy(), host(kt), host(xt), host(qlt), host(q0t)


def assert_paths_equal(down, k, x, ql, q0, nsub, gauges, W, Gf, what, **kw):
    """Both paths on one plan; every output np.array_equal.  Returns the gauge path's outputs."""
    plan = make_plan(down)
    got = route_grads(plan, k, x, ql, q0, nsub, gauges, W, Gf, True, **kw)
    want = route_grads(plan, k, x, ql, q0, nsub, gauges, W, Gf, False, **kw)
    for g, w, name in zip(got, want, NAMES):
        assert (g is None) == (w is None), f'{what}: {name}'
        if g is not None:
            assert g.shape == w.shape and np.array_equal(g, w), f'{what}: {name}'
    return got


def scrambled_gauges(down):
    """Seven gauges, not ascending: params index n - 1, an interior confluence, index 0, a headwater, an outlet and two more reaches
    (where index 0 or n - 1 is the only reach of a kind, it stands for that kind and another reach fills the place)."""
    n = down.shape[0]
    n_up = np.bincount(down[down >= 0], minlength=n)
    picked = [n - 1]

    def pick(candidates):
        free = [int(c) for c in candidates if c not in picked and c != 0]
        picked.append(free[0] if free else next(c for c in range(n // 2, n) if c not in picked))

    pick(np.flatnonzero((n_up >= 2) & (down >= 0)))
    picked.append(0)
    pick(np.flatnonzero(n_up == 0))
    pick(np.flatnonzero(down < 0))
    pick(range(n // 3, n))
    pick(range(n // 7, n))
    g = np.array(picked)
    assert np.unique(g).size == 7 and (np.diff(g) < 0).any() and (np.diff(g) > 0).any()
    assert ((n_up[g] >= 2) & (down[g] >= 0)).any() and (n_up[g] == 0).any() and (down[g] < 0).any()
    return g


# ---- 1. equal to the dense path ----

@pytest.mark.parametrize('nsub', [1, 2, 3])
def test_equal_to_dense_path(nsub):
    n, T = 500, 30
    down, k, x = cpu.network('forest', n, seed=8)
    ql, q0, G, Gf = inputs(n, T, 40 + nsub, low=-1.5)      # negative lateral inflow: some discharges clamp
    gauges = scrambled_gauges(down)
    d_g, *_ = assert_paths_equal(down, k, x, ql, q0, nsub, gauges, G[:, :7].copy(), Gf, f'forest nsub={nsub}')
    assert (d_g <= 0).any() and (d_g > 0).any()      # the clamp mask passes and blocks gradient within the gauge block


# ---- 2. all reaches as gauges ----

def test_all_reaches_reversed():
    n, T, nsub = 500, 30, 2
    down, k, x = cpu.network('forest', n, seed=8)
    ql, q0, G, Gf = inputs(n, T, 51, low=-1.5)
    rev = np.arange(n)[::-1].copy()
    got = assert_paths_equal(down, k, x, ql, q0, nsub, rev, G, Gf, 'G = n reversed')
    # and against the dense call proper, its columns reversed back
    plan = make_plan(down)
    kt, xt = torch.tensor(k, requires_grad=True), torch.tensor(x, requires_grad=True)
    qlt, q0t = torch.tensor(ql, device=DEV, requires_grad=True), torch.tensor(q0, device=DEV, requires_grad=True)
    d, qf = rr.grad.rapid_route(plan, q0t, qlt, kt, xt, DT_RUNOFF / nsub, DT_RUNOFF)
    ((d * torch.tensor(G[:, ::-1].copy(), device=DEV)).sum() + (qf * torch.tensor(Gf, device=DEV)).sum()).backward()
    want = (d.detach().cpu().numpy()[:, ::-1], qf.detach().cpu().numpy(), kt.grad.numpy(), xt.grad.numpy(), qlt.grad.cpu().numpy(),
            q0t.grad.cpu().numpy())
    for g, w, name in zip(got, want, NAMES):
        assert np.array_equal(g, w), name


# ---- 3. minimal shapes ----

def test_one_reach_one_row_one_gauge():
    down, k, x = cpu.network('postorder', 1, seed=5)
    ql, q0, G, Gf = inputs(1, 1, 52, low=0.5)
    assert_paths_equal(down, k, x, ql, q0, 1, np.array([0]), G, Gf, 'n = T = G = 1')


def test_chain_four_substeps():
    n, T, nsub = 40, 10, 4
    down, k, x = cpu.network('chain', n, seed=6)
    ql, q0, G, Gf = inputs(n, T, 53, low=-1.5)
    gauges = np.array([39, 0, 17, 18, 5])
    d_g, *_ = assert_paths_equal(down, k, x, ql, q0, nsub, gauges, G[:, :5].copy(), Gf, 'chain nsub=4')
    assert (d_g <= 0).any() and (d_g > 0).any()


# ---- 4. channel-only routing; only q0 requires grad ----

def test_channel_only():
    n, T, nsub = 120, 20, 2
    down, k, x = cpu.network('forest', n, seed=9)
    _, q0, G, Gf = inputs(n, T, 54)
    gauges = scrambled_gauges(down)
    got = assert_paths_equal(down, k, x, None, q0, nsub, gauges, G[:, :7].copy(), Gf, 'channel-only', rows=T)
    assert got[4] is None and got[2] is not None


def test_only_q0_requires_grad():
    # no coefficient gradient is asked for: grad_coef is NULL and no replay runs
    n, T, nsub = 120, 20, 2
    down, k, x = cpu.network('forest', n, seed=9)
    ql, q0, G, Gf = inputs(n, T, 55, low=-1.5)
    gauges = scrambled_gauges(down)
    got = assert_paths_equal(down, k, x, ql, q0, nsub, gauges, G[:, :7].copy(), Gf, 'q0 only', need_kx=False, need_ql=False)
    assert got[2] is None and got[3] is None and got[4] is None and np.abs(got[5]).max() > 0
    # a loss on q_final alone: no discharge gradient reaches the adjoint (discharge_g and grad_out_g are both NULL)
    assert_paths_equal(down, k, x, ql, q0, nsub, gauges, None, Gf, 'q_final only')


# ---- 5. against independent truth ----

@pytest.mark.parametrize('kind,n,T,nsub,low', [('tree', 300, 12, 2, -0.5), ('forest', 500, 8, 3, 0.0)])
def test_gradients_match_restatement(kind, n, T, nsub, low):
    down, k, x = cpu.network(kind, n, seed=n + T)
    ql, q0, G, Gf = inputs(n, T, n + 3, low=low)
    gauges = scrambled_gauges(down)
    W = G[:, :7].copy()
    full = np.zeros((T, n))
    full[:, gauges] = W      # the cotangent scattered to full width
    _, _, gk, gx, gql, gq0 = route_grads(make_plan(down), k, x, ql, q0, nsub, gauges, W, Gf, True)
    _, wk, wx, wql, wq0 = cpu.dense_loss_grads(down, k, x, ql, q0, DT_RUNOFF / nsub, DT_RUNOFF, full, Gf)
    for got, want, what in ((gk, wk, 'k'), (gx, wx, 'x'), (gql, wql, 'qlateral'), (gq0, wq0, 'q0')):
        assert_grad(got, want, f'{kind} n={n}: d/d{what}')


# ---- 6. windows ----

def test_windows_equal_one_call():
    n, T, nsub = 500, 30, 2
    down, k, x = cpu.network('forest', n, seed=8)
    ql, q0, G, Gf = inputs(n, T, 6)
    gauges = scrambled_gauges(down)
    plan = make_plan(down)
    one = route_grads(plan, k, x, ql, q0, nsub, gauges, G[:, :7].copy(), Gf, True)
    win = route_grads(plan, k, x, ql, q0, nsub, gauges, G[:, :7].copy(), Gf, True, rows_per_window=7)
    for a, b, what in zip(win, one, NAMES):
        assert_grad(a, b, f'windows: {what}', rtol=1e-12)


# ---- 7. batch ----

def batch_grads(plan, k, x, ql, q0, nsub, gauges, W, Gf, **kw):
    kt, xt = torch.tensor(k, requires_grad=True), torch.tensor(x, requires_grad=True)
    qlt, q0t = torch.tensor(ql, device=DEV, requires_grad=True), torch.tensor(q0, device=DEV, requires_grad=True)
    d, qf = rr.grad.rapid_route_batch(plan, q0t, qlt, kt, xt, DT_RUNOFF / nsub, DT_RUNOFF, gauges=gauges, **kw)
    ((d * torch.tensor(W, device=DEV)).sum() + (qf * torch.tensor(Gf, device=DEV)).sum()).backward()
    return d.detach().cpu().numpy(), qf.detach().cpu().numpy(), kt.grad.numpy(), xt.grad.numpy(), qlt.grad.cpu().numpy(), q0t.grad.cpu().numpy()


@pytest.mark.parametrize('shared_q0', [False, True])
def test_batch_members_match_single_gauge_calls(shared_q0):
    n, T, nsub, B = 300, 16, 2, 3
    down, k, x = cpu.network('forest', n, seed=12)
    gauges = scrambled_gauges(down)
    rng = np.random.default_rng(60)
    ql = rng.uniform(-1.5, 2.0, (B, T, n)) * DT_RUNOFF
    q0 = rng.uniform(0.0, 3.0, n if shared_q0 else (B, n))
    W, Gf = rng.standard_normal((B, T, 7)), rng.standard_normal((B, n))
    plan = make_plan(down)
    d, qf, gk, gx, gql, gq0 = batch_grads(plan, k, x, ql, q0, nsub, gauges, W, Gf, members_per_sweep=2)      # groups of 2 and 1
    assert d.shape == (B, T, 7) and qf.shape == (B, n)
    one = [route_grads(plan, k, x, ql[m], q0 if shared_q0 else q0[m], nsub, gauges, W[m], Gf[m], True) for m in range(B)]
    for m in range(B):
        assert np.array_equal(d[m], one[m][0]) and np.array_equal(qf[m], one[m][1]), f'member {m}: forward'
        assert np.array_equal(gql[m], one[m][4]), f'member {m}: qlateral.grad'
        if not shared_q0:
            assert np.array_equal(gq0[m], one[m][5]), f'member {m}: q0.grad'
    total = lambda j: one[0][j] + one[1][j] + one[2][j]      # noqa: E731  (in member order)
    assert_grad(gk, total(2), 'k.grad against the member-ordered sum', rtol=1e-12)
    assert_grad(gx, total(3), 'x.grad against the member-ordered sum', rtol=1e-12)
    if shared_q0:      # one q0 for all: autograd adds the members' rows, in an order of its own
        assert_grad(gq0, total(5), 'shared q0.grad against the sum over the members', rtol=1e-12)


def test_batch_of_one_is_the_single_call():
    n, T, nsub = 300, 16, 3
    down, k, x = cpu.network('forest', n, seed=12)
    gauges = scrambled_gauges(down)
    ql, q0, G, Gf = inputs(n, T, 61, low=-1.5)
    W = G[:, :7].copy()
    plan = make_plan(down)
    got = batch_grads(plan, k, x, ql[None], q0[None], nsub, gauges, W[None], Gf[None])
    want = route_grads(plan, k, x, ql, q0, nsub, gauges, W, Gf, True)
    for g, w, name in zip(got, want, NAMES):
        g = g[0] if name in ('gauge discharge', 'q_final', 'qlateral.grad', 'q0.grad') else g
        assert np.array_equal(g, w), name


# ---- 8. determinism ----

def test_two_backward_passes_bit_identical():
    n, T, nsub = 5000, 40, 1
    net = synth.synth_network(n, seed=12)
    ql, q0, G, Gf = inputs(n, T, 13)
    gauges = np.random.default_rng(14).permutation(n)[:50]
    plan = make_plan(net.down_index)
    a = route_grads(plan, net.k, net.x, ql, q0, nsub, gauges, G[:, :50].copy(), Gf, True)
    b = route_grads(plan, net.k, net.x, ql, q0, nsub, gauges, G[:, :50].copy(), Gf, True)
    for u, v in zip(a, b):
        assert np.array_equal(u, v)


# ---- 9. work memory and refusals ----

def test_work_memory_and_refusals():
    n, T, G = 50, 6, 4
    down, k, x = cpu.network('tree', n, seed=4)
    indptr, indices = cpu.csc_from_down(down)
    c1, c2, c3 = oracle.muskingum_coefficients(k, x, DT_RUNOFF)
    c4 = (c1 + c2) / DT_RUNOFF
    plan = Plan(indptr, indices)
    plan.set_coeffs(-c1[indices], c2, c3, c4)
    for members, nsub in ((1, 1), (1, 3), (3, 2)):
        lean = plan.rapid_adjoint_gauges_work_bytes(members, G, T, nsub, False)
        assert lean <= plan.rapid_adjoint_batch_work_bytes(members, T, nsub) - 8 * n * T * members
        assert plan.rapid_adjoint_gauges_work_bytes(members, G, T, nsub, True) == lean + 8 * n * T * members
    buf = lambda count: DeviceBuffer(max(count, 1) * 8)     # noqa: E731
    q0, ql, dis, gout, coef, gq0, gql = buf(n), buf(T * n), buf(T * G), buf(T * G), buf(4 * n), buf(n), buf(T * n)
    for b, a in ((q0, np.ones(n)), (ql, np.ones(T * n)), (dis, np.ones(T * G)), (gout, np.ones(T * G))):
        b.upload(a)
    gauges = torch.tensor([7, 0, n - 1, 3], dtype=torch.int32, device=DEV)
    need = plan.rapid_adjoint_gauges_work_bytes(1, G, T, 1, False)
    need_rows = plan.rapid_adjoint_gauges_work_bytes(1, G, T, 1, True)
    work = DeviceBuffer(need_rows)

    def code(*args):
        with pytest.raises(_lib.RRError) as e:
            plan.rapid_adjoint_gauges_dev(*args)
        return e.value.code, e.value.message

    ok = (1, G, gauges, q0, n, ql, T, T * n, dis, gout, T * G, None, None, gq0, coef, work, need, T, 1)

    def but(**kw):
        names = ('members', 'n_gauges', 'gauges', 'q0', 'q0_pitch', 'lateral', 'lat_rows', 'lat_pitch', 'discharge_g', 'grad_out_g',
                 'gauge_pitch', 'grad_qfinal', 'grad_lateral', 'grad_q0', 'grad_coef', 'work', 'work_bytes', 'T', 'nsub')
        assert set(kw) <= set(names)
        return tuple(kw.get(name, v) for name, v in zip(names, ok))

    plan.rapid_adjoint_gauges_dev(*ok)                                                     # accepted
    plan.rapid_adjoint_gauges_dev(*but(gauge_pitch=0))                                     # one member: any gauge pitch
    c, msg = code(*but(work_bytes=need - 1))
    assert c == _lib.RR_E_INVALID and str(need) in msg                                     # one byte short
    c, msg = code(*but(grad_lateral=gql))                                                  # grad_lateral on memory sized without it
    assert c == _lib.RR_E_INVALID and str(need_rows) in msg
    plan.rapid_adjoint_gauges_dev(*but(grad_lateral=gql, work_bytes=need_rows))            # and on memory sized with it
    assert code(*but(n_gauges=0))[0] == _lib.RR_E_INVALID
    assert code(*but(n_gauges=n + 1))[0] == _lib.RR_E_INVALID
    assert code(*but(gauges=None))[0] == _lib.RR_E_INVALID
    assert code(*but(grad_out_g=None))[0] == _lib.RR_E_INVALID                             # discharge_g without grad_out_g
    assert code(*but(discharge_g=None))[0] == _lib.RR_E_INVALID                            # and the reverse
    two = DeviceBuffer(plan.rapid_adjoint_gauges_work_bytes(2, G, T, 1, False))
    assert code(*but(members=2, q0_pitch=0, lat_pitch=0, lateral=None, gauge_pitch=T * G - 1, work=two, work_bytes=two.nbytes))[0] \
        == _lib.RR_E_INVALID                                                               # short gauge pitch
    assert code(*but(members=0))[0] == _lib.RR_E_INVALID
    assert code(*but(q0=None))[0] == _lib.RR_E_INVALID                                     # the batch call's: q0 for the coefficients
    assert code(*but(lat_rows=T - 1))[0] == _lib.RR_E_INVALID
    assert code(*but(T=0))[0] == _lib.RR_E_INVALID
    for bad in (0, n + 1):
        with pytest.raises(_lib.RRError) as e:
            plan.rapid_adjoint_gauges_work_bytes(1, bad, T, 1, False)
        assert e.value.code == _lib.RR_E_INVALID
    _lib.lib().rr_dev_synchronize(0)
    # per-edge weights: one tributary weighted differently
    w = -c1[indices]
    e = int(np.flatnonzero(np.bincount(indices, minlength=n)[indices] >= 2)[0])      # an edge into a confluence
    w[e] *= 1.5
    plan.set_coeffs(w, c2, c3, c4)
    assert code(*ok)[0] == _lib.RR_E_UNSUPPORTED
    plan.set_coeffs(-c1[indices], c2, c3, c4)
    plan.rapid_adjoint_gauges_dev(*ok)                                                     # accepted again
    _lib.lib().rr_dev_synchronize(0)
    # a plan with boundary reaches
    plan.set_boundary([], [int(np.flatnonzero(down < 0)[0])])
    assert code(*ok)[0] == _lib.RR_E_UNSUPPORTED


# ---- 10. with the scores ----

def test_chains_with_scores():
    n, T, nsub = 500, 30, 2
    down, k, x = cpu.network('forest', n, seed=8)
    ql, q0, _, _ = inputs(n, T, 70, low=0.2)
    gauges = scrambled_gauges(down)
    rng = np.random.default_rng(71)
    obs = torch.tensor(rng.uniform(0.5, 3.0, (T, 7)), device=DEV)      # no constant column
    plan = make_plan(down)
    grads = []
    for use_gauges in (True, False):
        kt, xt = torch.tensor(k, requires_grad=True), torch.tensor(x, requires_grad=True)
        args = (plan, torch.tensor(q0, device=DEV), torch.tensor(ql, device=DEV), kt, xt, DT_RUNOFF / nsub, DT_RUNOFF)
        if use_gauges:
            d, _ = rr.grad.rapid_route(*args, gauges=gauges)
            kge = rr.grad.scores(obs, d)['kge2012']
        else:
            d, _ = rr.grad.rapid_route(*args)
            kge = rr.grad.scores(obs, d, columns=gauges)['kge2012']
        assert bool(torch.isfinite(kge).all())
        kge.sum().backward()
        grads.append((kge.detach().cpu().numpy(), kt.grad.numpy(), xt.grad.numpy()))
    (kge_g, gk, gx), (kge_d, wk, wx) = grads
    assert np.array_equal(kge_g, kge_d)
    assert np.isfinite(gk).all() and np.isfinite(gx).all() and np.isfinite(wk).all() and np.isfinite(wx).all()
    assert np.abs(wk).max() > 0
    assert_grad(gk, wk, 'scores: k.grad')
    assert_grad(gx, wx, 'scores: x.grad')


# ---- 11. peak memory ----

def test_backward_allocates_no_full_width_cotangent():
    n, T, G, nsub = 20_000, 64, 8, 1
    net = synth.synth_network(n, seed=15)
    ql, q0, W, _ = inputs(n, T, 16)
    gauges = np.random.default_rng(17).permutation(n)[:G]
    plan = make_plan(net.down_index)
    qlt, q0t, Wt = torch.tensor(ql, device=DEV), torch.tensor(q0, device=DEV), torch.tensor(W[:, :G].copy(), device=DEV)
    gauges_t = torch.as_tensor(gauges, device=DEV)
    rise = {}
    for use_gauges in (True, False):
        kt, xt = torch.tensor(net.k, requires_grad=True), torch.tensor(net.x, requires_grad=True)
        if use_gauges:
            d, _ = rr.grad.rapid_route(plan, q0t, qlt, kt, xt, DT_RUNOFF / nsub, DT_RUNOFF, gauges=gauges)
        else:
            d, _ = rr.grad.rapid_route(plan, q0t, qlt, kt, xt, DT_RUNOFF / nsub, DT_RUNOFF)
            d = d[:, gauges_t]
        loss = (d * Wt).sum()
        torch.cuda.synchronize(DEV)
        torch.cuda.reset_peak_memory_stats(DEV)
        before = torch.cuda.memory_allocated(DEV)
        loss.backward()
        torch.cuda.synchronize(DEV)
        rise[use_gauges] = torch.cuda.max_memory_allocated(DEV) - before
        del d, loss, kt, xt
    bound = 8 * n * T + plan.rapid_adjoint_gauges_work_bytes(1, G, T, nsub, False)
    print(f'peak rise of backward: gauges {rise[True]} bytes, dense {rise[False]} bytes, bound {bound} bytes')
    assert rise[True] < bound
    assert not rise[False] < bound      # the dense path holds a (T, n) cotangent beside its larger work memory: the bound tells them apart
