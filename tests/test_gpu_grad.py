"""rr.grad on the GPU (rr_rapid_adjoint_dev: k_tick into the state tape, k_adj_tick, k_adj_reduce / k_adj_merge, k_adj_rows):
the forward is the production route call, bit for bit; every gradient (k, x, qlateral, q0, through the discharge and through
q_final) agrees with torch autograd through the pure-torch restatement of tests/test_grad.py (checked there against the
oracle) to rtol 1e-9; gradcheck; windows against one call; repeat runs bit-identical; a 100k-reach directional difference;
and the ABI's refusals.  The restatement is a dense solve per sub-step, so these cases stop at 2,000 reaches, where the reduction has one
sub-step per range: the sizes beyond it, and every element at its own scale, are tests/test_gpu_grad_per_reach.py's (DESIGN.md
section 2c)."""
import numpy as np
import pytest
import torch

import river_route_amd as rr
import test_grad as cpu
from oracle import oracle
from river_route_amd import _lib, synth
from river_route_amd.engine import DeviceBuffer, Plan

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
KNOBS = ('RR_WAVE', 'RR_WAVE_K', 'RR_TILE_BLOCK', 'RR_TILE_LEAN', 'RR_UH_PAIRS', 'RR_DIRECT')


@pytest.fixture(autouse=True)
def _default_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def make_plan(down):
    indptr, indices = cpu.csc_from_down(down)
    return Plan(indptr, indices)


def inputs(n, T, seed, low=0.0):
    rng = np.random.default_rng(seed)
    ql = rng.uniform(low, 2.0, (T, n)) * 3600.0
    q0 = rng.uniform(0.0, 3.0, n)
    return ql, q0, rng.standard_normal((T, n)), rng.standard_normal(n)


def gpu_loss_grads(plan, k, x, ql, q0, dt, dt_runoff, G, Gf, rows=None, rows_per_window=None):
    kt, xt = torch.tensor(k, requires_grad=True), torch.tensor(x, requires_grad=True)
    qlt = None if ql is None else torch.tensor(ql, device=DEV, requires_grad=True)
    q0t = torch.tensor(q0, device=DEV, requires_grad=True)
    d, qf = rr.grad.rapid_route(plan, q0t, qlt, kt, xt, dt, dt_runoff, rows_per_window=rows_per_window, rows=rows)
    L = (d * torch.tensor(G, device=DEV)).sum() + (qf * torch.tensor(Gf, device=DEV)).sum()
    L.backward()
    return (d.detach().cpu().numpy(), qf.detach().cpu().numpy(), kt.grad.numpy(), xt.grad.numpy(),
            None if qlt is None else qlt.grad.cpu().numpy(), q0t.grad.cpu().numpy())


def assert_grad(got, want, what, rtol=1e-9):
    scale = max(float(np.abs(want).max()), 1e-300)
    np.testing.assert_allclose(got, want, rtol=rtol, atol=rtol * scale, err_msg=what)


@pytest.mark.parametrize('order,knob', [('random', None), ('random', 'tick'), ('postorder', None)])
def test_forward_bit_equal_to_plan_rapid_route(monkeypatch, order, knob):
    if knob == 'tick':
        monkeypatch.setenv('RR_WAVE', '0')
    n, T, nsub, dt_runoff = 3000, 64, 1, 3600.0
    net = synth.synth_network(n, seed=5, order=order)
    plan = make_plan(net.down_index)
    ql, q0, _, _ = inputs(n, T, 1)
    c1, c2, c3 = oracle.muskingum_coefficients(net.k, net.x, dt_runoff / nsub)
    d, qf = rr.grad.rapid_route(plan, torch.tensor(q0, device=DEV), torch.tensor(ql, device=DEV), torch.tensor(net.k),
                                torch.tensor(net.x), dt_runoff / nsub, dt_runoff)
    ref = make_plan(net.down_index)
    _, indices = cpu.csc_from_down(net.down_index)
    ref.set_coeffs(-c1[indices], c2, c3, (c1 + c2) / dt_runoff)
    q, want = q0.copy(), np.zeros((T, n))
    ref.rapid_route(q, ql, want, nsub)
    assert np.array_equal(d.cpu().numpy(), want)
    assert np.array_equal(qf.cpu().numpy(), q)


CASES = [('tree', 1, 1, 1), ('tree', 2, 3, 2), ('tree', 50, 40, 1), ('postorder', 200, 24, 2), ('forest', 300, 16, 4),
         ('chain', 120, 30, 1), ('tree', 150, 300, 1), ('forest', 250, 12, 4), ('tree', 2000, 3, 1)]


@pytest.mark.parametrize('kind,n,T,nsub', CASES)
def test_gradients_match_restatement(kind, n, T, nsub):
    dt_runoff = 3600.0
    dt = dt_runoff / nsub
    down, k, x = cpu.network(kind, n, seed=n + T + nsub)
    ql, q0, G, Gf = inputs(n, T, n + 17)
    plan = make_plan(down)
    d, qf, gk, gx, gql, gq0 = gpu_loss_grads(plan, k, x, ql, q0, dt, dt_runoff, G, Gf)
    _, wk, wx, wql, wq0 = cpu.dense_loss_grads(down, k, x, ql, q0, dt, dt_runoff, G, Gf)
    for got, want, what in ((gk, wk, 'k'), (gx, wx, 'x'), (gql, wql, 'qlateral'), (gq0, wq0, 'q0')):
        assert_grad(got, want, f'{kind} n={n} T={T} nsub={nsub}: d/d{what}')


def test_channel_only_and_final_state_only():
    n, T, nsub, dt_runoff = 120, 20, 2, 3600.0
    down, k, x = cpu.network('forest', n, seed=9)
    _, q0, G, Gf = inputs(n, T, 4)
    plan = make_plan(down)
    _, _, gk, gx, _, gq0 = gpu_loss_grads(plan, k, x, None, q0, dt_runoff / nsub, dt_runoff, G, Gf, rows=T)
    _, wk, wx, _, wq0 = cpu.dense_loss_grads(down, k, x, None, q0, dt_runoff / nsub, dt_runoff, G, Gf)
    for got, want, what in ((gk, wk, 'k'), (gx, wx, 'x'), (gq0, wq0, 'q0')):
        assert_grad(got, want, f'channel-only d/d{what}')
    # a loss of q_final alone: no discharge gradient reaches the adjoint
    ql, q0, _, _ = inputs(n, T, 5)
    kt = torch.tensor(k, requires_grad=True)
    qlt = torch.tensor(ql, device=DEV, requires_grad=True)
    _, qf = rr.grad.rapid_route(plan, torch.tensor(q0, device=DEV), qlt, kt, torch.tensor(x), dt_runoff / nsub, dt_runoff)
    (qf * torch.tensor(Gf, device=DEV)).sum().backward()
    _, wk, _, wql, _ = cpu.dense_loss_grads(down, k, x, ql, q0, dt_runoff / nsub, dt_runoff, np.zeros((T, n)), Gf)
    assert_grad(kt.grad.numpy(), wk, 'q_final only: d/dk')
    assert_grad(qlt.grad.cpu().numpy(), wql, 'q_final only: d/dql')


def test_clamp_active_and_negative_c3():
    n, T, nsub, dt_runoff = 200, 24, 1, 3600.0
    down, k, x = cpu.network('tree', n, seed=21)
    k = k.copy()
    k[::3] = 300.0             # dt / k = 12 > 2 (1 - x): c3 < 0 on every third reach
    ql, q0, G, Gf = inputs(n, T, 22, low=-1.5)
    c3 = oracle.muskingum_coefficients(k, x, dt_runoff / nsub)[2]
    assert (c3 < 0).any()
    plan = make_plan(down)
    d, _, gk, gx, gql, gq0 = gpu_loss_grads(plan, k, x, ql, q0, dt_runoff / nsub, dt_runoff, G, Gf)
    assert (d == 0).mean() > 0.05          # the clamp is active for a good share of the outputs
    _, wk, wx, wql, wq0 = cpu.dense_loss_grads(down, k, x, ql, q0, dt_runoff / nsub, dt_runoff, G, Gf)
    for got, want, what in ((gk, wk, 'k'), (gx, wx, 'x'), (gql, wql, 'qlateral'), (gq0, wq0, 'q0')):
        assert_grad(got, want, f'clamp / negative c3: d/d{what}')


def test_gradcheck():
    n, T, nsub, dt_runoff = 20, 8, 2, 3600.0
    down, k, x = cpu.network('tree', n, seed=2)
    ql, q0, _, _ = inputs(n, T, 3, low=0.3)
    plan = make_plan(down)

    def f(q0_, ql_, k_, x_):
        return rr.grad.rapid_route(plan, q0_, ql_, k_, x_, dt_runoff / nsub, dt_runoff)

    args = (torch.tensor(q0, device=DEV, requires_grad=True), torch.tensor(ql, device=DEV, requires_grad=True),
            torch.tensor(k, requires_grad=True), torch.tensor(x, requires_grad=True))
    assert torch.autograd.gradcheck(f, args, eps=1e-6, atol=1e-6, rtol=1e-5)


def test_windows_equal_one_call():
    n, T, nsub, dt_runoff = 500, 30, 2, 3600.0
    down, k, x = cpu.network('forest', n, seed=8)
    ql, q0, G, Gf = inputs(n, T, 6)
    plan = make_plan(down)
    one = gpu_loss_grads(plan, k, x, ql, q0, dt_runoff / nsub, dt_runoff, G, Gf)
    win = gpu_loss_grads(plan, k, x, ql, q0, dt_runoff / nsub, dt_runoff, G, Gf, rows_per_window=7)
    for a, b, what in zip(win, one, ('discharge', 'q_final', 'k', 'x', 'qlateral', 'q0')):
        assert_grad(a, b, f'windows: {what}', rtol=1e-12)


def test_two_backward_passes_bit_identical():
    n, T, nsub, dt_runoff = 5000, 40, 1, 3600.0
    net = synth.synth_network(n, seed=12)
    ql, q0, G, Gf = inputs(n, T, 13)
    plan = make_plan(net.down_index)
    a = gpu_loss_grads(plan, net.k, net.x, ql, q0, dt_runoff / nsub, dt_runoff, G, Gf)
    b = gpu_loss_grads(plan, net.k, net.x, ql, q0, dt_runoff / nsub, dt_runoff, G, Gf)
    for u, v in zip(a, b):
        assert np.array_equal(u, v)


def test_100k_reaches_directional_difference():
    # dt = 900 s <= every k and 2 x < dt / k: c1, c2, c3 > 0, so with positive inflows no output meets the clamp and the differences
    # cross no kink
    n, T, nsub, dt_runoff = 100_000, 200, 4, 3600.0
    dt = dt_runoff / nsub
    net = synth.synth_network(n, seed=31)
    k, x = net.k, 0.05 + 0.01 * synth.u01(34, np.arange(n))
    c1, c2, c3 = oracle.muskingum_coefficients(k, x, dt)
    assert (c1 > 0).all() and (c2 > 0).all() and (c3 > 0).all()
    ql, q0, G, _ = inputs(n, T, 32, low=0.2)
    plan = make_plan(net.down_index)
    Gd = torch.tensor(G, device=DEV)
    kt = torch.tensor(k, requires_grad=True)
    qlt = torch.tensor(ql, device=DEV, requires_grad=True)
    q0t = torch.tensor(q0, device=DEV)
    d, _ = rr.grad.rapid_route(plan, q0t, qlt, kt, torch.tensor(x), dt, dt_runoff)
    assert bool((d > 0).all())
    (d * Gd).sum().backward()
    rng = np.random.default_rng(33)
    vk = torch.tensor(k * rng.uniform(-1.0, 1.0, n))
    vq = torch.tensor(ql * rng.uniform(-1.0, 1.0, (T, n)), device=DEV)

    def loss(k_, ql_):
        with torch.no_grad():
            d_, _ = rr.grad.rapid_route(plan, q0t, ql_, k_, torch.tensor(x), dt, dt_runoff)
            return float((d_ * Gd).sum())

    h = 1e-5
    kk = torch.tensor(k)
    fd = (loss(kk + h * vk, qlt.detach()) - loss(kk - h * vk, qlt.detach())) / (2 * h)
    an = float((kt.grad * vk).sum())
    assert abs(fd - an) <= 1e-5 * abs(an), (fd, an)
    h = 1e-2      # the loss is linear in qlateral here: a long step keeps the round-off of the two sums small
    fd = (loss(kk, qlt.detach() + h * vq) - loss(kk, qlt.detach() - h * vq)) / (2 * h)
    an = float((qlt.grad * vq).sum())
    assert abs(fd - an) <= 1e-6 * abs(an), (fd, an)


def test_abi_refusals():
    n, T = 50, 6
    down, k, x = cpu.network('tree', n, seed=4)
    indptr, indices = cpu.csc_from_down(down)
    c1, c2, c3 = oracle.muskingum_coefficients(k, x, 3600.0)
    c4 = (c1 + c2) / 3600.0
    plan = Plan(indptr, indices)
    buf = lambda count: DeviceBuffer(max(count, 1) * 8)     # noqa: E731
    q0, ql, dis, G, coef, gq0, gql = buf(n), buf(T * n), buf(T * n), buf(T * n), buf(4 * n), buf(n), buf(T * n)

    def code(*args):
        with pytest.raises(_lib.RRError) as e:
            plan.rapid_adjoint_dev(*args)
        return e.value.code, e.value.message

    assert code(q0, ql, T, dis, G, None, gql, gq0, coef, None, 0, T, 1)[0] == _lib.RR_E_STATE     # before set_coeffs
    plan.set_coeffs(-c1[indices], c2, c3, c4)
    need = plan.rapid_adjoint_work_bytes(T, 1)
    work = DeviceBuffer(need)
    assert need >= 8 * n * (2 * T + 2 * T + 2 * plan.depth)
    assert code(q0, ql, T, dis, G, None, gql, gq0, coef, work, need - 8, T, 1)[0] == _lib.RR_E_INVALID
    c, msg = code(q0, ql, T, dis, G, None, gql, gq0, coef, None, 0, T, 1)
    assert c == _lib.RR_E_INVALID and str(need) in msg
    assert code(None, ql, T, dis, G, None, gql, gq0, coef, work, need, T, 1)[0] == _lib.RR_E_INVALID      # q0 for the coefficients
    assert code(q0, ql, T - 1, dis, G, None, gql, gq0, coef, work, need, T, 1)[0] == _lib.RR_E_INVALID    # short lateral rows
    assert code(q0, ql, T, None, G, None, gql, gq0, coef, work, need, T, 1)[0] == _lib.RR_E_INVALID       # grad_out without discharge
    assert code(q0, None, 0, dis, G, None, gql, gq0, coef, work, need, T, 1)[0] == _lib.RR_E_INVALID      # grad_lateral, channel-only
    assert code(q0, ql, T, dis, G, None, gql, gq0, coef, work, need, 0, 1)[0] == _lib.RR_E_INVALID        # T = 0
    assert code(q0, ql, T, dis, G, None, gql, gq0, coef, work, need, T, 0)[0] == _lib.RR_E_INVALID        # nsub = 0
    with pytest.raises(_lib.RRError) as e:
        plan.rapid_adjoint_work_bytes(0, 1)
    assert e.value.code == _lib.RR_E_INVALID
    # per-edge weights: one tributary weighted differently
    w = -c1[indices]
    e = int(np.flatnonzero(np.bincount(indices, minlength=n)[indices] >= 2)[0])      # an edge into a confluence
    w[e] *= 1.5
    plan.set_coeffs(w, c2, c3, c4)
    assert code(q0, ql, T, dis, G, None, gql, gq0, coef, work, need, T, 1)[0] == _lib.RR_E_UNSUPPORTED
    plan.set_coeffs(-c1[indices], c2, c3, c4)
    plan.rapid_adjoint_dev(q0, ql, T, dis, G, None, gql, gq0, coef, work, need, T, 1)     # accepted again
    _lib.lib().rr_dev_synchronize(0)
    # a plan with boundary reaches
    outlet = int(np.flatnonzero(down < 0)[0])
    plan.set_boundary([], [outlet])
    assert code(q0, ql, T, dis, G, None, gql, gq0, coef, work, need, T, 1)[0] == _lib.RR_E_UNSUPPORTED
