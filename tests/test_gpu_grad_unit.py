"""rr.grad for UnitMuskingum on the GPU (rr_unit_adjoint_dev: k_tick_unit into the state tape, k_adj_tick_unit, k_adj_reduce_unit /
k_adj_merge_unit, k_adj_rows_unit; rr_uh_adjoint_dev: k_uh_adjoint_depth, k_uh_adjoint_kernel): the forward is the production
call, bit for bit; every gradient (k, x, lateral or depth, uh_kernel, uh_state, q_ch0, q_full0) agrees with torch autograd through
the pure-torch restatements of tests/test_grad_unit.py (checked there against the oracle) to rtol 1e-9; gradcheck; windows against
one call; repeat runs bit-identical; a 100k-reach directional difference; and the ABI's refusals.  Case for case the grid of
tests/test_gpu_grad.py; the sizes beyond the dense restatement (several sub-steps per range of the reduction, more than 65,535 rows)
and every element at its own scale are tests/test_gpu_grad_per_reach.py's."""
import numpy as np
import pytest
import torch

import river_route_amd as rr
import test_gpu_grad as gpu_grad
import test_grad as cpu
import test_grad_unit as unit
from oracle import oracle
from river_route_amd import _lib, engine, synth
from river_route_amd.engine import DeviceBuffer, Plan
from test_gpu_grad import CASES, KNOBS, make_plan

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)


@pytest.fixture(autouse=True)
def _default_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def assert_grad(got, want, what, rtol=1e-9):
    """test_gpu_grad.assert_grad (tolerance scaled by the largest wanted value), for state vectors that may be empty too."""
    assert got.shape == want.shape, what
    if want.size:
        gpu_grad.assert_grad(got, want, what, rtol=rtol)


def dev(a, grad=False):
    return torch.tensor(a, device=DEV, requires_grad=grad)


def gpu_unit_loss_grads(plan, k, x, d, dt, dt_runoff, rows_per_window=None, weights=('G', 'Gc', 'Gf')):
    """L through rr.grad.unit_route: outputs and gradients as numpy, by the names of unit.dense_unit_loss_grads."""
    kt, xt = torch.tensor(k, requires_grad=True), torch.tensor(x, requires_grad=True)
    t = {key: dev(d[key], True) for key in ('lat', 'q_ch0', 'q_full0')}
    out, qc, qf = rr.grad.unit_route(plan, t['q_ch0'], t['q_full0'], t['lat'], kt, xt, dt, dt_runoff, rows_per_window=rows_per_window)
    L = sum((v * dev(d[w])).sum() for v, w in ((out, 'G'), (qc, 'Gc'), (qf, 'Gf')) if w in weights)
    L.backward()
    z = lambda v: (torch.zeros_like(v) if v.grad is None else v.grad).cpu().numpy()      # noqa: E731
    return dict(k=z(kt), x=z(xt), lat=z(t['lat']), q_ch0=z(t['q_ch0']), q_full0=z(t['q_full0']), out=out.detach().cpu().numpy(),
                q_ch=qc.detach().cpu().numpy(), q_full=qf.detach().cpu().numpy())


def gpu_unit_muskingum_loss_grads(plan, k, x, d, dt, dt_runoff, rows_per_window=None, weights=('G', 'Gc', 'Gf', 'Gs')):
    kt, xt = torch.tensor(k, requires_grad=True), torch.tensor(x, requires_grad=True)
    t = {key: dev(d[key], True) for key in ('lat', 'q_ch0', 'q_full0', 'kernel', 'state')}
    out, qc, qf, st = rr.grad.unit_muskingum(plan, t['q_ch0'], t['q_full0'], t['lat'], t['kernel'], t['state'], kt, xt, dt, dt_runoff,
                                             rows_per_window=rows_per_window)
    L = sum((v * dev(d[w])).sum() for v, w in ((out, 'G'), (qc, 'Gc'), (qf, 'Gf'), (st, 'Gs')) if w in weights)
    L.backward()
    z = lambda v: (torch.zeros_like(v) if v.grad is None else v.grad).cpu().numpy()      # noqa: E731
    return dict(k=z(kt), x=z(xt), depth=z(t['lat']), q_ch0=z(t['q_ch0']), q_full0=z(t['q_full0']), kernel=z(t['kernel']),
                state=z(t['state']), out=out.detach().cpu().numpy(), q_ch=qc.detach().cpu().numpy(), q_full=qf.detach().cpu().numpy(),
                uh_state=st.detach().cpu().numpy())


def only(d, weights):
    """The inputs with every loss weight outside `weights` set to zero (for the restatement's side of a partial loss)."""
    return {key: (np.zeros_like(v) if key in ('G', 'Gc', 'Gf', 'Gs') and key not in weights else v) for key, v in d.items()}


ROUTE_GRADS = ('k', 'x', 'lat', 'q_ch0', 'q_full0')
FULL_GRADS = ('k', 'x', 'depth', 'kernel', 'state', 'q_ch0', 'q_full0')


@pytest.mark.parametrize('order,knob', [('random', None), ('random', 'tick'), ('postorder', None)])
def test_forward_bit_equal_to_plan_unit_route_and_uh_convolve(monkeypatch, order, knob):
    if knob == 'tick':
        monkeypatch.setenv('RR_WAVE', '0')
    n, T, nsub, n_ks, dt_runoff = 3000, 64, 1, 12, 3600.0
    net = synth.synth_network(n, seed=5, order=order)
    down = net.down_index.astype(np.int64)
    plan = make_plan(down)
    d = unit.unit_inputs(down, T, 1, n_ks=n_ks)
    ni = plan.n_inner
    # the convolution alone
    conv, st = rr.grad.uh_convolve(dev(d['kernel']), dev(d['state']), dev(d['lat']))
    state_in = dev(d['state'])
    st_ref, conv_ref = state_in.clone(), torch.empty((T, n), dtype=torch.float64, device=DEV)
    engine.uh_convolve_dev(dev(d['kernel']), st_ref, dev(d['lat']), conv_ref, T, n_ks, n)
    torch.cuda.synchronize()
    assert torch.equal(conv, conv_ref) and torch.equal(st, st_ref)
    # routing of that lateral, and the chain
    out, qc, qf = rr.grad.unit_route(plan, dev(d['q_ch0']), dev(d['q_full0']), conv, torch.tensor(net.k), torch.tensor(net.x),
                                     dt_runoff / nsub, dt_runoff)
    out2, qc2, qf2, st2 = rr.grad.unit_muskingum(plan, dev(d['q_ch0']), dev(d['q_full0']), dev(d['lat']), dev(d['kernel']), state_in,
                                                 torch.tensor(net.k), torch.tensor(net.x), dt_runoff / nsub, dt_runoff)
    assert torch.equal(state_in, dev(d['state']))          # the inputs are not modified
    c1, c2, c3 = oracle.muskingum_coefficients(net.k, net.x, dt_runoff / nsub)
    ref = make_plan(down)
    _, indices = cpu.csc_from_down(down)
    ref.set_coeffs(-c1[indices], c2, c3, None)
    b_qc, b_qf, b_conv, b_out = DeviceBuffer(max(ni, 1) * 8), DeviceBuffer(max(ni, 1) * 8), DeviceBuffer(T * n * 8), DeviceBuffer(T * n * 8)
    b_qc.upload(d['q_ch0'].copy()); b_qf.upload(d['q_full0'].copy()); b_conv.upload(conv_ref.cpu().numpy())
    ref.unit_route_dev(b_qc, b_qf, b_conv, T, b_out, T, T, nsub)
    want = b_out.download(np.float64, (T, n))
    for got in (out, out2):
        assert np.array_equal(got.cpu().numpy(), want)
    for got in (qc, qc2):
        assert np.array_equal(got.cpu().numpy(), b_qc.download(np.float64, (ni,)))
    for got in (qf, qf2):
        assert np.array_equal(got.cpu().numpy(), b_qf.download(np.float64, (ni,)))
    assert torch.equal(st2, st_ref)


@pytest.mark.parametrize('kind,n,T,nsub', CASES)
def test_route_gradients_match_restatement(kind, n, T, nsub):
    dt_runoff = 3600.0
    dt = dt_runoff / nsub
    down, k, x = cpu.network(kind, n, seed=n + T + nsub)
    d = unit.unit_inputs(down, T, n + 17)
    plan = make_plan(down)
    got = gpu_unit_loss_grads(plan, k, x, d, dt, dt_runoff)
    want = unit.dense_unit_loss_grads(down, k, x, d, dt, nsub)
    for name in ROUTE_GRADS:
        assert_grad(got[name], want[name], f'{kind} n={n} T={T} nsub={nsub}: d/d{name}')


# n_ks 1, 3, 48 and T < n_ks over the same networks
UH_CASES = [('tree', 1, 1, 1, 1), ('tree', 2, 3, 2, 3), ('tree', 50, 40, 1, 48), ('postorder', 200, 24, 2, 3), ('forest', 300, 16, 4, 48),
            ('chain', 120, 30, 1, 1), ('tree', 150, 300, 1, 3), ('forest', 250, 12, 4, 48), ('tree', 2000, 3, 1, 48)]


@pytest.mark.parametrize('kind,n,T,nsub,n_ks', UH_CASES)
def test_unit_muskingum_gradients_match_restatement(kind, n, T, nsub, n_ks):
    dt_runoff = 3600.0
    dt = dt_runoff / nsub
    down, k, x = cpu.network(kind, n, seed=n + T + nsub)
    d = unit.unit_inputs(down, T, n + 19, n_ks=n_ks)
    plan = make_plan(down)
    got = gpu_unit_muskingum_loss_grads(plan, k, x, d, dt, dt_runoff)
    want = unit.dense_unit_muskingum_loss_grads(down, k, x, d, dt, nsub)
    for name in FULL_GRADS:
        assert_grad(got[name], want[name], f'{kind} n={n} T={T} nsub={nsub} n_ks={n_ks}: d/d{name}')


@pytest.mark.parametrize('n,T,n_ks', [(300, 40, 12), (1000, 5, 48), (70, 9, 1), (1, 1, 1), (2500, 300, 3)])
def test_uh_convolve_gradients_match_restatement(n, T, n_ks):
    rng = np.random.default_rng(n + T)
    kernel, state, depth = rng.uniform(0, 1, (n_ks, n)), rng.uniform(0, 5, (n_ks, n)), rng.uniform(0, 3, (T, n))
    Gc, Gs = rng.standard_normal((T, n)), rng.standard_normal((n_ks, n))
    for use in (('c', 's'), ('c',), ('s',)):
        ts = [torch.tensor(v, requires_grad=True) for v in (kernel, state, depth)]
        gs = [dev(v, True) for v in (kernel, state, depth)]
        conv, st = unit.dense_uh_convolve(*ts)
        gconv, gst = rr.grad.uh_convolve(*gs)
        L = sum(((conv * torch.as_tensor(Gc)).sum(),) * ('c' in use) + ((st * torch.as_tensor(Gs)).sum(),) * ('s' in use))
        Lg = sum(((gconv * dev(Gc)).sum(),) * ('c' in use) + ((gst * dev(Gs)).sum(),) * ('s' in use))
        L.backward()
        Lg.backward()
        for g, w, name in zip(gs, ts, ('kernel', 'state', 'depth')):
            assert_grad(g.grad.cpu().numpy(), w.grad.numpy(), f'n={n} T={T} n_ks={n_ks} loss on {use}: d/d{name}')


@pytest.mark.parametrize('weights', [('G',), ('Gc', 'Gf'), ('Gs',)])
def test_partial_losses(weights):
    """A loss on the discharge only, on the final states only, on uh_state_out only."""
    n, T, nsub, n_ks, dt_runoff = 120, 20, 2, 6, 3600.0
    down, k, x = cpu.network('forest', n, seed=9)
    d = unit.unit_inputs(down, T, 4, n_ks=n_ks)
    plan = make_plan(down)
    got = gpu_unit_muskingum_loss_grads(plan, k, x, d, dt_runoff / nsub, dt_runoff, weights=weights)
    want = unit.dense_unit_muskingum_loss_grads(down, k, x, only(d, weights), dt_runoff / nsub, nsub)
    for name in FULL_GRADS:
        assert_grad(got[name], want[name], f'loss on {weights}: d/d{name}')
    if 'Gs' not in weights:
        got = gpu_unit_loss_grads(plan, k, x, d, dt_runoff / nsub, dt_runoff, weights=weights)
        want = unit.dense_unit_loss_grads(down, k, x, only(d, weights), dt_runoff / nsub, nsub)
        for name in ROUTE_GRADS:
            assert_grad(got[name], want[name], f'unit_route, loss on {weights}: d/d{name}')


def test_clamp_active_and_negative_c3():
    n, T, nsub, dt_runoff = 200, 24, 1, 3600.0
    down, k, x = cpu.network('tree', n, seed=21)
    k = k.copy()
    k[::3] = 300.0             # dt / k = 12 > 2 (1 - x): c3 < 0 on every third reach
    d = unit.unit_inputs(down, T, 22, low=-3.0)
    c3 = oracle.muskingum_coefficients(k, x, dt_runoff / nsub)[2]
    assert (c3 < 0).any()
    plan = make_plan(down)
    got = gpu_unit_loss_grads(plan, k, x, d, dt_runoff / nsub, dt_runoff)
    inner = unit.split(down)[1]
    assert (got['out'][:, inner] == 0).mean() > 0.05          # the clamp is active for a good share of the inner outputs
    assert (got['out'][:, unit.split(down)[0]] < 0).any()      # and headwaters pass negative inflow through
    want = unit.dense_unit_loss_grads(down, k, x, d, dt_runoff / nsub, nsub)
    for name in ROUTE_GRADS:
        assert_grad(got[name], want[name], f'clamp / negative c3: d/d{name}')


def test_gradcheck():
    n, T, nsub, n_ks, dt_runoff = 20, 8, 2, 3, 3600.0
    down, k, x = cpu.network('tree', n, seed=2)
    d = unit.unit_inputs(down, T, 3, low=0.3, n_ks=n_ks)
    plan = make_plan(down)

    def f(qc_, qf_, depth_, kern_, st_, k_, x_):
        return rr.grad.unit_muskingum(plan, qc_, qf_, depth_, kern_, st_, k_, x_, dt_runoff / nsub, dt_runoff)

    args = tuple(dev(d[key], True) for key in ('q_ch0', 'q_full0', 'lat', 'kernel', 'state')) + (
        torch.tensor(k, requires_grad=True), torch.tensor(x, requires_grad=True))
    assert torch.autograd.gradcheck(f, args, eps=1e-6, atol=1e-6, rtol=1e-5)


def test_windows_equal_one_call():
    n, T, nsub, n_ks, dt_runoff = 500, 30, 2, 12, 3600.0
    down, k, x = cpu.network('forest', n, seed=8)
    d = unit.unit_inputs(down, T, 6, n_ks=n_ks)
    plan = make_plan(down)
    one = gpu_unit_loss_grads(plan, k, x, d, dt_runoff / nsub, dt_runoff)
    win = gpu_unit_loss_grads(plan, k, x, d, dt_runoff / nsub, dt_runoff, rows_per_window=7)
    for name in one:
        assert_grad(win[name], one[name], f'unit_route windows: {name}', rtol=1e-12)
    one = gpu_unit_muskingum_loss_grads(plan, k, x, d, dt_runoff / nsub, dt_runoff)
    win = gpu_unit_muskingum_loss_grads(plan, k, x, d, dt_runoff / nsub, dt_runoff, rows_per_window=7)       # 7 < n_ks: windows shorter than the kernel
    for name in one:
        assert_grad(win[name], one[name], f'unit_muskingum windows: {name}', rtol=1e-12)
    want = unit.dense_unit_muskingum_loss_grads(down, k, x, d, dt_runoff / nsub, nsub, window=7)
    for name in FULL_GRADS:
        assert_grad(win[name], want[name], f'windows against the windowed restatement: d/d{name}')


def test_two_backward_passes_bit_identical():
    n, T, nsub, n_ks, dt_runoff = 5000, 40, 1, 12, 3600.0
    net = synth.synth_network(n, seed=12)
    down = net.down_index.astype(np.int64)
    d = unit.unit_inputs(down, T, 13, n_ks=n_ks)
    plan = make_plan(down)
    a = gpu_unit_muskingum_loss_grads(plan, net.k, net.x, d, dt_runoff / nsub, dt_runoff)
    b = gpu_unit_muskingum_loss_grads(plan, net.k, net.x, d, dt_runoff / nsub, dt_runoff)
    for name in a:
        assert np.array_equal(a[name], b[name]), name


def test_100k_reaches_directional_difference():
    # dt = 900 s <= every k and 2 x < dt / k: c1, c2, c3 > 0, so with positive inflows no output meets the clamp and the differences
    # cross no kink
    n, T, nsub, dt_runoff = 100_000, 200, 4, 3600.0
    dt = dt_runoff / nsub
    net = synth.synth_network(n, seed=31)
    down = net.down_index.astype(np.int64)
    k, x = net.k, 0.05 + 0.01 * synth.u01(34, np.arange(n))
    c1, c2, c3 = oracle.muskingum_coefficients(k, x, dt)
    assert (c1 > 0).all() and (c2 > 0).all() and (c3 > 0).all()
    d = unit.unit_inputs(down, T, 32, low=0.2)
    plan = make_plan(down)
    Gd = dev(d['G'])
    kt = torch.tensor(k, requires_grad=True)
    latt = dev(d['lat'], True)
    qc0, qf0 = dev(d['q_ch0']), dev(d['q_full0'])
    out, _, _ = rr.grad.unit_route(plan, qc0, qf0, latt, kt, torch.tensor(x), dt, dt_runoff)
    assert bool((out > 0).all())
    (out * Gd).sum().backward()
    rng = np.random.default_rng(33)
    vk = torch.tensor(k * rng.uniform(-1.0, 1.0, n))
    vq = dev(d['lat'] * rng.uniform(-1.0, 1.0, (T, n)))

    def loss(k_, lat_):
        with torch.no_grad():
            o, _, _ = rr.grad.unit_route(plan, qc0, qf0, lat_, k_, torch.tensor(x), dt, dt_runoff)
            return float((o * Gd).sum())

    h = 1e-5
    kk = torch.tensor(k)
    fd = (loss(kk + h * vk, latt.detach()) - loss(kk - h * vk, latt.detach())) / (2 * h)
    an = float((kt.grad * vk).sum())
    print(f'directional difference on k: fd {fd!r} analytic {an!r} rel {abs(fd - an) / abs(an):.3e}')
    assert abs(fd - an) <= 1e-5 * abs(an), (fd, an)
    h = 1e-2      # the loss is linear in the lateral rows here: a long step keeps the round-off of the two sums small
    fd = (loss(kk, latt.detach() + h * vq) - loss(kk, latt.detach() - h * vq)) / (2 * h)
    an = float((latt.grad * vq).sum())
    print(f'directional difference on the rows: fd {fd!r} analytic {an!r} rel {abs(fd - an) / abs(an):.3e}')
    assert abs(fd - an) <= 1e-6 * abs(an), (fd, an)


def test_abi_refusals():
    n, T = 50, 6
    down, k, x = cpu.network('tree', n, seed=4)
    indptr, indices = cpu.csc_from_down(down)
    c1, c2, c3 = oracle.muskingum_coefficients(k, x, 3600.0)
    plan = Plan(indptr, indices)
    ni = plan.n_inner
    buf = lambda count: DeviceBuffer(max(count, 1) * 8)     # noqa: E731
    qc, qf, lat, dis, G, coef, gqc, gqf, glat = buf(ni), buf(ni), buf(T * n), buf(T * n), buf(T * n), buf(3 * n), buf(ni), buf(ni), buf(T * n)

    def code(*args):
        with pytest.raises(_lib.RRError) as e:
            plan.unit_adjoint_dev(*args)
        return e.value.code, e.value.message

    assert code(qc, qf, lat, T, dis, G, None, None, glat, gqc, gqf, coef, None, 0, T, 1)[0] == _lib.RR_E_STATE     # before set_coeffs
    plan.set_coeffs(-c1[indices], c2, c3, None)
    need = plan.unit_adjoint_work_bytes(T, 1)
    work = DeviceBuffer(need)
    assert need >= 8 * n * (2 * T + 2 * T + 2 * plan.depth)
    assert code(qc, qf, lat, T, dis, G, None, None, glat, gqc, gqf, coef, work, need - 8, T, 1)[0] == _lib.RR_E_INVALID      # short work memory
    c, msg = code(qc, qf, lat, T, dis, G, None, None, glat, gqc, gqf, coef, None, 0, T, 1)
    assert c == _lib.RR_E_INVALID and str(need) in msg
    assert code(None, qf, lat, T, dis, G, None, None, glat, gqc, gqf, coef, work, need, T, 1)[0] == _lib.RR_E_INVALID     # q_ch0 for the coefficients
    assert code(qc, qf, None, 0, dis, G, None, None, glat, gqc, gqf, coef, work, need, T, 1)[0] == _lib.RR_E_INVALID      # lateral for the coefficients
    assert code(qc, qf, lat, T - 1, dis, G, None, None, glat, gqc, gqf, coef, work, need, T, 1)[0] == _lib.RR_E_INVALID   # short lateral rows
    assert code(qc, qf, lat, T, None, G, None, None, glat, gqc, gqf, coef, work, need, T, 1)[0] == _lib.RR_E_INVALID      # grad_out without discharge
    assert code(qc, qf, lat, T, dis, G, None, None, glat, gqc, gqf, coef, work, need, 0, 1)[0] == _lib.RR_E_INVALID       # T = 0
    assert code(qc, qf, lat, T, dis, G, None, None, glat, gqc, gqf, coef, work, need, T, 0)[0] == _lib.RR_E_INVALID       # nsub = 0
    with pytest.raises(_lib.RRError) as e:
        plan.unit_adjoint_work_bytes(0, 1)
    assert e.value.code == _lib.RR_E_INVALID
    # general edge data (set_unit_weights)
    plan.set_unit_weights(c1, np.full(indices.shape[0], 0.9))
    assert code(qc, qf, lat, T, dis, G, None, None, glat, gqc, gqf, coef, work, need, T, 1)[0] == _lib.RR_E_UNSUPPORTED
    plan.set_unit_weights(None, None)
    plan.unit_adjoint_dev(qc, qf, lat, T, dis, G, None, None, glat, gqc, gqf, coef, work, need, T, 1)     # accepted again
    _lib.lib().rr_dev_synchronize(0)
    # the convolution's adjoint: short work memory, missing inputs
    n_ks = 3
    kern, depth, gk, gd = buf(n_ks * n), buf(T * n), buf(n_ks * n), buf(T * n)
    uneed = engine.uh_adjoint_work_bytes(T, n_ks, n)
    assert uneed == 8 * T * n_ks * n
    uwork = DeviceBuffer(uneed)
    for args in ((kern, depth, G, None, gd, gk, None, uwork, uneed - 8, T, n_ks, n), (None, depth, G, None, gd, gk, None, uwork, uneed, T, n_ks, n),
                 (kern, None, G, None, gd, gk, None, uwork, uneed, T, n_ks, n), (kern, depth, G, None, gd, gk, None, uwork, uneed, 0, n_ks, n)):
        with pytest.raises(_lib.RRError) as e:
            engine.uh_adjoint_dev(*args)
        assert e.value.code == _lib.RR_E_INVALID
    engine.uh_adjoint_dev(kern, depth, G, None, gd, gk, None, uwork, uneed, T, n_ks, n)
    _lib.lib().rr_dev_synchronize(0)
    # a plan with boundary reaches
    outlet = int(np.flatnonzero(down < 0)[0])
    plan.set_boundary([], [outlet])
    assert code(qc, qf, lat, T, dis, G, None, None, glat, gqc, gqf, coef, work, need, T, 1)[0] == _lib.RR_E_UNSUPPORTED
