"""rr.grad.unit_route_batch / uh_convolve_batch / unit_muskingum_batch on the GPU (rr_unit_adjoint_batch_dev: the member-batched
k_tick_unit, k_adj_tick_unit, k_adj_reduce_unit and the *_unit_batch one-pass kernels).  Per member the forward, dL/dlateral (or
dL/ddepth), dL/dq_ch0, dL/dq_full0 and dL/duh_state are the bits rr.grad.unit_route / unit_muskingum give for that member alone
(compared as uint64 patterns, so the sign of a zero counts); dL/dk, dL/dx and dL/duh_kernel are the single call's bits for one
member, the sum of the single calls in member order to 1e-12 for several, and the restatement's (tests/test_grad_unit.py) to 1e-9;
shared states, partial losses, a loss on one member of three, negative c3 with the clamp active; groups and windows against one
sweep; repeat runs; the ABI's refusals.  Case for case the grid of tests/test_gpu_grad_batch.py."""
import numpy as np
import pytest
import torch

import river_route_amd as rr
import test_grad as cpu
import test_grad_unit as unit
from oracle import oracle
from river_route_amd import _lib, synth
from river_route_amd.engine import DeviceBuffer, Plan

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
KNOBS = ('RR_WAVE', 'RR_WAVE_K', 'RR_TILE_BLOCK', 'RR_TILE_LEAN', 'RR_UH_PAIRS', 'RR_DIRECT')
DT_RUNOFF = 3600.0
ROUTE_IN = ('lat', 'q_ch0', 'q_full0')
FULL_IN = ('lat', 'q_ch0', 'q_full0', 'kernel', 'state')
WEIGHTS = (('out', 'G'), ('q_ch', 'Gc'), ('q_full', 'Gf'), ('uh_state', 'Gs'))


@pytest.fixture(autouse=True)
def _default_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def make_plan(down):
    indptr, indices = cpu.csc_from_down(down)
    return Plan(indptr, indices)


def dev(a, grad=False):
    return torch.tensor(a, device=DEV, requires_grad=grad)


def members_inputs(down, B, T, seed, low=0.0, n_ks=None):
    """Per member its own unit.unit_inputs (rows, states, loss weights); one kernel for all."""
    ds = [unit.unit_inputs(down, T, seed + 101 * m, low=low, n_ks=n_ks) for m in range(B)]
    for d in ds[1:]:
        if n_ks is not None:
            d['kernel'] = ds[0]['kernel']
    return ds


def stacked(ds, key):
    return np.stack([d[key] for d in ds])


def numpy_of(t):
    return t.detach().cpu().numpy()


def run(plan, k, x, ds, nsub, full, batch, weights=('G', 'Gc', 'Gf', 'Gs'), shared=(), **kw):
    """L = sum over members and outputs of (weights x output) through the batched (ds: the members) or the single (ds: one member's
    dict) functions, routing alone or with the convolution chained in (full).  Outputs and gradients as numpy by name; `shared`
    names inputs given once for all members (the first member's)."""
    kt, xt = torch.tensor(k, requires_grad=True), torch.tensor(x, requires_grad=True)
    names = FULL_IN if full else ROUTE_IN
    if batch:
        t = {key: dev(ds[0][key] if key in shared else stacked(ds, key), True) for key in names if key != 'kernel'}
    else:
        t = {key: dev(ds[key], True) for key in names if key != 'kernel'}
    dt = DT_RUNOFF / nsub
    if full:
        t['kernel'] = dev((ds[0] if batch else ds)['kernel'], True)
        f = rr.grad.unit_muskingum_batch if batch else rr.grad.unit_muskingum
        outs = f(plan, t['q_ch0'], t['q_full0'], t['lat'], t['kernel'], t['state'], kt, xt, dt, DT_RUNOFF, **kw)
    else:
        f = rr.grad.unit_route_batch if batch else rr.grad.unit_route
        outs = f(plan, t['q_ch0'], t['q_full0'], t['lat'], kt, xt, dt, DT_RUNOFF, **kw)
    L = 0.0
    for v, (_, w) in zip(outs, WEIGHTS):
        if w in weights:
            L = L + (v * dev(stacked(ds, w) if batch else ds[w])).sum()
    L.backward()
    z = lambda v: numpy_of(torch.zeros_like(v) if v.grad is None else v.grad)      # noqa: E731
    res = dict(k=z(kt), x=z(xt), **{key: z(v) for key, v in t.items()})
    res.update({name: numpy_of(v) for v, (name, _) in zip(outs, WEIGHTS)})
    return res


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def assert_close(got, want, what, rtol):
    assert got.shape == want.shape, what
    if want.size:
        scale = max(float(np.abs(want).max()), 1e-300)
        np.testing.assert_allclose(got, want, rtol=rtol, atol=rtol * scale, err_msg=what)


def in_member_order(parts):
    total = parts[0].copy()
    for p in parts[1:]:
        total = total + p
    return total


def check_against_single_calls(plan, k, x, ds, nsub, full, got, what, **kw):
    """Per member every output and every per-member gradient bit-equal to the single call's; the summed gradients (k, x, kernel) its bits
    for one member, the member-ordered sum to 1e-12 for several.  Returns the members' single-call results."""
    B = len(ds)
    one = [run(plan, k, x, d, nsub, full, False, **kw) for d in ds]
    per_member = ('out', 'q_ch', 'q_full', 'lat', 'q_ch0', 'q_full0') + (('uh_state', 'state') if full else ())
    for m in range(B):
        for name in per_member:
            assert same_bits(got[name][m], one[m][name]), f'{what}: {name} of member {m}'
    for name in ('k', 'x') + (('kernel',) if full else ()):
        if B == 1:
            assert same_bits(got[name], one[0][name]), f'{what}: dL/d{name} of one member'
        else:
            assert_close(got[name], in_member_order([o[name] for o in one]), f'{what}: dL/d{name} against the single calls', 1e-12)
    return one


# kind, n, T, nsub, B, lowest lateral inflow
CASES = [('tree', 1, 1, 1, 2, 0.0), ('tree', 2, 3, 2, 3, 0.0), ('tree', 50, 40, 1, 1, 0.0), ('tree', 50, 40, 1, 3, -1.0),
         ('postorder', 300, 24, 2, 5, 0.0), ('forest', 300, 16, 4, 2, 0.0), ('chain', 120, 30, 1, 3, 0.0), ('tree', 150, 300, 1, 2, 0.0),
         ('tree', 2000, 3, 1, 3, 0.0)]


@pytest.mark.parametrize('kind,n,T,nsub,B,low', CASES)
def test_members_match_single_calls_and_restatement(kind, n, T, nsub, B, low):
    down, k, x = cpu.network(kind, n, seed=n + T + nsub)
    ds = members_inputs(down, B, T, n + 17 * B, low=low)
    plan = make_plan(down)
    if n == 1:
        assert plan.n_inner == 0      # a lone headwater: empty states, no tick
    if B == 1:      # the bits of one member's dL/dk are checked where the reduction has several sub-step ranges to merge
        assert T * nsub > 1
    what = f'{kind} n={n} T={T} nsub={nsub} B={B}'
    got = run(plan, k, x, ds, nsub, False, True)
    check_against_single_calls(plan, k, x, ds, nsub, False, got, what)
    if low < 0:
        masks = got['out'][:, :, unit.split(down)[1]] == 0
        assert masks.any() and any((masks[m] != masks[0]).any() for m in range(1, B)), 'the members clamp at different places'
    dense = [unit.dense_unit_loss_grads(down, k, x, d, DT_RUNOFF / nsub, nsub) for d in ds]
    for name in ('k', 'x'):
        assert_close(got[name], in_member_order([w[name] for w in dense]), f'{what}: dL/d{name} against the restatement', 1e-9)
    for m in range(B):
        for name in ROUTE_IN:
            assert_close(got[name][m], dense[m][name], f'{what}: dL/d{name} of member {m} against the restatement', 1e-9)


# n_ks 1, 3, 48 and one case with T < n_ks
UH_CASES = [('tree', 2, 3, 2, 1, 2), ('postorder', 200, 24, 2, 3, 3), ('forest', 250, 12, 4, 48, 2), ('chain', 60, 30, 1, 48, 3)]


@pytest.mark.parametrize('kind,n,T,nsub,n_ks,B', UH_CASES)
def test_unit_muskingum_batch(kind, n, T, nsub, n_ks, B):
    down, k, x = cpu.network(kind, n, seed=n + T + nsub)
    ds = members_inputs(down, B, T, n + 19, n_ks=n_ks)
    plan = make_plan(down)
    what = f'{kind} n={n} T={T} nsub={nsub} n_ks={n_ks} B={B}'
    got = run(plan, k, x, ds, nsub, True, True)
    check_against_single_calls(plan, k, x, ds, nsub, True, got, what)
    dense = [unit.dense_unit_muskingum_loss_grads(down, k, x, d, DT_RUNOFF / nsub, nsub) for d in ds]
    for name in ('k', 'x', 'kernel'):
        assert_close(got[name], in_member_order([w[name] for w in dense]), f'{what}: dL/d{name} against the restatement', 1e-9)
    for m in range(B):
        for name, theirs in (('lat', 'depth'), ('state', 'state'), ('q_ch0', 'q_ch0'), ('q_full0', 'q_full0')):
            assert_close(got[name][m], dense[m][theirs], f'{what}: dL/d{theirs} of member {m} against the restatement', 1e-9)


def test_uh_convolve_batch_members_are_uh_convolve():
    n, T, n_ks, B = 300, 20, 12, 3
    rng = np.random.default_rng(5)
    kernel, state, depth = rng.uniform(0, 1, (n_ks, n)), rng.uniform(0, 5, (B, n_ks, n)), rng.uniform(0, 3, (B, T, n))
    Gc, Gs = rng.standard_normal((B, T, n)), rng.standard_normal((B, n_ks, n))
    kt, st, dt = dev(kernel, True), dev(state, True), dev(depth, True)
    conv, out = rr.grad.uh_convolve_batch(kt, st, dt)
    ((conv * dev(Gc)).sum() + (out * dev(Gs)).sum()).backward()
    parts = []
    for m in range(B):
        k1, s1, d1 = dev(kernel, True), dev(state[m], True), dev(depth[m], True)
        c1, o1 = rr.grad.uh_convolve(k1, s1, d1)
        ((c1 * dev(Gc[m])).sum() + (o1 * dev(Gs[m])).sum()).backward()
        assert same_bits(numpy_of(conv[m]), numpy_of(c1)) and same_bits(numpy_of(out[m]), numpy_of(o1))
        assert same_bits(numpy_of(st.grad[m]), numpy_of(s1.grad)) and same_bits(numpy_of(dt.grad[m]), numpy_of(d1.grad))
        parts.append(numpy_of(k1.grad))
    assert_close(numpy_of(kt.grad), in_member_order(parts), 'dL/dkernel in member order', 1e-12)


def test_shared_states_get_the_sum_of_the_members():
    n, T, nsub, n_ks, B = 200, 12, 2, 6, 3
    down, k, x = cpu.network('forest', n, seed=14)
    ds = members_inputs(down, B, T, 15, n_ks=n_ks)
    plan = make_plan(down)
    rows = [dict(d, q_ch0=ds[0]['q_ch0'], q_full0=ds[0]['q_full0'], state=ds[0]['state']) for d in ds]
    per_member = run(plan, k, x, rows, nsub, True, True)
    shared = run(plan, k, x, rows, nsub, True, True, shared=('q_ch0', 'q_full0', 'state'))
    assert shared['q_ch0'].shape == (plan.n_inner,) and shared['state'].shape == (n_ks, n)
    for name in ('q_ch0', 'q_full0', 'state'):
        assert_close(shared[name], in_member_order(list(per_member[name])), f'shared {name}', 1e-12)
    for name in ('out', 'q_ch', 'q_full', 'uh_state', 'lat', 'k', 'x', 'kernel'):
        assert same_bits(shared[name], per_member[name]), name      # the same tapes, the same sums
    # one state shared and the other per member: both go as dense rows
    mixed = run(plan, k, x, rows, nsub, False, True, shared=('q_ch0',))
    route = run(plan, k, x, rows, nsub, False, True)
    assert_close(mixed['q_ch0'], in_member_order(list(route['q_ch0'])), 'q_ch0 alone shared', 1e-12)
    for name in ('out', 'lat', 'q_full0', 'k', 'x'):
        assert same_bits(mixed[name], route[name]), name


@pytest.mark.parametrize('weights', [('Gc', 'Gf'), ('Gs',)])
def test_partial_losses(weights):
    """A loss on the final states only, on uh_state_out only."""
    n, T, nsub, n_ks, B = 120, 20, 2, 6, 3
    down, k, x = cpu.network('forest', n, seed=9)
    ds = members_inputs(down, B, T, 4, n_ks=n_ks)
    plan = make_plan(down)
    got = run(plan, k, x, ds, nsub, True, True, weights=weights)
    check_against_single_calls(plan, k, x, ds, nsub, True, got, f'loss on {weights}', weights=weights)
    zero = lambda d: {key: (np.zeros_like(v) if key in ('G', 'Gc', 'Gf', 'Gs') and key not in weights else v) for key, v in d.items()}      # noqa: E731
    dense = [unit.dense_unit_muskingum_loss_grads(down, k, x, zero(d), DT_RUNOFF / nsub, nsub) for d in ds]
    for name in ('k', 'x', 'kernel'):
        assert_close(got[name], in_member_order([w[name] for w in dense]), f'loss on {weights}: dL/d{name}', 1e-9)
    for m in range(B):
        for name, theirs in (('lat', 'depth'), ('state', 'state'), ('q_ch0', 'q_ch0'), ('q_full0', 'q_full0')):
            assert_close(got[name][m], dense[m][theirs], f'loss on {weights}: dL/d{theirs} of member {m}', 1e-9)
    if 'Gs' not in weights:
        got = run(plan, k, x, ds, nsub, False, True, weights=weights)
        check_against_single_calls(plan, k, x, ds, nsub, False, got, f'unit_route_batch, loss on {weights}', weights=weights)


def test_loss_on_one_member_of_three():
    n, T, nsub, B = 300, 10, 2, 3
    down, k, x = cpu.network('tree', n, seed=23)
    ds = members_inputs(down, B, T, 24)
    plan = make_plan(down)
    kt = torch.tensor(k, requires_grad=True)
    t = {key: dev(stacked(ds, key), True) for key in ROUTE_IN}
    out, qc, qf = rr.grad.unit_route_batch(plan, t['q_ch0'], t['q_full0'], t['lat'], kt, torch.tensor(x), DT_RUNOFF / nsub, DT_RUNOFF)
    ((out[1] * dev(ds[1]['G'])).sum() + (qc[1] * dev(ds[1]['Gc'])).sum() + (qf[1] * dev(ds[1]['Gf'])).sum()).backward()
    g = {key: numpy_of(v.grad) for key, v in t.items()}
    for m in (0, 2):
        for key in ROUTE_IN:
            assert (g[key][m] == 0).all(), (key, m)
    one = run(plan, k, x, ds[1], nsub, False, False)
    for key in ROUTE_IN:
        assert same_bits(g[key][1], one[key]), key
    assert_close(kt.grad.numpy(), one['k'], 'one member of three: dL/dk', 1e-12)


def test_clamp_active_and_negative_c3():
    n, T, nsub, B = 200, 24, 1, 3
    down, k, x = cpu.network('tree', n, seed=21)
    k = k.copy()
    k[::3] = 300.0             # dt / k = 12 > 2 (1 - x): c3 < 0 on every third reach
    ds = members_inputs(down, B, T, 22, low=-3.0)
    assert (oracle.muskingum_coefficients(k, x, DT_RUNOFF / nsub)[2] < 0).any()
    plan = make_plan(down)
    got = run(plan, k, x, ds, nsub, False, True)
    hw, inner = unit.split(down)
    assert (got['out'][:, :, inner] == 0).mean() > 0.05          # the clamp is active for a good share of the inner outputs
    assert (got['out'][:, :, hw] < 0).any()                      # and headwaters pass negative inflow through
    check_against_single_calls(plan, k, x, ds, nsub, False, got, 'clamp / negative c3')
    dense = [unit.dense_unit_loss_grads(down, k, x, d, DT_RUNOFF / nsub, nsub) for d in ds]
    for name in ('k', 'x'):
        assert_close(got[name], in_member_order([w[name] for w in dense]), f'clamp / negative c3: dL/d{name}', 1e-9)
    for m in range(B):
        for name in ROUTE_IN:
            assert_close(got[name][m], dense[m][name], f'clamp / negative c3: dL/d{name} of member {m}', 1e-9)


def test_groups_and_windows_equal_one_sweep():
    n, T, nsub, n_ks, B = 500, 30, 2, 12, 5
    down, k, x = cpu.network('forest', n, seed=8)
    ds = members_inputs(down, B, T, 6, n_ks=n_ks)
    plan = make_plan(down)
    summed = ('k', 'x', 'kernel')
    for full in (False, True):
        whole = run(plan, k, x, ds, nsub, full, True)
        groups = run(plan, k, x, ds, nsub, full, True, members_per_sweep=2)
        for name in whole:
            if name in summed:
                assert_close(groups[name], whole[name], f'groups of two: {name}', 1e-12)
            else:
                assert same_bits(groups[name], whole[name]), f'groups of two: {name}'
        windows = run(plan, k, x, ds, nsub, full, True, rows_per_window=7)       # 7 < n_ks: windows shorter than the kernel
        for name in whole:
            assert_close(windows[name], whole[name], f'windows: {name}', 1e-12)
        windows_in_groups = run(plan, k, x, ds, nsub, full, True, rows_per_window=7, members_per_sweep=2)
        for name in whole:
            if name in summed:
                assert_close(windows_in_groups[name], windows[name], f'windows in groups of two: {name}', 1e-12)
            else:
                assert same_bits(windows_in_groups[name], windows[name]), f'windows in groups of two: {name}'


def test_two_backward_passes_bit_identical():
    n, T, nsub, n_ks, B = 5000, 40, 1, 12, 3
    net = synth.synth_network(n, seed=12)
    down = net.down_index.astype(np.int64)
    ds = members_inputs(down, B, T, 13, n_ks=n_ks)
    plan = make_plan(down)
    a = run(plan, net.k, net.x, ds, nsub, True, True)
    b = run(plan, net.k, net.x, ds, nsub, True, True)
    for name in a:
        assert same_bits(a[name], b[name]), name


def test_20k_reaches_four_members():
    # the one case where a member's tapes (2 x 96 sub-steps x 20,000 values) are long beside the tick's window
    n, T, nsub, B = 20_000, 48, 2, 4
    net = synth.synth_network(n, seed=41)
    down = net.down_index.astype(np.int64)
    ds = members_inputs(down, B, T, 42, low=-0.5)
    plan = make_plan(down)
    got = run(plan, net.k, net.x, ds, nsub, False, True)
    check_against_single_calls(plan, net.k, net.x, ds, nsub, False, got, '20k x 48 x 2, B=4')


def test_abi_refusals():
    n, T, B = 50, 6, 3
    down, k, x = cpu.network('tree', n, seed=4)
    indptr, indices = cpu.csc_from_down(down)
    c1, c2, c3 = oracle.muskingum_coefficients(k, x, 3600.0)
    plan = Plan(indptr, indices)
    ni = plan.n_inner
    buf = lambda count: DeviceBuffer(max(count, 1) * 8)     # noqa: E731
    qc, qf, lat, dis, G, coef = buf(B * ni), buf(B * ni), buf(B * T * n), buf(B * T * n), buf(B * T * n), buf(3 * n)
    gqc, gqf, glat = buf(B * ni), buf(B * ni), buf(B * T * n)
    outputs = (coef, gqc, gqf, glat)
    for b in outputs:
        b.upload(np.full(b.nbytes // 8, -7.0))

    def code(members, work, nbytes, state_pitch=ni, lat_pitch=T * n, out_pitch=T * n, rows=T, nsub=1):
        with pytest.raises(_lib.RRError) as e:
            plan.unit_adjoint_batch_dev(members, qc, qf, state_pitch, lat, T, lat_pitch, dis, G, out_pitch, None, None, glat, gqc, gqf, coef,
                                        work, nbytes, rows, nsub)
        for b in outputs:      # a refused call writes nothing
            assert (b.download(np.float64, (b.nbytes // 8,)) == -7.0).all()
        return e.value.code, e.value.message

    assert code(B, None, 0)[0] == _lib.RR_E_STATE                     # before set_coeffs
    plan.set_coeffs(-c1[indices], c2, c3, None)
    need = plan.unit_adjoint_batch_work_bytes(B, T, 1)
    assert plan.unit_adjoint_batch_work_bytes(1, T, 1) == plan.unit_adjoint_work_bytes(T, 1)
    # the header's formula: every section but the permutation's rows once per member; here the six sub-steps are six ranges
    S, splits = T, min(T, -(-2048 // (B * -(-n // 256))))
    assert splits == S
    assert need == 8 * n * (B * (2 * S + 2 * T + 2 * plan.depth + 3 * splits + 6) + min(T, 16))
    work = DeviceBuffer(need)
    for members in (0, 65536):
        c, msg = code(members, work, need)
        assert c == _lib.RR_E_INVALID and 'members' in msg
        with pytest.raises(_lib.RRError) as e:
            plan.unit_adjoint_batch_work_bytes(members, T, 1)
        assert e.value.code == _lib.RR_E_INVALID
    for short in (dict(state_pitch=ni - 1), dict(state_pitch=-ni), dict(lat_pitch=T * n - 1), dict(out_pitch=T * n - 1)):
        c, msg = code(B, work, need, **short)
        assert c == _lib.RR_E_INVALID and 'pitch' in msg, short
    c, msg = code(B, work, need - 8)
    assert c == _lib.RR_E_INVALID and str(need) in msg and 'rr_unit_adjoint_batch_work_bytes' in msg
    assert code(B, None, 0)[0] == _lib.RR_E_INVALID
    assert code(B, work, need, rows=0)[0] == _lib.RR_E_INVALID          # what the single call refuses comes first
    assert code(B, work, need, nsub=0)[0] == _lib.RR_E_INVALID
    # general edge data (set_unit_weights)
    plan.set_unit_weights(c1, np.full(indices.shape[0], 0.9))
    assert code(B, work, need)[0] == _lib.RR_E_UNSUPPORTED
    plan.set_unit_weights(None, None)
    # per-edge weights: one tributary weighted differently
    w = -c1[indices]
    e = int(np.flatnonzero(np.bincount(indices, minlength=n)[indices] >= 2)[0])      # an edge into a confluence
    w[e] *= 1.5
    plan.set_coeffs(w, c2, c3, None)
    assert code(B, work, need)[0] == _lib.RR_E_UNSUPPORTED
    plan.set_coeffs(-c1[indices], c2, c3, None)
    args = (lat, T, T * n, dis, G, T * n, None, None, glat, gqc, gqf, coef, work, need, T, 1)
    plan.unit_adjoint_batch_dev(B, qc, qf, ni, *args)     # accepted again
    plan.unit_adjoint_batch_dev(B, qc, qf, 0, *args)      # one pair of states for all
    _lib.lib().rr_dev_synchronize(0)
