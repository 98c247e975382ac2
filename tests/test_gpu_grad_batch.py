"""rr.grad.rapid_route_batch on the GPU (rr_rapid_adjoint_batch_dev: the member-batched k_tick, k_adj_tick, k_adj_reduce and the
*_batch one-pass kernels).  Per member the forward, dL/dqlateral and dL/dq0 are the bits rr.grad.rapid_route gives for that member
alone (compared as uint64 patterns, so the sign of a zero counts); dL/dk and dL/dx are rapid_route's bits for one member, the sum of
the single calls in member order to 1e-12 for several, and the restatement's (tests/test_grad.py) to 1e-9; shared q0, channel-only,
a loss on q_final, a loss on one member of three; groups and windows against one sweep; repeat runs; the ABI's refusals."""
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
DT_RUNOFF = 3600.0


@pytest.fixture(autouse=True)
def _default_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def make_plan(down):
    indptr, indices = cpu.csc_from_down(down)
    return Plan(indptr, indices)


def inputs(B, n, T, seed, low=0.0):
    """Per member its own lateral rows, initial state and loss weights: (ql[B, T, n], q0[B, n], G[B, T, n], Gf[B, n])."""
    rng = np.random.default_rng(seed)
    return (rng.uniform(low, 2.0, (B, T, n)) * DT_RUNOFF, rng.uniform(0.0, 3.0, (B, n)), rng.standard_normal((B, T, n)),
            rng.standard_normal((B, n)))


def batch_grads(plan, k, x, ql, q0, nsub, G, Gf, rows=None, **kw):
    """(discharge, q_final, dL/dk, dL/dx, dL/dql, dL/dq0) of L = sum(G discharge) + sum(Gf q_final) through rapid_route_batch."""
    kt, xt = torch.tensor(k, requires_grad=True), torch.tensor(x, requires_grad=True)
    qlt = None if ql is None else torch.tensor(ql, device=DEV, requires_grad=True)
    q0t = torch.tensor(q0, device=DEV, requires_grad=True)
    d, qf = rr.grad.rapid_route_batch(plan, q0t, qlt, kt, xt, DT_RUNOFF / nsub, DT_RUNOFF, rows=rows, **kw)
    L = 0.0
    if G is not None:
        L = L + (d * torch.tensor(G, device=DEV)).sum()
    if Gf is not None:
        L = L + (qf * torch.tensor(Gf, device=DEV)).sum()
    L.backward()
    return (d.detach().cpu().numpy(), qf.detach().cpu().numpy(), kt.grad.numpy(), xt.grad.numpy(),
            None if qlt is None else qlt.grad.cpu().numpy(), q0t.grad.cpu().numpy())


def single_grads(plan, k, x, ql, q0, nsub, G, Gf, rows=None):
    """The same through rr.grad.rapid_route, one member."""
    kt, xt = torch.tensor(k, requires_grad=True), torch.tensor(x, requires_grad=True)
    qlt = None if ql is None else torch.tensor(ql, device=DEV, requires_grad=True)
    q0t = torch.tensor(q0, device=DEV, requires_grad=True)
    d, qf = rr.grad.rapid_route(plan, q0t, qlt, kt, xt, DT_RUNOFF / nsub, DT_RUNOFF, rows=rows)
    L = (d * torch.tensor(G, device=DEV)).sum() + (qf * torch.tensor(Gf, device=DEV)).sum()
    L.backward()
    return (d.detach().cpu().numpy(), qf.detach().cpu().numpy(), kt.grad.numpy(), xt.grad.numpy(),
            None if qlt is None else qlt.grad.cpu().numpy(), q0t.grad.cpu().numpy())


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def assert_close(got, want, what, rtol):
    scale = max(float(np.abs(want).max()), 1e-300)
    np.testing.assert_allclose(got, want, rtol=rtol, atol=rtol * scale, err_msg=what)


def in_member_order(parts):
    total = parts[0].copy()
    for p in parts[1:]:
        total = total + p
    return total


def check_against_single_calls(plan, k, x, ql, q0, nsub, G, Gf, got, what):
    """Assertions 1, 2 and the first two of 3 of a batched result `got`; returns the members' single-call results."""
    B = q0.shape[0]
    one = [single_grads(plan, k, x, ql[m], q0[m], nsub, G[m], Gf[m]) for m in range(B)]
    d, qf, gk, gx, gql, gq0 = got
    for m in range(B):
        assert same_bits(d[m], one[m][0]), f'{what}: discharge of member {m}'
        assert same_bits(qf[m], one[m][1]), f'{what}: q_final of member {m}'
        assert same_bits(gql[m], one[m][4]), f'{what}: dL/dqlateral of member {m}'
        assert same_bits(gq0[m], one[m][5]), f'{what}: dL/dq0 of member {m}'
    for j, name in ((2, 'k'), (3, 'x')):
        if B == 1:
            assert same_bits(got[j], one[0][j]), f'{what}: dL/d{name} of one member'
        else:
            assert_close(got[j], in_member_order([o[j] for o in one]), f'{what}: dL/d{name} against the single calls', 1e-12)
    return one


# kind, n, T, nsub, B, lowest lateral inflow
CASES = [('tree', 1, 1, 1, 2, 0.0), ('tree', 2, 3, 2, 3, 0.0), ('tree', 50, 40, 1, 1, 0.0), ('tree', 50, 40, 1, 3, -1.0),
         ('postorder', 300, 24, 2, 5, -1.0), ('forest', 300, 16, 4, 2, 0.0), ('chain', 120, 30, 1, 3, 0.0), ('tree', 150, 300, 1, 2, 0.0),
         ('tree', 2000, 3, 1, 3, 0.0)]


@pytest.mark.parametrize('kind,n,T,nsub,B,low', CASES)
def test_members_match_single_calls_and_restatement(kind, n, T, nsub, B, low):
    down, k, x = cpu.network(kind, n, seed=n + T + nsub)
    ql, q0, G, Gf = inputs(B, n, T, n + 17 * B, low=low)
    plan = make_plan(down)
    if B == 1:      # the bits of one member's dL/dk are checked where the reduction has several sub-step ranges to merge
        assert T * nsub > 1
    what = f'{kind} n={n} T={T} nsub={nsub} B={B}'
    got = batch_grads(plan, k, x, ql, q0, nsub, G, Gf)
    check_against_single_calls(plan, k, x, ql, q0, nsub, G, Gf, got, what)
    if low < 0 and B > 1 and n > 2:
        masks = got[0] == 0
        assert masks.any() and any((masks[m] != masks[0]).any() for m in range(1, B)), 'the members clamp at different places'
    dense = [cpu.dense_loss_grads(down, k, x, ql[m], q0[m], DT_RUNOFF / nsub, DT_RUNOFF, G[m], Gf[m]) for m in range(B)]
    assert_close(got[2], in_member_order([w[1] for w in dense]), f'{what}: dL/dk against the restatement', 1e-9)
    assert_close(got[3], in_member_order([w[2] for w in dense]), f'{what}: dL/dx against the restatement', 1e-9)
    for m in range(B):
        assert_close(got[4][m], dense[m][3], f'{what}: dL/dqlateral of member {m} against the restatement', 1e-9)
        assert_close(got[5][m], dense[m][4], f'{what}: dL/dq0 of member {m} against the restatement', 1e-9)


def test_shared_q0_gets_the_sum_of_the_members():
    n, T, nsub, B = 200, 12, 2, 3
    down, k, x = cpu.network('forest', n, seed=14)
    ql, q0, G, Gf = inputs(B, n, T, 15)
    plan = make_plan(down)
    rows = np.ascontiguousarray(np.broadcast_to(q0[0], (B, n)))
    per_member = batch_grads(plan, k, x, ql, rows, nsub, G, Gf)
    shared = batch_grads(plan, k, x, ql, q0[0], nsub, G, Gf)
    assert shared[5].shape == (n,)
    assert_close(shared[5], in_member_order(list(per_member[5])), 'shared q0: dL/dq0', 1e-12)
    for j in (0, 1, 4):
        assert same_bits(shared[j], per_member[j])
    for j in (2, 3):
        assert same_bits(shared[j], per_member[j])      # the same tapes, the same sums


def test_channel_only_and_final_state_only():
    n, T, nsub, B = 120, 20, 2, 3
    down, k, x = cpu.network('forest', n, seed=9)
    ql, q0, G, Gf = inputs(B, n, T, 4)
    plan = make_plan(down)
    got = batch_grads(plan, k, x, None, q0, nsub, G, Gf, rows=T)
    dense = [cpu.dense_loss_grads(down, k, x, None, q0[m], DT_RUNOFF / nsub, DT_RUNOFF, G[m], Gf[m]) for m in range(B)]
    assert_close(got[2], in_member_order([w[1] for w in dense]), 'channel-only: dL/dk', 1e-9)
    assert_close(got[3], in_member_order([w[2] for w in dense]), 'channel-only: dL/dx', 1e-9)
    for m in range(B):
        one = single_grads(plan, k, x, None, q0[m], nsub, G[m], Gf[m], rows=T)
        assert same_bits(got[0][m], one[0]) and same_bits(got[1][m], one[1]) and same_bits(got[5][m], one[5])
        assert_close(got[5][m], dense[m][4], f'channel-only: dL/dq0 of member {m}', 1e-9)
    # a loss of q_final alone: no discharge gradient reaches the adjoint
    got = batch_grads(plan, k, x, ql, q0, nsub, None, Gf)
    dense = [cpu.dense_loss_grads(down, k, x, ql[m], q0[m], DT_RUNOFF / nsub, DT_RUNOFF, np.zeros((T, n)), Gf[m]) for m in range(B)]
    assert_close(got[2], in_member_order([w[1] for w in dense]), 'q_final only: dL/dk', 1e-9)
    for m in range(B):
        assert_close(got[4][m], dense[m][3], f'q_final only: dL/dqlateral of member {m}', 1e-9)
        assert_close(got[5][m], dense[m][4], f'q_final only: dL/dq0 of member {m}', 1e-9)


def test_loss_on_one_member_of_three():
    n, T, nsub, B = 300, 10, 2, 3
    down, k, x = cpu.network('tree', n, seed=23)
    ql, q0, G, Gf = inputs(B, n, T, 24)
    plan = make_plan(down)
    G[0] = 0.0
    G[2] = 0.0
    Gf[0] = 0.0
    Gf[2] = 0.0
    kt = torch.tensor(k, requires_grad=True)
    qlt = torch.tensor(ql, device=DEV, requires_grad=True)
    q0t = torch.tensor(q0, device=DEV, requires_grad=True)
    d, qf = rr.grad.rapid_route_batch(plan, q0t, qlt, kt, torch.tensor(x), DT_RUNOFF / nsub, DT_RUNOFF)
    ((d[1] * torch.tensor(G[1], device=DEV)).sum() + (qf[1] * torch.tensor(Gf[1], device=DEV)).sum()).backward()
    gql, gq0 = qlt.grad.cpu().numpy(), q0t.grad.cpu().numpy()
    for m in (0, 2):
        assert (gql[m] == 0).all() and (gq0[m] == 0).all()
    one = single_grads(plan, k, x, ql[1], q0[1], nsub, G[1], Gf[1])
    assert same_bits(gql[1], one[4]) and same_bits(gq0[1], one[5])
    assert_close(kt.grad.numpy(), one[2], 'one member of three: dL/dk', 1e-12)


def test_groups_and_windows_equal_one_sweep():
    n, T, nsub, B = 500, 30, 2, 5
    down, k, x = cpu.network('forest', n, seed=8)
    ql, q0, G, Gf = inputs(B, n, T, 6)
    plan = make_plan(down)
    whole = batch_grads(plan, k, x, ql, q0, nsub, G, Gf)
    groups = batch_grads(plan, k, x, ql, q0, nsub, G, Gf, members_per_sweep=2)
    for j, name in enumerate(('discharge', 'q_final', 'k', 'x', 'qlateral', 'q0')):
        if name in ('k', 'x'):
            assert_close(groups[j], whole[j], f'groups of two: {name}', 1e-12)
        else:
            assert same_bits(groups[j], whole[j]), f'groups of two: {name}'
    windows = batch_grads(plan, k, x, ql, q0, nsub, G, Gf, rows_per_window=7)
    for j, name in enumerate(('discharge', 'q_final', 'k', 'x', 'qlateral', 'q0')):
        assert_close(windows[j], whole[j], f'windows: {name}', 1e-12)


def test_two_backward_passes_bit_identical():
    n, T, nsub, B = 5000, 40, 1, 3
    net = synth.synth_network(n, seed=12)
    ql, q0, G, Gf = inputs(B, n, T, 13)
    plan = make_plan(net.down_index)
    a = batch_grads(plan, net.k, net.x, ql, q0, nsub, G, Gf)
    b = batch_grads(plan, net.k, net.x, ql, q0, nsub, G, Gf)
    for u, v in zip(a, b):
        assert same_bits(u, v)


def test_20k_reaches_four_members():
    # the one case where a member's tapes (2 x 96 sub-steps x 20,000 values) are long beside the tick's window
    n, T, nsub, B = 20_000, 48, 2, 4
    net = synth.synth_network(n, seed=41)
    ql, q0, G, Gf = inputs(B, n, T, 42, low=-0.5)
    plan = make_plan(net.down_index)
    got = batch_grads(plan, net.k, net.x, ql, q0, nsub, G, Gf)
    check_against_single_calls(plan, net.k, net.x, ql, q0, nsub, G, Gf, got, '20k x 48 x 2, B=4')


def test_abi_refusals():
    n, T, B = 50, 6, 3
    down, k, x = cpu.network('tree', n, seed=4)
    indptr, indices = cpu.csc_from_down(down)
    c1, c2, c3 = oracle.muskingum_coefficients(k, x, 3600.0)
    c4 = (c1 + c2) / 3600.0
    plan = Plan(indptr, indices)
    buf = lambda count: DeviceBuffer(max(count, 1) * 8)     # noqa: E731
    q0, ql, dis, G, coef, gq0, gql = buf(B * n), buf(B * T * n), buf(B * T * n), buf(B * T * n), buf(4 * n), buf(B * n), buf(B * T * n)

    def code(members, work, nbytes, q0_pitch=n, lat_pitch=T * n, out_pitch=T * n, rows=T, nsub=1):
        with pytest.raises(_lib.RRError) as e:
            plan.rapid_adjoint_batch_dev(members, q0, q0_pitch, ql, T, lat_pitch, dis, G, out_pitch, None, gql, gq0, coef, work, nbytes, rows, nsub)
        return e.value.code, e.value.message

    assert code(B, None, 0)[0] == _lib.RR_E_STATE                     # before set_coeffs
    plan.set_coeffs(-c1[indices], c2, c3, c4)
    need = plan.rapid_adjoint_batch_work_bytes(B, T, 1)
    assert plan.rapid_adjoint_batch_work_bytes(1, T, 1) == plan.rapid_adjoint_work_bytes(T, 1)
    # the header's formula: every section but the permutation's rows once per member; here the six sub-steps are six ranges
    S, splits = T, min(T, -(-2048 // (B * -(-n // 256))))
    assert splits == S
    assert need == 8 * n * (B * (2 * S + 2 * T + 2 * plan.depth + 4 * splits + 2) + min(T, 16))
    work = DeviceBuffer(need)
    for members in (0, 65536):
        c, msg = code(members, work, need)
        assert c == _lib.RR_E_INVALID and 'members' in msg
        with pytest.raises(_lib.RRError) as e:
            plan.rapid_adjoint_batch_work_bytes(members, T, 1)
        assert e.value.code == _lib.RR_E_INVALID
    for short in (dict(q0_pitch=n - 1), dict(lat_pitch=T * n - 1), dict(out_pitch=T * n - 1)):
        c, msg = code(B, work, need, **short)
        assert c == _lib.RR_E_INVALID and 'pitch' in msg
    c, msg = code(B, work, need - 8)
    assert c == _lib.RR_E_INVALID and str(need) in msg and 'rr_rapid_adjoint_batch_work_bytes' in msg
    assert code(B, None, 0)[0] == _lib.RR_E_INVALID
    assert code(B, work, need, rows=0)[0] == _lib.RR_E_INVALID          # what the single call refuses comes first
    assert code(B, work, need, nsub=0)[0] == _lib.RR_E_INVALID
    # per-edge weights: one tributary weighted differently
    w = -c1[indices]
    e = int(np.flatnonzero(np.bincount(indices, minlength=n)[indices] >= 2)[0])      # an edge into a confluence
    w[e] *= 1.5
    plan.set_coeffs(w, c2, c3, c4)
    assert code(B, work, need)[0] == _lib.RR_E_UNSUPPORTED
    plan.set_coeffs(-c1[indices], c2, c3, c4)
    plan.rapid_adjoint_batch_dev(B, q0, n, ql, T, T * n, dis, G, T * n, None, gql, gq0, coef, work, need, T, 1)     # accepted again
    plan.rapid_adjoint_batch_dev(B, q0, 0, ql, T, T * n, dis, G, T * n, None, gql, gq0, coef, work, need, T, 1)     # one q0 for all
    _lib.lib().rr_dev_synchronize(0)
