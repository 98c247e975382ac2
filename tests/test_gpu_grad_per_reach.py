"""The routing adjoints on the GPU at every output element against the adjoint arbiter (oracle/rr_oracle_adj.c; DESIGN.md section
2c): rr_rapid_adjoint_dev / rr_unit_adjoint_dev and their _batch and _gauges forms, driven through Plan as a C caller would --
set_coeffs, the forward route call for the GPU's own discharge, the sizer, the adjoint call -- at the shapes where the reduction sums
several sub-steps per range (a ragged last range, ranges across row boundaries, one range, members x ranges), where the launch
shapes stride (more than 65,535 rows, more than 8192 x 256 mask elements), and over wide fan-in, no edges and partial losses.  Each case
asserts the sub-step ranges it is meant to have, through the sizer's answer; then that the GPU's own discharge clamps exactly the
elements the arbiter clamps; then every output under per_reach.assert_per_element.  The case table, its seeds and the references are
per_reach's, shared with tests/test_adjoint_oracle.py, which holds the arbiter itself to account and fixes K_ADJ.  One case per router
also goes through rr.grad end to end, for dL/dk and dL/dx."""
import time

import numpy as np
import pytest
import torch

import river_route_amd as rr
import per_reach as pr
from river_route_amd.engine import Plan

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
KNOBS = ('RR_WAVE', 'RR_WAVE_K', 'RR_TILE_BLOCK', 'RR_TILE_LEAN', 'RR_UH_PAIRS', 'RR_DIRECT')


@pytest.fixture(autouse=True)
def _default_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def dev(a):
    return None if a is None else torch.tensor(np.ascontiguousarray(a), device=DEV)


def poison(*shape):
    """An output the call must write all of: whatever it leaves is a NaN where the arbiter has none."""
    return torch.full(shape, float('nan'), dtype=torch.float64, device=DEV)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def report(what, worst, seconds=None):
    print(f'[grad per reach] {what}: worst ratio {max(worst.values()):.3f} of K = {pr.K_ADJ:g}  (' +
          ', '.join(f'{k} {v:.2f}' for k, v in worst.items()) + ')' + ('' if seconds is None else f'  forward + adjoint {seconds:.2f} s'))


def assert_mask(d, raw, columns, what):
    same = (d[..., columns] > 0) == (raw[..., columns] > 0)
    assert same.all(), (f'{what}: the GPU\'s own discharge clamps {int((~same).sum())} elements the arbiter does not (or the reverse): '
                        f'the gradient is discontinuous there, no gradient is compared')


def stack(rs, name):
    return np.stack([getattr(r, name) for r in rs])


# ------------------------------------------------------------------------------------------------ RapidMuskingum

def rapid_run(rs, form, shared=False, gauges=None, with_grad_lateral=True):
    """The members rs (rapid_adjoint_case results on one network) through one adjoint call of `form` ('single', 'batch', 'gauges').
    Returns (grad_coef[4, n], grad_q0[M, n], grad_lateral[M, T, n] or None, seconds)."""
    r = rs[0]
    M, n, T, nsub = len(rs), r.n, r.T, r.nsub
    plan = Plan(r.indptr, r.indices)
    channel = r.ql is None
    plan.set_coeffs(-r.c[0][r.indices], r.c[1], r.c[2], None if channel else r.c[3])
    q0 = dev(r.q0 if shared else stack(rs, 'q0'))
    ql = None if channel else dev(stack(rs, 'ql'))
    dis = poison(M, T, n)
    t0 = time.perf_counter()
    for m in range(M):
        q = (q0 if shared else q0[m]).clone()
        if channel:
            plan.muskingum_route_dev(q, dis[m], T, T, nsub)
        else:
            plan.rapid_route_dev(q, ql[m], T, dis[m], T, T, nsub)
    d = host(dis)
    for m in range(M):
        assert_mask(d[m], rs[m].exact.raw, slice(None), f'member {m}')
    G = None if r.G is None else dev(stack(rs, 'G'))
    Gf = None if r.Gf is None else dev(stack(rs, 'Gf'))
    g_coef, g_q0 = poison(4, n), poison(M, n)
    g_lat = poison(M, T, n) if (with_grad_lateral and not channel) else None
    splits = pr.adjoint_splits(n, T, nsub, M if form != 'single' else 1)
    if form == 'single':
        assert M == 1
        need = plan.rapid_adjoint_work_bytes(T, nsub)
        assert need == pr.adjoint_work_bytes(n, plan.depth, T, nsub, 'rapid'), f'the sizer does not lay out {splits} sub-step ranges'
        work = torch.empty(need, dtype=torch.uint8, device=DEV)
        plan.rapid_adjoint_dev(q0[0], None if channel else ql[0], T, dis[0], None if G is None else G[0], None if Gf is None else Gf[0],
                               None if g_lat is None else g_lat[0], g_q0[0], g_coef, work, need, T, nsub)
    elif form == 'batch':
        need = plan.rapid_adjoint_batch_work_bytes(M, T, nsub)
        assert need == pr.adjoint_work_bytes(n, plan.depth, T, nsub, 'rapid', M), f'the sizer does not lay out {splits} sub-step ranges'
        work = torch.empty(need, dtype=torch.uint8, device=DEV)
        plan.rapid_adjoint_batch_dev(M, q0, 0 if shared else n, ql, T, T * n, dis, G, T * n, Gf, g_lat, g_q0, g_coef, work, need, T, nsub)
    else:
        ng = gauges.size
        need = plan.rapid_adjoint_gauges_work_bytes(M, ng, T, nsub, g_lat is not None)
        assert need == pr.adjoint_work_bytes(n, plan.depth, T, nsub, 'rapid', M, ng, g_lat is not None), \
            f'the sizer does not lay out {splits} sub-step ranges'
        work = torch.empty(need, dtype=torch.uint8, device=DEV)
        gi = torch.tensor(gauges.astype(np.int64), device=DEV)
        dis_g, G_g = dis[:, :, gi].contiguous(), G[:, :, gi].contiguous()
        plan.rapid_adjoint_gauges_dev(M, ng, dev(gauges.astype(np.int32)), q0, 0 if shared else n, ql, T, T * n, dis_g, G_g, T * ng, Gf, g_lat,
                                      g_q0, g_coef, work, need, T, nsub)
    out = host(g_coef), host(g_q0), None if g_lat is None else host(g_lat)
    return (*out, time.perf_counter() - t0)


def judge_rapid(rs, got, what, lateral=True):
    g_coef, g_q0, g_lat, seconds = got
    worst = {}
    orc = rs[0].orc.grad_coef if len(rs) == 1 else sum(r.orc.grad_coef for r in rs[1:]) + rs[0].orc.grad_coef
    exact = rs[0].exact.grad_coef if len(rs) == 1 else pr.member_sum([r.exact.grad_coef for r in rs])
    scale = sum(r.exact.scale_coef for r in rs)
    for j, name in enumerate(('dc1', 'dc2', 'dc3', 'dc4dt')):
        worst[name] = pr.assert_per_element(g_coef[j], orc[j], exact[j], scale[j], f'{what}: dL/{name}')
    worst['dq0'] = max(pr.assert_per_element(g_q0[m], r.orc.grad_q0, r.exact.grad_q0, r.exact.scale_q0, f'{what}: member {m} dL/dq0')
                       for m, r in enumerate(rs))
    if lateral and rs[0].ql is not None:
        worst['dlateral'] = max(pr.assert_per_element(g_lat[m], r.orc.grad_lateral, r.exact.grad_lateral, r.exact.scale_lateral,
                                                      f'{what}: member {m} dL/dlateral') for m, r in enumerate(rs))
    else:
        assert g_lat is None
    report(what, worst, seconds)
    return worst


SINGLE = [(case, regime) for case, v in pr.ADJ_CASES.items() if v[3] == 1 and case != pr.PARTIAL_CASE for regime in v[5]]


@pytest.mark.parametrize('case,regime', SINGLE)
def test_rapid_every_output(case, regime):
    net, T, nsub, _, expect, _ = pr.ADJ_CASES[case]
    r = pr.rapid_adjoint_case(case, regime)
    assert pr.adjoint_splits(r.n, T, nsub) == expect
    got = rapid_run([r], 'single')
    judge_rapid([r], got, f'rapid {case} / {regime}')


@pytest.mark.parametrize('shared', [False, True], ids=['own q0', 'shared q0'])
def test_rapid_batch(shared):
    net, T, nsub, M, expect, _ = pr.ADJ_CASES['batch']
    rs = [pr.rapid_adjoint_case('batch', 'benign', m, 'both', shared and m > 0) for m in range(M)]
    assert pr.adjoint_splits(rs[0].n, T, nsub, M) == expect == (7, 14)
    judge_rapid(rs, rapid_run(rs, 'batch', shared=shared), f'rapid batch of {M}, {"shared" if shared else "own"} q0')


@pytest.mark.parametrize('members,with_grad_lateral', [(1, True), (1, False), (3, True), (3, False)])
def test_rapid_gauges(members, with_grad_lateral):
    case = 'ragged ranges'
    net, T, nsub, _, _, _ = pr.ADJ_CASES[case]
    rs = [pr.rapid_adjoint_case(case, 'benign', m, 'gauges') for m in range(members)]
    assert pr.adjoint_splits(rs[0].n, T, nsub, members) == {1: (71, 5), 3: (28, 13)}[members]
    got = rapid_run(rs, 'gauges', gauges=pr.gauge_columns(case), with_grad_lateral=with_grad_lateral)
    judge_rapid(rs, got, f'rapid {pr.N_GAUGES} gauges, {members} member(s), grad_lateral {with_grad_lateral}', lateral=with_grad_lateral)


@pytest.mark.parametrize('loss', ['channel', 'final', 'outlet'])
def test_rapid_partial_losses(loss):
    r = pr.rapid_adjoint_case(pr.PARTIAL_CASE, 'benign', 0, loss)
    if loss == 'outlet':
        mag = np.abs(r.exact.grad_q0[r.exact.scale_q0 > 0])
        assert mag.max() / mag[mag > 0].min() > 1e6      # many decades: the element's own scale is what matters here
    judge_rapid([r], rapid_run([r], 'single'), f'rapid partial loss: {loss}')


def test_rapid_through_rr_grad_to_k_and_x():
    case = 'ragged ranges'
    r = pr.rapid_adjoint_case(case, 'benign')
    plan = Plan(r.indptr, r.indices)
    kt, xt = torch.tensor(r.k, requires_grad=True), torch.tensor(r.x, requires_grad=True)
    qlt, q0t = dev(r.ql).requires_grad_(), dev(r.q0).requires_grad_()
    dt = pr.DT_RUNOFF / r.nsub
    d, qf = rr.grad.rapid_route(plan, q0t, qlt, kt, xt, dt, pr.DT_RUNOFF)
    assert_mask(host(d.detach()), r.exact.raw, slice(None), 'rr.grad.rapid_route')
    ((d * dev(r.G)).sum() + (qf * dev(r.Gf)).sum()).backward()
    worst = {}
    jk, jx = pr.coefficient_jacobian(r.k, r.x, dt)
    for name, jac, got in (('dk', jk, kt.grad.numpy()), ('dx', jx, xt.grad.numpy())):
        exact, scale = pr.chain_to_kx(jac, r.exact.grad_coef, r.exact.scale_coef)
        orc, _ = pr.chain_to_kx(jac, r.orc.grad_coef, r.exact.scale_coef)
        worst[name] = pr.assert_per_element(got, orc, exact, scale, f'rr.grad.rapid_route: dL/{name}')
    worst['dq0'] = pr.assert_per_element(host(q0t.grad), r.orc.grad_q0, r.exact.grad_q0, r.exact.scale_q0, 'rr.grad.rapid_route: dL/dq0')
    worst['dlateral'] = pr.assert_per_element(host(qlt.grad), r.orc.grad_lateral, r.exact.grad_lateral, r.exact.scale_lateral,
                                              'rr.grad.rapid_route: dL/dqlateral')
    report('rr.grad.rapid_route', worst)


# ------------------------------------------------------------------------------------------------ UnitMuskingum

def unit_run(rs, form, shared=False, gauges=None, with_grad_lateral=True):
    """rapid_run for UnitMuskingum.  Returns (grad_coef[3, n], grad_qch0[M, ni], grad_qfull0[M, ni], grad_lateral or None, seconds)."""
    r = rs[0]
    M, n, ni, T, nsub = len(rs), r.n, r.ni, r.T, r.nsub
    plan = Plan(r.indptr, r.indices)
    assert plan.n_inner == ni
    plan.set_coeffs(-r.c[0][r.indices], r.c[1], r.c[2], None)
    pad = max(ni, 1)      # (a network without inner reaches has no states: the pointers still have to be pointers)

    def states(name):
        a = np.zeros((1 if shared else M, pad))
        a[:, :ni] = getattr(r, name) if shared else stack(rs, name)
        return dev(a)
    qc0, qf0 = states('q_ch0'), states('q_full0')
    lat = dev(stack(rs, 'lat'))
    dis = poison(M, T, n)
    t0 = time.perf_counter()
    for m in range(M):
        k = 0 if shared else m
        plan.unit_route_dev(qc0[k].clone(), qf0[k].clone(), lat[m], T, dis[m], T, T, nsub)
    d = host(dis)
    for m in range(M):
        assert_mask(d[m], rs[m].exact.raw, r.inner, f'member {m}')
        hw = np.setdiff1d(np.arange(n), r.inner)
        assert np.array_equal(d[m][:, hw], rs[m].lat[:, hw])
    G = None if r.G is None else dev(stack(rs, 'G'))

    def final(name):
        if getattr(r, name) is None:
            return None
        a = np.zeros((M, pad))
        a[:, :ni] = stack(rs, name)
        return dev(a)
    Gc, Gf = final('Gc'), final('Gf')
    g_coef, g_qc, g_qf = poison(3, n), poison(M, pad), poison(M, pad)
    g_lat = poison(M, T, n) if with_grad_lateral else None
    splits = pr.adjoint_splits(n, T, nsub, M if form != 'single' else 1)
    pitch = 0 if shared else pad
    if form == 'single':
        assert M == 1
        need = plan.unit_adjoint_work_bytes(T, nsub)
        assert need == pr.adjoint_work_bytes(n, plan.depth, T, nsub, 'unit'), f'the sizer does not lay out {splits} sub-step ranges'
        work = torch.empty(need, dtype=torch.uint8, device=DEV)
        plan.unit_adjoint_dev(qc0[0], qf0[0], lat[0], T, dis[0], None if G is None else G[0], None if Gc is None else Gc[0],
                              None if Gf is None else Gf[0], g_lat[0], g_qc[0], g_qf[0], g_coef, work, need, T, nsub)
    elif form == 'batch':
        need = plan.unit_adjoint_batch_work_bytes(M, T, nsub)
        assert need == pr.adjoint_work_bytes(n, plan.depth, T, nsub, 'unit', M), f'the sizer does not lay out {splits} sub-step ranges'
        work = torch.empty(need, dtype=torch.uint8, device=DEV)
        plan.unit_adjoint_batch_dev(M, qc0, qf0, pitch, lat, T, T * n, dis, G, T * n, Gc, Gf, g_lat, g_qc, g_qf, g_coef, work, need, T, nsub)
    else:
        ng = gauges.size
        need = plan.unit_adjoint_gauges_work_bytes(M, ng, T, nsub, g_lat is not None)
        assert need == pr.adjoint_work_bytes(n, plan.depth, T, nsub, 'unit', M, ng, g_lat is not None), \
            f'the sizer does not lay out {splits} sub-step ranges'
        work = torch.empty(need, dtype=torch.uint8, device=DEV)
        gi = torch.tensor(gauges.astype(np.int64), device=DEV)
        dis_g, G_g = dis[:, :, gi].contiguous(), G[:, :, gi].contiguous()
        plan.unit_adjoint_gauges_dev(M, ng, dev(gauges.astype(np.int32)), qc0, qf0, pitch, lat, T, T * n, dis_g, G_g, T * ng, Gc, Gf, g_lat,
                                     g_qc, g_qf, g_coef, work, need, T, nsub)
    out = host(g_coef), host(g_qc)[:, :ni], host(g_qf)[:, :ni], None if g_lat is None else host(g_lat)
    return (*out, time.perf_counter() - t0)


def judge_unit(rs, got, what, lateral=True):
    g_coef, g_qc, g_qf, g_lat, seconds = got
    worst = {}
    orc = rs[0].orc.grad_coef if len(rs) == 1 else sum(r.orc.grad_coef for r in rs[1:]) + rs[0].orc.grad_coef
    exact = rs[0].exact.grad_coef if len(rs) == 1 else pr.member_sum([r.exact.grad_coef for r in rs])
    scale = sum(r.exact.scale_coef for r in rs)
    for j, name in enumerate(('dc1', 'dc2', 'dc3')):
        worst[name] = pr.assert_per_element(g_coef[j], orc[j], exact[j], scale[j], f'{what}: dL/{name}')
    for name, g, field in (('dq_ch0', g_qc, 'qch0'), ('dq_full0', g_qf, 'qfull0')):
        worst[name] = max(pr.assert_per_element(g[m], getattr(r.orc, 'grad_' + field), getattr(r.exact, 'grad_' + field),
                                                getattr(r.exact, 'scale_' + field), f'{what}: member {m} dL/{name}') for m, r in enumerate(rs))
    if lateral:
        worst['dlateral'] = max(pr.assert_per_element(g_lat[m], r.orc.grad_lateral, r.exact.grad_lateral, r.exact.scale_lateral,
                                                      f'{what}: member {m} dL/dlateral') for m, r in enumerate(rs))
    else:
        assert g_lat is None
    report(what, worst, seconds)
    return worst


@pytest.mark.parametrize('case,regime', SINGLE)
def test_unit_every_output(case, regime):
    net, T, nsub, _, expect, _ = pr.ADJ_CASES[case]
    r = pr.unit_adjoint_case(case, regime)
    assert pr.adjoint_splits(r.n, T, nsub) == expect
    if case == 'no edges':
        assert r.ni == 0
    got = unit_run([r], 'single')
    judge_unit([r], got, f'unit {case} / {regime}')


@pytest.mark.parametrize('shared', [False, True], ids=['own states', 'shared states'])
def test_unit_batch(shared):
    net, T, nsub, M, expect, _ = pr.ADJ_CASES['batch']
    rs = [pr.unit_adjoint_case('batch', 'benign', m, 'both', shared and m > 0) for m in range(M)]
    assert pr.adjoint_splits(rs[0].n, T, nsub, M) == expect == (7, 14)
    judge_unit(rs, unit_run(rs, 'batch', shared=shared), f'unit batch of {M}, {"shared" if shared else "own"} states')


@pytest.mark.parametrize('members,with_grad_lateral', [(1, True), (1, False), (3, True), (3, False)])
def test_unit_gauges(members, with_grad_lateral):
    case = 'ragged ranges'
    net, T, nsub, _, _, _ = pr.ADJ_CASES[case]
    rs = [pr.unit_adjoint_case(case, 'benign', m, 'gauges') for m in range(members)]
    assert pr.adjoint_splits(rs[0].n, T, nsub, members) == {1: (71, 5), 3: (28, 13)}[members]
    g = pr.gauge_columns(case)
    assert np.isin(g, rs[0].inner).any() and not np.isin(g, rs[0].inner).all()      # headwaters and inner reaches among them
    got = unit_run(rs, 'gauges', gauges=g, with_grad_lateral=with_grad_lateral)
    judge_unit(rs, got, f'unit {pr.N_GAUGES} gauges, {members} member(s), grad_lateral {with_grad_lateral}', lateral=with_grad_lateral)


@pytest.mark.parametrize('loss', ['final', 'outlet'])
def test_unit_partial_losses(loss):
    r = pr.unit_adjoint_case(pr.PARTIAL_CASE, 'benign', 0, loss)
    judge_unit([r], unit_run([r], 'single'), f'unit partial loss: {loss}')


def test_unit_through_rr_grad_to_k_and_x():
    case = 'ragged ranges'
    r = pr.unit_adjoint_case(case, 'benign')
    plan = Plan(r.indptr, r.indices)
    kt, xt = torch.tensor(r.k, requires_grad=True), torch.tensor(r.x, requires_grad=True)
    latt, qct, qft = dev(r.lat).requires_grad_(), dev(r.q_ch0).requires_grad_(), dev(r.q_full0).requires_grad_()
    dt = pr.DT_RUNOFF / r.nsub
    out, qc, qf = rr.grad.unit_route(plan, qct, qft, latt, kt, xt, dt, pr.DT_RUNOFF)
    assert_mask(host(out.detach()), r.exact.raw, r.inner, 'rr.grad.unit_route')
    ((out * dev(r.G)).sum() + (qc * dev(r.Gc)).sum() + (qf * dev(r.Gf)).sum()).backward()
    worst = {}
    jk, jx = pr.coefficient_jacobian(r.k, r.x, dt, with_c4=False)
    for name, jac, got in (('dk', jk, kt.grad.numpy()), ('dx', jx, xt.grad.numpy())):
        exact, scale = pr.chain_to_kx(jac, r.exact.grad_coef, r.exact.scale_coef)
        orc, _ = pr.chain_to_kx(jac, r.orc.grad_coef, r.exact.scale_coef)
        worst[name] = pr.assert_per_element(got, orc, exact, scale, f'rr.grad.unit_route: dL/{name}')
    for name, got, orc, exact, scale in (('dq_ch0', qct.grad, r.orc.grad_qch0, r.exact.grad_qch0, r.exact.scale_qch0),
                                         ('dq_full0', qft.grad, r.orc.grad_qfull0, r.exact.grad_qfull0, r.exact.scale_qfull0),
                                         ('dlateral', latt.grad, r.orc.grad_lateral, r.exact.grad_lateral, r.exact.scale_lateral)):
        worst[name] = pr.assert_per_element(host(got), orc, exact, scale, f'rr.grad.unit_route: dL/{name}')
    report('rr.grad.unit_route', worst)
