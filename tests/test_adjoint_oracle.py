"""The adjoint arbiter (oracle/rr_oracle_adj.c) earns its trust before a kernel is judged by it (tests/test_gpu_grad_per_reach.py;
DESIGN.md section 2c): against torch autograd through the dense restatements of tests/test_grad.py and tests/test_grad_unit.py with
the coefficients as leaves, judged as `got` under the per-element rule; against central finite differences of the forward oracle,
which know nothing of torch; its structure (scale >= |gradient|, zeros exactly where a gradient is structurally zero, a gauge loss
and a batch as compositions); the rule's teeth; the measurement that fixes K_ADJ and the clamp-margin condition over the whole case
table; and a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer on tiny networks."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import per_reach as pr
import test_grad as cpu
import test_grad_unit as unit
from oracle import oracle
from test_gpu_grad import CASES, assert_grad

HERE = os.path.dirname(os.path.abspath(__file__))
DT_RUNOFF = pr.DT_RUNOFF
# the existing element-wise GPU cases: CASES, then the clamp / negative-c3 case, channel-only and final-state-only of test_gpu_grad.py
RESTATED = [(kind, n, T, nsub, 'both', 0.0) for kind, n, T, nsub in CASES] + \
           [('tree', 200, 24, 1, 'clamp', -1.5), ('forest', 120, 20, 2, 'channel', 0.0), ('forest', 120, 20, 2, 'final', 0.0)]


def small_rapid(kind, n, T, nsub, what, low, seed_shift=0):
    down, k, x = cpu.network(kind, n, seed=n + T + nsub + seed_shift)
    k = k.copy()
    if what == 'clamp':
        k[::3] = 300.0
    rng = np.random.default_rng(n + 17)
    ql = rng.uniform(low, 2.0, (T, n)) * DT_RUNOFF
    q0, G, Gf = rng.uniform(0.0, 3.0, n), rng.standard_normal((T, n)), rng.standard_normal(n)
    if what == 'channel':
        ql = None
    if what == 'final':
        G = None
    c1, c2, c3 = oracle.muskingum_coefficients(k, x, DT_RUNOFF / nsub)
    return down, np.stack([c1, c2, c3, (c1 + c2) / DT_RUNOFF]), ql, q0, G, Gf


@pytest.mark.parametrize('kind,n,T,nsub,what,low', RESTATED)
def test_rapid_restatement_passes_the_rule(kind, n, T, nsub, what, low):
    down, c, ql, q0, G, Gf = small_rapid(kind, n, T, nsub, what, low)
    indptr, indices = pr.csc_from_down(down)
    orc, exact = pr.rapid_adjoint_refs(indptr, indices, c, q0, ql, G, Gf, nsub, T)
    ct = [torch.tensor(v, requires_grad=True) for v in c]
    q0t = torch.tensor(q0, requires_grad=True)
    qlt = None if ql is None else torch.tensor(ql, requires_grad=True)
    d, qf = cpu.dense_route(down, q0t, qlt, *ct, nsub, rows=T)
    assert np.array_equal(d.detach().numpy() > 0, exact.raw > 0), 'the restatement clamps other elements than the arbiter'
    if what == 'clamp':
        assert (c[2] < 0).any() and (exact.raw <= 0).mean() > 0.05
    L = (qf * torch.as_tensor(Gf)).sum() + (0.0 if G is None else (d * torch.as_tensor(G)).sum())
    L.backward()
    z = lambda v: np.zeros(v.shape) if v.grad is None else v.grad.numpy()      # noqa: E731
    for j in range(4):
        pr.assert_per_element(z(ct[j]), orc.grad_coef[j], exact.grad_coef[j], exact.scale_coef[j], f'restatement dL/dc{j + 1}')
    pr.assert_per_element(z(q0t), orc.grad_q0, exact.grad_q0, exact.scale_q0, 'restatement dL/dq0')
    if ql is not None:
        pr.assert_per_element(z(qlt), orc.grad_lateral, exact.grad_lateral, exact.scale_lateral, 'restatement dL/dlateral')
    else:
        assert not exact.grad_coef[3].any() and not exact.scale_coef[3].any()      # dL/dc4dt of a channel-only call


def small_unit(kind, n, T, nsub, what, low):
    down, k, x = cpu.network(kind, n, seed=n + T + nsub)
    k = k.copy()
    if what == 'clamp':
        k[::3] = 300.0
    d = unit.unit_inputs(down, T, n + 17, low=low)
    if what == 'final':
        d['G'] = None
    return down, np.stack(oracle.muskingum_coefficients(k, x, DT_RUNOFF / nsub)), d


def unit_refs(down, c, d, nsub):
    indptr, indices = pr.csc_from_down(down)
    args = (indptr, indices, c[0], c[1], c[2], d['q_ch0'], d['q_full0'], d['lat'], d['G'], d['Gc'], d['Gf'], nsub)
    return oracle.unit_adjoint(*args), oracle.unit_adjoint_ld(*args)


@pytest.mark.parametrize('kind,n,T,nsub,what,low', [c for c in RESTATED if c[4] != 'channel'])
def test_unit_restatement_passes_the_rule(kind, n, T, nsub, what, low):
    down, c, d = small_unit(kind, n, T, nsub, what, low)
    orc, exact = unit_refs(down, c, d, nsub)
    ct = [torch.tensor(v, requires_grad=True) for v in c]
    t = {key: torch.tensor(d[key], requires_grad=True) for key in ('lat', 'q_ch0', 'q_full0')}
    out, qc, qf = unit.dense_unit_route(down, t['q_ch0'], t['q_full0'], t['lat'], *ct, nsub)
    inner = pr.inner_reaches(down)
    assert np.array_equal(out.detach().numpy()[:, inner] > 0, exact.raw[:, inner] > 0), 'the restatement clamps other elements than the arbiter'
    L = (qc * torch.as_tensor(d['Gc'])).sum() + (qf * torch.as_tensor(d['Gf'])).sum()
    if d['G'] is not None:
        L = L + (out * torch.as_tensor(d['G'])).sum()
    if not L.requires_grad:      # a network without inner reaches and without dL/ddischarge: nothing depends on anything
        assert inner.size == 0 and not exact.grad_lateral.any()
        return
    L.backward()
    z = lambda v: np.zeros(v.shape) if v.grad is None else v.grad.numpy()      # noqa: E731
    for j in range(3):
        pr.assert_per_element(z(ct[j]), orc.grad_coef[j], exact.grad_coef[j], exact.scale_coef[j], f'restatement dL/dc{j + 1}')
    pr.assert_per_element(z(t['q_ch0']), orc.grad_qch0, exact.grad_qch0, exact.scale_qch0, 'restatement dL/dq_ch0')
    pr.assert_per_element(z(t['q_full0']), orc.grad_qfull0, exact.grad_qfull0, exact.scale_qfull0, 'restatement dL/dq_full0')
    pr.assert_per_element(z(t['lat']), orc.grad_lateral, exact.grad_lateral, exact.scale_lateral, 'restatement dL/dlateral')


def test_unit_closed_form_of_the_kernel_header_passes_the_rule():
    """tests/test_grad_unit.closed_form_unit_adjoint is the kernel header's recursion in numpy loops, written before this arbiter."""
    down, c, d = small_unit('forest', 80, 9, 2, 'clamp', -1.5)
    orc, exact = unit_refs(down, c, d, 2)
    g, _ = unit.closed_form_unit_adjoint(down, d['q_ch0'], d['q_full0'], d['lat'], c[0], c[1], c[2], 2, d['G'], d['Gc'], d['Gf'])
    for j in range(3):
        pr.assert_per_element(g[f'c{j + 1}'], orc.grad_coef[j], exact.grad_coef[j], exact.scale_coef[j], f'closed form dL/dc{j + 1}')
    pr.assert_per_element(g['q_ch0'], orc.grad_qch0, exact.grad_qch0, exact.scale_qch0, 'closed form dL/dq_ch0')
    pr.assert_per_element(g['q_full0'], orc.grad_qfull0, exact.grad_qfull0, exact.scale_qfull0, 'closed form dL/dq_full0')
    pr.assert_per_element(g['lat'], orc.grad_lateral, exact.grad_lateral, exact.scale_lateral, 'closed form dL/dlateral')


# ------------------------------------------------------------------------------------------------ finite differences of the forward oracle

def central(loss, arrays, which, at, h):
    hi, lo = [a.copy() for a in arrays], [a.copy() for a in arrays]
    hi[which][at] += h
    lo[which][at] -= h
    return (loss(*hi) - loss(*lo)) / (2 * h)


@pytest.mark.parametrize('kind,nsub', [('tree', 1), ('forest', 2), ('chain', 4)])
def test_rapid_arbiter_matches_finite_differences_of_the_forward_oracle(kind, nsub):
    n, T = 40, 6
    down, k, x = cpu.network(kind, n, seed=7)
    rng = np.random.default_rng(11)
    ql = rng.uniform(0.2, 2.0, (T, n)) * DT_RUNOFF       # positive: no clamp kink inside the differences
    q0, G, Gf = rng.uniform(0.5, 3.0, n), rng.standard_normal((T, n)), rng.standard_normal(n)
    c1, c2, c3 = oracle.muskingum_coefficients(k, x, DT_RUNOFF / nsub)
    c = [c1, c2, c3, (c1 + c2) / DT_RUNOFF]
    indptr, indices = pr.csc_from_down(down)

    def loss(c1_, c2_, c3_, c4_, q0_, ql_):
        q, d = q0_.copy(), np.zeros((T, n))
        oracle.rapid_route(indptr, indices, -c1_[indices], c2_, c3_, c4_, q, ql_, d, nsub)
        return float((G * d).sum() + (Gf * q).sum())

    exact = oracle.rapid_adjoint_ld(indptr, indices, *c, q0, ql, G, Gf, nsub)
    assert (exact.raw > 0).all()
    arrays = [*c, q0, ql]
    has_up = pr.inner_reaches(down)
    for j in range(4):
        for i in (int(has_up[0]), int(has_up[has_up.size // 2]), n - 1):
            fd = central(loss, arrays, j, i, 1e-6 * max(abs(c[j][i]), 1e-3))
            assert abs(fd - exact.grad_coef[j, i]) <= 1e-6 * max(abs(fd), np.abs(exact.grad_coef[j]).max()), (j, i, fd, exact.grad_coef[j, i])
    for i in (0, n // 2, n - 1):
        fd = central(loss, arrays, 4, i, 1e-3)
        assert abs(fd - exact.grad_q0[i]) <= 1e-6 * max(abs(fd), np.abs(exact.grad_q0).max()), (i, fd, exact.grad_q0[i])
    for at in ((0, 0), (T // 2, n // 3), (T - 1, n - 1)):
        fd = central(loss, arrays, 5, at, 1e-3 * ql[at])
        assert abs(fd - exact.grad_lateral[at]) <= 1e-6 * max(abs(fd), np.abs(exact.grad_lateral).max()), (at, fd, exact.grad_lateral[at])


@pytest.mark.parametrize('kind,nsub', [('tree', 1), ('forest', 2), ('chain', 4)])
def test_unit_arbiter_matches_finite_differences_of_the_forward_oracle(kind, nsub):
    from tests_support import unit_split_arrays
    n, T = 40, 6
    down, k, x = cpu.network(kind, n, seed=7)
    d = unit.unit_inputs(down, T, 11, low=0.2)            # positive: no clamp kink inside the differences
    c = list(oracle.muskingum_coefficients(k, x, DT_RUNOFF / nsub))
    indptr, indices = pr.csc_from_down(down)
    hw_idx, inner_idx, A_in, A_hw = unit_split_arrays(indptr, indices, n)

    def loss(c1_, c2_, c3_, qc_, qf_, lat_):
        c1i, c2i, c3i = c1_[inner_idx], c2_[inner_idx], c3_[inner_idx]
        qc, qf, out = qc_.copy(), qf_.copy(), np.zeros((T, n))
        oracle.unit_route(A_in.indptr, A_in.indices, -c1i[A_in.indices], A_in.indptr, A_in.indices, A_in.data, A_hw.indptr, A_hw.indices,
                          A_hw.data, c1i, c2i, c3i, hw_idx, inner_idx, qc, qf, lat_, out, nsub)
        return float((d['G'] * out).sum() + (d['Gc'] * qc).sum() + (d['Gf'] * qf).sum())

    exact = oracle.unit_adjoint_ld(indptr, indices, *c, d['q_ch0'], d['q_full0'], d['lat'], d['G'], d['Gc'], d['Gf'], nsub)
    assert np.array_equal(inner_idx, pr.inner_reaches(down)) and (exact.raw > 0).all()
    arrays = [*c, d['q_ch0'], d['q_full0'], d['lat']]
    picks = (0, inner_idx.size // 2, inner_idx.size - 1)
    for j in range(3):
        for kk in picks:
            i = int(inner_idx[kk])
            fd = central(loss, arrays, j, i, 1e-6 * max(abs(c[j][i]), 1e-3))
            assert abs(fd - exact.grad_coef[j, i]) <= 1e-6 * max(abs(fd), np.abs(exact.grad_coef[j]).max()), (j, i, fd, exact.grad_coef[j, i])
    for which, got in ((3, exact.grad_qch0), (4, exact.grad_qfull0)):
        for kk in picks:
            fd = central(loss, arrays, which, kk, 1e-3)
            assert abs(fd - got[kk]) <= 1e-6 * max(abs(fd), np.abs(got).max()), (which, kk, fd, got[kk])
    for at in ((0, 0), (T // 2, n // 3), (T - 1, n - 1), (1, int(hw_idx[0])), (2, int(inner_idx[0]))):
        fd = central(loss, arrays, 5, at, 1e-3 * d['lat'][at])
        assert abs(fd - exact.grad_lateral[at]) <= 1e-6 * max(abs(fd), np.abs(exact.grad_lateral).max()), (at, fd, exact.grad_lateral[at])


# ------------------------------------------------------------------------------------------------ structure

def test_rapid_structure():
    r = pr.rapid_adjoint_case('fan-in comb', 'clamp')
    down = pr.network('comb')[0]
    headwater = np.setdiff1d(np.arange(r.n), pr.inner_reaches(down))
    for side in (r.orc, r.exact):
        for g, s in ((side.grad_coef, side.scale_coef), (side.grad_q0, side.scale_q0), (side.grad_lateral, side.scale_lateral)):
            assert (s >= np.abs(g)).all() and np.isfinite(s).all()
        # a headwater has no tributaries: nothing ever multiplies its c1 or c2
        assert not side.grad_coef[:2, headwater].any() and not side.scale_coef[:2, headwater].any()
        assert (side.scale_coef[:2, pr.inner_reaches(down)] > 0).all() and (side.scale_coef[2:] > 0).all()
    ch = pr.rapid_adjoint_case(pr.PARTIAL_CASE, 'benign', 0, 'channel')
    assert not ch.exact.grad_coef[3].any() and not ch.exact.scale_coef[3].any() and ch.exact.grad_lateral is None


def test_unit_structure():
    r = pr.unit_adjoint_case('fan-in comb', 'clamp')
    headwater = np.setdiff1d(np.arange(r.n), r.inner)
    for side in (r.orc, r.exact):
        for g, s in ((side.grad_coef, side.scale_coef), (side.grad_qch0, side.scale_qch0), (side.grad_qfull0, side.scale_qfull0),
                     (side.grad_lateral, side.scale_lateral)):
            assert (s >= np.abs(g)).all() and np.isfinite(s).all()
        assert not side.grad_coef[:, headwater].any() and not side.scale_coef[:, headwater].any()      # their coefficients are never read
        assert (side.scale_coef[:, r.inner] > 0).all()
        outlet = r.inner == r.n - 1
        assert not side.grad_qfull0[outlet].any() and not side.scale_qfull0[outlet].any()      # nothing reads the outlet's q_full0
    lone = pr.unit_adjoint_case('no edges', 'benign')
    assert lone.ni == 0 and np.array_equal(lone.exact.grad_lateral, lone.G) and not lone.exact.grad_coef.any()


def test_a_gauge_loss_is_a_cotangent_that_is_zero_off_the_gauges():
    """The gauge columns hold headwaters and inner reaches; and, the adjoint being linear in its cotangents over one forward run, the
    gauge loss and the loss over every other column add up to the full one, element by element under the rule."""
    case = 'ragged ranges'
    r = pr.rapid_adjoint_case(case, 'benign', 0, 'gauges')
    g = pr.gauge_columns(case)
    down = pr.network('random')[0]
    off = np.setdiff1d(np.arange(r.n), g)
    hw = np.setdiff1d(np.arange(r.n), pr.inner_reaches(down))
    assert g.size == pr.N_GAUGES and not r.G[:, off].any() and r.G[:, g].all()
    assert np.isin(g, hw).any() and np.isin(g, pr.inner_reaches(down)).any() and g[0] == r.n - 1
    full = pr.rapid_adjoint_case(case, 'benign', 0, 'both')
    rest = full.G - r.G
    _, other = pr.rapid_adjoint_refs(r.indptr, r.indices, r.c, r.q0, r.ql, rest, None, r.nsub)
    for (name, orc, exact, scale), a, b, sa, sb in zip(pr.rapid_outputs(full),
                                                       [*r.exact.grad_coef, r.exact.grad_q0, r.exact.grad_lateral],
                                                       [*other.grad_coef, other.grad_q0, other.grad_lateral],
                                                       [*r.exact.scale_coef, r.exact.scale_q0, r.exact.scale_lateral],
                                                       [*other.scale_coef, other.scale_q0, other.scale_lateral]):
        pr.assert_per_element(a + b, orc, exact, np.maximum(scale, sa + sb), f'gauges + the rest: {name}')


def test_a_batch_is_a_loop_over_its_members():
    members = [pr.rapid_adjoint_case('batch', 'benign', m) for m in range(4)]
    total = pr.member_sum([m.exact.grad_coef for m in members])
    scale = sum(m.exact.scale_coef for m in members)
    orc = sum(m.orc.grad_coef for m in members[1:]) + members[0].orc.grad_coef
    assert (scale >= np.abs(total)).all()
    for j in range(4):
        assert pr.assert_per_element(orc[j], orc[j], total[j], scale[j], f'members summed in fp64, row {j}') <= 1.0
    assert not np.array_equal(members[0].ql, members[1].ql) and not np.array_equal(members[0].q0, members[1].q0)
    assert np.array_equal(pr.rapid_adjoint_case('batch', 'benign', 1, 'both', True).q0, members[0].q0)


# ------------------------------------------------------------------------------------------------ the rule has teeth

def test_the_rule_fails_what_the_global_tolerance_passes():
    r = pr.rapid_adjoint_case(pr.PARTIAL_CASE, 'benign', 0, 'outlet')
    name, orc, exact, scale = pr.rapid_outputs(r)[4]
    assert name == 'dL/dq0'
    live = np.flatnonzero(scale > 0)
    mag = np.abs(exact[live])
    assert mag.max() / mag[mag > 0].min() >= 1e3, 'the case should span at least three decades'
    unit_ = max(pr.element_error(orc, exact, scale), pr.EPS)
    assert pr.assert_per_element(orc, orc, exact, scale, name) <= 1.0
    # 64 units at one element: four times what the rule allows
    big = int(live[np.argmax(mag)])
    got = orc.copy()
    got[big] = exact[big] + 64 * unit_ * scale[big]
    with pytest.raises(AssertionError, match='off by'):
        pr.assert_per_element(got, orc, exact, scale, name)
    # a small-gradient element wrong by 1e-10 of the largest gradient: inside today's global tolerance, far outside its own scale
    small = int(live[np.argmin(np.abs(np.log10(np.where(mag > 0, mag, 1e300)) - np.log10(1e-6 * mag.max())))])
    assert 0 < scale[small] <= 1e-3 * mag.max()
    got = orc.copy()
    got[small] += 1e-10 * mag.max()
    assert_grad(got, exact, 'the global tolerance')
    with pytest.raises(AssertionError, match='off by'):
        pr.assert_per_element(got, orc, exact, scale, name)
    # and a value where the gradient is structurally zero
    down = pr.network(pr.ADJ_CASES[pr.PARTIAL_CASE][0])[0]
    hw = int(np.setdiff1d(np.arange(r.n), pr.inner_reaches(down))[0])
    got = r.orc.grad_coef[0].copy()
    got[hw] = 1e-300
    with pytest.raises(AssertionError, match='structurally zero'):
        pr.assert_per_element(got, r.orc.grad_coef[0], r.exact.grad_coef[0], r.exact.scale_coef[0], 'dL/dc1')


# ------------------------------------------------------------------------------------------------ K and the clamp margin, over the case table

@pytest.fixture(scope='module')
def reordered(tmp_path_factory):
    return oracle.build_adjoint_reordered(str(tmp_path_factory.mktemp('adjoint_reordered')))


def _rule_k(worst):
    """Section 2c: 16, the forward rule's value, if three times the worst measured ratio is within it; else the next power of two above."""
    return 16.0 if 3.0 * worst <= 16.0 else float(2 ** int(np.floor(np.log2(3.0 * worst)) + 1))


def test_k_and_the_clamp_margin_over_the_case_table(reordered):
    """Every definition of the table at its own size: a second correctly rounded fp64 evaluation (reverse summation order, fused
    multiply-adds) sets the measured ratio K_ADJ follows from; no unclamped mean sits within the forward bound of zero; the clamp
    regimes clamp more than 5 % of the outputs; every case has the sub-step ranges the table says.  Prints one line per definition."""
    worst, lines = 0.0, []
    for case, regime, member, loss, shared in pr.every_case():
        net, T, nsub, members, expect, _ = pr.ADJ_CASES[case]
        n = pr.network(net)[0].size
        assert pr.adjoint_splits(n, T, nsub, members) == expect, f'{case}: the table\'s sub-step ranges'
        for router in ('rapid', 'unit'):
            if router == 'unit' and loss == 'channel':
                continue
            if router == 'rapid':
                r = pr.rapid_adjoint_case(case, regime, member, loss, shared)
                alt = oracle.rapid_adjoint(r.indptr, r.indices, *r.c, r.q0, r.ql, r.G, r.Gf, r.nsub, r.T, lib_=reordered)
                outs = [(nm, a, o, e, s) for (nm, o, e, s), a in zip(pr.rapid_outputs(r), [*alt.grad_coef, alt.grad_q0, alt.grad_lateral])]
            else:
                r = pr.unit_adjoint_case(case, regime, member, loss, shared)
                alt = oracle.unit_adjoint(r.indptr, r.indices, *r.c, r.q_ch0, r.q_full0, r.lat, r.G, r.Gc, r.Gf, r.nsub, lib_=reordered)
                outs = [(nm, a, o, e, s) for (nm, o, e, s), a in
                        zip(pr.unit_outputs(r), [*alt.grad_coef, alt.grad_qch0, alt.grad_qfull0, alt.grad_lateral])]
            near, clamped = pr.forward_margin(r.orc.raw, r.exact.raw)
            assert near == 0, f'{router} {case} / {regime}: {near} unclamped means within the forward bound of zero -- choose another seed'
            assert np.array_equal(r.orc.raw > 0, r.exact.raw > 0) and np.array_equal(alt.raw > 0, r.exact.raw > 0)
            if regime == 'clamp':
                assert clamped > 0.05, f'{router} {case}: the clamp is active on {clamped:.1%} of the outputs only'
            ratios = []
            for nm, a, o, e, s in outs:
                assert not ((s > 0) & (s < 2.0 ** -970)).any(), f'{router} {case} {nm}: a scale so small that 2^-52 of it is no double'
                ratios.append(pr.assert_per_element(a, o, e, s, f'{router} {case} / {regime} reordered {nm}', K=np.inf))
                e_orc = pr.element_error(o, e, s)
                lines.append(f'{router:5s} {case:18s} {regime:6s} m{member} {loss:7s} {"shared" if shared else "own":6s} {nm:12s} '
                             f'E_orc {e_orc / pr.EPS:8.2f} eps  reordered {ratios[-1]:6.2f}')
            worst = max(worst, max(ratios))
    print('\n'.join(lines))
    print(f'worst reordered ratio {worst:.3f}; K by the rule {_rule_k(worst):g}')
    assert pr.K_ADJ == _rule_k(worst), f'K_ADJ {pr.K_ADJ:g} is not what the measured worst ratio {worst:.3f} gives: {_rule_k(worst):g}'


# ------------------------------------------------------------------------------------------------ the C file under the sanitizers

def test_stand_alone_program_under_the_sanitizers(tmp_path):
    cc = shutil.which('gcc') or shutil.which('cc')
    assert cc, 'no C compiler on the path'
    exe = str(tmp_path / 'adjoint_oracle_main')
    subprocess.run([cc, '-std=c11', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-o', exe,
                    os.path.join(HERE, 'adjoint_oracle_main.c'), os.path.join(os.path.dirname(oracle.__file__), 'rr_oracle_adj.c'), '-lm'],
                   check=True, capture_output=True, text=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == '', f'exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}'
    assert r.stdout.strip().endswith('adjoint oracle: all cases ok'), r.stdout[-2000:]


def test_a_platform_without_extended_precision_fails_the_build():
    src = os.path.join(os.path.dirname(oracle.__file__), 'rr_oracle_adj.c')
    narrow = subprocess.run(['gcc', '-std=c11', '-mlong-double-64', '-fsyntax-only', src], capture_output=True, text=True)
    assert narrow.returncode != 0 and 'long double' in narrow.stderr
