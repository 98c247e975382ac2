"""gauges= of rr.grad.unit_route, unit_route_batch, unit_muskingum and unit_muskingum_batch on the GPU (rr_unit_adjoint_gauges_dev: the
slot map kernels, k_adj_mask_unit_gauges over the (T, G) blocks, the gauge form of k_adj_tick_unit in its four instantiations,
k_adj_rows_unit_gauges and its member form).  The gauge path and the dense path with the loss on discharge[..., gauges] perform the
same floating-point operations on the same values (a position without a gauge reads the 0.0 the dense cotangent holds there), so every
output is compared with np.array_equal; against the pure-torch restatement of tests/test_grad_unit.py, whose cotangent is scattered
to full width, the tolerance is the project's 1e-9.  Windows, members, the composite functions, repeat runs, the work memory and its
refusals, the scores on top, and the peak memory of a backward pass."""
import numpy as np
import pytest
import torch

import river_route_amd as rr
import test_grad as cpu
import test_grad_unit as unit
from oracle import oracle
from river_route_amd import _lib, synth
from river_route_amd.engine import DeviceBuffer, Plan
from test_gpu_grad_gauges import scrambled_gauges
from test_gpu_grad_unit import _default_knobs, assert_grad, dev  # noqa: F401  (the fixture resets the engine's knobs)
from test_gpu_grad_unit_batch import DEV, DT_RUNOFF, FULL_IN, ROUTE_IN, WEIGHTS, in_member_order, make_plan, members_inputs, numpy_of, stacked

pytestmark = pytest.mark.gpu
OUTPUTS = ('out', 'q_ch', 'q_full', 'uh_state')


def run(plan, k, x, ds, nsub, gauges, use_gauges, full=False, batch=False, weights=None, need=None, shared=(), **kw):
    """L = sum of (weights x output) with the discharge read at `gauges` (its weights: the first G columns of 'G'): through gauges=
    (use_gauges) or through the dense call and an indexed view of its discharge.  ds: one member's dict, or with `batch` the members';
    full: the convolution chained in; need: the inputs that require grad (None: all); shared: states given once for all members.
    Outputs and gradients as numpy by name, the discharge at the gauges as 'out'; None for a gradient autograd did not produce."""
    names = FULL_IN if full else ROUTE_IN
    need = set(('k', 'x') + names) if need is None else set(need)
    weights = tuple(w for _, w in WEIGHTS[:4 if full else 3]) if weights is None else weights
    kt, xt = torch.tensor(k, requires_grad='k' in need), torch.tensor(x, requires_grad='x' in need)
    first = ds[0] if batch else ds

    def value(key):
        if not batch or key == 'kernel' or key in shared:
            return first[key]
        return stacked(ds, key)

    t = {key: dev(value(key), key in need) for key in names}
    f = getattr(rr.grad, ('unit_muskingum' if full else 'unit_route') + ('_batch' if batch else ''))
    args = (plan, t['q_ch0'], t['q_full0'], t['lat']) + ((t['kernel'], t['state']) if full else ()) + (kt, xt, DT_RUNOFF / nsub, DT_RUNOFF)
    if use_gauges:
        outs = f(*args, gauges=gauges, **kw)
    else:
        outs = f(*args, **kw)
        outs = (outs[0][..., torch.as_tensor(np.asarray(gauges), dtype=torch.int64, device=DEV)], *outs[1:])
    L = 0.0
    for v, (_, w) in zip(outs, WEIGHTS):
        if w in weights:
            W = stacked(ds, w) if batch else ds[w]
            L = L + (v * dev(np.ascontiguousarray(W[..., :len(gauges)]) if w == 'G' else W)).sum()
    L.backward()
    res = {key: None if v.grad is None else numpy_of(v.grad) for key, v in (('k', kt), ('x', xt), *t.items())}
    res.update({name: numpy_of(v) for v, name in zip(outs, OUTPUTS)})
    return res


def assert_same(got, want, what):
    assert got.keys() == want.keys(), what
    for name in got:
        g, w = got[name], want[name]
        assert (g is None) == (w is None), f'{what}: {name}'
        if g is not None:
            assert g.shape == w.shape and np.array_equal(g, w), f'{what}: {name}'


def assert_paths_equal(plan, k, x, ds, nsub, gauges, what, **kw):
    """Both paths on one plan; every output and gradient np.array_equal.  Returns the gauge path's."""
    got = run(plan, k, x, ds, nsub, gauges, True, **kw)
    assert got['out'].shape[-1] == len(gauges)
    assert_same(got, run(plan, k, x, ds, nsub, gauges, False, **kw), what)
    return got


# ---- 1. equal to the dense path; the headwater rule ----

@pytest.mark.parametrize('nsub', [1, 2, 3])
def test_equal_to_dense_path(nsub):
    n, T = 500, 30
    down, k, x = cpu.network('forest', n, seed=8)
    d = unit.unit_inputs(down, T, 40 + nsub, low=-1.5)      # negative lateral inflow: inner gauges clamp
    gauges = scrambled_gauges(down)
    hw, inner = unit.split(down)
    plan = make_plan(down)
    got = assert_paths_equal(plan, k, x, d, nsub, gauges, f'forest nsub={nsub}')
    is_inner = np.isin(gauges, inner)
    assert (~is_inner).any()                                                                  # a headwater
    assert (got['out'][:, is_inner] <= 0).any() and (got['out'][:, is_inner] > 0).any()       # inner: a clamped and an unclamped element
    assert np.abs(got['k']).max() > 0 and np.abs(got['lat']).max() > 0
    # the rule this form exists for: a loss on one headwater gauge alone leaves every mu zero, so its dL/dlateral column is the
    # cotangent itself -- not divided by nsub, not clamped (its lateral inflow is negative somewhere) -- and every other column is zero
    j = int(np.flatnonzero(~is_inner)[0])
    h = int(gauges[j])
    assert (d['lat'][:, h] < 0).any()
    lone = dict(d, G=np.zeros_like(d['G']))
    lone['G'][:, j] = d['G'][:, j]
    got = assert_paths_equal(plan, k, x, lone, nsub, gauges, f'headwater alone nsub={nsub}', weights=('G',))
    assert np.array_equal(got['lat'][:, h], d['G'][:, j])
    assert not np.delete(got['lat'], h, axis=1).any() and not got['k'].any()


# ---- 2. all reaches as gauges ----

def test_all_reaches_reversed():
    n, T, nsub = 500, 30, 2
    down, k, x = cpu.network('forest', n, seed=8)
    d = unit.unit_inputs(down, T, 51, low=-1.5)
    rev = np.arange(n)[::-1].copy()
    plan = make_plan(down)
    got = assert_paths_equal(plan, k, x, d, nsub, rev, 'G = n reversed')
    # and against the dense call proper, its columns reversed back
    kt, xt = torch.tensor(k, requires_grad=True), torch.tensor(x, requires_grad=True)
    t = {key: dev(d[key], True) for key in ROUTE_IN}
    out, qc, qf = rr.grad.unit_route(plan, t['q_ch0'], t['q_full0'], t['lat'], kt, xt, DT_RUNOFF / nsub, DT_RUNOFF)
    ((out * dev(d['G'][:, ::-1].copy())).sum() + (qc * dev(d['Gc'])).sum() + (qf * dev(d['Gf'])).sum()).backward()
    want = dict(k=kt.grad.numpy(), x=xt.grad.numpy(), **{key: numpy_of(v.grad) for key, v in t.items()},
                out=numpy_of(out)[:, ::-1], q_ch=numpy_of(qc), q_full=numpy_of(qf))
    assert_same(got, want, 'against the dense call proper')


# ---- 3. minimal shapes ----

def test_one_reach_one_row_one_gauge():
    # a lone headwater: no inner reach, no state, no tick; the row pass alone takes the block to grad_lateral
    down, k, x = cpu.network('postorder', 1, seed=5)
    d = unit.unit_inputs(down, 1, 52, low=0.5)
    plan = make_plan(down)
    assert plan.n_inner == 0
    got = assert_paths_equal(plan, k, x, d, 1, np.array([0]), 'n = T = G = 1')
    assert np.array_equal(got['lat'], d['G'])
    d = unit.unit_inputs(down, 1, 52, low=-1.5)
    d['lat'][:] = -3.0      # a negative headwater discharge is not clamped either
    got = assert_paths_equal(plan, k, x, d, 3, np.array([0]), 'n = T = G = 1, nsub = 3')
    assert np.array_equal(got['lat'], d['G'])


def test_chain_four_substeps():
    n, T, nsub = 40, 10, 4
    down, k, x = cpu.network('chain', n, seed=6)
    d = unit.unit_inputs(down, T, 53, low=-3.0)
    hw, inner = unit.split(down)
    gauges = np.array([int(np.flatnonzero(down < 0)[0]), int(hw[0]), 17])      # the outlet, the head, the middle
    assert hw.size == 1 and np.unique(gauges).size == 3
    got = assert_paths_equal(make_plan(down), k, x, d, nsub, gauges, 'chain nsub=4')
    assert (got['out'][:, [0, 2]] <= 0).any() and (got['out'][:, [0, 2]] > 0).any()


@pytest.mark.parametrize('kind', ['headwaters', 'inner'])
def test_gauges_of_one_kind(kind):
    n, T, nsub = 120, 20, 2
    down, k, x = cpu.network('forest', n, seed=9)
    d = unit.unit_inputs(down, T, 54, low=-1.5)
    hw, inner = unit.split(down)
    gauges = (hw if kind == 'headwaters' else inner)[::-3][:9].copy()      # descending
    assert gauges.size == 9
    got = assert_paths_equal(make_plan(down), k, x, d, nsub, gauges, f'all gauges {kind}')
    if kind == 'inner':
        assert (got['out'] <= 0).any() and (got['out'] > 0).any()


# ---- 4. which inputs require grad ----

def test_which_inputs_require_grad():
    n, T, nsub = 120, 20, 2
    down, k, x = cpu.network('forest', n, seed=9)
    d = unit.unit_inputs(down, T, 55, low=-1.5)
    gauges = scrambled_gauges(down)
    plan = make_plan(down)
    # only the states: grad_coef is NULL, no replay runs and no tape is written
    got = assert_paths_equal(plan, k, x, d, nsub, gauges, 'states only', need=('q_ch0', 'q_full0'))
    assert got['k'] is None and got['x'] is None and got['lat'] is None and np.abs(got['q_ch0']).max() > 0 and np.abs(got['q_full0']).max() > 0
    # only k and x: the work memory has no gradient rows and the row pass does not run
    got = assert_paths_equal(plan, k, x, d, nsub, gauges, 'k and x only', need=('k', 'x'))
    assert got['lat'] is None and got['q_ch0'] is None and np.abs(got['k']).max() > 0 and np.abs(got['x']).max() > 0
    # only the lateral rows: no replay, the row pass reads the blocks
    got = assert_paths_equal(plan, k, x, d, nsub, gauges, 'lateral only', need=('lat',))
    assert got['k'] is None and np.abs(got['lat']).max() > 0
    # a loss on the final states alone: no discharge gradient reaches the adjoint (discharge_g and grad_out_g are both NULL)
    got = assert_paths_equal(plan, k, x, d, nsub, gauges, 'final states only', weights=('Gc', 'Gf'))
    assert np.abs(got['k']).max() > 0 and np.abs(got['lat']).max() > 0


# ---- 5. against independent truth ----

@pytest.mark.parametrize('kind,n,T,nsub,low', [('tree', 300, 12, 2, -0.5), ('forest', 500, 8, 3, 0.0)])
def test_gradients_match_restatement(kind, n, T, nsub, low):
    down, k, x = cpu.network(kind, n, seed=n + T)
    d = unit.unit_inputs(down, T, n + 3, low=low)
    gauges = scrambled_gauges(down)
    full = dict(d, G=np.zeros((T, n)))
    full['G'][:, gauges] = d['G'][:, :7]      # the cotangent scattered to full width
    got = run(make_plan(down), k, x, d, nsub, gauges, True)
    want = unit.dense_unit_loss_grads(down, k, x, full, DT_RUNOFF / nsub, nsub)
    for name in ('k', 'x', 'lat', 'q_ch0', 'q_full0'):
        assert_grad(got[name], want[name], f'{kind} n={n}: d/d{name}')


# ---- 6. windows ----

def test_windows_equal_one_call():
    n, T, nsub = 500, 30, 2
    down, k, x = cpu.network('forest', n, seed=8)
    d = unit.unit_inputs(down, T, 6)
    gauges = scrambled_gauges(down)
    plan = make_plan(down)
    one = run(plan, k, x, d, nsub, gauges, True)
    win = run(plan, k, x, d, nsub, gauges, True, rows_per_window=7)
    assert win['out'].shape == (T, 7)
    for name in one:
        assert_grad(win[name], one[name], f'windows: {name}', rtol=1e-12)


# ---- 7. members ----

@pytest.mark.parametrize('shared', [(), ('q_ch0', 'q_full0')], ids=['own states', 'shared states'])
def test_batch_members_match_single_gauge_calls(shared):
    n, T, nsub, B = 300, 16, 2, 3
    down, k, x = cpu.network('forest', n, seed=12)
    gauges = scrambled_gauges(down)
    ds = members_inputs(down, B, T, 60, low=-1.5)
    if shared:
        for m in range(1, B):
            ds[m]['q_ch0'], ds[m]['q_full0'] = ds[0]['q_ch0'], ds[0]['q_full0']
    plan = make_plan(down)
    got = run(plan, k, x, ds, nsub, gauges, True, batch=True, shared=shared, members_per_sweep=2)      # groups of 2 and 1
    assert got['out'].shape == (B, T, 7) and got['q_ch'].shape == (B, plan.n_inner)
    one = [run(plan, k, x, ds[m], nsub, gauges, True) for m in range(B)]
    for m in range(B):
        for name in ('out', 'q_ch', 'q_full', 'lat') + (() if shared else ('q_ch0', 'q_full0')):
            assert np.array_equal(got[name][m], one[m][name]), f'member {m}: {name}'
    for name in ('k', 'x') + tuple(shared):      # one state for all: autograd adds the members' rows, in an order of its own
        assert_grad(got[name], in_member_order([o[name] for o in one]), f'{name} against the member-ordered sum', rtol=1e-12)


def test_batch_of_one_is_the_single_call():
    n, T, nsub = 300, 16, 3
    down, k, x = cpu.network('forest', n, seed=12)
    gauges = scrambled_gauges(down)
    d = unit.unit_inputs(down, T, 61, low=-1.5)
    plan = make_plan(down)
    got = run(plan, k, x, [d], nsub, gauges, True, batch=True)
    want = run(plan, k, x, d, nsub, gauges, True)
    for name in want:
        g = got[name] if name in ('k', 'x') else got[name][0]
        assert np.array_equal(g, want[name]), name


# ---- 8. the composite functions ----

@pytest.mark.parametrize('batch', [False, True], ids=['unit_muskingum', 'unit_muskingum_batch'])
def test_composite_functions(batch):
    n, T, nsub, n_ks, B = 500, 12, 2, 3, 2
    down, k, x = cpu.network('forest', n, seed=8)
    gauges = scrambled_gauges(down)
    ds = members_inputs(down, B, T, 62, low=-0.5, n_ks=n_ks)
    plan = make_plan(down)
    kw = dict(members_per_sweep=1) if batch else {}
    got = assert_paths_equal(plan, k, x, ds if batch else ds[0], nsub, gauges, 'composite', full=True, batch=batch, **kw)
    for name in ('kernel', 'lat', 'state', 'k'):      # 'lat' holds the runoff depths here
        assert np.abs(got[name]).max() > 0, name
    win = assert_paths_equal(plan, k, x, ds if batch else ds[0], nsub, gauges, 'composite in windows', full=True, batch=batch, rows_per_window=5,
                             **kw)
    assert win['out'].shape == got['out'].shape      # each window gathered its own rows


# ---- 9. repeatability ----

def test_two_backward_passes_bit_identical():
    n, T, nsub = 5000, 40, 1
    net = synth.synth_network(n, seed=12)
    down = net.down_index.astype(np.int64)
    d = unit.unit_inputs(down, T, 13)
    gauges = np.random.default_rng(14).permutation(n)[:50]
    plan = make_plan(down)
    assert_same(run(plan, net.k, net.x, d, nsub, gauges, True), run(plan, net.k, net.x, d, nsub, gauges, True), 'repeat')


# ---- 10. the C ABI through the bindings ----

def test_work_memory_and_refusals():
    n, T, G = 50, 6, 4
    down, k, x = cpu.network('tree', n, seed=4)
    indptr, indices = cpu.csc_from_down(down)
    c1, c2, c3 = oracle.muskingum_coefficients(k, x, DT_RUNOFF)
    plan = Plan(indptr, indices)
    ni = plan.n_inner
    plan.set_coeffs(-c1[indices], c2, c3, None)
    for members, nsub in ((1, 1), (1, 3), (3, 2)):
        assert members * T * G <= n * min(T, 16)
        lean = plan.unit_adjoint_gauges_work_bytes(members, G, T, nsub, False)
        assert lean == plan.unit_adjoint_batch_work_bytes(members, T, nsub) - 8 * n * T * members
        assert plan.unit_adjoint_gauges_work_bytes(members, G, T, nsub, True) == lean + 8 * n * T * members
        S = T * nsub
        splits = min(S, -(-2048 // (members * -(-n // 256))))
        steps = -(-S // splits)
        splits = -(-S // steps)
        assert lean == 8 * (n * members * (2 * S + T + 2 * plan.depth + 3 * splits + 6) + max(n * min(T, 16), members * T * G))
    # blocks larger than the permutation's rows: the rows grow to hold them
    grown = 8 * (3 * T * n - n * min(T, 16))
    assert plan.unit_adjoint_gauges_work_bytes(3, n, T, 1, False) == plan.unit_adjoint_batch_work_bytes(3, T, 1) - 8 * n * T * 3 + grown
    buf = lambda count: DeviceBuffer(max(count, 1) * 8)     # noqa: E731
    qc, qf, lat, dis, gout, coef = buf(2 * ni), buf(2 * ni), buf(2 * T * n), buf(2 * T * G), buf(2 * T * G), buf(3 * n)
    gqc, gqf, glat = buf(2 * ni), buf(2 * ni), buf(2 * T * n)
    for b in (qc, qf, lat, dis, gout):
        b.upload(np.ones(b.nbytes // 8))
    gauges = torch.tensor([7, 0, n - 1, 3], dtype=torch.int32, device=DEV)
    need = plan.unit_adjoint_gauges_work_bytes(1, G, T, 1, False)
    need_rows = plan.unit_adjoint_gauges_work_bytes(1, G, T, 1, True)
    work = DeviceBuffer(need_rows)

    def code(*args):
        with pytest.raises(_lib.RRError) as e:
            plan.unit_adjoint_gauges_dev(*args)
        return e.value.code, e.value.message

    names = ('members', 'n_gauges', 'gauges', 'q_ch0', 'q_full0', 'state_pitch', 'lateral', 'lat_rows', 'lat_pitch', 'discharge_g', 'grad_out_g',
             'gauge_pitch', 'grad_qch_final', 'grad_qfull_final', 'grad_lateral', 'grad_qch0', 'grad_qfull0', 'grad_coef', 'work', 'work_bytes',
             'T', 'nsub')
    ok = (1, G, gauges, qc, qf, ni, lat, T, T * n, dis, gout, T * G, None, None, None, gqc, gqf, coef, work, need, T, 1)
    assert len(ok) == len(names)

    def but(**kw):
        assert set(kw) <= set(names)
        return tuple(kw.get(name, v) for name, v in zip(names, ok))

    plan.unit_adjoint_gauges_dev(*ok)                                                      # accepted
    plan.unit_adjoint_gauges_dev(*but(gauge_pitch=0))                                      # one member: any gauge pitch
    c, msg = code(*but(work_bytes=need - 1))
    assert c == _lib.RR_E_INVALID and str(need) in msg and 'rr_unit_adjoint_gauges_work_bytes' in msg      # one byte short
    c, msg = code(*but(grad_lateral=glat))                                                 # grad_lateral on memory sized without it
    assert c == _lib.RR_E_INVALID and str(need_rows) in msg
    plan.unit_adjoint_gauges_dev(*but(grad_lateral=glat, work_bytes=need_rows))            # and on memory sized with it
    plan.unit_adjoint_gauges_dev(*but(discharge_g=None, grad_out_g=None, grad_qfull_final=qf))       # a loss on a final state alone
    assert code(*but(n_gauges=0))[0] == _lib.RR_E_INVALID
    assert code(*but(n_gauges=n + 1))[0] == _lib.RR_E_INVALID
    assert code(*but(gauges=None))[0] == _lib.RR_E_INVALID
    assert code(*but(grad_out_g=None))[0] == _lib.RR_E_INVALID                             # discharge_g without grad_out_g
    assert code(*but(discharge_g=None))[0] == _lib.RR_E_INVALID                            # and the reverse
    two = DeviceBuffer(plan.unit_adjoint_gauges_work_bytes(2, G, T, 1, False))
    c, msg = code(*but(members=2, gauge_pitch=T * G - 1, work=two, work_bytes=two.nbytes))
    assert c == _lib.RR_E_INVALID and 'pitch' in msg                                       # short gauge pitch
    plan.unit_adjoint_gauges_dev(*but(members=2, work=two, work_bytes=two.nbytes))         # two members, accepted
    assert code(*but(members=2, state_pitch=ni - 1, work=two, work_bytes=two.nbytes))[0] == _lib.RR_E_INVALID      # the batch call's refusals
    assert code(*but(members=0))[0] == _lib.RR_E_INVALID
    assert code(*but(members=65536))[0] == _lib.RR_E_INVALID
    assert code(*but(q_ch0=None))[0] == _lib.RR_E_INVALID                                  # the states for the coefficients
    assert code(*but(lat_rows=T - 1))[0] == _lib.RR_E_INVALID
    assert code(*but(T=0))[0] == _lib.RR_E_INVALID
    assert code(*but(nsub=0))[0] == _lib.RR_E_INVALID
    for bad in (0, n + 1):
        with pytest.raises(_lib.RRError) as e:
            plan.unit_adjoint_gauges_work_bytes(1, bad, T, 1, False)
        assert e.value.code == _lib.RR_E_INVALID
    _lib.lib().rr_dev_synchronize(0)
    # general edge data (set_unit_weights)
    plan.set_unit_weights(c1, np.full(indices.shape[0], 0.9))
    assert code(*ok)[0] == _lib.RR_E_UNSUPPORTED
    plan.set_unit_weights(None, None)
    # per-edge weights: one tributary weighted differently
    w = -c1[indices]
    e = int(np.flatnonzero(np.bincount(indices, minlength=n)[indices] >= 2)[0])      # an edge into a confluence
    w[e] *= 1.5
    plan.set_coeffs(w, c2, c3, None)
    assert code(*ok)[0] == _lib.RR_E_UNSUPPORTED
    plan.set_coeffs(-c1[indices], c2, c3, None)
    plan.unit_adjoint_gauges_dev(*ok)                                                      # accepted again
    _lib.lib().rr_dev_synchronize(0)
    # a plan with boundary reaches
    plan.set_boundary([], [int(np.flatnonzero(down < 0)[0])])
    assert code(*ok)[0] == _lib.RR_E_UNSUPPORTED


# ---- 11. with the scores ----

def test_chains_with_scores():
    n, T, nsub = 500, 30, 2
    down, k, x = cpu.network('forest', n, seed=8)
    d = unit.unit_inputs(down, T, 70, low=0.2)
    gauges = scrambled_gauges(down)
    rng = np.random.default_rng(71)
    obs = torch.tensor(rng.uniform(20.0, 150.0, (T, 7)), device=DEV)      # no constant column
    plan = make_plan(down)
    grads = []
    for use_gauges in (True, False):
        kt, xt = torch.tensor(k, requires_grad=True), torch.tensor(x, requires_grad=True)
        args = (plan, dev(d['q_ch0']), dev(d['q_full0']), dev(d['lat']), kt, xt, DT_RUNOFF / nsub, DT_RUNOFF)
        if use_gauges:
            out, _, _ = rr.grad.unit_route(*args, gauges=gauges)
            kge = rr.grad.scores(obs, out)['kge2012']
        else:
            out, _, _ = rr.grad.unit_route(*args)
            kge = rr.grad.scores(obs, out, columns=gauges)['kge2012']
        assert bool(torch.isfinite(kge).all())
        kge.sum().backward()
        grads.append((numpy_of(kge), kt.grad.numpy(), xt.grad.numpy()))
    (kge_g, gk, gx), (kge_d, wk, wx) = grads
    assert np.array_equal(kge_g, kge_d)
    assert np.isfinite(gk).all() and np.isfinite(gx).all() and np.isfinite(wk).all() and np.isfinite(wx).all()
    assert np.abs(wk).max() > 0
    assert_grad(gk, wk, 'scores: k.grad')
    assert_grad(gx, wx, 'scores: x.grad')


# ---- 12. peak memory ----

def test_backward_allocates_no_full_width_cotangent():
    n, T, G, nsub = 20_000, 64, 8, 1
    net = synth.synth_network(n, seed=15)
    down = net.down_index.astype(np.int64)
    d = unit.unit_inputs(down, T, 16)
    gauges = np.random.default_rng(17).permutation(n)[:G]
    plan = make_plan(down)
    qc, qf, lat, Wt = dev(d['q_ch0']), dev(d['q_full0']), dev(d['lat']), dev(d['G'][:, :G].copy())
    gauges_t = torch.as_tensor(gauges, device=DEV)
    rise = {}
    for use_gauges in (True, False):
        kt, xt = torch.tensor(net.k, requires_grad=True), torch.tensor(net.x, requires_grad=True)
        if use_gauges:
            out, _, _ = rr.grad.unit_route(plan, qc, qf, lat, kt, xt, DT_RUNOFF / nsub, DT_RUNOFF, gauges=gauges)
        else:
            out, _, _ = rr.grad.unit_route(plan, qc, qf, lat, kt, xt, DT_RUNOFF / nsub, DT_RUNOFF)
            out = out[:, gauges_t]
        loss = (out * Wt).sum()
        torch.cuda.synchronize(DEV)
        torch.cuda.reset_peak_memory_stats(DEV)
        before = torch.cuda.memory_allocated(DEV)
        loss.backward()
        torch.cuda.synchronize(DEV)
        rise[use_gauges] = torch.cuda.max_memory_allocated(DEV) - before
        del out, loss, kt, xt
    bound = 8 * n * T + plan.unit_adjoint_gauges_work_bytes(1, G, T, nsub, False)
    print(f'peak rise of backward: gauges {rise[True]} bytes, dense {rise[False]} bytes, bound {bound} bytes')
    assert rise[True] < bound
    assert not rise[False] < bound      # the dense path holds a (T, n) cotangent beside its larger work memory: the bound tells them apart
