"""Who owns device memory (csrc/rr_devbuf.hpp: every device array of a plan and of the host-pointer entry points is a DevBuf), seen from
outside through rr_dev_alloc_stats -- allocations alive / made in this process -- and the test switch RR_ALLOC_FAIL_AT=k, which rr_plan_create
reads: the k-th device allocation from then on is refused once.  A plan taken through every call that allocates and then closed leaves
nothing alive; a plan whose k-th allocation is refused, for EVERY k, is an RR_E_ALLOC and leaves nothing alive; a refused allocation inside
rr_plan_set_boundary leaves a plan that the same call repairs (the ghost table among its arrays); inside rr_plan_reserve* one that closes clean.

Two networks cover the allocation paths: the 70-reach forest of test_gpu_inpass_walk in tiles of 8 (several tiles, tile ghosts, no direct
plan) and a 300-reach post-order network of test_direct._case (direct plan with a skeleton and holes).  Each test is one child process, so
the counters start at 0.  No route call is made on a plan after an injected failure: return codes and ownership only."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
T = 200      # rows of the calls reserved for (two record batches, the second partial)


# ------------------------------------------------------------------------------------------------ the child process

def network(name):
    """(indptr, indices, coeffs, ghosts, exports): the plan's arguments and two (ghost, export) pairs -- headwaters and outlet-most reaches."""
    from oracle import oracle
    from river_route_amd import synth
    if name == 'forest':
        from test_gpu_inpass_walk import csc_from_down, forest
        os.environ['RR_TILE_BLOCK'] = '8'
        down = forest()
        k, x = 900.0 + 6300.0 * synth.u01(11, np.arange(down.size)), 0.05 + 0.4 * synth.u01(12, np.arange(down.size))
    else:
        from test_direct import csc_from_down
        os.environ.pop('RR_TILE_BLOCK', None)
        net = synth.synth_network(300, seed=17, order='postorder')      # test_direct._case(300, 17)
        down, k, x = net.down_index, net.k, net.x
    indptr, indices = csc_from_down(down)
    c1, c2, c3 = oracle.muskingum_coefficients(k, x, 900.0)
    hw = np.flatnonzero(np.bincount(down[down >= 0], minlength=down.size) == 0)
    out = np.flatnonzero(down < 0)
    last = int(out[-1])
    inner = int(np.flatnonzero(down == last)[0])      # flows into the last outlet: an export with a downstream reach in the plan
    return indptr, indices, (-c1[indices], c2, c3, (c1 + c2) / 900.0), ([int(hw[0])], [int(hw[1])]), ([last], [inner]), c1


def make_plan(name, coeffs=True):
    from river_route_amd.engine import Plan
    indptr, indices, cf, ghosts, exports, c1 = network(name)
    plan = Plan(indptr, indices)
    if name == 'direct':
        assert plan.direct_info()['ok'] and plan.direct_info()['holes'] > 0 and plan.direct_info()['skeleton_positions'] > 0, plan.direct_info()
    else:
        assert not plan.direct_info()['ok'] and plan.tile_info()['tiles'] > 3 and plan.tile_info()['ghosts'] > 0, plan.tile_info()
    if coeffs:
        plan.set_coeffs(*cf)
    return plan


def stats():
    from river_route_amd.engine import dev_alloc_stats
    return dev_alloc_stats()


def arm(k):
    """The k-th device allocation from here on is refused (0: none): the switch is read by rr_plan_create -- of a host-only plan, which
    allocates nothing on the device."""
    from river_route_amd._lib import RR_DEVICE_NONE
    from river_route_amd.engine import Plan
    os.environ['RR_ALLOC_FAIL_AT'] = str(k)
    Plan(np.zeros(2, np.int32), np.zeros(0, np.int32), device=RR_DEVICE_NONE).close()
    del os.environ['RR_ALLOC_FAIL_AT']


def refused(call):
    """True if `call` raised RR_E_ALLOC with the injected refusal's message, False if it succeeded."""
    from river_route_amd._lib import RR_E_ALLOC, RRError
    try:
        call()
    except RRError as e:
        assert e.code == RR_E_ALLOC, (e.code, e.message)
        return True
    return False


def route_vs_oracle(name, kernel, plan=None):
    """One short rapid_route_dev call on `plan` (None: a fresh one, closed afterwards) against the oracle, as
    test_direct.test_direct_rows_vs_oracle compares it."""
    from conftest import assert_close
    from oracle import oracle
    from river_route_amd import synth
    from river_route_amd.engine import DeviceBuffer
    indptr, indices, cf, _, _, _ = network(name)
    n, rows = indptr.size - 1, 40
    q0, ql = 2.0 * synth.u01(3, np.arange(n)), synth.synth_qlateral(n, 0, rows)
    q_ref, d_ref = q0.copy(), np.zeros((rows, n))
    oracle.rapid_route(indptr, indices, *cf, q_ref, ql, d_ref, 1)
    own = plan is None
    plan = make_plan(name) if own else plan
    d_q, d_ql, d_out = DeviceBuffer(n * 8).upload(q0), DeviceBuffer(ql.nbytes).upload(ql), DeviceBuffer(ql.nbytes)
    plan.rapid_route_dev(d_q, d_ql, rows, d_out, rows, rows, 1)
    assert plan.last_kernel() == kernel, plan.last_kernel()
    assert_close(d_out.download(np.float64, (rows, n)), d_ref, 'discharge')
    assert_close(d_q.download(np.float64, (n,)), q_ref, 'q_t')
    for b in (d_q, d_ql, d_out):
        b.free()
    if own:
        plan.close()


def lifecycle(name):
    from conftest import assert_close
    from oracle import oracle
    from river_route_amd import engine, synth
    indptr, indices, cf, ghosts, exports, c1 = network(name)
    base = stats()['made']
    plan = make_plan(name, coeffs=False)
    created = stats()['made'] - base
    assert created > 30 and stats()['live'] == created
    plan.set_coeffs(*cf)
    plan.set_coeffs(*cf)
    plan.set_unit_weights(c1, np.ones(indices.size))
    plan.set_unit_weights()
    plan.set_boundary(ghosts[0], exports[0])
    plan.set_boundary(ghosts[1], exports[1])
    plan.set_boundary([], [])
    for mode in (engine.MODE_RAPID, engine.MODE_MUSKINGUM, engine.MODE_UNIT):
        for host_rows in (False, True):
            plan.reserve(mode, T, 1, host_rows=host_rows)
    assert plan.reserve_ensemble(2, T)['tiled'] and plan.reserve_ensemble(5, T)['tiled']
    assert plan.rapid_adjoint_work_bytes(T) > 0 and plan.unit_adjoint_work_bytes(T) > 0
    assert stats()['live'] > created
    route_vs_oracle(name, 'direct' if name == 'direct' else 'tile', plan)      # on the arrays all of the above has laid out again
    plan.close()
    assert stats()['live'] == 0, stats()
    os.environ['RR_WAVE'] = '0'      # the streaming kernel: the call uploads the tiled permutations
    route_vs_oracle(name, 'tick')
    del os.environ['RR_WAVE']
    assert stats()['live'] == 0, stats()
    # the host-pointer entry points that stage their arrays themselves, each against what its own test compares it with
    n, n_ks = 24, 5
    kern, depth = synth.synth_uh_kernel(n, n_ks), synth.synth_runoff_depth(n, 0, 12)
    uh = oracle.UnitHydrograph(kern)
    uh.state = 0.1 * kern.copy()
    want, state = uh.convolve(depth), 0.1 * kern.copy()
    assert_close(engine.uh_convolve(kern, state, depth), want, 'convolved')      # test_gpu_kernels.test_unit_vs_oracle
    assert_close(state, uh.state, 'uh state')
    from test_gpu_runoff import case
    W, runoff, area = case(30, 12, 9, np.float64, False)                            # test_gpu_runoff.test_kernel_vs_oracle
    got, want = engine.runoff_to_qlateral(W.indptr, W.indices, W.data, runoff, area, 0), oracle.runoff_to_qlateral_core(W, runoff, area, False, False, False)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    assert_close(np.nan_to_num(got), np.nan_to_num(want), 'qlateral')
    from test_gpu_grid_weights import test_unaligned_rectangle_closed_form
    test_unaligned_rectangle_closed_form()                                            # rr_grid_overlap_area on a 10 x 12 grid, closed form
    assert engine.copy_bandwidth(nbytes=1 << 20, reps=1) > 0.0
    assert stats()['live'] == 0, stats()
    return dict(created=created, made=stats()['made'] - base)


def inject_create(name):
    base = stats()['made']
    make_plan(name, coeffs=False).close()
    A = stats()['made'] - base
    assert A > 30 and stats()['live'] == 0
    from river_route_amd.engine import Plan
    indptr, indices = network(name)[:2]
    cases = 0
    for k in range(1, A + 1):
        os.environ['RR_ALLOC_FAIL_AT'] = str(k)
        assert refused(lambda: Plan(indptr, indices)), f'allocation {k} of {A}: the plan was created'
        from river_route_amd._lib import lib
        assert 'hipMalloc of ' in lib().rr_last_error().decode() and lib().rr_last_error().decode().endswith('(injected)'), lib().rr_last_error()
        assert stats()['live'] == 0, (k, stats())
        cases += 1
    os.environ['RR_ALLOC_FAIL_AT'] = str(A + 1)      # one more than the plan makes: nothing is refused
    plan = Plan(indptr, indices)
    del os.environ['RR_ALLOC_FAIL_AT']
    arm(0)
    assert stats()['live'] == A
    plan.close()
    assert stats()['live'] == 0
    return dict(A=A, cases=cases)


def inject_set_boundary(name):
    ghosts, exports = network(name)[3:5]
    good = make_plan(name)
    base = stats()['made']
    good.set_boundary(ghosts[0], exports[0])
    A = stats()['made'] - base
    assert A >= 1
    want = (good.direct_info(), good.tile_info())
    good.close()
    cases = 0
    for k in range(1, A + 1):
        plan = make_plan(name)
        arm(k)
        assert refused(lambda: plan.set_boundary(ghosts[0], exports[0])), f'allocation {k} of {A}: the call succeeded'
        arm(0)
        plan.set_boundary(ghosts[0], exports[0])
        assert (plan.direct_info(), plan.tile_info()) == want, (k, plan.direct_info(), plan.tile_info())
        plan.close()
        assert stats()['live'] == 0, (k, stats())
        cases += 1
    return dict(A=A, cases=cases)


def inject_reserve(name):
    from river_route_amd import engine
    calls = {'reserve': lambda p: p.reserve(engine.MODE_RAPID, T, 1), 'reserve_host': lambda p: p.reserve(engine.MODE_RAPID, T, 1, host_rows=True),
             'reserve_stream': lambda p: p.reserve(engine.MODE_RAPID, 8, 1), 'reserve_ensemble': lambda p: p.reserve_ensemble(3, T)}
    out = {}
    for what, call in calls.items():
        plan = make_plan(name)
        base = stats()['made']
        call(plan)
        A = stats()['made'] - base
        plan.close()
        assert A >= 1 and stats()['live'] == 0, (what, A, stats())
        n_refused = 0
        for k in range(1, A + 1):
            plan = make_plan(name)
            arm(k)
            n_refused += refused(lambda: call(plan))      # success is legitimate: reserve_core falls back to shorter tasks when the ring is refused
            arm(0)
            plan.close()
            assert stats()['live'] == 0, (what, k, stats())
        out[what] = dict(A=A, refused=n_refused)
    return out


if __name__ == '__main__':
    assert stats() == dict(live=0, made=0)      # a fresh process
    print('RESULT ' + json.dumps({name: globals()[sys.argv[1]](name) for name in ('forest', 'direct')}))
    sys.exit(0)


# ------------------------------------------------------------------------------------------------ the tests

def child(what):
    root = os.path.dirname(HERE)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([root, HERE, os.environ.get('PYTHONPATH', '')]))
    for k in ('RR_WAVE', 'RR_WAVE_K', 'RR_TILE_BLOCK', 'RR_TILE_LEAN', 'RR_UH_PAIRS', 'RR_REC_BATCHES', 'RR_DIRECT', 'RR_HW_INPASS', 'RR_ALLOC_FAIL_AT'):
        env.pop(k, None)
    flags = ['-s'] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable, *flags, os.path.abspath(__file__), what], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f'{what}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}'
    res = json.loads(r.stdout.split('RESULT ')[-1])
    print(what, res)
    return res


def test_everything_a_plan_and_the_host_entry_points_allocate_is_released():
    res = child('lifecycle')
    assert set(res) == {'forest', 'direct'}


def test_plan_create_with_each_allocation_refused_in_turn():
    for name, r in child('inject_create').items():
        assert r['cases'] == r['A'] > 30, (name, r)


def test_set_boundary_with_each_allocation_refused_in_turn_is_repaired_by_the_same_call():
    res = child('inject_set_boundary')
    for name, r in res.items():
        assert r['cases'] == r['A'] >= 1, (name, r)
    assert res['direct']['A'] > res['forest']['A']      # the direct plan is laid out again, with the ghost table


def test_reserve_and_reserve_ensemble_with_each_allocation_refused_in_turn():
    for name, r in child('inject_reserve').items():
        for what, c in r.items():
            assert c['A'] >= 1 and 0 <= c['refused'] <= c['A'], (name, what, c)
        assert r['reserve_ensemble']['refused'] >= 3, (name, r)      # nothing shorter to fall back to for the members' state (three arrays)
