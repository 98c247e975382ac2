"""gauges= of rr.grad.unit_route, unit_route_batch, unit_muskingum and unit_muskingum_batch on the host: every bad value raises
ValueError naming the argument, on a host-only plan, so the check is made before any device call; and the new ABI entry points refuse a
host-only plan as the dense ones do."""
import numpy as np
import pytest
import torch

import river_route_amd as rr
from river_route_amd import _lib
from test_grad import host_only_plan

N, T, N_KS = 5, 4, 3
F64 = dict(dtype=torch.float64)

BAD = [
    ('float dtype', np.array([0.0, 2.0]), 'integer'),
    ('float tensor', torch.tensor([0.0, 2.0]), 'integer'),
    ('bool tensor', torch.tensor([True, False]), 'integer'),
    ('rank 0', np.int64(2), '1-D'),
    ('rank 2', np.array([[0, 1], [2, 3]]), '1-D'),
    ('rank 2 tensor', torch.tensor([[0, 1], [2, 3]]), '1-D'),
    ('empty', np.zeros(0, dtype=np.int64), 'empty'),
    ('empty tensor', torch.zeros(0, dtype=torch.int64), 'empty'),
    ('duplicate', np.array([1, 3, 1]), 'more than once'),
    ('negative', np.array([0, -1]), 'reach -1'),
    ('index n', np.array([0, N]), f'reach {N}'),
    ('index n, int32 tensor', torch.tensor([N, 0], dtype=torch.int32), f'reach {N}'),
]


def calls(plan):
    """The four functions with good arguments but `gauges`, as callables of it (batched: one member)."""
    ni = plan.n_inner
    qc, qf, rows = torch.ones(ni, **F64), torch.ones(ni, **F64), torch.ones((T, N), **F64)
    k, x = torch.full((N,), 3600.0, **F64), torch.full((N,), 0.2, **F64)
    kern, st = torch.full((N_KS, N), 1.0 / N_KS, **F64), torch.zeros((N_KS, N), **F64)
    return {
        'unit_route': lambda **kw: rr.grad.unit_route(plan, qc, qf, rows, k, x, 900.0, 3600.0, **kw),
        'unit_route_batch': lambda **kw: rr.grad.unit_route_batch(plan, qc[None], qf[None], rows[None], k, x, 900.0, 3600.0, **kw),
        'unit_muskingum': lambda **kw: rr.grad.unit_muskingum(plan, qc, qf, rows, kern, st, k, x, 900.0, 3600.0, **kw),
        'unit_muskingum_batch': lambda **kw: rr.grad.unit_muskingum_batch(plan, qc[None], qf[None], rows[None], kern, st[None], k, x, 900.0,
                                                                          3600.0, **kw),
    }


FUNCTIONS = ('unit_route', 'unit_route_batch', 'unit_muskingum', 'unit_muskingum_batch')


@pytest.mark.parametrize('function', FUNCTIONS)
@pytest.mark.parametrize('what,gauges,match', BAD, ids=[b[0] for b in BAD])
def test_bad_gauges_raise_before_a_device(function, what, gauges, match):
    call = calls(host_only_plan(N))[function]
    with pytest.raises(ValueError, match='gauges') as e:
        call(gauges=gauges)
    assert match in str(e.value)


@pytest.mark.parametrize('function', FUNCTIONS)
def test_good_gauges_reach_the_device_check(function):
    # every accepted form gets as far as the last check, the plan's device: the gauges are not what is refused
    call = calls(host_only_plan(N))[function]
    for gauges in (np.array([4, 0, 2]), [4, 0, 2], torch.tensor([4, 0, 2]), np.array([3], dtype=np.int32), np.arange(N)[::-1]):
        with pytest.raises(ValueError, match='host-only'):
            call(gauges=gauges)
    with pytest.raises(ValueError, match='host-only'):
        call()      # and so does the call without the keyword


def test_other_arguments_are_still_checked_with_gauges():
    plan = host_only_plan(N)
    ni = plan.n_inner
    qc, qf, rows = torch.ones(ni, **F64), torch.ones(ni, **F64), torch.ones((T, N), **F64)
    k, x = torch.full((N,), 3600.0, **F64), torch.full((N,), 0.2, **F64)
    with pytest.raises(TypeError, match='float64'):
        rr.grad.unit_route(plan, qc.float(), qf, rows, k, x, 900.0, 3600.0, gauges=[0])
    with pytest.raises(ValueError, match='rows_per_window'):
        rr.grad.unit_route(plan, qc, qf, rows, k, x, 900.0, 3600.0, rows_per_window=0, gauges=[0])
    with pytest.raises(ValueError, match='members_per_sweep'):
        rr.grad.unit_route_batch(plan, qc[None], qf[None], rows[None], k, x, 900.0, 3600.0, members_per_sweep=0, gauges=[0])
    with pytest.raises(TypeError, match='Plan'):
        rr.grad.unit_route_batch(object(), qc[None], qf[None], rows[None], k, x, 900.0, 3600.0, gauges=[0])


def test_host_only_plan_has_no_unit_gauge_adjoint():
    plan = host_only_plan()
    with pytest.raises(_lib.RRError) as e:
        plan.unit_adjoint_gauges_work_bytes(1, 2, 4, 1)
    assert e.value.code == _lib.RR_E_UNSUPPORTED
    with pytest.raises(_lib.RRError) as e:
        plan.unit_adjoint_gauges_dev(1, 2, None, None, None, 0, None, 0, 0, None, None, 0, None, None, None, None, None, None, None, 0, 4, 1)
    assert e.value.code == _lib.RR_E_UNSUPPORTED
    assert 'rr_unit_adjoint_gauges_work_bytes' in _lib.EXPORTS and 'rr_unit_adjoint_gauges_dev' in _lib.EXPORTS
