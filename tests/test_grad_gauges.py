"""gauges= of rr.grad.rapid_route and rr.grad.rapid_route_batch on the host: every bad value raises ValueError naming the argument,
on a host-only plan, so the check is made before any device call; and the new ABI entry points refuse a host-only plan as the
dense ones do."""
import numpy as np
import pytest
import torch

import river_route_amd as rr
from river_route_amd import _lib
from test_grad import host_only_plan

N, T = 5, 4
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


def args():
    return (torch.ones(N, **F64), torch.ones((T, N), **F64), torch.full((N,), 3600.0, **F64), torch.full((N,), 0.2, **F64))


@pytest.mark.parametrize('what,gauges,match', BAD, ids=[b[0] for b in BAD])
def test_bad_gauges_raise_before_a_device(what, gauges, match):
    plan = host_only_plan(N)
    q0, ql, k, x = args()
    with pytest.raises(ValueError, match='gauges') as e:
        rr.grad.rapid_route(plan, q0, ql, k, x, 900.0, 3600.0, gauges=gauges)
    assert match in str(e.value)
    with pytest.raises(ValueError, match='gauges') as e:
        rr.grad.rapid_route_batch(plan, q0, ql[None], k, x, 900.0, 3600.0, gauges=gauges)
    assert match in str(e.value)


def test_good_gauges_reach_the_device_check():
    # every accepted form gets as far as the last check, the plan's device: the gauges are not what is refused
    plan = host_only_plan(N)
    q0, ql, k, x = args()
    for gauges in (np.array([4, 0, 2]), [4, 0, 2], torch.tensor([4, 0, 2]), np.array([3], dtype=np.int32), np.arange(N)[::-1]):
        with pytest.raises(ValueError, match='host-only'):
            rr.grad.rapid_route(plan, q0, ql, k, x, 900.0, 3600.0, gauges=gauges)
        with pytest.raises(ValueError, match='host-only'):
            rr.grad.rapid_route_batch(plan, q0, ql[None], k, x, 900.0, 3600.0, gauges=gauges)


def test_other_arguments_are_still_checked_with_gauges():
    plan = host_only_plan(N)
    q0, ql, k, x = args()
    with pytest.raises(TypeError, match='float64'):
        rr.grad.rapid_route(plan, q0.float(), ql, k, x, 900.0, 3600.0, gauges=[0])
    with pytest.raises(ValueError, match='rows_per_window'):
        rr.grad.rapid_route(plan, q0, ql, k, x, 900.0, 3600.0, rows_per_window=0, gauges=[0])
    with pytest.raises(ValueError, match='members_per_sweep'):
        rr.grad.rapid_route_batch(plan, q0, ql[None], k, x, 900.0, 3600.0, members_per_sweep=0, gauges=[0])


def test_host_only_plan_has_no_gauge_adjoint():
    plan = host_only_plan()
    with pytest.raises(_lib.RRError) as e:
        plan.rapid_adjoint_gauges_work_bytes(1, 2, 4, 1)
    assert e.value.code == _lib.RR_E_UNSUPPORTED
    with pytest.raises(_lib.RRError) as e:
        plan.rapid_adjoint_gauges_dev(1, 2, None, None, 0, None, 0, 0, None, None, 0, None, None, None, None, None, 0, 4, 1)
    assert e.value.code == _lib.RR_E_UNSUPPORTED
