"""rr.grad.rapid_route_batch on the host: every argument is checked before a device is needed (a host-only plan is refused last), and
rr.grad.rapid_route keeps refusing a 3-D qlateral with the message it had."""
import pytest
import torch

import river_route_amd as rr
import test_grad as cpu
from river_route_amd import _lib


def test_batch_arguments_checked_before_a_device():
    n, B, T = 5, 3, 4
    plan = cpu.host_only_plan(n)
    f64 = dict(dtype=torch.float64)
    q0, ql = torch.ones((B, n), **f64), torch.ones((B, T, n), **f64)
    k, x = torch.full((n,), 3600.0, **f64), torch.full((n,), 0.2, **f64)
    g = rr.grad.rapid_route_batch
    with pytest.raises(TypeError, match='Plan'):
        g(object(), q0, ql, k, x, 900.0, 3600.0)
    # wrong number of dimensions
    with pytest.raises(ValueError, match='3-D'):
        g(plan, q0, ql[0], k, x, 900.0, 3600.0)
    with pytest.raises(ValueError, match='3-D'):
        g(plan, q0, ql[None], k, x, 900.0, 3600.0)
    with pytest.raises(ValueError, match='q0 must be'):
        g(plan, q0[None], ql, k, x, 900.0, 3600.0)
    # dtype
    with pytest.raises(TypeError, match='float64'):
        g(plan, q0, ql.float(), k, x, 900.0, 3600.0)
    with pytest.raises(TypeError, match='float64'):
        g(plan, q0.float(), ql, k, x, 900.0, 3600.0)
    with pytest.raises(TypeError, match='float64'):
        g(plan, q0, ql, k.float(), x, 900.0, 3600.0)
    # non-contiguous
    with pytest.raises(ValueError, match='contiguous'):
        g(plan, q0, torch.ones((T, B, n), **f64).transpose(0, 1), k, x, 900.0, 3600.0)
    with pytest.raises(ValueError, match='contiguous'):
        g(plan, torch.ones((n, B), **f64).t(), ql, k, x, 900.0, 3600.0)
    # B of q0 against B of qlateral; the reach count
    with pytest.raises(ValueError, match='shape'):
        g(plan, torch.ones((B + 1, n), **f64), ql, k, x, 900.0, 3600.0)
    with pytest.raises(ValueError, match='shape'):
        g(plan, q0, torch.ones((B, T, n + 1), **f64), k, x, 900.0, 3600.0)
    with pytest.raises(ValueError, match='shape'):
        g(plan, torch.ones(n + 1, **f64), ql, k, x, 900.0, 3600.0)
    # channel-only: q0 gives the member count, rows gives T
    with pytest.raises(ValueError, match='member count'):
        g(plan, torch.ones(n, **f64), None, k, x, 900.0, 3600.0, rows=T)
    with pytest.raises(ValueError, match='rows'):
        g(plan, q0, None, k, x, 900.0, 3600.0)
    with pytest.raises(ValueError, match='rows'):
        g(plan, q0, None, k, x, 900.0, 3600.0, rows=0)
    # members_per_sweep, rows_per_window
    with pytest.raises(ValueError, match='members_per_sweep'):
        g(plan, q0, ql, k, x, 900.0, 3600.0, members_per_sweep=0)
    with pytest.raises(ValueError, match='rows_per_window'):
        g(plan, q0, ql, k, x, 900.0, 3600.0, rows_per_window=0)
    # the time steps
    with pytest.raises(ValueError, match='whole number'):
        g(plan, q0, ql, k, x, 900.0, 1000.0)
    with pytest.raises(ValueError, match='positive'):
        g(plan, q0, ql, k, x, 0.0, 3600.0)
    # the host-only plan itself: last, for every form of the call
    with pytest.raises(ValueError, match='host-only'):
        g(plan, q0, ql, k, x, 900.0, 3600.0)
    with pytest.raises(ValueError, match='host-only'):
        g(plan, torch.ones(n, **f64), ql, k, x, 900.0, 3600.0, rows_per_window=2, members_per_sweep=2)
    with pytest.raises(ValueError, match='host-only'):
        g(plan, q0, None, k, x, 900.0, 3600.0, rows=T)


def test_rapid_route_still_refuses_three_dimensions():
    n = 5
    plan = cpu.host_only_plan(n)
    f64 = dict(dtype=torch.float64)
    with pytest.raises(ValueError) as e:
        rr.grad.rapid_route(plan, torch.ones(n, **f64), torch.ones((2, 4, n), **f64), torch.full((n,), 3600.0, **f64),
                            torch.full((n,), 0.2, **f64), 900.0, 3600.0)
    assert str(e.value) == 'qlateral must be a 2-D (T, n) tensor (ensembles have no adjoint: route members one by one)'


def test_host_only_plan_has_no_batched_adjoint():
    plan = cpu.host_only_plan()
    with pytest.raises(_lib.RRError) as e:
        plan.rapid_adjoint_batch_work_bytes(2, 4, 1)
    assert e.value.code == _lib.RR_E_UNSUPPORTED
    with pytest.raises(_lib.RRError) as e:
        plan.rapid_adjoint_batch_dev(2, None, 0, None, 0, 0, None, None, 0, None, None, None, None, None, 0, 4, 1)
    assert e.value.code == _lib.RR_E_UNSUPPORTED
    assert 'rr_rapid_adjoint_batch_dev' in e.value.message
