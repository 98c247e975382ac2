"""rr.grad.unit_route_batch, uh_convolve_batch and unit_muskingum_batch on the host: every argument is checked before a device is
needed (a host-only plan is refused last), a host-only plan has no batched Unit adjoint, and rr.grad.unit_route, uh_convolve and
unit_muskingum keep refusing 3-D rows with the message they had."""
import pytest
import torch

import river_route_amd as rr
import test_grad as cpu
from river_route_amd import _lib

F64 = dict(dtype=torch.float64)


def args(n=5, B=3, T=4, n_ks=3):
    plan = cpu.host_only_plan(n)
    ni = plan.n_inner
    return dict(plan=plan, ni=ni, qc=torch.ones((B, ni), **F64), qf=torch.ones((B, ni), **F64), rows=torch.ones((B, T, n), **F64),
                k=torch.full((n,), 3600.0, **F64), x=torch.full((n,), 0.2, **F64), kern=torch.ones((n_ks, n), **F64),
                st=torch.zeros((B, n_ks, n), **F64))


def test_unit_route_batch_arguments_checked_before_a_device():
    n, B, T = 5, 3, 4
    a = args(n, B, T)
    plan, ni, qc, qf, lat, k, x = (a[key] for key in ('plan', 'ni', 'qc', 'qf', 'rows', 'k', 'x'))
    g = rr.grad.unit_route_batch
    with pytest.raises(TypeError, match='Plan'):
        g(object(), qc, qf, lat, k, x, 900.0, 3600.0)
    # wrong number of dimensions
    with pytest.raises(ValueError, match='3-D'):
        g(plan, qc, qf, lat[0], k, x, 900.0, 3600.0)
    with pytest.raises(ValueError, match='3-D'):
        g(plan, qc, qf, lat[None], k, x, 900.0, 3600.0)
    with pytest.raises(ValueError, match='q_ch0 must be'):
        g(plan, qc[None], qf, lat, k, x, 900.0, 3600.0)
    with pytest.raises(ValueError, match='q_full0 must be'):
        g(plan, qc, torch.tensor(1.0, **F64), lat, k, x, 900.0, 3600.0)
    # dtype
    with pytest.raises(TypeError, match='float64'):
        g(plan, qc, qf, lat.float(), k, x, 900.0, 3600.0)
    with pytest.raises(TypeError, match='float64'):
        g(plan, qc.float(), qf, lat, k, x, 900.0, 3600.0)
    with pytest.raises(TypeError, match='float64'):
        g(plan, qc, qf, lat, k, x.float(), 900.0, 3600.0)
    # non-contiguous
    with pytest.raises(ValueError, match='contiguous'):
        g(plan, qc, qf, torch.ones((T, B, n), **F64).transpose(0, 1), k, x, 900.0, 3600.0)
    with pytest.raises(ValueError, match='contiguous'):
        g(plan, torch.ones((ni, B), **F64).t(), qf, lat, k, x, 900.0, 3600.0)
    # B of the states against B of the rows; the reach counts
    with pytest.raises(ValueError, match='shape'):
        g(plan, torch.ones((B + 1, ni), **F64), qf, lat, k, x, 900.0, 3600.0)
    with pytest.raises(ValueError, match='shape'):
        g(plan, qc, torch.ones((B - 1, ni), **F64), lat, k, x, 900.0, 3600.0)
    with pytest.raises(ValueError, match='shape'):
        g(plan, qc, qf, torch.ones((B, T, n + 1), **F64), k, x, 900.0, 3600.0)
    with pytest.raises(ValueError, match='shape'):
        g(plan, torch.ones(n, **F64), qf, lat, k, x, 900.0, 3600.0)          # a shared state has n_inner values, not n
    with pytest.raises(ValueError, match='no rows'):
        g(plan, qc, qf, torch.ones((B, 0, n), **F64), k, x, 900.0, 3600.0)
    with pytest.raises(ValueError, match='no members'):
        g(plan, qc[:0], qf[:0], torch.ones((0, T, n), **F64), k, x, 900.0, 3600.0)
    # members_per_sweep, rows_per_window, the time steps
    with pytest.raises(ValueError, match='members_per_sweep'):
        g(plan, qc, qf, lat, k, x, 900.0, 3600.0, members_per_sweep=0)
    with pytest.raises(ValueError, match='rows_per_window'):
        g(plan, qc, qf, lat, k, x, 900.0, 3600.0, rows_per_window=0)
    with pytest.raises(ValueError, match='whole number'):
        g(plan, qc, qf, lat, k, x, 900.0, 1000.0)
    with pytest.raises(ValueError, match='positive'):
        g(plan, qc, qf, lat, k, x, 0.0, 3600.0)
    # the host-only plan itself: last, for every form of the call
    with pytest.raises(ValueError, match='host-only'):
        g(plan, qc, qf, lat, k, x, 900.0, 3600.0)
    with pytest.raises(ValueError, match='host-only'):
        g(plan, qc[0], qf, lat, k, x, 900.0, 3600.0, rows_per_window=2, members_per_sweep=2)


def test_unit_muskingum_batch_arguments_checked_before_a_device():
    n, B, T, n_ks = 5, 3, 4, 3
    a = args(n, B, T, n_ks)
    plan, qc, qf, depth, k, x, kern, st = (a[key] for key in ('plan', 'qc', 'qf', 'rows', 'k', 'x', 'kern', 'st'))
    m = rr.grad.unit_muskingum_batch
    with pytest.raises(ValueError, match='3-D'):
        m(plan, qc, qf, depth[0], kern, st, k, x, 900.0, 3600.0)
    with pytest.raises(ValueError, match='uh_kernel'):
        m(plan, qc, qf, depth, kern[0], st, k, x, 900.0, 3600.0)
    with pytest.raises(ValueError, match='uh_state must be'):
        m(plan, qc, qf, depth, kern, st[None], k, x, 900.0, 3600.0)
    with pytest.raises(ValueError, match='shape'):
        m(plan, qc, qf, depth, kern, st[:, :2], k, x, 900.0, 3600.0)
    with pytest.raises(ValueError, match='shape'):
        m(plan, qc, qf, depth, kern, st[:2], k, x, 900.0, 3600.0)             # B of uh_state against B of the rows
    with pytest.raises(ValueError, match='shape'):
        m(plan, qc[:2], qf, depth, kern, st, k, x, 900.0, 3600.0)
    with pytest.raises(TypeError, match='float64'):
        m(plan, qc, qf, depth, kern.float(), st, k, x, 900.0, 3600.0)
    with pytest.raises(TypeError, match='float64'):
        m(plan, qc, qf, depth, kern, st.float(), k, x, 900.0, 3600.0)
    with pytest.raises(ValueError, match='contiguous'):
        m(plan, qc, qf, depth, kern, torch.zeros((n_ks, B, n), **F64).transpose(0, 1), k, x, 900.0, 3600.0)
    with pytest.raises(ValueError, match='members_per_sweep'):
        m(plan, qc, qf, depth, kern, st, k, x, 900.0, 3600.0, members_per_sweep=-1)
    with pytest.raises(ValueError, match='host-only'):
        m(plan, qc, qf, depth, kern, st, k, x, 900.0, 3600.0)
    with pytest.raises(ValueError, match='host-only'):
        m(plan, qc[0], qf[0], depth, kern, st[0], k, x, 900.0, 3600.0, rows_per_window=2)


def test_uh_convolve_batch_arguments_checked_before_a_device():
    n, B, T, n_ks = 5, 3, 4, 3
    a = args(n, B, T, n_ks)
    depth, kern, st = a['rows'], a['kern'], a['st']
    u = rr.grad.uh_convolve_batch
    with pytest.raises(ValueError, match='2-D'):
        u(kern[0], st, depth)
    with pytest.raises(ValueError, match='3-D'):
        u(kern, st, depth[0])
    with pytest.raises(ValueError, match='state must be'):
        u(kern, st[0, 0], depth)
    with pytest.raises(ValueError, match='shape'):
        u(kern, st[:2], depth)
    with pytest.raises(ValueError, match='shape'):
        u(kern, st[0, :2], depth)
    with pytest.raises(TypeError, match='float64'):
        u(kern, st, depth.float())
    with pytest.raises(ValueError, match='contiguous'):
        u(kern, st, torch.ones((T, B, n), **F64).transpose(0, 1))
    with pytest.raises(ValueError, match='GPU'):
        u(kern, st, depth)          # host tensors
    with pytest.raises(ValueError, match='GPU'):
        u(kern, st[0], depth)


def test_single_series_functions_still_refuse_three_dimensions():
    n = 5
    a = args(n)
    plan, qc, qf, rows, k, x, kern, st = (a[key] for key in ('plan', 'qc', 'qf', 'rows', 'k', 'x', 'kern', 'st'))
    text = ' must be a 2-D (T, n) tensor (ensembles have no adjoint: route members one by one)'
    with pytest.raises(ValueError) as e:
        rr.grad.unit_route(plan, qc[0], qf[0], rows, k, x, 900.0, 3600.0)
    assert str(e.value) == 'lateral' + text
    with pytest.raises(ValueError) as e:
        rr.grad.unit_muskingum(plan, qc[0], qf[0], rows, kern, st[0], k, x, 900.0, 3600.0)
    assert str(e.value) == 'depth' + text
    with pytest.raises(ValueError) as e:
        rr.grad.uh_convolve(kern, st[0], rows)
    assert str(e.value) == 'depth' + text


def test_host_only_plan_has_no_batched_unit_adjoint():
    plan = cpu.host_only_plan()
    with pytest.raises(_lib.RRError) as e:
        plan.unit_adjoint_batch_work_bytes(2, 4, 1)
    assert e.value.code == _lib.RR_E_UNSUPPORTED
    with pytest.raises(_lib.RRError) as e:
        plan.unit_adjoint_batch_dev(2, None, None, 0, None, 0, 0, None, None, 0, None, None, None, None, None, None, None, 0, 4, 1)
    assert e.value.code == _lib.RR_E_UNSUPPORTED
    assert 'rr_unit_adjoint_batch_dev' in e.value.message
