"""Parameter ensembles without a GPU: the C ABI names and every Python argument check of Plan.set_member_coeffs and
Plan.rapid_route_members, on a host-only plan -- each raises before any device work; arguments that pass meet the host-only refusal."""
import os
import re

import numpy as np
import pytest

from river_route_amd import _lib
from river_route_amd._lib import RR_DEVICE_NONE, RR_E_NO_DEVICE, RR_E_STATE, RRError
from river_route_amd.engine import Plan

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'rr_hip.h')

# a five-reach tree: 0 -> 2 <- 1, 2 -> 4 <- 3
INDPTR = np.array([0, 1, 2, 3, 4, 4], np.int32)
INDICES = np.array([2, 2, 4, 4], np.int32)
N, E, M, T = 5, 4, 3, 8


def test_header_declares_the_member_calls_the_binding_loads():
    text = open(HEADER).read()
    for name in ('rr_plan_set_member_coeffs', 'rr_rapid_route_members_dev'):
        assert re.search(rf'\bint {name}\(', text), name
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name)
    assert len(_lib._SIGNATURES['rr_plan_set_member_coeffs'][1]) == 8
    assert _lib._SIGNATURES['rr_rapid_route_members_dev'] == _lib._SIGNATURES['rr_rapid_route_ensemble_dev']


@pytest.fixture()
def plan():
    with Plan(INDPTR, INDICES, device=RR_DEVICE_NONE) as p:
        yield p


def sets(m=M):
    return [np.full((m, E), -0.3), np.full((m, N), 0.2), np.full((m, N), 0.5), np.full((m, N), 1e-4)]


@pytest.mark.parametrize('bad', ['rank', 'members', 'edges', 'reaches', 'empty'])
def test_set_member_coeffs_checks_its_arrays_before_the_library(plan, bad):
    a = sets()
    if bad == 'rank':
        a[1] = a[1][0]
    elif bad == 'members':
        a[3] = a[3][:2]
    elif bad == 'edges':
        a[0] = np.full((M, E + 1), -0.3)
    elif bad == 'reaches':
        a[2] = np.full((M, N - 1), 0.5)
    else:
        a = [x[:0] for x in a]
    with pytest.raises(ValueError):
        plan.set_member_coeffs(*a)
    assert getattr(plan, '_member_sets', None) is None


def test_set_member_coeffs_makes_contiguous_float64_then_meets_the_host_only_refusal(plan):
    a = sets()
    a[1] = a[1].astype(np.float32)                   # another dtype
    a[2] = np.asfortranarray(a[2])                   # another memory order
    a[3] = [list(row) for row in a[3]]               # not an array at all
    a[0].setflags(write=False)
    with pytest.raises(RRError) as e:
        plan.set_member_coeffs(*a)
    assert e.value.code == RR_E_NO_DEVICE
    for kept, shape in zip(plan._member_sets, [(M, E), (M, N), (M, N), (M, N)]):
        assert kept.dtype == np.float64 and kept.flags['C_CONTIGUOUS'] and kept.shape == shape
    assert np.array_equal(plan._member_sets[1], np.full((M, N), np.float32(0.2), np.float64))


def test_rapid_route_members_before_the_setter(plan):
    with pytest.raises(RRError) as e:
        plan.rapid_route_members(np.zeros(N), np.zeros((T, N)), np.zeros((M, T, N)), 1)
    assert e.value.code == RR_E_STATE and 'set_member_coeffs' in e.value.message


@pytest.mark.parametrize('bad', ['ql_rank', 'ql_reaches', 'ql_members', 'q_t', 'out_members', 'out_dtype', 'out_readonly', 'out_order', 'out_list',
                                 'factor_f64', 'factor_rows', 'factor_zero'])
def test_rapid_route_members_checks_its_arrays_before_any_device_work(plan, bad):
    with pytest.raises(RRError):
        plan.set_member_coeffs(*sets())      # host-only: the arrays are kept, nothing is on a device
    ql = {'ql_rank': np.zeros(N), 'ql_reaches': np.zeros((T, N - 1)), 'ql_members': np.zeros((M + 1, T, N))}.get(bad, np.zeros((T, N)))
    q_t = np.zeros((M - 1, N)) if bad == 'q_t' else np.zeros(N)
    out, factor = np.zeros((M, T, N)), 1
    if bad == 'out_members':
        out = np.zeros((M + 1, T, N))
    elif bad == 'out_dtype':
        out = np.zeros((M, T, N), np.float16)
    elif bad == 'out_readonly':
        out.setflags(write=False)
    elif bad == 'out_order':
        out = np.asfortranarray(out)
    elif bad == 'out_list':
        out = out.tolist()
    elif bad == 'factor_f64':
        factor = 2                                             # float64 rows are never averaged
    elif bad == 'factor_rows':
        out, factor = np.zeros((M, T // 2 + 1, N), np.float32), 2
    elif bad == 'factor_zero':
        out, factor = np.zeros((M, T, N), np.float32), 0
    with pytest.raises(ValueError):
        plan.rapid_route_members(q_t, ql, out, 1, factor=factor)


@pytest.mark.parametrize('shared', [True, False])
def test_rapid_route_members_meets_the_host_only_refusal(plan, shared):
    with pytest.raises(RRError):
        plan.set_member_coeffs(*sets())
    ql = np.zeros((T, N), np.float32) if shared else np.zeros((M, T, N))
    with pytest.raises(RRError) as e:
        plan.rapid_route_members(np.zeros((M, N)), ql, np.zeros((M, T // 2, N), np.float32), 1, factor=2)
    assert e.value.code == RR_E_NO_DEVICE


def test_the_library_refuses_a_host_only_plan_itself(plan):
    a = sets()
    rc = _lib.lib().rr_plan_set_member_coeffs(plan._h, M, _lib.ptr(a[0]), E, _lib.ptr(a[1]), _lib.ptr(a[2]), _lib.ptr(a[3]), N)
    assert rc == RR_E_NO_DEVICE
    out, q = np.zeros((M, 32, N)), np.zeros((M, N))
    rc = _lib.lib().rr_rapid_route_members_dev(plan._h, M, _lib.ptr(q), N, _lib.ptr(np.zeros((32, N))), 0, 0, _lib.ptr(out), 0, 32 * N, 1, 32, 1, None)
    assert rc == RR_E_NO_DEVICE
