"""Scores of an ensemble's members without a GPU: the C ABI names, and every Python argument check of rr.metrics.MemberAccumulator,
rr.metrics.scores_members and Plan.rapid_route_members_scores -- each raises ValueError before any device work; arguments that pass
meet the refusal their neighbours meet without a device."""
import os
import re

import numpy as np
import pytest

import river_route_amd as rr
from river_route_amd import _lib
from river_route_amd._lib import RR_DEVICE_NONE, RR_E_INVALID, RR_E_NO_DEVICE, RR_E_STATE, RRError
from river_route_amd.engine import Plan

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'rr_hip.h')

# a five-reach tree: 0 -> 2 <- 1, 2 -> 4 <- 3
INDPTR = np.array([0, 1, 2, 3, 4, 4], np.int32)
INDICES = np.array([2, 2, 4, 4], np.int32)
N, E, M, T, G = 5, 4, 3, 8, 4
GAUGES = np.array([4, 2, 0, 2])


def test_header_declares_the_members_calls_the_binding_loads():
    text = open(HEADER).read()
    for name in ('rr_metrics_members_work_bytes', 'rr_metrics_update_members_dev'):
        assert re.search(rf'\bint {name}\(', text), name
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name)
    assert len(_lib._SIGNATURES['rr_metrics_members_work_bytes'][1]) == 4
    # rr_metrics_update_dev's arguments plus members, the two member pitches and skip_missing
    assert len(_lib._SIGNATURES['rr_metrics_update_members_dev'][1]) == len(_lib._SIGNATURES['rr_metrics_update_dev'][1]) + 4
    for name in ('scores_members', 'MemberAccumulator'):
        assert name in rr.metrics.__all__ and callable(getattr(rr.metrics, name))
    assert callable(Plan.rapid_route_members_scores)


def test_work_bytes_follow_the_split_rule_and_refuse_bad_sizes():
    import ctypes as C
    L, out = _lib.lib(), C.c_int64(-1)
    single = C.c_int64(-1)
    for n, rows in ((1, 1), (300, 100), (2000, 744), (100_000, 93)):
        assert L.rr_metrics_members_work_bytes(n, 1, rows, C.byref(out)) == 0 and L.rr_metrics_work_bytes(n, rows, C.byref(single)) == 0
        assert out.value == single.value, (n, rows)                      # one member: the single call's cut
    # 3 members x 2 column blocks x 4 chunks <= 2048: one split per 32-row chunk, as the single call has
    assert L.rr_metrics_members_work_bytes(300, 3, 100, C.byref(out)) == 0 and out.value == 4 * 9 * 3 * 300 * 8
    # 8 x 2 x 250 > 2048: 128 workgroup rows wanted, 250 chunks -> 2 chunks per split, 125 splits
    assert L.rr_metrics_members_work_bytes(300, 8, 8000, C.byref(out)) == 0 and out.value == 125 * 9 * 8 * 300 * 8
    assert L.rr_metrics_members_work_bytes(300, 8, 0, C.byref(out)) == 0 and out.value == 0
    for bad in ((300, 0, 10), (300, -1, 10), (-1, 2, 10), (300, 2, -1), (1 << 20, 1 << 11, 10)):
        assert L.rr_metrics_members_work_bytes(*bad, C.byref(out)) == RR_E_INVALID, bad
    assert L.rr_metrics_members_work_bytes(300, 2, 10, None) == RR_E_INVALID
    assert L.rr_metrics_members_work_bytes((1 << 20) - 1, 1 << 11, 10, C.byref(out)) == 0


# ---- rr.metrics.MemberAccumulator / scores_members ----

@pytest.mark.parametrize('bad', ['pred_2d', 'pred_4d', 'true_1d', 'true_members', 'true_columns', 'rows', 'pred_columns', 'columns_length',
                                 'columns_negative', 'columns_float', 'columns_range', 'no_members'])
def test_scores_members_checks_its_arrays_before_the_library(bad):
    y_true, y_pred, columns = np.ones((T, G)), np.ones((M, T, G)), None
    if bad == 'pred_2d':
        y_pred = np.ones((T, G))
    elif bad == 'pred_4d':
        y_pred = np.ones((1, M, T, G))
    elif bad == 'true_1d':
        y_true = np.ones(T)
    elif bad == 'true_members':
        y_true = np.ones((M + 1, T, G))
    elif bad == 'true_columns':
        y_true = np.ones((T, G + 1))
    elif bad == 'rows':
        y_true = np.ones((T + 1, G))
    elif bad == 'pred_columns':
        y_pred = np.ones((M, T, G + 2))                      # wider, and no columns= to say which
    elif bad == 'columns_length':
        y_pred, columns = np.ones((M, T, N)), GAUGES[:-1]
    elif bad == 'columns_negative':
        y_pred, columns = np.ones((M, T, N)), np.array([4, 2, -1, 2])
    elif bad == 'columns_float':
        y_pred, columns = np.ones((M, T, N)), GAUGES.astype(np.float64)
    elif bad == 'columns_range':
        y_pred, columns = np.ones((M, T, N)), np.array([4, 2, N, 2])
    elif bad == 'no_members':
        y_pred = np.ones((0, T, G))
    with pytest.raises(ValueError):
        rr.metrics.scores_members(y_true, y_pred, columns=columns)


@pytest.mark.parametrize('kw', [dict(n=0, members=2), dict(n=3, members=0), dict(n=1 << 20, members=1 << 11),
                                dict(n=G, members=M, columns=GAUGES[:2]), dict(n=G, members=M, columns=-GAUGES),
                                dict(n=G, members=M, columns=[0.5] * G)])
def test_member_accumulator_checks_its_arguments_before_the_library(kw):
    with pytest.raises(ValueError):
        rr.metrics.MemberAccumulator(**kw)


def test_arguments_that_pass_meet_the_refusal_of_the_single_call():
    """Without a device both meet what rr.metrics.scores meets: the library has no device to allocate on."""
    if _lib.device_count() > 0:      # (run where a device is visible: nothing refuses, and the scores come back)
        res = rr.metrics.scores_members(np.ones((T, G)), np.ones((M, T, N), np.float32), columns=GAUGES, skip_missing=True)
        assert all(v.shape == (M, G) for v in res.values())
        return
    with pytest.raises(RRError) as single:
        rr.metrics.scores(np.ones((T, G)), np.ones((T, G)))
    for y_true in (np.ones((T, G), np.float32), np.ones((M, T, G))):
        with pytest.raises(RRError) as e:
            rr.metrics.scores_members(y_true, np.ones((M, T, N), np.float32), columns=GAUGES, skip_missing=True)
        assert e.value.code == single.value.code


# ---- Plan.rapid_route_members_scores ----

@pytest.fixture()
def plan():
    with Plan(INDPTR, INDICES, device=RR_DEVICE_NONE) as p:
        yield p


def sets(m=M):
    return [np.full((m, E), -0.3), np.full((m, N), 0.2), np.full((m, N), 0.5), np.full((m, N), 1e-4)]


def test_rapid_route_members_scores_before_the_setter(plan):
    with pytest.raises(RRError) as e:
        plan.rapid_route_members_scores(np.zeros(N), np.zeros((T, N)), np.zeros((T, G)), GAUGES, 1)
    assert e.value.code == RR_E_STATE and 'set_member_coeffs' in e.value.message


@pytest.mark.parametrize('bad', ['ql_rank', 'ql_reaches', 'ql_members', 'q_t', 'factor_zero', 'factor_f64', 'dtype', 'observed_rows',
                                 'observed_rows_factor', 'observed_gauges', 'observed_rank', 'gauges_rank', 'gauges_float', 'gauges_negative',
                                 'gauges_range', 'gauges_empty', 'skip_rows_all', 'skip_rows_more', 'skip_rows_negative'])
def test_rapid_route_members_scores_checks_its_arguments_before_any_device_work(plan, bad):
    with pytest.raises(RRError):
        plan.set_member_coeffs(*sets())      # host-only: the arrays are kept, nothing is on a device
    ql = {'ql_rank': np.zeros(N), 'ql_reaches': np.zeros((T, N - 1)), 'ql_members': np.zeros((M + 1, T, N))}.get(bad, np.zeros((T, N)))
    q_t = np.zeros((M - 1, N)) if bad == 'q_t' else np.zeros(N)
    kw = dict(observed=np.zeros((T, G)), gauges=GAUGES, factor=1, skip_rows=0, dtype=np.float32)
    if bad == 'factor_zero':
        kw.update(factor=0)
    elif bad == 'factor_f64':
        kw.update(factor=2, dtype=np.float64, observed=np.zeros((T // 2, G)))      # float64 rows are never averaged
    elif bad == 'dtype':
        kw.update(dtype=np.float16)
    elif bad == 'observed_rows':
        kw.update(observed=np.zeros((T - 1, G)))
    elif bad == 'observed_rows_factor':
        kw.update(factor=2)                                                        # T // 2 rows are scored, T observed
    elif bad == 'observed_gauges':
        kw.update(observed=np.zeros((T, G + 1)))
    elif bad == 'observed_rank':
        kw.update(observed=np.zeros((M, T, G)))
    elif bad == 'gauges_rank':
        kw.update(gauges=GAUGES.reshape(2, 2))
    elif bad == 'gauges_float':
        kw.update(gauges=GAUGES.astype(np.float64))
    elif bad == 'gauges_negative':
        kw.update(gauges=np.array([4, 2, -1, 2]))
    elif bad == 'gauges_range':
        kw.update(gauges=np.array([4, 2, N, 2]))
    elif bad == 'gauges_empty':
        kw.update(gauges=np.zeros(0, np.int64), observed=np.zeros((T, 0)))
    elif bad == 'skip_rows_all':
        kw.update(skip_rows=T)
    elif bad == 'skip_rows_more':
        kw.update(skip_rows=T + 3)
    elif bad == 'skip_rows_negative':
        kw.update(skip_rows=-1)
    with pytest.raises(ValueError):
        plan.rapid_route_members_scores(q_t, ql, num_substeps=1, **kw)


@pytest.mark.parametrize('shared', [True, False])
def test_rapid_route_members_scores_meets_the_host_only_refusal(plan, shared):
    with pytest.raises(RRError):
        plan.set_member_coeffs(*sets())
    ql = np.zeros((T, N), np.float32) if shared else np.zeros((M, T, N))
    with pytest.raises(RRError) as e:
        plan.rapid_route_members_scores(np.zeros((M, N)), ql, np.zeros((T // 2, G), np.float32), GAUGES, 1, factor=2, skip_missing=True,
                                        skip_rows=3)
    assert e.value.code == RR_E_NO_DEVICE
    with pytest.raises(RRError) as e:
        plan.rapid_route_members_scores(np.zeros(N), ql, np.zeros((T, G)), GAUGES, 1, dtype=np.float64)
    assert e.value.code == RR_E_NO_DEVICE


def test_the_existing_members_call_checks_as_before(plan):
    """The checks rapid_route_members now shares with the scores call are the ones it had."""
    with pytest.raises(RRError):
        plan.set_member_coeffs(*sets())
    with pytest.raises(ValueError, match='members'):
        plan.rapid_route_members(np.zeros(N), np.zeros((M + 1, T, N)), np.zeros((M, T, N)), 1)
    with pytest.raises(ValueError, match='discharge must be'):
        plan.rapid_route_members(np.zeros(N), np.zeros((T, N)), np.zeros((M, T, N)), 1, factor=2)
    with pytest.raises(RRError) as e:
        plan.rapid_route_members(np.zeros(N), np.zeros((T, N)), np.zeros((M, T, N)), 1)
    assert e.value.code == RR_E_NO_DEVICE
