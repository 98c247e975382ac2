"""Ensemble calls without a GPU: the C ABI names, flag values and Python argument checks of Plan.rapid_route_ensemble."""
import os
import re

import numpy as np
import pytest

from river_route_amd import _lib, engine

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'rr_hip.h')


def _defines():
    return {m.group(1): int(m.group(2)) for m in re.finditer(r'#define (RR_\w+) (-?\d+)', open(HEADER).read())}


def test_header_declares_the_ensemble_calls_the_binding_loads():
    text = open(HEADER).read()
    for name in ('rr_plan_reserve_ensemble', 'rr_rapid_route_ensemble_dev'):
        assert re.search(rf'\bint {name}\(', text), name
        assert name in _lib.EXPORTS
    d = _defines()
    assert d['RR_ROWS_F32_IN'] == 16 and d['RR_ROWS_F32_OUT'] == 4      # the bits Plan.reserve_ensemble passes
    assert d['RR_KERNEL_TILE_ENSEMBLE'] == 3
    assert len({d[k] for k in ('RR_ROWS_NOT_PLAIN', 'RR_ROWS_F32_OUT', 'RR_ROWS_UH', 'RR_ROWS_F32_IN')}) == 4


@pytest.mark.parametrize('bad', ['qlateral', 'discharge', 'factor'])
def test_rapid_route_ensemble_checks_its_arrays_before_any_device_work(bad):
    plan = engine.Plan.__new__(engine.Plan)
    plan.n, plan.device = 5, 0
    ql = np.zeros((2, 8, 5)) if bad != 'qlateral' else np.zeros((2, 8, 4))
    out = np.zeros((2, 8, 5)) if bad != 'discharge' else np.zeros((2, 8, 5), np.float16)
    with pytest.raises(ValueError):
        plan.rapid_route_ensemble(np.zeros(5), ql, out, 1, factor=2 if bad == 'factor' else 1)


# ---- RapidMuskingum in ensemble mode: members with the same dates routed in groups ----
import pandas as pd  # noqa: E402

import river_route_amd as rr  # noqa: E402
from river_route_amd.routers import muskingum as musk_mod  # noqa: E402


class LoopPlan:
    """Stand-in for engine.Plan backed by oracle/: the routers' host path, plus an ensemble call that loops over its members."""
    cap, direct = 64, False
    groups: list = []

    def __init__(self, indptr, indices, device=0):
        self.indptr, self.indices = np.asarray(indptr, np.int32), np.asarray(indices, np.int32)
        self.n = len(self.indptr) - 1

    def close(self):
        pass

    def set_coeffs(self, lhs, c2, c3, c4_dt=None):
        self.lhs, self.c2, self.c3, self.c4 = lhs, c2, c3, c4_dt

    def rapid_route(self, q_t, ql, d, nsub):
        from oracle import oracle
        oracle.rapid_route(self.indptr, self.indices, self.lhs, self.c2, self.c3, self.c4, q_t, ql, d, nsub)

    def reserve(self, mode, T, num_substeps=1, **kw):
        return dict(direct=self.direct, tiled=not self.direct)

    def reserve_ensemble(self, members, T, num_substeps=1, f32_in=False, f32_out=False):
        return dict(members_max=self.cap)

    def rapid_route_ensemble(self, q_t, qlateral, discharge, num_substeps, factor=1):
        M, T, n = qlateral.shape
        assert M <= self.cap
        LoopPlan.groups.append(M)
        states = np.empty((M, n))
        for m in range(M):
            q, d = np.array(q_t, dtype=np.float64), np.zeros((T, n))
            self.rapid_route(q, np.ascontiguousarray(qlateral[m], dtype=np.float64), d, num_substeps)
            states[m] = q
            discharge[m] = d.reshape((-1, factor, n)).mean(axis=1).astype(discharge.dtype) if factor > 1 else d
        return states


class NoEnsemblePlan(LoopPlan):
    rapid_route_ensemble = None

    def __getattribute__(self, name):
        if name in ('rapid_route_ensemble', 'reserve_ensemble'):
            raise AttributeError(name)
        return super().__getattribute__(name)


def _route(monkeypatch, tmp_path, golden_routers, plan_cls, dates, series, **cfg):
    g = golden_routers
    params = tmp_path / 'params.parquet'
    pd.DataFrame({'river_id': g['river_ids'], 'downstream_river_id': g['downstream_ids'], 'k': g['k'], 'x': g['x']}).to_parquet(params)
    init = tmp_path / 'init.parquet'
    pd.DataFrame({'Q': g['q0']}).to_parquet(init)
    files = []
    for i in range(len(series)):
        f = tmp_path / f'ql{i}.nc'
        f.touch()
        files.append(str(f))
    monkeypatch.setattr(musk_mod, 'Plan', plan_cls)

    class InMemory(rr.RapidMuskingum):
        def _qlateral_generator(self):
            yield from zip(dates, series, self.cfg.qlateral_files, self.cfg.discharge_files)

    got = []
    r = InMemory(params_file=str(params), qlateral_files=files, discharge_dir=str(tmp_path), log=False, channel_state_init_file=str(init),
                 runoff_processing_mode='ensemble', dt_routing=900, **cfg)
    r.set_write_discharges(lambda d, q, f, rf='': got.append((np.asarray(d), np.asarray(q), f, rf)))
    import logging
    r.logger = logging.getLogger('river_route_amd.test_ensemble')      # (log=False disables the router's own logger)
    r.logger.setLevel(25)
    r.route()
    return r, got


def _members(golden_routers, M, same_dates=True):
    g = golden_routers
    dates = [g['dates0'].astype('datetime64[s]') if same_dates or m % 2 == 0 else g['dates1'].astype('datetime64[s]') for m in range(M)]
    series = [g['vol0'] * (1.0 + 0.25 * m) + g['vol1'] * (0.1 * m) for m in range(M)]
    return dates, series


def _assert_same(a, b):
    (r1, got1), (r2, got2) = a, b
    assert len(got1) == len(got2)
    for (d1, q1, f1, rf1), (d2, q2, f2, rf2) in zip(got1, got2):
        assert np.array_equal(d1, d2) and (f1, rf1) == (f2, rf2)
        assert q1.dtype == q2.dtype == np.float32 and np.array_equal(q1.view(np.int32), q2.view(np.int32))
    assert len(r1._ensemble_member_states) == len(r2._ensemble_member_states)
    for s1, s2 in zip(r1._ensemble_member_states, r2._ensemble_member_states):
        assert np.array_equal(s1.view(np.int64), s2.view(np.int64))
    assert np.array_equal(r1.channel_state.view(np.int64), r2.channel_state.view(np.int64))


@pytest.mark.parametrize('cfg', [{}, {'dt_discharge': 3 * 3600}])      # float32 means fused into the group call / of float64 rows on the host
@pytest.mark.parametrize('cap,host_members,want', [(64, 100, [7]), (3, 100, [3, 3]), (64, 2, [2, 2, 2])])
def test_groups_respect_the_caps_and_give_what_the_loop_gives(monkeypatch, tmp_path, golden_routers, caplog, cfg, cap, host_members, want):
    dates, series = _members(golden_routers, 7)
    monkeypatch.setattr(LoopPlan, 'cap', cap)
    monkeypatch.setattr(LoopPlan, 'groups', [])
    monkeypatch.setattr(rr.RapidMuskingum, '_ensemble_host_bytes', host_members * series[0].nbytes)
    with caplog.at_level(25, logger='river_route_amd.test_ensemble'):
        batched = _route(monkeypatch, tmp_path, golden_routers, LoopPlan, dates, series, **cfg)
    assert LoopPlan.groups == want      # (a member left alone goes through the loop)
    progress = [r.getMessage() for r in caplog.records if r.levelno == 25 and 'reach-steps/s' in r.getMessage()]
    assert [p.rsplit(' for ', 1)[1] for p in progress] == [str(tmp_path / f'ql{i}.nc') for i in range(7)]      # one PROGRESS line per file, in order
    monkeypatch.setattr(LoopPlan, 'groups', [])
    loop = _route(monkeypatch, tmp_path, golden_routers, NoEnsemblePlan, dates, series, **cfg)
    assert LoopPlan.groups == []
    _assert_same(batched, loop)


@pytest.mark.parametrize('why', ['dates', 'direct', 'sequential'])
def test_falls_back_to_the_loop(monkeypatch, tmp_path, golden_routers, why):
    dates, series = _members(golden_routers, 4, same_dates=why != 'dates')
    monkeypatch.setattr(LoopPlan, 'groups', [])
    monkeypatch.setattr(LoopPlan, 'direct', why == 'direct')
    cfg = {'runoff_processing_mode': 'sequential'} if why == 'sequential' else {}
    if cfg:
        return _sequential_unchanged(monkeypatch, tmp_path, golden_routers, dates, series)
    batched = _route(monkeypatch, tmp_path, golden_routers, LoopPlan, dates, series)
    assert LoopPlan.groups == []
    _assert_same(batched, _route(monkeypatch, tmp_path, golden_routers, NoEnsemblePlan, dates, series))


def _sequential_unchanged(monkeypatch, tmp_path, golden_routers, dates, series):
    g = golden_routers
    params = tmp_path / 'params.parquet'
    pd.DataFrame({'river_id': g['river_ids'], 'downstream_river_id': g['downstream_ids'], 'k': g['k'], 'x': g['x']}).to_parquet(params)
    monkeypatch.setattr(musk_mod, 'Plan', LoopPlan)

    class InMemory(rr.RapidMuskingum):
        def _qlateral_generator(self):
            yield from zip(dates, series, self.cfg.qlateral_files, self.cfg.discharge_files)
    files = [str(tmp_path / f'ql{i}.nc') for i in range(len(series))]
    for f in files:
        open(f, 'w').close()
    r = InMemory(params_file=str(params), qlateral_files=files, discharge_dir=str(tmp_path), log=False, dt_routing=900,
                 runoff_processing_mode='sequential')
    r.set_write_discharges(lambda *a, **k: None)
    r.route()
    assert LoopPlan.groups == []      # sequential mode hands each member's state to the next: never batched
