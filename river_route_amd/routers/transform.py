"""
`TransformMuskingum`: the shared per-file driver of the routers that take lateral inflow
(river_route/routers/TransformMuskingum.py:14-152): input generator, time-step algebra, sequential / ensemble
state hand-off, resampling to dt_discharge and the float32 cast before the writer.
"""
from __future__ import annotations

from abc import ABC, abstractmethod

import numpy as np

from .muskingum import PROGRESS, Muskingum

__all__ = ['TransformMuskingum']


class TransformMuskingum(Muskingum, ABC):
    _ROUTER_REQUIRED_CONFIGS: tuple[str, ...] = ()
    _as_volumes: bool = False
    _device_postprocess: bool = True   # keep each file on the GPU from lateral upload to float32 discharge

    def _qlateral_generator(self):
        """Yields (dates datetime64[s], lateral float64 (T, n), input file, output file) per input file."""
        if self.cfg.qlateral_files:
            from ..io import read_qlateral
            for lateral_file, discharge_file in zip(self.cfg.qlateral_files, self.cfg.discharge_files):
                self.logger.info('-' * 60)
                rows = self._file_rows(lateral_file)
                if rows is not None:      # a NetCDF-3 float32 file: its rows go from the page cache to the device as they are (nc3.py)
                    yield rows[0], rows[1], lateral_file, discharge_file
                    continue
                # a router that converts on the device takes a float32 file as float32 (RapidMuskingum: rr_rapid_route_f32in_dev)
                dates, array = read_qlateral(lateral_file, self.cfg.var_t, keep_float32=self._own_engine_path())
                yield dates, array, lateral_file, discharge_file
        elif self.cfg.grid_runoff_files and self.cfg.grid_weights_file:
            # gridded runoff -> catchment inflow on the device (TransformMuskingum.py:38-51 -> runoff.runoff_to_qlateral).  A
            # router on its own engine path gets the prepared source instead of the (time, river) array, so the inflow is
            # computed on the device, where the engine takes that on its way into the engine's records (_device.route_file)
            from ..runoff import prepare_runoff, runoff_to_qlateral
            kw = dict(grid_weights_file=self.cfg.grid_weights_file, var_runoff=self.cfg.var_grid_runoff, var_x=self.cfg.var_x,
                      var_y=self.cfg.var_y, var_t=self.cfg.var_t, var_river_id=self.cfg.var_river_id,
                      cumulative=self.cfg.grid_accumulation_type == 'cumulative', device=self.cfg.device)
            for runoff_file, discharge_file in zip(self.cfg.grid_runoff_files, self.cfg.discharge_files):
                self.logger.info('-' * 60)
                self.logger.debug(f'Calculating qlateral: {runoff_file}')
                if self._own_engine_path():
                    src = prepare_runoff(runoff_file, **kw)
                    if not src.irregular:
                        yield src.time_index.astype('datetime64[s]'), src, runoff_file, discharge_file
                        continue
                ds = runoff_to_qlateral(runoff_file, as_volumes=self._as_volumes, **kw)
                yield (ds['time'].values.astype('datetime64[s]'),
                       ds['qlateral'].values.astype(np.float64, copy=False), runoff_file, discharge_file)

    def _file_rows(self, lateral_file):
        """(dates, nc3.RowBlock) where the router can take a qlateral file's rows straight from the file -- a flat (NetCDF-3) float32
        variable, the router's own engine path and the default discharge writer -- else None."""
        if not (self._own_engine_path() and '_write_discharges' not in self.__dict__ and type(self)._write_discharges is Muskingum._write_discharges):
            return None
        from .. import nc3
        from ..io import _decode_cf_time
        blk = nc3.locate_rows(lateral_file, 'qlateral')
        if blk is None or blk.dtype.kind != 'f' or blk.dtype.itemsize != 4 or blk.cols != self.A.shape[0] or blk.rows < 2:
            return None
        try:
            values, atts = nc3.read_vector(lateral_file, self.cfg.var_t)
            return _decode_cf_time(values, atts['units']), blk
        except (KeyError, ValueError):
            return None

    def _validate_router_configs(self) -> None:
        laterals = list(self.cfg.qlateral_files or [])
        grids = list(self.cfg.grid_runoff_files or []) if self.cfg.grid_weights_file else []
        if laterals and self.cfg.grid_runoff_files and self.cfg.grid_weights_file:
            raise ValueError('Provide qlateral_files or grid_runoff_files with grid_weights_file, not both')
        if not laterals and not grids:
            raise ValueError('Provide qlateral_files or grid_runoff_files with grid_weights_file')
        if len(self.cfg.discharge_files) != len(laterals) + len(self.cfg.grid_runoff_files or []):
            raise ValueError('Number of resolved discharge output files must match number of input files')

    # the four time steps, coarsest first, and the rule each adjacent pair obeys (docs/references/time-options.md:32-50)
    _STEP_PAIRS = (('dt_total', 'dt_runoff'), ('dt_total', 'dt_discharge'), ('dt_discharge', 'dt_runoff'), ('dt_runoff', 'dt_routing'))

    def _set_network_and_time_dependent_vectors(self, dates: np.ndarray) -> None:
        """Time-step defaults and rules (river_route/routers/TransformMuskingum.py:66-106), then the coefficients."""
        self.logger.debug('Setting and validating time parameters')
        cfg = self.cfg
        from_dates = int((dates[1] - dates[0]).astype('timedelta64[s]').astype(int)) if not cfg.dt_runoff else None
        self.dt_runoff = cfg.dt_runoff or from_dates
        self.dt_discharge = cfg.dt_discharge or self.dt_runoff
        self.dt_total = cfg.dt_total or self.dt_runoff * dates.shape[0]
        if not cfg.dt_routing:
            self.logger.warning('dt_routing was not provided or is Null/False, defaulting to dt_runoff')
        self.dt_routing = cfg.dt_routing or self.dt_runoff

        steps = (self.dt_total, self.dt_runoff, self.dt_discharge, self.dt_routing)
        if steps == self._network_time_signature:
            return      # same grid as the previous file: counts and coefficients stand
        value = dict(zip(('dt_total', 'dt_runoff', 'dt_discharge', 'dt_routing'), steps))
        for rule, message in ((lambda a, b: a >= b, '{} must be >= {}'), (lambda a, b: a % b == 0, '{} must be an integer multiple of {}')):
            for coarse, fine in self._STEP_PAIRS:
                if not rule(value[coarse], value[fine]):
                    raise ValueError(message.format(coarse, fine))
        self.num_runoff_steps = self.dt_total // self.dt_runoff
        self.num_runoff_steps_per_discharge = self.dt_discharge // self.dt_runoff
        self.num_routing_steps_per_runoff = self.dt_runoff // self.dt_routing
        self._set_muskingum_coefficients(self.dt_routing)
        self.c4 = self.c1 + self.c2
        self._network_time_signature = steps

    def _own_engine_path(self, plan_call: str = 'rapid_route_dev') -> bool:
        """Whether this router keeps its files on the GPU: device post-processing is on, `_router` is the engine's own (a subclass that
        brings its own `_router`, the reference's extension point, gets the host path) and the plan has the device calls (feature test
        on `plan_call`: a stand-in plan without it gets the host path)."""
        return (self._device_postprocess and type(self)._router is getattr(type(self), '_engine_router', None)
                and hasattr(self._plan, plan_call))

    def _route_one_file(self, source, sink=None) -> tuple[np.ndarray, np.ndarray | None]:
        """(final state, float32 discharge at dt_discharge) of one file: on the GPU from the lateral upload to the float32 rows
        (_device.route_file, which also decides when a file must take the host path after all), or on the host."""
        if self._own_engine_path():
            from ._device import route_file
            return route_file(self, source, sink)
        return self._route_on_host(source)

    def _route_on_host(self, qlateral: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
        """`_router` + the post-processing of TransformMuskingum.py:128-142 on the host."""
        per = self.num_runoff_steps_per_discharge
        q_t, q_array = self._router(qlateral)
        if per > 1:
            q_array = q_array.reshape((-1, per, q_array.shape[1])).mean(axis=1)
        return q_t, q_array.astype(np.float32, copy=False)

    def _execute_routing(self) -> None:
        members: list[np.ndarray] = []
        files = self._qlateral_generator()
        if self.cfg.progress_bar:
            from tqdm import tqdm
            files = tqdm(files, total=len(self.cfg.qlateral_files or self.cfg.grid_runoff_files), desc='Files Routed')
        sequential = self.cfg.runoff_processing_mode == 'sequential'
        # ensemble mode: consecutive members with the same dates may be routed together (_route_ensemble_group); each member is then
        # written, logged and kept exactly as the loop below does it for a file of its own
        batching = not sequential and self._ensemble_batching()
        pending: list[tuple] = []

        def flush():
            group = list(pending)
            pending.clear()
            routed = self._route_ensemble_group(group) if len(group) > 1 else None
            for k, item in enumerate(group):
                self._route_and_write(*item, sequential, members, routed[k] if routed else None)

        for item in files:
            if pending and not self._joins_ensemble_group(pending, item):
                flush()
            if batching and self._ensemble_candidate(item, first=not pending):
                pending.append(item)
                continue
            flush()
            self._route_and_write(*item, sequential, members)
        flush()
        if not sequential:
            self._ensemble_member_states = members
            self.channel_state = np.mean(np.array(members), axis=0)
        self.logger.info('-' * 60)

    def _route_and_write(self, dates, qlateral, runoff_file, discharge_file, sequential: bool, members: list, routed=None) -> None:
        """One input file: route it (or take `routed` = (final state, float32 discharge, seconds) of a batched ensemble group), log,
        hand the state on, write."""
        import time
        self.logger.info(f'Routing qlateral: {runoff_file}')
        self._set_network_and_time_dependent_vectors(dates)
        self.logger.debug('Starting routing computation')
        t0 = time.perf_counter()
        if routed is not None:
            q_t, q_array, seconds = routed
        else:      # (a file's rows go to the discharge file where the engine takes them from file to file: no array comes back then)
            q_t, q_array = self._route_one_file(qlateral, (discharge_file, dates[::self.num_runoff_steps_per_discharge], runoff_file))
            seconds = time.perf_counter() - t0
        reach_steps = self.A.shape[0] * self.num_runoff_steps * self.num_routing_steps_per_runoff
        self.logger.log(PROGRESS, f'{reach_steps / max(seconds, 1e-9):.3e} reach-steps/s '
                                  f'({reach_steps * 16 / max(seconds, 1e-9) / 1e9:.1f} GB/s of lateral + discharge rows) for {runoff_file}')
        if sequential:
            self.channel_state = q_t
        else:
            members.append(np.array(q_t, copy=True))
        if self.num_runoff_steps_per_discharge > 1:
            self.logger.debug('Resampling dates and discharges to specified timestep')
            dates = dates[::self.num_runoff_steps_per_discharge]
        if q_array is not None:
            self.logger.debug('Writing Discharge Array to File')
            self._write_discharges(dates, q_array, discharge_file, runoff_file)

    # ---- ensemble members routed together (RapidMuskingum: Plan.rapid_route_ensemble) ----
    _ensemble_host_bytes = 8 << 30      # lateral rows of one group held in host memory at once

    def _ensemble_batching(self) -> bool:
        """The router batches ensemble members where it has the group call, the plan has the ensemble call (feature test: a stand-in plan
        without it keeps the loop) and its own engine path and device post-processing are in force."""
        return hasattr(self, '_route_ensemble_group') and self._own_engine_path('rapid_route_ensemble')

    def _joins_ensemble_group(self, pending: list, item) -> bool:
        dates, qlateral = item[0], item[1]
        first = pending[0][1]
        return (isinstance(qlateral, np.ndarray) and np.array_equal(np.asarray(dates), np.asarray(pending[0][0]))
                and qlateral.shape == first.shape and len(pending) < self._ensemble_cap
                and sum(p[1].nbytes for p in pending) + qlateral.nbytes <= self._ensemble_host_bytes)

    @staticmethod
    def _ensemble_batch_wins(n: int, T: int, nsub: int) -> bool:
        """The crossover: a group beats the loop of single-member calls 1.6x - 2.9x at 100k reaches, where one member
        leaves most of the card idle and pays the pipeline's fill and drain, and loses at 1M reaches (0.97x), where one member fills the card
        and only ten members' record rings fit it.  Batch below half a million reaches.  (T x nsub >= 32: the time-tiled kernel's minimum.)"""
        return n < 500_000 and T * nsub >= 32

    def _ensemble_candidate(self, item, first: bool) -> bool:
        """Whether this member may be routed in a group: an array (not a file's rows or gridded runoff) of the expected shape, a single
        member's call would not take the direct row path (faster per member), the crossover says the group wins and at least two
        members' rings fit the card.  `first`: no group is open, so the time options may be set from this member's dates."""
        from .. import engine
        dates, qlateral = item[0], item[1]
        if not (isinstance(qlateral, np.ndarray) and qlateral.dtype in (np.float32, np.float64) and qlateral.ndim == 2 and dates.shape[0] >= 2):
            return False
        if not first:
            return True      # (_joins_ensemble_group has compared it with the group's first member)
        self._set_network_and_time_dependent_vectors(dates)
        T, n, nsub, per = self.num_runoff_steps, self.A.shape[0], self.num_routing_steps_per_runoff, self.num_runoff_steps_per_discharge
        if qlateral.shape != (T, n) or not self._ensemble_batch_wins(n, T, nsub):
            return False
        from .._lib import RRError
        try:
            self._lateral_coefficient()      # (a reservation needs the plan's coefficients: they decide which kernel routes)
            fused = engine.REC_BATCH_ROWS % (per * nsub) == 0
            if self._plan.reserve(engine.MODE_RAPID, T, nsub, f32_out=fused).get('direct'):
                return False
            self._ensemble_cap = int(self._plan.reserve_ensemble(1, T, nsub, f32_in=qlateral.dtype == np.float32, f32_out=fused)['members_max'])
        except RRError:
            return False
        return self._ensemble_cap >= 2

    @abstractmethod
    def _router(self, qlateral: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
        """(final state float64[n], discharge float64[T, n]) for one input file, host arrays."""

    # ---- what the per-file device driver (_device.route_file) asks of a router with an engine path of its own (`_engine_router`) ----
    #   _lateral_coefficient()            put the router's coefficients on the plan (they stay there until recomputed)
    #   _device_state(arena) -> state     upload the router's state; the handle goes to the engine calls and to _device_state_back
    #   _device_state_back(state)         the final state float64[n] after a routing call the engine took
    #   _device_calls()                   {(rows in, rows out): call(state, d_in, T, d_out)}: in 'f64' | 'f32' | 'runoff', out 'f32' | 'f64'
    def _device_lower(self, arena, state, kind: str, d_rows, T: int):
        """(kind, rows) the router makes of rows the engine refused in every form of their own, or None."""
        return None

    def _check_lateral(self, qlateral: np.ndarray, keep_float32: bool = False) -> np.ndarray:
        qlateral = np.asarray(qlateral)
        ql = np.ascontiguousarray(qlateral, dtype=np.float32 if keep_float32 and qlateral.dtype == np.float32 else np.float64)
        self._check_shape(ql.shape)
        return ql

    def _check_shape(self, shape: tuple) -> None:
        """The rows of one input, an array's or a file's, are those the time options and the network expect."""
        if tuple(shape) != (self.num_runoff_steps, self.A.shape[0]):
            raise ValueError(f'lateral inflow has shape {tuple(shape)}, expected '
                             f'({self.num_runoff_steps}, {self.A.shape[0]}) from the time options')
