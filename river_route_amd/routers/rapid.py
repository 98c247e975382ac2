"""`RapidMuskingum` (river_route/routers/RapidMuskingum.py:10-33): Muskingum routing with direct lateral inflow."""
from __future__ import annotations

import numpy as np

from .transform import TransformMuskingum

__all__ = ['RapidMuskingum']


class RapidMuskingum(TransformMuskingum):
    _as_volumes = True   # qlateral is a volume (m3) per runoff step

    def _lateral_coefficient(self) -> None:
        """c4 / dt_runoff turns a volume per runoff step into the discharge term of the routing step (RapidMuskingum.py:24)."""
        self._upload_coefficients(self.c4 / self.dt_runoff, ('rapid', int(self.dt_runoff)))

    def _router(self, qlateral: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
        state = np.array(self.channel_state, dtype=np.float64, order='C')
        routed = np.zeros((self.num_runoff_steps, state.shape[0]), dtype=np.float64)
        self._lateral_coefficient()
        self._plan.rapid_route(state, qlateral, routed, self.num_routing_steps_per_runoff)
        return state, routed

    _engine_router = _router

    def _route_ensemble_group(self, group: list) -> list | None:
        """Ensemble members (dates, lateral, in file, out file) with the same dates, routed together on the device (Plan.rapid_route_ensemble):
        [(final state, float32 discharge, seconds)] per member, each what _route_one_file gives for that member alone,
        or None where the group call does not apply (the members then go through the loop)."""
        import time
        from .. import engine
        from .._lib import RR_E_ALLOC, RR_E_UNSUPPORTED, RRError
        T, n, nsub, per = self.num_runoff_steps, self.A.shape[0], self.num_routing_steps_per_runoff, self.num_runoff_steps_per_discharge
        laterals = [item[1] for item in group]
        f32_in = all(q.dtype == np.float32 for q in laterals)
        ql = np.stack([np.asarray(q, dtype=np.float32 if f32_in else np.float64) for q in laterals])      # (float32 -> float64 is exact)
        fused = engine.REC_BATCH_ROWS % (per * nsub) == 0
        out = np.empty((len(group), T // per, n), np.float32) if fused else np.empty((len(group), T, n))
        self._lateral_coefficient()
        t0 = time.perf_counter()
        try:
            states = self._plan.rapid_route_ensemble(np.array(self.channel_state, dtype=np.float64), ql, out, nsub, factor=per if fused else 1)
        except RRError as e:
            if e.code not in (RR_E_UNSUPPORTED, RR_E_ALLOC):
                raise
            return None
        if not fused:      # rr_resample_cast_dev's arithmetic, as _route_one_file's host form: sequential sum over `per` rows, one division
            out = np.stack([(o.reshape((-1, per, n)).mean(axis=1) if per > 1 else o).astype(np.float32) for o in out])
        seconds = (time.perf_counter() - t0) / len(group)
        return [(states[k], out[k], seconds) for k in range(len(group))]

    # ---- the hooks of the per-file device driver (_device.route_file) ----
    def _device_state(self, arena):
        return arena.put(np.array(self.channel_state, dtype=np.float64, order='C'))

    def _device_state_back(self, d_q) -> np.ndarray:
        return d_q.download(np.float64, (self.A.shape[0],))

    def _device_calls(self) -> dict:
        """The engine call per (rows in, rows out): lateral volumes as float64 rows, as float32 rows (converted in the pass that fills
        the engine's records) or as gridded runoff (computed in that pass: _device.RunoffPieces); discharge as float32 rows, each the
        mean of `per` routed rows, or as float64 rows."""
        plan, nsub, per = self._plan, self.num_routing_steps_per_runoff, self.num_runoff_steps_per_discharge
        return {
            ('f64', 'f32'): lambda d_q, d_ql, T, d_out: plan.rapid_route_f32_dev(d_q, d_ql, T, d_out, T, nsub, per),
            ('f64', 'f64'): lambda d_q, d_ql, T, d_out: plan.rapid_route_dev(d_q, d_ql, T, d_out, T, T, nsub),
            ('f32', 'f32'): lambda d_q, d_ql, T, d_out: plan.rapid_route_f32in_dev(d_q, d_ql, T, T, nsub, discharge32=d_out, factor=per),
            ('f32', 'f64'): lambda d_q, d_ql, T, d_out: plan.rapid_route_f32in_dev(d_q, d_ql, T, T, nsub, discharge=d_out, out_rows=T),
            ('runoff', 'f32'): lambda d_q, r, T, d_out: plan.rapid_route_runoff_dev(
                d_q, r.n_points, r.indptr, r.indices, r.weights, r.block, r.is_f32, 1, r.stride_p, r.area, r.flags, T, discharge32=d_out, factor=per),
        }

