"""
`UnitMuskingum` (river_route/routers/UnitMuskingum.py:11-104): unit-hydrograph lateral inflow superimposed on
Muskingum channel routing; headwaters carry the convolved runoff only.
"""
from __future__ import annotations

import numpy as np

from ..uhkernels import UnitHydrograph
from .transform import TransformMuskingum

__all__ = ['UnitMuskingum']


class UnitMuskingum(TransformMuskingum):
    _ROUTER_REQUIRED_CONFIGS = ('uh_kernel_file',)
    _uh: UnitHydrograph | None = None
    _as_volumes = False   # inputs are runoff depths (m)

    def _hook_before_route(self) -> None:
        if self._uh is None:
            self.logger.debug('Loading UH kernel')
            self._uh = UnitHydrograph(self.cfg.uh_kernel_file, device=self.cfg.device)
            if self.cfg.uh_state_init_file:
                self._uh.set_state(self.cfg.uh_state_init_file)
        if not hasattr(self, 'hw_idx'):
            incoming = np.asarray(self.A.sum(axis=1)).flatten()
            self.hw_idx = np.where(incoming == 0)[0]
            self.inner_idx = np.where(incoming != 0)[0]
            self.logger.info(
                f'Headwater split: {len(self.hw_idx)} headwater, {len(self.inner_idx)} inner '
                f'({len(self.hw_idx) / self.A.shape[0] * 100:.0f}% excluded from solve)')

    def _check_kernel(self) -> None:
        """The kernel file must describe this network: one column of taps per reach (scipy's fftconvolve raises in the
        reference; raw device addresses would not)."""
        n = self.A.shape[0]
        if self._uh.kernel.ndim != 2 or self._uh.kernel.shape[1] != n or np.shape(self._uh.state) != self._uh.kernel.shape:
            raise ValueError(f'unit-hydrograph kernel {self._uh.kernel.shape} / state {np.shape(self._uh.state)} do not match '
                             f'the network: expected (n_kernel_steps, {n})')

    def _seed(self) -> np.ndarray:
        """Channel and full discharge of the inner reaches both restart from channel_state at every file (UnitMuskingum.py:78-79)."""
        return np.array(self.channel_state[self.inner_idx], dtype=np.float64, order='C')

    def _router(self, qlateral: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
        self._check_kernel()
        lateral = self._uh.convolve(qlateral)                       # rr_uh_convolve
        n = self.river_ids.shape[0]
        routed = np.zeros((self.num_runoff_steps, n), dtype=np.float64)
        q_ch = self._seed()
        q_full = q_ch.copy()
        self._upload_coefficients(None, ('unit',))
        self._plan.unit_route(q_ch, q_full, lateral, routed, self.num_routing_steps_per_runoff)
        state = np.empty(n, dtype=np.float64)
        state[self.hw_idx] = lateral[-1][self.hw_idx]       # a headwater's state is its last lateral inflow
        state[self.inner_idx] = q_full
        return state, routed

    _engine_router = _router

    # ---- the hooks of the per-file device driver (_device.route_file) ----
    def _lateral_coefficient(self) -> None:
        """The convolved inflow enters the routing step as it is: three coefficients, no fourth."""
        self._check_kernel()
        self._upload_coefficients(None, ('unit',))

    def _check_shape(self, shape: tuple) -> None:
        self._check_kernel()      # (first, as before the depths were ever looked at: a kernel of another network is the error to report)
        super()._check_shape(shape)

    def _device_state(self, arena):
        """Kernel and UH state, the seed as channel and as full discharge of the inner reaches, and room for the router state the
        fused calls write (UnitMuskingum.py:95-97)."""
        from types import SimpleNamespace
        seed = self._seed()
        kern, uh = arena.put(self._uh.kernel), arena.put(np.ascontiguousarray(self._uh.state, dtype=np.float64))
        return SimpleNamespace(kern=kern, uh=uh, q_ch=arena.put(seed), q_full=arena.put(seed), final=arena.empty(self.A.shape[0] * 8), conv=None, T=0)

    def _device_state_back(self, s) -> np.ndarray:
        """The router state, then the UH state: an input the engine refused in every form has left it as it was."""
        n = self.A.shape[0]
        if s.conv is None:
            state = s.final.download(np.float64, (n,))
        else:
            state = s.conv.download(np.float64, (n,), offset=(s.T - 1) * n * 8)    # headwaters keep the last lateral row
            state[self.inner_idx] = s.q_full.download(np.float64, self.inner_idx.shape)
        self._uh.state = s.uh.download(np.float64, self._uh.kernel.shape)
        return state

    def _device_calls(self) -> dict:
        """The engine call per (rows in, rows out).  Runoff depths, float64 or float32 rows: the convolution fused into the pass that turns
        rows into records, so the convolved lateral never exists as rows (a time-tiled call, at most 64 kernel steps; float32 discharge
        only).  'conv', the convolved rows of _device_lower: the routing calls."""
        plan, nsub, per, n_ks = self._plan, self.num_routing_steps_per_runoff, self.num_runoff_steps_per_discharge, self._uh.kernel.shape[0]
        return {
            ('f64', 'f32'): lambda s, d_depth, T, d_out: plan.unit_route_uh_dev(
                s.q_ch, s.q_full, s.final, s.kern, s.uh, n_ks, d_depth, T, nsub, discharge32=d_out, factor=per),
            ('f32', 'f32'): lambda s, d_depth, T, d_out: plan.unit_route_uh_f32in_dev(
                s.q_ch, s.q_full, s.final, s.kern, s.uh, n_ks, d_depth, T, nsub, discharge32=d_out, factor=per),
            ('conv', 'f32'): lambda s, d_conv, T, d_out: plan.unit_route_f32_dev(s.q_ch, s.q_full, d_conv, T, d_out, T, nsub, per),
            ('conv', 'f64'): lambda s, d_conv, T, d_out: plan.unit_route_dev(s.q_ch, s.q_full, d_conv, T, d_out, T, T, nsub),
        }

    def _device_lower(self, arena, s, kind: str, d_depth, T: int):
        """Float64 depths the fused call refused: rr_uh_convolve_dev into rows of their own, ('conv', rows).  Float32 depths: None, the
        driver widens them."""
        from ..engine import uh_convolve_dev
        if kind != 'f64':
            return None
        s.conv, s.T = arena.empty(T * self.A.shape[0] * 8), T
        uh_convolve_dev(s.kern, s.uh, d_depth, s.conv, T, self._uh.kernel.shape[0], self.A.shape[0], device=self.cfg.device)
        return 'conv', s.conv

    def _write_final_state(self) -> None:
        super()._write_final_state()
        if self.cfg.uh_state_final_file and self._uh is not None:
            self._uh.write_state(self.cfg.uh_state_final_file)
