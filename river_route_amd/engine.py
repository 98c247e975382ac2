"""
Python handle on an rr_plan (include/rr_hip.h): network layout + device-resident coefficients + route calls.
Host arrays are numpy; `*_dev` methods take raw device addresses / torch tensors and a HIP stream handle.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import RRError, check, ptr

__all__ = ['Plan', 'RRError', 'uh_convolve', 'uh_convolve_dev', 'uh_adjoint_work_bytes', 'uh_adjoint_dev', 'runoff_to_qlateral', 'DeviceBuffer', 'partition_forest', 'synchronize',
           'resample_cast_dev', 'copy_bandwidth', 'runoff_to_qlateral_dev', 'runoff_adjoint_work_bytes', 'runoff_adjoint_dev', 'rows_upload', 'rows_download', 'metrics_work_bytes',
           'metrics_update_dev', 'metrics_finish_dev', 'metrics_adjoint_work_bytes', 'metrics_adjoint_dev', 'metrics_update_missing_dev',
           'metrics_adjoint_missing_dev', 'grid_overlap_area',
           'grid_overlap_area_dev']


MODE_RAPID, MODE_MUSKINGUM, MODE_UNIT = 0, 1, 2      # include/rr_hip.h: RR_MODE_*
REC_BATCH_ROWS = 128      # tick-rows of a record batch: float32 means fused into the out-pass need factor x sub-steps to divide it


def _f64(a, name):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if not a.flags['WRITEABLE']:
        a = a.copy()
    return a


def _inplace_f64(a, name, shape):
    if not (isinstance(a, np.ndarray) and a.dtype == np.float64 and a.flags['C_CONTIGUOUS'] and a.flags['WRITEABLE']):
        raise TypeError(f'{name} must be a writeable C-contiguous float64 numpy array (it is updated in place)')
    if a.shape != shape:
        raise ValueError(f'{name} has shape {a.shape}, expected {shape}')
    return a


class Plan:
    """Structure analysis of one river network, bound to one GPU.  Built from the CSC adjacency the reference's
    routers hold (river_route/routers/Muskingum.py:189-191)."""

    def __init__(self, csc_indptr, csc_indices, device: int = 0):
        indptr = np.ascontiguousarray(csc_indptr, dtype=np.int32)
        indices = np.ascontiguousarray(csc_indices, dtype=np.int32)
        if indptr.ndim != 1 or indptr.shape[0] < 1:
            raise ValueError('csc_indptr must be a 1-D array of length n + 1')
        self.n = int(indptr.shape[0] - 1)
        if indices.shape[0] != int(indptr[-1]):
            raise ValueError('csc_indices length does not match csc_indptr[-1]')
        self.device = int(device)
        self._h = C.c_void_p()
        check(_lib.lib().rr_plan_create(self.n, ptr(indptr), ptr(indices) if indices.size else None,
                                        self.device, C.byref(self._h)))
        self._indptr, self._indices = indptr, indices
        info = np.zeros(8, dtype=np.int64)
        check(_lib.lib().rr_plan_info(self._h, ptr(info)))
        self.n_edges, self.depth, self.widest_level, self.n_headwaters, self.n_outlets = (int(v) for v in info[1:6])
        self.identity_order = bool(info[6])
        self.n_inner = self.n - self.n_headwaters

    # -- lifetime --
    def close(self) -> None:
        if getattr(self, '_h', None) is not None and self._h.value:
            _lib.lib().rr_plan_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- inspection --
    def layout(self):
        """(perm, lag, child_ptr) of the engine order, see rr_plan_layout."""
        perm = np.empty(self.n, dtype=np.int32)
        lag = np.empty(self.n, dtype=np.int32)
        child_ptr = np.empty(self.n + 1, dtype=np.int32)
        check(_lib.lib().rr_plan_layout(self._h, ptr(perm), ptr(lag), ptr(child_ptr)))
        return perm, lag, child_ptr

    def tile_info(self) -> dict:
        """Shape of the time-tiled kernel's layout, see rr_plan_tile_info."""
        info = np.zeros(8, dtype=np.int64)
        check(_lib.lib().rr_plan_tile_info(self._h, ptr(info)))
        return dict(ok=bool(info[0]), block=int(info[1]), positions=int(info[2]), ghosts=int(info[3]), tiles=int(info[4]),
                    levels=int(info[5]), threads=int(info[6]), batch_rows=int(info[7]))

    def inpass_info(self) -> dict:
        """Headwaters the in-pass routes, see rr_plan_inpass_info."""
        info = np.zeros(5, dtype=np.int64)
        check(_lib.lib().rr_plan_inpass_info(self._h, ptr(info)))
        return dict(enabled=bool(info[0]), eligible=int(info[1]), headwater_positions=int(info[2]), mirrored_or_boundary=int(info[3]),
                    wide_tile=int(info[4]))

    def tile_layout(self) -> dict:
        """Arrays of the subtree-tile layout, see rr_plan_tile_layout."""
        t = self.tile_info()
        nt, npos = t['tiles'], t['positions']
        out = dict(tile_ptr=np.empty(nt + 1, np.int32), tile_level=np.empty(nt, np.int32), perm=np.empty(npos, np.int32),
                   lag=np.empty(npos, np.int32), cfirst=np.empty(npos, np.int32), ccnt=np.empty(npos, np.uint32),
                   xpos=np.empty(npos, np.int32))
        check(_lib.lib().rr_plan_tile_layout(self._h, *(ptr(out[k]) for k in ('tile_ptr', 'tile_level', 'perm', 'lag', 'cfirst',
                                                                               'ccnt', 'xpos'))))
        return out

    def set_options(self, rows_per_chunk: int = 0, sample_every: int = -1) -> None:
        check(_lib.lib().rr_plan_set_options(self._h, int(rows_per_chunk), int(sample_every)))

    def set_row_format(self, in32_big_endian: bool = False, out32_big_endian: bool = False) -> None:
        """rr_plan_set_row_format: the float32 rows of the calls to come are big-endian (a NetCDF-3 file's bytes as they are)."""
        check(_lib.lib().rr_plan_set_row_format(self._h, int(bool(in32_big_endian)), int(bool(out32_big_endian))))

    def profile(self) -> dict:
        p = np.zeros(10, dtype=np.float64)
        check(_lib.lib().rr_plan_profile(self._h, ptr(p)))
        return dict(launches=int(p[0]), sampled=int(p[1]), sampled_ms=float(p[2]), min_ms=float(p[3]),
                    max_ms=float(p[4]), sampled_reaches=float(p[5]), region_ms=float(p[6]), reach_steps=float(p[7]),
                    brackets=int(p[8]), ticks_per_launch=int(p[9]))

    def profile_aux(self) -> dict:
        """rr_plan_profile_aux: the kernels around the routing kernel in the last call, {name: {launches, sampled, sampled_ms}}."""
        a = np.zeros(12, dtype=np.float64)
        check(_lib.lib().rr_plan_profile_aux(self._h, ptr(a)))
        names = ('k_rec_in', 'k_rec_out', 'k_tile (skeleton)', 'k_rec_out (holes)')
        return {nm: dict(launches=int(a[3 * k]), sampled=int(a[3 * k + 1]), sampled_ms=float(a[3 * k + 2])) for k, nm in enumerate(names) if a[3 * k] > 0}

    # -- coefficients --
    def set_coeffs(self, lhs_off_data, c2, c3, c4_dt=None) -> None:
        lhs = _f64(lhs_off_data, 'lhs_off_data')
        c2, c3 = _f64(c2, 'c2'), _f64(c3, 'c3')
        if lhs.shape != (self.n_edges,) or c2.shape != (self.n,) or c3.shape != (self.n,):
            raise ValueError('coefficient arrays do not match the plan (lhs_off_data per CSC entry, c2/c3 per reach)')
        c4 = None
        if c4_dt is not None:
            c4 = _f64(c4_dt, 'c4_dt')
            if c4.shape != (self.n,):
                raise ValueError('c4_dt must have one value per reach')
        check(_lib.lib().rr_plan_set_coeffs(self._h, ptr(lhs) if lhs.size else None, ptr(c2), ptr(c3), ptr(c4)))

    def set_unit_weights(self, c1=None, a_data=None) -> None:
        """rr_plan_set_unit_weights: general a_inner_data / a_hw_data (per CSC entry) and c1 per reach for unit_route; None, None
        goes back to the unit weights of the reference's callers."""
        if c1 is None and a_data is None:
            check(_lib.lib().rr_plan_set_unit_weights(self._h, None, None))
            return
        c1, a = _f64(c1, 'c1'), _f64(a_data, 'a_data')
        if c1.shape != (self.n,) or a.shape != (self.n_edges,):
            raise ValueError('c1 must have one value per reach and a_data one per CSC entry')
        check(_lib.lib().rr_plan_set_unit_weights(self._h, ptr(c1), ptr(a) if a.size else None))

    # -- host-array routing: the reference's kernel boundary --
    def rapid_route(self, q_t, qlateral, discharge_array, num_substeps: int) -> None:
        ql = np.ascontiguousarray(qlateral, dtype=np.float64)
        if ql.ndim != 2 or ql.shape[1] != self.n:
            raise ValueError(f'qlateral must have shape (T, {self.n})')
        T = ql.shape[0]
        _inplace_f64(q_t, 'q_t', (self.n,))
        _inplace_f64(discharge_array, 'discharge_array', (T, self.n))
        check(_lib.lib().rr_rapid_route(self._h, ptr(q_t), ptr(ql), ptr(discharge_array), T, int(num_substeps)))

    def muskingum_route(self, q_t, discharge_array, num_output_steps: int, num_routing_per_output: int) -> None:
        _inplace_f64(q_t, 'q_t', (self.n,))
        _inplace_f64(discharge_array, 'discharge_array', (int(num_output_steps), self.n))
        check(_lib.lib().rr_muskingum_route(self._h, ptr(q_t), ptr(discharge_array), int(num_output_steps),
                                            int(num_routing_per_output)))

    def unit_route(self, q_ch, q_full, convolved_lateral, discharge_array, num_substeps: int) -> None:
        conv = np.ascontiguousarray(convolved_lateral, dtype=np.float64)
        if conv.ndim != 2 or conv.shape[1] != self.n:
            raise ValueError(f'convolved_lateral must have shape (T, {self.n})')
        T = conv.shape[0]
        _inplace_f64(q_ch, 'q_ch', (self.n_inner,))
        _inplace_f64(q_full, 'q_full', (self.n_inner,))
        _inplace_f64(discharge_array, 'discharge_array', (T, self.n))
        check(_lib.lib().rr_unit_route(self._h, ptr(q_ch), ptr(q_full), ptr(conv), ptr(discharge_array), T,
                                       int(num_substeps)))

    # -- work memory --
    def reserve(self, mode: int, T: int, num_substeps: int = 1, host_rows: bool = False, plain_rows: bool = True, f32_out: bool = False, uh: bool = False) -> dict:
        """rr_plan_reserve: allocate what route calls of up to T rows x num_substeps sub-steps work in (the record ring, events,
        with host_rows the PCIe staging).  The *_dev entry points of the C ABI only enqueue and fail with RR_E_STATE when this
        has not been done; the methods below call it for the shape they are given (no-op once large enough).  plain_rows=False:
        the call hands over no lateral rows in a device array (fused convolution, gridded runoff), so the direct row path does not
        apply (RR_ROWS_NOT_PLAIN); f32_out: it writes float32 rows (RR_ROWS_F32_OUT); uh: it is unit_route_uh*_dev (RR_ROWS_UH: on the
        direct row path the convolved rows are work memory)."""
        info = np.zeros(8, dtype=np.int64)
        check(_lib.lib().rr_plan_reserve(self._h, int(mode), int(T), int(num_substeps), int(bool(host_rows)) | (0 if plain_rows else 2) | (4 if f32_out else 0) | (8 if uh else 0), ptr(info)))
        if int(info[0]) == 0 and int(T) * int(num_substeps) >= 32 and self.n > 0 and not getattr(self, '_warned_streaming', False):
            # the time-tiled kernel takes every call of 32 sub-steps or more -- unless the network does not tile, the coefficients give the
            # tributaries of a reach different weights, or its record ring (depth + tile levels x K tick-rows of every reach) does not fit
            # the card: the streaming kernel then routes at about a third of the rate.  Say so once, where the routers' log shows it.
            import logging
            self._warned_streaming = True
            logging.getLogger('river_route_amd').warning(
                'routing %d reaches (network depth %d) with the streaming kernel k_tick: the time-tiled kernel does not apply to this call '
                '(record ring too large for the device, per-edge weights, or a reach with more tributaries than a tile holds); '
                'expect about a third of its rate', self.n, self.depth)
        return dict(tiled=int(info[0]) == 1, direct=int(info[0]) == 2, ticks_per_launch=int(info[1]), ring_chunks=int(info[2]), work_bytes=int(info[3]),
                    staging_bytes=int(info[4]), pinned_bytes=int(info[5]), pipeline_ticks=int(info[6]), ring_bytes=int(info[7]))

    def direct_info(self) -> dict:
        """Whether the direct row path applies to this plan (the params order numbers small subtrees contiguously) and its shape,
        see rr_plan_direct_info."""
        info = np.zeros(8, dtype=np.int64)
        why = C.create_string_buffer(256)
        check(_lib.lib().rr_plan_direct_info(self._h, ptr(info), C.cast(why, C.c_void_p), 256))
        return dict(ok=bool(info[0]), tiles=int(info[1]), holes=int(info[2]), outlets=int(info[3]), skeleton_positions=int(info[4]),
                    skeleton_tiles=int(info[5]), skeleton_levels=int(info[6]), window_rows=int(info[7]), why=why.value.decode())

    def direct_layout(self) -> dict:
        """Arrays of the direct row path's layout, see rr_plan_direct_layout."""
        nt = self.direct_info()['tiles']
        out = dict(tile_c0=np.empty(nt, np.int32), tile_nc=np.empty(nt, np.int32), tile_lag_lo=np.empty(nt, np.int32), tile_span=np.empty(nt, np.int32),
                   delay=np.empty(self.n, np.int32), up3=np.empty(self.n, np.int32), xinfo=np.empty(self.n, np.int32))
        check(_lib.lib().rr_plan_direct_layout(self._h, *(ptr(out[k]) for k in ('tile_c0', 'tile_nc', 'tile_lag_lo', 'tile_span', 'delay', 'up3', 'xinfo'))))
        return out

    def last_kernel(self) -> str:
        """'tick' (streaming), 'tile' (time-tiled over records), 'direct' (direct row path) or 'tile_ensemble' (time-tiled, members
        batched: rapid_route_ensemble*, rapid_route_members*): what the last call ran."""
        return ('tick', 'tile', 'direct', 'tile_ensemble')[int(_lib.lib().rr_plan_last_kernel(self._h))]

    # -- device-pointer routing (enqueue only) --
    def rapid_route_dev(self, q_t, qlateral, ql_rows, discharge, out_rows, T, num_substeps, stream=None) -> None:
        self.reserve(MODE_RAPID, T, num_substeps)
        check(_lib.lib().rr_rapid_route_dev(self._h, ptr(q_t), ptr(qlateral), int(ql_rows), ptr(discharge),
                                            int(out_rows), int(T), int(num_substeps), stream))

    # -- adjoint of rapid_route_dev (rr.grad) --
    def rapid_adjoint_work_bytes(self, T: int, num_substeps: int = 1) -> int:
        """rr_rapid_adjoint_work_bytes: bytes of work memory rapid_adjoint_dev needs for T rows x num_substeps sub-steps (readies
        the plan for adjoint calls on first use)."""
        out = C.c_int64(0)
        check(_lib.lib().rr_rapid_adjoint_work_bytes(self._h, int(T), int(num_substeps), C.byref(out)))
        return int(out.value)

    def rapid_adjoint_dev(self, q0, lateral, lat_rows, discharge, grad_out, grad_qfinal, grad_lateral, grad_q0, grad_coef, work,
                          work_bytes, T, num_substeps, stream=None) -> None:
        """rr_rapid_adjoint_dev (enqueue only): gradients through one rapid_route_dev call with the coefficients last set; any of
        lateral, grad_out, grad_qfinal and the three outputs may be None."""
        check(_lib.lib().rr_rapid_adjoint_dev(self._h, ptr(q0), ptr(lateral), int(lat_rows), ptr(discharge), ptr(grad_out),
                                              ptr(grad_qfinal), ptr(grad_lateral), ptr(grad_q0), ptr(grad_coef), ptr(work),
                                              int(work_bytes), int(T), int(num_substeps), stream))

    def rapid_adjoint_batch_work_bytes(self, members: int, T: int, num_substeps: int = 1) -> int:
        """rr_rapid_adjoint_batch_work_bytes: bytes of work memory rapid_adjoint_batch_dev needs for `members` series of T rows x
        num_substeps sub-steps (readies the plan for adjoint calls on first use)."""
        out = C.c_int64(0)
        check(_lib.lib().rr_rapid_adjoint_batch_work_bytes(self._h, int(members), int(T), int(num_substeps), C.byref(out)))
        return int(out.value)

    def rapid_adjoint_batch_dev(self, members, q0, q0_pitch, lateral, lat_rows, lat_pitch, discharge, grad_out, out_pitch, grad_qfinal,
                                grad_lateral, grad_q0, grad_coef, work, work_bytes, T, num_substeps, stream=None) -> None:
        """rr_rapid_adjoint_batch_dev (enqueue only): rapid_adjoint_dev for `members` series at once, member m's arrays m pitches
        (in values) behind the first's; grad_qfinal and grad_q0 are [members, n], grad_coef[4, n] is the sum over the members."""
        check(_lib.lib().rr_rapid_adjoint_batch_dev(self._h, int(members), ptr(q0), int(q0_pitch), ptr(lateral), int(lat_rows), int(lat_pitch),
                                                    ptr(discharge), ptr(grad_out), int(out_pitch), ptr(grad_qfinal), ptr(grad_lateral),
                                                    ptr(grad_q0), ptr(grad_coef), ptr(work), int(work_bytes), int(T), int(num_substeps),
                                                    stream))

    def rapid_adjoint_gauges_work_bytes(self, members: int, n_gauges: int, T: int, num_substeps: int = 1, with_grad_lateral: bool = False) -> int:
        """rr_rapid_adjoint_gauges_work_bytes: bytes of work memory rapid_adjoint_gauges_dev needs for `members` series of T rows x
        num_substeps sub-steps with dL/d(discharge) at n_gauges reaches; with_grad_lateral: the call will be given a grad_lateral
        (readies the plan for adjoint calls on first use)."""
        out = C.c_int64(0)
        check(_lib.lib().rr_rapid_adjoint_gauges_work_bytes(self._h, int(members), int(n_gauges), int(T), int(num_substeps),
                                                            int(bool(with_grad_lateral)), C.byref(out)))
        return int(out.value)

    def rapid_adjoint_gauges_dev(self, members, n_gauges, gauges, q0, q0_pitch, lateral, lat_rows, lat_pitch, discharge_g, grad_out_g,
                                 gauge_pitch, grad_qfinal, grad_lateral, grad_q0, grad_coef, work, work_bytes, T, num_substeps,
                                 stream=None) -> None:
        """rr_rapid_adjoint_gauges_dev (enqueue only): rapid_adjoint_batch_dev with the discharge and its gradient given as
        [members, T, n_gauges] at the reaches gauges[n_gauges] (device int32, params order, distinct; not range-checked)."""
        check(_lib.lib().rr_rapid_adjoint_gauges_dev(self._h, int(members), int(n_gauges), ptr(gauges), ptr(q0), int(q0_pitch), ptr(lateral),
                                                     int(lat_rows), int(lat_pitch), ptr(discharge_g), ptr(grad_out_g), int(gauge_pitch),
                                                     ptr(grad_qfinal), ptr(grad_lateral), ptr(grad_q0), ptr(grad_coef), ptr(work),
                                                     int(work_bytes), int(T), int(num_substeps), stream))

    # -- adjoint of unit_route_dev (rr.grad) --
    def unit_adjoint_work_bytes(self, T: int, num_substeps: int = 1) -> int:
        """rr_unit_adjoint_work_bytes: bytes of work memory unit_adjoint_dev needs for T rows x num_substeps sub-steps (readies
        the plan for adjoint calls on first use)."""
        out = C.c_int64(0)
        check(_lib.lib().rr_unit_adjoint_work_bytes(self._h, int(T), int(num_substeps), C.byref(out)))
        return int(out.value)

    def unit_adjoint_dev(self, q_ch0, q_full0, lateral, lat_rows, discharge, grad_out, grad_qch_final, grad_qfull_final, grad_lateral,
                         grad_qch0, grad_qfull0, grad_coef, work, work_bytes, T, num_substeps, stream=None) -> None:
        """rr_unit_adjoint_dev (enqueue only): gradients through one unit_route_dev call with the coefficients last set; any of the
        three incoming gradients and the four outputs may be None."""
        check(_lib.lib().rr_unit_adjoint_dev(self._h, ptr(q_ch0), ptr(q_full0), ptr(lateral), int(lat_rows), ptr(discharge), ptr(grad_out),
                                             ptr(grad_qch_final), ptr(grad_qfull_final), ptr(grad_lateral), ptr(grad_qch0), ptr(grad_qfull0),
                                             ptr(grad_coef), ptr(work), int(work_bytes), int(T), int(num_substeps), stream))

    def unit_adjoint_batch_work_bytes(self, members: int, T: int, num_substeps: int = 1) -> int:
        """rr_unit_adjoint_batch_work_bytes: bytes of work memory unit_adjoint_batch_dev needs for `members` series of T rows x
        num_substeps sub-steps (readies the plan for adjoint calls on first use)."""
        out = C.c_int64(0)
        check(_lib.lib().rr_unit_adjoint_batch_work_bytes(self._h, int(members), int(T), int(num_substeps), C.byref(out)))
        return int(out.value)

    def unit_adjoint_batch_dev(self, members, q_ch0, q_full0, state_pitch, lateral, lat_rows, lat_pitch, discharge, grad_out, out_pitch,
                               grad_qch_final, grad_qfull_final, grad_lateral, grad_qch0, grad_qfull0, grad_coef, work, work_bytes, T,
                               num_substeps, stream=None) -> None:
        """rr_unit_adjoint_batch_dev (enqueue only): unit_adjoint_dev for `members` series at once, member m's arrays m pitches (in
        values) behind the first's; the final-state gradients and grad_qch0 / grad_qfull0 are [members, n_inner], grad_coef[3, n] is
        the sum over the members."""
        check(_lib.lib().rr_unit_adjoint_batch_dev(self._h, int(members), ptr(q_ch0), ptr(q_full0), int(state_pitch), ptr(lateral),
                                                   int(lat_rows), int(lat_pitch), ptr(discharge), ptr(grad_out), int(out_pitch),
                                                   ptr(grad_qch_final), ptr(grad_qfull_final), ptr(grad_lateral), ptr(grad_qch0),
                                                   ptr(grad_qfull0), ptr(grad_coef), ptr(work), int(work_bytes), int(T), int(num_substeps),
                                                   stream))

    def unit_adjoint_gauges_work_bytes(self, members: int, n_gauges: int, T: int, num_substeps: int = 1, with_grad_lateral: bool = False) -> int:
        """rr_unit_adjoint_gauges_work_bytes: bytes of work memory unit_adjoint_gauges_dev needs for `members` series of T rows x
        num_substeps sub-steps with dL/d(discharge) at n_gauges reaches; with_grad_lateral: the call will be given a grad_lateral
        (readies the plan for adjoint calls on first use)."""
        out = C.c_int64(0)
        check(_lib.lib().rr_unit_adjoint_gauges_work_bytes(self._h, int(members), int(n_gauges), int(T), int(num_substeps),
                                                           int(bool(with_grad_lateral)), C.byref(out)))
        return int(out.value)

    def unit_adjoint_gauges_dev(self, members, n_gauges, gauges, q_ch0, q_full0, state_pitch, lateral, lat_rows, lat_pitch, discharge_g,
                                grad_out_g, gauge_pitch, grad_qch_final, grad_qfull_final, grad_lateral, grad_qch0, grad_qfull0, grad_coef,
                                work, work_bytes, T, num_substeps, stream=None) -> None:
        """rr_unit_adjoint_gauges_dev (enqueue only): unit_adjoint_batch_dev with the discharge and its gradient given as
        [members, T, n_gauges] at the reaches gauges[n_gauges] (device int32, params order, distinct; not range-checked)."""
        check(_lib.lib().rr_unit_adjoint_gauges_dev(self._h, int(members), int(n_gauges), ptr(gauges), ptr(q_ch0), ptr(q_full0),
                                                    int(state_pitch), ptr(lateral), int(lat_rows), int(lat_pitch), ptr(discharge_g),
                                                    ptr(grad_out_g), int(gauge_pitch), ptr(grad_qch_final), ptr(grad_qfull_final),
                                                    ptr(grad_lateral), ptr(grad_qch0), ptr(grad_qfull0), ptr(grad_coef), ptr(work),
                                                    int(work_bytes), int(T), int(num_substeps), stream))

    def muskingum_route_dev(self, q_t, discharge, out_rows, num_output_steps, num_routing_per_output,
                            stream=None) -> None:
        self.reserve(MODE_MUSKINGUM, num_output_steps, num_routing_per_output)
        check(_lib.lib().rr_muskingum_route_dev(self._h, ptr(q_t), ptr(discharge), int(out_rows),
                                                int(num_output_steps), int(num_routing_per_output), stream))

    def unit_route_dev(self, q_ch, q_full, convolved, conv_rows, discharge, out_rows, T, num_substeps,
                       stream=None) -> None:
        self.reserve(MODE_UNIT, T, num_substeps)
        check(_lib.lib().rr_unit_route_dev(self._h, ptr(q_ch), ptr(q_full), ptr(convolved), int(conv_rows),
                                           ptr(discharge), int(out_rows), int(T), int(num_substeps), stream))


    # -- device-pointer routing with the routers' post-processing fused in: float32 rows, `factor` routed rows averaged --
    def rapid_route_f32_dev(self, q_t, qlateral, ql_rows, discharge32, T, num_substeps, factor=1, stream=None) -> None:
        self.reserve(MODE_RAPID, T, num_substeps, f32_out=True)
        check(_lib.lib().rr_rapid_route_f32_dev(self._h, ptr(q_t), ptr(qlateral), int(ql_rows), ptr(discharge32), int(T),
                                                int(num_substeps), int(factor), stream))

    def rapid_route_f32in_dev(self, q_t, qlateral32, ql_rows, T, num_substeps, discharge=None, out_rows=0, discharge32=None, factor=1,
                              stream=None) -> None:
        """rr_rapid_route_f32in_dev: float32 lateral rows in (exact in float64); exactly one of discharge / discharge32."""
        self.reserve(MODE_RAPID, T, num_substeps, f32_out=discharge32 is not None)
        check(_lib.lib().rr_rapid_route_f32in_dev(self._h, ptr(q_t), ptr(qlateral32), int(ql_rows), ptr(discharge), int(out_rows),
                                                  ptr(discharge32), int(factor), int(T), int(num_substeps), stream))

    # -- ensembles: members over the same period routed together on the time-tiled kernel (include/rr_hip.h) --
    def reserve_ensemble(self, members: int, T: int, num_substeps: int = 1, f32_in: bool = False, f32_out: bool = False) -> dict:
        """rr_plan_reserve_ensemble: work memory of rapid_route_ensemble_dev calls of up to `members` members; members_max is the largest
        group whose record rings fit the card at this shape."""
        info = np.zeros(9, dtype=np.int64)
        check(_lib.lib().rr_plan_reserve_ensemble(self._h, int(members), int(T), int(num_substeps), (16 if f32_in else 0) | (4 if f32_out else 0), ptr(info)))
        return dict(tiled=int(info[0]) == 1, ticks_per_launch=int(info[1]), ring_chunks=int(info[2]), work_bytes=int(info[3]),
                    pipeline_ticks=int(info[6]), ring_bytes=int(info[7]), members_max=int(info[8]))

    def rapid_route_ensemble_dev(self, members, q_t, q_pitch, lateral, lateral_is_f32, lateral_member_pitch, discharge, discharge_is_f32,
                                 discharge_member_pitch, factor, T, num_substeps, stream=None) -> None:
        """rr_rapid_route_ensemble_dev (enqueue only): member m's rows at m * pitch elements, its state at q_t + m * q_pitch."""
        self.reserve_ensemble(members, T, num_substeps, f32_in=bool(lateral_is_f32), f32_out=bool(discharge_is_f32))
        check(_lib.lib().rr_rapid_route_ensemble_dev(self._h, int(members), ptr(q_t), int(q_pitch), ptr(lateral), int(bool(lateral_is_f32)),
                                                     int(lateral_member_pitch), ptr(discharge), int(bool(discharge_is_f32)), int(discharge_member_pitch),
                                                     int(factor), int(T), int(num_substeps), stream))

    def _route_member_groups(self, q_t, qlateral, M, discharge, num_substeps, factor, route_dev, per_group=None, sink=None) -> np.ndarray:
        """The host-array driver behind rapid_route_ensemble and rapid_route_members: M members' rows (M, T, n) -- or one (T, n) forcing that
        all members share, uploaded once and passed with member pitch 0 -- go to the device in groups of the size the reservation reports
        (members_max), each group routed by `route_dev` (rapid_route_ensemble_dev's signature).  `per_group(g0, m)` is called before each
        group with its range, and once before the first reservation with (0, 0): rapid_route_members puts the group's coefficient sets
        on the plan there.  Returns the (M, n) final states.
        Each group's (m, rows, n) discharge block is downloaded into `discharge`; with a `sink` it stays on the device instead: `discharge`
        is then the rows' dtype (float32 or float64), no host array, and `sink(g0, m, d_out)` is called after each group is enqueued, on the
        stream it was enqueued on, with the device buffer that holds its block (reused by the next group)."""
        ql = np.asarray(qlateral)
        if ql.dtype != np.float32:
            ql = np.asarray(ql, dtype=np.float64)
        shared, (T, n) = ql.ndim == 2, ql.shape[-2:]
        q0 = np.array(np.broadcast_to(np.asarray(q_t, dtype=np.float64), (M, n)), order='C')      # (a copy: returned as the final states)
        if sink is not None:
            out_dtype = np.dtype(discharge)
            f32_out = out_dtype == np.float32
            rows = T // int(factor) if f32_out else T
            if out_dtype not in (np.float32, np.float64) or not (f32_out or int(factor) == 1):
                raise ValueError('the rows are float64 (factor 1) or float32 (each the mean of `factor` routed rows)')
        else:
            f32_out = isinstance(discharge, np.ndarray) and discharge.dtype == np.float32
            rows = T // int(factor) if f32_out else T
            if not (isinstance(discharge, np.ndarray) and discharge.dtype in (np.float32, np.float64) and discharge.flags['C_CONTIGUOUS']
                    and discharge.flags['WRITEABLE'] and discharge.shape == (M, rows, n) and (f32_out or int(factor) == 1)):
                raise ValueError(f'discharge must be a writeable C-contiguous float64 ({M}, {T}, {n}) array, or float32 ({M}, T / factor, {n})')
            out_dtype = discharge.dtype
        f32_in = ql.dtype == np.float32
        nsub = int(num_substeps)
        if M == 0 or T == 0 or n == 0:
            return q0
        if per_group:
            per_group(0, 0)
        group = min(M, self.reserve_ensemble(1, T, nsub, f32_in, f32_out)['members_max'])
        if group < 1:
            raise RRError(_lib.RR_E_UNSUPPORTED, 'the record ring of one member does not fit the card at this shape')
        # members_max budgets the record rings only: the group's rows must fit beside them, so a group the device refuses is halved
        lat_each, out_each = T * n * ql.itemsize, rows * n * out_dtype.itemsize
        while True:
            bufs = []
            try:
                for b in (lat_each * (1 if shared else group), out_each * group, n * 8 * group):
                    bufs.append(DeviceBuffer(b, self.device))
                self.reserve_ensemble(group, T, nsub, f32_in, f32_out)
                break
            except RRError as e:
                for b in bufs:
                    b.free()
                if e.code != _lib.RR_E_ALLOC or group == 1:
                    raise
                group = (group + 1) // 2
        d_ql, d_out, d_q = bufs
        try:
            if shared:
                d_ql.upload(np.ascontiguousarray(ql))
            for g0 in range(0, M, group):
                m = min(group, M - g0)
                if per_group:
                    per_group(g0, m)
                if not shared:
                    d_ql.upload(np.ascontiguousarray(ql[g0:g0 + m]))
                d_q.upload(q0[g0:g0 + m])
                route_dev(m, d_q, n, d_ql, f32_in, 0 if shared else T * n, d_out, f32_out, rows * n, int(factor), T, nsub)
                if sink is not None:
                    sink(g0, m, d_out)
                else:
                    discharge[g0:g0 + m] = d_out.download(discharge.dtype, (m, rows, n))
                q0[g0:g0 + m] = d_q.download(np.float64, (m, n))
        finally:
            for b in (d_ql, d_out, d_q):
                b.free()
        return q0

    def rapid_route_ensemble(self, q_t, qlateral, discharge, num_substeps: int, factor: int = 1) -> np.ndarray:
        """Host arrays: qlateral (M, T, n) float64 or float32; q_t (n,) -- every member starts there -- or (M, n); discharge (M, T, n)
        float64, or (M, T / factor, n) float32 (each row the mean of `factor` routed rows).  Returns the (M, n) final states.  The members
        go to the device in groups of the size the reservation reports (members_max)."""
        ql = np.asarray(qlateral)
        if ql.ndim != 3 or ql.shape[2] != self.n:
            raise ValueError(f'qlateral must have shape (M, T, {self.n})')
        return self._route_member_groups(q_t, ql, ql.shape[0], discharge, num_substeps, factor, self.rapid_route_ensemble_dev)

    # -- parameter ensembles: the members of an ensemble call with a coefficient set each (include/rr_hip.h) --
    def _member_arrays(self, lhs_off_data, c2, c3, c4_dt):
        arrays = [_f64(a, nm) for a, nm in ((lhs_off_data, 'lhs_off_data'), (c2, 'c2'), (c3, 'c3'), (c4_dt, 'c4_dt'))]
        if any(a.ndim != 2 for a in arrays):
            raise ValueError('member coefficients are 2-D: lhs_off_data (M, n_edges), c2 / c3 / c4_dt (M, n)')
        M = arrays[1].shape[0]
        if M < 1 or arrays[0].shape != (M, self.n_edges) or any(a.shape != (M, self.n) for a in arrays[1:]):
            raise ValueError(f'member coefficients must be lhs_off_data (M, {self.n_edges}) and c2, c3, c4_dt (M, {self.n}) with one M >= 1; got '
                             + ', '.join(str(a.shape) for a in arrays))
        return arrays

    def _upload_member_coeffs(self, g0: int, m: int) -> None:
        lhs, c2, c3, c4 = (a[g0:g0 + m] for a in self._member_sets)      # (row slices of C-contiguous arrays: contiguous)
        self._member_on_device = None
        check(_lib.lib().rr_plan_set_member_coeffs(self._h, m, ptr(lhs) if lhs.size else None, self.n_edges, ptr(c2), ptr(c3), ptr(c4), self.n))
        self._member_on_device = (g0, m)

    def set_member_coeffs(self, lhs_off_data, c2, c3, c4_dt) -> None:
        """rr_plan_set_member_coeffs: M coefficient sets for rapid_route_members*, lhs_off_data (M, n_edges), c2 / c3 / c4_dt (M, n); anything
        array-like is made C-contiguous float64.  The plan's own coefficients (set_coeffs) are not touched.  The arrays are kept on the plan
        (before the library sees them: where it refuses them, rapid_route_members meets the same refusal): rapid_route_members sets slices
        of them again when it has to route in groups."""
        self._member_sets = self._member_arrays(lhs_off_data, c2, c3, c4_dt)
        self._upload_member_coeffs(0, self._member_sets[1].shape[0])

    def rapid_route_members_dev(self, members, q_t, q_pitch, lateral, lateral_is_f32, lateral_member_pitch, discharge, discharge_is_f32,
                                discharge_member_pitch, factor, T, num_substeps, stream=None) -> None:
        """rr_rapid_route_members_dev (enqueue only): rapid_route_ensemble_dev with member m routed by coefficient set m of the sets on the
        device; lateral_member_pitch 0: one forcing for all members."""
        self.reserve_ensemble(members, T, num_substeps, f32_in=bool(lateral_is_f32), f32_out=bool(discharge_is_f32))
        check(_lib.lib().rr_rapid_route_members_dev(self._h, int(members), ptr(q_t), int(q_pitch), ptr(lateral), int(bool(lateral_is_f32)),
                                                    int(lateral_member_pitch), ptr(discharge), int(bool(discharge_is_f32)), int(discharge_member_pitch),
                                                    int(factor), int(T), int(num_substeps), stream))

    def rapid_route_members(self, q_t, qlateral, discharge, num_substeps: int, factor: int = 1) -> np.ndarray:
        """Host arrays, M = the number of sets last given to set_member_coeffs: qlateral (T, n) -- one forcing, uploaded once and shared by
        all members -- or (M, T, n), float64 or float32; q_t (n,) or (M, n); discharge (M, T, n) float64, or (M, T / factor, n) float32 (each
        row the mean of `factor` routed rows).  Returns the (M, n) final states.  Where the reservation (members_max) or the device's memory
        does not take all members at once they are routed in groups, each group's coefficient sets set again from the arrays the plan keeps."""
        ql, M, q_in, sets_on_plan = self._members_inputs(q_t, qlateral, factor)
        return self._route_member_groups(q_in, ql, M, discharge, num_substeps, factor, self.rapid_route_members_dev, sets_on_plan)

    def _members_inputs(self, q_t, qlateral, factor):
        """The checks rapid_route_members and rapid_route_members_scores share, before any device work: (qlateral as an array, M, q_t as
        float64, the per-group hook that keeps the group's coefficient sets on the plan)."""
        ql = np.asarray(qlateral)
        if ql.ndim not in (2, 3) or ql.shape[-1] != self.n:
            raise ValueError(f'qlateral must have shape (T, {self.n}) or (M, T, {self.n})')
        sets = getattr(self, '_member_sets', None)
        if sets is None:
            raise RRError(_lib.RR_E_STATE, 'rapid_route_members before set_member_coeffs')
        M, n = sets[1].shape[0], self.n
        if ql.ndim == 3 and ql.shape[0] != M:
            raise ValueError(f'qlateral has {ql.shape[0]} members, set_member_coeffs was given {M} sets')
        q_in = np.asarray(q_t, dtype=np.float64)
        if q_in.shape not in ((n,), (M, n)):
            raise ValueError(f'q_t must have shape ({n},) or ({M}, {n})')
        if int(factor) < 1:
            raise ValueError('factor must be >= 1')

        def sets_on_plan(g0, m):
            on = getattr(self, '_member_on_device', None)
            if m == 0:      # no group yet: reserve_ensemble wants coefficients on the plan, whichever
                if on is None:
                    self._upload_member_coeffs(0, M)
            elif on != (g0, m) and not (g0 == 0 and on == (0, M)):
                self._upload_member_coeffs(g0, m)
        return ql, M, q_in, sets_on_plan

    def rapid_route_members_scores(self, q_t, qlateral, observed, gauges, num_substeps: int, factor: int = 1, skip_missing: bool = False,
                                   skip_rows: int = 0, dtype=np.float32):
        """Route the M members of set_member_coeffs as rapid_route_members does and score each at its gauges without the discharge
        leaving the device: returns (scores, q_final), scores {'me', 'mae', 'mse', 'pearson_r', 'kge2012'[, 'count']} -> (M, G) float64
        (rr.metrics.scores_members' keys) and q_final the (M, n) final states.  q_t and qlateral are rapid_route_members'.  The scored
        rows are the rows rapid_route_members would write: dtype float32 -- (M, T // factor, n), each the mean of `factor` routed rows
        -- or float64 -- (M, T, n), factor 1.  observed: (rows, G) float32 or float64, uploaded once; gauges: (G,) reach indices in
        params order, repeats allowed; skip_missing: a NaN in `observed` is a gap (rr.metrics.scores); skip_rows: the first output rows
        (spin-up) are left out of the scores.  Each group's (m, rows, n) block is scored by an rr.metrics.MemberAccumulator on the
        stream it was routed on; only the scores and the final states come back.  Member m's scores are the bits of
        rr.metrics.scores(observed[skip_rows:], out[m][skip_rows:], columns=gauges) on rapid_route_members' rows wherever
        m_group x ceil(G / 256) x ceil(rows / 32) <= 2048."""
        from . import metrics
        ql, M, q_in, sets_on_plan = self._members_inputs(q_t, qlateral, factor)
        T, n = ql.shape[-2:]
        out_dtype = np.dtype(dtype)
        if out_dtype not in (np.float32, np.float64):
            raise ValueError('dtype must be float32 or float64')
        if out_dtype == np.float64 and int(factor) != 1:
            raise ValueError('float64 rows are never averaged: factor must be 1 (or pass dtype=float32)')
        rows, skip = (T // int(factor) if out_dtype == np.float32 else T), int(skip_rows)
        cols = np.asarray(gauges)
        if cols.ndim != 1 or cols.size < 1 or not np.issubdtype(cols.dtype, np.integer):
            raise ValueError('gauges must be a 1-D integer array of at least one reach index')
        if cols.min() < 0 or cols.max() >= n:
            raise ValueError(f'gauges holds a reach index outside 0 .. {n - 1}')
        G = cols.shape[0]
        obs = np.asarray(observed)
        if obs.dtype not in (np.float32, np.float64):
            obs = obs.astype(np.float64)
        if obs.shape != (rows, G):
            raise ValueError(f'observed must have shape ({rows}, {G}): one row per output row, one column per gauge; got {obs.shape}')
        if not 0 <= skip < rows:
            raise ValueError(f'skip_rows must leave at least one of the {rows} rows (0 <= skip_rows < rows)')
        obs = np.ascontiguousarray(obs)
        keys = metrics.SCORES + (('count',) if skip_missing else ())
        scores = {k: np.empty((M, G)) for k in keys}
        d_obs = []

        def score_group(g0, m, d_out):
            if not d_obs:
                d_obs.append(DeviceBuffer(obs.nbytes, self.device).upload(obs))
            acc = metrics.MemberAccumulator(G, m, columns=cols, device=self.device, skip_missing=skip_missing)
            acc._enter_stream(None)
            acc._launch(rows - skip, d_obs[0].address + skip * G * obs.itemsize, obs.dtype == np.float32, G, 0,
                        d_out.address + skip * n * out_dtype.itemsize, out_dtype == np.float32, n, rows * n, None)
            for k, v in acc.result().items():
                scores[k][g0:g0 + m] = v
        try:
            q_final = self._route_member_groups(q_in, ql, M, out_dtype, num_substeps, factor, self.rapid_route_members_dev, sets_on_plan,
                                                sink=score_group)
        finally:
            for b in d_obs:
                b.free()
        return scores, q_final

    def muskingum_route_f32_dev(self, q_t, discharge32, num_output_steps, num_routing_per_output, stream=None) -> None:
        self.reserve(MODE_MUSKINGUM, num_output_steps, num_routing_per_output, f32_out=True)
        check(_lib.lib().rr_muskingum_route_f32_dev(self._h, ptr(q_t), ptr(discharge32), int(num_output_steps),
                                                    int(num_routing_per_output), stream))

    def unit_route_f32_dev(self, q_ch, q_full, convolved, conv_rows, discharge32, T, num_substeps, factor=1, stream=None) -> None:
        self.reserve(MODE_UNIT, T, num_substeps, f32_out=True)
        check(_lib.lib().rr_unit_route_f32_dev(self._h, ptr(q_ch), ptr(q_full), ptr(convolved), int(conv_rows),
                                               ptr(discharge32), int(T), int(num_substeps), int(factor), stream))

    def rapid_route_runoff_dev(self, q_t, n_points, indptr, indices, weights, runoff, runoff_is_f32, stride_t, stride_p, area, flags, T,
                               discharge=None, discharge32=None, factor=1, stream=None) -> None:
        """Gridded runoff -> records -> routing in one call (rr_rapid_route_runoff_dev); exactly one of discharge / discharge32."""
        self.reserve(MODE_RAPID, T, 1, plain_rows=False)
        check(_lib.lib().rr_rapid_route_runoff_dev(self._h, ptr(q_t), int(n_points), ptr(indptr), ptr(indices), ptr(weights), ptr(runoff),
                                                   int(bool(runoff_is_f32)), int(stride_t), int(stride_p), ptr(area), int(flags),
                                                   ptr(discharge), ptr(discharge32), int(factor), int(T), stream))

    def unit_route_uh_dev(self, q_ch, q_full, q_final, uh_kernel, uh_state, n_ks, depth, T, num_substeps, discharge=None,
                          discharge32=None, factor=1, stream=None) -> None:
        """Convolution + routing of one file in one call (rr_unit_route_uh_dev); exactly one of discharge / discharge32."""
        self.reserve(MODE_UNIT, T, num_substeps, f32_out=discharge32 is not None, uh=True)
        check(_lib.lib().rr_unit_route_uh_dev(self._h, ptr(q_ch), ptr(q_full), ptr(q_final), ptr(uh_kernel), ptr(uh_state),
                                              int(n_ks), ptr(depth), ptr(discharge), ptr(discharge32), int(factor), int(T),
                                              int(num_substeps), stream))

    def unit_route_uh_f32in_dev(self, q_ch, q_full, q_final, uh_kernel, uh_state, n_ks, depth32, T, num_substeps, discharge=None,
                                discharge32=None, factor=1, stream=None) -> None:
        """rr_unit_route_uh_f32in_dev: the same from float32 runoff depths (as runoff files store them)."""
        self.reserve(MODE_UNIT, T, num_substeps, f32_out=discharge32 is not None, uh=True)
        check(_lib.lib().rr_unit_route_uh_f32in_dev(self._h, ptr(q_ch), ptr(q_full), ptr(q_final), ptr(uh_kernel), ptr(uh_state),
                                                    int(n_ks), ptr(depth32), ptr(discharge), ptr(discharge32), int(factor), int(T),
                                                    int(num_substeps), stream))

    # -- partitioned networks: boundary reaches + streaming calls (include/rr_hip.h) --
    def set_boundary(self, ghost_reaches, export_reaches) -> None:
        g = np.ascontiguousarray(ghost_reaches, dtype=np.int64)
        e = np.ascontiguousarray(export_reaches, dtype=np.int64)
        check(_lib.lib().rr_plan_set_boundary(self._h, g.size, ptr(g) if g.size else None, e.size,
                                              ptr(e) if e.size else None))
        self.n_ghost, self.n_export = int(g.size), int(e.size)

    def stream_begin(self, q_t, lateral, lat_rows, discharge, out_rows, T, num_substeps, ghost_series=None,
                     export_series=None, stream=None) -> None:
        # rings shorter than 32 rows keep to records (include/rr_hip.h, rr_stream_begin): reserve for the schedule the call will get
        plain = (lateral is None or min(int(lat_rows), int(T)) >= min(32, int(T))) and min(int(out_rows), int(T)) >= min(32, int(T))
        self.reserve(MODE_MUSKINGUM if lateral is None else MODE_RAPID, T, num_substeps, plain_rows=plain)
        check(_lib.lib().rr_stream_begin(self._h, 0 if lateral is None else 1, ptr(q_t), ptr(lateral), int(lat_rows),
                                         ptr(discharge), int(out_rows), int(T), int(num_substeps), ptr(ghost_series),
                                         ptr(export_series), stream))

    def stream_advance(self, lateral_rows_ready: int, ghost_substeps_ready: int) -> int:
        ready = C.c_int64(0)
        check(_lib.lib().rr_stream_advance(self._h, int(lateral_rows_ready), int(ghost_substeps_ready), C.byref(ready)))
        return int(ready.value)

    def stream_end(self, q_t=None) -> None:
        check(_lib.lib().rr_stream_end(self._h, ptr(q_t)))

    def stream_begin_unit(self, q_ch, q_full, lateral, lat_rows, discharge, out_rows, T, num_substeps, ghost_series=None,
                          export_series=None, stream=None) -> None:
        self.reserve(MODE_UNIT, T, num_substeps, plain_rows=False)
        check(_lib.lib().rr_stream_begin_unit(self._h, ptr(q_ch), ptr(q_full), ptr(lateral), int(lat_rows), ptr(discharge),
                                              int(out_rows), int(T), int(num_substeps), ptr(ghost_series), ptr(export_series), stream))

    def stream_end_unit(self, q_ch=None, q_full=None) -> None:
        check(_lib.lib().rr_stream_end_unit(self._h, ptr(q_ch), ptr(q_full)))


def partition_forest(csc_indptr, csc_indices, n_parts: int):
    """(part_of int32[n], part_sizes int64[n_parts]) -- rr_partition_forest; host-only."""
    indptr = np.ascontiguousarray(csc_indptr, dtype=np.int32)
    indices = np.ascontiguousarray(csc_indices, dtype=np.int32)
    n = indptr.shape[0] - 1
    part_of = np.empty(n, dtype=np.int32)
    sizes = np.zeros(n_parts, dtype=np.int64)
    check(_lib.lib().rr_partition_forest(n, ptr(indptr), ptr(indices) if indices.size else None, int(n_parts),
                                         ptr(part_of), ptr(sizes)))
    return part_of, sizes


def uh_convolve(kernel, state, lateral, device: int = 0) -> np.ndarray:
    """UnitHydrograph.convolve (river_route/uhkernels/UnitHydrograph.py:77-107) on the GPU.
    kernel (n_ks, n); state (n_ks, n) updated in place; lateral (T, n) -> (T, n)."""
    k = np.ascontiguousarray(kernel, dtype=np.float64)
    lat = np.ascontiguousarray(lateral, dtype=np.float64)
    n_ks, n = k.shape
    _inplace_f64(state, 'state', (n_ks, n))
    if lat.ndim != 2 or lat.shape[1] != n:
        raise ValueError(f'lateral must have shape (T, {n})')
    out = np.empty_like(lat)
    check(_lib.lib().rr_uh_convolve(int(device), ptr(k), ptr(state), ptr(lat), ptr(out), lat.shape[0], n_ks, n))
    return out


def uh_convolve_dev(kernel, state, lateral, out, T, n_ks, n, device: int = 0, stream=None) -> None:
    check(_lib.lib().rr_uh_convolve_dev(int(device), ptr(kernel), ptr(state), ptr(lateral), ptr(out), int(T),
                                        int(n_ks), int(n), stream))


def uh_adjoint_work_bytes(T, n_ks, n) -> int:
    """rr_uh_adjoint_work_bytes: bytes of work memory uh_adjoint_dev needs for its kernel gradient (0: none)."""
    out = C.c_int64(0)
    check(_lib.lib().rr_uh_adjoint_work_bytes(int(T), int(n_ks), int(n), C.byref(out)))
    return int(out.value)


def uh_adjoint_dev(kernel, depth, grad_convolved, grad_state_out, grad_depth, grad_kernel, grad_state, work, work_bytes, T, n_ks, n,
                   device: int = 0, stream=None) -> None:
    """rr_uh_adjoint_dev (enqueue only): gradients through one uh_convolve_dev call; either incoming gradient and any output may be
    None."""
    check(_lib.lib().rr_uh_adjoint_dev(int(device), ptr(kernel), ptr(depth), ptr(grad_convolved), ptr(grad_state_out), ptr(grad_depth),
                                       ptr(grad_kernel), ptr(grad_state), ptr(work), int(work_bytes), int(T), int(n_ks), int(n), stream))


RUNOFF_CUMULATIVE, RUNOFF_FORCE_POSITIVE, RUNOFF_KEEP_NAN = 1, 2, 4


def runoff_to_qlateral(indptr, indices, weights, runoff_tp, area=None, flags: int = 0, device: int = 0) -> np.ndarray:
    """rr_runoff_to_qlateral: (T, n_rivers) float64 from a CSR weight matrix (n_rivers x n_points, float64 data,
    int32 structure) and a (T, n_points) float32/float64 runoff block (river_route/runoff.py:288-330).  The block is
    handed over point-major so every gathered grid point is one contiguous run of time steps."""
    indptr = np.ascontiguousarray(indptr, dtype=np.int32)
    indices = np.ascontiguousarray(indices, dtype=np.int32)
    weights = np.ascontiguousarray(weights, dtype=np.float64)
    runoff_tp = np.asarray(runoff_tp)
    if runoff_tp.ndim != 2:
        raise ValueError('runoff must be (time, points)')
    if runoff_tp.dtype not in (np.float32, np.float64):
        runoff_tp = runoff_tp.astype(np.float64)
    T, n_points = runoff_tp.shape
    n_rivers = indptr.shape[0] - 1
    if indices.shape[0] and (indices.min() < 0 or indices.max() >= n_points):
        raise ValueError('weight matrix refers to grid points outside the runoff block')
    t_pad = -(-T // 16) * 16                                  # rows padded to whole 16-step chunks: vector gathers
    point_major = np.zeros((n_points, t_pad), dtype=runoff_tp.dtype)
    point_major[:, :T] = runoff_tp.T                          # (n_points, t_pad): stride_t = 1, stride_p = t_pad
    out = np.empty((T, n_rivers), dtype=np.float64)
    if area is not None:
        area = np.ascontiguousarray(area, dtype=np.float64)
        if area.shape != (n_rivers,):
            raise ValueError('area must have one value per river')
    check(_lib.lib().rr_runoff_to_qlateral(int(device), n_rivers, n_points, T, ptr(indptr), ptr(indices), ptr(weights),
                                           ptr(point_major), int(point_major.dtype == np.float32), 1, t_pad,
                                           ptr(area) if area is not None else None, int(flags), ptr(out)))
    return out


def runoff_to_qlateral_dev(n_rivers, n_points, T, indptr, indices, weights, runoff, runoff_is_f32, stride_t, stride_p, area, flags, out,
                           device: int = 0, stream=None) -> None:
    """rr_runoff_to_qlateral_dev: device arrays in, (T, n_rivers) float64 device rows out; only enqueues."""
    check(_lib.lib().rr_runoff_to_qlateral_dev(int(device), int(n_rivers), int(n_points), int(T), ptr(indptr), ptr(indices), ptr(weights),
                                               ptr(runoff), int(bool(runoff_is_f32)), int(stride_t), int(stride_p),
                                               ptr(area) if area is not None else None, int(flags), ptr(out), stream))


def runoff_adjoint_work_bytes(n_rivers: int, n_points: int, T: int) -> int:
    """rr_runoff_adjoint_work_bytes: device work memory one rr_runoff_adjoint_dev of T rows needs (Gs, river-major)."""
    out = C.c_int64(0)
    check(_lib.lib().rr_runoff_adjoint_work_bytes(int(n_rivers), int(n_points), int(T), C.byref(out)))
    return int(out.value)


def runoff_adjoint_dev(n_rivers, n_points, T, indptr, indices, weights, t_indptr, t_pairs, runoff, runoff_is_f32, stride_t, stride_p, area,
                       flags, grad_qlateral, grad_runoff, grad_stride_t, grad_weights, work, work_bytes, device: int = 0, stream=None) -> None:
    """rr_runoff_adjoint_dev: dL/drunoff (the runoff's type, (T, n_points) rows grad_stride_t elements apart) and dL/dweights from
    dL/dqlateral of one runoff_to_qlateral_dev call; either output may be None; only enqueues."""
    check(_lib.lib().rr_runoff_adjoint_dev(int(device), int(n_rivers), int(n_points), int(T), ptr(indptr), ptr(indices), ptr(weights),
                                           ptr(t_indptr), ptr(t_pairs), ptr(runoff), int(bool(runoff_is_f32)), int(stride_t), int(stride_p),
                                           ptr(area), int(flags), ptr(grad_qlateral), ptr(grad_runoff), int(grad_stride_t),
                                           ptr(grad_weights), ptr(work), int(work_bytes), stream))


def resample_cast_dev(discharge, num_rows, n, factor, out, device: int = 0, stream=None) -> None:
    """Device-side mean over `factor` rows + float32 cast (rr_resample_cast_dev)."""
    check(_lib.lib().rr_resample_cast_dev(int(device), ptr(discharge), int(num_rows), int(n), int(factor), ptr(out), stream))


METRICS_STATE, METRICS_SCORES = 9, 5      # include/rr_hip.h: RR_METRICS_STATE, RR_METRICS_SCORES


def metrics_work_bytes(n: int, rows: int) -> int:
    """rr_metrics_work_bytes: device work memory one rr_metrics_update_dev of `rows` rows of n columns needs."""
    out = C.c_int64(0)
    check(_lib.lib().rr_metrics_work_bytes(int(n), int(rows), C.byref(out)))
    return int(out.value)


def metrics_update_dev(n, rows, y_true, true_is_f32, true_pitch, y_pred, pred_is_f32, pred_pitch, pred_columns, state, work,
                       work_bytes, device: int = 0, stream=None) -> None:
    """rr_metrics_update_dev: merge `rows` device rows into the [9][n] float64 score state; only enqueues."""
    check(_lib.lib().rr_metrics_update_dev(int(device), int(n), int(rows), ptr(y_true), int(bool(true_is_f32)), int(true_pitch),
                                           ptr(y_pred), int(bool(pred_is_f32)), int(pred_pitch), ptr(pred_columns), ptr(state),
                                           ptr(work), int(work_bytes), stream))


def metrics_finish_dev(n, state, out, device: int = 0, stream=None) -> None:
    """rr_metrics_finish_dev: [9][n] state -> out[5][n] (me, mae, mse, pearson_r, kge2012); only enqueues."""
    check(_lib.lib().rr_metrics_finish_dev(int(device), int(n), ptr(state), ptr(out), stream))


def metrics_adjoint_work_bytes(n: int) -> int:
    """rr_metrics_adjoint_work_bytes: device work memory one rr_metrics_adjoint_dev over n scored columns needs."""
    out = C.c_int64(0)
    check(_lib.lib().rr_metrics_adjoint_work_bytes(int(n), C.byref(out)))
    return int(out.value)


def metrics_adjoint_dev(n, rows, y_true, true_is_f32, true_pitch, y_pred, pred_is_f32, pred_pitch, state, grad_scores, n_distinct, order,
                        distinct_columns, segments, grad_pred, grad_pitch, work, work_bytes, device: int = 0, stream=None) -> None:
    """rr_metrics_adjoint_dev: dL/dy_pred from the [9][n] score state and dL/d(scores)[5][n]; only enqueues.  order, distinct_columns
    and segments are the sorted column map (all None: column j against column j)."""
    check(_lib.lib().rr_metrics_adjoint_dev(int(device), int(n), int(rows), ptr(y_true), int(bool(true_is_f32)), int(true_pitch), ptr(y_pred),
                                            int(bool(pred_is_f32)), int(pred_pitch), ptr(state), ptr(grad_scores), int(n_distinct),
                                            ptr(order), ptr(distinct_columns), ptr(segments), ptr(grad_pred), int(grad_pitch), ptr(work),
                                            int(work_bytes), stream))


def metrics_update_missing_dev(n, rows, y_true, true_is_f32, true_pitch, y_pred, pred_is_f32, pred_pitch, pred_columns, state, work,
                               work_bytes, device: int = 0, stream=None) -> None:
    """rr_metrics_update_missing_dev: metrics_update_dev that leaves out the pairs whose y_true is NaN; only enqueues."""
    check(_lib.lib().rr_metrics_update_missing_dev(int(device), int(n), int(rows), ptr(y_true), int(bool(true_is_f32)), int(true_pitch),
                                                   ptr(y_pred), int(bool(pred_is_f32)), int(pred_pitch), ptr(pred_columns), ptr(state),
                                                   ptr(work), int(work_bytes), stream))


def metrics_members_work_bytes(n: int, members: int, rows: int) -> int:
    """rr_metrics_members_work_bytes: device work memory one rr_metrics_update_members_dev of `rows` rows of `members` x n columns needs."""
    out = C.c_int64(0)
    check(_lib.lib().rr_metrics_members_work_bytes(int(n), int(members), int(rows), C.byref(out)))
    return int(out.value)


def metrics_update_members_dev(n, members, rows, y_true, true_is_f32, true_pitch, true_member_pitch, y_pred, pred_is_f32, pred_pitch,
                               pred_member_pitch, pred_columns, skip_missing, state, work, work_bytes, device: int = 0, stream=None) -> None:
    """rr_metrics_update_members_dev: merge `rows` device rows of each of `members` members into the [9][members * n] float64 score state
    (true_member_pitch 0: one observation block for all members); only enqueues."""
    check(_lib.lib().rr_metrics_update_members_dev(int(device), int(n), int(members), int(rows), ptr(y_true), int(bool(true_is_f32)),
                                                   int(true_pitch), int(true_member_pitch), ptr(y_pred), int(bool(pred_is_f32)),
                                                   int(pred_pitch), int(pred_member_pitch), ptr(pred_columns), int(bool(skip_missing)),
                                                   ptr(state), ptr(work), int(work_bytes), stream))


def metrics_adjoint_missing_dev(n, rows, y_true, true_is_f32, true_pitch, y_pred, pred_is_f32, pred_pitch, state, grad_scores, n_distinct,
                                order, distinct_columns, segments, grad_pred, grad_pitch, work, work_bytes, device: int = 0,
                                stream=None) -> None:
    """rr_metrics_adjoint_missing_dev: metrics_adjoint_dev for a state metrics_update_missing_dev left: an element whose y_true is NaN
    gets exactly 0 from that column; only enqueues."""
    check(_lib.lib().rr_metrics_adjoint_missing_dev(int(device), int(n), int(rows), ptr(y_true), int(bool(true_is_f32)), int(true_pitch),
                                                    ptr(y_pred), int(bool(pred_is_f32)), int(pred_pitch), ptr(state), ptr(grad_scores),
                                                    int(n_distinct), ptr(order), ptr(distinct_columns), ptr(segments), ptr(grad_pred),
                                                    int(grad_pitch), ptr(work), int(work_bytes), stream))


def grid_overlap_area(row_rings, ring_offsets, ring_weight, lon, lat, x_bounds, y_bounds, row_cells, pair_offsets,
                      device: int = 0) -> np.ndarray:
    """rr_grid_overlap_area: host arrays in, float64[n_pairs] clipped cea areas (m^2) out, one per (row, candidate cell) pair."""
    row_rings = np.ascontiguousarray(row_rings, dtype=np.int64)
    ring_offsets = np.ascontiguousarray(ring_offsets, dtype=np.int64)
    pair_offsets = np.ascontiguousarray(pair_offsets, dtype=np.int64)
    ring_weight, lon, lat, x_bounds, y_bounds = (np.ascontiguousarray(a, dtype=np.float64) for a in (ring_weight, lon, lat, x_bounds, y_bounds))
    row_cells = np.ascontiguousarray(row_cells, dtype=np.int32)
    n_rows, n_rings = row_rings.shape[0] - 1, ring_offsets.shape[0] - 1
    if pair_offsets.shape[0] != n_rows + 1 or ring_weight.shape[0] != n_rings or lon.shape != lat.shape or row_cells.size != 3 * n_rows:
        raise ValueError('grid_overlap_area: array lengths disagree')
    n_pairs = int(pair_offsets[-1]) if n_rows >= 0 and pair_offsets.size else 0
    out = np.zeros(n_pairs, dtype=np.float64)
    check(_lib.lib().rr_grid_overlap_area(int(device), n_rows, n_rings, lon.shape[0], x_bounds.shape[0] - 1, y_bounds.shape[0] - 1,
                                          n_pairs, ptr(row_rings), ptr(ring_offsets), ptr(ring_weight), ptr(lon), ptr(lat),
                                          ptr(x_bounds), ptr(y_bounds), ptr(row_cells), ptr(pair_offsets), ptr(out)))
    return out


def grid_overlap_area_dev(n_rows, n_rings, n_vertices, nx, ny, n_pairs, row_rings, ring_offsets, ring_weight, lon, lat, x_bounds,
                          y_bounds, row_cells, pair_offsets, area, device: int = 0, stream=None) -> None:
    """rr_grid_overlap_area_dev: the same on device arrays; only enqueues."""
    check(_lib.lib().rr_grid_overlap_area_dev(int(device), int(n_rows), int(n_rings), int(n_vertices), int(nx), int(ny), int(n_pairs),
                                              ptr(row_rings), ptr(ring_offsets), ptr(ring_weight), ptr(lon), ptr(lat), ptr(x_bounds),
                                              ptr(y_bounds), ptr(row_cells), ptr(pair_offsets), ptr(area), stream))


class DeviceBuffer:
    """A raw hipMalloc'd buffer for callers that do not use torch."""

    def __init__(self, nbytes: int, device: int = 0):
        self.device, self.nbytes = int(device), int(nbytes)
        p = C.c_void_p()
        check(_lib.lib().rr_dev_malloc(self.device, self.nbytes, C.byref(p)))
        self.address = int(p.value or 0)

    def upload(self, array: np.ndarray, offset: int = 0) -> 'DeviceBuffer':
        a = np.ascontiguousarray(array)
        check(_lib.lib().rr_dev_upload(self.device, self.address + offset, ptr(a), a.nbytes))
        return self

    def download(self, dtype, shape, offset: int = 0) -> np.ndarray:
        out = np.empty(shape, dtype=dtype)
        check(_lib.lib().rr_dev_download(self.device, ptr(out), self.address + offset, out.nbytes))
        return out

    def free(self) -> None:
        if self.address:
            _lib.lib().rr_dev_free(self.device, self.address)
            self.address = 0

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def dev_alloc_stats() -> dict:
    """rr_dev_alloc_stats: the engine's device allocations alive now and made since the process started (plans, calls and DeviceBuffers alike)."""
    out = np.zeros(2, dtype=np.int64)
    check(_lib.lib().rr_dev_alloc_stats(ptr(out)))
    return dict(live=int(out[0]), made=int(out[1]))


def rows_upload(dst, dst_pitch: int, path, file_offset: int, file_pitch: int, row_bytes: int, n_rows: int, device: int = 0, stream=None) -> None:
    """rr_rows_upload: rows of a file straight into a device array (pinned staging, reader threads beside the copy engine)."""
    check(_lib.lib().rr_rows_upload(int(device), ptr(dst), int(dst_pitch), str(path).encode(), int(file_offset), int(file_pitch), int(row_bytes), int(n_rows), stream))


def rows_download(src, src_pitch: int, path, file_offset: int, file_pitch: int, row_bytes: int, n_rows: int, device: int = 0, stream=None) -> None:
    """rr_rows_download: device rows straight into (an existing region of) a file."""
    check(_lib.lib().rr_rows_download(int(device), ptr(src), int(src_pitch), str(path).encode(), int(file_offset), int(file_pitch), int(row_bytes), int(n_rows), stream))


def copy_bandwidth(device: int = 0, nbytes: int = 1 << 31, reps: int = 10) -> float:
    """Measured device copy rate in GB/s (read + write), see rr_copy_bandwidth."""
    out = C.c_double(0.0)
    check(_lib.lib().rr_copy_bandwidth(int(device), int(nbytes), int(reps), C.byref(out)))
    return float(out.value)


def synchronize(device: int = 0) -> None:
    check(_lib.lib().rr_dev_synchronize(int(device)))
