"""Device-resident handling of one input file: buffers that are freed together, the one statement of what an engine refusal
means, and the walk through the forms in which the engine takes a file (post-processing of
river_route/routers/TransformMuskingum.py:128-142 on the GPU).

`route_file` is the routers' per-file driver.  From the router it needs four hooks (RapidMuskingum, UnitMuskingum):
`_lateral_coefficient()` puts the coefficients on the plan, `_device_state(arena)` uploads the state and returns a handle to it,
`_device_calls()` gives the engine call of each (rows in, rows out) pair and `_device_state_back(state)` reads the state back;
UnitMuskingum adds `_device_lower`, the convolution as a pass of its own."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

from .. import engine
from .._lib import RR_E_ALLOC, RR_E_UNSUPPORTED, RRError

__all__ = ['Arena', 'DeviceOutOfMemory', 'RunoffPieces', 'route_file', 'taken']


class DeviceOutOfMemory(RuntimeError):
    """The file does not fit on the card next to the engine's own buffers: route it through the host-array path."""


class Arena:
    """Device buffers of one file; everything is released on exit, whatever happened in between."""

    def __init__(self, device: int):
        self.device, self._held = device, []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for b in self._held:
            b.free()
        self._held.clear()

    def empty(self, nbytes: int) -> engine.DeviceBuffer:
        try:
            buf = engine.DeviceBuffer(max(int(nbytes), 8), self.device)
        except RRError as e:
            if e.code == RR_E_ALLOC:
                raise DeviceOutOfMemory(str(e)) from e
            raise
        self._held.append(buf)
        return buf

    def put(self, array: np.ndarray) -> engine.DeviceBuffer:
        a = np.ascontiguousarray(array)
        return self.empty(a.nbytes).upload(a)

    def release(self, buf: engine.DeviceBuffer) -> None:
        buf.free()
        self._held.remove(buf)


def taken(call, last: bool = False, alloc_escapes: bool = False) -> bool:
    """The refusal policy of the device path, stated once.  Makes a call into the engine (a routing call of the plan, a file copy, rr_runoff_to_qlateral_dev); True where the engine took it.

    RR_E_UNSUPPORTED is "the engine does not take this form": False, and the caller tries the next form -- unless this was the `last`
    one, then the error leaves route().  RR_E_ALLOC is "no room": DeviceOutOfMemory, which ends the device path of this source (a file or
    gridded runoff is then taken as a host array, a host array goes to the host path).  `alloc_escapes` marks the calls that have
    always handed RR_E_ALLOC on as the RRError it is.  Every other code is an error and propagates."""
    try:
        call()
        return True
    except RRError as e:
        if e.code == RR_E_UNSUPPORTED and not last:
            return False
        if e.code == RR_E_ALLOC and not alloc_escapes:
            raise DeviceOutOfMemory(str(e)) from e
        raise


class RunoffPieces(NamedTuple):
    """Gridded runoff on the device: the point-major block (stride 1 along time, `stride_p` between points) and the CSR weights."""
    n_points: int
    indptr: engine.DeviceBuffer
    indices: engine.DeviceBuffer
    weights: engine.DeviceBuffer
    block: engine.DeviceBuffer
    is_f32: bool
    stride_p: int
    area: engine.DeviceBuffer | None
    flags: int


def route_file(router, source, sink=None):
    """(final state, float32 discharge rows at dt_discharge) of one input file, on the device where it fits.

    `source` is a host array (T, n), the flat float32 rows of a NetCDF-3 file (nc3.RowBlock) or gridded runoff (RunoffSource); `sink`
    is None for host rows, or (discharge file, its dates, the routed file's name) for a RowBlock, whose rows then go from the device
    into that file and are returned as None.  The forms, in order: file to file; the inflow computed inside the routing call; float32
    rows; float64 rows; each with the float32 discharge written by the routing call itself, else float64 rows and rr_resample_cast_dev.
    The file copies and rr_runoff_to_qlateral_dev are under the same policy as the routing calls (`taken`).  A file or runoff source the device path gives up on is taken as a host array; a host array it gives up on goes to the host path."""
    from ..nc3 import RowBlock
    from ..runoff import RunoffSource
    if isinstance(source, (RowBlock, RunoffSource)):
        try:
            routed = _file_form(router, source, *sink) if isinstance(source, RowBlock) else _runoff_forms(router, source)
        except DeviceOutOfMemory:
            routed = None
        if routed is not None:
            return routed
        if isinstance(source, RowBlock):
            from ..io import read_qlateral
            source = read_qlateral(source.path, router.cfg.var_t, keep_float32=True)[1]
        else:
            source = source.to_array(router._as_volumes)      # the two-step form: (time, river) rows, then the routing call
    try:
        return _array_forms(router, source)
    except DeviceOutOfMemory as e:
        router.logger.warning(f'file does not fit on the device ({e}); routing it in chunks from host memory')
        return router._route_on_host(source)


def _file_form(router, rows, discharge_file, dates_out, runoff_file):
    """One file whose float32 rows lie flat in it -> the discharge file, without the (time, river) block ever being a host array:
    engine.rows_upload (page cache -> pinned chunks -> device), the float32-in float32-out routing call with the file's byte order
    converted in the kernels that read and write the rows (Plan.set_row_format), the discharge file's header
    (nc3.create_discharge_file: the layout of Muskingum.py:337-351), engine.rows_download.  None where the engine refuses the form."""
    from .. import nc3
    T, n, per, dev = rows.rows, router.A.shape[0], router.num_runoff_steps_per_discharge, router.cfg.device
    router._check_shape((T, rows.cols))
    router._lateral_coefficient()
    with Arena(dev) as arena:
        d_rows, d_out = arena.empty(T * n * 4), arena.empty((T // per) * n * 4)
        state = router._device_state(arena)
        # (the two file copies are under the policy like the routing call: RR_E_ALLOC is their pinned staging not being there)
        if not taken(lambda: engine.rows_upload(d_rows, n * 4, rows.path, rows.offset, rows.pitch, n * 4, T, device=dev)):
            return None
        router._plan.set_row_format(rows.big_endian, True)      # a NetCDF-3 discharge file: big-endian rows out
        try:
            if not taken(lambda: router._device_calls()['f32', 'f32'](state, d_rows, T, d_out)):
                return None
        finally:
            router._plan.set_row_format(False, False)
        out = nc3.create_discharge_file(discharge_file, dates_out, router.river_ids, router.cfg.var_river_id, router.cfg.var_discharge, runoff_file)
        if not taken(lambda: engine.rows_download(d_out, n * 4, out.path, out.offset, out.pitch, n * 4, T // per, device=dev)):
            return None      # (the array forms write the discharge file again)
        return router._device_state_back(state), None


def _runoff_forms(router, source):
    """Gridded runoff of one file routed without leaving the GPU: the runoff block and the weight table go up once.  Where the router
    has the call and there is one routing step per runoff step, the catchment inflow is computed inside the pass that fills the engine's
    records (rr_rapid_route_runoff_dev): it never exists as (time, river) rows, on the host or in HBM (13.7 ms against 16.3 ms for 1M
    reaches x 744 steps, profiles/r02_runoff_path.txt).  Otherwise, or where the engine refuses that, rr_runoff_to_qlateral_dev writes
    it as float64 device rows (volumes for RapidMuskingum, depths for UnitMuskingum) and the forms for such rows follow."""
    T, n, per, dev = source.runoff_tp.shape[0], router.A.shape[0], router.num_runoff_steps_per_discharge, router.cfg.device
    if source.river_ids.shape[0] != n or T != router.num_runoff_steps:
        raise ValueError(f'gridded runoff covers {source.river_ids.shape[0]} rivers x {T} steps, the network and time options '
                         f'expect {n} x {router.num_runoff_steps}')
    block = source.point_major()
    in_pass = router._device_calls().get(('runoff', 'f32'))
    if in_pass is not None and router.num_routing_steps_per_runoff == 1:
        router._lateral_coefficient()
        with Arena(dev) as arena:
            state, d_f32 = router._device_state(arena), arena.empty((T // per) * n * 4)
            pieces = RunoffPieces(block.shape[0], arena.put(source.indptr), arena.put(source.indices), arena.put(source.weights), arena.put(block),
                                  block.dtype == np.float32, block.shape[1], arena.put(source.area), source.flags)
            if taken(lambda: in_pass(state, pieces, T, d_f32), alloc_escapes=True):      # (RR_E_ALLOC of this call has always escaped)
                q_array = d_f32.download(np.float32, (T // per, n))
                return router._device_state_back(state), q_array
    with Arena(dev) as arena:
        d_block, d_ptr, d_idx, d_w = arena.put(block), arena.put(source.indptr), arena.put(source.indices), arena.put(source.weights)
        d_area = arena.put(source.area) if router._as_volumes else None
        d_lat = arena.empty(T * n * 8)
        if not taken(lambda: engine.runoff_to_qlateral_dev(n, block.shape[0], T, d_ptr, d_idx, d_w, d_block, block.dtype == np.float32, 1,
                                                           block.shape[1], d_area, source.flags, d_lat, device=dev),
                     alloc_escapes=True):      # (more steps than one call takes: the source as a host array; RR_E_ALLOC has always escaped here)
            return None
        arena.release(d_block)
        return _rows_forms(router, arena, 'f64', d_lat, T, last=False)


def _array_forms(router, array):
    """A host array: float32 rows are uploaded as they are and converted in the pass that fills the engine's records (bit for bit what
    their float64 copy gives: float32 -> float64 is exact); where the engine refuses every float32-in form, the rows are widened."""
    ql = router._check_lateral(array, keep_float32=True)
    if ql.dtype == np.float32:
        with Arena(router.cfg.device) as arena:
            routed = _rows_forms(router, arena, 'f32', arena.put(ql), ql.shape[0], last=False)
        if routed is not None:
            return routed
        ql = ql.astype(np.float64)
    with Arena(router.cfg.device) as arena:
        return _rows_forms(router, arena, 'f64', arena.put(ql), ql.shape[0], last=True)


def _rows_forms(router, arena, kind, d_rows, T, last: bool):
    """(T, n) rows of `kind` on the device -> (final state, float32 discharge rows), or None where the engine refuses every form for
    such rows (`last`: there is nothing after them, the refusal leaves route()).

    The fused call writes float32 rows itself (the mean over `per` rows and the cast happen in the pass that returns the records to
    params order); where the engine refuses it, the plain call routes into float64 rows and rr_resample_cast_dev reduces them.  A kind
    without a plain call (UnitMuskingum's runoff depths) may be lowered by the router to one that has it (`_device_lower`)."""
    n, per = router.A.shape[0], router.num_runoff_steps_per_discharge
    router._lateral_coefficient()
    state = router._device_state(arena)
    calls = router._device_calls()
    while True:
        d_f32 = arena.empty((T // per) * n * 4)
        fused, plain = calls[kind, 'f32'], calls.get((kind, 'f64'))
        # (the fused calls that have no plain one were never part of the fused/plain sequence: their RR_E_ALLOC escapes as an RRError,
        # rr_unit_route_uh_dev's among them, where every other no-room takes the host path)
        if taken(lambda: fused(state, d_rows, T, d_f32), alloc_escapes=plain is None):
            break
        if plain is not None:
            d_f64 = arena.empty(T * n * 8)
            if not taken(lambda: plain(state, d_rows, T, d_f64), last=last):
                return None
            engine.resample_cast_dev(d_f64, T, n, per, d_f32, arena.device)
            break
        arena.release(d_f32)
        lowered = router._device_lower(arena, state, kind, d_rows, T)
        if lowered is None:
            return None
        kind, d_rows = lowered
    q_array = d_f32.download(np.float32, (T // per, n))
    return router._device_state_back(state), q_array
