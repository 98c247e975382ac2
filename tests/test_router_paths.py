"""
Which engine calls the routers make for one input file, in which order, and what they do when the engine refuses a form or the
device has no room: the ladder of river_route_amd/routers (flat float32 file -> gridded runoff -> float32 rows -> float64 rows ->
host path), pinned call for call without a GPU and without the library.

The engine is a recording stand-in plan with the device calls (`*_dev`), the device buffer a host-backed fake that counts live
buffers, and the module-level device functions are recorders; nc3 runs for real on a tmp_path file.  The stand-in answers
RR_E_UNSUPPORTED or RR_E_ALLOC at the engine calls it is told to, the fake buffer RR_E_ALLOC at the k-th allocation, and the recorders
of the file copies and of rr_runoff_to_qlateral_dev the code they are given.  What the
routers must do then is written down once, as `Model` below (a transcription of the documented ladder, not of the code), and every
case compares the recorded run with it: the sequence of calls (name, T, nsub, factor, output kind), the row-format calls, the
warning, the final exception, whether the unit-hydrograph state object was replaced, and that no device buffer stays alive.
"""
import logging

import numpy as np
import pandas as pd
import pytest
import scipy.sparse

import river_route_amd as rr
from river_route_amd import engine, nc3
from river_route_amd import uhkernels as uhk_mod
from river_route_amd._lib import RR_E_ALLOC, RR_E_UNSUPPORTED, RRError
from river_route_amd.routers import _device
from river_route_amd.routers import muskingum as musk_mod
from river_route_amd.runoff import RunoffSource

N, T, N_KS, POINTS = 5, 8, 3, 4
T0 = np.datetime64('2021-03-04T00:00:00', 's')
DATES = T0 + 3600 * np.arange(T).astype('timedelta64[s]')
U, A = RR_E_UNSUPPORTED, RR_E_ALLOC


class Recorder:
    """The events of one route() and the failures to inject into it."""

    def __init__(self, call_codes=(), alloc_fail=None, function_codes=None):
        self.events, self.formats = [], []
        self.call_codes, self.alloc_fail, self.function_codes = dict(enumerate(call_codes, 1)), alloc_fail, function_codes or {}
        self.calls = self.allocs = self.live = 0

    def function(self, name, *what):
        """A module-level device function (no engine call of the plan): recorded, and refused where the run says so."""
        self.events.append((name, *what))
        if name in self.function_codes:
            raise RRError(self.function_codes[name], f'injected in {name}')

    def engine_call(self, name, rows, nsub, factor, out):
        self.calls += 1
        self.events.append((name, int(rows), int(nsub), int(factor), out))
        code = self.call_codes.get(self.calls)
        if code is not None:
            raise RRError(code, f'injected at engine call {self.calls}')


REC: Recorder = None      # (the stand-ins are built by the routers, so they find the run's recorder here)


class FakeBuffer:
    """engine.DeviceBuffer on host memory."""

    def __init__(self, nbytes, device=0):
        REC.allocs += 1
        if REC.allocs == REC.alloc_fail:
            raise RRError(A, f'injected at allocation {REC.allocs}')
        self.device, self.nbytes, self.mem, self.address = device, int(nbytes), bytearray(int(nbytes)), 1
        REC.live += 1

    def upload(self, array, offset=0):
        raw = np.ascontiguousarray(array).tobytes()
        self.mem[offset:offset + len(raw)] = raw
        return self

    def download(self, dtype, shape, offset=0):
        count = int(np.prod(shape))
        return np.frombuffer(bytes(self.mem), dtype=dtype, count=count, offset=offset).reshape(shape).copy()

    def free(self):
        if self.address:
            self.address = 0
            REC.live -= 1


def _out(discharge, discharge32):
    assert (discharge is None) != (discharge32 is None)
    return 'f32' if discharge32 is not None else 'f64'


class RecordingPlan:
    """Stand-in for engine.Plan with the device calls: records, and refuses where the run's recorder says so."""

    def __init__(self, indptr, indices, device=0):
        self.n = len(indptr) - 1

    def close(self):
        pass

    def set_coeffs(self, lhs, c2, c3, c4_dt=None):
        pass

    def reserve(self, *a, **k):
        return dict(direct=False)

    def set_row_format(self, in32_big_endian=False, out32_big_endian=False):
        REC.formats.append((bool(in32_big_endian), bool(out32_big_endian)))
        REC.events.append(('set_row_format', bool(in32_big_endian), bool(out32_big_endian)))

    # the host calls
    def rapid_route(self, q_t, ql, d, nsub):
        REC.events.append(('rapid_route', ql.shape[0], int(nsub)))

    def unit_route(self, q_ch, q_full, conv, d, nsub):
        REC.events.append(('unit_route', conv.shape[0], int(nsub)))

    # the device calls, with engine.Plan's signatures
    def rapid_route_dev(self, q_t, qlateral, ql_rows, discharge, out_rows, T, num_substeps, stream=None):
        REC.engine_call('rapid_route_dev', T, num_substeps, 1, 'f64')

    def rapid_route_f32_dev(self, q_t, qlateral, ql_rows, discharge32, T, num_substeps, factor=1, stream=None):
        REC.engine_call('rapid_route_f32_dev', T, num_substeps, factor, 'f32')

    def rapid_route_f32in_dev(self, q_t, qlateral32, ql_rows, T, num_substeps, discharge=None, out_rows=0, discharge32=None, factor=1, stream=None):
        REC.engine_call('rapid_route_f32in_dev', T, num_substeps, factor, _out(discharge, discharge32))

    def rapid_route_runoff_dev(self, q_t, n_points, indptr, indices, weights, runoff, runoff_is_f32, stride_t, stride_p, area, flags, T,
                               discharge=None, discharge32=None, factor=1, stream=None):
        REC.engine_call('rapid_route_runoff_dev', T, 1, factor, _out(discharge, discharge32))

    def unit_route_dev(self, q_ch, q_full, convolved, conv_rows, discharge, out_rows, T, num_substeps, stream=None):
        REC.engine_call('unit_route_dev', T, num_substeps, 1, 'f64')

    def unit_route_f32_dev(self, q_ch, q_full, convolved, conv_rows, discharge32, T, num_substeps, factor=1, stream=None):
        REC.engine_call('unit_route_f32_dev', T, num_substeps, factor, 'f32')

    def unit_route_uh_dev(self, q_ch, q_full, q_final, uh_kernel, uh_state, n_ks, depth, T, num_substeps, discharge=None, discharge32=None,
                          factor=1, stream=None):
        REC.engine_call('unit_route_uh_dev', T, num_substeps, factor, _out(discharge, discharge32))

    def unit_route_uh_f32in_dev(self, q_ch, q_full, q_final, uh_kernel, uh_state, n_ks, depth32, T, num_substeps, discharge=None,
                                discharge32=None, factor=1, stream=None):
        REC.engine_call('unit_route_uh_f32in_dev', T, num_substeps, factor, _out(discharge, discharge32))


@pytest.fixture(autouse=True)
def stand_ins(monkeypatch):
    monkeypatch.setattr(musk_mod, 'Plan', RecordingPlan)
    recorders = dict(
        DeviceBuffer=FakeBuffer,
        resample_cast_dev=lambda d, rows, n, factor, out, device=0, stream=None: REC.function('resample_cast_dev', rows, factor),
        uh_convolve_dev=lambda k, s, lat, out, T, n_ks, n, device=0, stream=None: REC.function('uh_convolve_dev', T),
        runoff_to_qlateral_dev=lambda n, p, T, *a, **kw: REC.function('runoff_to_qlateral_dev', T),
        rows_upload=lambda dst, dp, path, off, fp, rb, rows, device=0, stream=None: REC.function('rows_upload', rows),
        rows_download=lambda src, sp, path, off, fp, rb, rows, device=0, stream=None: REC.function('rows_download', rows))
    for name, fake in recorders.items():      # (the routers reach these through the engine module or through names bound in _device)
        monkeypatch.setattr(engine, name, fake)
        if hasattr(_device, name):
            monkeypatch.setattr(_device, name, fake)
    monkeypatch.setattr(engine, 'runoff_to_qlateral', lambda indptr, indices, w, runoff_tp, *a, **kw: np.zeros((runoff_tp.shape[0], len(indptr) - 1)))

    def host_convolve(kernel, state, lateral, device=0):
        REC.events.append(('uh_convolve', lateral.shape[0]))
        return np.zeros(lateral.shape)
    monkeypatch.setattr(uhk_mod, 'uh_convolve', host_convolve)


@pytest.fixture(scope='module')
def inputs(tmp_path_factory):
    from scipy.io import netcdf_file
    tmp = tmp_path_factory.mktemp('paths')
    params = tmp / 'params.parquet'      # 1 -> 3 <- 2, 3 -> 5 <- 4
    pd.DataFrame({'river_id': [1, 2, 3, 4, 5], 'downstream_river_id': [3, 3, 5, 5, -1], 'k': [3000.0] * N, 'x': [0.2] * N}).to_parquet(params)
    kernel = tmp / 'uh.npz'
    scipy.sparse.save_npz(kernel, scipy.sparse.csr_matrix(np.full((N_KS, N), 1.0 / N_KS)))
    rows32 = np.linspace(0.0, 1.0, T * N, dtype=np.float32).reshape(T, N)
    lateral = tmp / 'ql.nc'
    with netcdf_file(str(lateral), 'w', version=2) as ds:
        ds.createDimension('time', T)
        ds.createDimension('river_id', N)
        tv = ds.createVariable('time', 'f8', ('time',))
        tv.units = 'seconds since 1970-01-01 00:00:00'
        tv[:] = DATES.astype(np.int64).astype(np.float64)
        ds.createVariable('qlateral', 'f4', ('time', 'river_id'))[:] = rows32
    runoff = RunoffSource(np.ones((T, POINTS), np.float32), np.array([0, 1, 2, 3, 4, 4], np.int32), np.arange(POINTS, dtype=np.int32),
                          np.ones(POINTS), np.ones(N), 0, DATES, np.arange(1, N + 1, dtype=np.int64), False)
    return dict(tmp=tmp, params=str(params), kernel=str(kernel), lateral=str(lateral),
                sources={'file': None, 'runoff': runoff, 'f32': rows32, 'f64': rows32.astype(np.float64)})


class Outcome:
    def __init__(self, events, error, uh_replaced, allocs, live=0):      # (live: of the recorded run only)
        self.events, self.error, self.uh_replaced, self.allocs, self.live = events, error, uh_replaced, allocs, live


def run(inputs, router, source, per, nsub, call_codes=(), alloc_fail=None, function_codes=None) -> Outcome:
    """One route() of one file on the real routers, with the failures injected."""
    global REC
    REC = Recorder(call_codes, alloc_fail, function_codes)
    cls = rr.RapidMuskingum if router == 'rapid' else rr.UnitMuskingum
    item = inputs['sources'][source]
    out_dir = inputs['tmp'] / f'{router}_{source}'
    out_dir.mkdir(exist_ok=True)
    if item is not None:      # arrays and gridded runoff are handed over by the generator; the file goes through the real one
        class cls(cls):
            def _qlateral_generator(self):
                yield DATES, item, self.cfg.qlateral_files[0], self.cfg.discharge_files[0]
    kw = dict(uh_kernel_file=inputs['kernel']) if router == 'unit' else {}
    r = cls(params_file=inputs['params'], qlateral_files=[inputs['lateral']], discharge_dir=str(out_dir), dt_routing=3600 // nsub,
            dt_discharge=3600 * per, log_level='WARNING', **kw)

    class Warnings(logging.Handler):
        def emit(self, record):
            if 'does not fit on the device' in record.getMessage():
                assert record.levelno == logging.WARNING
                REC.events.append(('warning',))
    r.logger.handlers[:] = [Warnings()]
    if router == 'unit':
        r._uh = uhk_mod.UnitHydrograph(inputs['kernel'])      # (what _hook_before_route loads, held here to see whether its state is replaced)
    uh_before = r._uh.state if router == 'unit' else None
    error = None
    try:
        r.route()
    except RRError as e:
        error = e.code
    if REC.formats:
        assert REC.formats[-1] == (False, False)
    return Outcome(REC.events, error, router == 'unit' and r._uh.state is not uh_before, REC.allocs, REC.live)


# ---- the ladder as documented: what one file must do, given the codes the engine answers and the allocation that finds no room ----
class NoRoom(Exception):
    """DeviceOutOfMemory: an arena allocation failed, or an engine call that converts RR_E_ALLOC met it."""


class Refused(Exception):
    """RR_E_UNSUPPORTED from the last form of a kind of rows."""


class Escape(Exception):
    """An RRError that leaves route()."""

    def __init__(self, code):
        self.code = code


class Model:
    def __init__(self, router, per, nsub, call_codes=(), alloc_fail=None, function_codes=None):
        self.router, self.per, self.nsub = router, per, nsub
        self.codes, self.alloc_fail, self.function_codes = dict(enumerate(call_codes, 1)), alloc_fail, function_codes or {}
        self.events, self.calls, self.allocs, self.uh_replaced = [], 0, 0, False

    def alloc(self, count=1):
        for _ in range(count):
            self.allocs += 1
            if self.allocs == self.alloc_fail:
                raise NoRoom

    def call(self, name, out, alloc=NoRoom):
        """An engine call: True where it is taken, False on a refusal; RR_E_ALLOC raises `alloc`."""
        self.calls += 1
        self.events.append((name, T, 1 if name == 'rapid_route_runoff_dev' else self.nsub, self.per if out == 'f32' else 1, out))
        code = self.codes.get(self.calls)
        if code == A:
            raise Escape(A) if alloc is Escape else alloc()
        return code is None

    def function(self, name, *what):
        """A module-level device function: its code where the run injects one (the caller says what that means), else None."""
        self.events.append((name, *what))
        return self.function_codes.get(name)

    def fused_then_plain(self, fused, plain):
        """The float32 rows of one routed file: the call that writes them itself, else float64 rows and the resampling cast."""
        self.alloc()                                       # float32 rows out
        if not self.call(fused, 'f32'):
            self.alloc()                                   # float64 rows out
            if not self.call(plain, 'f64'):
                raise Refused
            self.events.append(('resample_cast_dev', T, self.per))

    def file_form(self, name, state_buffers):
        """Form 1.  True: written to the discharge file."""
        try:
            self.alloc(2 + state_buffers)
            if self.function('rows_upload', T) in (U, A):      # (RR_E_ALLOC: the pinned staging could not be allocated)
                return False
            self.events.append(('set_row_format', True, True))
            try:
                taken = self.call(name, 'f32')
            finally:
                self.events.append(('set_row_format', False, False))
            return taken and self.function('rows_download', T // self.per) not in (U, A)
        except NoRoom:
            return False

    def host(self):
        self.events.append(('warning',))
        self.events += [('rapid_route', T, self.nsub)] if self.router == 'rapid' else [('uh_convolve', T), ('unit_route', T, self.nsub)]

    def runoff_rows(self):
        """rr_runoff_to_qlateral_dev inside the gridded-runoff attempt: a refusal ends the attempt, RR_E_ALLOC leaves route()."""
        code = self.function('runoff_to_qlateral_dev', T)
        if code == U:
            raise Refused
        if code == A:
            raise Escape(A)

    def route(self, source) -> Outcome:
        error = None
        try:
            (self.rapid if self.router == 'rapid' else self.unit)(source)
        except Escape as e:
            error = e.code
        except Refused:
            error = U
        return Outcome(self.events, error, self.uh_replaced, self.allocs)

    def rapid(self, source):
        if source == 'file':
            if self.file_form('rapid_route_f32in_dev', 1):
                return
            source = 'f32'
        if source == 'runoff':
            try:
                if self.nsub == 1:
                    self.alloc(2 + 5)                      # state, float32 rows out; CSR pieces, block, area
                    if self.call('rapid_route_runoff_dev', 'f32', alloc=Escape):
                        return
                self.alloc(6)                              # block, CSR pieces, area, float64 lateral rows
                self.runoff_rows()
                self.alloc()                               # state
                return self.fused_then_plain('rapid_route_f32_dev', 'rapid_route_dev')
            except (NoRoom, Refused):
                source = 'f64'
        try:
            if source == 'f32':
                try:
                    self.alloc(2)                          # rows, state
                    return self.fused_then_plain('rapid_route_f32in_dev', 'rapid_route_f32in_dev')
                except Refused:
                    pass
            self.alloc(2)
            self.fused_then_plain('rapid_route_f32_dev', 'rapid_route_dev')
        except NoRoom:
            self.host()

    def unit_float64(self):
        """Form 4 of UnitMuskingum on float64 depths already on the device."""
        self.alloc(5 + 1)                                  # kernel, UH state, seed twice, final state; float32 rows out
        if not self.call('unit_route_uh_dev', 'f32', alloc=Escape):
            self.alloc()                                   # convolved rows (the float32 rows were released)
            self.events.append(('uh_convolve_dev', T))
            self.fused_then_plain('unit_route_f32_dev', 'unit_route_dev')
        self.uh_replaced = True

    def unit(self, source):
        if source == 'file':
            if self.file_form('unit_route_uh_f32in_dev', 5):
                self.uh_replaced = True
                return
            source = 'f32'
        if source == 'runoff':
            try:
                self.alloc(5)                              # block, CSR pieces, float64 depth rows
                self.runoff_rows()
                return self.unit_float64()
            except (NoRoom, Refused):
                source = 'f64'
        try:
            if source == 'f32':
                self.alloc(1 + 5 + 1)
                if self.call('unit_route_uh_f32in_dev', 'f32', alloc=Escape):
                    self.uh_replaced = True
                    return
            self.alloc()
            self.unit_float64()
        except NoRoom:
            self.host()


def compare(inputs, router, source, per, nsub, call_codes=(), alloc_fail=None, function_codes=None) -> Outcome:
    """The recorded run, after comparing it with the model's."""
    want = Model(router, per, nsub, call_codes, alloc_fail, function_codes).route(source)
    got = run(inputs, router, source, per, nsub, call_codes, alloc_fail, function_codes)
    where = f'{router} {source} per={per} nsub={nsub} codes={call_codes} alloc_fail={alloc_fail} functions={function_codes}'
    assert got.events == want.events, where
    assert got.error == want.error, where
    assert got.uh_replaced == want.uh_replaced, where
    assert got.allocs == want.allocs, where
    assert got.live == 0, where
    return got


CASES = [(router, source, per, nsub) for router in ('rapid', 'unit') for source in ('file', 'runoff', 'f32', 'f64') for per in (1, 2)
         for nsub in ((1, 2) if source == 'runoff' else (1,))]


@pytest.mark.parametrize('router,source,per,nsub', CASES)
def test_forms_refusals_and_no_room(inputs, router, source, per, nsub):
    """Every form taken cleanly; every form reached by the refusals before it, then refused (-> the next form, or the RRError that
    today leaves route() from the last one) or out of memory in the engine call (-> the array forms, the host path with the warning,
    or the escapes: RapidMuskingum's runoff call and UnitMuskingum's fused convolution calls hand RR_E_ALLOC on as an RRError)."""
    refused = 0
    while True:
        clean = compare(inputs, router, source, per, nsub, (U,) * refused)
        compare(inputs, router, source, per, nsub, (U,) * refused + (A,))
        if clean.error is not None:      # the last form refused as well: nothing further to reach
            assert clean.error == U
            break
        refused += 1
    assert refused >= 2


@pytest.mark.parametrize('router,source,per,nsub', CASES)
def test_no_room_at_each_arena_allocation(inputs, router, source, per, nsub):
    """Every allocation of every form finding no room: the file and gridded-runoff forms go on with the array forms, the array forms
    with the host path and its warning; nothing escapes, nothing stays allocated."""
    refused = 0
    while True:
        clean = Model(router, per, nsub, (U,) * refused).route(source)
        if clean.error is not None:
            break
        for k in range(1, clean.allocs + 1):
            got = compare(inputs, router, source, per, nsub, (U,) * refused, alloc_fail=k)
            assert got.error != A, (refused, k)      # (RR_E_UNSUPPORTED may still leave it: the refusals go on in the forms that follow)
        refused += 1


def test_unit_fused_convolution_out_of_memory_escapes(inputs):
    """The one case where RR_E_ALLOC leaves route() as an RRError instead of taking the host path: rr_unit_route_uh_dev on float64 depths."""
    got = run(inputs, 'unit', 'f64', 1, 1, (A,))
    assert got.error == A and got.events == [('unit_route_uh_dev', T, 1, 1, 'f32')] and not got.uh_replaced and got.live == 0


@pytest.mark.parametrize('router', ['rapid', 'unit'])
@pytest.mark.parametrize('per', [1, 2])
def test_refusals_outside_the_engine_calls(inputs, router, per):
    """The device functions around the routing call answer too.  rr_rows_upload and rr_rows_download report RR_E_ALLOC where their pinned
    staging cannot be allocated: the file form ends and the file is read as an array (after rows_download: the array forms write the
    discharge file again).  rr_runoff_to_qlateral_dev refuses (RR_E_UNSUPPORTED) more than 1,048,560 steps in a call: the gridded-runoff
    attempt ends and the source is taken as a host array; its RR_E_ALLOC is not converted and leaves route()."""
    for name in ('rows_upload', 'rows_download'):
        for code in (A, U):
            got = compare(inputs, router, 'file', per, 1, function_codes={name: code})
            assert got.error is None and got.events[-1][0] in ('rapid_route_f32in_dev', 'unit_route_uh_f32in_dev')      # the float32 array form
    for nsub in (1, 2):
        refused = (U,) if (router, nsub) == ('rapid', 1) else ()      # (past the call that computes the inflow inside the routing pass)
        got = compare(inputs, router, 'runoff', per, nsub, refused, function_codes={'runoff_to_qlateral_dev': U})
        assert got.error is None and got.events[-1][0] in ('rapid_route_f32_dev', 'unit_route_uh_dev')      # the float64 array form
        got = compare(inputs, router, 'runoff', per, nsub, refused, function_codes={'runoff_to_qlateral_dev': A})
        assert got.error == A
