"""
Skill scores of a routed run: river_route.metrics of the reference (`rr.metrics.kge2012(obs, sim)`), plus a batched form
that scores every column of a (time, reach) array where it already lies, on the GPU.

1-D inputs (one series each) are scored on the host with numpy, exactly as the reference does: a numpy scalar comes back
and no GPU or built library is needed.  2-D inputs of shape (T, n) give one score per column, shape (n,), computed on the
GPU in one streaming read (rr_metrics_update_dev / rr_metrics_finish_dev, include/rr_hip.h): numpy arrays are uploaded
and numpy comes back; torch tensors on the device (float32 or float64) are read in place when their columns are adjacent
and their rows do not overlap (any row stride from the width up; other views, broadcast rows among them, are copied
first), and device tensors come back.  `scores` returns all five scores of one pass; `Accumulator` scores a series that
arrives in row blocks, its per-column state staying on the device between blocks.

The device path merges per-column counts, means, M2 terms and co-moments exactly (Chan et al.) and matches the host
path run on each column of the float64 data (float32 data: widened to float64) to rtol 1e-10 -- for series whose |mean| / std stays
below 1e7: pearson_r and kge2012 err by about 0.03 x 2^-53 x (|mean| / std of both series), me, mae and mse by roundings only (DESIGN.md
sections 9 and 2d).  One divergence is known:
a column that is exactly constant has M2 == 0 on the device, so its pearson_r and kge2012 are nan, where numpy's
mean-then-subtract can leave a tiny non-zero standard deviation (1.4e-17 for 35,040 copies of 0.1) and the reference's
KGE then returns a finite number.

Gauge records with gaps: every function, `scores` and `Accumulator` take skip_missing=False.  With True a NaN in y_true marks a
missing observation and that pair is left out (1-D on the host: dropped before the reference's numpy calls; per column on the
GPU: rr_metrics_update_missing_dev), each column scored over its own kept pairs, whose number `scores` returns as 'count'.

Ensembles: `scores_members` and `MemberAccumulator` score the (members, T, m) rows of a generation of members against one shared
(T, n) observation block, or one per member, in one launch per update (rr_metrics_update_members_dev): member m's scores are those
`scores` gives for member m alone.  Plan.rapid_route_members_scores routes and scores a parameter ensemble without the discharge
leaving the device.
"""
from __future__ import annotations

import sys

import numpy as np

__all__ = ['mean_error', 'mean_absolute_error', 'mean_square_error', 'pearson_r', 'kling_gupta_efficiency_2012',
           'me', 'mae', 'mse', 'kge2012', 'scores', 'Accumulator', 'scores_members', 'MemberAccumulator', 'SCORES']

SCORES = ('me', 'mae', 'mse', 'pearson_r', 'kge2012')       # the rows of rr_metrics_finish_dev's out[5][n]
_UNUSED = object()      # Accumulator._stream before the first launch


def _torch_tensor(a) -> bool:
    t = sys.modules.get('torch')
    return t is not None and isinstance(a, t.Tensor)


def _kept(y_true, y_pred):
    """The pairs of two 1-D series whose y_true is not NaN (skip_missing=True on the host); without a NaN the inputs themselves,
    so a gap-free series is scored by the very same numpy calls."""
    t, p = np.asarray(y_true), np.asarray(y_pred)
    if t.ndim != 1 or t.shape != p.shape:
        raise ValueError(f'skip_missing needs two 1-D series of one length (got shapes {t.shape} and {p.shape})')
    keep = ~np.isnan(t)
    return (y_true, y_pred) if keep.all() else (t[keep], p[keep])


def _batched(y_true, y_pred) -> bool:
    """Per-column scores on the GPU: a torch tensor, or a 2-D array."""
    return _torch_tensor(y_true) or _torch_tensor(y_pred) or np.ndim(y_true) == 2 or np.ndim(y_pred) == 2


def mean_error(y_true, y_pred, skip_missing=False):
    """Mean of y_true - y_pred (the reference's sign: positive when the simulation is low)."""
    if _batched(y_true, y_pred):
        return scores(y_true, y_pred, skip_missing=skip_missing)['me']
    if skip_missing:
        y_true, y_pred = _kept(y_true, y_pred)
        if len(y_true) == 0:
            return np.float64(np.nan)
    return np.mean(np.asarray(y_true) - np.asarray(y_pred))


def mean_absolute_error(y_true, y_pred, skip_missing=False):
    """Mean of |y_true - y_pred|."""
    if _batched(y_true, y_pred):
        return scores(y_true, y_pred, skip_missing=skip_missing)['mae']
    if skip_missing:
        y_true, y_pred = _kept(y_true, y_pred)
        if len(y_true) == 0:
            return np.float64(np.nan)
    return np.mean(np.abs(np.asarray(y_true) - np.asarray(y_pred)))


def mean_square_error(y_true, y_pred, skip_missing=False):
    """Mean of (y_true - y_pred) ** 2."""
    if _batched(y_true, y_pred):
        return scores(y_true, y_pred, skip_missing=skip_missing)['mse']
    if skip_missing:
        y_true, y_pred = _kept(y_true, y_pred)
        if len(y_true) == 0:
            return np.float64(np.nan)
    return np.mean((np.asarray(y_true) - np.asarray(y_pred)) ** 2)


def pearson_r(y_true, y_pred, skip_missing=False):
    """Pearson correlation as np.corrcoef gives it: clipped to [-1, 1], nan when either series has zero variance."""
    if _batched(y_true, y_pred):
        return scores(y_true, y_pred, skip_missing=skip_missing)['pearson_r']
    if skip_missing:
        y_true, y_pred = _kept(y_true, y_pred)
        if len(y_true) == 0:
            return np.float64(np.nan)
    return np.corrcoef(y_true, y_pred)[0, 1]


def kling_gupta_efficiency_2012(y_true, y_pred, skip_missing=False):
    """Kling-Gupta efficiency as the reference computes it: 1 - sqrt((r - 1)^2 + (beta - 1)^2 + (gamma - 1)^2) with
    beta = mean_pred / mean_true and gamma = (mean_pred / std_pred) / (mean_true / std_true), standard deviations with
    ddof 0; nan when std_true, std_pred or mean_true is 0.

    Note: this gamma is the INVERSE of the coefficient-of-variation ratio of Kling et al. (2012), (std_pred / mean_pred) /
    (std_true / mean_true).  It is kept as the reference has it, so that scores agree with the reference's."""
    if _batched(y_true, y_pred):
        return scores(y_true, y_pred, skip_missing=skip_missing)['kge2012']
    if skip_missing:
        y_true, y_pred = _kept(y_true, y_pred)
        if len(y_true) == 0:
            return np.float64(np.nan)
    r = pearson_r(y_true, y_pred)
    mean_true, mean_pred = np.mean(y_true), np.mean(y_pred)
    std_true, std_pred = np.std(y_true), np.std(y_pred)
    if std_true == 0 or std_pred == 0 or mean_true == 0:
        return np.nan
    beta = mean_pred / mean_true
    gamma = (mean_pred / std_pred) / (mean_true / std_true)
    return 1 - np.sqrt(np.power(r - 1, 2) + np.power(beta - 1, 2) + np.power(gamma - 1, 2))


me = mean_error
mae = mean_absolute_error
mse = mean_square_error
kge2012 = kling_gupta_efficiency_2012


def scores(y_true, y_pred, columns=None, skip_missing=False) -> dict:
    """All five scores per column from one read of (T, n) y_true and (T, m) y_pred: {'me', 'mae', 'mse', 'pearson_r',
    'kge2012'} -> (n,) arrays (numpy in: numpy out; torch in: device tensors out).  columns: optional int array of
    length n, column j of y_true is scored against column columns[j] of y_pred (repeats allowed; no gather copy is
    made); without it m must equal n.  1-D inputs are scored as one column.

    skip_missing=True: an element of y_true that is NaN (as stored) is a missing observation, and column j's pair at that row
    is left out of all its sums; y_pred there is never looked at.  Every column is scored over its own kept pairs, and the
    result has one more key, 'count': (n,) float64, the pairs kept per column (0: all five scores NaN; 1: pearson_r and
    kge2012 NaN).  Inf is not missing, and a NaN of y_pred at a kept row still makes the column NaN."""
    t, p = _Rows(y_true, 'y_true'), _Rows(y_pred, 'y_pred')
    device = t.device if t.device is not None else (p.device if p.device is not None else 0)
    acc = Accumulator(t.cols, columns=columns, device=device, skip_missing=skip_missing)
    acc._update(t, p)
    return acc.result()


class Accumulator:
    """Per-column scores of series that arrive in row blocks: the rows of each input file of a run, or rows streamed
    from disk.  `update(true_rows, pred_rows)` merges (k, n) and (k, m) blocks into a per-column state kept on the GPU;
    `result()` returns the scores of all rows so far as `scores` does.  Splitting the rows differently changes results
    by rounding only (within 1e-12 relative); the same blocks in the same order give bit-identical results.
    skip_missing (fixed at construction): every update leaves out the pairs whose true value is NaN, as `scores` describes,
    and `result()` has the key 'count'; `rows` stays the number of rows seen, missing or not."""

    def __init__(self, n: int, columns=None, device: int = 0, skip_missing: bool = False):
        from . import engine
        self._engine = engine
        self.n, self.device, self.rows = int(n), int(device), 0
        self.skip_missing = bool(skip_missing)
        if self.n < 1:
            raise ValueError('Accumulator needs n >= 1 columns')
        self._columns, self._cols_dev = None, None
        if columns is not None:
            cols = np.asarray(columns.detach().cpu() if _torch_tensor(columns) else columns)
            if cols.shape != (self.n,) or not np.issubdtype(cols.dtype, np.integer):
                raise ValueError(f'columns must be a 1-D integer array of length {self.n}')
            if cols.min() < 0 or cols.max() > np.iinfo(np.int32).max:
                raise ValueError('columns holds a negative or too large column index')
            self._columns = cols.astype(np.int32)
            self._cols_dev = engine.DeviceBuffer(self._columns.nbytes, self.device).upload(self._columns)
        self._state = engine.DeviceBuffer(engine.METRICS_STATE * self.n * 8, self.device)
        self._state.upload(np.zeros(engine.METRICS_STATE * self.n))
        self._work, self._stream, self._torch = None, _UNUSED, False

    def update(self, true_rows, pred_rows) -> 'Accumulator':
        self._update(_Rows(true_rows, 'true_rows'), _Rows(pred_rows, 'pred_rows'))
        return self

    def _update(self, t: '_Rows', p: '_Rows') -> None:
        e = self._engine
        if t.cols != self.n:
            raise ValueError(f'true rows have {t.cols} columns, the accumulator {self.n}')
        if t.rows != p.rows:
            raise ValueError(f'true rows ({t.rows}) and predicted rows ({p.rows}) differ in number')
        if self._columns is None and p.cols != self.n:
            raise ValueError(f'predicted rows have {p.cols} columns, expected {self.n} (or pass columns=)')
        if self._columns is not None and self._columns.max() >= p.cols:
            raise ValueError(f'columns refers to column {int(self._columns.max())} of predicted rows with {p.cols} columns')
        for r in (t, p):
            if r.device is not None and r.device != self.device:
                raise ValueError(f'rows on device {r.device}, accumulator on device {self.device}')
        if t.rows == 0:
            return
        torch_in = t.tensor is not None or p.tensor is not None
        stream = None
        if torch_in:
            import torch
            stream = torch.cuda.current_stream(self.device).cuda_stream
            self._torch = True
        self._enter_stream(stream)
        t.to_device(self.device)
        p.to_device(self.device)
        need = e.metrics_work_bytes(self.n, t.rows)
        if self._work is None or self._work.nbytes < need:
            if self._work is not None:
                self._work.free()
            self._work = e.DeviceBuffer(need, self.device)
        update = e.metrics_update_missing_dev if self.skip_missing else e.metrics_update_dev
        update(self.n, t.rows, t.address, t.is_f32, t.pitch, p.address, p.is_f32, p.pitch, self._cols_dev, self._state,
               self._work, self._work.nbytes, device=self.device, stream=stream)
        if t.uploaded is not None or p.uploaded is not None:
            e.synchronize(self.device)            # the uploaded copies are freed on return
        self.rows += t.rows

    def _enter_stream(self, stream) -> None:
        """Enqueue on `stream` from here on: work the state and the work slab took part in on another stream is finished first."""
        if self._stream is not _UNUSED and stream != self._stream:
            self._engine.synchronize(self.device)
        self._stream = stream

    def result(self) -> dict:
        """{'me', 'mae', 'mse', 'pearson_r', 'kge2012'} -> (n,) scores of every row so far: device tensors if any update
        came as torch tensors, else numpy arrays.  With skip_missing also 'count', the pairs kept per column (row 0 of the state)."""
        e = self._engine
        if self._torch:
            import torch
            stream = torch.cuda.current_stream(self.device).cuda_stream
            self._enter_stream(stream)
            out = torch.empty((len(SCORES), self.n), dtype=torch.float64, device=torch.device('cuda', self.device))
            e.metrics_finish_dev(self.n, self._state, out.data_ptr(), device=self.device, stream=stream)
            if self.skip_missing:
                # row 0 of the state, copied on the stream the finish was enqueued on
                count = torch.as_tensor(_DeviceDoubles(self._state.address, self.n), device=out.device).clone()
        else:
            self._enter_stream(None)
            buf = e.DeviceBuffer(len(SCORES) * self.n * 8, self.device)
            e.metrics_finish_dev(self.n, self._state, buf, device=self.device)
            e.synchronize(self.device)
            out = buf.download(np.float64, (len(SCORES), self.n))
            buf.free()
            if self.skip_missing:
                count = self._state.download(np.float64, (self.n,))      # row 0 of the state
        res = {k: out[i] for i, k in enumerate(SCORES)}
        if self.skip_missing:
            res['count'] = count
        return res


class _DeviceDoubles:
    """`count` float64 values at a device address, for torch.as_tensor to look at in place (__cuda_array_interface__)."""

    def __init__(self, address: int, count: int):
        self.__cuda_array_interface__ = {'shape': (int(count),), 'typestr': '<f8', 'data': (int(address), False), 'strides': None,
                                         'version': 2}


class _Rows:
    """One input of an update: a (rows, cols) float32/float64 block in device memory, row `pitch` elements apart.
    numpy arrays (other dtypes: as float64) are uploaded by to_device; torch tensors on the GPU are used in place."""

    def __init__(self, a, name: str):
        self.tensor, self.uploaded, self.device = None, None, None
        if _torch_tensor(a):
            import torch
            if a.device.type != 'cuda':
                raise ValueError(f'{name}: torch tensor must be on the GPU (got {a.device})')
            if a.dtype not in (torch.float32, torch.float64):
                a = a.to(torch.float64)
            if a.dim() == 1:
                a = a.reshape(-1, 1)
            if a.dim() != 2:
                raise ValueError(f'{name} must be 1-D or 2-D (time, column)')
            # the kernel reads element (r, c) at r * pitch + c: rows that share elements (a broadcast or overlapping
            # view, row stride below the width) or columns that are not adjacent are copied into whole rows first
            if (a.shape[1] > 1 and a.stride(1) != 1) or (a.shape[0] > 1 and a.stride(0) < a.shape[1]):
                a = a.contiguous()
            self.tensor, self.device = a, a.device.index or 0
            self.rows, self.cols = int(a.shape[0]), int(a.shape[1])
            self.is_f32 = a.dtype == torch.float32
            self.pitch = int(a.stride(0)) if self.rows > 1 else self.cols
        else:
            a = np.asarray(a)
            if a.dtype not in (np.float32, np.float64):
                a = a.astype(np.float64)
            if a.ndim == 1:
                a = a.reshape(-1, 1)
            if a.ndim != 2:
                raise ValueError(f'{name} must be 1-D or 2-D (time, column)')
            self.host = np.ascontiguousarray(a)
            self.rows, self.cols = int(a.shape[0]), int(a.shape[1])
            self.is_f32 = a.dtype == np.float32
            self.pitch = self.cols

    def to_device(self, device: int) -> None:
        if self.tensor is not None or self.uploaded is not None:
            return
        from .engine import DeviceBuffer
        self.uploaded = DeviceBuffer(max(self.host.nbytes, 8), device).upload(self.host)

    @property
    def address(self) -> int:
        return int(self.tensor.data_ptr()) if self.tensor is not None else int(self.uploaded.address)


def scores_members(y_true, y_pred, columns=None, skip_missing=False) -> dict:
    """`scores` for every member of an ensemble from one read: y_pred is (members, T, m); y_true is (T, n), one observation block
    that all members are scored against, or (members, T, n).  Returns {'me', 'mae', 'mse', 'pearson_r', 'kge2012'[, 'count']} ->
    (members, n) arrays (numpy in: numpy out; torch in: device tensors out), row m what `scores` gives for member m alone -- bit
    for bit wherever members x ceil(n / 256) x ceil(T / 32) <= 2048 (both then cut the rows alike), within 1e-12 relative otherwise.
    columns (one map for all members) and skip_missing are those of `scores`."""
    t, p = _MemberRows(y_true, 'y_true', shared_ok=True), _MemberRows(y_pred, 'y_pred')
    columns = _member_columns(columns, t.cols)
    _check_member_rows(t.cols, p.members, columns, None, t, p)
    device = t.device if t.device is not None else (p.device if p.device is not None else 0)
    acc = MemberAccumulator(t.cols, p.members, columns=columns, device=device, skip_missing=skip_missing)
    acc._update(t, p)
    return acc.result()


def _member_columns(columns, n: int):
    """columns= as an int32 array of length n (None stays None), checked on the host."""
    if columns is None:
        return None
    cols = np.asarray(columns.detach().cpu() if _torch_tensor(columns) else columns)
    if cols.shape != (n,) or not np.issubdtype(cols.dtype, np.integer):
        raise ValueError(f'columns must be a 1-D integer array of length {n}')
    if cols.size and (cols.min() < 0 or cols.max() > np.iinfo(np.int32).max):
        raise ValueError('columns holds a negative or too large column index')
    return cols.astype(np.int32)


def _check_member_rows(n, members, columns, device, t: '_MemberRows', p: '_MemberRows') -> None:
    """Every shape rule of one members update, on the host (device None: any)."""
    if p.members != members:
        raise ValueError(f'predicted rows have {p.members} members, expected {members}')
    if t.members is not None and t.members != members:
        raise ValueError(f'true rows have {t.members} members, predicted rows {members} (or pass one 2-D block for all)')
    if t.cols != n:
        raise ValueError(f'true rows have {t.cols} columns, expected {n}')
    if t.rows != p.rows:
        raise ValueError(f'true rows ({t.rows}) and predicted rows ({p.rows}) differ in number')
    if columns is None and p.cols != n:
        raise ValueError(f'predicted rows have {p.cols} columns, expected {n} (or pass columns=)')
    if columns is not None and columns.size and columns.max() >= p.cols:
        raise ValueError(f'columns refers to column {int(columns.max())} of predicted rows with {p.cols} columns')
    for r in (t, p):
        if r.device is not None and device is not None and r.device != device:
            raise ValueError(f'rows on device {r.device}, accumulator on device {device}')
    if t.device is not None and p.device is not None and t.device != p.device:
        raise ValueError(f'true rows on device {t.device}, predicted rows on device {p.device}')


class MemberAccumulator:
    """`Accumulator` for the members of an ensemble: `update(true_rows, pred_rows)` merges a (members, k, m) block of predicted rows
    and its observations -- (k, n), shared by all members, or (members, k, n) -- into a per-member, per-column state kept on the GPU,
    one launch for all members; `result()` returns the scores of all rows so far, each (members, n).  numpy / torch in and out,
    streams, the reuse of the work slab, row blocks (1e-12 relative against one pass; the same blocks give the same bits) and
    skip_missing are `Accumulator`'s.  Torch tensors are read in place when their columns are adjacent and neither their rows nor
    their members overlap (any row and member stride from there up); other views are copied first."""

    def __init__(self, n: int, members: int, columns=None, device: int = 0, skip_missing: bool = False):
        from . import engine
        self._engine = engine
        self.n, self.members, self.device, self.rows = int(n), int(members), int(device), 0
        self.skip_missing = bool(skip_missing)
        if self.n < 1 or self.members < 1:
            raise ValueError('MemberAccumulator needs n >= 1 columns and members >= 1')
        if self.n * self.members > np.iinfo(np.int32).max:
            raise ValueError('MemberAccumulator: members * n must stay below 2^31')
        self._columns, self._cols_dev = _member_columns(columns, self.n), None
        if self._columns is not None:
            self._cols_dev = engine.DeviceBuffer(self._columns.nbytes, self.device).upload(self._columns)
        self._state = engine.DeviceBuffer(engine.METRICS_STATE * self.members * self.n * 8, self.device)
        self._state.upload(np.zeros(engine.METRICS_STATE * self.members * self.n))
        self._work, self._stream, self._torch = None, _UNUSED, False

    def update(self, true_rows, pred_rows) -> 'MemberAccumulator':
        self._update(_MemberRows(true_rows, 'true_rows', shared_ok=True), _MemberRows(pred_rows, 'pred_rows'))
        return self

    def _update(self, t: '_MemberRows', p: '_MemberRows') -> None:
        _check_member_rows(self.n, self.members, self._columns, self.device, t, p)
        if t.rows == 0:
            return
        stream = None
        if t.tensor is not None or p.tensor is not None:
            import torch
            stream = torch.cuda.current_stream(self.device).cuda_stream
            self._torch = True
        self._enter_stream(stream)
        t.to_device(self.device)
        p.to_device(self.device)
        self._launch(t.rows, t.address, t.is_f32, t.pitch, t.member_pitch, p.address, p.is_f32, p.pitch, p.member_pitch, stream)
        if t.uploaded is not None or p.uploaded is not None:
            self._engine.synchronize(self.device)            # the uploaded copies are freed on return

    def _launch(self, rows, y_true, true_is_f32, true_pitch, true_member_pitch, y_pred, pred_is_f32, pred_pitch, pred_member_pitch, stream) -> None:
        """One rr_metrics_update_members_dev of device rows at raw addresses, on `stream` (entered by the caller)."""
        e = self._engine
        need = e.metrics_members_work_bytes(self.n, self.members, rows)
        if self._work is None or self._work.nbytes < need:
            if self._work is not None:
                self._work.free()
            self._work = e.DeviceBuffer(need, self.device)
        e.metrics_update_members_dev(self.n, self.members, rows, y_true, true_is_f32, true_pitch, true_member_pitch, y_pred, pred_is_f32,
                                     pred_pitch, pred_member_pitch, self._cols_dev, self.skip_missing, self._state, self._work,
                                     self._work.nbytes, device=self.device, stream=stream)
        self.rows += rows

    _enter_stream = Accumulator._enter_stream

    def result(self) -> dict:
        """{'me', 'mae', 'mse', 'pearson_r', 'kge2012'} -> (members, n) scores of every row so far: device tensors if any update came
        as torch tensors, else numpy arrays.  With skip_missing also 'count', the pairs kept per member and column."""
        e, total, shape = self._engine, self.members * self.n, (self.members, self.n)
        if self._torch:
            import torch
            stream = torch.cuda.current_stream(self.device).cuda_stream
            self._enter_stream(stream)
            out = torch.empty((len(SCORES),) + shape, dtype=torch.float64, device=torch.device('cuda', self.device))
            e.metrics_finish_dev(total, self._state, out.data_ptr(), device=self.device, stream=stream)
            if self.skip_missing:
                # row 0 of the state, copied on the stream the finish was enqueued on
                count = torch.as_tensor(_DeviceDoubles(self._state.address, total), device=out.device).clone().reshape(shape)
        else:
            self._enter_stream(None)
            buf = e.DeviceBuffer(len(SCORES) * total * 8, self.device)
            e.metrics_finish_dev(total, self._state, buf, device=self.device)
            e.synchronize(self.device)
            out = buf.download(np.float64, (len(SCORES),) + shape)
            buf.free()
            if self.skip_missing:
                count = self._state.download(np.float64, shape)      # row 0 of the state
        res = {k: out[i] for i, k in enumerate(SCORES)}
        if self.skip_missing:
            res['count'] = count
        return res


class _MemberRows:
    """One input of a members update: (members, rows, cols) float32/float64 in device memory, rows `pitch` and members `member_pitch`
    elements apart -- or, where shared_ok, one (rows, cols) block for all members (members None, member_pitch 0).  numpy arrays are
    uploaded by to_device; torch tensors on the GPU are used in place where the kernel's addressing reads them as they are."""

    def __init__(self, a, name: str, shared_ok: bool = False):
        self.tensor, self.uploaded, self.device = None, None, None
        dims = '2-D (time, column) or 3-D (member, time, column)' if shared_ok else '3-D (member, time, column)'
        if _torch_tensor(a):
            import torch
            if a.device.type != 'cuda':
                raise ValueError(f'{name}: torch tensor must be on the GPU (got {a.device})')
            if a.dim() != 3 and not (shared_ok and a.dim() == 2):
                raise ValueError(f'{name} must be {dims}')
            if a.dtype not in (torch.float32, torch.float64):
                a = a.to(torch.float64)
            lead = a.dim() - 2
            self.members = int(a.shape[0]) if lead else None
            self.rows, self.cols = int(a.shape[lead]), int(a.shape[lead + 1])
            # the kernel reads element (m, r, c) at m * member_pitch + r * pitch + c: columns that are not adjacent, rows that share
            # elements and members that share elements (broadcast or overlapping views) are copied into whole blocks first
            pitch = int(a.stride(lead)) if self.rows > 1 else self.cols
            span = (self.rows - 1) * pitch + self.cols
            if ((self.cols > 1 and a.stride(lead + 1) != 1) or pitch < self.cols
                    or (lead and self.members > 1 and a.stride(0) < span)):
                a = a.contiguous()
                pitch = self.cols
                span = self.rows * self.cols
            self.tensor, self.device = a, a.device.index or 0
            self.is_f32 = a.dtype == torch.float32
            self.pitch = pitch
            self.member_pitch = 0 if not lead else (int(a.stride(0)) if self.members > 1 else span)
        else:
            a = np.asarray(a)
            if a.ndim != 3 and not (shared_ok and a.ndim == 2):
                raise ValueError(f'{name} must be {dims}')
            if a.dtype not in (np.float32, np.float64):
                a = a.astype(np.float64)
            self.host = np.ascontiguousarray(a)
            self.members = int(a.shape[0]) if a.ndim == 3 else None
            self.rows, self.cols = int(a.shape[-2]), int(a.shape[-1])
            self.is_f32 = a.dtype == np.float32
            self.pitch = self.cols
            self.member_pitch = self.rows * self.cols if a.ndim == 3 else 0

    to_device = _Rows.to_device
    address = _Rows.address
