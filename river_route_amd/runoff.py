"""
Gridded runoff -> catchment lateral inflow: the step immediately upstream of the routing hot path
(river_route/runoff.py:218-352).  Same function name, keyword arguments, order of
operations and units as the reference; the weights product, the cumulative difference, the clip, the NaN fill and
the area scaling run on the GPU (`rr_runoff_to_qlateral`, river_route_amd/csrc/rr_kernels_runoff.hpp:
k_runoff_to_qlateral), the index bookkeeping (pandas) and the rare irregular-time-step resampling stay on the host
exactly as the reference does them.

The weight table that path reads is made here too (river_route/runoff.py:25-191): `grid_weights` restates the reference's
Voronoi overlay for a regular lon/lat grid, whose Voronoi cells are axis-aligned rectangles.  The catchment polygons are
clipped to their candidate cells and measured in the cylindrical equal-area projection on the GPU
(`rr_grid_overlap_area`, csrc/rr_kernels_overlap.hpp: k_overlap_area); cells, WKB decoding, candidate ranges and the
table's pandas steps stay on the host.

The reference returns an xarray Dataset; xarray is not a dependency of this package, so the result is a small
`QlateralDataset` with the same names: `ds['qlateral'].values` (time, river_id), `ds['time'].values`,
`ds['river_id'].values`, `ds.attrs`, `'qlateral' in ds`, `ds.dims`.
"""
from __future__ import annotations

import logging
import struct
from dataclasses import dataclass, field

import numpy as np

from . import engine
from .io import _decode_cf_time, read_variables

__all__ = ['runoff_to_qlateral', 'QlateralDataset', 'RunoffSource', 'prepare_runoff', 'cell_xy_from_regular_grid', 'grid_weights',
           'catchment_cell_areas']

logger = logging.getLogger(__name__)


@dataclass
class _Var:
    values: np.ndarray
    dims: tuple
    attrs: dict = field(default_factory=dict)


class QlateralDataset:
    """The three variables runoff_to_qlateral returns (river_route/runoff.py:343-352), by name."""

    def __init__(self, time, river_id, qlateral, units, long_name, timestep, attrs):
        self._vars = {
            'time': _Var(time, ('time',), {'long_name': 'time', 'standard_name': 'time', 'axis': 'T', 'time_step': f'{timestep}'}),
            'river_id': _Var(river_id, ('river_id',), {'long_name': 'unique ID number for each river'}),
            'qlateral': _Var(qlateral, ('time', 'river_id'), {'units': units, 'long_name': long_name}),
        }
        self.dims = {'time': time.shape[0], 'river_id': river_id.shape[0]}
        self.attrs = attrs

    def __getitem__(self, name):
        return self._vars[name]

    def __contains__(self, name):
        return name in self._vars


def _get_conversion_factor(unit):
    """river_route/runoff.py:206-215."""
    if unit is None:
        logger.warning('No units attribute found. Assuming meters')
        return 1
    if unit in ('m', 'meters', 'kg m-2'):
        return 1
    if unit in ('mm', 'millimeters'):
        return .001
    raise ValueError(f'Unknown units: {unit}')


def _read_runoff_points(paths, var_runoff, var_x, var_y, var_t, x_index, y_index):
    """(T, points) block of the runoff variable at the (x, y) index pairs, concatenated over the files in time
    order, its `units` attribute and the time axis (runoff.py:266-279: open_mfdataset + isel + transpose)."""
    blocks, times, units = [], [], None
    for path in paths:
        got = read_variables(path, [var_runoff, var_t])
        arr, dims, attrs = got[var_runoff]
        for d in (var_t, var_x, var_y):
            if d not in dims:
                raise KeyError(f'{var_runoff} in {path} has no dimension {d!r} (has {dims})')
        arr = np.moveaxis(arr, [dims.index(var_t), dims.index(var_y), dims.index(var_x)], [0, 1, 2])
        if arr.ndim != 3:
            raise ValueError(f'{var_runoff} in {path} must have exactly the dimensions ({var_t}, {var_y}, {var_x})')
        blocks.append(arr[:, y_index, x_index])
        units = units if units is not None else attrs.get('units')
        tv, _, tattrs = got[var_t]
        if np.issubdtype(tv.dtype, np.datetime64):
            times.append(tv.astype('datetime64[s]'))
        else:
            times.append(_decode_cf_time(tv, tattrs.get('units', 'seconds since 1970-01-01')))
    time_index = np.concatenate(times)
    block = np.concatenate(blocks, axis=0)
    if len(paths) > 1:
        order = np.argsort(time_index, kind='stable')      # open_mfdataset combines by coordinates
        time_index, block = time_index[order], block[order]
    return block, units, time_index


@dataclass
class RunoffSource:
    """Everything rr_runoff_to_qlateral needs for one set of runoff files, before any arithmetic of the path: the
    (time, points) runoff block, the CSR weights (proportion x unit conversion, duplicates summed, ascending point order
    as the reference's csr_matrix), catchment areas, flags, the time axis and the river ids in column order.  The routers
    upload it as it is, so that the catchment inflow is computed on the GPU and routed from there without a trip through host
    memory (routers/_device.py: _runoff_forms; rr_rapid_route_runoff_dev takes the same pieces and computes the inflow
    on the way into the engine's records); `to_array()` is the reference's (time, river) array."""
    runoff_tp: np.ndarray
    indptr: np.ndarray
    indices: np.ndarray
    weights: np.ndarray
    area: np.ndarray
    flags: int
    time_index: np.ndarray
    river_ids: np.ndarray
    irregular: bool
    device: int = 0

    def point_major(self):
        """(points, padded time) copy of the block, rows padded to whole 16-step chunks, float32 or float64 as read."""
        block = self.runoff_tp if self.runoff_tp.dtype in (np.float32, np.float64) else self.runoff_tp.astype(np.float64)
        T, n_points = block.shape
        t_pad = -(-T // 16) * 16
        out = np.zeros((n_points, t_pad), dtype=block.dtype)
        out[:, :T] = block.T
        return out

    def to_array(self, as_volumes: bool, keep_nan: bool = False) -> np.ndarray:
        return engine.runoff_to_qlateral(self.indptr, self.indices, self.weights, self.runoff_tp, self.area if as_volumes else None,
                                         self.flags | (engine.RUNOFF_KEEP_NAN if keep_nan else 0), self.device)


def prepare_runoff(runoff_data, grid_weights_file, *, var_runoff: str = 'ro', var_x: str = 'lon', var_y: str = 'lat', var_t: str = 'time',
                   var_river_id: str = 'river_id', runoff_depth_unit: str | None = None, cumulative: bool = False,
                   force_positive_runoff: bool = False, force_uniform_timesteps: bool = True, device: int = 0) -> RunoffSource:
    """File reading and index bookkeeping of runoff_to_qlateral (river_route/runoff.py:255-298), no arithmetic of the path."""
    import pandas as pd
    import scipy.sparse

    cols = [var_river_id, 'x_index', 'y_index', 'proportion', 'area_sqm']
    table = read_variables(grid_weights_file, cols)
    weight_df = pd.DataFrame({c: np.asarray(table[c][0]).ravel() for c in cols})
    unique_indexes = (weight_df[['x_index', 'y_index']].drop_duplicates().reset_index(drop=True).reset_index().astype(int))
    river_ids_ordered = weight_df[var_river_id].drop_duplicates().to_numpy()     # index already topologically sorted

    paths = [runoff_data] if isinstance(runoff_data, (str, bytes)) or hasattr(runoff_data, '__fspath__') else list(runoff_data)
    runoff_raw, file_units, time_index = _read_runoff_points(
        paths, var_runoff, var_x, var_y, var_t, unique_indexes['x_index'].to_numpy(), unique_indexes['y_index'].to_numpy())
    conversion_factor = _get_conversion_factor(runoff_depth_unit or (file_units if file_units is not None else 'm'))

    # sparse weights (n_rivers, n_unique_points), built the way the reference builds them so that duplicate entries
    # are summed and the terms of a row are stored in the same (ascending point) order
    point_idx = weight_df[['x_index', 'y_index']].merge(unique_indexes, on=['x_index', 'y_index'], how='left')['index'].to_numpy()
    river_id_to_row = pd.Series(np.arange(len(river_ids_ordered)), index=river_ids_ordered)
    river_idx = river_id_to_row.loc[weight_df[var_river_id].to_numpy()].to_numpy()
    weights = scipy.sparse.csr_matrix((weight_df['proportion'].to_numpy() * conversion_factor, (river_idx, point_idx)),
                                      shape=(len(river_ids_ordered), len(unique_indexes)))
    weights.sum_duplicates()
    catchment_area = weight_df.groupby(var_river_id)['area_sqm'].sum().reindex(river_ids_ordered).to_numpy()

    time_diff = np.diff(time_index)
    irregular = bool(time_index.shape[0] > 2 and not np.all(time_diff == time_index[1] - time_index[0]) and force_uniform_timesteps)
    flags = (engine.RUNOFF_CUMULATIVE if cumulative else 0) | (engine.RUNOFF_FORCE_POSITIVE if force_positive_runoff else 0)
    return RunoffSource(runoff_raw, weights.indptr.astype(np.int32), weights.indices.astype(np.int32), np.ascontiguousarray(weights.data, dtype=np.float64),
                        np.ascontiguousarray(catchment_area, dtype=np.float64), flags, time_index, river_ids_ordered.astype(np.int64, copy=False),
                        irregular, device)


def runoff_to_qlateral(runoff_data, grid_weights_file, *, var_runoff: str = 'ro', var_x: str = 'lon', var_y: str = 'lat',
                       var_t: str = 'time', var_river_id: str = 'river_id', runoff_depth_unit: str | None = None,
                       cumulative: bool = False, force_positive_runoff: bool = False,
                       force_uniform_timesteps: bool = True, as_volumes: bool = False, device: int = 0) -> QlateralDataset:
    """Area-weighted aggregation of gridded runoff depths to per-catchment lateral inflow (depths in m, or volumes
    in m3 with `as_volumes`), river_route/runoff.py:218-352.  `device` (HIP ordinal) is the only extra argument."""
    import pandas as pd
    src = prepare_runoff(runoff_data, grid_weights_file, var_runoff=var_runoff, var_x=var_x, var_y=var_y, var_t=var_t,
                         var_river_id=var_river_id, runoff_depth_unit=runoff_depth_unit, cumulative=cumulative,
                         force_positive_runoff=force_positive_runoff, force_uniform_timesteps=force_uniform_timesteps, device=device)
    time_index, river_ids_ordered, catchment_area = src.time_index, src.river_ids, src.area
    if not src.irregular:
        qlateral = src.to_array(as_volumes)
    else:
        # runoff.py:311-330: the resampling sits between the clip and the NaN fill, so the device stops before the fill
        qlateral = src.to_array(False, keep_nan=True)
        timestep = int((time_index[1] - time_index[0]) / np.timedelta64(1, 's'))
        logger.warning(f'Time steps are not uniform, resampling to the first timestep: {timestep} seconds')
        df = pd.DataFrame(qlateral, index=time_index, columns=river_ids_ordered)
        df = df.cumsum().resample(rule=f'{timestep}s').interpolate(method='linear')
        df = pd.concat([df.iloc[[0]], df.diff().iloc[1:]])
        time_index = df.index.values.astype('datetime64[s]')
        qlateral = df.to_numpy(dtype=np.float64)
        qlateral[np.isnan(qlateral)] = 0.0
        if as_volumes:
            qlateral *= catchment_area[np.newaxis, :]

    units, long_name = ('m3', 'Incremental qlateral volumes') if as_volumes else ('m', 'Incremental qlateral depths')
    start_date = pd.Timestamp(time_index[0]).strftime('%Y%m%d%H')
    end_date = pd.Timestamp(time_index[-1]).strftime('%Y%m%d%H')
    timestep = int((time_index[1] - time_index[0]) / np.timedelta64(1, 's')) if len(time_index) > 1 else 0
    attrs = {'title': f'Incremental qlateral {long_name.split()[-1]}',
             'description': f'Incremental qlateral ({units}) for each river', 'source': 'river_route_amd',
             'history': f'Created on {pd.Timestamp.now().strftime("%Y-%m-%d %H:%M:%S")}',
             'start_date': start_date, 'end_date': end_date}
    return QlateralDataset(time_index.astype('datetime64[s]'), river_ids_ordered.astype(np.int64, copy=False), qlateral, units,
                           long_name, timestep, attrs)


# ---- grid weights: catchment / grid-cell overlap (river_route/runoff.py:25-191) ----

# A (catchment, cell) piece whose area is at most this share of its cell's area is dropped.  The reference's overlay keeps
# only polygonal pieces (GEOS drops the line and point intersections of catchments that merely touch a cell); measured
# areas of such contacts are roundoff, a few ulps of the cell's projected coordinates, which this threshold absorbs.
DROP_SHARE = 1e-9

_CEA_A = 6378137.0                            # PROJ's default ellipsoid, GRS80 (csrc/rr_kernels_overlap.hpp: cea_y)
_CEA_F = 1.0 / 298.257222101
_CEA_ES = 2.0 * _CEA_F - _CEA_F * _CEA_F
_CEA_X_PER_DEG = _CEA_A * 0.017453292519943295


def _cea_y(lat_deg):
    """Northing of +proj=cea (GRS80, lat_ts 0) in metres, numpy form of the kernel's cea_y (PROJ's pj_qsfn)."""
    e = np.sqrt(_CEA_ES)
    s = np.sin(np.asarray(lat_deg, dtype=np.float64) * 0.017453292519943295)
    con = e * s
    return 0.5 * _CEA_A * (1.0 - _CEA_ES) * (s / (1.0 - con * con) - (0.5 / e) * np.log((1.0 - con) / (1.0 + con)))


def cell_xy_from_regular_grid(dataset, x_var: str = 'lon', y_var: str = 'lat'):
    """Cell centre x and y coordinates of a regular grid file (river_route/runoff.py:25-39)."""
    out = []
    for name in (x_var, y_var):
        try:
            out.append(np.asarray(read_variables(dataset, [name])[name][0]))
        except (KeyError, IndexError):
            raise KeyError(f'{name} must be a variable in {dataset}') from None
    x, y = out
    if x.ndim != 1 or y.ndim != 1:
        raise ValueError('Regular grid requires 1D x/y coordinate arrays')
    return x, y


def _voronoi_clip_margin(x_lo, x_hi, y_lo, y_hi):
    """How far the outermost cells reach past the outermost centres.  The reference's cells come from GEOS's
    VoronoiDiagramBuilder, which clips the diagram to the sites' bounding box grown on every side by
    max(width, height); that is this rule, from GEOS's documented behaviour, not checked against GEOS here.  It only matters
    for catchments that reach beyond the grid's outermost centres."""
    return max(x_hi - x_lo, y_hi - y_lo)


def _nearest_index(values, targets):
    """np.argmin(np.abs(values - t)) for every t (the first of equal distances), without the len(values) x len(targets) array."""
    order = np.argsort(values, kind='stable')
    sv = values[order]
    pos = np.searchsorted(sv, targets)
    lo, hi = np.clip(pos - 1, 0, sv.size - 1), np.clip(pos, 0, sv.size - 1)
    d_lo, d_hi = np.abs(sv[lo] - targets), np.abs(sv[hi] - targets)
    pick = np.where(d_hi < d_lo, order[hi], np.where(d_lo < d_hi, order[lo], np.minimum(order[lo], order[hi])))
    return pick.astype(np.int64)


@dataclass
class _Cells:
    """Voronoi cells of a regular grid as rectangles, in sorted (ascending) order along each axis."""
    x_bounds: np.ndarray        # (nx + 1,) ascending, longitudes in -180..180
    y_bounds: np.ndarray        # (ny + 1,) ascending
    x: np.ndarray               # (nx,) centroid of each sorted column (the boundary midpoint)
    y: np.ndarray               # (ny,) centroid of each sorted row
    x_index: np.ndarray         # (nx,) index into the file's x of each sorted column
    y_index: np.ndarray         # (ny,) index into the file's y of each sorted row


def _regular_cells(x, y) -> _Cells:
    """The cells grid_weights + voronoi_diagram_from_regular_xy make (river_route/runoff.py:42-67, 146-156): x above 180
    less 360, cell boundaries halfway between neighbouring centres, outer cells out to the clip envelope; x / y are cell
    centroids, x_index is argmin |x_sorted - centroid| mapped back through the sort, y_index is argmin |y - centroid| on y
    as the file stores it."""
    x = np.asarray(x, dtype=np.float64).ravel()
    y = np.asarray(y, dtype=np.float64).ravel()
    if x.size < 2 or y.size < 2:
        raise ValueError('a regular grid needs at least two cell centres along each axis')
    x_geo = x.copy()
    x_geo[x_geo > 180] -= 360
    sort_order = np.argsort(x_geo)
    xs = x_geo[sort_order]
    ys = np.sort(y)
    if np.any(np.diff(xs) == 0) or np.any(np.diff(ys) == 0):
        raise ValueError('a regular grid needs distinct cell centres (after moving x above 180 to x - 360)')
    e = _voronoi_clip_margin(xs[0], xs[-1], ys[0], ys[-1])
    xb = np.concatenate([[xs[0] - e], 0.5 * (xs[:-1] + xs[1:]), [xs[-1] + e]])
    yb = np.concatenate([[ys[0] - e], 0.5 * (ys[:-1] + ys[1:]), [ys[-1] + e]])
    xc, yc = 0.5 * (xb[:-1] + xb[1:]), 0.5 * (yb[:-1] + yb[1:])
    return _Cells(xb, yb, xc, yc, sort_order[_nearest_index(xs, xc)].astype(np.int64), _nearest_index(y, yc))


_WKB_POLYGON, _WKB_MULTIPOLYGON = 3, 6


def _wkb_header(buf, pos, row):
    """-> (byte order '<' / '>', base type, ordinates per vertex, position after the header) of the geometry at pos."""
    if pos >= len(buf) or buf[pos] not in (0, 1):
        raise ValueError(f'geometry of row {row}: not WKB (byte-order flag {buf[pos] if pos < len(buf) else None!r})')
    end = '<' if buf[pos] == 1 else '>'
    (code,) = struct.unpack_from(end + 'I', buf, pos + 1)
    pos += 5
    z, m = bool(code & 0x80000000), bool(code & 0x40000000)          # EWKB flags
    if code & 0x20000000:                                              # EWKB SRID: skipped
        pos += 4
    code &= 0x0FFFFFFF
    iso = code // 1000                                                 # ISO: +1000 Z, +2000 M, +3000 ZM
    z, m = z or iso in (1, 3), m or iso in (2, 3)
    return end, code % 1000, 2 + z + m, pos


def _decode_wkb(geometries):
    """WKB Polygon / MultiPolygon rows (either byte order, ISO or EWKB Z / M, EWKB SRID) -> flat arrays: lon, lat (float64),
    ring_offsets (int64, n_rings + 1), ring_row (int64: the row of each ring), ring_exterior (bool).  Extra ordinates are
    dropped.  Any other type raises ValueError naming the row."""
    lons, lats, lengths, ring_row, ring_ext = [], [], [], [], []

    def polygon(buf, pos, end, dims, row):
        (n_rings,) = struct.unpack_from(end + 'I', buf, pos)
        pos += 4
        dt = np.dtype(end + 'f8')
        for k in range(n_rings):
            (n_pts,) = struct.unpack_from(end + 'I', buf, pos)
            xy = np.frombuffer(buf, dtype=dt, count=n_pts * dims, offset=pos + 4).reshape(n_pts, dims)
            lons.append(xy[:, 0])
            lats.append(xy[:, 1])
            lengths.append(n_pts)
            ring_row.append(row)
            ring_ext.append(k == 0)
            pos += 4 + 8 * n_pts * dims
        return pos

    names = {1: 'Point', 2: 'LineString', 4: 'MultiPoint', 5: 'MultiLineString', 7: 'GeometryCollection'}
    for row, geom in enumerate(geometries):
        buf = bytes(geom) if not isinstance(geom, bytes) else geom
        end, kind, dims, pos = _wkb_header(buf, 0, row)
        if kind == _WKB_POLYGON:
            polygon(buf, pos, end, dims, row)
        elif kind == _WKB_MULTIPOLYGON:
            (n_parts,) = struct.unpack_from(end + 'I', buf, pos)
            pos += 4
            for _ in range(n_parts):
                pend, pkind, pdims, pos = _wkb_header(buf, pos, row)
                if pkind != _WKB_POLYGON:
                    raise ValueError(f'geometry of row {row}: a MultiPolygon part is WKB type {pkind} ({names.get(pkind, "unknown")}), not Polygon')
                pos = polygon(buf, pos, pend, pdims, row)
        else:
            raise ValueError(f'geometry of row {row}: WKB type {kind} ({names.get(kind, "unknown")}) is not Polygon or MultiPolygon')
    lon = np.concatenate(lons).astype(np.float64, copy=False) if lons else np.zeros(0)
    lat = np.concatenate(lats).astype(np.float64, copy=False) if lats else np.zeros(0)
    ring_offsets = np.zeros(len(lengths) + 1, dtype=np.int64)
    np.cumsum(lengths, out=ring_offsets[1:])
    return (np.ascontiguousarray(lon), np.ascontiguousarray(lat), ring_offsets, np.asarray(ring_row, dtype=np.int64),
            np.asarray(ring_ext, dtype=bool))


def _ring_weights(lon, lat, ring_offsets, ring_exterior):
    """+1 / -1 per ring so that exteriors add and holes subtract whatever their orientation: role x sign of the ring's
    signed (lon/lat shoelace, counter-clockwise positive) area; 0 for rings without area."""
    n_rings = ring_offsets.shape[0] - 1
    counts = np.diff(ring_offsets)
    full = counts > 0
    area = np.zeros(n_rings)
    if lon.size:
        start = np.repeat(ring_offsets[:-1], counts)
        nxt = np.arange(lon.size, dtype=np.int64) + 1
        nxt[ring_offsets[1:][full] - 1] = ring_offsets[:-1][full]
        x, y = lon - lon[start], lat - lat[start]            # relative to the ring's first vertex: no cancellation
        cross = x * y[nxt] - x[nxt] * y
        area[full] = np.add.reduceat(cross, ring_offsets[:-1][full])
    return np.where(ring_exterior, 1.0, -1.0) * np.sign(area)


def _candidate_cells(lon, lat, ring_offsets, ring_row, n_rows, cells: _Cells):
    """Each row's block of cells its bounding box overlaps: row_cells (n_rows, 3) = first sorted column, first sorted row,
    rows in the block; pair_offsets (n_rows + 1) by prefix sum; row_rings (n_rows + 1)."""
    nx, ny = cells.x_bounds.size - 1, cells.y_bounds.size - 1
    row_rings = np.zeros(n_rows + 1, dtype=np.int64)
    np.cumsum(np.bincount(ring_row, minlength=n_rows), out=row_rings[1:])
    v_start = ring_offsets[row_rings]
    has = v_start[1:] > v_start[:-1]
    lo_x, hi_x, lo_y, hi_y = (np.zeros(n_rows) for _ in range(4))
    if has.any():
        starts = v_start[:-1][has]
        lo_x[has], hi_x[has] = np.minimum.reduceat(lon, starts), np.maximum.reduceat(lon, starts)
        lo_y[has], hi_y[has] = np.minimum.reduceat(lat, starts), np.maximum.reduceat(lat, starts)

    def span(b, lo, hi, n):
        first = np.clip(np.searchsorted(b, lo, side='right') - 1, 0, n - 1)
        last = np.clip(np.searchsorted(b, hi, side='left') - 1, 0, n - 1)
        ok = has & (hi > b[0]) & (lo < b[-1]) & (hi > lo)
        return first, np.where(ok, last - first + 1, 0).clip(min=0)

    ix0, cnx = span(cells.x_bounds, lo_x, hi_x, nx)
    iy0, cny = span(cells.y_bounds, lo_y, hi_y, ny)
    n_pairs = cnx.astype(np.int64) * cny
    if n_pairs.size and n_pairs.max() >= 2 ** 31:
        raise ValueError('a catchment spans more than 2^31 grid cells')
    pair_offsets = np.zeros(n_rows + 1, dtype=np.int64)
    np.cumsum(n_pairs, out=pair_offsets[1:])
    row_cells = np.stack([ix0, iy0, np.maximum(cny, 1)], axis=1).astype(np.int32)
    return row_rings, row_cells, pair_offsets


def _pairs_table(river_ids, area, row_cells, pair_offsets, cells: _Cells, id_name: str):
    """Kernel output -> the reference's table (river_route/runoff.py:86-104): slivers dropped, pieces of the same
    (river, cell) summed, sorted by river then area (largest first; ties keep (x_index, y_index) order), proportions."""
    import pandas as pd
    counts = np.diff(pair_offsets)
    row = np.repeat(np.arange(counts.size), counts)
    k = np.arange(area.size, dtype=np.int64) - pair_offsets[:-1][row]
    ny_r = row_cells[row, 2].astype(np.int64)
    ix = row_cells[row, 0] + k // ny_r
    iy = row_cells[row, 1] + k % ny_r
    yb = _cea_y(np.clip(cells.y_bounds, -90.0, 90.0))
    cell_area = np.diff(cells.x_bounds)[ix] * _CEA_X_PER_DEG * np.diff(yb)[iy]
    keep = area > DROP_SHARE * cell_area
    row, ix, iy = row[keep], ix[keep], iy[keep]
    df = pd.DataFrame({id_name: np.asarray(river_ids)[row], 'x_index': cells.x_index[ix], 'y_index': cells.y_index[iy],
                       'x': cells.x[ix], 'y': cells.y[iy], 'area_sqm': area[keep]})
    df = (df.groupby([id_name, 'x_index', 'y_index', 'x', 'y'], as_index=False)
          .agg({'area_sqm': 'sum'})
          .sort_values([id_name, 'area_sqm'], ascending=[True, False], kind='stable')
          .reset_index(drop=True))
    total = df[[id_name, 'area_sqm']].groupby(id_name).sum().rename(columns={'area_sqm': 'area_sqm_total'})
    df = df.merge(total, left_on=id_name, right_index=True, how='left')
    df['proportion'] = df['area_sqm'] / df['area_sqm_total']
    return df[[id_name, 'x_index', 'y_index', 'x', 'y', 'area_sqm', 'proportion']]


def _cell_areas(x, y, river_ids, geometries, device, id_name):
    cells = _regular_cells(x, y)
    river_ids = np.asarray(river_ids)
    n_rows = river_ids.shape[0]
    if len(geometries) != n_rows:
        raise ValueError(f'{n_rows} river ids but {len(geometries)} geometries')
    lon, lat, ring_offsets, ring_row, ring_ext = _decode_wkb(geometries)
    weight = _ring_weights(lon, lat, ring_offsets, ring_ext)
    row_rings, row_cells, pair_offsets = _candidate_cells(lon, lat, ring_offsets, ring_row, n_rows, cells)
    area = engine.grid_overlap_area(row_rings, ring_offsets, weight, lon, lat, cells.x_bounds, cells.y_bounds, row_cells,
                                    pair_offsets, device)
    return _pairs_table(river_ids, area, row_cells, pair_offsets, cells, id_name)


def catchment_cell_areas(x, y, river_ids, geometries, device: int = 0):
    """The weight table of grid_weights from arrays: x, y the grid's 1-D cell centres (as a file stores them), river_ids one
    per geometry, geometries a sequence of WKB bytes (Polygon / MultiPolygon, lon/lat degrees).  -> DataFrame with columns
    ['river_id', 'x_index', 'y_index', 'x', 'y', 'area_sqm', 'proportion'], in the reference's order."""
    return _cell_areas(x, y, river_ids, geometries, device, 'river_id')


def _write_weights(path, df, attrs):
    """The weight table as NetCDF, one dimension `index` (what xarray's DataFrame.to_xarray().to_netcdf() writes), with
    io.write_discharge's fallbacks: netCDF4 when installed, else NetCDF-3 through scipy (integers as i4, range-checked)."""
    int_cols = [c for c in df.columns if np.issubdtype(df[c].dtype, np.integer)]
    columns = {'index': np.arange(len(df), dtype=np.int64), **{c: df[c].to_numpy() for c in df.columns}}
    try:
        import netCDF4 as nc
        with nc.Dataset(str(path), mode='w', format='NETCDF4') as ds:
            ds.createDimension('index', size=len(df))
            for name, values in columns.items():
                kind = 'i8' if name == 'index' or name in int_cols else 'f8'
                ds.createVariable(name, kind, ('index',))[:] = values
            ds.setncatts(attrs)
        return
    except ImportError:
        pass
    from scipy.io import netcdf_file
    for name, values in columns.items():
        if (name == 'index' or name in int_cols) and values.size and (values.min() < -2 ** 31 or values.max() >= 2 ** 31):
            raise ValueError(f'{name} holds values outside the 32-bit range NetCDF-3 integers can store; install netCDF4')
    with netcdf_file(str(path), 'w', version=2) as ds:
        ds.createDimension('index', len(df))
        for name, values in columns.items():
            is_int = name == 'index' or name in int_cols
            v = ds.createVariable(name, 'i4' if is_int else 'f8', ('index',))
            v[:] = values.astype(np.int32 if is_int else np.float64)
        for k, v in attrs.items():
            setattr(ds, k, v)


def grid_weights(grid_path, catchments_path, *, var_x: str = 'lon', var_y: str = 'lat', var_river_id: str = 'river_id',
                 crs: int = 4326, save_voronoi_path=None, save_weights_path=None, routing_params_path=None, device: int = 0):
    """Grid weights of a regular lon/lat grid file and a catchments (Geo)Parquet file (river_route/runoff.py:119-191): the
    area of each catchment in each grid cell (cylindrical equal-area m^2) and its share of the catchment.  Returns a
    DataFrame with columns [var_river_id, 'x_index', 'y_index', 'x', 'y', 'area_sqm', 'proportion'] in the reference's row
    order; `device` (HIP ordinal) is the only extra argument.  Only crs=4326 is supported, and save_voronoi_path (a
    GeoParquet of the cells) is not."""
    import pandas as pd
    from . import __version__
    if crs != 4326:
        raise ValueError(f'grid_weights: only crs=4326 (lon/lat degrees) is supported, got {crs!r}')
    if save_voronoi_path:
        raise ValueError('grid_weights: save_voronoi_path (GeoParquet of the Voronoi cells) is not supported')
    x, y = cell_xy_from_regular_grid(grid_path, x_var=var_x, y_var=var_y)
    catchments = pd.read_parquet(catchments_path)
    if var_river_id not in catchments.columns:
        raise KeyError(f'catchments_gdf must contain a {var_river_id} column')
    if 'geometry' not in catchments.columns:
        raise KeyError(f'{catchments_path} has no geometry column')
    df = _cell_areas(x, y, catchments[var_river_id].to_numpy(), catchments['geometry'].to_numpy(), device, var_river_id)

    if routing_params_path is not None:
        ordered_ids = pd.read_parquet(routing_params_path)[var_river_id].to_numpy()
        id_to_order = {int(rid): i for i, rid in enumerate(ordered_ids)}
        df = (df.assign(_sort_key=df[var_river_id].map(id_to_order))
              .sort_values(['_sort_key', 'area_sqm'], ascending=[True, False])
              .drop(columns='_sort_key')
              .reset_index(drop=True))
    else:
        logger.warning('routing_params_path not provided; weight table row order may not match routing network order')

    if save_weights_path:
        _write_weights(save_weights_path, df, {'description': 'proportions of runoff cells that intersect river catchments',
                                               'grid_path': str(grid_path), 'catchments_path': str(catchments_path),
                                               'river_route_version': __version__})
    return df
