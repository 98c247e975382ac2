"""rr.runoff.grid_weights host side (no GPU): WKB decoding, the grid's cells, cell_xy_from_regular_grid, and the table's
pandas steps on canned areas (river_route/runoff.py:25-191)."""
import logging
import struct

import numpy as np
import pandas as pd
import pytest

from river_route_amd import runoff


def wkb_polygon(rings, end='<', dims=2, iso=False, srid=None, header=True):
    """WKB Polygon of (n, 2) rings; dims 3 adds a Z ordinate (ISO +1000 or EWKB flag), srid an EWKB SRID prefix."""
    code = 3
    if dims == 3:
        code = code + 1000 if iso else code | 0x80000000
    if srid is not None:
        code |= 0x20000000
    out = (bytes([1 if end == '<' else 0]) + struct.pack(end + 'I', code)) if header else b''
    if srid is not None:
        out += struct.pack(end + 'I', srid)
    out += struct.pack(end + 'I', len(rings))
    for ring in rings:
        ring = np.asarray(ring, dtype=np.float64)
        if dims == 3:
            ring = np.column_stack([ring, np.full(len(ring), 7.0)])
        out += struct.pack(end + 'I', len(ring)) + ring.astype(end + 'f8').tobytes()
    return out


def wkb_multipolygon(polys, end='<'):
    out = bytes([1 if end == '<' else 0]) + struct.pack(end + 'I', 6) + struct.pack(end + 'I', len(polys))
    return out + b''.join(wkb_polygon(p, end=end) for p in polys)


SQUARE = [(0, 0), (1, 0), (1, 1), (0, 1), (0, 0)]
HOLE = [(0.2, 0.2), (0.2, 0.4), (0.4, 0.4), (0.4, 0.2), (0.2, 0.2)]


def test_wkb_polygon_with_hole_and_multipolygon():
    geoms = [wkb_polygon([SQUARE, HOLE]), wkb_multipolygon([[SQUARE], [np.add(SQUARE, 5)]])]
    lon, lat, ro, ring_row, ext = runoff._decode_wkb(geoms)
    assert ro.tolist() == [0, 5, 10, 15, 20]
    assert ring_row.tolist() == [0, 0, 1, 1]
    assert ext.tolist() == [True, False, True, True]
    np.testing.assert_array_equal(lon[:5], [0, 1, 1, 0, 0])
    np.testing.assert_array_equal(lat[15:20], [5, 5, 6, 6, 5])
    w = runoff._ring_weights(lon, lat, ro, ext)
    # weight x signed area: the CCW exterior adds (+1 x +), the CW hole subtracts (+1 x -)
    assert w.tolist() == [1.0, 1.0, 1.0, 1.0]


def test_wkb_orientation_does_not_matter():
    cw = SQUARE[::-1]
    lon, lat, ro, _, ext = runoff._decode_wkb([wkb_polygon([cw, HOLE[::-1]])])
    # a CW exterior (-1 x -) still adds, a CCW hole (-1 x +) still subtracts
    assert runoff._ring_weights(lon, lat, ro, ext).tolist() == [-1.0, -1.0]


@pytest.mark.parametrize('kw', [dict(end='>'), dict(dims=3, iso=True), dict(dims=3, srid=4326), dict(end='>', dims=3, srid=4326)])
def test_wkb_variants_decode_the_same(kw):
    ref = runoff._decode_wkb([wkb_polygon([SQUARE, HOLE])])
    got = runoff._decode_wkb([wkb_polygon([SQUARE, HOLE], **kw)])
    for a, b in zip(ref, got):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize('code,name', [(1, 'Point'), (2, 'LineString')])
def test_wkb_rejects_other_types_naming_the_row(code, name):
    bad = bytes([1]) + struct.pack('<I', code) + struct.pack('<dd', 1.0, 2.0)
    with pytest.raises(ValueError, match=rf'row 1\b.*{name}'):
        runoff._decode_wkb([wkb_polygon([SQUARE]), bad])


def test_cells_uniform_grid():
    x, y = np.arange(0.0, 4.0), np.arange(10.0, 13.0)
    c = runoff._regular_cells(x, y)
    e = 3.0                                                  # max(width 3, height 2)
    np.testing.assert_array_equal(c.x_bounds, [-e, 0.5, 1.5, 2.5, 3 + e])
    np.testing.assert_array_equal(c.y_bounds, [10 - e, 10.5, 11.5, 12 + e])
    np.testing.assert_array_equal(c.x, [(-e + 0.5) / 2, 1.0, 2.0, (2.5 + 3 + e) / 2])     # centroids, not centres
    np.testing.assert_array_equal(c.x_index, [0, 1, 2, 3])
    np.testing.assert_array_equal(c.y_index, [0, 1, 2])


def test_cells_nonuniform_0_360_and_descending_latitude():
    x = np.array([0.0, 90.0, 180.0, 270.0])          # 270 -> -90
    y = np.array([60.0, 30.0, 20.0, -10.0])          # descending, uneven
    c = runoff._regular_cells(x, y)
    e = max(270.0, 70.0)
    np.testing.assert_array_equal(c.x_bounds, [-90 - e, -45, 45, 135, 180 + e])
    np.testing.assert_array_equal(c.y_bounds, [-10 - e, 5, 25, 45, 60 + e])
    # sorted columns are -90, 0, 90, 180: file indices 3, 0, 1, 2
    np.testing.assert_array_equal(c.x_index, [3, 0, 1, 2])
    # sorted rows -10, 20, 30, 60 are file rows 3, 2, 1, 0; centroid of row 20 is 15 -> nearest 20; row 30's is 35 -> 30
    np.testing.assert_array_equal(c.y, [(-10 - e + 5) / 2, 15.0, 35.0, (45 + 60 + e) / 2])
    np.testing.assert_array_equal(c.y_index, [3, 2, 1, 0])


def test_cells_argmin_follows_centroid_not_centre():
    # uneven spacing: the centroid of the middle column (between 0.5 and 5) is 2.75, nearest centre 1 -- but of the third
    # column (between 5 and 9.5+e) it lies beyond 9 and still maps to 9; argmin ties go to the first index
    x = np.array([0.0, 1.0, 9.0])
    y = np.array([0.0, 1.0])
    c = runoff._regular_cells(x, y)
    np.testing.assert_array_equal(c.x, [(-9 + 0.5) / 2, 2.75, (5 + 18) / 2])
    np.testing.assert_array_equal(c.x_index, [0, 1, 2])
    assert runoff._nearest_index(np.array([0.0, 2.0]), np.array([1.0])).tolist() == [0]
    assert runoff._nearest_index(np.array([2.0, 0.0]), np.array([1.0])).tolist() == [0]


@pytest.mark.parametrize('x,y', [([0.0], [0.0, 1.0]), ([0.0, 1.0], [5.0]), ([0.0, 360.0], [0.0, 1.0]), ([0.0, 1.0], [2.0, 2.0])])
def test_cells_reject_short_or_repeated_axes(x, y):
    with pytest.raises(ValueError):
        runoff._regular_cells(np.array(x), np.array(y))


def test_candidate_cells_cover_the_bounding_box():
    c = runoff._regular_cells(np.arange(0.0, 10.0), np.arange(0.0, 5.0))
    geoms = [wkb_polygon([[(1.2, 1.2), (3.7, 1.2), (3.7, 2.1), (1.2, 1.2)]]), wkb_polygon([[(50, 50), (51, 50), (51, 51), (50, 50)]]),
             wkb_polygon([[(2.5, 0.5), (3.5, 0.5), (3.5, 1.5), (2.5, 0.5)]])]
    lon, lat, ro, ring_row, _ = runoff._decode_wkb(geoms)
    row_rings, row_cells, pair_offsets = runoff._candidate_cells(lon, lat, ro, ring_row, 3, c)
    assert row_rings.tolist() == [0, 1, 2, 3]
    # row 0: columns 1..4 (x 0.5..4.5), rows 1..2; row 1 is past the clip envelope (x < 9.5 + 9): no cells
    assert row_cells[0].tolist() == [1, 1, 2]
    # row 2 lies exactly on boundaries 2.5..3.5 x 0.5..1.5: one cell
    assert row_cells[2].tolist() == [3, 1, 1]
    assert pair_offsets.tolist() == [0, 8, 8, 9]


def test_cell_xy_from_regular_grid(tmp_path):
    from scipy.io import netcdf_file
    path = tmp_path / 'grid.nc'
    with netcdf_file(str(path), 'w') as ds:
        ds.createDimension('lon', 3)
        ds.createDimension('lat', 2)
        ds.createDimension('t', 2)
        ds.createVariable('lon', 'f8', ('lon',))[:] = [0.0, 1.0, 2.0]
        ds.createVariable('lat', 'f8', ('lat',))[:] = [5.0, 4.0]
        ds.createVariable('xx', 'f8', ('t', 'lon'))[:] = 0.0
    x, y = runoff.cell_xy_from_regular_grid(path)
    assert x.tolist() == [0.0, 1.0, 2.0] and y.tolist() == [5.0, 4.0]
    with pytest.raises(KeyError, match=f'longitude must be a variable in {path}'):
        runoff.cell_xy_from_regular_grid(path, x_var='longitude')
    with pytest.raises(KeyError, match=f'latitude must be a variable in {path}'):
        runoff.cell_xy_from_regular_grid(path, y_var='latitude')
    with pytest.raises(ValueError, match='Regular grid requires 1D x/y coordinate arrays'):
        runoff.cell_xy_from_regular_grid(path, x_var='xx')


def _canned():
    """3 rows over a 4 x 3 grid with hand-set areas: rows 0 and 2 share river 7 (summed), row 1 is river 3."""
    c = runoff._regular_cells(np.arange(0.0, 4.0), np.array([2.0, 1.0, 0.0]))
    row_cells = np.array([[0, 0, 2], [1, 1, 1], [0, 0, 1]], dtype=np.int32)
    pair_offsets = np.array([0, 4, 6, 7])
    # row 0: cells (0,0) (0,1) (1,0) (1,1); row 1: (1,1) (2,1); row 2: (0,0)
    area = np.array([5.0e6, 2.0e6, 2.0e6, 1e-30, 4.0e6, 4.0e6, 1.0e6])
    return c, row_cells, pair_offsets, area, np.array([7, 3, 7])


def test_table_order_ties_duplicates_and_proportions():
    c, row_cells, pair_offsets, area, ids = _canned()
    df = runoff._pairs_table(ids, area, row_cells, pair_offsets, c, 'river_id')
    assert list(df.columns) == ['river_id', 'x_index', 'y_index', 'x', 'y', 'area_sqm', 'proportion']
    # the sliver is dropped; river 3 first, its tie keeps (x_index, y_index) order; river 7's (0,0) pieces summed
    sorted_rows = [2, 1, 0]                                       # sorted row j -> file y index
    got = list(zip(df.river_id, df.x_index, df.y_index, df.area_sqm))
    assert got == [(3, 1, sorted_rows[1], 4.0e6), (3, 2, sorted_rows[1], 4.0e6), (7, 0, sorted_rows[0], 6.0e6),
                   (7, 0, sorted_rows[1], 2.0e6), (7, 1, sorted_rows[0], 2.0e6)]
    np.testing.assert_allclose(df.groupby('river_id').proportion.sum(), 1.0, rtol=1e-15)
    assert df.x.tolist()[2] == c.x[0] and df.y.tolist()[2] == c.y[0]


def _write_grid(path, x, y):
    from scipy.io import netcdf_file
    with netcdf_file(str(path), 'w') as ds:
        ds.createDimension('lon', len(x))
        ds.createDimension('lat', len(y))
        ds.createVariable('lon', 'f8', ('lon',))[:] = x
        ds.createVariable('lat', 'f8', ('lat',))[:] = y


def test_grid_weights_refusals_and_missing_id(tmp_path):
    grid = tmp_path / 'grid.nc'
    _write_grid(grid, [0.0, 1.0], [0.0, 1.0])
    cat = tmp_path / 'cat.parquet'
    pd.DataFrame({'id': [1], 'geometry': [wkb_polygon([SQUARE])]}).to_parquet(cat)
    with pytest.raises(ValueError, match='crs=4326'):
        runoff.grid_weights(grid, cat, crs=3857)
    with pytest.raises(ValueError, match='save_voronoi_path'):
        runoff.grid_weights(grid, cat, save_voronoi_path=tmp_path / 'v.parquet')
    with pytest.raises(KeyError, match='catchments_gdf must contain a river_id column'):
        runoff.grid_weights(grid, cat)


def test_params_reorder_missing_river_and_file_round_trip(tmp_path, monkeypatch, caplog):
    """grid_weights after the kernel, with the kernel's areas canned: reorder by a params file that lacks one river (it goes
    last), the warning without one, and the NetCDF the table is saved to read back unchanged by prepare_runoff."""
    c, row_cells, pair_offsets, area, ids = _canned()
    grid = tmp_path / 'grid.nc'
    _write_grid(grid, np.arange(0.0, 4.0), np.array([2.0, 1.0, 0.0]))
    cat = tmp_path / 'cat.parquet'
    pd.DataFrame({'river_id': ids, 'geometry': [wkb_polygon([SQUARE])] * 3}).to_parquet(cat)
    monkeypatch.setattr(runoff, '_cell_areas', lambda x, y, rid, geoms, device, name: runoff._pairs_table(
        rid, area, row_cells, pair_offsets, runoff._regular_cells(x, y), name))
    params = tmp_path / 'params.parquet'
    pd.DataFrame({'river_id': [7, 11]}).to_parquet(params)
    out = tmp_path / 'weights.nc'
    df = runoff.grid_weights(grid, cat, routing_params_path=params, save_weights_path=out)
    assert df.river_id.tolist() == [7, 7, 7, 3, 3]
    assert df.area_sqm.tolist() == [6.0e6, 2.0e6, 2.0e6, 4.0e6, 4.0e6]

    from river_route_amd.io import read_variables
    back = read_variables(out, ['river_id', 'x_index', 'y_index', 'x', 'y', 'area_sqm', 'proportion', 'index'])
    for col in df.columns:
        np.testing.assert_array_equal(back[col][0], df[col].to_numpy())
        assert back[col][1] == ('index',)
    assert back['index'][0].tolist() == list(range(5))
    from scipy.io import netcdf_file
    with netcdf_file(str(out), 'r', mmap=False) as ds:
        assert ds.river_route_version.decode() == __import__('river_route_amd').__version__
        assert ds.description.decode() == 'proportions of runoff cells that intersect river catchments'

    # prepare_runoff reads the saved table: rivers in file order, the summed areas, one weight per (river, cell)
    from scipy.io import netcdf_file as nf
    ro = tmp_path / 'ro.nc'
    with nf(str(ro), 'w') as ds:
        ds.createDimension('time', 2)
        ds.createDimension('lat', 3)
        ds.createDimension('lon', 4)
        t = ds.createVariable('time', 'f8', ('time',))
        t[:] = [0.0, 3600.0]
        t.units = 'seconds since 2000-01-01'
        ds.createVariable('lon', 'f8', ('lon',))[:] = np.arange(4.0)
        ds.createVariable('lat', 'f8', ('lat',))[:] = [2.0, 1.0, 0.0]
        r = ds.createVariable('ro', 'f8', ('time', 'lat', 'lon'))
        r[:] = 0.0
        r.units = 'm'
    src = runoff.prepare_runoff(ro, out)
    assert src.river_ids.tolist() == [7, 3]
    np.testing.assert_array_equal(src.area, [1.0e7, 8.0e6])

    caplog.clear()
    with caplog.at_level(logging.WARNING, logger='river_route_amd.runoff'):
        df2 = runoff.grid_weights(grid, cat)
    assert df2.river_id.tolist() == [3, 3, 7, 7, 7]
    assert 'routing_params_path not provided' in caplog.text


def test_netcdf3_ids_out_of_range(tmp_path):
    df = pd.DataFrame({'river_id': [2 ** 40], 'x_index': [0], 'y_index': [0], 'x': [0.0], 'y': [0.0], 'area_sqm': [1.0],
                       'proportion': [1.0]})
    try:
        import netCDF4  # noqa: F401
        pytest.skip('netCDF4 writes 64-bit integers')
    except ImportError:
        pass
    with pytest.raises(ValueError, match='river_id'):
        runoff._write_weights(tmp_path / 'w.nc', df, {})
