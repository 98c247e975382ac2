"""rr_grid_overlap_area / rr.runoff.grid_weights on the GPU: analytic rectangles, random star polygons against an independent
numpy clip-then-project, conservation, degenerate edges, repeatability, scale, ABI errors and the path end to end."""
import numpy as np
import pandas as pd
import pytest

from river_route_amd import _lib, engine, runoff

from test_grid_weights import _write_grid, wkb_multipolygon, wkb_polygon

pytestmark = pytest.mark.gpu
KX = runoff._CEA_X_PER_DEG
cea = runoff._cea_y


def sh_area(ring, x0, x1, y0, y1):
    """Sutherland-Hodgman clip of a lon/lat ring to [x0, x1] x [y0, y1], then cea projection and shoelace (signed)."""
    pts = [tuple(p) for p in np.asarray(ring, dtype=np.float64)]

    def clip(pts, inside, cut):
        out = []
        for i in range(len(pts)):
            a, b = pts[i - 1], pts[i]
            if inside(b):
                if not inside(a):
                    out.append(cut(a, b))
                out.append(b)
            elif inside(a):
                out.append(cut(a, b))
        return out

    at_x = lambda xc: lambda a, b: (xc, a[1] + (xc - a[0]) * (b[1] - a[1]) / (b[0] - a[0]))      # noqa: E731
    at_y = lambda yc: lambda a, b: (a[0] + (yc - a[1]) * (b[0] - a[0]) / (b[1] - a[1]), yc)      # noqa: E731
    for inside, cut in ((lambda p: p[0] >= x0, at_x(x0)), (lambda p: p[0] <= x1, at_x(x1)),
                        (lambda p: p[1] >= y0, at_y(y0)), (lambda p: p[1] <= y1, at_y(y1))):
        if not pts:
            return 0.0
        pts = clip(pts, inside, cut)
    if len(pts) < 3:
        return 0.0
    X, Y = np.array([p[0] for p in pts]) * KX, cea(np.array([p[1] for p in pts]))
    return 0.5 * float(np.sum(X * np.roll(Y, -1) - np.roll(X, -1) * Y))


def reference_table(x, y, polys):
    """{(row, x_index, y_index): area} by sh_area over every cell, rings weighted +-1 (exterior / hole)."""
    c = runoff._regular_cells(x, y)
    yb = np.clip(c.y_bounds, -90, 90)
    out = {}
    for row, rings in enumerate(polys):
        for i in range(c.x.size):
            for j in range(c.y.size):
                a = 0.0
                for k, ring in enumerate(rings):
                    s = sh_area(ring, c.x_bounds[i], c.x_bounds[i + 1], yb[j], yb[j + 1])
                    a += abs(s) if k == 0 else -abs(s)
                cell = (c.x_bounds[i + 1] - c.x_bounds[i]) * KX * (cea(yb[j + 1]) - cea(yb[j]))
                if a > runoff.DROP_SHARE * cell:
                    out[(row, int(c.x_index[i]), int(c.y_index[j]))] = (a, cell)
    return out


def star(cx, cy, r, m, rng, ccw=True):
    ang = np.sort(rng.uniform(0, 2 * np.pi, m))
    rad = r * rng.uniform(0.3, 1.0, m)
    ring = np.column_stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)])
    ring = ring if ccw else ring[::-1]
    return np.vstack([ring, ring[:1]])


def table_of(df, key='river_id'):
    return {(int(r), int(i), int(j)): a for r, i, j, a in zip(df[key], df.x_index, df.y_index, df.area_sqm)}


def test_aligned_rectangles_cover_exactly_their_cells():
    x, y = np.arange(10.0, 20.0, 0.25), np.arange(40.0, 45.0, 0.25)[::-1]
    c = runoff._regular_cells(x, y)
    rects = [(11.125, 12.625, 41.375, 42.125), (15.125, 15.375, 43.625, 43.875)]
    geoms = [wkb_polygon([[(a, c0), (b, c0), (b, d), (a, d), (a, c0)]]) for a, b, c0, d in rects]
    df = runoff.catchment_cell_areas(x, y, [1, 2], geoms)
    for rid, (a, b, c0, d) in enumerate(rects, start=1):
        sub = df[df.river_id == rid]
        cols = np.nonzero((c.x_bounds[:-1] >= a) & (c.x_bounds[1:] <= b))[0]
        rows = np.nonzero((c.y_bounds[:-1] >= c0) & (c.y_bounds[1:] <= d))[0]
        assert len(sub) == cols.size * rows.size                        # no slivers from the touching neighbours
        want = {(int(c.x_index[i]), int(c.y_index[j])): (c.x_bounds[i + 1] - c.x_bounds[i]) * KX * (cea(c.y_bounds[j + 1]) - cea(c.y_bounds[j]))
                for i in cols for j in rows}
        for i, j, area in zip(sub.x_index, sub.y_index, sub.area_sqm):
            np.testing.assert_allclose(area, want[(i, j)], rtol=1e-12)


def test_unaligned_rectangle_closed_form():
    x, y = np.arange(0.0, 5.0, 0.5), np.arange(-3.0, 3.0, 0.5)
    c = runoff._regular_cells(x, y)
    a, b, c0, d = 0.8, 2.9, -1.1, 1.37
    df = runoff.catchment_cell_areas(x, y, [5], [wkb_polygon([[(a, c0), (a, d), (b, d), (b, c0), (a, c0)]])])    # clockwise
    got = table_of(df)
    want = {}
    for i in range(c.x.size):
        for j in range(c.y.size):
            w = min(b, c.x_bounds[i + 1]) - max(a, c.x_bounds[i])
            lo, hi = max(c0, c.y_bounds[j]), min(d, c.y_bounds[j + 1])
            if w > 0 and hi > lo:
                want[(5, int(c.x_index[i]), int(c.y_index[j]))] = w * KX * (cea(hi) - cea(lo))
    assert set(got) == set(want)
    for k in want:
        np.testing.assert_allclose(got[k], want[k], rtol=1e-12)


def _random_polys(rng, n, x_lo, x_hi, y_lo, y_hi, r):
    polys = []
    for i in range(n):
        cx, cy = rng.uniform(x_lo, x_hi), rng.uniform(y_lo, y_hi)
        outer = star(cx, cy, r, int(rng.integers(12, 48)), rng, ccw=bool(i % 2))
        rings = [outer]
        if i % 3 == 0:
            rings.append(star(cx, cy, 0.1 * r, 8, rng, ccw=bool(i % 4)))       # a hole near the centre, either orientation
        polys.append(rings)
    return polys


def _geoms(polys):
    return [wkb_polygon(rings) for rings in polys]


def test_random_stars_match_numpy_clipper():
    rng = np.random.default_rng(11)
    x, y = np.arange(100.0, 103.0, 0.25), np.arange(30.0, 33.0, 0.25)[::-1]
    polys = _random_polys(rng, 24, 100.5, 102.5, 30.5, 32.5, 0.45)
    # two multipart rows: their parts are rows 24, 25 of the reference, summed under one id
    parts = [[star(100.8, 30.8, 0.2, 20, rng)], [star(101.9, 31.9, 0.2, 20, rng, ccw=False)]]
    geoms = _geoms(polys) + [wkb_multipolygon(parts)]
    df = runoff.catchment_cell_areas(x, y, np.arange(25), geoms)
    want = reference_table(x, y, polys + parts)
    merged = {}
    for (row, i, j), v in want.items():
        key = (min(row, 24), i, j)
        merged[key] = (merged.get(key, (0.0, v[1]))[0] + v[0], v[1])
    got = table_of(df)
    assert set(got) == set(merged)
    for k, (a, cell) in merged.items():
        assert abs(got[k] - a) <= 1e-9 * cell, (k, got[k], a)
    np.testing.assert_allclose(df.groupby('river_id').proportion.sum(), 1.0, rtol=1e-12)


def densified_area(ring, xb, yb):
    """cea area of a ring with every crossing of the grid lines inserted as a vertex (what the pieces add up to)."""
    ring = np.asarray(ring, dtype=np.float64)
    pts = []
    for a, b in zip(ring[:-1], ring[1:]):
        ts = [0.0]
        for g, k in ((xb, 0), (yb, 1)):
            if b[k] != a[k]:
                t = (g - a[k]) / (b[k] - a[k])
                ts.extend(t[(t > 0) & (t < 1)])
        for t in sorted(ts):
            pts.append(a + t * (b - a))
    pts = np.array(pts)
    X, Y = pts[:, 0] * KX, cea(pts[:, 1])
    return 0.5 * abs(float(np.sum(X * np.roll(Y, -1) - np.roll(X, -1) * Y)))


def test_conservation():
    rng = np.random.default_rng(5)
    x, y = np.arange(-10.0, -5.0, 0.25), np.arange(60.0, 64.0, 0.25)
    c = runoff._regular_cells(x, y)
    polys = [[star(rng.uniform(-9, -6), rng.uniform(61, 63), 0.6, 40, rng, ccw=bool(i % 2))] for i in range(10)]
    # rectilinear staircase: every split is exact, so the pieces add up to the plain cea area
    stair = np.array([(-9.1, 60.3), (-7.3, 60.3), (-7.3, 61.2), (-6.4, 61.2), (-6.4, 62.9), (-9.1, 62.9), (-9.1, 60.3)])
    df = runoff.catchment_cell_areas(x, y, np.arange(11), [wkb_polygon(p) for p in polys] + [wkb_polygon([stair])])
    tot = df.groupby('river_id').area_sqm.sum()
    for i, rings in enumerate(polys):
        np.testing.assert_allclose(tot[i], densified_area(rings[0], c.x_bounds, c.y_bounds), rtol=1e-9)
    X, Y = stair[:, 0] * KX, cea(stair[:, 1])
    np.testing.assert_allclose(tot[10], 0.5 * abs(np.sum(X[:-1] * Y[1:] - X[1:] * Y[:-1])), rtol=1e-9)


def test_degenerate_edges():
    x, y = np.arange(0.0, 4.0), np.arange(0.0, 4.0)          # boundaries at .5
    ring = [(0.5, 0.5), (1.5, 0.5), (1.5, 0.5), (2.5, 1.5), (2.5, 2.5), (1.5, 2.5), (1.0, 2.5), (0.5, 1.5), (0.5, 0.5)]
    # on boundaries, a zero-length edge, a diagonal through the cell corner (1.5, 0.5) -> (2.5, 1.5), vertical and
    # horizontal edges, an edge ending mid-side
    df = runoff.catchment_cell_areas(x, y, [1], [wkb_polygon([ring])])
    want = reference_table(x, y, [[ring]])
    got = table_of(df)
    assert set(got) == {(1, i, j) for (_, i, j) in want}
    for (_, i, j), (a, cell) in want.items():
        assert abs(got[(1, i, j)] - a) <= 1e-9 * cell


def test_repeatable_bits():
    rng = np.random.default_rng(3)
    x, y = np.arange(0.0, 20.0, 0.25), np.arange(0.0, 10.0, 0.25)
    geoms = _geoms(_random_polys(rng, 300, 1, 19, 1, 9, 0.7))
    a = runoff.catchment_cell_areas(x, y, np.arange(300), geoms)
    b = runoff.catchment_cell_areas(x, y, np.arange(300), geoms)
    assert a.area_sqm.to_numpy().tobytes() == b.area_sqm.to_numpy().tobytes()
    pd.testing.assert_frame_equal(a, b)


def test_scale_1e5_against_clipper_subset():
    rng = np.random.default_rng(8)
    x, y = np.arange(0.0, 360.0, 0.25), np.arange(90.0, -90.25, -0.25)           # the ERA5 0.25 degree grid
    n = 100_000
    cx, cy = rng.uniform(-170, 170, n), rng.uniform(-60, 60, n)
    m = 16
    ang = np.sort(rng.uniform(0, 2 * np.pi, (n, m)), axis=1)
    rad = 0.08 * rng.uniform(0.3, 1.0, (n, m))
    rings = np.stack([cx[:, None] + rad * np.cos(ang), cy[:, None] + rad * np.sin(ang)], axis=2)
    rings = np.concatenate([rings, rings[:, :1]], axis=1)
    head = bytes([1]) + (3).to_bytes(4, 'little') + (1).to_bytes(4, 'little') + (m + 1).to_bytes(4, 'little')
    geoms = [head + r.tobytes() for r in rings]
    df = runoff.catchment_cell_areas(x, y, np.arange(n), geoms)
    assert df.river_id.nunique() == n
    c = runoff._regular_cells(x, y)
    col_of = {int(v): i for i, v in enumerate(c.x_index)}
    row_of = {int(v): j for j, v in enumerate(c.y_index)}
    got = table_of(df)
    for r in rng.choice(n, 60, replace=False):
        ring = rings[r]
        sub = df[df.river_id == r]
        for i, j, area in zip(sub.x_index, sub.y_index, sub.area_sqm):
            ci, rj = col_of[int(i)], row_of[int(j)]
            ref = sh_area(ring, c.x_bounds[ci], c.x_bounds[ci + 1], c.y_bounds[rj], c.y_bounds[rj + 1])
            cell = (c.x_bounds[ci + 1] - c.x_bounds[ci]) * KX * (cea(c.y_bounds[rj + 1]) - cea(c.y_bounds[rj]))
            assert abs(abs(ref) - area) <= 1e-9 * cell
        assert len(sub) == sum(1 for k in got if k[0] == r)


def test_abi_errors():
    lib = _lib.lib()
    z64 = np.zeros(2, dtype=np.int64)
    one = np.ones(2)
    cells = np.zeros(3, dtype=np.int32)
    rc = lib.rr_grid_overlap_area(0, 1, 1, 2, 0, 1, 1, z64.ctypes.data, z64.ctypes.data, one.ctypes.data, one.ctypes.data,
                                  one.ctypes.data, one.ctypes.data, one.ctypes.data, cells.ctypes.data, z64.ctypes.data, one.ctypes.data)
    assert rc == _lib.RR_E_INVALID and b'sizes' in lib.rr_last_error()
    # offsets that do not end at the counts
    rc = lib.rr_grid_overlap_area(0, 1, 1, 2, 1, 1, 1, z64.ctypes.data, z64.ctypes.data, one.ctypes.data, one.ctypes.data,
                                  one.ctypes.data, one.ctypes.data, one.ctypes.data, cells.ctypes.data, z64.ctypes.data, one.ctypes.data)
    assert rc == _lib.RR_E_INVALID and b'offsets' in lib.rr_last_error()
    with pytest.raises(_lib.RRError) as e:       # candidate cells past the grid
        engine.grid_overlap_area([0, 1], [0, 2], [1.0], [0.0, 1.0], [0.0, 1.0], [0.0, 1.0], [0.0, 1.0], [[0, 0, 2]], [0, 2])
    assert e.value.code == _lib.RR_E_INVALID
    rc = lib.rr_grid_overlap_area_dev(0, 1, 1, 2, 1, 1, 1, None, None, None, None, None, None, None, None, None, None, None)
    assert rc == _lib.RR_E_INVALID and b'null' in lib.rr_last_error()
    rc = lib.rr_grid_overlap_area_dev(99, 1, 1, 2, 1, 1, 1, None, None, None, None, None, None, None, None, None, None, None)
    assert rc == _lib.RR_E_NO_DEVICE


def test_end_to_end_uniform_runoff(tmp_path):
    from scipy.io import netcdf_file
    rng = np.random.default_rng(2)
    x, y = np.arange(0.0, 360.0, 2.0), np.arange(60.0, 29.0, -2.0)            # 0..360 longitudes, descending latitude
    ids = np.arange(1, 41)
    polys = _random_polys(rng, 40, -20, 20, 35, 55, 3.0)
    grid = tmp_path / 'grid.nc'
    _write_grid(grid, x, y)
    cat = tmp_path / 'cat.parquet'
    pd.DataFrame({'river_id': ids, 'geometry': _geoms(polys)}).to_parquet(cat)
    weights = tmp_path / 'weights.nc'
    df = runoff.grid_weights(grid, cat, save_weights_path=weights)
    assert set(df.river_id) == set(ids)
    T, d = 4, 0.003
    ro = tmp_path / 'ro.nc'
    with netcdf_file(str(ro), 'w') as ds:
        ds.createDimension('time', T)
        ds.createDimension('lat', y.size)
        ds.createDimension('lon', x.size)
        t = ds.createVariable('time', 'f8', ('time',))
        t[:] = np.arange(T) * 3600.0
        t.units = 'seconds since 2001-01-01'
        ds.createVariable('lon', 'f8', ('lon',))[:] = x
        ds.createVariable('lat', 'f8', ('lat',))[:] = y
        r = ds.createVariable('ro', 'f8', ('time', 'lat', 'lon'))
        r[:] = d
        r.units = 'm'
    depth = runoff.runoff_to_qlateral(ro, weights)
    np.testing.assert_allclose(depth['qlateral'].values, d, rtol=1e-12)
    vol = runoff.runoff_to_qlateral(ro, weights, as_volumes=True)
    total = df.groupby('river_id').area_sqm.sum().reindex(vol['river_id'].values).to_numpy()
    q = vol['qlateral'].values
    np.testing.assert_allclose(q, np.broadcast_to(d * total, q.shape), rtol=1e-12)

    # the routers take the file: a params file of the same rivers, all headwaters draining to one outlet chain
    import river_route_amd as rr
    n = ids.size
    params = tmp_path / 'params.parquet'
    pd.DataFrame({'river_id': ids, 'downstream_river_id': np.r_[ids[1:], -1], 'k': np.full(n, 3600.0), 'x': np.full(n, 0.2)}).to_parquet(params)
    out = tmp_path / 'q.nc'
    rr.RapidMuskingum(params_file=str(params), grid_runoff_files=[str(ro)], grid_weights_file=str(weights),
                      discharge_files=[str(out)], dt_routing=3600, var_x='lon', var_y='lat', log=False).route()
    assert out.exists()
