"""rr.runoff.grid_weights at continental scale: 1,000,000 synthetic 64-vertex catchments of about 100 km^2 each (random
star polygons, seed 0, latitudes within +-60) on the 1440 x 721 ERA5 0.25-degree grid (0..359.75 longitudes, latitudes
90 .. -90 descending).

Reported:
  kernel      k_overlap_area alone (rr_grid_overlap_area_dev on device arrays), HIP events, median of --reps after --warmup;
  call        the whole grid_weights call broken into its steps, host clock, the second of two passes:
              read (grid NetCDF + catchment table), decode (WKB -> flat arrays, ring weights), candidates (cells and
              pair offsets), upload, kernel, download, table (pandas: drop, group, sort, proportions), write (NetCDF);
  lake        one 100,000-vertex polygon over about a thousand cells: the longest single wave of the layout (one wave per pair).
Edge-cell evaluations = sum over pairs of the row's vertex count.

The catchment table is written with to_parquet where a parquet engine is installed and pickled otherwise (same
DataFrame, one `geometry` column of WKB bytes).

    python profiles/microbench/grid_weights_bw.py [--n 1000000] [--reps 5] [--warmup 2] [--json out.json]
"""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import numpy as np
import pandas as pd
import torch

from river_route_amd import engine, runoff


def star_wkb(cx, cy, radius_deg, m, rng):
    """(n,) WKB Polygon bytes: star rings of m vertices (+ the closing one), radius widened in longitude by 1/cos(lat)."""
    n = cx.size
    ang = np.sort(rng.uniform(0, 2 * np.pi, (n, m)), axis=1)
    rad = radius_deg * rng.uniform(0.6, 1.0, (n, m))
    ring = np.stack([cx[:, None] + rad * np.cos(ang) / np.cos(np.radians(cy))[:, None], cy[:, None] + rad * np.sin(ang)], axis=2)
    ring = np.concatenate([ring, ring[:, :1]], axis=1)
    head = bytes([1]) + (3).to_bytes(4, 'little') + (1).to_bytes(4, 'little') + (m + 1).to_bytes(4, 'little')
    return [head + r.tobytes() for r in ring]


def write_grid(path):
    from scipy.io import netcdf_file
    with netcdf_file(str(path), 'w') as ds:
        ds.createDimension('lon', 1440)
        ds.createDimension('lat', 721)
        ds.createVariable('lon', 'f8', ('lon',))[:] = np.arange(1440) * 0.25
        ds.createVariable('lat', 'f8', ('lat',))[:] = 90.0 - np.arange(721) * 0.25


def events(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def device_launch(n_rows, host):
    """Device copies of the kernel's inputs and a launcher of rr_grid_overlap_area_dev on the current stream."""
    names = ('row_rings', 'ring_offsets', 'ring_weight', 'lon', 'lat', 'x_bounds', 'y_bounds', 'row_cells', 'pair_offsets')
    dev = [torch.from_numpy(np.ascontiguousarray(host[k])).cuda() for k in names]
    n_pairs = int(host['pair_offsets'][-1])
    area = torch.empty(max(n_pairs, 1), dtype=torch.float64, device='cuda')
    sizes = (n_rows, host['ring_offsets'].size - 1, host['lon'].size, host['x_bounds'].size - 1, host['y_bounds'].size - 1, n_pairs)

    def launch():
        engine.grid_overlap_area_dev(*sizes, *dev, area, stream=torch.cuda.current_stream().cuda_stream)
    return launch, area, n_pairs


def staged(grid, cat, out, read_table):
    """grid_weights step by step (the same functions it calls), each step timed."""
    t = {}
    c0 = time.perf_counter()
    x, y = runoff.cell_xy_from_regular_grid(grid)
    df = read_table(cat)
    t['read'] = time.perf_counter() - c0
    c0 = time.perf_counter()
    cells = runoff._regular_cells(x, y)
    ids, geoms = df['river_id'].to_numpy(), df['geometry'].to_numpy()
    lon, lat, ro, ring_row, ext = runoff._decode_wkb(geoms)
    w = runoff._ring_weights(lon, lat, ro, ext)
    t['decode'] = time.perf_counter() - c0
    c0 = time.perf_counter()
    row_rings, row_cells, pair_offsets = runoff._candidate_cells(lon, lat, ro, ring_row, ids.size, cells)
    t['candidates'] = time.perf_counter() - c0
    c0 = time.perf_counter()
    host = dict(row_rings=row_rings, ring_offsets=ro, ring_weight=w, lon=lon, lat=lat, x_bounds=cells.x_bounds,
                y_bounds=cells.y_bounds, row_cells=row_cells, pair_offsets=pair_offsets)
    launch, area, n_pairs = device_launch(ids.size, host)
    torch.cuda.synchronize()
    t['upload'] = time.perf_counter() - c0
    c0 = time.perf_counter()
    launch()
    torch.cuda.synchronize()
    t['kernel'] = time.perf_counter() - c0
    c0 = time.perf_counter()
    a = area[:n_pairs].cpu().numpy()
    t['download'] = time.perf_counter() - c0
    c0 = time.perf_counter()
    table = runoff._pairs_table(ids, a, row_cells, pair_offsets, cells, 'river_id')
    t['table'] = time.perf_counter() - c0
    c0 = time.perf_counter()
    runoff._write_weights(out, table, {'description': 'proportions of runoff cells that intersect river catchments'})
    t['write'] = time.perf_counter() - c0
    evals = int(np.sum(np.diff(pair_offsets) * np.diff(ro[row_rings])))
    return t, table, launch, n_pairs, evals


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=1_000_000)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--json')
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    try:
        import pyarrow  # noqa: F401
        write_table, read_table = (lambda df, p: df.to_parquet(p)), pd.read_parquet
    except ImportError:
        write_table, read_table = (lambda df, p: df.to_pickle(p)), pd.read_pickle

    res = {'n_catchments': args.n, 'vertices_per_ring': 65, 'grid': '1440 x 721, 0.25 deg'}
    with tempfile.TemporaryDirectory() as tmp:
        grid, cat, out = os.path.join(tmp, 'grid.nc'), os.path.join(tmp, 'cat.bin'), os.path.join(tmp, 'weights.nc')
        write_grid(grid)
        # about 100 km^2: a star of radius 0.6..1 x 0.0705 deg, widened in longitude by 1/cos(lat)
        geoms = []
        for lo in range(0, args.n, 100_000):
            k = min(100_000, args.n - lo)
            geoms += star_wkb(rng.uniform(-179, 179, k), rng.uniform(-60, 60, k), 0.0705, 64, rng)
        write_table(pd.DataFrame({'river_id': np.arange(1, args.n + 1, dtype=np.int64), 'geometry': geoms}), cat)
        del geoms

        staged(grid, cat, out, read_table)                     # warm-up: code objects, allocator, page cache
        t, table, launch, n_pairs, evals = staged(grid, cat, out, read_table)
        ms = events(launch, args.reps, args.warmup)
        res.update(pairs=n_pairs, rows_out=len(table), edge_cell_evaluations=evals, kernel_ms=float(np.median(ms)),
                   kernel_ms_all=[round(v, 4) for v in ms], call_s={k: round(v, 4) for k, v in t.items()},
                   call_total_s=round(sum(t.values()), 3),
                   mean_area_km2=float(table.groupby('river_id').area_sqm.sum().mean() / 1e6),
                   weights_file_bytes=os.path.getsize(out))

    # one large lake: 100,000 vertices, radius ~4 deg: about a thousand candidate cells, each one wave over all its edges
    lake = star_wkb(np.array([20.0]), np.array([10.0]), 4.0, 100_000, rng)
    lon, lat, ro, ring_row, ext = runoff._decode_wkb(lake)
    cells = runoff._regular_cells(np.arange(1440) * 0.25, 90.0 - np.arange(721) * 0.25)
    row_rings, row_cells, pair_offsets = runoff._candidate_cells(lon, lat, ro, ring_row, 1, cells)
    host = dict(row_rings=row_rings, ring_offsets=ro, ring_weight=runoff._ring_weights(lon, lat, ro, ext), lon=lon, lat=lat,
                x_bounds=cells.x_bounds, y_bounds=cells.y_bounds, row_cells=row_cells, pair_offsets=pair_offsets)
    launch, area, n_pairs = device_launch(1, host)
    lake_ms = events(launch, args.reps, args.warmup)
    res['lake'] = {'vertices': int(lon.size), 'pairs': n_pairs, 'kernel_ms': float(np.median(lake_ms)),
                   'area_km2': float(area[:n_pairs].sum().item() / 1e6)}
    line = json.dumps(res)
    print(line)
    if args.json:
        with open(args.json, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
