"""Backward time of rr.grad.runoff_to_qlateral against what a user has without it, the backward of a torch
restatement (index_add over the pairs), on the shape of DESIGN.md section 11: 1,000,000 catchments on the ERA5 0.25 degree grid, about
2.5 pairs per catchment, 744 rows (a month of hourly runoff), float32 and float64 runoff, cumulative input with the clip on.

    python profiles/microbench/grad_runoff_bw.py [--json OUT] [--reps 5] [--warmup 1] [--cases 1M_f32,1M_f64]

--json adds to a file that exists, so the cases can be run one process each into one file.

The table is synthetic: catchments come basin after basin (1,000 to a basin, a basin a 32 x 32 patch of cells somewhere on the grid),
each over 1 to 4 cells of a 2 x 2 block, and the runoff block holds the grid points some catchment uses, as rr.runoff.prepare_runoff
leaves it.  Per case, HIP events on torch's stream, the median of `reps` runs after `warmup`, kernel path and restatement alternating
in one process:
  forward             rr.grad.runoff_to_qlateral (k_runoff_to_qlateral) on the (T, points) block as read from a file;
  backward_runoff     its backward to the runoff alone (river pass + point pass), cotangent given;
  backward_both       the same with grad_weights (the weight pass too);
  *_point_major       the three again on a point-major block with rows of a multiple of 16 elements (the kernels' vector path);
  torch_*             forward, and backward to the runoff alone and to both, of the restatement.
backward_runoff_TBps is the compulsory traffic -- the cotangent read once, the runoff read once, grad_runoff written once -- over
backward_runoff_ms; the passes really move more (the runoff is gathered once per pair, Gs goes through work memory: `moved_bytes`)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import river_route_amd as rr  # noqa: E402
from river_route_amd import engine  # noqa: E402

# catchments, rows, runoff dtype
CASES = {'1M_f32': (1_000_000, 744, 'float32'), '1M_f64': (1_000_000, 744, 'float64')}
EXTRA = {'tiny': (3000, 40, 'float32')}      # not in the default list: a rehearsal size
NX, NY = 1440, 721


def synth_table(n, seed=5):
    """(indptr, indices, n_points, weights, area) of n catchments on the NX x NY grid, rows in ascending point order."""
    rng = np.random.default_rng(seed)
    basin = np.arange(n) // 1000
    n_basins = int(basin[-1]) + 1
    ox, oy = rng.integers(0, NX - 34, n_basins), rng.integers(0, NY - 34, n_basins)
    cx, cy = ox[basin] + rng.integers(0, 32, n), oy[basin] + rng.integers(0, 32, n)
    count = rng.integers(1, 5, n)      # 1 .. 4 cells: 2.5 on average
    rows, cells = [], []
    for j, (dx, dy) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):
        has = np.flatnonzero(count > j)
        rows.append(has)
        cells.append((cy[has] + dy) * NX + cx[has] + dx)
    rows, cells = np.concatenate(rows), np.concatenate(cells)
    used, point = np.unique(cells, return_inverse=True)
    order = np.lexsort((point, rows))
    indptr = np.concatenate(([0], np.cumsum(np.bincount(rows, minlength=n))))
    return indptr.astype(np.int32), point[order].astype(np.int32), int(used.shape[0]), rng.uniform(0.05, 1.0, rows.shape[0]), rng.uniform(5e7, 2e8, n)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def run_case(name, n, T, dtype, reps, warmup):
    dev = torch.device('cuda', 0)
    gen = torch.Generator(dev).manual_seed(7)
    indptr, indices, P, w_host, area_host = synth_table(n)
    nnz = int(indices.shape[0])
    rmap = rr.grad.RunoffMap(indptr, indices, P)
    rt = getattr(torch, dtype)
    R = torch.cumsum(torch.rand((T, P), dtype=torch.float64, device=dev, generator=gen) - 0.1, dim=0).to(rt)      # some increments negative
    t_pad = -(-T // 16) * 16
    block = torch.zeros((P, t_pad), dtype=rt, device=dev)
    block[:, :T] = R.t()
    R_pm = block[:, :T].t()
    w = torch.tensor(w_host, device=dev)
    area = torch.tensor(area_host, device=dev)
    G = torch.rand((T, n), dtype=torch.float64, device=dev, generator=gen) - 0.5
    river = torch.as_tensor(rmap.pair_river.astype(np.int64), device=dev)
    cols = torch.as_tensor(indices.astype(np.int64), device=dev)

    def ours(runoff, wt):
        return rr.grad.runoff_to_qlateral(rmap, runoff, wt, area, cumulative=True, force_positive=True)

    def restated(runoff, wt):
        S = torch.zeros((T, n), dtype=torch.float64, device=dev).index_add(1, river, runoff[:, cols] * wt)
        return torch.cat([S[:1], S[1:] - S[:-1]]).clamp(min=0) * area

    paths = {'': (ours, R), '_point_major': (ours, R_pm), 'torch_': (restated, R)}
    t = {}
    grads = {}
    for it in range(warmup + reps):
        for tag, (fn, runoff) in paths.items():
            for what in ('runoff', 'both'):
                r = runoff.detach().requires_grad_()
                wt = w.detach().requires_grad_(what == 'both')
                fwd, q = timed(lambda: fn(r, wt))
                bwd, g = timed(lambda: torch.autograd.grad(q, (r, wt) if what == 'both' else (r,), G))
                key = (lambda s: f'torch_{s}' if tag == 'torch_' else f'{s}{tag}')
                if it >= warmup:
                    t.setdefault(key('forward'), []).append(fwd)
                    t.setdefault(key(f'backward_{what}'), []).append(bwd)
                grads[(tag, what)] = g
                del q, g, r, wt
    med = {k + '_ms': float(np.median(v)) for k, v in t.items()}
    es = R.element_size()
    compulsory = 8 * T * n + 2 * es * T * P
    moved = 8 * T * n + es * T * nnz + 2 * 8 * t_pad * n + 8 * t_pad * nnz + es * T * P      # G, R per pair, Gs out and in per river and pair, grad_runoff
    diff = {}
    for what in ('runoff', 'both'):
        for j, label in enumerate(('grad_runoff', 'grad_weights')[:len(grads[('', what)])]):
            a, b = grads[('', what)][j].double(), grads[('torch_', what)][j].double()
            diff[f'{label}_{what}_max_abs_diff_over_max'] = float((a - b).abs().max() / b.abs().max())
            diff[f'{label}_{what}_layouts_bit_equal'] = bool(torch.equal(grads[('', what)][j], grads[('_point_major', what)][j]))
    return dict(case=name, catchments=n, grid_points=P, pairs=nnz, rows=T, runoff_dtype=dtype, cumulative=True, force_positive=True, **med,
                torch_over_ours_backward_runoff=med['torch_backward_runoff_ms'] / med['backward_runoff_ms'],
                torch_over_ours_backward_both=med['torch_backward_both_ms'] / med['backward_both_ms'],
                torch_over_ours_forward=med['torch_forward_ms'] / med['forward_ms'],
                compulsory_bytes=compulsory, moved_bytes=moved, backward_runoff_TBps=compulsory / (med['backward_runoff_ms'] * 1e-3) / 1e12,
                backward_runoff_point_major_TBps=compulsory / (med['backward_runoff_point_major_ms'] * 1e-3) / 1e12,
                work_bytes=engine.runoff_adjoint_work_bytes(n, P, T), all_ms=t, **diff)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--json')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--cases', default=','.join(CASES))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('grad_runoff_bw.py: no GPU visible (this measures the device path only)')
    # a file that is there already is added to (a case measured again replaces its entry): the cases can run one process each
    res = dict(copy_bandwidth_GBps=engine.copy_bandwidth(0), device=torch.cuda.get_device_name(0), cases=[])
    if a.json and os.path.exists(a.json):
        with open(a.json) as f:
            res = json.load(f)
    for name in a.cases.split(','):
        r = run_case(name, *{**CASES, **EXTRA}[name], a.reps, a.warmup)
        print(json.dumps({k: v for k, v in r.items() if k != 'all_ms'}), flush=True)
        res['cases'] = [c for c in res['cases'] if c['case'] != name] + [r]
        torch.cuda.empty_cache()
        if a.json:      # after every case: a later case that does not fit leaves the earlier ones on file
            with open(a.json, 'w') as f:
                json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
