"""What skip_missing=True costs: rr_metrics_update_missing_dev beside rr_metrics_update_dev and rr_metrics_adjoint_missing_dev beside
rr_metrics_adjoint_dev (DESIGN.md sections 9 and 12c, "Missing observations"), on the shapes of metrics_bw.py and grad_scores_bw.py:
a year of 15-minute steps (35,040 rows) of
  (a) 100,000 float64 columns against 100,000 float64 columns,
  (b) the same in float32,
  (c) 2,000 float32 gauge columns against 2,000 columns (columns=) of a float32 routed array of 500,000 columns,
each with three gap patterns in y_true:
  none        no NaN: the masked kernels do the unmasked kernels' arithmetic plus their compares and selects;
  random30    30 % of the elements NaN at random (seeded): neighbouring lanes and neighbouring rows differ;
  gauge_like  the year cut into 8 blocks of 4,380 rows, every column keeps one contiguous run of whole blocks (a gauge that starts
              late, stops early, or both; 1 to 8 blocks, seeded) and is NaN elsewhere: long runs, whole chunks and row splits empty.

    python profiles/microbench/metrics_missing_bw.py [--reps 7] [--warmup 2] [--scale 1.0] [--json out.json]

One process; times come from HIP events on the stream the work is on.  In every case the unmasked and the masked call ALTERNATE
(unmasked, masked, unmasked, ...), `reps` of each after `warmup` of each, on the same inputs, state and work memory, so both see the
same card in the same minute; the median, the minimum and the maximum of each are reported.  `update` is k_metrics_partial[_missing]
+ k_metrics_merge, `adjoint` k_metrics_adjoint_coef + k_metrics_adjoint_rows[_missing]: the second kernel of each pair is the same
code in both.  The masked kernels issue the same loads and stores, so both are given in TB/s of the same compulsory bytes: update
T x n x (size of y_true + size of y_pred), adjoint that plus one gradient element.  The yardstick of a masked kernel is its unmasked
twin in the same run, and the margin is the spread (max - min) of the twin's own repetitions."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import numpy as np
import torch

import river_route_amd as rr
from river_route_amd import engine

BLOCKS = 8


def alternate(fns, reps, warmup, stream):
    """fns run in turn, round after round: per function the list of its `reps` times in ms."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            fn()
            b.record(stream)
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return ms


def stats(prefix, ms, nbytes):
    med = float(np.median(ms))
    return {f'{prefix}_ms_median': med, f'{prefix}_ms_min': float(min(ms)), f'{prefix}_ms_max': float(max(ms)),
            f'{prefix}_TBps_median': nbytes / (med * 1e-3) / 1e12}


def put_gaps(obs, pattern, g):
    """obs with the pattern's NaN (in place, block of columns by block so the mask stays small); the share of elements missing."""
    T, n = obs.shape
    if pattern == 'none':
        return 0.0
    missing = 0
    step = max(1, (1 << 28) // T)
    for c0 in range(0, n, step):
        view = obs[:, c0:c0 + step]
        w = view.shape[1]
        if pattern == 'random30':
            mask = torch.rand((T, w), generator=g, device=obs.device, dtype=torch.float32) < 0.3
        else:
            first = torch.randint(0, BLOCKS, (w,), generator=g, device=obs.device)
            last = first + (torch.rand(w, generator=g, device=obs.device) * (BLOCKS - first)).long()      # first <= last < BLOCKS
            block = (torch.arange(T, device=obs.device) // ((T + BLOCKS - 1) // BLOCKS))[:, None]
            mask = (block < first[None, :]) | (block > last[None, :])
        view.masked_fill_(mask, float('nan'))
        missing += int(mask.sum())
        del mask
    return missing / (T * n)


def case(name, pattern, y_true, y_pred, columns, reps, warmup, missing_share):
    dev = y_true.device
    stream = torch.cuda.current_stream(dev)
    di = dev.index or 0
    T, n = y_true.shape
    m = int(y_pred.shape[1])
    W = torch.rand((5, n), dtype=torch.float64, device=dev, generator=torch.Generator(dev).manual_seed(1)) + 0.5
    cols_dev = order = distinct = segments = None
    nd = n
    if columns is not None:
        maps = rr.grad._sorted_columns(columns, n, m)
        nd = len(maps[2])
        maps = torch.from_numpy(np.concatenate(maps)).to(dev)
        cols_dev, order, distinct, segments = rr.grad.column_map_pointers(maps, n, nd)
    f32 = [t.dtype == torch.float32 for t in (y_true, y_pred)]
    state = torch.zeros((engine.METRICS_STATE, n), dtype=torch.float64, device=dev)
    fwork = torch.empty(max(engine.metrics_work_bytes(n, T) // 8, 1), dtype=torch.float64, device=dev)

    def update_with(call):
        def run():
            call(n, T, y_true.data_ptr(), f32[0], y_true.stride(0), y_pred.data_ptr(), f32[1], y_pred.stride(0), cols_dev, state.data_ptr(),
                 fwork.data_ptr(), fwork.numel() * 8, device=di, stream=stream.cuda_stream)
        return run

    read = T * n * (y_true.element_size() + y_pred.element_size())
    row = dict(case=name, gaps=pattern, missing_share=missing_share, rows=T, columns=n, true_dtype=str(y_true.dtype),
               pred_dtype=str(y_pred.dtype), pred_columns=m, gathered=columns is not None, update_bytes=read,
               adjoint_bytes=read + T * n * y_pred.element_size(), reps=reps)
    plain, masked = alternate([update_with(engine.metrics_update_dev), update_with(engine.metrics_update_missing_dev)], reps, warmup, stream)
    row.update(stats('update', plain, read))
    row.update(stats('update_missing', masked, read))
    row['update_missing_over_update'] = row['update_missing_ms_median'] / row['update_ms_median']
    row['update_spread_ms'] = row['update_ms_max'] - row['update_ms_min']

    # the state the adjoint reads: one masked update (the unmasked adjoint runs on it as well: the same constants, the same work)
    state.zero_()
    update_with(engine.metrics_update_missing_dev)()
    grad = torch.zeros((T, m), dtype=y_pred.dtype, device=dev)
    work = torch.empty(max(engine.metrics_adjoint_work_bytes(n) // 8, 1), dtype=torch.float64, device=dev)

    def adjoint_with(call):
        def run():
            call(n, T, y_true.data_ptr(), f32[0], y_true.stride(0), y_pred.data_ptr(), f32[1], y_pred.stride(0), state, W, nd, order, distinct,
                 segments, grad, m, work, work.numel() * 8, device=di, stream=stream.cuda_stream)
        return run

    plain, masked = alternate([adjoint_with(engine.metrics_adjoint_dev), adjoint_with(engine.metrics_adjoint_missing_dev)], reps, warmup, stream)
    row.update(stats('adjoint', plain, row['adjoint_bytes']))
    row.update(stats('adjoint_missing', masked, row['adjoint_bytes']))
    row['adjoint_missing_over_adjoint'] = row['adjoint_missing_ms_median'] / row['adjoint_ms_median']
    row['adjoint_spread_ms'] = row['adjoint_ms_max'] - row['adjoint_ms_min']
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--scale', type=float, default=1.0, help='columns x scale (a quick trial at small sizes)')
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('metrics_missing_bw.py: no GPU visible (this measures the device path only)')
    dev = torch.device('cuda', 0)
    T = 35_040
    n = max(1, int(100_000 * a.scale))
    rows = [dict(copy_bandwidth_GBps=engine.copy_bandwidth(0), device=torch.cuda.get_device_name(0))]
    print(json.dumps(rows[-1]), flush=True)
    patterns = ('none', 'random30', 'gauge_like')

    for name, dtype in (('dense_f64', torch.float64), ('dense_f32', torch.float32)):
        g = torch.Generator(device=dev).manual_seed(7)
        clean = torch.rand((T, n), generator=g, device=dev, dtype=dtype) + 1.0
        sim = 0.9 * clean + 0.1 * torch.rand((T, n), generator=g, device=dev, dtype=dtype)
        for pattern in patterns:
            obs = clean.clone()
            share = put_gaps(obs, pattern, g)
            rows.append(case(name, pattern, obs, sim, None, a.reps, a.warmup, share))
            del obs
        del clean, sim
        torch.cuda.empty_cache()

    g = torch.Generator(device=dev).manual_seed(7)
    n_routed, n_gauges = max(1, int(500_000 * a.scale)), max(1, int(2_000 * a.scale))
    routed = torch.rand((T, n_routed), generator=g, device=dev, dtype=torch.float32)
    columns = np.sort(np.random.default_rng(3).choice(n_routed, n_gauges, replace=False))
    clean = routed[:, torch.from_numpy(columns).to(dev)] * 1.05 + 0.01 * torch.rand((T, n_gauges), generator=g, device=dev, dtype=torch.float32)
    for pattern in patterns:
        obs = clean.clone()
        share = put_gaps(obs, pattern, g)
        rows.append(case('gauges_gathered_f32', pattern, obs, routed, columns, a.reps, a.warmup, share))
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
