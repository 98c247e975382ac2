"""Bandwidth of rr.metrics.scores on device arrays: a year of 15-minute steps (35,040 rows) of
  (a) 100,000 float64 columns against 100,000 float64 columns,
  (b) the same in float32,
  (c) 2,000 float64 gauge columns against 2,000 columns gathered (columns=) from a 1,000,000-column routed array.
      The routed array is float32 (the routers' output type): a float64 one, 280 GB, would not fit beside the rest.
Times come from HIP events on the stream the work is on, after warm-up calls of the same shape: `update` is the
k_metrics_partial + k_metrics_merge pair alone (state and work memory allocated beforehand), `scores` the whole
call (state allocation and zeroing, the two kernels, k_metrics_finish, the result tensor).  Compulsory bytes are the
elements a score needs, each read once: T x n x (size of y_true + size of y_pred) (in (c) the gathered elements only;
a gathered 4-byte element costs the memory system at least a 64-byte line).

    python profiles/microbench/metrics_bw.py [--reps 5] [--warmup 2] [--scale 1.0] [--json out.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import numpy as np
import torch

import river_route_amd as rr
from river_route_amd import engine


def timed(fn, reps, warmup, stream):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def case(name, y_true, y_pred, columns, reps, warmup):
    dev = y_true.device
    stream = torch.cuda.current_stream(dev)
    T, n = y_true.shape
    cols_dev = None
    if columns is not None:
        cols_dev = torch.from_numpy(columns.astype(np.int32)).to(dev)
    state = torch.zeros((engine.METRICS_STATE, n), dtype=torch.float64, device=dev)
    work = torch.empty(engine.metrics_work_bytes(n, T) // 8, dtype=torch.float64, device=dev)

    def update():
        engine.metrics_update_dev(n, T, y_true.data_ptr(), y_true.dtype == torch.float32, y_true.stride(0), y_pred.data_ptr(),
                                  y_pred.dtype == torch.float32, y_pred.stride(0), cols_dev.data_ptr() if cols_dev is not None else None,
                                  state.data_ptr(), work.data_ptr(), work.numel() * 8, device=dev.index or 0, stream=stream.cuda_stream)

    def scores():
        rr.metrics.scores(y_true, y_pred, columns=columns)

    nbytes = T * n * (y_true.element_size() + y_pred.element_size())
    ms_u = timed(update, reps, warmup, stream)
    ms_s = timed(scores, reps, warmup, stream)
    row = dict(case=name, rows=T, columns=n, true_dtype=str(y_true.dtype), pred_dtype=str(y_pred.dtype),
               pred_columns=int(y_pred.shape[1]), gathered=columns is not None, compulsory_bytes=nbytes,
               work_bytes=int(work.numel() * 8),
               update_ms_median=float(np.median(ms_u)), update_ms_min=float(min(ms_u)),
               update_TBps_median=nbytes / (np.median(ms_u) * 1e-3) / 1e12,
               scores_ms_median=float(np.median(ms_s)), scores_ms_min=float(min(ms_s)),
               scores_TBps_median=nbytes / (np.median(ms_s) * 1e-3) / 1e12)
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--scale', type=float, default=1.0, help='columns x scale (a quick trial at small sizes)')
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('metrics_bw.py: no GPU visible (this measures the device path only)')
    dev = torch.device('cuda', 0)
    g = torch.Generator(device=dev).manual_seed(7)
    T = 35_040
    n = max(1, int(100_000 * a.scale))
    rows = []
    obs = torch.rand((T, n), generator=g, device=dev, dtype=torch.float64) + 1.0
    sim = 0.9 * obs + 0.1 * torch.rand((T, n), generator=g, device=dev, dtype=torch.float64)
    rows.append(case('dense_f64', obs, sim, None, a.reps, a.warmup))
    obs, sim = obs.float(), sim.float()
    rows.append(case('dense_f32', obs, sim, None, a.reps, a.warmup))
    del obs, sim
    torch.cuda.empty_cache()
    n_routed, n_gauges = max(1, int(1_000_000 * a.scale)), max(1, int(2_000 * a.scale))
    routed = torch.rand((T, n_routed), generator=g, device=dev, dtype=torch.float32)
    columns = np.sort(np.random.default_rng(3).choice(n_routed, n_gauges, replace=False))
    gauges = routed[:, torch.from_numpy(columns).to(dev)].double() * 1.05 + 0.01
    rows.append(case('gauges_gathered', gauges, routed, columns, a.reps, a.warmup))
    del routed, gauges
    torch.cuda.empty_cache()
    rows.append(dict(copy_bandwidth_GBps=engine.copy_bandwidth(0), device=torch.cuda.get_device_name(0)))
    print(json.dumps(rows[-1]), flush=True)
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
