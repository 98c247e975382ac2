"""Bandwidth of the backward pass of rr.grad.scores on the shapes of metrics_bw.py: a year of 15-minute
steps (35,040 rows) of
  (a) 100,000 float64 columns against 100,000 float64 columns,
  (b) the same in float32,
  (c) 2,000 float64 gauge columns against 2,000 columns (columns=) of a float32 routed array of 1,000,000 columns, or of the widest
      power-of-two fraction of that whose rows and gradient rows both fit in the card's free memory (`pred_columns` says which).

    python profiles/microbench/grad_scores_bw.py [--reps 3] [--warmup 1] [--scale 1.0] [--json out.json]

Times come from HIP events on the stream the work is on, the median of `reps` runs after `warmup` runs of the same shape:
  adjoint   rr_metrics_adjoint_dev alone (k_metrics_adjoint_coef + k_metrics_adjoint_rows; state, work memory and the gradient rows
            allocated beforehand).  Modelled bytes: every element of both inputs read once and one gradient element written, 24 B per
            float64 element, 12 B per float32 one (in (c) the gathered elements only);
  zero_fill the caller's torch.zeros of the gradient rows, which only a column map needs;
  backward  loss.backward() through rr.grad.scores, everything included;
  update    the forward's k_metrics_partial + k_metrics_merge on the same inputs (two reads, no store), as metrics_bw.py times it;
  torch     what this replaces: forward + backward of the scores restated in torch on the same card, with its peak allocation beside
            that of rr.grad.scores (both above the inputs).  Where the restatement does not fit, it runs on the widest power-of-two
            fraction of the columns that does, and `torch_columns` says so: its time and memory grow with the columns.
and engine.copy_bandwidth in the same process."""
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
    return float(np.median(ms))


def torch_scores(t, p):
    """The five scores of every column, as a user restates them today (float64, two-pass moments)."""
    t, p = t.double(), p.double()
    N = t.shape[0]
    d = t - p
    mt, mp = t.mean(0), p.mean(0)
    a, b = t - mt, p - mp
    m2t, m2p, c = (a * a).sum(0), (b * b).sum(0), (a * b).sum(0)
    r = (c / m2t.sqrt() / m2p.sqrt()).clamp(-1.0, 1.0)
    st, sp = (m2t / N).sqrt(), (m2p / N).sqrt()
    kge = 1.0 - ((r - 1.0) ** 2 + (mp / mt - 1.0) ** 2 + ((mp / sp) / (mt / st) - 1.0) ** 2).sqrt()
    return d.mean(0), d.abs().mean(0), (d * d).mean(0), r, kge


def loss_of(s, W):
    return sum((w * v).sum() for w, v in zip(W, s))


def case(name, y_true, y_pred, columns, reps, warmup):
    dev = y_true.device
    stream = torch.cuda.current_stream(dev)
    T, n = y_true.shape
    m = int(y_pred.shape[1])
    W = torch.rand((5, n), dtype=torch.float64, device=dev, generator=torch.Generator(dev).manual_seed(1)) + 0.5
    row = dict(case=name, rows=T, columns=n, true_dtype=str(y_true.dtype), pred_dtype=str(y_pred.dtype), pred_columns=m,
               gathered=columns is not None)
    nbytes = T * n * (y_true.element_size() + 2 * y_pred.element_size())
    row['modelled_bytes'] = nbytes

    # the whole call, and its peak allocation above the inputs
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    p = y_pred.requires_grad_()

    def whole():
        p.grad = None
        loss_of(rr.grad.scores(y_true, p, columns=columns).values(), W).backward()

    row['forward_backward_ms'] = timed(whole, reps, warmup, stream)
    row['peak_bytes_above_inputs'] = int(torch.cuda.max_memory_allocated(dev) - base)
    loss = loss_of(rr.grad.scores(y_true, p, columns=columns).values(), W)

    def backward():
        p.grad = None
        loss.backward(retain_graph=True)

    row['backward_ms'] = timed(backward, reps, warmup, stream)
    p.grad = None
    del loss
    y_pred.requires_grad_(False)

    # the kernels alone
    cols_dev = order = distinct = segments = None
    nd = n
    if columns is not None:
        maps = rr.grad._sorted_columns(columns, n, m)
        nd = len(maps[2])
        maps = torch.from_numpy(np.concatenate(maps)).to(dev)
        cols_dev, order, distinct, segments = rr.grad.column_map_pointers(maps, n, nd)
    state = torch.zeros((engine.METRICS_STATE, n), dtype=torch.float64, device=dev)
    fwork = torch.empty(engine.metrics_work_bytes(n, T) // 8, dtype=torch.float64, device=dev)
    f32 = [t.dtype == torch.float32 for t in (y_true, y_pred)]

    def update():
        engine.metrics_update_dev(n, T, y_true.data_ptr(), f32[0], y_true.stride(0), y_pred.data_ptr(), f32[1], y_pred.stride(0), cols_dev,
                                  state.data_ptr(), fwork.data_ptr(), fwork.numel() * 8, device=dev.index or 0, stream=stream.cuda_stream)

    row['update_ms'] = timed(update, reps, warmup, stream)
    row['update_TBps'] = T * n * (y_true.element_size() + y_pred.element_size()) / (row['update_ms'] * 1e-3) / 1e12
    state.zero_()
    update()
    grad = torch.zeros((T, m), dtype=y_pred.dtype, device=dev)
    work = torch.empty(engine.metrics_adjoint_work_bytes(n) // 8, dtype=torch.float64, device=dev)

    def adjoint():
        engine.metrics_adjoint_dev(n, T, y_true.data_ptr(), f32[0], y_true.stride(0), y_pred.data_ptr(), f32[1], y_pred.stride(0), state, W, nd,
                                   order, distinct, segments, grad, m, work, work.numel() * 8, device=dev.index or 0, stream=stream.cuda_stream)

    row['adjoint_ms'] = timed(adjoint, reps, warmup, stream)
    row['adjoint_TBps'] = nbytes / (row['adjoint_ms'] * 1e-3) / 1e12
    del grad
    if columns is not None:
        row['zero_fill_ms'] = timed(lambda: torch.zeros((T, m), dtype=y_pred.dtype, device=dev), reps, warmup, stream)
        row['zero_fill_TBps'] = T * m * y_pred.element_size() / (row['zero_fill_ms'] * 1e-3) / 1e12
    del state, fwork, work
    torch.cuda.empty_cache()

    # what it replaces; on the columns that fit
    keep = n
    while True:
        yt = y_true[:, :keep]
        cols = None if columns is None else torch.from_numpy(np.asarray(columns)[:keep]).to(dev)
        if columns is None:
            yp = y_pred[:, :keep].detach().requires_grad_()
        else:
            yp = y_pred.detach().requires_grad_()

        def restated():
            yp.grad = None
            loss_of(torch_scores(yt, yp if cols is None else yp[:, cols]), W[:, :keep]).backward()

        try:
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated(dev)
            torch.cuda.reset_peak_memory_stats(dev)
            row['torch_forward_backward_ms'] = timed(restated, reps, warmup, stream)
            row['torch_peak_bytes_above_inputs'] = int(torch.cuda.max_memory_allocated(dev) - base)
            row['torch_columns'] = keep
            break
        except torch.cuda.OutOfMemoryError:
            yp.grad = None
            del yp
            torch.cuda.empty_cache()
            if keep == 1 or columns is not None:
                row['torch_columns'] = 0
                break
            keep = max(1, keep // 2)
    if row['torch_columns']:
        share = row['torch_columns'] / n
        row['torch_over_ours_time'] = row['torch_forward_backward_ms'] / share / row['forward_backward_ms']
        row['torch_over_ours_memory'] = row['torch_peak_bytes_above_inputs'] / share / max(row['peak_bytes_above_inputs'], 1)
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--scale', type=float, default=1.0, help='columns x scale (a quick trial at small sizes)')
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('grad_scores_bw.py: no GPU visible (this measures the device path only)')
    dev = torch.device('cuda', 0)
    g = torch.Generator(device=dev).manual_seed(7)
    T = 35_040
    n = max(1, int(100_000 * a.scale))
    rows = [dict(copy_bandwidth_GBps=engine.copy_bandwidth(0), device=torch.cuda.get_device_name(0))]
    print(json.dumps(rows[-1]), flush=True)
    obs = torch.rand((T, n), generator=g, device=dev, dtype=torch.float64) + 1.0
    sim = 0.9 * obs + 0.1 * torch.rand((T, n), generator=g, device=dev, dtype=torch.float64)
    rows.append(case('dense_f64', obs, sim, None, a.reps, a.warmup))
    obs, sim = obs.float(), sim.float()
    torch.cuda.empty_cache()
    rows.append(case('dense_f32', obs, sim, None, a.reps, a.warmup))
    del obs, sim
    torch.cuda.empty_cache()
    n_routed, n_gauges = max(1, int(1_000_000 * a.scale)), max(1, int(2_000 * a.scale))
    free = torch.cuda.mem_get_info(dev)[0]
    while n_routed > n_gauges and 2.2 * T * n_routed * 4 > free:      # the rows, their gradient, and room for the rest
        n_routed //= 2
    routed = torch.rand((T, n_routed), generator=g, device=dev, dtype=torch.float32)
    columns = np.sort(np.random.default_rng(3).choice(n_routed, n_gauges, replace=False))
    gauges = routed[:, torch.from_numpy(columns).to(dev)].double() * 1.05 + 0.01 * torch.rand((T, n_gauges), generator=g, device=dev, dtype=torch.float64)
    rows.append(case('gauges_gathered', gauges, routed, columns, a.reps, a.warmup))
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
