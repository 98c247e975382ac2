"""Forward and backward time of rr.grad.unit_muskingum on the synthetic network, beside the Rapid adjoint
on the same shape in the same process, and rr_uh_adjoint_dev alone as bytes moved over time.

    python profiles/microbench/grad_unit_bw.py [--json OUT] [--reps 3] [--warmup 1] [--cases 100k_year,config4]

Per case: forward (rr_uh_convolve_dev + rr_unit_route_dev per window) and backward (rr_unit_adjoint_dev + rr_uh_adjoint_dev per
window) of the loss sum(discharge) with gradients for k, x, depth, uh_kernel, uh_state, q_ch0 and q_full0; the same for
rr.grad.rapid_route with the same rows as qlateral and the same windows (the yardstick); then the convolution's adjoint alone with
the bytes it must move at least (dL/dconvolved read once, depth read once, dL/ddepth written once, kernel read and dL/dkernel
written once) and rr_copy_bandwidth over the same number of bytes.  HIP events, median of `reps` after `warmup` runs.  The loss is
a plain sum so that its gradient is an expanded scalar: at 1M reaches x 3,504 rows every (T, n) array is 28 GB."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import river_route_amd as rr  # noqa: E402
from river_route_amd import engine, synth  # noqa: E402
from river_route_amd.engine import Plan  # noqa: E402

# reaches, rows, sub-steps, kernel steps, rows per window (None: one call)
CASES = {'100k_year': (100_000, 8760, 1, 48, None), 'config4': (1_000_000, 3504, 1, 48, 438)}


def timed(fn_forward, reps, warmup):
    fwd, bwd = [], []
    for it in range(warmup + reps):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        torch.cuda.synchronize()
        e[0].record()
        d, leaves = fn_forward()
        e[1].record()
        loss = d.sum()
        torch.cuda.synchronize()
        e[2].record()
        loss.backward()
        e[3].record()
        torch.cuda.synchronize()
        if it >= warmup:
            fwd.append(e[0].elapsed_time(e[1]))
            bwd.append(e[2].elapsed_time(e[3]))
        del d, loss, leaves
    return fwd, bwd


def run_case(name, n, T, nsub, n_ks, window, reps, warmup):
    dev = torch.device('cuda', 0)
    net = synth.synth_network(n)
    has = net.down_index >= 0
    indptr = np.concatenate([[0], np.cumsum(has)]).astype(np.int32)
    plan = Plan(indptr, net.down_index[has].astype(np.int32))
    dt_runoff = 3600.0
    g = torch.Generator(dev).manual_seed(1234)
    depth = torch.rand((T, n), dtype=torch.float64, device=dev, generator=g) * 1e-3
    kern = torch.from_numpy(synth.synth_uh_kernel(n, n_ks, tr=dt_runoff / nsub)).to(dev)
    state = torch.zeros_like(kern)
    qc0 = torch.zeros(plan.n_inner, dtype=torch.float64, device=dev)
    q0 = torch.zeros(n, dtype=torch.float64, device=dev)
    k0, x0 = torch.tensor(net.k), torch.tensor(net.x)
    leaf = lambda t: t.clone().requires_grad_(True)      # noqa: E731

    def unit_forward():
        lv = [leaf(t) for t in (qc0, qc0, depth, kern, state, k0, x0)]
        d = rr.grad.unit_muskingum(plan, *lv, dt_runoff / nsub, dt_runoff, rows_per_window=window)[0]
        return d, lv

    def rapid_forward():
        lv = [leaf(t) for t in (q0, depth, k0, x0)]
        d = rr.grad.rapid_route(plan, *lv, dt_runoff / nsub, dt_runoff, rows_per_window=window)[0]
        return d, lv

    ufwd, ubwd = timed(unit_forward, reps, warmup)
    unit_kernel = plan.last_kernel()
    rfwd, rbwd = timed(rapid_forward, reps, warmup)
    rows = T if window is None else min(T, window)
    out = dict(case=name, reaches=n, rows=T, substeps=nsub, uh_steps=n_ks, window=window, depth=plan.depth,
               unit_forward_ms=float(np.median(ufwd)), unit_backward_ms=float(np.median(ubwd)), unit_backward_all_ms=ubwd,
               rapid_forward_ms=float(np.median(rfwd)), rapid_backward_ms=float(np.median(rbwd)), rapid_backward_all_ms=rbwd,
               unit_over_rapid_backward=float(np.median(ubwd) / np.median(rbwd)),
               unit_work_bytes_per_backward_call=plan.unit_adjoint_work_bytes(rows, nsub),
               uh_work_bytes_per_backward_call=engine.uh_adjoint_work_bytes(rows, n_ks, n),
               ticks_per_backward_call=2 * (rows * nsub + plan.depth - 1), last_forward_kernel=unit_kernel)

    # the convolution's adjoint alone, one window's rows
    f64 = dict(dtype=torch.float64, device=dev)
    gconv = torch.rand((rows, n), generator=g, **f64)
    gdepth, gkern = torch.empty((rows, n), **f64), torch.empty((n_ks, n), **f64)
    nbytes = engine.uh_adjoint_work_bytes(rows, n_ks, n)
    work = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    ms = {}
    for what, args in (('depth', (gdepth, None)), ('kernel', (None, gkern)), ('both', (gdepth, gkern))):
        t = []
        for it in range(warmup + reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            engine.uh_adjoint_dev(kern, depth[:rows], gconv, None, args[0], args[1], None, work, nbytes, rows, n_ks, n, 0, stream)
            b.record()
            torch.cuda.synchronize()
            if it >= warmup:
                t.append(a.elapsed_time(b))
        ms[what] = float(np.median(t))
    must = dict(depth=8 * n * (2 * rows + n_ks), kernel=8 * n * (2 * rows + n_ks), both=8 * n * (3 * rows + 2 * n_ks))
    out['uh_adjoint'] = {w: dict(ms=ms[w], min_bytes=must[w], gbps_of_min_bytes=must[w] / ms[w] / 1e6) for w in ms}
    out['copy_gbps_same_bytes'] = engine.copy_bandwidth(0, min(must['both'], 4 << 30), 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--json')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--cases', default=','.join(CASES))
    a = ap.parse_args()
    res = dict(cases=[])
    for name in a.cases.split(','):
        r = run_case(name, *CASES[name], a.reps, a.warmup)
        print(json.dumps({k: v for k, v in r.items() if not k.endswith('_all_ms')}), flush=True)
        res['cases'].append(r)
        torch.cuda.empty_cache()
        if a.json:      # after every case: the large one may not fit beside other work on the card
            with open(a.json, 'w') as f:
                json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
