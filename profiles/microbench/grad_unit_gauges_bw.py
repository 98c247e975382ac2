"""Backward time and peak memory of a calibration step through rr.grad.unit_route with a loss at gauged reaches only: the dense path
(discharge[:, gauges] of the full-width call) against gauges= on the synthetic network.

    python profiles/microbench/grad_unit_gauges_bw.py [--json OUT] [--reps 5] [--warmup 1] [--cases 100k_month,...]

--json adds to a file that exists, so the cases can be run one process each into one file.

Per case: k and x require grad, the lateral rows and the states do not (the calibration case: no grad_lateral), the loss is
sum(W * discharge at the gauges).  `dense`: rr.grad.unit_route, the gauge columns indexed out of its (T, n) discharge; autograd hands
rr_unit_adjoint_dev a zero-filled (T, n) cotangent.  `gauges`: rr.grad.unit_route(..., gauges=), rr_unit_adjoint_gauges_dev on the
(T, G) cotangent.  Both in one process, alternating; HIP events around the forward and around loss.backward() of each, median of `reps`
after `warmup` runs; torch.cuda.max_memory_allocated of the backward pass, and of forward and backward together, above what the
inputs hold."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import river_route_amd as rr  # noqa: E402
from river_route_amd import synth  # noqa: E402
from river_route_amd.engine import Plan  # noqa: E402

# reaches, rows, sub-steps, gauges
CASES = {'100k_month': (100_000, 720, 1, 2000), '100k_year': (100_000, 8760, 1, 2000), '1M_month': (1_000_000, 744, 1, 2000)}
EXTRA = {'tiny': (3000, 48, 2, 16)}      # not in the default list: a rehearsal size
DT_RUNOFF = 3600.0


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def run_case(name, n, T, nsub, G, reps, warmup):
    dev = torch.device('cuda', 0)
    net = synth.synth_network(n)
    has = net.down_index >= 0
    indptr = np.concatenate([[0], np.cumsum(has)]).astype(np.int32)
    plan = Plan(indptr, net.down_index[has].astype(np.int32))
    ql = synth.synth_qlateral_torch(n, 0, T, dev, dt=DT_RUNOFF) * DT_RUNOFF
    qc0 = torch.full((plan.n_inner,), 1.0, dtype=torch.float64, device=dev)
    qf0 = torch.full((plan.n_inner,), 2.0, dtype=torch.float64, device=dev)
    gauges = np.random.default_rng(11).permutation(n)[:G]      # distinct, not ascending
    gauges_dev = torch.as_tensor(gauges, device=dev)
    W = torch.rand((T, G), dtype=torch.float64, device=dev, generator=torch.Generator(dev).manual_seed(7))
    k0, x0 = torch.tensor(net.k), torch.tensor(net.x)
    dt = DT_RUNOFF / nsub

    def forward(path, k, x):
        if path == 'gauges':
            return rr.grad.unit_route(plan, qc0, qf0, ql, k, x, dt, DT_RUNOFF, gauges=gauges)[0]
        return rr.grad.unit_route(plan, qc0, qf0, ql, k, x, dt, DT_RUNOFF)[0][:, gauges_dev]

    t = {f'{p}_{w}': [] for p in ('dense', 'gauges') for w in ('forward', 'backward')}
    peak, grads = {}, {}
    for it in range(warmup + reps):
        for path in ('dense', 'gauges'):
            k, x = k0.clone().requires_grad_(True), x0.clone().requires_grad_(True)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            inputs_bytes = torch.cuda.memory_allocated(dev)
            fwd, d = timed(lambda: forward(path, k, x))
            loss = (d * W).sum()
            torch.cuda.synchronize()
            held = torch.cuda.memory_allocated(dev)
            peak_forward = torch.cuda.max_memory_allocated(dev)
            torch.cuda.reset_peak_memory_stats(dev)
            bwd, _ = timed(loss.backward)
            peak_backward = torch.cuda.max_memory_allocated(dev)
            if it >= warmup:
                t[f'{path}_forward'].append(fwd)
                t[f'{path}_backward'].append(bwd)
            peak[path] = dict(kept_between_forward_and_backward_bytes=held - inputs_bytes, backward_peak_rise_bytes=peak_backward - held,
                              peak_above_inputs_bytes=max(peak_forward, peak_backward) - inputs_bytes)
            grads[path] = (k.grad.clone(), x.grad.clone())
            del d, loss, k, x
    med = {key + '_ms': float(np.median(v)) for key, v in t.items()}
    same = all(bool(torch.equal(a, b)) for a, b in zip(grads['dense'], grads['gauges']))
    hw_gauges = int(np.isin(gauges, np.flatnonzero(np.bincount(net.down_index[has], minlength=n) == 0)).sum())
    out = dict(case=name, reaches=n, rows=T, substeps=nsub, gauges=G, headwater_gauges=hw_gauges, depth=plan.depth, **med,
               backward_dense_over_gauges=med['dense_backward_ms'] / med['gauges_backward_ms'], all_ms=t,
               dense=peak['dense'], gauges_path=peak['gauges'], gradients_bit_equal=same,
               work_bytes_dense=plan.unit_adjoint_work_bytes(T, nsub),
               work_bytes_gauges=plan.unit_adjoint_gauges_work_bytes(1, G, T, nsub, False),
               cotangent_bytes_dense=8 * T * n, cotangent_bytes_gauges=8 * T * G, last_forward_kernel=plan.last_kernel())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--json')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--cases', default=','.join(CASES))
    a = ap.parse_args()
    # a file that is there already is added to (a case measured again replaces its entry): the cases can run one process each
    res = dict(cases=[])
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
