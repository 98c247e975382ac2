"""Backward time of rr.grad.unit_route_batch against the loop of rr.grad.unit_route backward passes over the same members
 on the synthetic network.

    python profiles/microbench/grad_unit_batch_bw.py [--json OUT] [--reps 5] [--warmup 1] [--cases 100k_month_b4,...]

--json adds to a file that exists, so the cases can be run one process each into one file.

Per case: B members with their own lateral rows and states, one k and x.  `loop`: B calls of rr.grad.unit_route, each with its own
backward pass (rr_unit_adjoint_dev; the path as it was before the batched call existed).  `batched`: one rr.grad.unit_route_batch call
and one backward pass (rr_unit_adjoint_batch_dev).  The loss is sum(W * discharge) with gradients for k, x, lateral, q_ch0 and q_full0;
HIP events around the forward and the backward of each, median of `reps` after `warmup` runs.  The single-member figures of the loop
are printed too (compare profiles/grad_unit_bw.json before trusting the ratio), and the work memory of each call."""
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

# reaches, rows, sub-steps, members
CASES = {'100k_month_b4': (100_000, 720, 1, 4), '100k_month_b8': (100_000, 720, 1, 8), '100k_month_b16': (100_000, 720, 1, 16),
         '1M_month_b2': (1_000_000, 744, 1, 2), '100k_year_b4': (100_000, 8760, 1, 4)}
# not in the default list: a small case to try the script on
EXTRA = {'10k_day_b3': (10_000, 24, 1, 3)}
DT_RUNOFF = 3600.0


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def run_case(name, n, T, nsub, B, reps, warmup):
    dev = torch.device('cuda', 0)
    net = synth.synth_network(n)
    has = net.down_index >= 0
    indptr = np.concatenate([[0], np.cumsum(has)]).astype(np.int32)
    plan = Plan(indptr, net.down_index[has].astype(np.int32))
    # one copy of the rows for both paths (at 100k x 8,760 x 4 they are 28 GB beside 116 GB of tapes): each run takes leaves that share it
    ql = torch.empty((B, T, n), dtype=torch.float64, device=dev)
    for m in range(B):
        ql[m] = synth.synth_qlateral_torch(n, m * T, (m + 1) * T, dev, dt=DT_RUNOFF) * DT_RUNOFF
    ni = plan.n_inner
    qc0 = torch.full((B, ni), 1.0, dtype=torch.float64, device=dev)
    qf0 = torch.full((B, ni), 2.0, dtype=torch.float64, device=dev)
    W = torch.rand((B, T, n), dtype=torch.float64, device=dev, generator=torch.Generator(dev).manual_seed(7))
    k0, x0 = torch.tensor(net.k), torch.tensor(net.x)
    dt = DT_RUNOFF / nsub
    t = dict(loop_forward=[], loop_backward=[], single_backward=[], batched_forward=[], batched_backward=[])
    for it in range(warmup + reps):
        keep = it >= warmup
        # the loop: one call and one backward pass per member
        k, x = k0.clone().requires_grad_(True), x0.clone().requires_grad_(True)
        fwd = bwd = 0.0
        for m in range(B):
            qlt, qct, qft = (v[m].detach().requires_grad_(True) for v in (ql, qc0, qf0))
            ms, (d, _, _) = timed(lambda: rr.grad.unit_route(plan, qct, qft, qlt, k, x, dt, DT_RUNOFF))
            fwd += ms
            loss = (d * W[m]).sum()
            ms, _ = timed(loss.backward)
            bwd += ms
            if keep:
                t['single_backward'].append(ms)
            del d, loss, qlt, qct, qft
        if keep:
            t['loop_forward'].append(fwd)
            t['loop_backward'].append(bwd)
        # batched
        k, x = k0.clone().requires_grad_(True), x0.clone().requires_grad_(True)
        qlt, qct, qft = (v.detach().requires_grad_(True) for v in (ql, qc0, qf0))
        fwd, (d, _, _) = timed(lambda: rr.grad.unit_route_batch(plan, qct, qft, qlt, k, x, dt, DT_RUNOFF))
        loss = (d * W).sum()
        bwd, _ = timed(loss.backward)
        if keep:
            t['batched_forward'].append(fwd)
            t['batched_backward'].append(bwd)
        del d, loss, qlt, qct, qft
    med = {key + '_ms': float(np.median(v)) for key, v in t.items()}
    out = dict(case=name, reaches=n, rows=T, substeps=nsub, members=B, depth=plan.depth, **med,
               backward_loop_over_batched=med['loop_backward_ms'] / med['batched_backward_ms'],
               all_ms={key: v for key, v in t.items() if key != 'single_backward'},
               work_bytes_single_call=plan.unit_adjoint_work_bytes(T, nsub),
               work_bytes_batched_call=plan.unit_adjoint_batch_work_bytes(B, T, nsub),
               tick_launches_batched=2 * (T * nsub + plan.depth - 1), tick_launches_loop=2 * B * (T * nsub + plan.depth - 1),
               last_forward_kernel=plan.last_kernel())
    out['batched_backward_reach_steps_per_s'] = B * n * T * nsub / (out['batched_backward_ms'] / 1e3)
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
