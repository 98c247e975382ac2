"""Forward and backward time of rr.grad.rapid_route on the synthetic network.

    python profiles/microbench/grad_bw.py [--json OUT] [--reps 3] [--warmup 1] [--cases 100k_year,1M_month]

Per case: the forward (rr_rapid_route_dev, the production path, through RapidRoute.forward), the backward
(rr_rapid_adjoint_dev: state tape, reverse ticks, reduction, lateral rows) with gradients for k, x, qlateral and q0 of the
loss sum(W * discharge), and their ratio; HIP events around each, median of `reps` after `warmup` runs.  Also the work memory
of one backward call and the modelled bytes per reach-step of each new kernel (from the kernels' loads and stores; the
downstream reach's values are counted once per reach, as the waves share their lines)."""
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

CASES = {'100k_year': (100_000, 8760, 1, None), '1M_month': (1_000_000, 744, 1, None)}

# bytes per reach-step, from the kernels' loads and stores (8-byte values, 4-byte indices)
MODEL = {
    'k_tick (state tape)': 'lag 4 + child_ptr 4 + c1row/c2/c3/c4 32 + own and upstream state 8 + 2 x 8 / reach + lateral 8 + tape store 8',
    'k_adj_tick': 'lag 4 + down 4 + w/c3 16 + c2[down] 8 + dL/dQ row 8 + own mu 8 + downstream mu 16 + mu store 8',
    'k_adj_reduce': 'mu 8 + own state 8 + upstream states 2 x 8 / reach + lateral 8 (+ lag / child_ptr once per column)',
    'k_adj_rows': 'mu 8 per sub-step + store 8 per row',
}
BYTES = {'k_tick (state tape)': 4 + 4 + 32 + 8 + 16 + 8 + 8, 'k_adj_tick': 4 + 4 + 16 + 8 + 8 + 8 + 16 + 8,
         'k_adj_reduce': 8 + 8 + 16 + 8, 'k_adj_rows': 16}


def run_case(name, n, T, nsub, window, reps, warmup):
    dev = torch.device('cuda', 0)
    net = synth.synth_network(n)
    has = net.down_index >= 0
    indptr = np.concatenate([[0], np.cumsum(has)]).astype(np.int32)
    plan = Plan(indptr, net.down_index[has].astype(np.int32))
    dt_runoff = 3600.0
    ql = synth.synth_qlateral_torch(n, 0, T, dev, dt=dt_runoff) * dt_runoff
    q0 = torch.full((n,), 1.0, dtype=torch.float64, device=dev)
    W = torch.rand((T, n), dtype=torch.float64, device=dev, generator=torch.Generator(dev).manual_seed(7))
    k0, x0 = torch.tensor(net.k), torch.tensor(net.x)
    fwd, bwd = [], []
    for it in range(warmup + reps):
        k = k0.clone().requires_grad_(True)
        x = x0.clone().requires_grad_(True)
        qlt = ql.clone().requires_grad_(True)
        q0t = q0.clone().requires_grad_(True)
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        torch.cuda.synchronize()
        e[0].record()
        d, qf = rr.grad.rapid_route(plan, q0t, qlt, k, x, dt_runoff / nsub, dt_runoff, rows_per_window=window)
        e[1].record()
        loss = (d * W).sum()
        torch.cuda.synchronize()
        e[2].record()
        loss.backward()
        e[3].record()
        torch.cuda.synchronize()
        if it >= warmup:
            fwd.append(e[0].elapsed_time(e[1]))
            bwd.append(e[2].elapsed_time(e[3]))
        del d, qf, loss
    rows = T if window is None else min(T, window)
    out = dict(case=name, reaches=n, rows=T, substeps=nsub, window=window, depth=plan.depth,
               forward_ms=float(np.median(fwd)), backward_ms=float(np.median(bwd)),
               ratio=float(np.median(bwd) / np.median(fwd)), forward_all_ms=fwd, backward_all_ms=bwd,
               work_bytes_per_backward_call=plan.rapid_adjoint_work_bytes(rows, nsub),
               ticks_per_backward_call=2 * (rows * nsub + plan.depth - 1),
               last_forward_kernel=plan.last_kernel())
    out['backward_reach_steps_per_s'] = n * T * nsub / (out['backward_ms'] / 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--json')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--cases', default=','.join(CASES))
    ap.add_argument('--window', type=int, default=0, help='rows per window for every case (0: one call)')
    a = ap.parse_args()
    res = dict(model_bytes_per_reach_step=BYTES, model=MODEL, cases=[])
    for name in a.cases.split(','):
        n, T, nsub, window = CASES[name]
        r = run_case(name, n, T, nsub, a.window or window, a.reps, a.warmup)
        print(json.dumps({k: v for k, v in r.items() if not k.endswith('_all_ms')}), flush=True)
        res['cases'].append(r)
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
