"""Scores of a generation of members at its gauges, two comparisons, both sides alternating in one process; wall
time between device synchronisations, median of --reps after one warm-up of each, with the spread.  One JSON line per shape.

(a) --part update: the update alone, on device-resident tensors: G gauge columns gathered from the (M, rows, n) float32 rows of M members
    against one shared (rows, G) float64 observation block.
    loop     M x (rr.metrics.Accumulator construction + rr_metrics_update_dev [or _missing_dev] + rr_metrics_finish_dev), as a loop of
             rr.metrics.scores calls on member m's rows does it
    members  one rr.metrics.MemberAccumulator construction + rr_metrics_update_members_dev + rr_metrics_finish_dev(M * G)

(b) --part generation: what a calibration pays per generation of M (k, x) sets on one basin and one shared float32 forcing, 744 rows x
    1 sub-step, float32 means of 8 rows, the setters excluded on all sides (set_member_coeffs once, before the timed region).
    host     what a user does without the new call: Plan.rapid_route_members into a host array + M rr.metrics.scores calls on host arrays
    device   Plan.rapid_route_members_dev into a torch tensor + M rr.metrics.scores calls on device tensors
    scores   Plan.rapid_route_members_scores

    python profiles/microbench/members_scores_bw.py [--part update generation] [--n 10000 100000] [--gen-n 10000 30000 100000]
           [--rows 744 8760] [--members 16 64] [--gauges 2000] [--reps 3]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))
import river_route_amd as rr  # noqa: E402
from oracle import oracle  # noqa: E402
from river_route_amd import synth  # noqa: E402
from river_route_amd.engine import Plan, synchronize  # noqa: E402


def timed(sides, reps, before=None):
    """{name: [seconds]} of each side, alternating, after one warm-up of each."""
    times = {name: [] for name, _ in sides}
    for _, fn in sides:
        fn(); synchronize()
    for _ in range(reps):
        for name, fn in sides:
            if before:
                before()
            synchronize()
            t0 = time.perf_counter(); fn(); synchronize()
            times[name].append(time.perf_counter() - t0)
    return times


def summary(times):
    ms = lambda v: round(v * 1e3, 3)      # noqa: E731
    out = {}
    for k, v in times.items():
        out[f'{k}_ms'] = ms(statistics.median(v))
        out[f'{k}_min_max_ms'] = [ms(min(v)), ms(max(v))]
    return out


def row_split_excess(many, single, m, rtol=1e-12):
    """The largest |members call - single call| of member m over the project's bound for two cuts of the same rows (the `check` rule of
    tests/test_gpu_metrics.py at rtol 1e-12: relative, plus rtol x mae for me and rtol x max|score| for pearson_r and kge2012); <= 1: within."""
    worst = 0.0
    for k in rr.metrics.SCORES:
        g, w = many[k][m], single[k]
        ok = ~w.isnan()
        if not bool((g.isnan() == w.isnan()).all()):
            return float('inf')
        if k == 'me':
            atol = rtol * single['mae'][ok].abs()
        elif k in ('pearson_r', 'kge2012'):
            atol = rtol * (w[ok].abs().max() if bool(ok.any()) else 0.0)
        else:
            atol = 0.0
        bound = rtol * w[ok].abs() + atol
        err = (g[ok] - w[ok]).abs()
        if err.numel():
            worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
    return worst


def part_update(a):
    import torch
    dev = torch.device('cuda', 0)
    for n in a.n:
        for rows in a.rows:
            for M in a.members:
                if M * rows * n * 4 > a.max_gb * 1e9:
                    print(json.dumps(dict(part='update', n=n, rows=rows, members=M, skipped=f'{M * rows * n * 4 / 1e9:.1f} GB of rows')), flush=True)
                    continue
                g = torch.Generator(device=dev).manual_seed(n + rows + M)
                pred = torch.rand((M, rows, n), generator=g, device=dev, dtype=torch.float32) + 1.0
                cols = np.sort(np.random.default_rng(1).choice(n, a.gauges, replace=False))
                obs = (pred[0][:, torch.from_numpy(cols).to(dev)].double() * 1.1 + 0.05 * torch.randn((rows, a.gauges), generator=g, device=dev, dtype=torch.float64))
                gappy = obs.clone()
                gappy[torch.rand(obs.shape, generator=g, device=dev) < 0.3] = float('nan')
                for skip_missing in (False, True):
                    y_true = gappy if skip_missing else obs

                    def loop():
                        return [rr.metrics.scores(y_true, pred[m], columns=cols, skip_missing=skip_missing) for m in range(M)]

                    def members():
                        return rr.metrics.scores_members(y_true, pred, columns=cols, skip_missing=skip_missing)
                    one, many = loop(), members()
                    same = all(torch.equal(many[k][m].view(torch.int64), one[m][k].view(torch.int64)) for m in range(M) for k in many)
                    worst = max(row_split_excess(many, one[m], m) for m in range(M))
                    t = timed((('loop', loop), ('members', members)), a.reps)
                    med = {k: statistics.median(v) for k, v in t.items()}
                    print(json.dumps(dict(part='update', n=n, gauges=a.gauges, rows=rows, members=M, skip_missing=skip_missing, **summary(t),
                                          speedup=round(med['loop'] / med['members'], 3), bit_identical=same, worst_error_over_row_split_bound=round(worst, 4),
                                          gathered_GBps=round(M * rows * a.gauges * 4 / med['members'] / 1e9, 1))), flush=True)
                del pred, obs, gappy
                torch.cuda.empty_cache()


def part_generation(a):
    import torch
    dev = torch.device('cuda', 0)
    dt, T, nsub, factor = 3600.0 * 3, 744, 1, 8
    rows = T // factor
    for n in a.gen_n:
        net = synth.synth_network(n, order='random')
        has = net.down_index >= 0
        indptr = np.concatenate([[0], np.cumsum(has)]).astype(np.int32)
        indices = net.down_index[has].astype(np.int32)
        ql = (synth.synth_qlateral(n, 0, T, dt=dt) * dt).astype(np.float32)
        G = min(a.gauges, n)
        gauges = np.sort(np.random.default_rng(2).choice(n, G, replace=False))
        for want in a.members:
            with Plan(indptr, indices) as plan:
                sets = [[], [], [], []]
                for m in range(want):      # the sets of profiles/microbench/member_coeffs_bw.py
                    c1, c2, c3 = oracle.muskingum_coefficients(net.k * (1 + 0.6 * m / want), np.clip(net.x + 0.2 * m / want, 0.0, 0.45), dt / nsub)
                    for dst, v in zip(sets, (-c1[indices], c2, c3, (c1 + c2) / dt)):
                        dst.append(v)
                sets = [np.ascontiguousarray(np.stack(s)) for s in sets]
                plan.set_member_coeffs(*sets)
                cap = plan.reserve_ensemble(1, T, nsub, f32_in=True, f32_out=True)['members_max']
                M = min(want, cap)
                if M < want:
                    plan.set_member_coeffs(*(s[:M] for s in sets))
                q0 = np.zeros((M, n))
                out = np.empty((M, rows, n), np.float32)
                plan.rapid_route_members(q0, ql, out, nsub, factor=factor)
                observed = out[M // 2][:, gauges].astype(np.float64) * 1.1 + 0.01
                d_ql, d_obs = torch.from_numpy(ql).to(dev), torch.from_numpy(observed).to(dev)
                d_out = torch.empty((M, rows, n), dtype=torch.float32, device=dev)
                d_q = torch.zeros((M, n), dtype=torch.float64, device=dev)

                def host():
                    plan.rapid_route_members(q0, ql, out, nsub, factor=factor)
                    return [rr.metrics.scores(observed, out[m], columns=gauges) for m in range(M)]

                def device():
                    d_q.zero_()
                    torch.cuda.current_stream().synchronize()      # (the routing call below is enqueued on the null stream)
                    plan.rapid_route_members_dev(M, d_q.data_ptr(), n, d_ql.data_ptr(), True, 0, d_out.data_ptr(), True, rows * n, factor, T, nsub)
                    res = [rr.metrics.scores(d_obs, d_out[m], columns=gauges) for m in range(M)]
                    return {k: torch.stack([r[k] for r in res]).cpu().numpy() for k in rr.metrics.SCORES}, d_q.cpu().numpy()

                def scores():
                    return plan.rapid_route_members_scores(q0, ql, observed, gauges, nsub, factor=factor)
                by_host, (by_device, _), (by_call, _) = host(), device(), scores()
                same = all(by_call[k][m].tobytes() == by_host[m][k].tobytes() == by_device[k][m].tobytes() for m in range(M) for k in rr.metrics.SCORES)
                t = timed((('host', host), ('device', device), ('scores', scores)), a.reps)
                med = {k: statistics.median(v) for k, v in t.items()}
                print(json.dumps(dict(part='generation', n=n, tiles=plan.tile_info()['tiles'], gauges=G, T=T, nsub=nsub, factor=factor, members=M,
                                      members_max=cap, **summary(t), speedup_over_host=round(med['host'] / med['scores'], 3),
                                      speedup_over_device=round(med['device'] / med['scores'], 3), bit_identical=same)), flush=True)
                del d_ql, d_obs, d_out, d_q
                torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--part', nargs='+', default=['update', 'generation'], choices=['update', 'generation'])
    ap.add_argument('--n', type=int, nargs='+', default=[10_000, 100_000])
    ap.add_argument('--gen-n', type=int, nargs='+', default=[10_000, 30_000, 100_000])
    ap.add_argument('--rows', type=int, nargs='+', default=[744, 8760])
    ap.add_argument('--members', type=int, nargs='+', default=[16, 64])
    ap.add_argument('--gauges', type=int, default=2000)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--max-gb', type=float, default=150.0, help='leave out update shapes whose member rows exceed this')
    a = ap.parse_args()
    if 'update' in a.part:
        part_update(a)
    if 'generation' in a.part:
        part_generation(a)


if __name__ == '__main__':
    main()
