"""Ensembles: a loop of single-member calls (rr_rapid_route_f32in_dev, float32 rows in and float32 means out) against one batched call
(rr_rapid_route_ensemble_dev) on the same plan and the same device-resident rows.  One JSON line per shape:
    python profiles/microbench/ensemble_bw.py [--n 100000 1000000] [--members 51] [--T 120] [--nsub 12] [--factor 0] [--reps 3]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))
from oracle import oracle  # noqa: E402
from river_route_amd import synth  # noqa: E402
from river_route_amd.engine import DeviceBuffer, Plan, synchronize  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, nargs='+', default=[100_000, 1_000_000])
    ap.add_argument('--members', type=int, default=51)
    ap.add_argument('--T', type=int, nargs='+', default=[120])
    ap.add_argument('--nsub', type=int, nargs='+', default=[12])
    ap.add_argument('--factor', type=int, default=0, help='0: float64 rows out; k: float32 means of k rows (k x nsub must divide 128)')
    ap.add_argument('--reps', type=int, default=3)
    a = ap.parse_args()
    for n in a.n:
        net = synth.synth_network(n, order='random')
        has = net.down_index >= 0
        indptr = np.concatenate([[0], np.cumsum(has)]).astype(np.int32)
        indices = net.down_index[has].astype(np.int32)
        for T in a.T:
            for nsub in a.nsub:
                dt = 3600.0 * 3
                c1, c2, c3 = oracle.muskingum_coefficients(net.k, net.x, dt / nsub)
                with Plan(indptr, indices) as plan:
                    plan.set_coeffs(-c1[indices], c2, c3, (c1 + c2) / dt)
                    f32_out = a.factor > 0
                    cap = plan.reserve_ensemble(1, T, nsub, f32_in=True, f32_out=f32_out)['members_max']
                    M = min(a.members, cap)
                    info = plan.reserve_ensemble(M, T, nsub, f32_in=True, f32_out=f32_out)
                    single = plan.reserve(0, T, nsub, f32_out=f32_out)
                    rows, osz = (T // a.factor, 4) if f32_out else (T, 8)
                    ql = (synth.synth_qlateral(n, 0, T, dt=dt) * dt).astype(np.float32)
                    d_ql = DeviceBuffer(M * T * n * 4)
                    for m in range(M):
                        d_ql.upload(ql, m * T * n * 4)
                    d_out = DeviceBuffer(M * rows * n * osz)
                    d_q = DeviceBuffer(M * n * 8).upload(np.zeros(M * n))

                    def loop():
                        for m in range(M):
                            out = dict(discharge32=d_out.address + m * rows * n * 4, factor=a.factor) if f32_out else dict(discharge=d_out.address + m * rows * n * 8, out_rows=T)
                            plan.rapid_route_f32in_dev(d_q.address + m * n * 8, d_ql.address + m * T * n * 4, T, T, nsub, **out)

                    def batch():
                        plan.rapid_route_ensemble_dev(M, d_q, n, d_ql, True, T * n, d_out, f32_out, rows * n, max(1, a.factor), T, nsub)

                    res = {}
                    for name, fn in (('loop', loop), ('batched', batch)):
                        fn(); synchronize()
                        best = 1e30
                        for _ in range(a.reps):
                            t0 = time.perf_counter(); fn(); synchronize()
                            best = min(best, time.perf_counter() - t0)
                        res[name] = best
                        res[name + '_kernel'] = plan.last_kernel()
                    for b in (d_ql, d_out, d_q):
                        b.free()
                    rs = n * T * nsub * M
                    print(json.dumps(dict(n=n, members=M, members_max=cap, T=T, nsub=nsub, factor=a.factor, tiles_levels=plan.tile_info().get('levels'),
                                          pipeline_ticks=info['pipeline_ticks'], single_kernel=('direct' if single['direct'] else 'tile' if single['tiled'] else 'tick'),
                                          loop_ms=round(res['loop'] * 1e3, 3), batched_ms=round(res['batched'] * 1e3, 3),
                                          speedup=round(res['loop'] / res['batched'], 3), batched_reach_steps_per_s=f"{rs / res['batched']:.3e}",
                                          kernels=[res['loop_kernel'], res['batched_kernel']])), flush=True)


if __name__ == '__main__':
    main()
