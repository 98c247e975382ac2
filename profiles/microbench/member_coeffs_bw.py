"""Parameter ensembles: M coefficient sets on one basin and one forcing, as a generation of a population-based calibration evaluates them.
    baseline   what a user does without them: M x (Plan.set_coeffs + one single-member call), float32 rows in (rapid_route_f32in_dev: the
               same device-resident forcing the candidate reads), float32 means out
    candidate  one Plan.set_member_coeffs + one Plan.rapid_route_members_dev, the forcing shared at pitch 0
Both in one process on one plan, alternating; wall time between device synchronisations (the setters are host work, and part of what is
replaced); median of --reps after one warm-up of each, with the spread.  Float32 means of --factor rows where factor x sub-steps divides
the 128 rows of a record batch, float64 rows otherwise (factor 0 in the output).  One JSON line per shape:
    python profiles/microbench/member_coeffs_bw.py [--n 10000 30000 100000] [--members 16 64] [--shapes 744x1 120x12] [--factor 8] [--reps 3]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))
from oracle import oracle  # noqa: E402
from river_route_amd import synth  # noqa: E402
from river_route_amd.engine import REC_BATCH_ROWS, DeviceBuffer, Plan, synchronize  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, nargs='+', default=[10_000, 30_000, 100_000])
    ap.add_argument('--members', type=int, nargs='+', default=[16, 64])
    ap.add_argument('--shapes', nargs='+', default=['744x1', '120x12'], help='rows x sub-steps')
    ap.add_argument('--factor', type=int, default=8)
    ap.add_argument('--reps', type=int, default=3)
    a = ap.parse_args()
    dt = 3600.0 * 3
    for n in a.n:
        net = synth.synth_network(n, order='random')
        has = net.down_index >= 0
        indptr = np.concatenate([[0], np.cumsum(has)]).astype(np.int32)
        indices = net.down_index[has].astype(np.int32)
        for shape in a.shapes:
            T, nsub = (int(v) for v in shape.split('x'))
            factor = a.factor if a.factor > 0 and REC_BATCH_ROWS % (a.factor * nsub) == 0 and T % a.factor == 0 else 0
            f32_out = factor > 0
            rows, osz = (T // factor, 4) if f32_out else (T, 8)
            ql = (synth.synth_qlateral(n, 0, T, dt=dt) * dt).astype(np.float32)
            for want in a.members:
                with Plan(indptr, indices) as plan:
                    sets = [[], [], [], []]
                    for m in range(want):      # the sets of tests/test_gpu_member_coeffs.py, the shifts scaled to the member count
                        c1, c2, c3 = oracle.muskingum_coefficients(net.k * (1 + 0.6 * m / want), np.clip(net.x + 0.2 * m / want, 0.0, 0.45), dt / nsub)
                        for dst, v in zip(sets, (-c1[indices], c2, c3, (c1 + c2) / dt)):
                            dst.append(v)
                    sets = [np.ascontiguousarray(np.stack(s)) for s in sets]
                    plan.set_member_coeffs(*sets)
                    cap = plan.reserve_ensemble(1, T, nsub, f32_in=True, f32_out=f32_out)['members_max']
                    M = min(want, cap)
                    sets = [s[:M] for s in sets]
                    info = plan.reserve_ensemble(M, T, nsub, f32_in=True, f32_out=f32_out)
                    d_ql = DeviceBuffer(T * n * 4).upload(ql)
                    d_out = DeviceBuffer(M * rows * n * osz)
                    q0 = np.zeros(M * n)
                    d_q = DeviceBuffer(M * n * 8).upload(q0)

                    def loop():
                        for m in range(M):
                            plan.set_coeffs(sets[0][m], sets[1][m], sets[2][m], sets[3][m])
                            out = dict(discharge32=d_out.address + m * rows * n * 4, factor=factor) if f32_out else dict(discharge=d_out.address + m * rows * n * 8, out_rows=T)
                            plan.rapid_route_f32in_dev(d_q.address + m * n * 8, d_ql, T, T, nsub, **out)

                    def members():
                        plan.set_member_coeffs(*sets)
                        plan.rapid_route_members_dev(M, d_q, n, d_ql, True, 0, d_out, f32_out, rows * n, max(1, factor), T, nsub)

                    times, kernels = {'loop': [], 'members': []}, {}
                    for name, fn in (('loop', loop), ('members', members)):      # warm-up: code objects, the reservations of both shapes
                        fn(); synchronize()
                        kernels[name] = plan.last_kernel()
                    for _ in range(a.reps):
                        for name, fn in (('loop', loop), ('members', members)):
                            d_q.upload(q0); synchronize()
                            t0 = time.perf_counter(); fn(); synchronize()
                            times[name].append(time.perf_counter() - t0)
                    # the setters alone: the host share of each side
                    t0 = time.perf_counter()
                    for m in range(M):
                        plan.set_coeffs(sets[0][m], sets[1][m], sets[2][m], sets[3][m])
                    synchronize(); t_set_loop = time.perf_counter() - t0
                    t0 = time.perf_counter(); plan.set_member_coeffs(*sets); synchronize(); t_set_members = time.perf_counter() - t0
                    for b in (d_ql, d_out, d_q):
                        b.free()
                    med = {k: statistics.median(v) for k, v in times.items()}
                    ms = lambda v: round(v * 1e3, 3)      # noqa: E731
                    print(json.dumps(dict(n=n, members=M, members_max=cap, T=T, nsub=nsub, factor=factor, tiles=plan.tile_info()['tiles'], tile_levels=plan.tile_info()['levels'],
                                          pipeline_ticks=info['pipeline_ticks'], loop_ms=ms(med['loop']), loop_min_max_ms=[ms(min(times['loop'])), ms(max(times['loop']))],
                                          members_ms=ms(med['members']), members_min_max_ms=[ms(min(times['members'])), ms(max(times['members']))],
                                          speedup=round(med['loop'] / med['members'], 3), set_coeffs_loop_ms=ms(t_set_loop), set_member_coeffs_ms=ms(t_set_members),
                                          members_reach_steps_per_s=f"{n * T * nsub * M / med['members']:.3e}", kernels=[kernels['loop'], kernels['members']])), flush=True)


if __name__ == '__main__':
    main()
