"""Host-clock times of Plan.set_coeffs and Plan.set_member_coeffs (8 sets) at bench.py's default network size, one process per call of
this script; the library is whichever RR_LIB_PATH names (profiles/coef_tables_refactor_ab.md: a library built from the parent commit and
the tree's own, alternating).  Prints one JSON line.
    PYTHONPATH=. RR_LIB_PATH=<librr_hip.so> python profiles/microbench/coef_setters_ab.py <label> <timed runs>"""
import json
import sys
import time

import numpy as np

from oracle import oracle
from river_route_amd import synth
from river_route_amd.engine import Plan, synchronize

label, runs = sys.argv[1], int(sys.argv[2])
n, M, dt = 1_000_000, 8, 900.0
net = synth.synth_network(n)
has = net.down_index >= 0
indptr = np.concatenate([[0], np.cumsum(has)]).astype(np.int32)
indices = net.down_index[has].astype(np.int32)


def one_set(m):
    c1, c2, c3 = oracle.muskingum_coefficients(net.k * (1 + 0.05 * m), net.x, dt)
    return np.ascontiguousarray(-c1[indices]), c2, c3, (c1 + c2) / dt


sets = [one_set(m) for m in range(M)]
members = [np.ascontiguousarray(np.stack(col)) for col in zip(*sets)]
with Plan(indptr, indices) as plan:
    single, multi = [], []
    for r in range(runs + 1):      # the first of each is the warm-up
        synchronize()
        t0 = time.perf_counter()
        plan.set_coeffs(*sets[r % M])
        single.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        plan.set_member_coeffs(*members)
        multi.append((time.perf_counter() - t0) * 1e3)
    info = plan.tile_info()
print(json.dumps(dict(label=label, n=n, members=M, positions=info['positions'], set_coeffs_ms=[round(v, 3) for v in single[1:]],
                      set_member_coeffs_ms=[round(v, 3) for v in multi[1:]], warmup_ms=[round(single[0], 3), round(multi[0], 3)])))
