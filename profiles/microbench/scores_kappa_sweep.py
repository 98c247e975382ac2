"""Where the GPU scores lose rtol 1e-10: rr.metrics.scores on columns of kappa = |mean| / std from 1 to 1e10, against the long-double
arbiter (oracle/rr_oracle_scores.c), next to the host 1-D path (numpy, two-pass) on the same columns.  DESIGN.md sections 2d and 9.

    python profiles/microbench/scores_kappa_sweep.py [T] [columns per decade]

One line per decade: the worst error of each score over the columns, me / mae / mse relative (me: of mae), pearson_r absolute, kge2012
of |r| + |beta| + |gamma|, each in units of u = 2^-53 and, for r and kge, of u (kappa_t + kappa_p)."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [REPO, os.path.join(REPO, 'tests')]

import per_column as pc      # noqa: E402
import river_route_amd as rr      # noqa: E402


def main():
    T = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
    cols = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    rng = np.random.default_rng(9)
    print(f'T = {T}, {cols} columns per decade; errors in u = 2^-53 (r, kge also in u (kappa_t + kappa_p))')
    print('kappa | gpu me mae mse | gpu r (abs, /u kappa) | gpu kge (abs/S, /u kappa) | host r | host kge')
    for decade in range(0, 11):
        kappa = 10.0 ** decade
        sigma = 10.0 ** rng.uniform(-1, 1, cols)
        x = (rng.gamma(2.0, 0.5, (T, cols)) - 1.0) / np.sqrt(0.5)
        t = sigma * (kappa + x)
        p = sigma * (kappa * rng.uniform(0.8, 1.2, cols) + rng.uniform(0.6, 1.4, cols) * x + rng.normal(0.0, 0.3, (T, cols)))
        ref = pc.ScoreRef(t, p)
        gpu = pc.score_errors(rr.metrics.scores(t, p), ref.arb)
        host = pc.score_errors(ref.host, ref.arb)
        uk = pc.U * ref.kappa
        print(f'1e{decade} | ' + ' '.join(f'{gpu[k].max() / pc.U:.2f}' for k in ('me', 'mae', 'mse'))
              + f" | {gpu['pearson_r'].max():.3g} = {gpu['pearson_r'].max() / pc.U:.3g} u, {(gpu['pearson_r'] / uk).max():.3f}"
              + f" | {gpu['kge2012'].max():.3g} = {gpu['kge2012'].max() / pc.U:.3g} u, {(gpu['kge2012'] / uk).max():.3f}"
              + f" | {host['pearson_r'].max():.3g} | {host['kge2012'].max():.3g}")


if __name__ == '__main__':
    main()
