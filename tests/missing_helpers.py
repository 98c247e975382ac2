"""What the skip_missing= tests share: the one gap pattern every GPU shape carries, numpy on each column's kept pairs (the
reference of the scores) and the masked float64 restatement of test_grad_scores.dense_scores (the reference of the gradient)."""
import warnings

import numpy as np

import river_route_amd as rr

SCORES = rr.metrics.SCORES


def gap_mask(T, n, seed):
    """missing[T, n]: 30 % of the elements at random (seeded), with these columns overwritten wherever the shape has them:
    0 gap-free; 1 rows 32..127 missing (whole chunks, whole row splits of narrow inputs); 2 row 0 of every 32-row chunk missing
    (the pivot row); 3 the last row missing (the tail chunk); 4 only row 5 kept (N = 1); 5 nothing kept (N = 0)."""
    miss = np.random.default_rng(seed).random((T, n)) < 0.3
    if n > 0:
        miss[:, 0] = False
    if n > 1:
        miss[:, 1] = False
        miss[32:128, 1] = True
    if n > 2:
        miss[:, 2] = False
        miss[0::32, 2] = True
    if n > 3:
        miss[:, 3] = False
        miss[T - 1, 3] = True
    if n > 4:
        miss[:, 4] = True
        miss[5:6, 4] = False
    if n > 5:
        miss[:, 5] = True
    return miss


def with_gaps(obs, miss):
    out = np.array(obs)
    out[miss] = np.nan
    return out


def host_scores_kept(y_true, y_pred, columns=None):
    """The host 1-D path (the reference's numpy calls) on each column's kept pairs of the float64 data, and the pairs kept."""
    t = np.asarray(y_true, dtype=np.float64)
    p = np.asarray(y_pred, dtype=np.float64)
    p = p[:, columns] if columns is not None else p
    fns = [rr.metrics.me, rr.metrics.mae, rr.metrics.mse, rr.metrics.pearson_r, rr.metrics.kge2012]
    out = {k: np.full(t.shape[1], np.nan) for k in SCORES}
    keep = ~np.isnan(t)
    with warnings.catch_warnings(), np.errstate(all='ignore'):
        warnings.simplefilter('ignore')
        for j in range(t.shape[1]):
            if keep[:, j].any():
                tj, pj = np.ascontiguousarray(t[keep[:, j], j]), np.ascontiguousarray(p[keep[:, j], j])
                for k, f in zip(SCORES, fns):
                    out[k][j] = f(tj, pj)
    out['count'] = keep.sum(0).astype(np.float64)
    return out


def dense_scores_missing(t, p):
    """test_grad_scores.dense_scores over the pairs whose t is not NaN (float64 torch tensors): torch.where on the mask,
    N = mask.sum(0).  p at a skipped element is never looked at and gets the gradient 0."""
    import torch
    mask = ~torch.isnan(t)
    N = mask.sum(0).to(t.dtype)
    zero = torch.zeros_like(t)
    tz, pz = torch.where(mask, t, zero), torch.where(mask, p, zero)
    d = tz - pz
    mt, mp = tz.sum(0) / N, pz.sum(0) / N
    a, b = torch.where(mask, tz - mt, zero), torch.where(mask, pz - mp, zero)
    m2t, m2p, c = (a * a).sum(0), (b * b).sum(0), (a * b).sum(0)
    r = (c / m2t.sqrt() / m2p.sqrt()).clamp(-1.0, 1.0)
    st, sp = (m2t / N).sqrt(), (m2p / N).sqrt()
    beta, gamma = mp / mt, (mp / sp) / (mt / st)
    kge = 1.0 - ((r - 1.0) ** 2 + (beta - 1.0) ** 2 + (gamma - 1.0) ** 2).sqrt()
    undefined = (st == 0) | (sp == 0) | (mt == 0)
    kge = kge + torch.where(undefined, torch.full_like(kge, float('nan')), torch.zeros_like(kge))
    return {'me': d.sum(0) / N, 'mae': d.abs().sum(0) / N, 'mse': (d * d).sum(0) / N, 'pearson_r': r, 'kge2012': kge}
