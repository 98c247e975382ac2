// rr_kernels_metrics_missing.hpp -- the skill scores of rr_kernels_metrics.hpp and their gradient (rr_kernels_metrics_adjoint.hpp)
// over gauge records with gaps: element (r, j) is missing when y_true[r, j] is NaN, and the pair (y_true[r, j], y_pred[r, col[j]])
// is then left out of column j's sums and gets no gradient (DESIGN.md sections 9 and 12c, "Missing observations").
// Part of the one translation unit rr_engine.hip builds (included from there, after every kernel but those of
// rr_kernels_metrics_members.hpp; not a stand-alone header).
//
// The two row loops of k_metrics_partial and k_metrics_adjoint_rows are restated here, not shared through a template parameter:
// kernels lie in the code object in the order they are first named and the routing kernels' speed depends on their place, so the
// existing kernels and their instantiations stay exactly as they are and these come after all of them.  The state (MStat), its
// merge, k_metrics_merge, k_metrics_finish, k_metrics_adjoint_coef and madj_term are the existing ones: they divide by the state's
// own count, which here is the number of kept pairs.
#pragma once

namespace {

// k_metrics_partial with pairs left out: the same grid, column map, row splits and slab layout, the same chunks of kMetricsChunk
// rows with kMetricsBatch rows of both inputs loaded before the first is used.  Every load is issued whether the pair is kept or
// not (the bytes moved are the unmasked kernel's) and the validity flag drives selects, never a branch: the lanes of a wave have
// different gaps.  A skipped pair adds 0 to every shifted sum and to the count, and its y_pred is never looked at.
// The pivot of a chunk's shifted sums is its first KEPT pair: any kept value would do, the first makes a gap-free column repeat
// k_metrics_partial's sums operation by operation, and a NaN is never a pivot.  The chunk's state has cnt = the pairs kept, its
// means and M2 come from the shifted sums with one divide per chunk; a chunk that keeps nothing gives the all-zero empty state,
// which mstat_merge skips, so a column missing for a whole split leaves that split's slab state all-zero.
template <typename TT, typename TP>
__global__ __launch_bounds__(kBlock) void k_metrics_partial_missing(const TT *__restrict__ yt, int64_t tpitch, const TP *__restrict__ yp,
                                                                    int64_t ppitch, const int32_t *__restrict__ cols, int64_t n,
                                                                    int64_t rows, int64_t rows_per_split, double *__restrict__ slab)
{
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= n) return;
    const int64_t r0 = (int64_t)blockIdx.y * rows_per_split, r1 = min(rows, r0 + rows_per_split);
    const TT *pt = yt + r0 * tpitch + j;
    const TP *pp = yp + r0 * ppitch + (cols ? (int64_t)cols[j] : j);
    MStat s = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int64_t r = r0; r < r1; r += kMetricsChunk) {
        const int m = (int)min((int64_t)kMetricsChunk, r1 - r);
        double kt = 0, kp = 0;      // the pivot, once `kept` is not 0
        int kept = 0;
        double st = 0, sp = 0, stt = 0, spp = 0, stp = 0, sd = 0, sad = 0, sd2 = 0;
        auto body = [&](TT xt, TP xp) {
            const bool ok = xt == xt;      // the element as stored; inf is kept
            const bool first = ok && kept == 0;
            const double t = (double)xt, p = (double)xp;
            kt = first ? t : kt;
            kp = first ? p : kp;
            kept += ok ? 1 : 0;
            const double a = ok ? t - kt : 0.0, b = ok ? p - kp : 0.0, d = ok ? t - p : 0.0;
            st += a;
            sp += b;
            stt = fma(a, a, stt);
            spp = fma(b, b, spp);
            stp = fma(a, b, stp);
            sd += d;
            sad += fabs(d);
            sd2 = fma(d, d, sd2);
        };
        if (m == kMetricsChunk) {
            // all kMetricsBatch rows' loads are issued before the first is used: 2 x kMetricsBatch loads in flight per lane
            for (int i0 = 0; i0 < kMetricsChunk; i0 += kMetricsBatch) {
                TT xt[kMetricsBatch];
                TP xp[kMetricsBatch];
#pragma unroll
                for (int i = 0; i < kMetricsBatch; ++i) {
                    xt[i] = pt[(i0 + i) * tpitch];
                    xp[i] = pp[(i0 + i) * ppitch];
                }
#pragma unroll
                for (int i = 0; i < kMetricsBatch; ++i) body(xt[i], xp[i]);
            }
        } else {
            for (int i = 0; i < m; ++i) body(pt[i * tpitch], pp[i * ppitch]);
        }
        pt += m * tpitch;
        pp += m * ppitch;
        // shifted sums -> (mean, M2, C) of the kept pairs; nothing kept: every sum and both pivots are 0, inv = 0 keeps the state
        // all-zero.  Rounding can leave an M2 a hair below zero (NaN stays NaN).
        const double inv = kept > 0 ? 1.0 / kept : 0.0;
        MStat b;
        b.cnt = kept;
        b.mt = kt + st * inv;
        b.mp = kp + sp * inv;
        b.m2t = fma(-st * inv, st, stt);
        b.m2p = fma(-sp * inv, sp, spp);
        b.c = fma(-st * inv, sp, stp);
        if (b.m2t < 0.0) b.m2t = 0.0;
        if (b.m2p < 0.0) b.m2p = 0.0;
        b.sd = sd;
        b.sad = sad;
        b.sd2 = sd2;
        mstat_merge(s, b);
    }
    mstat_store(s, slab + (int64_t)blockIdx.y * RR_METRICS_STATE * n, n, j);
}

// One share of a gradient element: exactly 0 where the observation is missing, whatever the column's constants are (NaN among
// them), hence a select and not a multiply by the flag.
__device__ __forceinline__ double madj_term_missing(const MAdjCoef &k, double t, double p)
{
    const double v = madj_term(k, t, p);
    return t == t ? v : 0.0;
}

// k_metrics_adjoint_rows with each share masked by its own y_true element: the same lanes, row ranges, column map and order of
// the shares.  Every owned element is stored, a skipped one as 0, so without a column map the caller's grad needs no zero fill.
template <typename TT, typename TP>
__global__ __launch_bounds__(kBlock) void k_metrics_adjoint_rows_missing(const TT *__restrict__ yt, int64_t tpitch, const TP *__restrict__ yp,
                                                                         int64_t ppitch, const double *__restrict__ coef, int64_t n,
                                                                         const int32_t *__restrict__ order, const int32_t *__restrict__ ucols,
                                                                         const int32_t *__restrict__ seg, int64_t n_lanes, int64_t rows,
                                                                         int64_t rows_per_split, TP *__restrict__ grad, int64_t gpitch)
{
    const int64_t u = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (u >= n_lanes) return;
    const int64_t r0 = (int64_t)blockIdx.y * rows_per_split, r1 = min(rows, r0 + rows_per_split);
    const int64_t s0 = seg ? (int64_t)seg[u] : u, s1 = seg ? (int64_t)seg[u + 1] : u + 1;
    const int64_t j0 = order ? (int64_t)order[s0] : s0, c = ucols ? (int64_t)ucols[u] : u;
    const MAdjCoef k0 = madj_load(coef, n, j0);
    const TT *pt = yt + r0 * tpitch + j0;
    const TP *pp = yp + r0 * ppitch + c;
    TP *pg = grad + r0 * gpitch + c;
    int64_t r = r0;
    for (; r + kMetricsAdjBatch <= r1; r += kMetricsAdjBatch) {
        // all loads of the batch are issued before the first is used: 2 x kMetricsAdjBatch in flight per lane
        TT xt[kMetricsAdjBatch];
        TP xp[kMetricsAdjBatch];
#pragma unroll
        for (int i = 0; i < kMetricsAdjBatch; ++i) {
            xt[i] = pt[i * tpitch];
            xp[i] = pp[i * ppitch];
        }
        double v[kMetricsAdjBatch];
#pragma unroll
        for (int i = 0; i < kMetricsAdjBatch; ++i) v[i] = madj_term_missing(k0, (double)xt[i], (double)xp[i]);
        for (int64_t s = s0 + 1; s < s1; ++s) {      // a column of y_pred scored more than once: each share by its own y_true column
            const int64_t j = order[s];
            const MAdjCoef k = madj_load(coef, n, j);
            const TT *qt = yt + r * tpitch + j;
#pragma unroll
            for (int i = 0; i < kMetricsAdjBatch; ++i) v[i] += madj_term_missing(k, (double)qt[i * tpitch], (double)xp[i]);
        }
#pragma unroll
        for (int i = 0; i < kMetricsAdjBatch; ++i) pg[i * gpitch] = (TP)v[i];
        pt += kMetricsAdjBatch * tpitch;
        pp += kMetricsAdjBatch * ppitch;
        pg += kMetricsAdjBatch * gpitch;
    }
    for (; r < r1; ++r) {
        const double p = (double)pp[0];
        double v = madj_term_missing(k0, (double)pt[0], p);
        for (int64_t s = s0 + 1; s < s1; ++s) {
            const int64_t j = order[s];
            v += madj_term_missing(madj_load(coef, n, j), (double)yt[r * tpitch + j], p);
        }
        pg[0] = (TP)v;
        pt += tpitch;
        pp += ppitch;
        pg += gpitch;
    }
}

}  // namespace
