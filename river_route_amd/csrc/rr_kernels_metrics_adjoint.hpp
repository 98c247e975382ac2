// rr_kernels_metrics_adjoint.hpp -- the gradient of a loss through the per-column skill scores of rr_kernels_metrics.hpp
// (river_route/metrics.py) with respect to the simulated rows.
// Part of the translation unit rr_scores.hip builds (included from there, after rr_kernels_metrics.hpp; not a stand-alone header).
#pragma once

namespace {

// Per scored column, field-major ([field][n]) in the caller's work memory: with G the gradient that arrives at the five scores,
//   dL/dp[r] = A + B (t[r] - mt) + P (p[r] - mp) + S sign(t[r] - p[r])
constexpr int kMetricsAdjCoef = 6;      // A, B, P, S, mt, mp
// Rows of both inputs one lane has in flight (the forward's kMetricsBatch).  metrics_split's row ranges are whole chunks, so only
// the last range of a call meets the row-by-row tail loop; any remainder is correct.
constexpr int kMetricsAdjBatch = 8;

struct MAdjCoef {
    double A, B, P, S, mt, mp;
};

__device__ __forceinline__ MAdjCoef madj_load(const double *__restrict__ c, int64_t n, int64_t j)
{
    return MAdjCoef{c[j], c[n + j], c[2 * n + j], c[3 * n + j], c[4 * n + j], c[5 * n + j]};
}

// One element's share: the centred form (an uncentred one cancels for series with a large offset); sign(0) = 0.
// MISSING: exactly 0 where the observation is missing (NaN), whatever the column's constants are (NaN among them), hence a select
// and not a multiply by the flag.
template <bool MISSING>
__device__ __forceinline__ double madj_term(const MAdjCoef &k, double t, double p)
{
    const double d = t - p;
    double v = fma(k.B, t - k.mt, k.A);
    v = fma(k.P, p - k.mp, v);
    v = v + (d > 0.0 ? k.S : (d < 0.0 ? -k.S : 0.0));
    if constexpr (MISSING) return t == t ? v : 0.0;
    else return v;
}

// State and the gradient of the five scores (g[5][n], the rows of k_metrics_finish's out) -> coef[6][n].  Every divide and square
// root of the backward pass is here.  A score whose incoming gradient is exactly 0 adds nothing, whatever its value; where
// k_metrics_finish's rules make a score NaN and its gradient is not 0, A is NaN and so is the column's gradient.  r passes no
// gradient where the unclipped value lies strictly outside [-1, 1] (torch.clamp's rule), in its own score and inside the KGE.
__global__ __launch_bounds__(kBlock) void k_metrics_adjoint_coef(const double *__restrict__ state, const double *__restrict__ g, int64_t n,
                                                                 double *__restrict__ coef)
{
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= n) return;
    const MStat s = mstat_load(state, n, j);
    const double nan = __builtin_nan("");
    const double N = s.cnt;
    const double g_me = g[j], g_mae = g[n + j], g_mse = g[2 * n + j], g_r = g[3 * n + j], g_kge = g[4 * n + j];
    double A = 0.0, B = 0.0, P = 0.0, S = 0.0;
    if (g_me != 0.0) A -= g_me / N;
    if (g_mae != 0.0) S = -g_mae / N;
    if (g_mse != 0.0) {
        const double w = 2.0 * g_mse / N;
        B -= w;
        P += w;
        A -= w * (s.mt - s.mp);
    }
    if (g_r != 0.0 || g_kge != 0.0) {
        const bool has_r = s.m2t > 0.0 && s.m2p > 0.0;
        const double root_t = sqrt(s.m2t), root_p = sqrt(s.m2p);
        const double r_raw = has_r ? s.c / root_t / root_p : nan;      // as k_metrics_finish divides
        const bool clipped = r_raw > 1.0 || r_raw < -1.0;
        const double r = r_raw > 1.0 ? 1.0 : (r_raw < -1.0 ? -1.0 : r_raw);
        const double r_B = clipped ? 0.0 : 1.0 / (root_t * root_p), r_P = clipped ? 0.0 : -r_raw / s.m2p;
        if (g_r != 0.0) {
            if (!has_r) A = nan;
            B = fma(g_r, r_B, B);
            P = fma(g_r, r_P, P);
        }
        if (g_kge != 0.0) {
            const double std_t = sqrt(s.m2t / N), std_p = sqrt(s.m2p / N);
            if (std_t == 0.0 || std_p == 0.0 || s.mt == 0.0) {
                A = nan;
            } else {
                const double beta = s.mp / s.mt, gamma = (s.mp / std_p) / (s.mt / std_t);
                const double E = sqrt((r - 1.0) * (r - 1.0) + (beta - 1.0) * (beta - 1.0) + (gamma - 1.0) * (gamma - 1.0));
                const double cv = std_t / s.mt;
                const double gamma_P = -cv * s.mp / (N * std_p * std_p * std_p), gamma_A = cv / (N * std_p), beta_A = 1.0 / (N * s.mt);
                const double w = -g_kge / E;
                B = fma(w, (r - 1.0) * r_B, B);
                P = fma(w, (r - 1.0) * r_P + (gamma - 1.0) * gamma_P, P);
                A = fma(w, (beta - 1.0) * beta_A + (gamma - 1.0) * gamma_A, A);
            }
        }
    }
    coef[j] = A;
    coef[n + j] = B;
    coef[2 * n + j] = P;
    coef[3 * n + j] = S;
    coef[4 * n + j] = s.mt;
    coef[5 * n + j] = s.mp;
}

// grad[r, c] for rows [y R, y R + R) of the scored columns of y_pred: workgroup (x, y) takes 256 of them, one per lane, so a wave
// reads and writes along rows as k_metrics_partial does.  Without a column map lane u scores column u of y_true against column u
// of y_pred.  With one, lane u owns the u-th distinct scored column ucols[u] of y_pred and the y_true columns order[seg[u]] ..
// order[seg[u + 1] - 1] scored against it (a stable sort of the map: ascending index), whose shares it adds in that order: no
// atomics, and columns of y_pred nobody scores are never written.  The first share's constants stay in registers; those of a
// repeated column are reloaded per batch of rows.  Per element: two loads, two subtractions (the centring), two FMAs, a sign select
// with its add, and one store of y_pred's type; no divide.
// MISSING (rr_kernels_metrics.hpp: mstat_rows): each share is masked by its own y_true element.  Every owned element is stored, a
// skipped one as 0, so without a column map the caller's grad needs no zero fill.
template <bool MISSING, typename TT, typename TP>
__global__ __launch_bounds__(kBlock) void k_metrics_adjoint_rows(const TT *__restrict__ yt, int64_t tpitch, const TP *__restrict__ yp,
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
        for (int i = 0; i < kMetricsAdjBatch; ++i) v[i] = madj_term<MISSING>(k0, (double)xt[i], (double)xp[i]);
        for (int64_t s = s0 + 1; s < s1; ++s) {      // a column of y_pred scored more than once
            const int64_t j = order[s];
            const MAdjCoef k = madj_load(coef, n, j);
            const TT *qt = yt + r * tpitch + j;
#pragma unroll
            for (int i = 0; i < kMetricsAdjBatch; ++i) v[i] += madj_term<MISSING>(k, (double)qt[i * tpitch], (double)xp[i]);
        }
#pragma unroll
        for (int i = 0; i < kMetricsAdjBatch; ++i) pg[i * gpitch] = (TP)v[i];
        pt += kMetricsAdjBatch * tpitch;
        pp += kMetricsAdjBatch * ppitch;
        pg += kMetricsAdjBatch * gpitch;
    }
    for (; r < r1; ++r) {
        const double p = (double)pp[0];
        double v = madj_term<MISSING>(k0, (double)pt[0], p);
        for (int64_t s = s0 + 1; s < s1; ++s) {
            const int64_t j = order[s];
            v += madj_term<MISSING>(madj_load(coef, n, j), (double)yt[r * tpitch + j], p);
        }
        pg[0] = (TP)v;
        pt += tpitch;
        pp += ppitch;
        pg += gpitch;
    }
}

}  // namespace
