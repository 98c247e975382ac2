/*
 * rr_oracle_scores.c -- the arbiter of the skill scores and of their gradient: the five per-column scores of rr.metrics
 * (river_route_amd/metrics.py: me, mae, mse, pearson_r, kge2012) and dL/dy_pred of a loss through them,
 * in long double with every sum Neumaier-compensated, each output rounded to double once.
 *
 * TEST INFRASTRUCTURE ONLY, as rr_oracle.c: nothing under river_route_amd/ may import, link or call this file.
 *
 * The specification is the documented rules of river_route_amd/metrics.py and k_metrics_finish, not the kernels' arithmetic:
 *   - two passes: the means first, then the deviations a = t - mt, b = p - mp, then the corrected moments
 *     M2t = sum a^2 - (sum a)^2 / N,  M2p likewise,  C = sum a b - (sum a)(sum b) / N  (the correction removes what the rounding of
 *     the long-double mean leaves);  a column whose kept values are all equal has M2 = 0 and its mean is that value, exactly;
 *   - r = C / sqrt(M2t) / sqrt(M2p), clipped to [-1, 1], NaN when an M2 is 0;  standard deviations with ddof 0;
 *     beta = mp / mt, gamma = (mp / sp) / (mt / st) (the reference's inverse CV ratio);  KGE = 1 - sqrt((r-1)^2 + (beta-1)^2 + (gamma-1)^2),
 *     NaN when st, sp or mt is 0;  no pair: all five NaN;
 *   - skip_missing: a pair whose y_true is NaN as stored is left out of every sum; y_pred there is never looked at.
 * Inputs are the doubles the GPU gets (float32 data: widened by the caller).  Column j of y_true (T x n, row-major) is scored against
 * column cols[j] of y_pred (T x m), or column j without a map (then m == n).
 *
 * orcl_scores: out[SC_ROWS][n], the rows of enum below.
 * orcl_scores_grad: with G[5][n] = dL/d(me, mae, mse, r, kge) the closed form of section 12c on the long-double moments,
 *     dL/dp[r] = A + B (t[r] - mt) + P (p[r] - mp) + S sign(t[r] - p[r]),
 *   grad[T][m] (shares of a repeated column added in ascending j), scale[T][m] = the sum over the shares of
 *   |A| + |B (t - mt)| + |P (p - mp)| + |S|, and bm[n] = |B mt| + |P mp| per scored column.  A score whose incoming gradient is exactly 0
 *   adds nothing; where the rules above make a score NaN and its gradient is not 0, A is NaN.  A skipped element adds exactly 0.
 *   The clamp of r follows torch.clamp: no gradient where the unclipped value lies strictly outside [-1, 1].  In exact arithmetic
 *   it never does (Cauchy-Schwarz), so an unclipped value that long-double rounding leaves a hair outside is treated as +-1 on the
 *   boundary, where the gradient passes.
 *
 * Errors: -1 allocation, -5 a column index outside [0, m).
 */
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

_Static_assert(LDBL_MANT_DIG >= 64, "the scores arbiter needs a long double wider than double");

typedef long double LD;

enum { SC_COUNT, SC_ME, SC_MAE, SC_MSE, SC_R, SC_KGE, SC_MT, SC_MP, SC_KAPPA_T, SC_KAPPA_P, SC_BETA, SC_GAMMA, SC_R_RAW, SC_ROWS };

/* Neumaier's compensated sum: the running sum and what its additions lost */
typedef struct { LD s, c; } NSum;

static inline void nadd(NSum *a, LD x)
{
    const LD t = a->s + x;
    if (fabsl(a->s) >= fabsl(x)) a->c += (a->s - t) + x;
    else a->c += (x - t) + a->s;
    a->s = t;
}

static inline LD nval(const NSum *a) { return a->s + a->c; }

typedef struct {
    LD N, mt, mp, m2t, m2p, c, sd, sad, sd2;
    /* finished */
    LD r_raw, r, st, sp, beta, gamma, kge;
    int has_r, has_kge;
} Mom;

static inline int kept(double t, int skip) { return !(skip && t != t); }

static void col_moments(int64_t T, const double *t, int64_t ts, const double *p, int64_t ps, int skip, Mom *o)
{
    NSum st = {0, 0}, sp = {0, 0}, sd = {0, 0}, sad = {0, 0}, sd2 = {0, 0};
    int64_t cnt = 0;
    double t0 = 0, p0 = 0;
    int same_t = 1, same_p = 1;
    for (int64_t r = 0; r < T; ++r) {
        const double x = t[r * ts];
        if (!kept(x, skip)) continue;
        const double y = p[r * ps];
        if (cnt == 0) t0 = x, p0 = y;
        same_t &= x == t0;
        same_p &= y == p0;
        ++cnt;
        const LD d = (LD)x - (LD)y;
        nadd(&st, x);
        nadd(&sp, y);
        nadd(&sd, d);
        nadd(&sad, fabsl(d));
        nadd(&sd2, d * d);
    }
    const LD N = (LD)cnt;
    o->N = N;
    o->sd = nval(&sd), o->sad = nval(&sad), o->sd2 = nval(&sd2);
    o->mt = cnt ? (same_t ? (LD)t0 : nval(&st) / N) : 0;
    o->mp = cnt ? (same_p ? (LD)p0 : nval(&sp) / N) : 0;
    NSum a1 = {0, 0}, b1 = {0, 0}, aa = {0, 0}, bb = {0, 0}, ab = {0, 0};
    for (int64_t r = 0; r < T; ++r) {
        const double x = t[r * ts];
        if (!kept(x, skip)) continue;
        const LD a = (LD)x - o->mt, b = (LD)p[r * ps] - o->mp;
        nadd(&a1, a);
        nadd(&b1, b);
        nadd(&aa, a * a);
        nadd(&bb, b * b);
        nadd(&ab, a * b);
    }
    o->m2t = o->m2p = o->c = 0;
    if (cnt) {
        const LD sa = nval(&a1), sb = nval(&b1);
        if (!same_t) o->m2t = nval(&aa) - sa * sa / N;
        if (!same_p) o->m2p = nval(&bb) - sb * sb / N;
        if (!same_t && !same_p) o->c = nval(&ab) - sa * sb / N;
        if (o->m2t < 0) o->m2t = 0;
        if (o->m2p < 0) o->m2p = 0;
    }
    /* k_metrics_finish's rules */
    o->has_r = cnt && o->m2t > 0 && o->m2p > 0;
    o->r_raw = o->has_r ? o->c / sqrtl(o->m2t) / sqrtl(o->m2p) : (LD)NAN;
    o->r = o->r_raw > 1 ? 1 : (o->r_raw < -1 ? -1 : o->r_raw);
    o->st = cnt ? sqrtl(o->m2t / N) : (LD)NAN;
    o->sp = cnt ? sqrtl(o->m2p / N) : (LD)NAN;
    o->has_kge = cnt && !(o->st == 0 || o->sp == 0 || o->mt == 0);
    o->beta = o->gamma = o->kge = (LD)NAN;
    if (o->has_kge) {
        o->beta = o->mp / o->mt;
        o->gamma = (o->mp / o->sp) / (o->mt / o->st);
        o->kge = 1 - sqrtl((o->r - 1) * (o->r - 1) + (o->beta - 1) * (o->beta - 1) + (o->gamma - 1) * (o->gamma - 1));
    }
}

static int check_cols(int64_t n, int64_t m, const int32_t *cols)
{
    if (!cols) return n == m ? 0 : -5;
    for (int64_t j = 0; j < n; ++j)
        if (cols[j] < 0 || cols[j] >= m) return -5;
    return 0;
}

int orcl_scores(int64_t T, int64_t n, const double *yt, const double *yp, int64_t m, const int32_t *cols, int skip, double *out)
{
    if (check_cols(n, m, cols)) return -5;
    for (int64_t j = 0; j < n; ++j) {
        Mom q;
        col_moments(T, yt + j, n, yp + (cols ? cols[j] : j), m, skip, &q);
        const int any = q.N > 0;
        out[SC_COUNT * n + j] = (double)q.N;
        out[SC_ME * n + j] = any ? (double)(q.sd / q.N) : NAN;
        out[SC_MAE * n + j] = any ? (double)(q.sad / q.N) : NAN;
        out[SC_MSE * n + j] = any ? (double)(q.sd2 / q.N) : NAN;
        out[SC_R * n + j] = (double)q.r;
        out[SC_KGE * n + j] = (double)q.kge;
        out[SC_MT * n + j] = any ? (double)q.mt : NAN;
        out[SC_MP * n + j] = any ? (double)q.mp : NAN;
        out[SC_KAPPA_T * n + j] = any ? (double)(fabsl(q.mt) / q.st) : NAN;
        out[SC_KAPPA_P * n + j] = any ? (double)(fabsl(q.mp) / q.sp) : NAN;
        out[SC_BETA * n + j] = (double)q.beta;
        out[SC_GAMMA * n + j] = (double)q.gamma;
        out[SC_R_RAW * n + j] = (double)q.r_raw;
    }
    return 0;
}

int orcl_scores_grad(int64_t T, int64_t n, const double *yt, const double *yp, int64_t m, const int32_t *cols, int skip, const double *G,
                     double *grad, double *scale, double *bm)
{
    if (check_cols(n, m, cols)) return -5;
    LD *acc = calloc((size_t)(2 * T * m > 0 ? 2 * T * m : 1), sizeof(LD));      /* the shares of a repeated column add up in long double */
    if (!acc) return -1;
    LD *ag = acc, *as = acc + T * m;
    for (int64_t j = 0; j < n; ++j) {
        const int64_t c = cols ? cols[j] : j;
        Mom q;
        col_moments(T, yt + j, n, yp + c, m, skip, &q);
        const LD N = q.N, g_me = G[j], g_mae = G[n + j], g_mse = G[2 * n + j], g_r = G[3 * n + j], g_kge = G[4 * n + j];
        LD A = 0, B = 0, P = 0, S = 0;
        if (N > 0) {
            if (g_me != 0) A -= g_me / N;
            if (g_mae != 0) S = -g_mae / N;
            if (g_mse != 0) {
                const LD w = 2 * g_mse / N;
                B -= w;
                P += w;
                A -= w * (q.mt - q.mp);
            }
            /* on the boundary the clamp passes the gradient (header comment) */
            const LD r_B = q.has_r ? 1 / (sqrtl(q.m2t) * sqrtl(q.m2p)) : 0, r_P = q.has_r ? -q.r / q.m2p : 0;
            if (g_r != 0) {
                if (!q.has_r) A = (LD)NAN;
                B += g_r * r_B;
                P += g_r * r_P;
            }
            if (g_kge != 0) {
                if (!q.has_kge) {
                    A = (LD)NAN;
                } else {
                    const LD E = sqrtl((q.r - 1) * (q.r - 1) + (q.beta - 1) * (q.beta - 1) + (q.gamma - 1) * (q.gamma - 1));
                    const LD cv = q.st / q.mt;
                    const LD gamma_P = -cv * q.mp / (N * q.sp * q.sp * q.sp), gamma_A = cv / (N * q.sp), beta_A = 1 / (N * q.mt);
                    const LD w = -g_kge / E;
                    B += w * (q.r - 1) * r_B;
                    P += w * ((q.r - 1) * r_P + (q.gamma - 1) * gamma_P);
                    A += w * ((q.beta - 1) * beta_A + (q.gamma - 1) * gamma_A);
                }
            }
        }
        bm[j] = (double)(fabsl(B * q.mt) + fabsl(P * q.mp));
        for (int64_t r = 0; r < T; ++r) {
            const double x = yt[r * n + j];
            if (!kept(x, skip)) continue;
            const LD y = yp[r * m + c], d = (LD)x - y;
            const LD tb = B * ((LD)x - q.mt), tp = P * (y - q.mp), ts = d > 0 ? S : (d < 0 ? -S : 0);
            ag[r * m + c] += A + tb + tp + ts;
            as[r * m + c] += fabsl(A) + fabsl(tb) + fabsl(tp) + fabsl(S);
        }
    }
    for (int64_t i = 0; i < T * m; ++i) {
        grad[i] = (double)ag[i];
        scale[i] = (double)as[i];
    }
    free(acc);
    return 0;
}
