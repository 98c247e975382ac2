// rr_kernels_metrics.hpp -- per-column skill scores (river_route/metrics.py) of (time, reach) rows already on the device.
// Part of the translation unit rr_scores.hip builds (included from there, after rr_common.hpp; not a stand-alone header).
#pragma once

namespace {

// Per-column state, RR_METRICS_STATE doubles per column, stored field-major ([field][n]) so every access is coalesced:
// the count, both means, both M2 (sum of squared deviations), the co-moment C = sum (t - mean_t)(p - mean_p), and the
// plain sums of d, |d| and d^2 with d = true - pred.  All-zero is the empty state.  Two states merge exactly
// (Chan, Golub & LeVeque's pairwise update), so a series may arrive in any number of row blocks.
struct MStat {
    double cnt, mt, mp, m2t, m2p, c, sd, sad, sd2;
};
static_assert(sizeof(MStat) == RR_METRICS_STATE * sizeof(double), "state layout");

// Rows one thread folds between two merges: the chunk's first row is the pivot of its shifted sums, so the per-element
// loop is adds and FMAs only; the one divide of a merge is paid once per chunk.
constexpr int kMetricsChunk = 32;
constexpr int kMetricsBatch = 8;
// Workgroups one update aims for (about eight per CU): narrow inputs split their rows over this many.
constexpr int64_t kMetricsTargetBlocks = 2048;

__device__ __forceinline__ MStat mstat_load(const double *__restrict__ s, int64_t n, int64_t j)
{
    return MStat{s[j], s[n + j], s[2 * n + j], s[3 * n + j], s[4 * n + j], s[5 * n + j], s[6 * n + j], s[7 * n + j], s[8 * n + j]};
}

__device__ __forceinline__ void mstat_store(const MStat &m, double *__restrict__ s, int64_t n, int64_t j)
{
    s[j] = m.cnt;
    s[n + j] = m.mt;
    s[2 * n + j] = m.mp;
    s[3 * n + j] = m.m2t;
    s[4 * n + j] = m.m2p;
    s[5 * n + j] = m.c;
    s[6 * n + j] = m.sd;
    s[7 * n + j] = m.sad;
    s[8 * n + j] = m.sd2;
}

// a <- a merged with b (a's rows first).  An empty side is skipped or copied as it is, so a state's first block keeps
// its exact means and an exactly constant column keeps M2 == 0.
__device__ __forceinline__ void mstat_merge(MStat &a, const MStat &b)
{
    if (b.cnt == 0.0) return;
    if (a.cnt == 0.0) { a = b; return; }
    const double nn = a.cnt + b.cnt, f = b.cnt / nn, w = a.cnt * f;
    const double dt = b.mt - a.mt, dp = b.mp - a.mp;
    a.mt += dt * f;
    a.mp += dp * f;
    a.m2t += b.m2t + dt * dt * w;
    a.m2p += b.m2p + dp * dp * w;
    a.c += b.c + dt * dp * w;
    a.cnt = nn;
    a.sd += b.sd;
    a.sad += b.sad;
    a.sd2 += b.sd2;
}

// The shifted sums of one chunk -> its state: cnt pairs, (mean, M2, C) with one divide (inv = 1 / cnt, or 0 for no pair: the
// all-zero empty state).  Rounding can leave an M2 a hair below zero (NaN stays NaN).
__device__ __forceinline__ MStat mstat_of_chunk(double cnt, double inv, double kt, double kp, double st, double sp, double stt, double spp,
                                                double stp, double sd, double sad, double sd2)
{
    MStat b;
    b.cnt = cnt;
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
    return b;
}

// The state of rows [r0, r1) of one lane's column, pt and pp at its elements of row r0: the one row loop of the scores.  Every
// element is widened to double on load.  The chunk's first row is the pivot of its shifted sums.
// MISSING (gauge records with gaps, DESIGN.md section 9 "Missing observations"): element (r, j) is missing when y_true[r, j] is NaN,
// and the pair is then left out of the column's sums.  Every load is issued whether the pair is kept or not (the bytes moved are the
// unmasked loop's) and the validity flag drives selects, never a branch: the lanes of a wave have different gaps.  A skipped pair
// adds 0 to every shifted sum and to the count, and its y_pred is never looked at.  The pivot is the chunk's first KEPT pair: any
// kept value would do, the first makes a gap-free column repeat the unmasked sums operation by operation, and a NaN is never a
// pivot.  A chunk that keeps nothing gives the all-zero empty state, which mstat_merge skips.
template <bool MISSING, typename TT, typename TP>
__device__ __forceinline__ MStat mstat_rows(const TT *__restrict__ pt, int64_t tpitch, const TP *__restrict__ pp, int64_t ppitch, int64_t r0,
                                            int64_t r1)
{
    MStat s = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int64_t r = r0; r < r1; r += kMetricsChunk) {
        const int m = (int)min((int64_t)kMetricsChunk, r1 - r);
        double kt = 0, kp = 0;      // the pivot: the first row (MISSING: the first kept pair, once `kept` is not 0)
        int kept = 0;
        if constexpr (!MISSING) {
            kt = (double)pt[0];
            kp = (double)pp[0];
        }
        double st = 0, sp = 0, stt = 0, spp = 0, stp = 0, sd = 0, sad = 0, sd2 = 0;
        auto body = [&](TT xt, TP xp) {
            const double t = (double)xt, p = (double)xp;
            double a, b, d;
            if constexpr (MISSING) {
                const bool ok = xt == xt;      // the element as stored; inf is kept
                const bool first = ok && kept == 0;
                kt = first ? t : kt;
                kp = first ? p : kp;
                kept += ok ? 1 : 0;
                a = ok ? t - kt : 0.0, b = ok ? p - kp : 0.0, d = ok ? t - p : 0.0;
            } else {
                a = t - kt, b = p - kp, d = t - p;
            }
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
        if constexpr (MISSING)
            mstat_merge(s, mstat_of_chunk(kept, kept > 0 ? 1.0 / kept : 0.0, kt, kp, st, sp, stt, spp, stp, sd, sad, sd2));
        else
            mstat_merge(s, mstat_of_chunk(m, m == kMetricsChunk ? 1.0 / kMetricsChunk : 1.0 / m, kt, kp, st, sp, stt, spp, stp, sd, sad, sd2));
    }
    return s;
}

// Partial states of one launch, for the members of an ensemble (one member: a single series).  Workgroup x
// takes columns [256 cb, 256 cb + 256) of member m, x = m * col_blocks + cb, over rows [y R, y R + R), and writes its states to
// slab[y][field][m * n + j].  Member m's rows of y_pred lie m * pmpitch elements after member 0's, its observations m * tmpitch
// after member 0's (pitch 0: one observation block for all members, which comes from L2 / MALL after the first member has read it).
// A workgroup never spans two members, so the member and both member offsets (formed in 64 bits) are uniform over it; the column map
// is one for all members.  Lane j reads y_true[r, j] and y_pred[r, col[j]]: along a row, so the true rows (and the predicted rows
// without a column map) are read coalesced.  The state is the single-series state over the flattened index f = m * n + j, so
// k_metrics_merge and k_metrics_finish work on it with members * n as their column count.
template <bool MISSING, typename TT, typename TP>
__global__ __launch_bounds__(kBlock) void k_metrics_partial(const TT *__restrict__ yt, int64_t tpitch, int64_t tmpitch,
                                                            const TP *__restrict__ yp, int64_t ppitch, int64_t pmpitch,
                                                            const int32_t *__restrict__ cols, int64_t n, int64_t col_blocks, int64_t members,
                                                            int64_t rows, int64_t rows_per_split, double *__restrict__ slab)
{
    const int64_t m = (int64_t)blockIdx.x / col_blocks, cb = (int64_t)blockIdx.x - m * col_blocks;
    const int64_t j = cb * kBlock + threadIdx.x;
    if (j >= n) return;
    const int64_t r0 = (int64_t)blockIdx.y * rows_per_split, r1 = min(rows, r0 + rows_per_split);
    const TT *pt = yt + m * tmpitch + r0 * tpitch + j;
    const TP *pp = yp + m * pmpitch + r0 * ppitch + (cols ? (int64_t)cols[j] : j);
    const MStat s = mstat_rows<MISSING>(pt, tpitch, pp, ppitch, r0, r1);
    mstat_store(s, slab + ((int64_t)blockIdx.y * RR_METRICS_STATE * members + m) * n, members * n, j);
}

// state[j] <- state[j] merged with the slab's partial states, folded in split order: the result depends on the inputs
// and the sequence of updates only, never on which workgroup finished first.  Narrow inputs have few lanes and many
// splits (2,000 columns: 8 workgroups folding 219 states each), so the next split's state is loaded while the current
// one merges instead of after it.  The fold order is the same either way.
__global__ __launch_bounds__(kBlock) void k_metrics_merge(const double *__restrict__ slab, int64_t splits, int64_t n,
                                                          double *__restrict__ state)
{
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= n) return;
    const int64_t step = RR_METRICS_STATE * n;
    MStat acc = mstat_load(slab, n, j);
    MStat next = splits > 1 ? mstat_load(slab + step, n, j) : acc;
    for (int64_t s = 1; s < splits; ++s) {
        const MStat cur = next;
        if (s + 1 < splits) next = mstat_load(slab + (s + 1) * step, n, j);
        mstat_merge(acc, cur);
    }
    MStat a = mstat_load(state, n, j);
    mstat_merge(a, acc);
    mstat_store(a, state, n, j);
}

// State -> out[5][n]: mean error, mean absolute error, mean square error, Pearson r, KGE-2012, with the reference's
// rules: r is clipped to [-1, 1] (np.corrcoef) and is NaN when either M2 is 0; the KGE standard deviations use ddof 0,
// KGE is NaN when std_true, std_pred or mean_true is 0, and gamma = (mean_pred / std_pred) / (mean_true / std_true)
// as the reference writes it.  No rows: all NaN.  NaN in a column's rows reaches all five through the sums.
__global__ __launch_bounds__(kBlock) void k_metrics_finish(const double *__restrict__ state, int64_t n, double *__restrict__ out)
{
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= n) return;
    const MStat s = mstat_load(state, n, j);
    const double nan = __builtin_nan("");
    const double N = s.cnt;
    out[0 * n + j] = s.sd / N;
    out[1 * n + j] = s.sad / N;
    out[2 * n + j] = s.sd2 / N;
    double r = (s.m2t > 0.0 && s.m2p > 0.0) ? s.c / sqrt(s.m2t) / sqrt(s.m2p) : nan;
    r = r > 1.0 ? 1.0 : (r < -1.0 ? -1.0 : r);
    out[3 * n + j] = r;
    const double std_t = sqrt(s.m2t / N), std_p = sqrt(s.m2p / N);
    double kge = nan;
    if (!(std_t == 0.0 || std_p == 0.0 || s.mt == 0.0)) {
        const double beta = s.mp / s.mt, gamma = (s.mp / std_p) / (s.mt / std_t);
        kge = 1.0 - sqrt((r - 1.0) * (r - 1.0) + (beta - 1.0) * (beta - 1.0) + (gamma - 1.0) * (gamma - 1.0));
    }
    out[4 * n + j] = kge;
}

// How an update of `rows` rows of n columns is cut: splits x rows_per_split, rows_per_split a whole number of chunks.
// A function of (n, rows) only, so rr_metrics_work_bytes and the update agree and a repeated update repeats its sums.
// members > 1: one row range takes members x ceil(n / 256) workgroups, a function of (n, members, rows).
inline void metrics_split(int64_t n, int64_t rows, int64_t &splits, int64_t &rows_per_split, int64_t members = 1)
{
    const int64_t col_blocks = members * ((n + kBlock - 1) / kBlock);
    const int64_t chunks = (rows + kMetricsChunk - 1) / kMetricsChunk;
    const int64_t want = std::max<int64_t>(1, (kMetricsTargetBlocks + col_blocks - 1) / col_blocks);
    splits = std::max<int64_t>(1, std::min(want, chunks));
    rows_per_split = (chunks + splits - 1) / splits * kMetricsChunk;
    splits = std::max<int64_t>(1, (rows + rows_per_split - 1) / rows_per_split);
}

}  // namespace
