// rr_kernels_metrics_members.hpp -- the skill scores of rr_kernels_metrics.hpp (and, with MISSING, of rr_kernels_metrics_missing.hpp)
// for the members of an ensemble in one launch: member m's rows of y_pred lie m * pred_member_pitch elements after member 0's, its
// observations m * true_member_pitch elements after member 0's (pitch 0: one observation block for all members, which then comes
// from L2 / MALL after the first member has read it).  DESIGN.md section 9c.
// Part of the one translation unit rr_engine.hip builds (included from there, LAST; not a stand-alone header): every kernel above
// keeps its place in the code object.
//
// The state is the single-call state over the flattened index f = m * n + j: RR_METRICS_STATE x (members * n) doubles, field-major,
// so k_metrics_merge and k_metrics_finish work on it unchanged with members * n as their column count.
//
// The two row loops are COPIES of k_metrics_partial's and k_metrics_partial_missing's, as __device__ functions: calling such a
// function from the existing kernels as well changed their code (other block layout and register assignment, seen in the
// --cuda-device-only -S output), and those kernels stay exactly as they are (rr_kernels_metrics_missing.hpp says why).  The copies
// keep the chunks, the pivots, the operations and their order, so a member scored here and alone over the same row ranges gives the
// same bits; tests/test_gpu_metrics_members.py holds them to that.  Change one loop: change its twin.
#pragma once

namespace {

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

// The state of rows [r0, r1) of one lane's column, pt and pp at its elements of row r0: k_metrics_partial's loop (MISSING:
// k_metrics_partial_missing's, whose pivot is the chunk's first kept pair and whose flag drives selects, never a branch).
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

// Workgroup x takes columns [256 cb, 256 cb + 256) of member m, x = m * col_blocks + cb, over rows [y R, y R + R), and writes its
// states to slab[y][field][m * n + j].  A workgroup never spans two members, so the member and both member offsets (formed in 64
// bits) are uniform over it; the column map is one for all members.
template <bool MISSING, typename TT, typename TP>
__global__ __launch_bounds__(kBlock) void k_metrics_partial_members(const TT *__restrict__ yt, int64_t tpitch, int64_t tmpitch,
                                                                    const TP *__restrict__ yp, int64_t ppitch, int64_t pmpitch,
                                                                    const int32_t *__restrict__ cols, int64_t n, int64_t col_blocks,
                                                                    int64_t members, int64_t rows, int64_t rows_per_split,
                                                                    double *__restrict__ slab)
{
    const int64_t m = (int64_t)blockIdx.x / col_blocks, cb = (int64_t)blockIdx.x - m * col_blocks;
    const int64_t j = cb * kBlock + threadIdx.x;
    if (j >= n) return;
    const int64_t r0 = (int64_t)blockIdx.y * rows_per_split, r1 = min(rows, r0 + rows_per_split);
    const TT *pt = yt + m * tmpitch + r0 * tpitch + j;
    const TP *pp = yp + m * pmpitch + r0 * ppitch + (cols ? (int64_t)cols[j] : j);
    const int64_t total = members * n;
    const MStat s = mstat_rows<MISSING>(pt, tpitch, pp, ppitch, r0, r1);
    // field k at q[k * total]: mstat_store's layout, written here -- with a call of mstat_store in this kernel the compiler formed the
    // store addresses of k_metrics_partial and k_metrics_partial_missing differently (multiplies for adds); so they stay as they were
    double *q = slab + ((int64_t)blockIdx.y * RR_METRICS_STATE * members + m) * n + j;
    const double field[RR_METRICS_STATE] = {s.cnt, s.mt, s.mp, s.m2t, s.m2p, s.c, s.sd, s.sad, s.sd2};
#pragma unroll
    for (int k = 0; k < RR_METRICS_STATE; ++k, q += total) *q = field[k];
}

}  // namespace
