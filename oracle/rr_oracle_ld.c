/*
 * rr_oracle_ld.c -- the extended-precision arbiter: the four loops of rr_oracle.c (rapid_route, muskingum_route,
 * unit_route, uh_convolve) with the same statements in the same order, carried in long double.
 *
 * TEST INFRASTRUCTURE ONLY, as rr_oracle.c: nothing under river_route_amd/ may import, link or call this file.
 *
 * What it is for: the fp64 oracle and the GPU kernels both round at every statement; this restatement keeps the state,
 * the right-hand side, the interval sums and the mean in long double (64-bit significand: 2^11 times finer), so its
 * output is the yardstick both are measured against, reach by reach (tests/per_reach.py).  Inputs and outputs are
 * double: coefficients, laterals and the initial state are taken as the doubles they are given -- the arbiter judges
 * the routing, not the coefficient formula -- and every output is rounded to double once, on the way out.
 *
 * Each routing form returns, next to the clamped interval means (`discharge`), the UNCLAMPED means (`raw`): a reach's
 * own scale is max_t |raw|, which is not zero where a negative mean was clamped away.  The final state comes back in
 * the state arrays, rounded once.
 *
 * Parity status: PINNED to rr_oracle.c (tests/test_per_reach.py: within 1e-13 per reach at the reach's own scale on
 * the golden cases and on every forcing regime of the per-reach tests), which is itself pinned to the reference.
 */
#include <float.h>
#include <stdint.h>
#include <stdlib.h>

_Static_assert(LDBL_MANT_DIG >= 64, "the arbiter needs a long double wider than double (x87 extended or better): "
                                    "on this platform it would only repeat the fp64 oracle");

#define ORC_OK 0
#define ORC_E_ALLOC -1

typedef long double ld;

/* substep_scatter_solve of rr_oracle.c: rhs += c2 * (A q_src) by CSC scatter, then forward substitution in column order */
static void substep_scatter_solve_ld(int64_t n, const int32_t *indptr, const int32_t *indices,
                                     const double *lhs_off, const double *c2,
                                     const ld *q_src, ld *q_dst, ld *rhs)
{
    for (int64_t col = 0; col < n; ++col) {
        const ld qv = q_src[col];
        for (int32_t j = indptr[col]; j < indptr[col + 1]; ++j) {
            const int32_t row = indices[j];
            rhs[row] += (ld)c2[row] * qv;
        }
    }
    for (int64_t col = 0; col < n; ++col) {
        q_dst[col] = rhs[col];
        for (int32_t j = indptr[col]; j < indptr[col + 1]; ++j)
            rhs[indices[j]] -= (ld)lhs_off[j] * q_dst[col];
    }
}

static void put_means(int64_t n, const ld *isum, ld inv, double *row, double *raw_row)
{
    for (int64_t i = 0; i < n; ++i) {
        const ld v = isum[i] * inv;
        raw_row[i] = (double)v;
        row[i] = v > 0.0L ? (double)v : 0.0;
    }
}

/* orc_muskingum_route in long double; raw is (num_output_steps, n) like discharge */
int orcl_muskingum_route(int64_t n, const int32_t *indptr, const int32_t *indices,
                         const double *lhs_off, const double *c2, const double *c3,
                         double *q_t, double *discharge, double *raw,
                         int64_t num_output_steps, int64_t num_routing_per_output)
{
    const size_t m = (size_t)(n ? n : 1);
    ld *buf = (ld *)malloc(sizeof(ld) * 3 * m);
    if (!buf) return ORC_E_ALLOC;
    ld *rhs = buf, *isum = buf + m, *q = buf + 2 * m;
    for (int64_t i = 0; i < n; ++i) q[i] = q_t[i];
    const ld inv = 1.0L / (ld)num_routing_per_output;
    for (int64_t o = 0; o < num_output_steps; ++o) {
        for (int64_t i = 0; i < n; ++i) isum[i] = 0.0L;
        for (int64_t s = 0; s < num_routing_per_output; ++s) {
            for (int64_t i = 0; i < n; ++i) rhs[i] = (ld)c3[i] * q[i];
            substep_scatter_solve_ld(n, indptr, indices, lhs_off, c2, q, q, rhs);
            for (int64_t i = 0; i < n; ++i) isum[i] += q[i];
        }
        put_means(n, isum, inv, discharge + o * n, raw + o * n);
    }
    for (int64_t i = 0; i < n; ++i) q_t[i] = (double)q[i];
    free(buf);
    return ORC_OK;
}

/* orc_rapid_route in long double */
int orcl_rapid_route(int64_t n, const int32_t *indptr, const int32_t *indices,
                     const double *lhs_off, const double *c2, const double *c3,
                     const double *c4_dt, double *q_t, const double *qlateral,
                     double *discharge, double *raw, int64_t num_runoff_steps, int64_t num_substeps)
{
    const size_t m = (size_t)(n ? n : 1);
    ld *buf = (ld *)malloc(sizeof(ld) * 3 * m);
    if (!buf) return ORC_E_ALLOC;
    ld *rhs = buf, *isum = buf + m, *q = buf + 2 * m;
    for (int64_t i = 0; i < n; ++i) q[i] = q_t[i];
    const ld inv = 1.0L / (ld)num_substeps;
    for (int64_t t = 0; t < num_runoff_steps; ++t) {
        const double *ql = qlateral + t * n;
        for (int64_t i = 0; i < n; ++i) isum[i] = 0.0L;
        for (int64_t s = 0; s < num_substeps; ++s) {
            for (int64_t i = 0; i < n; ++i) rhs[i] = (ld)c3[i] * q[i] + (ld)c4_dt[i] * (ld)ql[i];
            substep_scatter_solve_ld(n, indptr, indices, lhs_off, c2, q, q, rhs);
            for (int64_t i = 0; i < n; ++i) isum[i] += q[i];
        }
        put_means(n, isum, inv, discharge + t * n, raw + t * n);
    }
    for (int64_t i = 0; i < n; ++i) q_t[i] = (double)q[i];
    free(buf);
    return ORC_OK;
}

/* csc_spmv of rr_oracle.c */
static void csc_spmv_ld(int64_t nrows, int64_t ncols, const int32_t *indptr, const int32_t *indices,
                        const double *data, const ld *x, ld *y)
{
    for (int64_t i = 0; i < nrows; ++i) y[i] = 0.0L;
    for (int64_t col = 0; col < ncols; ++col) {
        const ld v = x[col];
        for (int32_t j = indptr[col]; j < indptr[col + 1]; ++j)
            y[indices[j]] += (ld)data[j] * v;
    }
}

/* orc_unit_route in long double.  Headwater columns of discharge and raw are the lateral rows as they are (doubles). */
int orcl_unit_route(int64_t n_inner, int64_t n_hw, int64_t n_total,
                    const int32_t *lhs_indptr, const int32_t *lhs_indices, const double *lhs_off,
                    const int32_t *a_in_indptr, const int32_t *a_in_indices, const double *a_in_data,
                    const int32_t *a_hw_indptr, const int32_t *a_hw_indices, const double *a_hw_data,
                    const double *c1_in, const double *c2_in, const double *c3_in,
                    const int64_t *hw_idx, const int64_t *inner_idx,
                    double *q_ch, double *q_full,
                    const double *convolved, double *discharge, double *raw,
                    int64_t num_runoff_steps, int64_t num_substeps)
{
    const size_t ni = (size_t)(n_inner ? n_inner : 1), nh = (size_t)(n_hw ? n_hw : 1);
    ld *buf = (ld *)malloc(sizeof(ld) * (8 * ni + nh));
    if (!buf) return ORC_E_ALLOC;
    ld *rhs = buf, *isum = buf + ni, *ql_in = buf + 2 * ni, *a_in_res = buf + 3 * ni,
       *a_hw_res = buf + 4 * ni, *c1_a_ql = buf + 5 * ni, *qc = buf + 6 * ni, *qf = buf + 7 * ni, *ql_hw = buf + 8 * ni;
    for (int64_t i = 0; i < n_inner; ++i) { qc[i] = q_ch[i]; qf[i] = q_full[i]; }
    const ld inv = 1.0L / (ld)num_substeps;
    for (int64_t t = 0; t < num_runoff_steps; ++t) {
        const double *lat = convolved + t * n_total;
        double *row = discharge + t * n_total, *raw_row = raw + t * n_total;
        for (int64_t i = 0; i < n_hw; ++i) ql_hw[i] = lat[hw_idx[i]];
        for (int64_t i = 0; i < n_inner; ++i) ql_in[i] = lat[inner_idx[i]];
        for (int64_t i = 0; i < n_hw; ++i) raw_row[hw_idx[i]] = row[hw_idx[i]] = lat[hw_idx[i]];      /* no clamp, no mean */
        csc_spmv_ld(n_inner, n_inner, a_in_indptr, a_in_indices, a_in_data, ql_in, a_in_res);
        csc_spmv_ld(n_inner, n_hw, a_hw_indptr, a_hw_indices, a_hw_data, ql_hw, a_hw_res);
        for (int64_t i = 0; i < n_inner; ++i) c1_a_ql[i] = (ld)c1_in[i] * (a_in_res[i] + a_hw_res[i]);
        for (int64_t i = 0; i < n_inner; ++i) isum[i] = 0.0L;
        for (int64_t s = 0; s < num_substeps; ++s) {
            for (int64_t i = 0; i < n_inner; ++i)
                rhs[i] = c1_a_ql[i] + (ld)c2_in[i] * a_hw_res[i] + (ld)c3_in[i] * qc[i];
            substep_scatter_solve_ld(n_inner, lhs_indptr, lhs_indices, lhs_off, c2_in, qf, qc, rhs);
            for (int64_t i = 0; i < n_inner; ++i) {
                qf[i] = qc[i] + ql_in[i];
                isum[i] += qf[i];
            }
        }
        for (int64_t i = 0; i < n_inner; ++i) {
            const ld v = isum[i] * inv;
            raw_row[inner_idx[i]] = (double)v;
            row[inner_idx[i]] = v > 0.0L ? (double)v : 0.0;
        }
    }
    for (int64_t i = 0; i < n_inner; ++i) { q_ch[i] = (double)qc[i]; q_full[i] = (double)qf[i]; }
    free(buf);
    return ORC_OK;
}

/* orc_uh_convolve in long double: the buffer of T + n_ks - 1 rows is long double, the carried state goes in and comes out
 * as double (rounded once).  There is no clamp: the rows are their own unclamped form. */
int orcl_uh_convolve(int64_t T, int64_t n_ks, int64_t n, const double *kernel, double *state,
                     const double *lateral, double *out)
{
    const int64_t M = T + n_ks - 1;
    const size_t cells = (size_t)(M > 0 ? M : 1) * (size_t)(n ? n : 1);
    ld *buf = (ld *)malloc(sizeof(ld) * cells);
    if (!buf) return ORC_E_ALLOC;
    for (size_t c = 0; c < cells; ++c) buf[c] = 0.0L;
    for (int64_t m = 0; m < M; ++m) {
        const int64_t s_lo = m - (T - 1) > 0 ? m - (T - 1) : 0;
        const int64_t s_hi = m < n_ks - 1 ? m : n_ks - 1;
        ld *b = buf + m * n;
        for (int64_t s = s_lo; s <= s_hi; ++s) {
            const double *kr = kernel + s * n, *lr = lateral + (m - s) * n;
            for (int64_t i = 0; i < n; ++i) b[i] += (ld)kr[i] * (ld)lr[i];
        }
    }
    for (int64_t s = 0; s < n_ks && s < M; ++s)
        for (int64_t i = 0; i < n; ++i) buf[s * n + i] += (ld)state[s * n + i];
    for (int64_t c = 0; c < n_ks * n; ++c) state[c] = 0.0;
    for (int64_t s = 0; s + 1 < n_ks; ++s)
        for (int64_t i = 0; i < n; ++i) state[s * n + i] = (double)buf[(T + s) * n + i];
    for (int64_t c = 0; c < T * n; ++c) out[c] = (double)buf[c];
    free(buf);
    return ORC_OK;
}
