// rr_kernels_adjoint.hpp -- the adjoint of RapidMuskingum routing (rr_rapid_adjoint_dev): the reverse routing
// tick, the per-column reduction of the coefficient gradients and the row pass of the lateral-inflow gradient.  The host side that
// launches them is rapid_adjoint in rr_adjoint.hpp.
// Part of the one translation unit rr_engine.hip builds (included from there, in order; not a stand-alone header).
//
// Forward, equation s = 1..S of reach i (S = T * nsub, sub-step s - 1 of row t = (s - 1) / nsub):
//   q[s,i] = c1[i] sum_u q[s,u] + c2[i] sum_u q[s-1,u] + c3[i] q[s-1,i] + c4dt[i] ql[t,i]
// Adjoint, backward from s = S, with d = down(i) and mu[S+1] = 0:
//   mu[s,i] = g[s,i] + c1[d] mu[s,d] + c2[d] mu[s+1,d] + c3[i] mu[s+1,i]
// A reach reads only its one downstream reach, at this step and the next: with D(i) = Dmax - lag(i) (levels to the outlet),
// reverse tick tau handles reach i at reverse step r = tau - D(i), s = S - r, and every tick is free of dependencies -- the
// forward's lag trick with the edges turned round.  Tapes are tick-indexed: row tau holds what every position wrote at tick tau.
#pragma once

namespace {

struct AdjTickArgs {
    const int32_t *lag;        // [n] engine order (no boundary flags: the adjoint refuses partitioned plans)
    const int32_t *down;       // [n] downstream position, -1 at outlets
    const double *w;           // [n] c1 of the downstream reach, stored at the upstream position (TickArgs::w)
    const double *c2, *c3;     // [n] engine order
    const double *g;           // [T, n] dL/d(discharge) in engine order, clamp mask and 1/nsub applied (NULL: none)
    const double *gf;          // [n] dL/d(q_final) in PARAMS order (NULL: none), read at r == 0 through perm
    const int32_t *perm;       // [n] params index of engine position p
    const double *ma;          // mu written one tick ago
    const double *mb;          // mu written two ticks ago
    double *mc;                // this tick's mu
    int64_t n;
    int32_t p_lo, p_hi;        // active engine positions
    int32_t dmax;
    int64_t tau;               // reverse tick
    int64_t total_substeps;    // S
    Div32 nsub;
};

// One reverse tick: mu of every active position.  One reach per lane over lag-ordered positions, like k_tick; the downstream
// reads hit a handful of cache lines per wave (the downstream reaches of consecutive positions are consecutive positions).
template <bool SINGLE_SUBSTEP>
__global__ __launch_bounds__(kBlock) void k_adj_tick(const AdjTickArgs a)
{
    const int32_t p = a.p_lo + (int32_t)(blockIdx.x * kBlock + threadIdx.x);
    if (p >= a.p_hi) return;
    const int32_t lag = a.lag[p] & kLagMask;
    const int64_t r = a.tau - (int64_t)(a.dmax - lag);
    if (r < 0 || r >= a.total_substeps) return;
    const uint32_t ts = (uint32_t)(a.total_substeps - 1 - r);     // forward sub-step of equation s = ts + 1
    uint32_t t;
    if (SINGLE_SUBSTEP) t = ts;
    else { uint32_t rem; t = a.nsub.div(ts, rem); }

    double m = a.g ? a.g[(int64_t)t * a.n + p] : 0.0;
    if (r == 0 && a.gf) m += a.gf[a.perm[p]];
    if (r > 0) m = __builtin_fma(a.c3[p], a.ma[p], m);
    const int32_t d = a.down[p];
    if (d >= 0) {
        m = __builtin_fma(a.w[p], a.ma[d], m);                   // c1[d] mu[s, d]: d ran reverse step r one tick ago
        if (r > 0) m = __builtin_fma(a.c2[d], a.mb[d], m);       // c2[d] mu[s+1, d]: two ticks ago
    }
    a.mc[p] = m;
}

// q tape row tau - 1 at every position's first forward tick holds q0: what k_tick reads as "its own last value" and, two ticks
// later, as "the old upstream value" of the reach below.  Storage row = tick + 2 (ticks -2 and -1 come first).
__global__ __launch_bounds__(kBlock) void k_adj_tape_init(double *qtape, const double *q0, const int32_t *perm, const int32_t *lag,
                                                          int64_t n)
{
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= n) return;
    qtape[(int64_t)((lag[p] & kLagMask) + 1) * n + p] = q0[perm[p]];
}

// dL/d(discharge) in params order with the forward's clamp and mean applied: the discharge row is max(mean, 0), so a value
// that came out <= 0 passes no gradient.
__global__ __launch_bounds__(kBlock) void k_adj_mask(double *dst, const double *grad_out, const double *discharge, int64_t count,
                                                     double inv_nsub)
{
    for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k < count; k += (int64_t)gridDim.x * kBlock)
        dst[k] = discharge[k] > 0.0 ? grad_out[k] * inv_nsub : 0.0;
}

struct AdjReduceArgs {
    const int32_t *lag, *child_ptr;
    const double *qtape;       // storage row tau + 2 = q written at forward tick tau
    const double *mtape;       // row tau = mu written at reverse tick tau
    const double *lat;         // [T, n] lateral rows in engine order (NULL: channel-only)
    double *slab;              // [splits][4][n] partial sums
    int64_t n;
    int64_t total_substeps, steps_per_split;
    int32_t dmax;
    Div32 nsub;
};

// Partial sums over one range of sub-steps per column (blockIdx.y = range): the four coefficient gradients
//   sum_s mu[s,i] * {sum_u q[s,u], sum_u q[s-1,u], q[s-1,i], ql[t(s-1),i]}.
// The ranges are merged in a fixed order by k_adj_merge: no atomics, repeated calls give the same bits.
template <bool SINGLE_SUBSTEP>
__global__ __launch_bounds__(kBlock) void k_adj_reduce(const AdjReduceArgs a)
{
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= a.n) return;
    const int64_t n = a.n;
    const int32_t lag = a.lag[p] & kLagMask;
    const int32_t u0 = a.child_ptr[p], u1 = a.child_ptr[p + 1];
    const int64_t s0 = (int64_t)blockIdx.y * a.steps_per_split, s1 = min(a.total_substeps, s0 + a.steps_per_split);
    double g1 = 0.0, g2 = 0.0, g3 = 0.0, g4 = 0.0;
    for (int64_t ts = s0; ts < s1; ++ts) {
        // forward tick of this sub-step: ts + lag; its inputs were written one (new upstream, own old) and two (old upstream) ticks before
        const double *q1 = a.qtape + (ts + lag + 1) * n, *q2 = q1 - n;
        const double mu = a.mtape[(a.total_substeps - 1 - ts + a.dmax - lag) * n + p];
        double s_new = 0.0, s_old = 0.0;
        for (int32_t u = u0; u < u1; ++u) { s_new += q1[u]; s_old += q2[u]; }
        g1 = __builtin_fma(mu, s_new, g1);
        g2 = __builtin_fma(mu, s_old, g2);
        g3 = __builtin_fma(mu, q1[p], g3);
        if (a.lat) {
            uint32_t t;
            if (SINGLE_SUBSTEP) t = (uint32_t)ts;
            else { uint32_t rem; t = a.nsub.div((uint32_t)ts, rem); }
            g4 = __builtin_fma(mu, a.lat[(int64_t)t * n + p], g4);
        }
    }
    double *out = a.slab + (int64_t)blockIdx.y * 4 * n + p;
    out[0] = g1; out[n] = g2; out[2 * n] = g3; out[3 * n] = g4;
}

// Merge of the ranges in order, scattered to params order; dL/dq0[i] = c3[i] mu[1,i] + c2[d] mu[1,d].
__global__ __launch_bounds__(kBlock) void k_adj_merge(const double *slab, int64_t splits, const double *mtape, const int32_t *lag,
                                                      const int32_t *down, const int32_t *perm, const double *c2, const double *c3,
                                                      int64_t n, int64_t total_substeps, int32_t dmax, int has_lateral,
                                                      double *grad_coef, double *grad_q0)
{
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= n) return;
    const int32_t i = perm[p];
    if (grad_coef) {
        double g[4] = {0.0, 0.0, 0.0, 0.0};
        for (int64_t k = 0; k < splits; ++k)
#pragma unroll
            for (int c = 0; c < 4; ++c) g[c] += slab[(k * 4 + c) * n + p];
        grad_coef[i] = g[0]; grad_coef[n + i] = g[1]; grad_coef[2 * n + i] = g[2]; grad_coef[3 * n + i] = has_lateral ? g[3] : 0.0;
    }
    if (grad_q0) {
        const int64_t tau = total_substeps - 1 + dmax - (lag[p] & kLagMask);      // reverse tick of s = 1
        double v = c3[p] * mtape[tau * n + p];
        const int32_t d = down[p];
        if (d >= 0) v = __builtin_fma(c2[d], mtape[(tau - 1) * n + d], v);
        grad_q0[i] = v;
    }
}

// dL/dql[t, p] = c4dt[p] * sum of mu over the sub-steps of row t, engine order (the rows then go to params order through the
// tiled permutation).  Row t's sub-steps ran at consecutive reverse ticks, latest first.
__global__ __launch_bounds__(kBlock) void k_adj_rows(double *dst, const double *mtape, const int32_t *lag, const double *c4, int64_t n,
                                                     int64_t T, int64_t nsub, int64_t total_substeps, int32_t dmax)
{
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= n) return;
    const int64_t base = total_substeps - 1 + dmax - (lag[p] & kLagMask);      // reverse tick of forward sub-step 0
    const double c = c4[p];
    for (int64_t t = blockIdx.y; t < T; t += gridDim.y) {
        double m = 0.0;
        for (int64_t k = 0; k < nsub; ++k) m += mtape[(base - (t * nsub + k)) * n + p];
        dst[t * n + p] = c * m;
    }
}

}  // namespace
