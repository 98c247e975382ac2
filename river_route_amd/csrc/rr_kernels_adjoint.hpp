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
//
// Member-batched forms (rr_rapid_adjoint_batch_dev): several forcing series on one plan and one coefficient
// set.  The members share every read-only plan array; member m owns a q tape, a mu tape, engine-order lateral and gradient rows,
// slab and scratch rows at member pitches (64-bit element counts).  The templated kernels take a trailing ENS flag and an args
// struct with the pitches appended, and form every index as (ENS ? index + offset : index), so their single-member instantiations
// are the code they were (rr_kernels_tick.hpp: TickEnsArgs); the member is blockIdx.y, in the reduction, whose y is the sub-step
// range, blockIdx.z.  The plain one-pass kernels take a leading ENS flag, scalar parameters and, last, what the member form adds
// (ArgsIf below); their body is a __forceinline__ function that the member form runs on the member's pointers.
//
// Gauge form (rr_rapid_adjoint_gauges_dev): dL/d(discharge) is given at G gauged reaches only.  The reverse
// tick takes a trailing GAUGES flag and an args struct with the slot map appended: a position reads slot[p] and, where that is >= 0,
// the masked (T, G) block; every other position starts from 0.0, which is what the dense form reads there.  k_adj_gauge_fill,
// k_adj_gauge_scatter and k_adj_gauge_slots build the map; the mask over the block is k_adj_mask itself on T * G elements.
#pragma once

namespace {

// The last parameter of a one-pass kernel: the pitches its member form takes besides the plain form's arguments, and nothing in the
// plain form.  The plain parameters stay scalars in one order for all forms and the empty struct comes last, where it moves no
// argument: anywhere else it takes eight bytes and moves every later offset, and one args struct in place of the scalars changes the
// kernarg loads of every form.  What a form adds in the middle of the list rides in a small struct with its neighbour instead
// (AdjMergeRanges, UnitMaskColumns, UnitRowsCotangent), which lays the arguments out as scalars would
// (profiles/adjoint_kernels_refactor_ab.md).
struct NoArgs {};
template <bool ON, class A> using ArgsIf = typename std::conditional<ON, A, NoArgs>::type;
template <bool ON, class A> ArgsIf<ON, A> args_if(const A &a)
{
    if constexpr (ON) return a;
    else return {};
}

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

// Member blockIdx.y: its mu tape rows (ma, mb, mc) at tape_pitch, its dL/d(discharge) rows at g_pitch and its dL/d(q_final) at gf_pitch.
struct AdjTickEnsArgs : AdjTickArgs {
    int64_t tape_pitch, g_pitch, gf_pitch;
};
// The gauge form of either: g is the masked (T, n_gauges) block (member blockIdx.y's at g_pitch), read where slot[p] >= 0.
struct AdjTickGaugeArgs : AdjTickArgs {
    const int32_t *slot;       // [n] engine order: the gauge column of position p, -1 where the reach has no gauge
    int64_t n_gauges;
};
struct AdjTickGaugeEnsArgs : AdjTickEnsArgs {
    const int32_t *slot;
    int64_t n_gauges;
};
template <bool ENS, bool GAUGES = false> using AdjTickArgsOf =
    typename std::conditional<GAUGES, typename std::conditional<ENS, AdjTickGaugeEnsArgs, AdjTickGaugeArgs>::type,
                              typename std::conditional<ENS, AdjTickEnsArgs, AdjTickArgs>::type>::type;
__device__ __forceinline__ int64_t member_tape0(const AdjTickArgs &) { return 0; }
__device__ __forceinline__ int64_t member_tape0(const AdjTickEnsArgs &e) { return (int64_t)blockIdx.y * e.tape_pitch; }
__device__ __forceinline__ int64_t member_g0(const AdjTickArgs &) { return 0; }
__device__ __forceinline__ int64_t member_g0(const AdjTickEnsArgs &e) { return (int64_t)blockIdx.y * e.g_pitch; }
__device__ __forceinline__ int64_t member_gf0(const AdjTickArgs &) { return 0; }
__device__ __forceinline__ int64_t member_gf0(const AdjTickEnsArgs &e) { return (int64_t)blockIdx.y * e.gf_pitch; }

// One reverse tick: mu of every active position.  One reach per lane over lag-ordered positions, like k_tick; the downstream
// reads hit a handful of cache lines per wave (the downstream reaches of consecutive positions are consecutive positions).
// ENS: the member-batched form; the fma sequence of a member is the single call's.  GAUGES: dL/d(discharge) comes from the gauge
// block through the slot map (one dependent load per position); the fma sequence is the dense form's on the same values.
template <bool SINGLE_SUBSTEP, bool ENS = false, bool GAUGES = false>
__global__ __launch_bounds__(kBlock) void k_adj_tick(const AdjTickArgsOf<ENS, GAUGES> a)
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

    const int64_t mt = member_tape0(a), mg = member_g0(a), mf = member_gf0(a);
    double m;
    if constexpr (GAUGES) {
        m = 0.0;
        if (a.g) {
            const int32_t j = a.slot[p];
            if (j >= 0) m = a.g[ENS ? (int64_t)t * a.n_gauges + j + mg : (int64_t)t * a.n_gauges + j];
        }
    } else
        m = a.g ? a.g[ENS ? (int64_t)t * a.n + p + mg : (int64_t)t * a.n + p] : 0.0;
    if (r == 0 && a.gf) m += a.gf[ENS ? a.perm[p] + mf : a.perm[p]];
    if (r > 0) m = __builtin_fma(a.c3[p], a.ma[ENS ? p + mt : p], m);
    const int32_t d = a.down[p];
    if (d >= 0) {
        m = __builtin_fma(a.w[p], a.ma[ENS ? d + mt : d], m);                   // c1[d] mu[s, d]: d ran reverse step r one tick ago
        if (r > 0) m = __builtin_fma(a.c2[d], a.mb[ENS ? d + mt : d], m);       // c2[d] mu[s+1, d]: two ticks ago
    }
    a.mc[ENS ? p + mt : p] = m;
}

// q tape row tau - 1 at every position's first forward tick holds q0: what k_tick reads as "its own last value" and, two ticks
// later, as "the old upstream value" of the reach below.  Storage row = tick + 2 (ticks -2 and -1 come first).
__device__ __forceinline__ void adj_tape_init(double *qtape, const double *q0, const int32_t *perm, const int32_t *lag, int64_t n)
{
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= n) return;
    qtape[(int64_t)((lag[p] & kLagMask) + 1) * n + p] = q0[perm[p]];
}
// ENS: member blockIdx.y, its tape at tape_pitch, its q0 at q0_pitch (0: one q0 for every member)
struct AdjTapeInitMember { int64_t tape_pitch, q0_pitch; };
template <bool ENS>
__global__ __launch_bounds__(kBlock) void k_adj_tape_init(double *qtape, const double *q0, const int32_t *perm, const int32_t *lag,
                                                          int64_t n, const ArgsIf<ENS, AdjTapeInitMember> mp)
{
    if constexpr (ENS) { qtape += (int64_t)blockIdx.y * mp.tape_pitch; q0 += (int64_t)blockIdx.y * mp.q0_pitch; }
    adj_tape_init(qtape, q0, perm, lag, n);
}

// dL/d(discharge) in params order with the forward's clamp and mean applied: the discharge row is max(mean, 0), so a value
// that came out <= 0 passes no gradient.
__device__ __forceinline__ void adj_mask(double *dst, const double *grad_out, const double *discharge, int64_t count, double inv_nsub)
{
    for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k < count; k += (int64_t)gridDim.x * kBlock)
        dst[k] = discharge[k] > 0.0 ? grad_out[k] * inv_nsub : 0.0;
}
// ENS: member blockIdx.y, its destination rows at dst_pitch, its discharge and dL/d(discharge) rows at row_pitch
struct AdjMaskMember { int64_t dst_pitch, row_pitch; };
template <bool ENS>
__global__ __launch_bounds__(kBlock) void k_adj_mask(double *dst, const double *grad_out, const double *discharge, int64_t count,
                                                     double inv_nsub, const ArgsIf<ENS, AdjMaskMember> mp)
{
    if constexpr (ENS) {
        const int64_t m = blockIdx.y;
        dst += m * mp.dst_pitch; grad_out += m * mp.row_pitch; discharge += m * mp.row_pitch;
    }
    adj_mask(dst, grad_out, discharge, count, inv_nsub);
}

// The slot map of a gauge call, three launches in stream order: pslot[n] (params order) filled with -1, pslot[gauges[j]] = j, then
// slot[p] = pslot[perm[p]] in engine order.  gauges[] is not range-checked here: the caller vouches for distinct indices in [0, n).
__global__ __launch_bounds__(kBlock) void k_adj_gauge_fill(int32_t *pslot, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) pslot[i] = -1;
}
__global__ __launch_bounds__(kBlock) void k_adj_gauge_scatter(int32_t *pslot, const int32_t *gauges, int64_t n_gauges)
{
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j < n_gauges) pslot[gauges[j]] = (int32_t)j;
}
__global__ __launch_bounds__(kBlock) void k_adj_gauge_slots(int32_t *slot, const int32_t *pslot, const int32_t *perm, int64_t n)
{
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p < n) slot[p] = pslot[perm[p]];
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

// Member blockIdx.z: its tapes at qtape_pitch / mtape_pitch, its lateral rows at lat_pitch, its [splits][4][n] of the slab at slab_pitch.
struct AdjReduceEnsArgs : AdjReduceArgs {
    int64_t qtape_pitch, mtape_pitch, lat_pitch, slab_pitch;
};
template <bool ENS> using AdjReduceArgsOf = typename std::conditional<ENS, AdjReduceEnsArgs, AdjReduceArgs>::type;
struct AdjReduceMember { int64_t q, m, lat, slab; };
__device__ __forceinline__ AdjReduceMember member_offsets(const AdjReduceArgs &) { return {0, 0, 0, 0}; }
__device__ __forceinline__ AdjReduceMember member_offsets(const AdjReduceEnsArgs &e)
{
    const int64_t m = blockIdx.z;
    return {m * e.qtape_pitch, m * e.mtape_pitch, m * e.lat_pitch, m * e.slab_pitch};
}

// Partial sums over one range of sub-steps per column (blockIdx.y = range): the four coefficient gradients
//   sum_s mu[s,i] * {sum_u q[s,u], sum_u q[s-1,u], q[s-1,i], ql[t(s-1),i]}.
// The ranges are merged in a fixed order by k_adj_merge: no atomics, repeated calls give the same bits.
// ENS: the member-batched form, member m's sums in slab [m][range][4][n].
template <bool SINGLE_SUBSTEP, bool ENS = false>
__global__ __launch_bounds__(kBlock) void k_adj_reduce(const AdjReduceArgsOf<ENS> a)
{
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= a.n) return;
    const int64_t n = a.n;
    const int32_t lag = a.lag[p] & kLagMask;
    const int32_t u0 = a.child_ptr[p], u1 = a.child_ptr[p + 1];
    const int64_t s0 = (int64_t)blockIdx.y * a.steps_per_split, s1 = min(a.total_substeps, s0 + a.steps_per_split);
    const AdjReduceMember mo = member_offsets(a);
    double g1 = 0.0, g2 = 0.0, g3 = 0.0, g4 = 0.0;
    for (int64_t ts = s0; ts < s1; ++ts) {
        // forward tick of this sub-step: ts + lag; its inputs were written one (new upstream, own old) and two (old upstream) ticks before
        const double *q1 = a.qtape + (ENS ? (ts + lag + 1) * n + mo.q : (ts + lag + 1) * n), *q2 = q1 - n;
        const double mu = a.mtape[ENS ? (a.total_substeps - 1 - ts + a.dmax - lag) * n + p + mo.m : (a.total_substeps - 1 - ts + a.dmax - lag) * n + p];
        double s_new = 0.0, s_old = 0.0;
        for (int32_t u = u0; u < u1; ++u) { s_new += q1[u]; s_old += q2[u]; }
        g1 = __builtin_fma(mu, s_new, g1);
        g2 = __builtin_fma(mu, s_old, g2);
        g3 = __builtin_fma(mu, q1[p], g3);
        if (a.lat) {
            uint32_t t;
            if (SINGLE_SUBSTEP) t = (uint32_t)ts;
            else { uint32_t rem; t = a.nsub.div((uint32_t)ts, rem); }
            g4 = __builtin_fma(mu, a.lat[ENS ? (int64_t)t * n + p + mo.lat : (int64_t)t * n + p], g4);
        }
    }
    double *out = a.slab + (ENS ? (int64_t)blockIdx.y * 4 * n + p + mo.slab : (int64_t)blockIdx.y * 4 * n + p);
    out[0] = g1; out[n] = g2; out[2 * n] = g3; out[3 * n] = g4;
}

// Merge of the ranges in order, scattered to params order; dL/dq0[i] = c3[i] mu[1,i] + c2[d] mu[1,d].
__device__ __forceinline__ void adj_merge(const double *slab, int64_t splits, const double *mtape, const int32_t *lag,
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
// ENS: member blockIdx.y writes its own dL/dq0 row (grad_q0[members][n]) from its mu tape at tape_pitch.  The coefficient gradients
// are one sum over the members: the slab [members][splits][4][n] is contiguous (adjoint_layout), so the blocks of member 0 fold all
// members x splits ranges in storage order -- members ascending, within a member the ranges in order -- and the others leave
// grad_coef alone.
template <bool ENS> struct AdjMergeRanges { int64_t splits; };      // the ranges a merge folds: splits, or splits x members
template <> struct AdjMergeRanges<true> { int64_t splits, members; };
struct AdjMergeMember { int64_t tape_pitch; };
template <bool ENS>
__global__ __launch_bounds__(kBlock) void k_adj_merge(const double *slab, const AdjMergeRanges<ENS> r, const double *mtape, const int32_t *lag,
                                                      const int32_t *down, const int32_t *perm, const double *c2, const double *c3,
                                                      int64_t n, int64_t total_substeps, int32_t dmax, int has_lateral,
                                                      double *grad_coef, double *grad_q0, const ArgsIf<ENS, AdjMergeMember> mp)
{
    int64_t ranges = r.splits;
    if constexpr (ENS) {
        const int64_t m = blockIdx.y;
        ranges *= r.members; mtape += m * mp.tape_pitch;
        if (m != 0) grad_coef = nullptr;
        if (grad_q0) grad_q0 += m * n;
    }
    adj_merge(slab, ranges, mtape, lag, down, perm, c2, c3, n, total_substeps, dmax, has_lateral, grad_coef, grad_q0);
}

// dL/dql[t, p] = c4dt[p] * sum of mu over the sub-steps of row t, engine order (the rows then go to params order through the
// tiled permutation).  Row t's sub-steps ran at consecutive reverse ticks, latest first.
__device__ __forceinline__ void adj_rows(double *dst, const double *mtape, const int32_t *lag, const double *c4, int64_t n,
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
// ENS: member blockIdx.z (y walks the rows), its gradient rows at dst_pitch, its mu tape at tape_pitch
struct AdjRowsMember { int64_t dst_pitch, tape_pitch; };
template <bool ENS>
__global__ __launch_bounds__(kBlock) void k_adj_rows(double *dst, const double *mtape, const int32_t *lag, const double *c4, int64_t n,
                                                     int64_t T, int64_t nsub, int64_t total_substeps, int32_t dmax,
                                                     const ArgsIf<ENS, AdjRowsMember> mp)
{
    if constexpr (ENS) { dst += (int64_t)blockIdx.z * mp.dst_pitch; mtape += (int64_t)blockIdx.z * mp.tape_pitch; }
    adj_rows(dst, mtape, lag, c4, n, T, nsub, total_substeps, dmax);
}

}  // namespace
