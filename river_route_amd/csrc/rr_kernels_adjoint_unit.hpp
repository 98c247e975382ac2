// rr_kernels_adjoint_unit.hpp -- the adjoint of UnitMuskingum routing (rr_unit_adjoint_dev) and of the unit-hydrograph convolution
// (rr_uh_adjoint_dev), DESIGN.md section 12.  The host side that launches them: unit_adjoint_enqueue in rr_adjoint.hpp, which shares its
// driver with the Rapid adjoint; rr_uh_adjoint_dev in rr_engine.hip.  Part of the one translation unit rr_engine.hip builds (included
// from there, after rr_kernels_adjoint.hpp; not a stand-alone header).
//
// Forward (river_route/routers/_numba_kernels.py:114-171 with the callers' unit edge weights), inner reach i with headwater
// tributaries H(i) and inner tributaries U(i), equation s = 1..S, row t = (s - 1) / nsub:
//   q_ch[s,i]   = c1[i] (sum_H l[t,h] + sum_U q_full[s,u]) + c2[i] (sum_H l[t,h] + sum_U q_full[s-1,u]) + c3[i] q_ch[s-1,i]
//   q_full[s,i] = q_ch[s,i] + l[t,i]
//   out[t,i]    = max(mean of q_full over the row's sub-steps, 0);      out[t,h] = l[t,h] (no clamp, no mean)
// Adjoint, backward from s = S, d = down(i) (an inner reach), g[s,i] = [out[t,i] > 0] dL/dout[t,i] / nsub, mu[S+1] = 0:
//   phi[s,i] = g[s,i] + [s=S] dL/dq_full_final[i] + c1[d] mu[s,d] + c2[d] mu[s+1,d]            (dL/dq_full[s,i])
//   mu[s,i]  = phi[s,i] + [s=S] dL/dq_ch_final[i] + c3[i] mu[s+1,i]                            (dL/dq_ch[s,i])
// Only mu is taped: phi reads nothing of reach i but g, so the row pass builds it again from the downstream reach's mu (two
// loads) where a phi tape would cost a second S x n array, and mu - c3 mu[s+1] would cancel.  Tick indexing as in
// rr_kernels_adjoint.hpp: reach at lag l runs forward sub-step ts at tick ts + l and reverse step r = S - 1 - ts at reverse tick
// r + Dmax - l; a headwater has the lag its position in the tree gives it and takes no part in the reverse ticks.
//
// Member-batched forms (rr_unit_adjoint_batch_dev), by the convention of rr_kernels_adjoint.hpp: the members
// share every read-only plan array; member m owns a q tape, a mu tape, engine-order lateral and gradient rows, slab and six scratch
// rows at member pitches (64-bit element counts).  The templated kernels take a trailing ENS flag and an args struct with the pitches
// appended and form every index as (ENS ? index + offset : index); the member is blockIdx.y, in the reduction, whose y is the
// sub-step range, blockIdx.z.  The plain one-pass kernels take a leading ENS flag and, last, the member form's pitches (ArgsIf in
// rr_kernels_adjoint.hpp); the member's offsets go onto the pointers first, behind `if constexpr (ENS)`, and the statements that
// follow are written once for both forms.
//
// Gauge form (rr_unit_adjoint_gauges_dev): dL/d(discharge) is given at G gauged reaches only, as masked (T, G)
// blocks, and the slot map of rr_kernels_adjoint.hpp (k_adj_gauge_fill / _scatter / _slots) says which column a position reads.  What
// differs from the Rapid gauge form is the headwater: its cotangent passes into dL/d(lateral) as it is, so the mask needs the
// position of every gauge and the row pass reads the block too, not only the reverse tick: k_adj_mask_unit and k_adj_rows_unit take
// a GAUGES flag after ENS, k_adj_tick_unit a trailing one.  Every other position starts from 0.0, which is what the dense form reads
// there, so the sums are the dense call's on the same values.  What a gauge form reads besides the dense form's arguments stands
// where the separate gauge kernels had it, in a small struct with its neighbour (UnitMaskColumns, UnitRowsCotangent), and the
// statements are the dense form's but for the reads behind `if constexpr (GAUGES)`.
#pragma once

namespace {

struct UnitAdjTickArgs {
    const int32_t *lag, *child_ptr, *down;
    const double *w;           // [n] c1 of the downstream reach, stored at the upstream position
    const double *c2, *c3;     // [n] engine order
    const double *g;           // [T, n] engine order: masked dL/d(discharge) (NULL: none)
    const double *gcf, *gff;   // [n] engine order: dL/d(q_ch final), dL/d(q_full final) at inner positions (NULL: none)
    const double *ma, *mb;     // mu written one / two ticks ago
    double *mc;                // this tick's mu
    int64_t n;
    int32_t p_lo, p_hi, dmax;
    int64_t tau, total_substeps;
    Div32 nsub;
};

// Member blockIdx.y: its mu tape rows (ma, mb, mc) at tape_pitch, its dL/d(discharge) rows at g_pitch and its two final-state
// gradient rows (in its scratch rows) at gf_pitch.
struct UnitAdjTickEnsArgs : UnitAdjTickArgs {
    int64_t tape_pitch, g_pitch, gf_pitch;
};
// The gauge form of either: g is the masked (T, n_gauges) block (member blockIdx.y's at g_pitch), read where slot[p] >= 0.
struct UnitAdjTickGaugeArgs : UnitAdjTickArgs {
    const int32_t *slot;       // [n] engine order: the gauge column of position p, -1 where the reach has no gauge
    int64_t n_gauges;
};
struct UnitAdjTickGaugeEnsArgs : UnitAdjTickEnsArgs {
    const int32_t *slot;
    int64_t n_gauges;
};
template <bool ENS, bool GAUGES = false> using UnitAdjTickArgsOf =
    typename std::conditional<GAUGES, typename std::conditional<ENS, UnitAdjTickGaugeEnsArgs, UnitAdjTickGaugeArgs>::type,
                              typename std::conditional<ENS, UnitAdjTickEnsArgs, UnitAdjTickArgs>::type>::type;
__device__ __forceinline__ int64_t member_tape0(const UnitAdjTickArgs &) { return 0; }
__device__ __forceinline__ int64_t member_tape0(const UnitAdjTickEnsArgs &e) { return (int64_t)blockIdx.y * e.tape_pitch; }
__device__ __forceinline__ int64_t member_g0(const UnitAdjTickArgs &) { return 0; }
__device__ __forceinline__ int64_t member_g0(const UnitAdjTickEnsArgs &e) { return (int64_t)blockIdx.y * e.g_pitch; }
__device__ __forceinline__ int64_t member_gf0(const UnitAdjTickArgs &) { return 0; }
__device__ __forceinline__ int64_t member_gf0(const UnitAdjTickEnsArgs &e) { return (int64_t)blockIdx.y * e.gf_pitch; }

// One reverse tick: mu of every active inner position (k_adj_tick with the two-state recurrence).
// ENS: the member-batched form; the fma sequence of a member is the single call's.  GAUGES: dL/d(discharge) comes from the gauge
// block through the slot map (one dependent load per position); the fma sequence is the dense form's on the same values.
template <bool SINGLE_SUBSTEP, bool ENS = false, bool GAUGES = false>
__global__ __launch_bounds__(kBlock) void k_adj_tick_unit(const UnitAdjTickArgsOf<ENS, GAUGES> a)
{
    const int32_t p = a.p_lo + (int32_t)(blockIdx.x * kBlock + threadIdx.x);
    if (p >= a.p_hi) return;
    if (a.child_ptr[p] == a.child_ptr[p + 1]) return;             // headwater: no state
    const int32_t lag = a.lag[p] & kLagMask;
    const int64_t r = a.tau - (int64_t)(a.dmax - lag);
    if (r < 0 || r >= a.total_substeps) return;
    const uint32_t ts = (uint32_t)(a.total_substeps - 1 - r);
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
    if (r == 0) {
        if (a.gff) m += a.gff[ENS ? p + mf : p];
        if (a.gcf) m += a.gcf[ENS ? p + mf : p];
    }
    const int32_t d = a.down[p];
    if (d >= 0) {
        m = __builtin_fma(a.w[p], a.ma[ENS ? d + mt : d], m);
        if (r > 0) m = __builtin_fma(a.c2[d], a.mb[ENS ? d + mt : d], m);
    }
    if (r > 0) m = __builtin_fma(a.c3[p], a.ma[ENS ? p + mt : p], m);
    a.mc[ENS ? p + mt : p] = m;
}

// dL/d(discharge) in params order with the forward's output rule applied: an inner reach's row is max(mean, 0), a headwater's is
// its lateral inflow as it is.  One column per lane, rows strided over blockIdx.y.
// GAUGES: grad_out and discharge are (T, n), n the number of gauges, column j being reach gauges[j]; the masked block (dst, dense)
// stays in gauge order.  gauges[] is not range-checked here: the caller vouches for distinct indices in [0, n_reaches).
// ENS: member blockIdx.z, its destination rows at dst_pitch (a gauge call's blocks are adjacent: T * n), its discharge and
// dL/d(discharge) rows at row_pitch.
struct UnitMaskMember { int64_t dst_pitch, row_pitch; };
template <bool GAUGES> struct UnitMaskColumns { const int32_t *inv; };      // the engine position of column i: inv[i], or inv[gauges[i]]
template <> struct UnitMaskColumns<true> { const int32_t *gauges, *inv; };
template <bool ENS, bool GAUGES>
__global__ __launch_bounds__(kBlock) void k_adj_mask_unit(double *dst, const double *grad_out, const double *discharge,
                                                          const UnitMaskColumns<GAUGES> col, const int32_t *child_ptr, int64_t n, int64_t T,
                                                          double inv_nsub, const ArgsIf<ENS, UnitMaskMember> mp)
{
    if constexpr (ENS) {
        const int64_t m = blockIdx.z;
        dst += m * mp.dst_pitch; grad_out += m * mp.row_pitch; discharge += m * mp.row_pitch;
    }
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    int32_t p;
    if constexpr (GAUGES) p = col.inv[col.gauges[i]];
    else p = col.inv[i];
    const bool hw = child_ptr[p] == child_ptr[p + 1];
    for (int64_t t = blockIdx.y; t < T; t += gridDim.y) {
        const int64_t k = t * n + i;
        const double g = grad_out[k];
        dst[k] = hw ? g : (discharge[k] > 0.0 ? g * inv_nsub : 0.0);
    }
}

// Inner-indexed vectors to engine positions: the tape's first rows (q_full0 where the reach below reads its "old" value), the
// q_ch row k_tick_unit updates in place and a copy of q_ch0 that stays (the c3 gradient's first term); the final-state gradients.
__device__ __forceinline__ void adj_unit_in(double *qtape, double *qch, double *qch0, const double *q_full0, const double *q_ch0,
                                            double *gcf, double *gff, const double *grad_qch_final, const double *grad_qfull_final,
                                            const int32_t *inner_pos, const int32_t *lag, int64_t n, int32_t n_inner)
{
    const int32_t k = (int32_t)(blockIdx.x * kBlock + threadIdx.x);
    if (k >= n_inner) return;
    const int32_t p = inner_pos[k];
    if (q_full0) {
        qtape[(int64_t)((lag[p] & kLagMask) + 1) * n + p] = q_full0[k];
        const double v = q_ch0[k];
        qch[p] = v; qch0[p] = v;
    }
    if (grad_qch_final) gcf[p] = grad_qch_final[k];
    if (grad_qfull_final) gff[p] = grad_qfull_final[k];
}
// ENS: member blockIdx.y, its tape at tape_pitch, its scratch rows (qch, qch0, gcf, gff) at scratch_pitch, its states at state_pitch
// (0: one pair of states for every member), its final-state gradients [members][n_inner], dense
struct UnitInMember { int64_t tape_pitch, scratch_pitch, state_pitch; };
template <bool ENS>
__global__ __launch_bounds__(kBlock) void k_adj_unit_in(double *qtape, double *qch, double *qch0, const double *q_full0, const double *q_ch0,
                                                        double *gcf, double *gff, const double *grad_qch_final, const double *grad_qfull_final,
                                                        const int32_t *inner_pos, const int32_t *lag, int64_t n, int32_t n_inner,
                                                        const ArgsIf<ENS, UnitInMember> mp)
{
    if constexpr (ENS) {
        const int64_t m = blockIdx.y, ms = m * mp.scratch_pitch;
        qtape += m * mp.tape_pitch; qch += ms; qch0 += ms; gcf += ms; gff += ms;
        if (q_full0) q_full0 += m * mp.state_pitch;
        if (q_ch0) q_ch0 += m * mp.state_pitch;
        if (grad_qch_final) grad_qch_final += m * n_inner;
        if (grad_qfull_final) grad_qfull_final += m * n_inner;
    }
    adj_unit_in(qtape, qch, qch0, q_full0, q_ch0, gcf, gff, grad_qch_final, grad_qfull_final, inner_pos, lag, n, n_inner);
}

struct UnitAdjReduceArgs {
    const int32_t *lag, *child_ptr;
    const uint16_t *hw_children;
    const double *qtape;       // storage row tau + 2 = what every position published at forward tick tau
    const double *mtape;       // row tau = mu written at reverse tick tau
    const double *lat;         // [T, n] lateral rows in engine order
    const double *qch0;        // [n] q_ch0 at inner positions
    double *slab;              // [splits][3][n] partial sums
    int64_t n, total_substeps, steps_per_split;
    int32_t dmax;
    Div32 nsub;
};

// Member blockIdx.z: its tapes at qtape_pitch / mtape_pitch, its lateral rows at lat_pitch, its q_ch0 row (in its scratch rows) at
// qch0_pitch, its [splits][3][n] of the slab at slab_pitch.
struct UnitAdjReduceEnsArgs : UnitAdjReduceArgs {
    int64_t qtape_pitch, mtape_pitch, lat_pitch, qch0_pitch, slab_pitch;
};
template <bool ENS> using UnitAdjReduceArgsOf = typename std::conditional<ENS, UnitAdjReduceEnsArgs, UnitAdjReduceArgs>::type;
struct UnitAdjReduceMember { int64_t q, m, lat, qch0, slab; };
__device__ __forceinline__ UnitAdjReduceMember member_offsets(const UnitAdjReduceArgs &) { return {0, 0, 0, 0, 0}; }
__device__ __forceinline__ UnitAdjReduceMember member_offsets(const UnitAdjReduceEnsArgs &e)
{
    const int64_t m = blockIdx.z;
    return {m * e.qtape_pitch, m * e.mtape_pitch, m * e.lat_pitch, m * e.qch0_pitch, m * e.slab_pitch};
}

// Partial sums over one range of sub-steps per inner reach (blockIdx.y = range):
//   sum_s mu[s,i] * {sum_H l + sum_U q_full[s,u],  sum_H l + sum_U q_full[s-1,u],  q_ch[s-1,i]}
// with q_ch[s-1,i] = q_full[s-1,i] - l[t(s-1),i] from the tape (q_ch0 at s = 1).  Merged in order by k_adj_merge_unit.
// ENS: the member-batched form, member m's sums in slab [m][range][3][n].
template <bool SINGLE_SUBSTEP, bool ENS = false>
__global__ __launch_bounds__(kBlock) void k_adj_reduce_unit(const UnitAdjReduceArgsOf<ENS> a)
{
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= a.n) return;
    const int32_t u0 = a.child_ptr[p], u1 = a.child_ptr[p + 1];
    if (u0 == u1) return;                                         // headwater: k_adj_merge_unit writes its zeros
    const int64_t n = a.n;
    const int32_t lag = a.lag[p] & kLagMask;
    const int32_t uh = u0 + (int32_t)a.hw_children[p];
    const int64_t s0 = (int64_t)blockIdx.y * a.steps_per_split, s1 = min(a.total_substeps, s0 + a.steps_per_split);
    const UnitAdjReduceMember mo = member_offsets(a);
    double g1 = 0.0, g2 = 0.0, g3 = 0.0;
    for (int64_t ts = s0; ts < s1; ++ts) {
        const double *q1 = a.qtape + (ENS ? (ts + lag + 1) * n + mo.q : (ts + lag + 1) * n), *q2 = q1 - n;
        const double mu = a.mtape[ENS ? (a.total_substeps - 1 - ts + a.dmax - lag) * n + p + mo.m : (a.total_substeps - 1 - ts + a.dmax - lag) * n + p];
        double s_hw = 0.0, s_new = 0.0, s_old = 0.0;
        for (int32_t u = u0; u < uh; ++u) s_hw += q1[u];
        for (int32_t u = uh; u < u1; ++u) { s_new += q1[u]; s_old += q2[u]; }
        double prev;
        if (ts == 0) prev = a.qch0[ENS ? p + mo.qch0 : p];
        else {
            uint32_t t;
            if (SINGLE_SUBSTEP) t = (uint32_t)(ts - 1);
            else { uint32_t rem; t = a.nsub.div((uint32_t)(ts - 1), rem); }
            prev = q1[p] - a.lat[ENS ? (int64_t)t * n + p + mo.lat : (int64_t)t * n + p];
        }
        g1 = __builtin_fma(mu, s_hw + s_new, g1);
        g2 = __builtin_fma(mu, s_hw + s_old, g2);
        g3 = __builtin_fma(mu, prev, g3);
    }
    double *out = a.slab + (ENS ? (int64_t)blockIdx.y * 3 * n + p + mo.slab : (int64_t)blockIdx.y * 3 * n + p);
    out[0] = g1; out[n] = g2; out[2 * n] = g3;
}

// Merge of the ranges in order, scattered to params order; zeros on headwaters (their coefficients are never read).
// ENS: the coefficient gradients are one sum over the members: the slab [members][splits][3][n] is contiguous (adjoint_layout), so one
// member's worth of blocks folds all members x splits ranges in storage order -- members ascending, within a member its ranges in order.
template <bool ENS>
__global__ __launch_bounds__(kBlock) void k_adj_merge_unit(const double *slab, const AdjMergeRanges<ENS> r, const int32_t *child_ptr,
                                                           const int32_t *perm, int64_t n, double *grad_coef)
{
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= n) return;
    const int32_t i = perm[p];
    double g[3] = {0.0, 0.0, 0.0};
    if (child_ptr[p] != child_ptr[p + 1]) {
        int64_t ranges = r.splits;
        if constexpr (ENS) ranges *= r.members;
        for (int64_t k = 0; k < ranges; ++k)
#pragma unroll
            for (int c = 0; c < 3; ++c) g[c] += slab[(k * 3 + c) * n + p];
    }
    grad_coef[i] = g[0]; grad_coef[n + i] = g[1]; grad_coef[2 * n + i] = g[2];
}

// dL/dq_ch0[i] = c3[i] mu[1,i], dL/dq_full0[i] = c2[d] mu[1,d], inner order.
__device__ __forceinline__ void adj_state_unit(double *grad_qch0, double *grad_qfull0, const double *mtape, const int32_t *inner_pos,
                                               const int32_t *lag, const int32_t *down, const double *c2, const double *c3, int64_t n,
                                               int32_t n_inner, int64_t total_substeps, int32_t dmax)
{
    const int32_t k = (int32_t)(blockIdx.x * kBlock + threadIdx.x);
    if (k >= n_inner) return;
    const int32_t p = inner_pos[k];
    const int64_t tau = total_substeps - 1 + dmax - (lag[p] & kLagMask);      // reverse tick of s = 1
    if (grad_qch0) grad_qch0[k] = c3[p] * mtape[tau * n + p];
    if (grad_qfull0) {
        const int32_t d = down[p];
        grad_qfull0[k] = d >= 0 ? c2[d] * mtape[(tau - 1) * n + d] : 0.0;
    }
}
// ENS: member blockIdx.y, its rows of grad_qch0 / grad_qfull0 [members][n_inner] from its mu tape at tape_pitch
struct UnitStateMember { int64_t tape_pitch; };
template <bool ENS>
__global__ __launch_bounds__(kBlock) void k_adj_state_unit(double *grad_qch0, double *grad_qfull0, const double *mtape, const int32_t *inner_pos,
                                                           const int32_t *lag, const int32_t *down, const double *c2, const double *c3, int64_t n,
                                                           int32_t n_inner, int64_t total_substeps, int32_t dmax,
                                                           const ArgsIf<ENS, UnitStateMember> mp)
{
    if constexpr (ENS) {
        const int64_t m = blockIdx.y;
        mtape += m * mp.tape_pitch;
        if (grad_qch0) grad_qch0 += m * n_inner;
        if (grad_qfull0) grad_qfull0 += m * n_inner;
    }
    adj_state_unit(grad_qch0, grad_qfull0, mtape, inner_pos, lag, down, c2, c3, n, n_inner, total_substeps, dmax);
}

// dL/dl[t, p] in engine order (g and dst may be the same rows: a lane reads its own element before it writes it):
//   inner      sum over the row's sub-steps of phi[s,p] = g[t,p] + [s=S] gff[p] + c1[d] mu[s,d] + c2[d] mu[s+1,d]
//   headwater  dL/dout[t,p] + (c1[d] + c2[d]) * sum over the row's sub-steps of mu[s,d]
// The downstream reach ran sub-step ts one reverse tick before this position's slot for ts, and ts + 1 two ticks before.
// GAUGES: g is the masked (T, n_gauges) block and slot the engine-order map, so a position's dL/d(discharge) is the block's element
// at (t, slot[p]) or 0.0; a headwater needs it as much as an inner reach (its row is dL/dout + ...).  dst and the block are different
// memory there.
// ENS: member blockIdx.z (y walks the rows), its gradient rows (dst, g) at row_pitch -- its block T * n_gauges doubles after the
// previous member's --, its dL/d(q_full final) row at gf_pitch, its mu tape at tape_pitch.
struct UnitRowsMember { int64_t row_pitch, gf_pitch, tape_pitch; };
template <bool GAUGES> struct UnitRowsCotangent { const double *g; };      // dL/d(discharge): dense rows, or the blocks and their slot map
template <> struct UnitRowsCotangent<true> { const double *g; const int32_t *slot; int64_t n_gauges; };
template <bool ENS, bool GAUGES>
__global__ __launch_bounds__(kBlock) void k_adj_rows_unit(double *dst, const UnitRowsCotangent<GAUGES> cot, const double *gff, const double *mtape,
                                                          const int32_t *lag, const int32_t *child_ptr, const int32_t *down, const double *w,
                                                          const double *c2, int64_t n, int64_t T, int64_t nsub, int64_t total_substeps,
                                                          int32_t dmax, const ArgsIf<ENS, UnitRowsMember> mp)
{
    const double *g = cot.g;
    if constexpr (ENS) {
        const int64_t member = blockIdx.z;
        dst += member * mp.row_pitch; mtape += member * mp.tape_pitch;
        if constexpr (GAUGES) { if (g) g += member * T * cot.n_gauges; }
        else if (g) g += member * mp.row_pitch;
        if (gff) gff += member * mp.gf_pitch;
    }
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= n) return;
    const int64_t base = total_substeps - 1 + dmax - (lag[p] & kLagMask);      // this position's reverse tick of forward sub-step 0
    const bool hw = child_ptr[p] == child_ptr[p + 1];
    const int32_t d = down[p];
    const double c1d = d >= 0 ? w[p] : 0.0, c2d = d >= 0 ? c2[d] : 0.0;
    const double *md = mtape + (d >= 0 ? d : 0);
    int32_t j = -1;                                                            // the gauge column of this position
    if constexpr (GAUGES) j = g ? cot.slot[p] : -1;
    for (int64_t t = blockIdx.y; t < T; t += gridDim.y) {
        double gv;
        if constexpr (GAUGES) gv = j >= 0 ? g[t * cot.n_gauges + j] : 0.0;
        else gv = g ? g[t * n + p] : 0.0;
        double v;
        if (hw) {
            double m = 0.0;
            if (d >= 0) for (int64_t k = 0; k < nsub; ++k) m += md[(base - (t * nsub + k) - 1) * n];
            v = __builtin_fma(c1d + c2d, m, gv);
        } else {
            v = 0.0;
            for (int64_t k = 0; k < nsub; ++k) {
                const int64_t ts = t * nsub + k;
                double phi = gv;
                if (ts == total_substeps - 1 && gff) phi += gff[p];
                if (d >= 0) {
                    phi = __builtin_fma(c1d, md[(base - ts - 1) * n], phi);
                    if (ts < total_substeps - 1) phi = __builtin_fma(c2d, md[(base - ts - 2) * n], phi);
                }
                v += phi;
            }
        }
        dst[t * n + p] = v;
    }
}

// ---- adjoint of the unit-hydrograph convolution (UnitHydrograph.py:93-107) ----
// buf[t'] = sum_j kernel[j] depth[t' - j] + [t' < n_ks] state[t'] for t' < T + n_ks - 1; convolved = buf[:T], state_out[:n_ks-1] =
// buf[T:], state_out[n_ks-1] = 0.  G[t'] = dL/dbuf[t']: dL/dconvolved[t'] below T, dL/dstate_out[t' - T] from T to T + n_ks - 2, else 0.
struct UhGrad {
    const double *gconv, *gstate;      // either may be NULL
    int64_t T, n, top;                 // top = T + n_ks - 1
    __device__ __forceinline__ double at(int64_t tp, int64_t i) const
    {
        if (tp < T) return gconv ? gconv[tp * n + i] : 0.0;
        return (gstate && tp < top) ? gstate[(tp - T) * n + i] : 0.0;
    }
};

// dL/ddepth[t, i] = sum_j kernel[j, i] G[t + j, i]: k_uh_convolve's sliding register window run the other way.  One reach per
// lane, TB consecutive rows per thread.
template <int TB>
__global__ __launch_bounds__(kBlock) void k_uh_adjoint_depth(const double *__restrict__ kernel, const UhGrad G, double *__restrict__ grad_depth,
                                                             int32_t n_ks)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= G.n) return;
    const int64_t t0 = (int64_t)blockIdx.y * TB;
    double acc[TB], win[TB];
#pragma unroll
    for (int j = 0; j < TB; ++j) { acc[j] = 0.0; win[j] = G.at(t0 + j, i); }
    for (int32_t s = 0; s < n_ks; ++s) {
        const double kv = kernel[(int64_t)s * G.n + i];
#pragma unroll
        for (int j = 0; j < TB; ++j) acc[j] = __builtin_fma(kv, win[j], acc[j]);
#pragma unroll
        for (int j = 0; j < TB - 1; ++j) win[j] = win[j + 1];
        win[TB - 1] = G.at(t0 + TB + s, i);
    }
#pragma unroll
    for (int j = 0; j < TB; ++j)
        if (t0 + j < G.T) grad_depth[(t0 + j) * G.n + i] = acc[j];
}

// Partial dL/dkernel[j, i] = sum_t depth[t, i] G[t + j, i] over one range of rows (blockIdx.y) for JB taps (blockIdx.z): the G
// window of the tap block slides in registers, one new value and one depth value per row.  slab[split][j][i]; with one range the
// slab is the result itself.
template <int JB>
__global__ __launch_bounds__(kBlock) void k_uh_adjoint_kernel(const double *__restrict__ depth, const UhGrad G, double *__restrict__ slab,
                                                              int32_t n_ks, int64_t rows_per_split)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= G.n) return;
    const int64_t t0 = (int64_t)blockIdx.y * rows_per_split, t1 = min(G.T, t0 + rows_per_split);
    const int32_t j0 = (int32_t)blockIdx.z * JB;
    double acc[JB], win[JB];
#pragma unroll
    for (int j = 0; j < JB; ++j) { acc[j] = 0.0; win[j] = G.at(t0 + j0 + j, i); }
    for (int64_t t = t0; t < t1; ++t) {
        const double dv = depth[t * G.n + i];
#pragma unroll
        for (int j = 0; j < JB; ++j) acc[j] = __builtin_fma(dv, win[j], acc[j]);
#pragma unroll
        for (int j = 0; j < JB - 1; ++j) win[j] = win[j + 1];
        win[JB - 1] = G.at(t + 1 + j0 + JB - 1, i);
    }
    double *out = slab + ((int64_t)blockIdx.y * n_ks + j0) * G.n + i;
#pragma unroll
    for (int j = 0; j < JB; ++j)
        if (j0 + j < n_ks) out[(int64_t)j * G.n] = acc[j];
}

// The row ranges merged in order.
__global__ __launch_bounds__(kBlock) void k_uh_adjoint_merge(const double *slab, int64_t splits, int64_t count, double *grad_kernel)
{
    for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k < count; k += (int64_t)gridDim.x * kBlock) {
        double v = 0.0;
        for (int64_t s = 0; s < splits; ++s) v += slab[s * count + k];
        grad_kernel[k] = v;
    }
}

// dL/dstate[t', i] = G[t', i] for t' < n_ks.
__global__ __launch_bounds__(kBlock) void k_uh_adjoint_state(const UhGrad G, double *grad_state, int64_t n_ks)
{
    for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k < n_ks * G.n; k += (int64_t)gridDim.x * kBlock)
        grad_state[k] = G.at(k / G.n, k % G.n);
}

}  // namespace
