// rr_adjoint.hpp -- the host side of the routing adjoints (rr_rapid_adjoint_*, rr_unit_adjoint_*): one driver
// (refusals, work-memory layout, forward replay, reverse sweep) and, per router, the kernels plugged into it and a few checks of its own.
// Part of the one translation unit rr_engine.hip builds (included from there, after rr_exec.hpp; not a stand-alone header).
#pragma once

namespace {

constexpr int64_t kAdjPermRows = 16;          // rows per pass of the tiled permutation
constexpr int64_t kAdjTargetBlocks = 2048;    // blocks of a split reduction: column blocks x sub-step ranges x members
constexpr int64_t kAdjMaxMembers = 65535;     // members of a batched call: a grid's second and third dimension

// What differs between the two routers outside the kernels: the name of the sizing entry point (the errors name it) and two row counts
// of the work memory: sums per reach in the reduction (c1..c4 / c1..c3) and scratch rows (the tick's running sum and its discarded
// discharge row; Unit adds q_ch, updated in place, q_ch0, dL/d(q_ch final) and dL/d(q_full final) in engine order).
// batch: the member-batched entry points; gauges: rr_rapid_adjoint_gauges_* and rr_unit_adjoint_gauges_*, dL/d(discharge) at gauged
// reaches only
struct AdjointKind { const char *sizer; int64_t slab_rows, scratch_rows; bool batch = false, gauges = false; };
constexpr AdjointKind kRapidAdjoint{"rr_rapid_adjoint_work_bytes", 4, 2};
constexpr AdjointKind kRapidAdjointBatch{"rr_rapid_adjoint_batch_work_bytes", 4, 2, true};
constexpr AdjointKind kRapidAdjointGauges{"rr_rapid_adjoint_gauges_work_bytes", 4, 2, true, true};
constexpr AdjointKind kUnitAdjoint{"rr_unit_adjoint_work_bytes", 3, 6};
constexpr AdjointKind kUnitAdjointBatch{"rr_unit_adjoint_batch_work_bytes", 3, 6, true};
constexpr AdjointKind kUnitAdjointGauges{"rr_unit_adjoint_gauges_work_bytes", 3, 6, true, true};

// The work memory of one adjoint call, in doubles, front to back: q tape (S + depth + 1 rows: ticks -2 .. S + Dmax - 1), mu tape
// (S + depth - 1 rows: reverse ticks 0 .. S + Dmax - 1; before the reverse ticks it holds the masked dL/d(discharge) in params
// order), lateral rows and gradient rows in engine order (T rows each), the permutation's intermediate rows, the reduction slab
// (slab_rows x n per sub-step range), the scratch rows.  A batched call (members > 1) has every section but the permutation's rows
// once per member, member m's part m pitches into the section: with one member this is the single call's layout, byte for byte.
// A gauge call (n_gauges > 0) keeps its masked (T, n_gauges) blocks, members adjacent, in the permutation's rows, which grow to hold
// them: the rows are idle from the lateral rows' permutation to the gradient rows', and the reverse ticks, which read the blocks, lie
// between (so does UnitMuskingum's row pass, which reads them too).  Its slot map (2 n int32) lives in member 0's first scratch row,
// the replay's, idle once the replay is enqueued; the rows Unit adds are not idle and lie behind it.  Without grad_rows (no
// grad_lateral) it has no gradient rows.
struct AdjointLayout {
    int64_t qtape, mtape, lat, grad, mrows, slab, scratch, total;      // offsets and total in doubles
    int64_t chunk, splits, steps_per_split;
    int64_t qtape_pitch, mtape_pitch, row_pitch, slab_pitch, scratch_pitch;      // doubles from one member's part to the next
};

AdjointLayout adjoint_layout(int64_t n, int64_t depth, int64_t T, int64_t nsub, const AdjointKind &K, int64_t members = 1,
                             int64_t n_gauges = 0, bool grad_rows = true)
{
    AdjointLayout L{};
    const int64_t S = T * nsub;
    L.chunk = std::min<int64_t>(T, kAdjPermRows);
    const int64_t col_blocks = ((n + kBlock - 1) / kBlock) * members;
    const int64_t want = std::max<int64_t>(1, (kAdjTargetBlocks + col_blocks - 1) / col_blocks);
    L.splits = std::max<int64_t>(1, std::min(want, S));
    L.steps_per_split = (S + L.splits - 1) / L.splits;
    L.splits = (S + L.steps_per_split - 1) / L.steps_per_split;
    L.qtape_pitch = (S + depth + 1) * n; L.mtape_pitch = (S + depth - 1) * n; L.row_pitch = T * n;
    L.slab_pitch = L.splits * K.slab_rows * n; L.scratch_pitch = K.scratch_rows * n;
    L.qtape = 0;
    L.mtape = L.qtape + members * L.qtape_pitch;
    L.lat = L.mtape + members * L.mtape_pitch;
    L.grad = L.lat + members * L.row_pitch;
    L.mrows = L.grad + (grad_rows ? members * L.row_pitch : 0);
    L.slab = L.mrows + std::max(L.chunk * n, members * T * n_gauges);
    L.scratch = L.slab + members * L.slab_pitch;
    L.total = L.scratch + members * L.scratch_pitch;
    return L;
}

// Plan data the adjoint reads besides the streaming layout: the tiled permutation tables and the downstream position of each position.
int adjoint_ready(rr_plan *P)
{
    if (!P->perm_ready) {
        int rc = upload_tiled_permutations(P);
        if (rc) return rc;
    }
    if (!P->d_adj_down) {
        const rr::HostPlan &H = P->h;
        std::vector<int32_t> down(H.n, -1);
        for (int64_t p = 0; p < H.n; ++p)
            for (int32_t u = H.child_ptr[p]; u < H.child_ptr[p + 1]; ++u) down[u] = (int32_t)p;
        DevBuf<int32_t> d;
        if (int rc = assign(d, down)) return rc;
        P->d_adj_down = std::move(d);
    }
    return RR_OK;
}

// One adjoint call: the arguments every *_adjoint_dev entry point has, and, once adjoint_check has passed, the sizes and the tapes.
struct AdjointCall {
    rr_plan *P;
    const double *lateral; int64_t lat_rows;
    const double *discharge, *grad_out;
    void *work; int64_t work_bytes;
    int64_t T, nsub;
    hipStream_t st;
    // a batched call (rr_rapid_adjoint_batch_*, rr_unit_adjoint_batch_*): members, and the doubles from one member's q0 (0: one q0
    // for all), lateral / grad_lateral rows and discharge / grad_out rows to the next's; for UnitMuskingum, whose states have n_inner
    // values, state_pitch instead of q0_pitch (0: one q_ch0 and one q_full0 for all).  The single-member entry points leave these as they are.
    int64_t members = 1, q0_pitch = 0, lat_pitch = 0, out_pitch = 0, state_pitch = 0;
    // a gauge call (rr_rapid_adjoint_gauges_*, rr_unit_adjoint_gauges_*): discharge and grad_out are (T, n_gauges) at reaches gauges[] (out_pitch: the gauge pitch);
    // grad_rows: the work memory has gradient rows (the sizer's with_grad_lateral; in a *_dev call, grad_lateral is given)
    int64_t n_gauges = 0; const int32_t *gauges = nullptr; bool grad_rows = true;
    // set by adjoint_check
    int64_t n, S, dmax, ticks;
    bool one;                                                       // nsub == 1: the kernels' SINGLE_SUBSTEP forms
    AdjointLayout L;
    double *qtape, *mtape, *elat, *egrad, *mrows, *slab, *scratch;

    // T rows of every member, params <-> engine order; member m's rows m pitches from the first's (one stream: the members share mrows)
    void rows_between(int which, const double *src, double *dst, int64_t src_pitch = 0, int64_t dst_pitch = 0) const
    {
        for (int64_t m = 0; m < members; ++m)
            for (int64_t t0 = 0; t0 < T; t0 += L.chunk)
                permute_rows_via(P, which, RowView{const_cast<double *>(src) + m * src_pitch, n, 0, (uint32_t)T},
                                 RowView{dst + m * dst_pitch, n, 0, (uint32_t)T}, t0, (int)std::min<int64_t>(L.chunk, T - t0), mrows, st);
    }
    // masked dL/d(discharge): (T, n) in engine order, or a gauge call's (T, n_gauges) blocks
    const double *egrad_out() const { return !grad_out ? nullptr : n_gauges ? gblock() : egrad; }
    double *gblock() const { return mrows; }
    int32_t *pslot() const { return reinterpret_cast<int32_t *>(scratch); }      // params order; the engine-order map follows it
    int32_t *slot() const { return pslot() + n; }
    dim3 reduce_grid() const { return dim3((unsigned)((n + kBlock - 1) / kBlock), (unsigned)L.splits, (unsigned)members); }
    template <bool ENS> AdjMergeRanges<ENS> merge_ranges() const      // what the merges fold: the slab's ranges, of every member
    {
        AdjMergeRanges<ENS> r{L.splits};
        if constexpr (ENS) r.members = members;
        return r;
    }
};

// A check that is an entry point's own: after which shared ones it is tested (the plan's boundary check, the sizes, the lateral rows,
// grad_out, the member pitches), whether it is hit, its status and text.  kAdjNothing is no refusal: no gradient is asked for, the call
// returns RR_OK.
enum class AdjOwn { Plan, Wanted, Lateral, GradOut, Pitch };
constexpr int kAdjNothing = 1;
struct OwnCheck { AdjOwn at; bool hit; int code; const char *what; };

// The refusals of the four entry points, in the order they are tested; `who` names the entry point in the errors.  With `bytes`, a
// sizing call (reads c.P, c.T, c.nsub; uploads the plan's tables); without, a *_dev call, whose context is filled in at the end.
int adjoint_check(const char *who, const AdjointKind &K, AdjointCall &c, int64_t *bytes, std::initializer_list<OwnCheck> own_checks)
{
    const auto no = [who](int code, const char *what) { return code > 0 ? code : fail(code, std::string(who) + what); };
    const auto own = [&](AdjOwn at) {
        for (const OwnCheck &o : own_checks)
            if (o.at == at && o.hit) return no(o.code, o.what);
        return RR_OK;
    };
    rr_plan *P = c.P;
    const bool sizing = bytes != nullptr;
    if (!P) return no(RR_E_INVALID, sizing ? ": null argument" : ": null plan");
    if (sizing) *bytes = 0;
    if (P->device < 0) return no(RR_E_UNSUPPORTED, ": host-only plan (RR_DEVICE_NONE): the adjoint runs on the GPU only");
    if (!sizing) {
        HIPCHK(hipSetDevice(P->device));
        if (P->n_ghost > 0 || P->n_export > 0)
            return no(RR_E_UNSUPPORTED, ": the plan has boundary reaches (rr_plan_set_boundary): partitioned networks have no adjoint");
        if (int rc = own(AdjOwn::Plan)) return rc;
        if (!P->coeffs_set) return no(RR_E_STATE, " called before rr_plan_set_coeffs");
        if (!P->weights_uniform)
            return no(RR_E_UNSUPPORTED, ": per-edge weights (lhs_off_data not -c1 of the downstream reach): the adjoint needs one c1 per reach");
        if (P->ses.open) return no(RR_E_STATE, ": a routing call is open");
    }
    const rr::HostPlan &H = P->h;
    const int64_t n = H.n, T = c.T, nsub = c.nsub;
    if (T < 1 || nsub < 1 || nsub > 0x7FFFFFFF) return no(RR_E_INVALID, ": need T >= 1 and sub-steps >= 1");
    if (T * nsub + H.depth > 0x7FFFFFFFLL) return no(RR_E_INVALID, ": too many sub-steps for one call: split the series into windows");
    if (K.gauges && (c.n_gauges < 1 || c.n_gauges > n)) return no(RR_E_INVALID, ": need 1 <= n_gauges <= n");
    const auto members_ok = [&] { return c.members >= 1 && c.members <= kAdjMaxMembers; };
    if (sizing) {
        if (!members_ok()) return no(RR_E_INVALID, ": need 1 <= members <= 65535");
        HIPCHK(hipSetDevice(P->device));
        if (n == 0) return RR_OK;
        if (int rc = adjoint_ready(P)) return rc;
        *bytes = adjoint_layout(n, H.depth, T, nsub, K, c.members, c.n_gauges, c.grad_rows).total * (int64_t)sizeof(double);
        return RR_OK;
    }
    if (int rc = own(AdjOwn::Wanted)) return rc;
    if (c.lateral && c.lat_rows < T) return no(RR_E_INVALID, ": fewer lateral rows than T");
    if (int rc = own(AdjOwn::Lateral)) return rc;
    if (c.grad_out && !c.discharge) return no(RR_E_INVALID, ": grad_out needs the discharge of the forward call (its clamp mask)");
    if (int rc = own(AdjOwn::GradOut)) return rc;
    if (!members_ok()) return no(RR_E_INVALID, ": need 1 <= members <= 65535");
    const bool out_short = K.gauges ? c.members > 1 && c.out_pitch < T * c.n_gauges : c.out_pitch < T * n;
    if (K.batch && ((c.q0_pitch != 0 && c.q0_pitch < n) || (c.lateral && c.lat_pitch < T * n) || ((c.discharge || c.grad_out) && out_short)))
        return no(RR_E_INVALID, K.gauges ? ": a member pitch shorter than one member's rows (q0_pitch: 0 or >= n; lat_pitch >= T * n; gauge_pitch >= T * n_gauges)"
                                         : ": a member pitch shorter than one member's rows (q0_pitch: 0 or >= n; lat_pitch, out_pitch >= T * n)");
    if (int rc = own(AdjOwn::Pitch)) return rc;
    const AdjointLayout L = adjoint_layout(n, H.depth, T, nsub, K, c.members, c.n_gauges, c.grad_rows);
    const int64_t need = L.total * (int64_t)sizeof(double);
    if (!c.work || c.work_bytes < need)
        return fail(RR_E_INVALID, std::string(who) + ": work memory smaller than " + K.sizer + " (" + std::to_string(need) + " bytes)");
    if (!P->perm_ready || !P->d_adj_down)
        return fail(RR_E_STATE, std::string(who) + ": call " + K.sizer + " first (it uploads the plan's permutation tables once)");

    c.n = n; c.S = T * nsub; c.dmax = H.depth - 1; c.ticks = c.S + c.dmax; c.one = nsub == 1; c.L = L;
    double *const base = static_cast<double *>(c.work);
    c.qtape = base + L.qtape; c.mtape = base + L.mtape; c.elat = base + L.lat; c.egrad = base + L.grad; c.mrows = base + L.mrows;
    c.slab = base + L.slab; c.scratch = base + L.scratch;
    return RR_OK;
}

int adjoint_work_bytes(const AdjointKind &K, rr_plan *P, int64_t T, int64_t nsub, int64_t *bytes, int64_t members = 1, int64_t n_gauges = 0,
                       bool grad_rows = true)
{
    if (!bytes) return fail(RR_E_INVALID, std::string(K.sizer) + ": null argument");
    AdjointCall c{};
    c.P = P; c.T = T; c.nsub = nsub; c.members = members; c.n_gauges = n_gauges; c.grad_rows = grad_rows;
    return adjoint_check(K.sizer, K, c, bytes, {});
}

// The forward again, into a tick-indexed tape: the tick kernel as the route calls run it, with its three rotating rows spread over the
// q tape.  Fills `a` (the TickArgs of the call, or the one inside a UnitTickArgs) and calls launch(grid) for every tick with work.
template <class Launch>
void adjoint_replay(const AdjointCall &c, TickArgs &a, Launch launch)
{
    const rr_plan *P = c.P;
    const int64_t n = c.n;
    a.child_ptr = P->d_child_ptr; a.lag = P->d_lag; a.w = P->d_w; a.c1row = P->d_c1row_h; a.c2 = P->d_c2; a.c3 = P->d_c3; a.c4 = P->d_c4;
    a.isum = c.scratch; a.bidx = P->d_bidx; a.ghost = nullptr; a.exports = nullptr; a.n_ghost = 0; a.n_export = 0;
    a.in = c.lateral ? c.elat : nullptr; a.in_ld = n; a.in_rows = Div32((uint32_t)c.T);
    a.out = c.scratch + n; a.out_ld = 0; a.out_rows = Div32(1u);      // discharge rows are not kept: every row lands on one scratch row
    a.total_substeps = c.S; a.nsub = Div32((uint32_t)c.nsub); a.inv_nsub = 1.0 / (double)c.nsub;
    for (int64_t tau = 0; tau < c.ticks; ++tau) {
        int64_t p_lo, p_hi;
        if (!tick_window(P->h, tau, c.S, p_lo, p_hi)) continue;
        a.p_lo = (int32_t)p_lo; a.p_hi = (int32_t)p_hi; a.tau = tau;
        a.xc = c.qtape + (tau + 2) * n; a.xa = a.xc - n; a.xb = a.xc - 2 * n;
        launch(grid1(p_hi - p_lo));
    }
}

// The reverse ticks: the reach at lag l runs reverse step tau - (Dmax - l), so the window of active lags is the forward's mirrored.
// Fills the fields AdjTickArgs and UnitAdjTickArgs share and calls launch(grid) for every tick with work.
template <class Args, class Launch>
void adjoint_reverse(const AdjointCall &c, Args &a, Launch launch)
{
    const rr_plan *P = c.P;
    const rr::HostPlan &H = P->h;
    const int64_t n = c.n, S = c.S, dmax = c.dmax;
    a.lag = P->d_lag; a.down = P->d_adj_down; a.w = P->d_w; a.c2 = P->d_c2; a.c3 = P->d_c3; a.g = c.egrad_out();
    a.n = n; a.dmax = (int32_t)dmax; a.total_substeps = S; a.nsub = Div32((uint32_t)c.nsub);
    for (int64_t tau = 0; tau < c.ticks; ++tau) {
        const int64_t lag_lo = std::max<int64_t>(0, dmax - tau), lag_hi = std::min<int64_t>(dmax, dmax - tau + S - 1);
        const int64_t p_lo = H.lag_start[lag_lo], p_hi = H.lag_start[lag_hi + 1];
        if (p_hi <= p_lo) continue;
        a.p_lo = (int32_t)p_lo; a.p_hi = (int32_t)p_hi; a.tau = tau;
        a.mc = c.mtape + tau * n;
        a.ma = tau >= 1 ? a.mc - n : a.mc;      // never read at tick 0 (nothing runs r > 0 or has a downstream reach there)
        a.mb = tau >= 2 ? a.mc - 2 * n : a.mc;  // read from tick 2 on only
        launch(grid1(p_hi - p_lo));
    }
}

// The fields AdjReduceArgs and UnitAdjReduceArgs share; the reduction runs on c.reduce_grid().
template <class Args>
void adjoint_reduce_args(const AdjointCall &c, Args &r)
{
    const rr_plan *P = c.P;
    r.lag = P->d_lag; r.child_ptr = P->d_child_ptr; r.qtape = c.qtape; r.mtape = c.mtape; r.lat = c.lateral ? c.elat : nullptr; r.slab = c.slab;
    r.n = c.n; r.total_substeps = c.S; r.steps_per_split = c.L.steps_per_split; r.dmax = (int32_t)c.dmax; r.nsub = Div32((uint32_t)c.nsub);
}

// The kernel forms of a checked call, stated once for both routers: enqueue(ENS, GAUGES) with the two flags as std::bool_constant.  A
// gauge call with one member runs the single-member kernels, so the single call's bits; a batch call runs the member forms whatever the
// member count; a plain call the single-member forms.
template <class Enqueue>
void adjoint_forms(const AdjointKind &K, const AdjointCall &c, Enqueue enqueue)
{
    const bool ens = K.gauges ? c.members > 1 : K.batch;
    if (K.gauges) ens ? enqueue(std::true_type{}, std::true_type{}) : enqueue(std::false_type{}, std::true_type{});
    else ens ? enqueue(std::true_type{}, std::false_type{}) : enqueue(std::false_type{}, std::false_type{});
}

// ---- RapidMuskingum ----

// What a checked call enqueues.  ENS: a batched call (rr_rapid_adjoint_batch_dev) -- the member-batched kernels on grids with a member
// dimension, so the two sweeps launch once per tick whatever the member count; otherwise the single-member kernels, launched as ever.
// GAUGES: a gauge call (rr_rapid_adjoint_gauges_dev) -- the mask runs over the (T, n_gauges) blocks, no cotangent is permuted and the
// reverse tick is its gauge form; the replay, the reduction, the merge and the row pass are the dense call's.
template <bool ENS, bool GAUGES = false>
void rapid_adjoint_enqueue(const AdjointCall &c, const double *q0, const double *grad_qfinal, double *grad_lateral, double *grad_q0,
                           double *grad_coef)
{
    rr_plan *const P = c.P;
    const double *const lateral = c.lateral, *const discharge = c.discharge, *const grad_out = c.grad_out;
    const int64_t T = c.T, nsub = c.nsub, n = c.n, S = c.S;
    const hipStream_t st = c.st;
    const AdjointLayout &L = c.L;
    const unsigned M = (unsigned)c.members;
    const int64_t lat_pitch = ENS ? c.lat_pitch : 0, out_pitch = ENS ? c.out_pitch : 0;
    // dL/d(discharge): clamp mask and mean in params order (in the mu tape's memory, free until the reverse ticks), then engine order
    if (grad_out && !GAUGES) {
        const int64_t count = T * n;
        const dim3 g((unsigned)std::min<int64_t>((count + kBlock - 1) / kBlock, 8192), M);
        hipLaunchKernelGGL(k_adj_mask<ENS>, g, dim3(kBlock), 0, st, c.mtape, grad_out, discharge, count, 1.0 / (double)nsub,
                           args_if<ENS>(AdjMaskMember{L.mtape_pitch, out_pitch}));
        c.rows_between(0, c.mtape, c.egrad, L.mtape_pitch, L.row_pitch);
    }
    if (grad_coef) {
        if (lateral) c.rows_between(0, lateral, c.elat, lat_pitch, L.row_pitch);
        const dim3 g((unsigned)((n + kBlock - 1) / kBlock), M);
        hipLaunchKernelGGL(k_adj_tape_init<ENS>, g, dim3(kBlock), 0, st, c.qtape, q0, (const int32_t *)P->d_perm, (const int32_t *)P->d_lag, n,
                           args_if<ENS>(AdjTapeInitMember{L.qtape_pitch, c.q0_pitch}));
        TickArgsOf<ENS> a{};
        if constexpr (ENS) { a.tape_pitch = L.qtape_pitch; a.in_pitch = L.row_pitch; a.scratch_pitch = L.scratch_pitch; }
        const auto tick = lateral ? (c.one ? k_tick<true, true, ENS> : k_tick<true, false, ENS>) : (c.one ? k_tick<false, true, ENS> : k_tick<false, false, ENS>);
        adjoint_replay(c, a, [&](dim3 g) { g.y = M; hipLaunchKernelGGL(tick, g, dim3(kBlock), 0, st, a); });
    }
    // a gauge call's dL/d(discharge): clamp mask and mean over the (T, n_gauges) blocks, and the slot map.  The blocks lie in the
    // permutation's rows and the map in scratch rows: what used them, the lateral rows' permutation and the replay, is enqueued already
    if (GAUGES && grad_out) {
        const int64_t count = T * c.n_gauges;
        const dim3 g((unsigned)std::min<int64_t>((count + kBlock - 1) / kBlock, 8192), M);
        hipLaunchKernelGGL(k_adj_mask<ENS>, g, dim3(kBlock), 0, st, c.gblock(), grad_out, discharge, count, 1.0 / (double)nsub,
                           args_if<ENS>(AdjMaskMember{count, out_pitch}));
        hipLaunchKernelGGL(k_adj_gauge_fill, grid1(n), dim3(kBlock), 0, st, c.pslot(), n);
        hipLaunchKernelGGL(k_adj_gauge_scatter, grid1(c.n_gauges), dim3(kBlock), 0, st, c.pslot(), c.gauges, c.n_gauges);
        hipLaunchKernelGGL(k_adj_gauge_slots, grid1(n), dim3(kBlock), 0, st, c.slot(), (const int32_t *)c.pslot(), (const int32_t *)P->d_perm, n);
    }
    AdjTickArgsOf<ENS, GAUGES> ra{};
    ra.gf = grad_qfinal; ra.perm = P->d_perm;
    if constexpr (ENS) { ra.tape_pitch = L.mtape_pitch; ra.g_pitch = GAUGES ? T * c.n_gauges : L.row_pitch; ra.gf_pitch = n; }
    if constexpr (GAUGES) { ra.slot = c.slot(); ra.n_gauges = c.n_gauges; }
    adjoint_reverse(c, ra, [&](dim3 g) {
        g.y = M;
        hipLaunchKernelGGL((c.one ? k_adj_tick<true, ENS, GAUGES> : k_adj_tick<false, ENS, GAUGES>), g, dim3(kBlock), 0, st, ra);
    });
    if (grad_coef) {
        AdjReduceArgsOf<ENS> r{};
        adjoint_reduce_args(c, r);
        if constexpr (ENS) { r.qtape_pitch = L.qtape_pitch; r.mtape_pitch = L.mtape_pitch; r.lat_pitch = L.row_pitch; r.slab_pitch = L.slab_pitch; }
        hipLaunchKernelGGL((c.one ? k_adj_reduce<true, ENS> : k_adj_reduce<false, ENS>), c.reduce_grid(), dim3(kBlock), 0, st, r);
    }
    if (grad_coef || grad_q0) {      // without dL/dq0 only member 0's blocks have work: they fold every member's ranges
        dim3 g = grid1(n);
        g.y = grad_q0 ? M : 1u;
        hipLaunchKernelGGL(k_adj_merge<ENS>, g, dim3(kBlock), 0, st, (const double *)c.slab, c.merge_ranges<ENS>(), (const double *)c.mtape,
                           (const int32_t *)P->d_lag, (const int32_t *)P->d_adj_down, (const int32_t *)P->d_perm, (const double *)P->d_c2,
                           (const double *)P->d_c3, n, S, (int32_t)c.dmax, lateral ? 1 : 0, grad_coef, grad_q0,
                           args_if<ENS>(AdjMergeMember{L.mtape_pitch}));
    }
    if (grad_lateral) {
        const dim3 g((unsigned)((n + kBlock - 1) / kBlock), (unsigned)std::min<int64_t>(T, 65535), M);
        hipLaunchKernelGGL(k_adj_rows<ENS>, g, dim3(kBlock), 0, st, c.egrad, (const double *)c.mtape, (const int32_t *)P->d_lag,
                           (const double *)P->d_c4, n, T, nsub, S, (int32_t)c.dmax, args_if<ENS>(AdjRowsMember{L.row_pitch, L.mtape_pitch}));
        c.rows_between(1, c.egrad, grad_lateral, L.row_pitch, lat_pitch);
    }
}

int rapid_adjoint(const char *who, const AdjointKind &K, AdjointCall &c, const double *q0, const double *grad_qfinal, double *grad_lateral,
                  double *grad_q0, double *grad_coef)
{
    rr_plan *const P = c.P;
    const double *const lateral = c.lateral;
    const int rc = adjoint_check(who, K, c, nullptr, {
        {AdjOwn::Wanted, P && (P->h.n == 0 || (!grad_lateral && !grad_q0 && !grad_coef)), kAdjNothing, ""},
        {AdjOwn::Wanted, grad_coef && !q0, RR_E_INVALID, ": the coefficient gradients need q0"},
        {AdjOwn::Lateral, P && lateral && !P->has_c4, RR_E_STATE, ": lateral rows but no c4_dt (rr_plan_set_coeffs got NULL)"},
        {AdjOwn::Wanted, K.gauges && !c.gauges, RR_E_INVALID, ": null gauges"},
        {AdjOwn::GradOut, K.gauges && c.discharge && !c.grad_out, RR_E_INVALID, ": discharge_g and grad_out_g come together or not at all"},
        {AdjOwn::GradOut, grad_lateral && !lateral, RR_E_INVALID, ": grad_lateral of a channel-only call (lateral is NULL)"}});
    if (rc) return rc == kAdjNothing ? RR_OK : rc;
    adjoint_forms(K, c, [&](auto ens, auto gauges) {
        rapid_adjoint_enqueue<decltype(ens)::value, decltype(gauges)::value>(c, q0, grad_qfinal, grad_lateral, grad_q0, grad_coef);
    });
    HIPCHK(hipGetLastError());
    return RR_OK;
}

// ---- UnitMuskingum ----

// What a checked call enqueues, as rapid_adjoint_enqueue: ENS is a batched call (rr_unit_adjoint_batch_dev) on grids with a member
// dimension; otherwise the single-member kernels, launched as ever.  ni: the plan's inner reaches (0: no state and no tick).
// GAUGES: a gauge call (rr_unit_adjoint_gauges_dev) -- the output rule is applied over the (T, n_gauges) blocks, no cotangent is staged
// in the mu tape or permuted, and the reverse tick and the row pass are their gauge forms; the rest is the dense call's.
template <bool ENS, bool GAUGES = false>
void unit_adjoint_enqueue(const AdjointCall &c, int64_t ni, const double *q_ch0, const double *q_full0, const double *grad_qch_final,
                          const double *grad_qfull_final, double *grad_lateral, double *grad_qch0, double *grad_qfull0, double *grad_coef)
{
    rr_plan *const P = c.P;
    const double *const lateral = c.lateral, *const discharge = c.discharge, *const grad_out = c.grad_out;
    const int64_t T = c.T, nsub = c.nsub, n = c.n, S = c.S;
    const hipStream_t st = c.st;
    const AdjointLayout &L = c.L;
    const unsigned M = (unsigned)c.members;
    const int64_t lat_pitch = ENS ? c.lat_pitch : 0, out_pitch = ENS ? c.out_pitch : 0;
    double *const qch = c.scratch + 2 * n, *const qch0e = qch + n, *const gcf = qch0e + n, *const gff = gcf + n;      // member m's: m scratch pitches on
    const bool tape = grad_coef && ni > 0;
    const unsigned col_blocks = (unsigned)((n + kBlock - 1) / kBlock), row_blocks = (unsigned)std::min<int64_t>(T, 65535);
    dim3 inner_grid = grid1(ni);      // the kernels over the inner reaches
    inner_grid.y = M;
    // dL/d(discharge) with the forward's output rule in params order (in the mu tape's memory, free until the reverse ticks), then engine order
    if (grad_out && !GAUGES) {
        hipLaunchKernelGGL((k_adj_mask_unit<ENS, false>), dim3(col_blocks, row_blocks, M), dim3(kBlock), 0, st, c.mtape, grad_out, discharge,
                           UnitMaskColumns<false>{P->d_inv}, (const int32_t *)P->d_child_ptr, n, T, 1.0 / (double)nsub,
                           args_if<ENS>(UnitMaskMember{L.mtape_pitch, out_pitch}));
        c.rows_between(0, c.mtape, c.egrad, L.mtape_pitch, L.row_pitch);
    }
    if (ni > 0 && (tape || grad_qch_final || grad_qfull_final)) {
        hipLaunchKernelGGL(k_adj_unit_in<ENS>, inner_grid, dim3(kBlock), 0, st, c.qtape, qch, qch0e, tape ? q_full0 : nullptr, q_ch0, gcf, gff,
                           grad_qch_final, grad_qfull_final, (const int32_t *)P->d_inner_pos, (const int32_t *)P->d_lag, n, (int32_t)ni,
                           args_if<ENS>(UnitInMember{L.qtape_pitch, L.scratch_pitch, c.state_pitch}));
    }
    if (tape) {      // k_tick_unit on its one-weight branch
        c.rows_between(0, lateral, c.elat, lat_pitch, L.row_pitch);
        UnitTickArgsOf<ENS> ua{};
        ua.hw_children = P->d_hwc; ua.qch = qch; ua.a2 = nullptr; ua.c1own = nullptr; ua.zc = nullptr; ua.za = nullptr;
        if constexpr (ENS) { ua.tape_pitch = L.qtape_pitch; ua.in_pitch = L.row_pitch; ua.scratch_pitch = L.scratch_pitch; }
        adjoint_replay(c, ua.t, [&](dim3 g) {
            g.y = M;
            hipLaunchKernelGGL((c.one ? k_tick_unit<true, ENS> : k_tick_unit<false, ENS>), g, dim3(kBlock), 0, st, ua);
        });
    }
    // a gauge call's dL/d(discharge): the output rule over the (T, n_gauges) blocks, and the slot map.  The blocks lie in the
    // permutation's rows and the map in the replay's first scratch row: what used them, the lateral rows' permutation and the replay, is
    // enqueued already.  With no inner reach the row pass still reads both.
    if (GAUGES && grad_out) {
        const dim3 g((unsigned)((c.n_gauges + kBlock - 1) / kBlock), row_blocks, M);
        hipLaunchKernelGGL((k_adj_mask_unit<ENS, true>), g, dim3(kBlock), 0, st, c.gblock(), grad_out, discharge,
                           UnitMaskColumns<true>{c.gauges, P->d_inv}, (const int32_t *)P->d_child_ptr, c.n_gauges, T, 1.0 / (double)nsub,
                           args_if<ENS>(UnitMaskMember{T * c.n_gauges, out_pitch}));
        hipLaunchKernelGGL(k_adj_gauge_fill, grid1(n), dim3(kBlock), 0, st, c.pslot(), n);
        hipLaunchKernelGGL(k_adj_gauge_scatter, grid1(c.n_gauges), dim3(kBlock), 0, st, c.pslot(), c.gauges, c.n_gauges);
        hipLaunchKernelGGL(k_adj_gauge_slots, grid1(n), dim3(kBlock), 0, st, c.slot(), (const int32_t *)c.pslot(), (const int32_t *)P->d_perm, n);
    }
    if (ni > 0) {      // with no inner reach there is no state and no tick
        UnitAdjTickArgsOf<ENS, GAUGES> a{};
        a.child_ptr = P->d_child_ptr; a.gcf = grad_qch_final ? gcf : nullptr; a.gff = grad_qfull_final ? gff : nullptr;
        if constexpr (ENS) { a.tape_pitch = L.mtape_pitch; a.g_pitch = GAUGES ? T * c.n_gauges : L.row_pitch; a.gf_pitch = L.scratch_pitch; }
        if constexpr (GAUGES) { a.slot = c.slot(); a.n_gauges = c.n_gauges; }
        adjoint_reverse(c, a, [&](dim3 g) {
            g.y = M;
            hipLaunchKernelGGL((c.one ? k_adj_tick_unit<true, ENS, GAUGES> : k_adj_tick_unit<false, ENS, GAUGES>), g, dim3(kBlock), 0, st, a);
        });
    }
    if (tape) {
        UnitAdjReduceArgsOf<ENS> r{};
        adjoint_reduce_args(c, r);
        r.hw_children = P->d_hwc; r.qch0 = qch0e;
        if constexpr (ENS) {
            r.qtape_pitch = L.qtape_pitch; r.mtape_pitch = L.mtape_pitch; r.lat_pitch = L.row_pitch; r.qch0_pitch = L.scratch_pitch;
            r.slab_pitch = L.slab_pitch;
        }
        hipLaunchKernelGGL((c.one ? k_adj_reduce_unit<true, ENS> : k_adj_reduce_unit<false, ENS>), c.reduce_grid(), dim3(kBlock), 0, st, r);
    }
    if (grad_coef)
        hipLaunchKernelGGL(k_adj_merge_unit<ENS>, grid1(n), dim3(kBlock), 0, st, (const double *)c.slab, c.merge_ranges<ENS>(),
                           (const int32_t *)P->d_child_ptr, (const int32_t *)P->d_perm, n, grad_coef);
    if (grad_qch0 || grad_qfull0)
        hipLaunchKernelGGL(k_adj_state_unit<ENS>, inner_grid, dim3(kBlock), 0, st, grad_qch0, grad_qfull0, (const double *)c.mtape,
                           (const int32_t *)P->d_inner_pos, (const int32_t *)P->d_lag, (const int32_t *)P->d_adj_down, (const double *)P->d_c2,
                           (const double *)P->d_c3, n, (int32_t)ni, S, (int32_t)c.dmax, args_if<ENS>(UnitStateMember{L.mtape_pitch}));
    if (grad_lateral) {      // a gauge call's blocks are read here for the last time: the permutation after it takes their rows back
        UnitRowsCotangent<GAUGES> cot{c.egrad_out()};
        if constexpr (GAUGES) { cot.slot = c.slot(); cot.n_gauges = c.n_gauges; }
        hipLaunchKernelGGL((k_adj_rows_unit<ENS, GAUGES>), dim3(col_blocks, row_blocks, M), dim3(kBlock), 0, st, c.egrad, cot,
                           grad_qfull_final ? (const double *)gff : nullptr, (const double *)c.mtape, (const int32_t *)P->d_lag,
                           (const int32_t *)P->d_child_ptr, (const int32_t *)P->d_adj_down, (const double *)P->d_w, (const double *)P->d_c2, n, T,
                           nsub, S, (int32_t)c.dmax, args_if<ENS>(UnitRowsMember{L.row_pitch, L.scratch_pitch, L.mtape_pitch}));
        c.rows_between(1, c.egrad, grad_lateral, L.row_pitch, lat_pitch);
    }
}

int unit_adjoint(const char *who, const AdjointKind &K, AdjointCall &c, const double *q_ch0, const double *q_full0, const double *grad_qch_final,
                 const double *grad_qfull_final, double *grad_lateral, double *grad_qch0, double *grad_qfull0, double *grad_coef)
{
    rr_plan *const P = c.P;
    const double *const lateral = c.lateral;
    const int64_t ni = P ? (int64_t)P->h.inner_pos.size() : 0;
    if (ni == 0) { grad_qch0 = nullptr; grad_qfull0 = nullptr; }      // no inner reach: the state vectors are empty
    // grad_lateral lies at lat_pitch whether or not the lateral rows are given (they are needed with grad_coef only)
    const bool rows_ok = c.T >= 1 && c.T <= 0x7FFFFFFFLL;
    const int rc = adjoint_check(who, K, c, nullptr, {
        {AdjOwn::Plan, P && P->unit_general, RR_E_UNSUPPORTED,
         ": general edge data (rr_plan_set_unit_weights): the adjoint is that of the reference callers' unit weights"},
        {AdjOwn::Wanted, P && (P->h.n == 0 || (!grad_lateral && !grad_qch0 && !grad_qfull0 && !grad_coef)), kAdjNothing, ""},
        {AdjOwn::Wanted, grad_coef && ni > 0 && (!q_ch0 || !q_full0 || !lateral), RR_E_INVALID,
         ": the coefficient gradients need q_ch0, q_full0 and the lateral rows"},
        {AdjOwn::Wanted, K.gauges && !c.gauges, RR_E_INVALID, ": null gauges"},
        {AdjOwn::GradOut, K.gauges && c.discharge && !c.grad_out, RR_E_INVALID, ": discharge_g and grad_out_g come together or not at all"},
        {AdjOwn::Pitch, K.batch && P && rows_ok && (c.state_pitch < 0 || (c.state_pitch != 0 && c.state_pitch < ni) ||
                                                    (grad_lateral && c.lat_pitch < c.T * P->h.n)), RR_E_INVALID,
         K.gauges ? ": a member pitch shorter than one member's states or rows (state_pitch: 0 or >= n_inner; lat_pitch >= T * n)"
                  : ": a member pitch shorter than one member's states or rows (state_pitch: 0 or >= n_inner; lat_pitch, out_pitch >= T * n)"}});
    if (rc) return rc == kAdjNothing ? RR_OK : rc;
    adjoint_forms(K, c, [&](auto ens, auto gauges) {
        unit_adjoint_enqueue<decltype(ens)::value, decltype(gauges)::value>(c, ni, q_ch0, q_full0, grad_qch_final, grad_qfull_final, grad_lateral,
                                                                            grad_qch0, grad_qfull0, grad_coef);
    });
    HIPCHK(hipGetLastError());
    return RR_OK;
}

}  // namespace
