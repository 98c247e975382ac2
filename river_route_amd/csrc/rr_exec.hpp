// rr_exec.hpp -- the plan object and the executor: schedule choice, record ring, streaming session, host PCIe pipeline,
// the route cores behind the C ABI.  Part of the one translation unit rr_engine.hip builds.
#pragma once

#include <atomic>

#include "rr_devbuf.hpp"

using rr::DevBuf;

// ------------------------------------------------------------------------------------------------
// plan object
// ------------------------------------------------------------------------------------------------

enum class Mode { Rapid, Muskingum, Unit };

// Where the (time, reach) rows in params order come from / go to.
struct Rows {
    const double *dev_in = nullptr;   // device array, rows_in rows
    const float *dev_in32 = nullptr;  // instead of dev_in: float32 lateral rows (RapidMuskingum; exact in float64)
    const double *host_in = nullptr;  // host array, T rows
    int64_t rows_in = 0;
    double *dev_out = nullptr;
    double *host_out = nullptr;
    int64_t rows_out = 0;
    float *dev_out32 = nullptr;       // instead of dev_out: float32 rows, each the mean of out_factor routed rows
    int64_t out_factor = 1;
    // UnitMuskingum with the convolution fused into the in-pass: dev_in holds runoff DEPTH rows, the lateral inflow is
    // computed on the way into the records (k_rec_in_uh)
    const double *uh_kernel = nullptr, *uh_state = nullptr;
    int64_t uh_nks = 0;
    // RapidMuskingum fed by gridded runoff: no lateral rows at all, the weights product runs in the in-pass (k_rec_in_runoff)
    const RunoffArgs *runoff = nullptr;
    // an ensemble call (rr_rapid_route_ensemble_dev): `members` sets of rows, member m's at m * in_pitch / m * out_pitch elements from
    // the first member's (0: a single-member call)
    int64_t members = 0, in_pitch = 0, out_pitch = 0;
    // a parameter ensemble (rr_rapid_route_members_dev): member m is routed with the plan's m-th coefficient set (rr_plan::d_mcoef, d_mc4);
    // in_pitch may be 0 there: one forcing shared by all members
    bool member_coeffs = false;
};

// What a route call hands over, as far as the choice of its kernel is concerned.  Built in two places only -- call_shape (from the
// call's Rows) and rr_plan_reserve (from its RR_ROWS_* bits) -- so that a reservation and the call it is made for get the same schedule.
struct CallShape {
    Mode mode = Mode::Rapid;
    int64_t T = 0, nsub = 1;
    bool host = false;           // rows in host arrays (the host-pointer entry points)
    bool dev_rows = false;       // device rows the direct row path reads as they are: lateral inflow (float64 or float32; none in channel-only routing), or depths (uh)
    bool in32 = false;           // float32 lateral rows or depths
    bool out32 = false;          // float32 output rows, each the mean of `factor` routed rows
    int64_t factor = 1;
    bool uh = false;             // UnitMuskingum with the unit-hydrograph convolution fused in: the rows are runoff depths
    bool runoff = false;         // gridded runoff: no lateral rows, the in-pass makes them
    int64_t ring_in = 0, ring_out = 0;      // streaming calls (rr_stream_begin*): rows of the caller's cyclic lateral / discharge arrays
    int64_t members = 0;         // ensemble calls: members routed together on the time-tiled kernel, one record ring each (0: a single-member call)
    bool member_coeffs = false;  // a parameter ensemble: the members' own coefficient sets (one weight per reach each: rr_plan_set_member_coeffs), not the plan's
};

// streaming k_tick over rows, time-tiled k_tile over records, the direct row path (rr_plan_last_kernel, rr_plan_reserve's info[0])
enum class Kernel { Tick = RR_KERNEL_TICK, Tile = RR_KERNEL_TILE, Direct = RR_KERNEL_DIRECT };

// The schedule of a call (choose_schedule): its kernel, task length(s) and work memory.
struct Schedule {
    Kernel kernel = Kernel::Tick;
    int64_t KC = 1;                   // record chunks per task (Tile); rows per task / 16 (Direct)
    int64_t KS = 1;                   // Direct: record chunks per task of the skeleton's launches
    int64_t chunks = 0;               // chunks of the record ring (Tile), of the skeleton's record ring (Direct)
    int64_t ring = 0;                 // doubles of P->d_ring: record ring (an ensemble's: one per member), or the work rows of the streaming kernel
    int64_t mrows = 0, stage = 0;     // doubles of the intermediate rows (streaming permutation, convolved rows) / of the host staging rows
    int64_t rec_nb = 1;               // Tile: record batches per launch of k_rec_in / k_rec_out (the ring holds rec_nb - 1 more)
};

// One routing call in flight: rows enter (permutation in), ticks run, finished rows leave (permutation out).
// route_core() runs a session start to finish; the rr_stream_* entry points keep it open between calls so the
// lag pipeline is never drained while forcing or boundary series arrive in chunks (multi-GPU).
struct Session {
    bool open = false;
    Mode mode = Mode::Rapid;
    int64_t T = 0, nsub = 1, total = 0, total_ticks = 0;
    Rows io;
    hipStream_t stream = nullptr;
    Kernel kernel = Kernel::Tick;
    bool in_place = false;        // Tick: engine order == params order, device rows: the streaming kernel works in the caller's arrays
    bool has_in = true;
    int64_t ring_rows = 0;
    int64_t rows_loaded = 0, rows_stored = 0, tau = 0;
    const double *ghost_series = nullptr;
    double *export_series = nullptr;
    TickArgs a{};
    int64_t KC = 1;               // record chunks per task: K = 16 * KC ticks
    int64_t rec_chunks = 0, in_batches = 0, n_in_batches = 0, out_batches = 0, n_out_batches = 0;
    int64_t rec_nb = 1;           // record batches per launch of the plain record passes (Schedule::rec_nb)
    int64_t ticks_stored = 0;     // tick-rows that have left the record ring
    int64_t out_limit = std::numeric_limits<int64_t>::max();   // rows the caller's output ring can take (host pipeline)
    int64_t diag = 0, n_diags = 0, n_macro = 0;
    int64_t ghost_batches = 0;    // batches of the boundary (ghost) series turned into records
    int64_t ghost_slack = 0, export_skew = 0;      // boundary reaches of a partitioned network in the time-tiled schedule (level skew included)
    TileArgs ta{};
    // direct row path (rr_kernels_direct.hpp): K rows per task, the skeleton behind it on records
    int64_t n_tasks = 0;          // direct launches: rows [d K, (d + 1) K) in launch d
    int64_t d_done = 0;           // direct launches made
    int64_t KS = 1;               // record chunks per task of the skeleton's launches (KS divides KC; shorter where the part feeds another GPU)
    bool export_lanes = false, export_skel = false;    // a boundary export is routed by a lane of a direct tile (final as soon as its rows are routed) / by the skeleton
    DirectArgs da{};
    bool bracket_open = false;
    int64_t bracket_reaches = 0;
    size_t max_samples = 0;
    int64_t members = 0;          // an ensemble call (Rows::members): member m's record ring at m * ring_stride doubles
    int64_t ring_stride = 0;
    bool hw = false;              // Tile: the plan's in-pass headwaters are not k_tile's to store in this call (rr_plan::hw_inpass); RapidMuskingum: k_rec_in routes them
};

// ---- host-pointer calls: PCIe pipeline around the time-tiled kernel ----
//
// The reference's kernel boundary hands over numpy arrays in pageable host memory.  hipMemcpy from pageable memory moves
// 22 GB/s here, and one direction at a time; registering the caller's arrays costs 43 ms per GB; pinned memory moves
// 49 GB/s each way at once (profiles/microbench/host_copy.hip).  So rows travel in chunks of 64 through three pinned
// buffers per direction, filled and emptied by eight copy threads each, while the DMA engines move the neighbouring
// chunks and the GPU routes what has arrived: caller -> pinned -> device staging ring -> records -> tiles -> records ->
// device staging ring -> pinned -> caller, every stage overlapping the others.  The open routing call is the streaming
// session the partitioned path uses (rows become ready chunk by chunk).
struct HostPipe {
    static constexpr int kPinned = 3, kCopyThreads = 8;
    int copy_threads = kCopyThreads;      // per direction: PCIe carries 26 GB/s each way whatever the count (profiles/r03_host_path_threads.txt)
    int64_t chunk_mib = 512;              // staging chunk: long enough for the DMA engines to reach their rate, short enough to pipeline
    int64_t chunk_rows = 64, ring_chunks = 8;
    double *pin_in[kPinned] = {nullptr, nullptr, nullptr}, *pin_out[kPinned] = {nullptr, nullptr, nullptr};
    DevBuf<double> dev_in, dev_out;       // the device rings (count(): doubles per ring)
    int64_t pin_cap = 0;                  // doubles per pinned buffer
    hipStream_t s_h2d = nullptr, s_d2h = nullptr;
    std::vector<hipEvent_t> ev_h2d, ev_d2h, ev_adv;
    void destroy()
    {
        for (int k = 0; k < kPinned; ++k) { if (pin_in[k]) (void)hipHostFree(pin_in[k]); if (pin_out[k]) (void)hipHostFree(pin_out[k]); pin_in[k] = pin_out[k] = nullptr; }
        dev_in.reset(); dev_out.reset(); pin_cap = 0;
        for (auto *v : {&ev_h2d, &ev_d2h, &ev_adv}) { for (hipEvent_t e : *v) (void)hipEventDestroy(e); v->clear(); }
        if (s_h2d) (void)hipStreamDestroy(s_h2d);
        if (s_d2h) (void)hipStreamDestroy(s_d2h);
        s_h2d = s_d2h = nullptr;
    }
};

// The device side of one rr::TilePlan, as k_tile's launches and the state kernels read it.  A plan has two: over its own tiles
// (rr_plan::ts) and over the skeleton of the direct row path (rr_plan::ks); tiles_of() picks the one a call's kernel runs on.
struct TileSet {
    const rr::TilePlan *tp;
    DevBuf<TileMeta> tmeta;       // per tile (rr_kernels_tile.hpp)
    DevBuf<int4> pmeta;           // per position {lag | flags, first upstream position, xpos, upstream counts}
    DevBuf<int32_t> perm;
    DevBuf<double> coef, sq, ss, si, sqch;      // per position: {c1row, c2, c3}; the carried state
    int32_t n_wide = 0;           // tiles with a reach of more than three upstream reaches: general kernel beside the LEAN one
};

struct rr_plan {
    rr::HostPlan h;
    int device = RR_DEVICE_NONE;
    bool coeffs_set = false, has_c4 = false;
    int64_t chunk_rows = 16, sample_every = 0;

    // streaming kernel (k_tick): lag-ordered layout of rr::HostPlan
    DevBuf<int32_t> d_child_ptr, d_lag, d_perm, d_inv, d_inner_pos;
    DevBuf<int32_t> d_bidx;   // ghost / export slot of flagged positions
    DevBuf<uint16_t> d_hwc;
    DevBuf<double> d_w, d_c1row_h, d_c2, d_c3, d_c4;
    DevBuf<double> d_x, d_isum, d_qch;
    DevBuf<double> d_a2, d_c1own, d_z;   // UnitMuskingum with general edge data (rr_plan_set_unit_weights): streaming kernel only
    bool unit_general = false;
    DevBuf<double> d_ring;
    DevBuf<double> d_stage;
    DevBuf<double> d_mrows;   // intermediate rows of the tiled permutation
    // tiled permutations: [0] params order -> engine order (pi = perm), [1] engine -> params (pi = inv)
    DevBuf<uint16_t> d_slot_a[2], d_slot_b[2];
    DevBuf<int32_t> d_m_index[2];
    int64_t perm_rows_per_block = 2;

    // time-tiled routing (k_tile): subtree tiles of rr::TilePlan
    rr::TilePlan tp;
    bool wave_enabled = true, wave_forced = false, weights_uniform = false;
    bool ens_enabled = true;     // the member-batched k_tile forms got their LDS (rr_plan_create)
    int wave_threads = 512;
    int64_t wave_K = 0;          // ticks per task (multiple of 16); 0 = chosen per call
    Schedule sch;                // prepare_call: the schedule of the call about to start (or running, or just ended)
    int64_t kc_cap = int64_t{1} << 20;      // longest task (record chunks) the device had room for; 0: no record ring fits, the plan streams
    int64_t nb_cap = kRecMaxLaunchBatches;  // most record batches per launch the device had room for (the ring holds one batch more for each beyond the first)
    TileSet ts{&tp};              // the tiles' device side: tmeta, pmeta, perm, coef {c1row, c2, c3}, the carried state
    DevBuf<int32_t> d_tinv;
    DevBuf<int32_t> d_inner_idx;
    bool export_inside = false;      // an export reach that another tile mirrors (it has a downstream reach in this plan): streaming kernel only
    DevBuf<double> d_coef_unit;   // ts.coef with zeros at the positions without upstream positions (UnitMuskingum's short tick)
    // Headwaters routed by the in-pass (rr_plan.hpp: mark_inpass_headwaters; RR_HW_INPASS=0: off).  The short tick of a call with one
    // sub-step per row, single member, reads d_pmeta_hw instead of ts.pmeta -- the eligible positions carry a ghost's flag there: published,
    // never stored -- and RapidMuskingum d_coef_hw instead of ts.coef: zeros at those positions, whose records k_rec_in has already routed.
    bool hw_inpass = true;
    std::vector<uint8_t> hw_elig;    // [np] eligible positions, with the plan's boundary reaches
    int64_t hw_counts[4] = {0, 0, 0, 0};
    std::vector<int32_t> meta_lag, meta_xpos, meta_flags;      // what upload_tile_meta last got (the boundary reaches' flags among them)
    DevBuf<int4> d_pmeta_hw;
    DevBuf<double> d_coef_hw;
    DevBuf<double> d_hwcoef;      // [3 n] {c1row, c2, c3} per params column, for k_rec_in
    DevBuf<double> d_hwq;         // [n] k_rec_in's carry: a column's discharge after the last batch turned into records; launch_state_in: the call's initial state
    std::vector<double> h_coef;      // ts.coef on the host: rr::tile_coef of the plan's set for its boundary ghosts, filled by lay_tile_coef alone
    DevBuf<double> d_esq, d_ess, d_esi;      // the carried state of an ensemble's members, np apart
    int64_t ens_cap = 0;             // members they have room for (rr_plan_reserve_ensemble)
    // Parameter ensembles (rr_plan_set_member_coeffs): member m's {c1row, c2, c3} per position in tile order, zeros at ghosts -- what ts.coef
    // would hold after rr_plan_set_coeffs with that member's arrays -- 3 np doubles apart, and its c4dt in params order, n apart.  Beside
    // the plan's own coefficient set, never instead of it.
    DevBuf<double> d_mcoef, d_mc4;
    int64_t mc_sets = 0;             // coefficient sets they hold
    DevBuf<double> d_full, d_chan;   // UnitMuskingum state scattered to params order
    DevBuf<int2> d_colmeta;   // per params column {position, lag}
    DevBuf<int2> d_ghostmeta; // the same per boundary ghost (column of the ghost series)
    DevBuf<double> d_c4_params;   // c4dt in params order (scale of the record permutation)
    size_t dev_total_bytes = 0;
    int cu_count = 256;

    // boundary reaches of a partitioned network
    int64_t n_ghost = 0, n_export = 0;
    bool boundary_whole = true;      // false from a failed rr_plan_set_boundary (counts and tables may disagree) to the next that succeeds: no route call until then
    int64_t ghost_min_lag = 0, export_max_lag = 0;
    std::vector<int32_t> ghost_reach, export_reach;   // params indices, in the caller's order

    Session ses;
    HostPipe pipe;      // staging of the host-pointer entry points (allocated at first use)
    // direct row path: column-range tiles where the params order numbers small subtrees contiguously (rr_plan.hpp: DirectPlan)
    rr::DirectPlan dp;
    bool direct_enabled = true;          // RR_DIRECT=0 (tests): records for every call
    bool uh_rows_ok = true;      // false once the device refused the convolved rows of rr_unit_route_uh*_dev on the direct row path: records from then on
    int direct_window = 1;               // rows of the LDS window: largest span + 1 of the plan's tiles
    DevBuf<DirectTile> d_dtiles;
    DevBuf<int4> d_dlane;
    DevBuf<int32_t> d_dsend_ptr, d_dsend_lane;
    DevBuf<double> d_dcoef, d_dq;
    TileSet ks{&dp.skel};             // the skeleton's tiles (TileArgs of its k_tile launches)
    DevBuf<int32_t> d_kholecol;
    DevBuf<int2> d_kholemeta;         // per hole {position in the skeleton, lag}: the out-pass that patches the holes
    DevBuf<int2> d_kghostmeta;        // per boundary ghost {position of the skeleton's ghost that mirrors it, lag}: the in-pass of the ghost series
    std::vector<double> h_reach_coef;    // the plan's coefficient set: {c1row, c2, c3, c4dt} per reach (rr::reach_coef): d_dcoef, and what rr_plan_set_boundary lays the tile tables out from again
    int32_t direct_block = 0;            // tile capacity the plan was built with (rr_plan_set_boundary lays the direct plan out again)
    int64_t n_kholes = 0;
    bool in32_big_endian = false, out32_big_endian = false;      // rr_plan_set_row_format: float32 rows as a big-endian file stores them
    bool lean_enabled = true;           // RR_TILE_LEAN=0 (tests): the general tick for every call
    bool uh_pairs = true;               // the fused convolution takes two record batches per launch where it can (RR_UH_PAIRS=0: tests)
    int32_t rec_batches = kRecLaunchBatches;   // record batches per launch of k_rec_in / k_rec_out in long calls (RR_REC_BATCHES: tests, A/B)
    bool rec_batches_forced = false;    // RR_REC_BATCHES was given: rec_batches in every call the time-tiled kernel takes
    bool perm_ready = false;            // the streaming kernel's tiled permutations are on the device
    DevBuf<int32_t> d_adj_down;      // adjoint (rr_rapid_adjoint_dev): downstream engine position of each position, -1 at outlets

    // profile of the last route call: the routing kernel (ev, rr_plan_profile) and, sampled the same way, the kernels around it
    // (aux: 0 in-pass, 1 out-pass, 2 the skeleton's k_tile launches of the direct row path, 3 its out-pass over the holes)
    static constexpr int kAuxKinds = 4, kAuxSamples = 256;
    std::vector<hipEvent_t> aux_ev;      // 2 per sample, made by rr_plan_reserve
    std::vector<int> aux_kind;
    int64_t aux_launches[kAuxKinds] = {0, 0, 0, 0};
    std::vector<hipEvent_t> ev;
    std::vector<int64_t> ev_reaches;
    hipEvent_t ev_first = nullptr, ev_last = nullptr;
    int64_t prof_launches = 0, prof_samples = 0, prof_brackets = 0, prof_reach_steps = 0;
    hipStream_t last_stream = nullptr;
};

// The engine's device memory: every allocation and release goes through these two (rr_devbuf.hpp declares them; DevBuf and
// rr_dev_malloc / rr_dev_free are their callers).  They count, for the whole process, the allocations alive and the allocations
// made (rr_dev_alloc_stats), and -- a test switch, RR_ALLOC_FAIL_AT=k read by rr_plan_create -- refuse the k-th one from then on, once.
namespace rr {
std::atomic<int64_t> g_dev_live{0}, g_dev_made{0}, g_dev_fail_in{0};      // g_dev_fail_in: allocations until the injected refusal (0: none)
thread_local std::string g_dev_refusal;      // the runtime's words for the last refused allocation (rr_dev_malloc has a message of its own around them)

int dev_mem_alloc(void **p, size_t bytes)
{
    *p = nullptr;
    const bool injected = g_dev_fail_in > 0 && --g_dev_fail_in == 0;
    const hipError_t e = injected ? hipErrorOutOfMemory : hipMalloc(p, bytes);
    if (e != hipSuccess) {
        *p = nullptr;
        g_dev_refusal = std::string(hipGetErrorString(e)) + (injected ? " (injected)" : "");
        return fail(RR_E_ALLOC, "hipMalloc of " + std::to_string(bytes) + " bytes failed: " + g_dev_refusal);
    }
    ++g_dev_live; ++g_dev_made;
    return RR_OK;
}

void dev_mem_free(void *p)
{
    if (p && hipFree(p) == hipSuccess) --g_dev_live;      // (a block the runtime would not free stays counted; rr_dev_free reports it)
}
}  // namespace rr

namespace {

template <typename T>
int dev_upload(T *dst, const T *src, size_t count)
{
    if (count == 0) return RR_OK;
    HIPCHK(hipMemcpy(dst, src, count * sizeof(T), hipMemcpyHostToDevice));
    return RR_OK;
}

template <typename T>
int dev_upload(T *dst, const std::vector<T> &src) { return dev_upload(dst, src.data(), src.size()); }

template <typename T>
int dev_upload(const DevBuf<T> &dst, const std::vector<T> &src) { return dev_upload(dst.get(), src); }

template <typename... B>
void reset_all(B &...buf) { (buf.reset(), ...); }

// Room for `src` (kept where the buffer already has it), then the upload.
template <typename T>
int assign(DevBuf<T> &buf, const std::vector<T> &src)
{
    if (int rc = buf.reserve(std::max<int64_t>(1, (int64_t)src.size()))) return rc;
    return dev_upload(buf, src);
}

int need_device(const rr_plan *plan)
{
    if (!plan) return fail(RR_E_INVALID, "null plan");
    if (plan->device < 0)
        return fail(RR_E_NO_DEVICE, "this plan is host-only (RR_DEVICE_NONE): the HIP engine has no CPU fallback");
    HIPCHK(hipSetDevice(plan->device));
    return RR_OK;
}

// Tile and position constants of a tile plan as k_tile reads them (TileArgs::tiles, ::pos), packed from the plan and the lag words, xpos
// words and tile flags to go with it (the boundary reaches of a partitioned network change all three).  Returns the number of wide tiles.
int32_t pack_tile_meta(const rr::TilePlan &TP, const std::vector<int32_t> &lag, const std::vector<int32_t> &xpos, const std::vector<int32_t> &flags, std::vector<TileMeta> &tm, std::vector<int4> &pm)
{
    tm.resize((size_t)TP.n_tiles); pm.resize((size_t)TP.np);
    for (int32_t t = 0; t < TP.n_tiles; ++t)
        tm[t] = TileMeta{TP.tile_ptr[t], TP.tile_ptr[t + 1], TP.tile_level[t], TP.tile_lag_lo[t], TP.tile_lag_hi[t], flags[t], 0, 0};
    for (int64_t p = 0; p < TP.np; ++p) pm[p] = make_int4(lag[p], TP.cfirst[p], xpos[p], (int32_t)TP.ccnt[p]);
    return (int32_t)std::count_if(flags.begin(), flags.end(), [](int32_t f) { return (f & kTileWide) != 0; });
}

// The plan's own tiles on the device (rr_plan_create; rr_plan_set_boundary and rr_plan_set_coeffs again), with the tables of the in-pass headwaters.
int upload_tile_meta(rr_plan *P, const std::vector<int32_t> &lag, const std::vector<int32_t> &xpos, const std::vector<int32_t> &flags)
{
    const rr::TilePlan &TP = P->tp;
    std::vector<TileMeta> tm; std::vector<int4> pm;
    P->ts.n_wide = pack_tile_meta(TP, lag, xpos, flags, tm, pm);
    int rc = P->ts.tmeta.reserve(std::max<int64_t>(1, TP.n_tiles));
    if (!rc) rc = P->ts.pmeta.reserve(std::max<int64_t>(1, TP.np));
    if (!rc) rc = dev_upload(P->ts.tmeta, tm);
    if (!rc) rc = dev_upload(P->ts.pmeta, pm);
    // the in-pass headwaters: a ghost's flag in the short tick's own position table, a flag in the column metadata for k_rec_in
    // (with the plan's coefficients once it has them: rr_plan_set_coeffs comes here again, mark_inpass_headwaters looks at c1row and c2)
    rr::mark_inpass_headwaters(TP, lag, kGhostBit, P->hw_elig, P->hw_counts, P->h_coef.empty() ? nullptr : P->h_coef.data());
    if (&lag != &P->meta_lag) { P->meta_lag = lag; P->meta_xpos = xpos; P->meta_flags = flags; }
    if (!P->hw_inpass) { P->hw_elig.assign((size_t)TP.np, 0); P->hw_counts[0] = 0; }
    for (int64_t p = 0; p < TP.np; ++p) if (P->hw_elig[p]) pm[p].x |= kTileGhostBit;
    const rr::HostPlan &H = P->h;
    std::vector<int2> cm((size_t)H.n);
    for (int64_t i = 0; i < H.n; ++i)      // a headwater column is flagged: UnitMuskingum's out-pass leaves it unclamped
        cm[i] = make_int2(TP.inv[i], (TP.lag[TP.inv[i]] & kLagMask) | (H.child_ptr[H.inv[i] + 1] == H.child_ptr[H.inv[i]] ? kColHeadwater : 0) |
                                         (P->hw_elig[TP.inv[i]] ? kColInpass : 0));
    if (!rc) rc = assign(P->d_pmeta_hw, pm);
    if (!rc) rc = assign(P->d_colmeta, cm);
    return rc;
}

// The plan's coefficient set in tile order, on the host: which headwaters the in-pass routes depends on it (upload_tile_meta), so it is
// laid out before the position tables go up -- by rr_plan_set_coeffs, and by rr_plan_set_boundary for the new boundary ghosts.
void lay_tile_coef(rr_plan *P, const rr::ReachCoef &reach)
{
    P->h_coef.resize(3 * (size_t)P->tp.np);
    rr::tile_coef(P->tp, reach, kTileGhostBit, P->ghost_reach, P->h_coef.data());
}

// The tile-order tables on the device: ts.coef and its masked forms (rr_plan.hpp: tile_coef).
int upload_tile_coef(rr_plan *P)
{
    if (P->h_coef.empty()) return RR_OK;
    std::vector<double> masked(P->h_coef), col(3 * (size_t)P->h.n);
    int rc = dev_upload(P->ts.coef, P->h_coef);
    rr::zero_tile_coef(masked.data(), P->hw_elig);      // RapidMuskingum's short tick where the in-pass routes headwaters
    if (!rc) rc = dev_upload(P->d_coef_hw, masked);
    rr::column_coef(P->tp, P->h_coef.data(), P->h.n, col.data());      // (a boundary ghost's zeros: its column is not routed by the in-pass)
    if (!rc) rc = dev_upload(P->d_hwcoef, col);
    // UnitMuskingum's short tick (_numba_kernels.py:122-123), on the same copy: an in-pass headwater has no upstream position either
    rr::zero_tile_coef_headwaters(P->tp, masked.data());
    return rc ? rc : dev_upload(P->d_coef_unit, masked);
}

// ---- kernel pickers: the instantiation a call gets, one function per kernel family.  They name every form the engine has and no other. ----

typedef void (*direct_kernel_t)(const DirectArgs);
struct DirectForm { bool in32, out32, sub, unit; direct_kernel_t kernel; };
#define RR_DF(I_, O_, S_, U_) DirectForm{I_, O_, S_, U_ != 0, k_direct<kDirectAhead, I_, O_, S_, U_>}
const DirectForm kDirectForms[] = {      // k_direct's twelve forms (upload_direct_plan walks them): UnitMuskingum reads float64 rows only
    RR_DF(false, true, true, 1), RR_DF(false, false, true, 1), RR_DF(false, true, false, 1), RR_DF(false, false, false, 1), RR_DF(true, true, true, 0),   RR_DF(true, true, false, 0),
    RR_DF(true, false, true, 0), RR_DF(true, false, false, 0), RR_DF(false, true, true, 0),  RR_DF(false, true, false, 0),  RR_DF(false, false, true, 0), RR_DF(false, false, false, 0)};
#undef RR_DF
direct_kernel_t direct_kernel(bool in32, bool out32, bool sub, bool unit)
{
    for (const DirectForm &f : kDirectForms) if (f.in32 == (in32 && !unit) && f.out32 == out32 && f.sub == sub && f.unit == unit) return f.kernel;
    return nullptr;      // (every combination is in the table)
}

// The direct row path's device arrays (rr::DirectPlan): per-column constants, the skeleton's tile arrays, the columns of the holes' out-pass.
// Called by rr_plan_create and again by rr_plan_set_boundary, which lays the plan out anew around the boundary reaches.
int upload_direct_plan(rr_plan *P)
{
    reset_all(P->d_dtiles, P->d_dlane, P->d_dsend_ptr, P->d_dsend_lane, P->d_dcoef, P->d_dq, P->ks.tmeta, P->ks.pmeta, P->ks.perm, P->d_kholecol, P->ks.coef,
              P->ks.sq, P->ks.ss, P->ks.si, P->ks.sqch, P->d_kholemeta, P->d_kghostmeta);      // the old layout goes before the new one is allocated (one left out here would only go later, at its alloc)
    P->n_kholes = 0; P->ks.n_wide = 0;
    P->direct_window = 3;
    for (int32_t sp : P->dp.tile_span) P->direct_window = std::max(P->direct_window, sp + 3);
    if (!P->dp.ok || P->device < 0) return RR_OK;
    const rr::HostPlan &H = P->h;
    const rr::DirectPlan &D = P->dp;
    const rr::TilePlan &K = D.skel;
    const int64_t n = H.n;
    for (const DirectForm &f : kDirectForms)      // > 64 KiB of dynamic LDS needs an explicit opt-in per kernel
        if (hipFuncSetAttribute((const void *)f.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)direct_lds_bytes(kDirectMaxWindow)) != hipSuccess) {
            (void)hipGetLastError();
            P->direct_enabled = false;
        }
    std::vector<DirectTile> dt((size_t)D.n_tiles);
    for (int32_t t = 0; t < D.n_tiles; ++t) dt[t] = DirectTile{D.tile_c0[t], D.tile_nc[t], D.tile_lag_lo[t], D.tile_span[t]};
    std::vector<int4> dl((size_t)n);
    for (int64_t i = 0; i < n; ++i) dl[i] = make_int4(D.delay[i], D.up3[i], D.xinfo[i], H.lag[H.inv[i]]);
    int rc = assign(P->d_dtiles, dt);
    if (!rc) rc = assign(P->d_dlane, dl);
    if (!rc) rc = assign(P->d_dsend_ptr, D.send_ptr);
    if (!rc) rc = assign(P->d_dsend_lane, D.send_lane);
    if (!rc) rc = P->d_dcoef.alloc(4 * n);
    if (!rc) rc = P->d_dq.alloc(n);
    std::vector<int32_t> klag(K.lag), kxpos(K.xpos), kflags(K.tile_flags);
    // boundary exports among the skeleton's reaches: flagged as in the plan's own tiles (rr_plan_set_boundary); the slot in the export
    // series travels in xpos[] (an export is an outlet of its part: no ghost of another tile mirrors it -- checked by build_direct_plan)
    for (size_t e = 0; e < P->export_reach.size(); ++e) {
        const int32_t i = P->export_reach[e];
        if (!D.big[i]) continue;
        const int32_t p = K.inv[i];
        klag[p] |= kExportBit; kxpos[p] = (int32_t)e; kflags[K.tile_of[p]] |= kTileExports;
    }
    std::vector<TileMeta> tm; std::vector<int4> pm;
    P->ks.n_wide = pack_tile_meta(K, klag, kxpos, kflags, tm, pm);
    std::vector<int2> hm, gm;
    std::vector<int32_t> hc;
    for (int64_t i = 0; i < n; ++i)
        if (D.big[i]) { hm.push_back(make_int2(K.inv[i], K.lag[K.inv[i]] & kLagMask)); hc.push_back((int32_t)i); }
    for (int32_t i : P->ghost_reach) { const int32_t g = K.ext_ghost[i]; gm.push_back(make_int2(g, K.lag[g] & kLagMask)); }
    P->n_kholes = (int64_t)hm.size();
    if (!rc) rc = assign(P->ks.tmeta, tm);
    if (!rc) rc = assign(P->ks.pmeta, pm);
    if (!rc) rc = assign(P->ks.perm, K.perm);
    if (!rc) rc = P->ks.coef.alloc(3 * K.np);
    for (DevBuf<double> *state : {&P->ks.sq, &P->ks.ss, &P->ks.si, &P->ks.sqch}) if (!rc) rc = state->alloc(K.np);
    if (!rc) rc = assign(P->d_kholemeta, hm);
    if (!rc) rc = assign(P->d_kholecol, hc);
    if (!rc) rc = assign(P->d_kghostmeta, gm);
    return rc;
}

// Coefficients of the direct row path: the per-reach table for the lanes, the skeleton's tile-order table for its k_tile launches.
int upload_direct_coef(rr_plan *P)
{
    if (!P->dp.ok || P->device < 0 || P->h_reach_coef.empty()) return RR_OK;
    int rc = dev_upload(P->d_dcoef, P->h_reach_coef);
    std::vector<double> kc(3 * (size_t)P->dp.skel.np);
    rr::tile_coef(P->dp.skel, rr::table_rows(P->h_reach_coef.data()), kTileGhostBit, {}, kc.data());
    return rc ? rc : dev_upload(P->ks.coef, kc);
}

// The two-phase tiled permutation params order <-> lag order of the streaming kernel (k_perm_a / k_perm_b).  Built when a
// call first streams: the time-tiled kernel, which takes almost every call, has its own record passes.
int upload_tiled_permutations(rr_plan *P)
{
    const rr::HostPlan &H = P->h;
    const int64_t n = H.n;
    const int32_t *pis[2] = {H.perm.data(), H.inv.data()};
    int rc = RR_OK;
    for (int w = 0; w < 2 && !rc; ++w) {
        rr::TiledPermutation tp;
        rr::build_tiled_permutation(pis[w], n, kPermE * kPermThreads, tp);
        rc = assign(P->d_slot_a[w], tp.slot_a);
        if (!rc) rc = assign(P->d_slot_b[w], tp.slot_b);
        if (!rc) rc = assign(P->d_m_index[w], tp.m_index);
    }
    if (rc) {      // all or nothing: a later call must not find half of the tables
        for (int w = 0; w < 2; ++w) reset_all(P->d_slot_a[w], P->d_slot_b[w], P->d_m_index[w]);
        return rc;
    }
    P->perm_ready = true;
    return RR_OK;
}

// Every fourth launch of a kind is bracketed by HIP events while the plan samples (rr_plan_set_options): aux_begin returns the
// sample's number or -1.
int aux_begin(rr_plan *P, int kind, hipStream_t stream)
{
    const int64_t seq = P->aux_launches[kind]++;
    if (P->sample_every < kSampleGroup || (seq & 3) != 0 || 2 * (P->aux_kind.size() + 1) > P->aux_ev.size()) return -1;
    if (hipEventRecord(P->aux_ev[2 * P->aux_kind.size()], stream) != hipSuccess) return -1;
    P->aux_kind.push_back(kind);
    return (int)P->aux_kind.size() - 1;
}
void aux_end(rr_plan *P, int sample, hipStream_t stream)
{
    if (sample >= 0) (void)hipEventRecord(P->aux_ev[2 * sample + 1], stream);
}

// ---- session -------------------------------------------------------------------------------------

// Record chunks per task.  A longer task amortises the load of the tile's state and of its first half chunk, which
// nothing overlaps; every tile level adds one task of skew to the pipeline and to the record ring.  Tasks of 128 and 256
// ticks are for long calls on networks whose ring then stays under a fifth of the card (choose_schedule): they are worth
// 11 % at 100k reaches, 7 % at 250k, 3 % at 500k (profiles/microbench/k_sweep_small.sh) and 2-3 % at 1M, where 128 ticks
// make the ring 50 GB (366.5 / 367.3 ms per year against 374.3 / 382.3 at 64 ticks, profiles/r03_k_sweep.txt).
int64_t pick_KC(const rr_plan *P, int64_t total_ticks)
{
    if (P->wave_K > 0) return std::max<int64_t>(1, std::min<int64_t>(P->wave_K, 256) / kRec);      // (RR_WAVE_K above 256 -- the longest task the schedule itself picks here -- is for the direct row path's lane tasks: the in-pass runs at most four batches of 128 tick-rows ahead of the out-pass)
    return total_ticks >= 32768 ? 16 : (total_ticks >= 16384 ? 8 : (total_ticks >= 4096 ? 4 : (total_ticks >= 512 ? 2 : 1)));
}

// Rows per task of the direct path: a task costs its tile `span` ticks of fill and drain (lanes start one after the other: 10 % at
// 512 rows, 5 % at 1,024).  The skeleton's tasks are cut separately (Schedule::KS, direct_KS below): every tile level of the skeleton costs
// one of ITS tasks of pipeline and of record ring, so long lane tasks over short skeleton tasks have both -- the year at 1M reaches
// 196.5 ms with 512 / 512, 186.4 with 1,024 / 512, 185.1 with 2,048 / 512; a 3,504-row call 24.4 ms with 256 / 256, 21.6 with 512 / 128; a
// 744-row call 7.4 ms with 128 / 128, 6.6 with 256 / 128 (profiles/r05_direct_ks_ab.txt; with the skeleton's tasks as long as the lanes',
// 1,024 rows lost to 512: 213 against 207 ms, profiles/r04_direct_k_and_fill.txt).
int64_t pick_direct_K(const rr_plan *P, int64_t T)
{
    if (P->wave_K > 0) return P->wave_K;
    return T >= 16384 ? 1024 : (T >= 2048 ? 512 : (T >= 512 ? 256 : (T >= 128 ? 128 : 64)));
}
int64_t direct_KS(int64_t task_chunks, int64_t total_ticks)      // record chunks per skeleton task: 512 ticks in long calls, 128 in short ones; divides the lanes' task
{
    int64_t ks = std::max<int64_t>(1, std::min<int64_t>(task_chunks, (total_ticks >= 16384 ? 512 : 128) / kRec));
    while (ks > 1 && task_chunks % ks) --ks;
    return ks;
}

// The shape of a route call (stream: rr_stream_begin*, whose rows arrive over rr_stream_advance in the caller's rings).  The direct row
// path reads device rows as they are, but not gridded runoff, and not a UnitMuskingum stream (rr_stream_begin_unit keeps to records, and
// engine.Plan.stream_begin_unit reserves for them).
CallShape call_shape(Mode mode, int64_t T, int64_t nsub, const Rows &io, bool stream = false)
{
    CallShape s;
    s.mode = mode; s.T = T; s.nsub = nsub;
    s.host = io.host_in != nullptr || io.host_out != nullptr;
    s.dev_rows = !s.host && !io.runoff && !(stream && mode == Mode::Unit);
    s.in32 = io.dev_in32 != nullptr;
    s.out32 = io.dev_out32 != nullptr; s.factor = io.out_factor;
    s.uh = io.uh_kernel != nullptr;
    s.runoff = io.runoff != nullptr;
    s.members = io.members; s.member_coeffs = io.member_coeffs;
    if (stream) { s.ring_in = mode == Mode::Muskingum ? 0 : io.rows_in; s.ring_out = io.rows_out; }
    return s;
}

// Which routing kernel a call uses.  The time-tiled schedule needs one upstream weight per reach, a network that tiles
// (rr::TilePlan) and room for its record ring; its fill and drain cost (levels x K) ticks more than the streaming kernel's, a
// few launches, so only calls of a handful of sub-steps stream.  RR_WAVE=1 forces it where it applies, RR_WAVE=0 forbids it.
//
// Records are indexed by tick = tick-row + lag, modulo the ring, per position: a position's slots never hold another
// position's data, so what the ring must cover is one position's tick-rows in flight.  Rows enter for all columns at once
// (ahead of the level-0 tiles) and leave for all columns at once (after the last level has passed their tick + depth), so
// every position keeps depth + levels * K tick-rows plus the batching of the two permutation passes; that its window sits
// lag ticks later than a headwater's does not widen it.  The ring may take five eighths of the card; a deep network that
// does not fit gets shorter tasks, then the streaming kernel.
//
// The choice is a pure function of the plan, the call's shape, kc_cap and nb_cap (lowered only when the device refuses an
// allocation), so rr_plan_reserve and the call it prepares for agree on it.
//
// host (the host-pointer entry points): the rows reach the time-tiled kernel through the PCIe pipeline's device rings (reserve_core
// prepares it); where that kernel does not apply they are routed chunk by chunk by the streaming kernel through staging rows.
// ring_in / ring_out (streaming calls, rr_stream_begin): rows of the caller's cyclic lateral / discharge arrays where those are shorter
// than the call (0: they hold every row).  A caller may refill such a ring between two rr_stream_advance calls, so a direct task must
// not span more rows than the ring holds: K is capped (a ring of fewer than 32 rows keeps to records, which take rows in batches of 128
// tick-rows the caller announces one by one).
// out32 (float32 output fused in, rr_*_f32*_dev): the direct task is a multiple of 128 rows, so that every output row -- the mean of
// `factor` routed rows, factor divides 128 -- lies inside one task.
// uh (rr_unit_route_uh*_dev: runoff depths + unit-hydrograph kernel): on the direct row path the convolution runs first, as a pass of its own
// into T rows of work memory (mrows) that the lanes then read -- the reference's own two steps (UnitMuskingum.py:72-98) -- where those rows
// fit a third of the card; otherwise the call keeps to records with the convolution fused into the in-pass.
Schedule choose_schedule(const rr_plan *P, const CallShape &s)
{
    Schedule sch;
    const Mode mode = s.mode;
    const int64_t T = s.T, nsub = s.nsub, total = T * nsub, dmax = P->h.depth - 1, n = P->h.n;
    // The direct row path: RapidMuskingum, one sub-step per row, float64 rows in device arrays, one weight per reach -- the
    // headline's call -- on a params order that numbers small subtrees contiguously (boundary reaches of a partitioned network
    // included: rr_plan_set_boundary lays the direct plan out around them).
    // Sub-steps (up to kDirectMaxSub a row) and channel-only routing take it too; with sub-steps only without boundary ghosts.  UnitMuskingum: below.
    // UnitMuskingum (float64 rows of convolved lateral inflow, no boundary reaches) takes it as well.
    const bool unit_direct = mode == Mode::Unit && nsub <= kDirectMaxSub && P->n_ghost == 0 && P->n_export == 0 && !P->unit_general && P->tp.ok &&
                             (!s.uh || (P->uh_rows_ok && (P->dev_total_bytes == 0 || T * n * 8 <= (int64_t)(P->dev_total_bytes / 3))));
    if (s.members == 0 && s.dev_rows && P->direct_enabled && P->dp.ok && (mode != Mode::Unit || unit_direct) && nsub <= kDirectMaxSub && (nsub == 1 || P->n_ghost == 0) &&
        P->weights_uniform && P->wave_enabled && total >= 8 && n < (int64_t{1} << 29)) {
        int64_t K = pick_direct_K(P, T);
        const int64_t levels = P->dp.skel.n_levels, np = P->dp.skel.np;
        if (s.ring_in > 0 && s.ring_in < T) K = std::min(K, s.ring_in / kRec * kRec);
        if (s.ring_out > 0 && s.ring_out < T) K = std::min(K, s.ring_out / kRec * kRec);
        if (s.out32) K = std::max<int64_t>(kRecRows, K / kRecRows * kRecRows);
        if (K >= 2 * kRec) {      // (a shorter task -- a ring of fewer than 32 rows -- keeps to records)
            sch.kernel = Kernel::Direct; sch.KC = K / kRec;
            // The skeleton's own tasks are shorter than the lanes' (several of the skeleton's launches per direct launch; a direct task is K rows =
            // K nsub ticks): see pick_direct_K -- and 64 ticks in a part that feeds another GPU, whose boundary series every level delays by one
            // task (as kc_long below).  KS divides KC nsub.
            sch.KS = direct_KS(sch.KC * nsub, total);
            if (P->n_export > 0 && P->wave_K <= 0) for (sch.KS = std::min<int64_t>(sch.KC * nsub, 4); (sch.KC * nsub) % sch.KS; --sch.KS) {}
            if (np > 0) {      // a record lives from the launch that forwards its first row to the out-pass behind the skeleton's last level
                // a ring cut to the call's length: with boundary ghosts it has to hold their in-pass's batches whole -- k_rec_in writes nine records per position and
                // batch, zeros past the call's end, and in a ring shorter than that a batch wrapped onto its own first records (a 40- or 130-row call of a shallow part:
                // wrong boundary inflow; a 200-row call: the last batch waited for its own slots for ever -- both found by profiles/microbench/parts_fuzz.py)
                int64_t whole_call = (total + dmax) / kRec + 2;
                if (P->n_ghost > 0) whole_call = std::max<int64_t>(whole_call, kRecBatch * ((total + 14) / kRecRows + 1) + (dmax >> 4) + 2);
                sch.chunks = std::min<int64_t>((levels * sch.KS * kRec + 2 * K * nsub + 2 * dmax + kRecRows + 2 * kRec) / kRec + 2, whole_call);
                sch.ring = sch.chunks * kRec * np;
            }
            if (s.uh) sch.mrows = T * n;      // the convolved rows
            if (np < (int64_t{1} << 25) && (P->dev_total_bytes == 0 || sch.ring * 8 <= (int64_t)(P->dev_total_bytes / 2))) return sch;
            sch = Schedule();
        }
    }
    bool ok = P->wave_enabled && P->tp.ok && (P->weights_uniform || s.member_coeffs) && n > 0 && P->tp.np < (int64_t{1} << 25) &&
              !P->export_inside && P->kc_cap >= 1 && !(mode == Mode::Unit && P->unit_general);
    if (ok && !P->wave_forced) ok = total >= 32;
    if (ok) {
        const int64_t np = P->tp.np, levels = P->tp.n_levels, members = std::max<int64_t>(1, s.members);      // an ensemble: the card's budget holds every member's ring
        const int64_t all_chunks = kRecBatch * ((total + 14) / kRecRows + 2) + (dmax >> 4) + 2;
        const int64_t slack = 4;      // room for the in-pass to run ahead of the routing: four batches of 128 tick-rows
        // The plain record passes take nb batches per launch in long calls -- the call lengths of pick_KC's long tasks; a shorter call's
        // ring stays as it was -- and the out-pass holds finished batches back until it has nb of them: nb - 1 more batches of ring.  The
        // largest nb whose ring fits the bounds below at the longest task that fits (RR_REC_BATCHES: that many in every call).
        const int64_t nb_max = P->rec_batches_forced || total >= 16384 ? std::max<int64_t>(1, std::min<int64_t>(P->rec_batches, P->nb_cap)) : 1;
        ok = false;
        // a part of a cut network that feeds another GPU keeps to 64 ticks: every tile level delays its boundary series by one
        // task, and the GPU downstream waits for it (10M reaches on 8 GPUs: whole job 7.2 against 7.1 x 10^11 reach-steps/s in the
        // time-weighted simulation, profiles/r03_pipeline_sim_time.txt)
        const int64_t kc_long = P->n_export > 0 && P->wave_K <= 0 ? 4 : (int64_t{1} << 20);
        for (int64_t KC = std::min(std::min(pick_KC(P, total + dmax), P->kc_cap), kc_long); KC >= 1 && !ok; KC /= 2) {
            for (int64_t nb = nb_max; nb >= 1; --nb) {
                const int64_t chunks = std::min<int64_t>(all_chunks, (dmax + levels * KC * kRec) / kRec + (slack + nb - 1) * kRecBatch);
                const int64_t bytes = chunks * kRec * np * (int64_t)sizeof(double) * members;
                // five eighths of the card; the shortest tasks may take thirteen sixteenths: the streaming kernel, the only alternative,
                // keeps depth x n work rows itself (1M reaches 24k deep: 204 GB of records at K = 16 against 192 GB of rows)
                if (P->dev_total_bytes > 0 && bytes > (int64_t)(P->dev_total_bytes / 16 * (KC == 1 ? 13 : 10))) continue;
                if (KC > 4 && P->wave_K <= 0 && P->dev_total_bytes > 0 && bytes > (int64_t)(P->dev_total_bytes / 5)) continue;      // long tasks only while the ring stays under a fifth of the card
                sch.kernel = Kernel::Tile; sch.KC = KC; sch.chunks = chunks; sch.ring = chunks * kRec * np * members; sch.rec_nb = nb;
                ok = true;
                break;
            }
        }
    }
    if (!ok) {      // streaming kernel: lateral rows come in, discharge rows overwrite them in place and stay until the outlet-most reaches have passed them
        const int64_t C = std::max<int64_t>(1, P->chunk_rows), lag_rows = (dmax + nsub - 1) / std::max<int64_t>(1, nsub);
        const bool in_place = P->h.identity && !s.host;
        sch.ring = in_place ? 0 : std::min<int64_t>(T, lag_rows + 2 * C + 2) * n;
        sch.mrows = in_place ? 0 : C * n;
        sch.stage = s.host ? C * n : 0;
    }
    return sch;
}

int host_pipe_prepare(rr_plan *P);

// Sizes and allocates what a call of this shape works in.  The only place on a route call's path that allocates: the
// host-pointer entry points come here by themselves, the *_dev ones expect rr_plan_reserve to have been here.
int reserve_core(rr_plan *P, const CallShape &s, Schedule *out)
{
    if (P->h.n == 0 || s.T <= 0) { *out = Schedule(); return RR_OK; }
    Schedule sch;
    for (;;) {
        sch = choose_schedule(P, s);
        if (sch.kernel == Kernel::Direct && s.uh && P->d_mrows.reserve(sch.mrows) != RR_OK) {      // no room for the convolved rows: the fused form on records
            (void)hipGetLastError();
            P->uh_rows_ok = false;
            continue;
        }
        if (P->d_ring.reserve(sch.ring) == RR_OK) break;
        (void)hipGetLastError();
        if (sch.kernel == Kernel::Direct) return fail(RR_E_ALLOC, "route: the skeleton's record ring does not fit on the device");
        if (sch.kernel == Kernel::Tick) return fail(RR_E_ALLOC, "route: the work rows of the streaming kernel do not fit on the device");
        if (s.members > 0) return fail(RR_E_ALLOC, "route: the record rings of " + std::to_string(s.members) + " ensemble members do not fit on the device");      // (kc_cap is the plan's: a smaller group is the remedy)
        if (sch.rec_nb > 1) P->nb_cap = sch.rec_nb / 2;      // fewer record batches per launch first: the ring loses the batches the out-pass held back
        else P->kc_cap = sch.KC / 2;      // then shorter tasks, a smaller ring; 0: this plan streams
    }
    int rc = P->d_mrows.reserve(sch.mrows);
    if (!rc) rc = P->d_stage.reserve(sch.stage);
    if (!rc && sch.kernel == Kernel::Tick && !P->perm_ready) rc = upload_tiled_permutations(P);
    if (!rc && sch.kernel == Kernel::Tile && s.host) rc = host_pipe_prepare(P);
    if (rc) return rc;
    // events: first / last of a call, the sampled launches (rr_plan_set_options), the second stream's
    if (!P->ev_first) { HIPCHK(hipEventCreate(&P->ev_first)); HIPCHK(hipEventCreate(&P->ev_last)); }
    const int64_t K = sch.KC * kRec, total_ticks = s.T * s.nsub + P->h.depth - 1;
    size_t samples = P->sample_every >= kSampleGroup ? (size_t)std::min<int64_t>(4096, total_ticks / P->sample_every + 1) : 0;
    if (sch.kernel == Kernel::Tile && samples > 0) samples = (size_t)std::min<int64_t>(4096, ((total_ticks + K - 1) / K + P->tp.n_levels) / 4 + 1);
    if (sch.kernel == Kernel::Direct && samples > 0) samples = (size_t)std::min<int64_t>(4096, (s.T + K - 1) / K + 1);      // every direct launch
    while (P->ev.size() < 2 * samples) { hipEvent_t e; HIPCHK(hipEventCreate(&e)); P->ev.push_back(e); }
    if (samples > 0) while (P->aux_ev.size() < 2 * rr_plan::kAuxSamples) { hipEvent_t e; HIPCHK(hipEventCreate(&e)); P->aux_ev.push_back(e); }
    *out = sch;
    return RR_OK;
}

// The schedule of the call about to start, kept on the plan for the call (P->sch).  The host-pointer entry points, which synchronise
// anyway, reserve here; the others only enqueue, so everything must have been reserved (rr_plan_reserve).  Float32 rows, the fused
// convolution and gridded runoff are parts of the record passes and of the direct row path: a call with any of them that would
// stream is refused (RR_E_UNSUPPORTED; `who` names the entry point).
int prepare_call(rr_plan *P, const CallShape &s, const char *who)
{
    if (s.host) return reserve_core(P, s, &P->sch);
    if (s.out32 && (s.factor < 1 || s.T % s.factor != 0))
        return fail(RR_E_INVALID, std::string(who) + ": float32 output: the number of rows must be a multiple of factor >= 1");
    if (s.out32 && kRecRows % (s.factor * s.nsub) != 0)
        return fail(RR_E_UNSUPPORTED, std::string(who) + ": float32 output: factor x sub-steps must divide the rows of a record batch (128)");
    const Schedule sch = choose_schedule(P, s);
    if ((s.in32 || s.out32 || s.uh || s.runoff) && sch.kernel == Kernel::Tick)
        return fail(RR_E_UNSUPPORTED, std::string(who) + " needs the time-tiled kernel or the direct row path, which this call does not get");
    const size_t samples = P->sample_every >= kSampleGroup ? 1 : 0;
    if (P->h.n > 0 && s.T > 0 && (sch.ring > P->d_ring.count() || sch.mrows > P->d_mrows.count() || sch.stage > P->d_stage.count() || !P->ev_first || P->ev.size() < 2 * samples ||
                                  (sch.kernel == Kernel::Tick && !P->perm_ready && sch.mrows > 0)))
        return fail(RR_E_STATE, "this call needs " + std::to_string((sch.ring + sch.mrows + sch.stage) * 8) + " bytes of work memory on the device (" +
                                    std::to_string((P->d_ring.count() + P->d_mrows.count() + P->d_stage.count()) * 8) + " reserved): call " +
                                    (s.members > 0 ? "rr_plan_reserve_ensemble(plan, " + std::to_string(s.members) + ", " : std::string("rr_plan_reserve(plan, mode, ")) +
                                    std::to_string(s.T) + ", " + std::to_string(s.nsub) + ", ...) first; the *_dev entry points only enqueue work");
    P->sch = sch;
    return RR_OK;
}

// The record passes run on the caller's stream between the routing launches.  (On a second stream beside them they slow the
// routing launch down by what they gain: 395 against 388 ms per year, slower on small networks too --
// profiles/r03_nt_and_rec_stream_ab.txt, r03_rec_stream_small_networks.txt.)
hipStream_t rec_stream(const rr_plan *P) { return P->ses.stream; }

// The tiles a kernel's k_tile launches, record passes and state kernels work on: the skeleton's on the direct row path, else the plan's own.
const TileSet &tiles_of(const rr_plan *P, Kernel kernel) { return kernel == Kernel::Direct ? P->ks : P->ts; }

int session_setup(rr_plan *P, Mode mode, int64_t T, int64_t nsub, const Rows &io, hipStream_t stream,
                  const double *ghost_series, double *export_series)
{
    const rr::HostPlan &H = P->h;
    const int64_t n = H.n;
    Session &S = P->ses;
    S = Session();
    S.mode = mode; S.T = T; S.nsub = nsub; S.total = T * nsub; S.io = io; S.stream = stream;
    S.members = io.members;
    S.ghost_series = ghost_series; S.export_series = export_series;
    const int64_t dmax = H.depth - 1;
    S.total_ticks = S.total + dmax;
    // the kernels index ticks, rows and chunks in 32 bits (Div32)
    if (S.total_ticks >= (int64_t{1} << 31) - (int64_t{1} << 20) || io.rows_in >= (int64_t{1} << 31) || io.rows_out >= (int64_t{1} << 31))
        return fail(RR_E_UNSUPPORTED, "more than 2^31 routing ticks or rows in one call: split it into several calls");
    S.has_in = mode != Mode::Muskingum;
    const bool host_io = io.host_out != nullptr || io.host_in != nullptr;
    S.kernel = P->sch.kernel;
    S.in_place = H.identity && !host_io && S.kernel == Kernel::Tick;
    const int64_t C = std::max<int64_t>(1, P->chunk_rows);

    P->prof_launches = P->prof_samples = P->prof_brackets = 0;
    P->aux_kind.clear();
    for (int k = 0; k < rr_plan::kAuxKinds; ++k) P->aux_launches[k] = 0;
    P->prof_reach_steps = n * S.total * std::max<int64_t>(1, S.members);
    P->ev_reaches.clear();
    P->last_stream = stream;
    if (n == 0 || S.total == 0) return RR_OK;      // (an empty call is open too: session_end closes it)
    if (P->n_ghost > 0 && !ghost_series) return fail(RR_E_INVALID, "plan has ghost reaches but no ghost series was given");
    if (P->n_export > 0 && !export_series) return fail(RR_E_INVALID, "plan has export reaches but no export series was given");

    S.KC = P->sch.KC; S.KS = P->sch.KS; S.rec_chunks = P->sch.chunks;     // ring sized by choose_schedule, allocated by rr_plan_reserve
    S.rec_nb = S.kernel == Kernel::Tile ? std::max<int64_t>(1, P->sch.rec_nb) : 1;
    if (S.kernel != Kernel::Tick) {      // the k_tile launches' arguments, over the plan's tiles or the skeleton's (whose tasks are KS chunks)
        const TileSet &ts = tiles_of(P, S.kernel);
        TileArgs &w = S.ta;
        w.tiles = ts.tmeta; w.pos = ts.pmeta; w.coef = ts.coef;
        w.sq = ts.sq; w.ss = ts.ss; w.si = ts.si; w.sqch = ts.sqch;
        w.np = (int32_t)ts.tp->np; w.KC = (int32_t)(S.kernel == Kernel::Direct ? S.KS : S.KC);
        S.n_macro = (S.total_ticks + w.KC * kRec - 1) / (w.KC * kRec);
        w.exports = export_series; w.n_export = (int32_t)P->n_export;
        w.rec = P->d_ring; w.rec_chunks = Div32((uint32_t)S.rec_chunks);
        w.n_macro = (int32_t)S.n_macro; w.total = (int32_t)S.total;
        w.has_lat = S.has_in ? 1 : 0; w.nsub = Div32((uint32_t)nsub); w.inv_nsub = 1.0 / (double)nsub;
    }
    if (S.kernel == Kernel::Direct) {
        if (io.uh_kernel || io.runoff || (!io.dev_out && !io.dev_out32) || (mode == Mode::Unit && (io.dev_in32 || P->n_ghost > 0 || P->n_export > 0)) || nsub > kDirectMaxSub ||
            (io.dev_out32 && (io.out_factor < 1 || (S.KC * kRec) % io.out_factor != 0 || T % io.out_factor != 0)))
            return fail(RR_E_STATE, "route: the direct row path was chosen for a call it does not take");      // (choose_schedule: dev_rows / out32)
        const rr::TilePlan &TP = P->dp.skel;
        const int64_t K = S.KC * kRec;
        S.n_tasks = (S.T + K - 1) / K;
        S.n_diags = TP.n_tiles > 0 ? S.n_macro + TP.n_levels - 1 : 0;
        S.n_in_batches = (S.total + 14) / kRecRows + 1;      // of the boundary series (if any)
        S.n_out_batches = TP.np > 0 ? (S.total + kRecRows - 1) / kRecRows : 0;
        for (int32_t i : P->export_reach) {
            if (!P->dp.big[i]) { S.export_lanes = true; continue; }
            S.export_skel = true;
            const int32_t p = TP.inv[i];
            S.export_skew = std::max<int64_t>(S.export_skew, (int64_t)TP.tile_level[TP.tile_of[p]] * S.KS * kRec + (TP.lag[p] & kLagMask));
        }
        DirectArgs &da = S.da;
        da.tiles = P->d_dtiles; da.n_tiles = P->dp.n_tiles; da.lane = P->d_dlane; da.coef = P->d_dcoef; da.q = P->d_dq; da.qch = nullptr;
        if (mode == Mode::Unit) { da.q = P->d_full; da.qch = P->d_chan; }      // UnitMuskingum: q_full and q_ch in params order (unit_state_in)
        da.send_ptr = P->d_dsend_ptr; da.send_lane = P->d_dsend_lane;
        da.in = S.has_in ? io.dev_in : nullptr; da.out = io.dev_out; da.n = n; da.in_rows = (uint32_t)std::max<int64_t>(1, io.rows_in); da.out_rows = (uint32_t)std::max<int64_t>(1, io.rows_out);
        da.in32 = S.has_in ? io.dev_in32 : nullptr; da.out32 = io.dev_out32; da.factor = (int32_t)std::max<int64_t>(1, io.out_factor);
        da.nsub = (int32_t)nsub; da.inv_nsub = 1.0 / (double)nsub;
        da.in32_sel = P->in32_big_endian ? kSelSwap : kSelNative; da.out32_sel = P->out32_big_endian ? kSelSwap : kSelNative;
        da.rec = P->d_ring; da.rec_chunks = (uint32_t)std::max<int64_t>(1, S.rec_chunks); da.np = (int32_t)TP.np;
        da.K = (int32_t)K; da.total = (int32_t)S.T;
        da.exports = export_series; da.n_export = (int32_t)P->n_export;
    }
    if (S.kernel == Kernel::Tile) {
        const rr::TilePlan &TP = P->tp;
        const int64_t K = S.KC * kRec;
        S.n_diags = S.n_macro + TP.n_levels - 1;
        S.n_in_batches = (S.total + 14) / kRecRows + 1;      // of the lateral rows (if any) and of the boundary series (if any)
        S.n_out_batches = (S.total + kRecRows - 1) / kRecRows;
        // external boundary reaches: a ghost in a tile of level l at lag L is read for sub-steps below (diag - l + 1) K - L,
        // an export reach there has produced the sub-steps below (diag - l) K - L
        S.ghost_slack = P->ghost_reach.empty() ? 0 : S.total_ticks + (int64_t)TP.n_levels * K;
        for (int32_t i : P->ghost_reach) { const int32_t p = TP.inv[i]; S.ghost_slack = std::min<int64_t>(S.ghost_slack, (int64_t)TP.tile_level[TP.tile_of[p]] * K + (TP.lag[p] & kLagMask)); }
        for (int32_t i : P->export_reach) { const int32_t p = TP.inv[i]; S.export_skew = std::max<int64_t>(S.export_skew, (int64_t)TP.tile_level[TP.tile_of[p]] * K + (TP.lag[p] & kLagMask)); }
        // headwaters routed by the in-pass: the short tick of a single-member call (launch_tile_diag); RapidMuskingum fed by lateral rows
        // has k_rec_in route them, UnitMuskingum's are final as any in-pass writes them (discharge = lateral inflow)
        S.hw = P->hw_inpass && P->lean_enabled && nsub == 1 && S.members == 0 &&
               (mode == Mode::Unit || (mode == Mode::Rapid && !io.runoff && !io.uh_kernel));
        if (S.members > 0) {      // an ensemble: one ring per member, the members' carried state np apart (k_tile<..., ENS>)
            if (S.members > P->ens_cap || (S.rec_chunks * kRec * TP.np) * S.members > P->d_ring.count()) return fail(RR_E_STATE, "route: the ensemble was not reserved");
            if (io.member_coeffs && S.members > P->mc_sets) return fail(RR_E_STATE, "route: fewer coefficient sets than members");
            S.ring_stride = S.rec_chunks * kRec * TP.np;
            S.ta.sq = P->d_esq; S.ta.ss = P->d_ess; S.ta.si = P->d_esi; S.ta.sqch = nullptr;
        }
    }
    if (getenv("RR_VERBOSE") && S.kernel == Kernel::Direct)
        fprintf(stderr, "rr: n=%lld T=%lld direct rows: K=%lld tiles=%d window=%d holes=%lld outlets=%lld; skeleton: positions=%lld tiles=%d levels=%d ring_chunks=%lld (%.1f GB)\n",
                (long long)n, (long long)T, (long long)(S.KC * kRec), P->dp.n_tiles, P->direct_window, (long long)P->dp.n_holes, (long long)P->dp.n_exports,
                (long long)P->dp.skel.np, P->dp.skel.n_tiles, P->dp.skel.n_levels, (long long)S.rec_chunks, (double)S.rec_chunks * kRec * P->dp.skel.np * 8 / 1e9);
    else if (getenv("RR_VERBOSE"))
        fprintf(stderr, "rr: n=%lld T=%lld nsub=%lld tiled=%d K=%lld tiles=%d levels=%d block=%d ghosts=%lld ring_chunks=%lld (%.1f GB) rec_batches=%lld lds=%zu hw_inpass=%d (%lld of %lld headwater positions)\n",
                (long long)n, (long long)T, (long long)nsub, (int)(S.kernel == Kernel::Tile), (long long)(S.KC * kRec), P->tp.n_tiles, P->tp.n_levels, P->tp.block,
                (long long)P->tp.n_ghost, (long long)S.rec_chunks, S.kernel == Kernel::Tile ? (double)S.rec_chunks * kRec * P->tp.np * 8 / 1e9 : 0.0,
                (long long)S.rec_nb, tile_lds_bytes(P->wave_threads), (int)S.hw, (long long)(S.hw ? P->hw_counts[0] : 0), (long long)P->hw_counts[1]);
    if (S.kernel == Kernel::Tick) {
        // work ring in engine order: lateral rows come in, discharge rows overwrite them in place; rows stay until the
        // outlet-most reaches have passed them
        const int64_t lag_rows = (dmax + nsub - 1) / nsub;
        S.ring_rows = S.in_place ? 0 : std::min<int64_t>(T, lag_rows + 2 * C + 2);
        if (S.ring_rows > 0xFFFFFFFFLL || T > 0x7FFFFFFFLL) return fail(RR_E_INVALID, "route: too many time rows");
        if (S.ring_rows * n > P->d_ring.count() || (!S.in_place && C * n > P->d_mrows.count()) || (host_io && C * n > P->d_stage.count()))      // prepare_call sized them
            return fail(RR_E_STATE, "route: work rows of the streaming kernel were not reserved");
        TickArgs &a = S.a;
        a.child_ptr = P->d_child_ptr; a.lag = P->d_lag; a.w = P->d_w; a.c2 = P->d_c2; a.c3 = P->d_c3; a.c4 = P->d_c4;
        a.c1row = P->weights_uniform ? P->d_c1row_h : nullptr;
        a.isum = P->d_isum; a.bidx = P->d_bidx;
        a.ghost = ghost_series; a.exports = export_series; a.n_ghost = (int32_t)P->n_ghost; a.n_export = (int32_t)P->n_export;
        a.total_substeps = S.total; a.nsub = Div32((uint32_t)nsub); a.inv_nsub = 1.0 / (double)nsub;
        if (S.in_place) {
            a.in = io.dev_in; a.in_ld = n; a.in_rows = Div32((uint32_t)std::max<int64_t>(1, io.rows_in));
            a.out = io.dev_out; a.out_ld = n; a.out_rows = Div32((uint32_t)io.rows_out);
        } else {
            a.in = S.has_in ? P->d_ring : nullptr; a.in_ld = n; a.in_rows = Div32((uint32_t)S.ring_rows);
            a.out = P->d_ring; a.out_ld = n; a.out_rows = Div32((uint32_t)S.ring_rows);
        }
    }
    S.max_samples = P->sample_every >= kSampleGroup ? (size_t)std::min<int64_t>(4096, S.total_ticks / P->sample_every + 1) : 0;
    if (S.kernel == Kernel::Tile && S.max_samples > 0) S.max_samples = (size_t)std::min<int64_t>(4096, S.n_diags / 4 + 1);     // every fourth launch
    if (S.kernel == Kernel::Direct && S.max_samples > 0) S.max_samples = (size_t)std::min<int64_t>(4096, S.n_tasks);            // every direct launch
    S.max_samples = std::min(S.max_samples, P->ev.size() / 2);      // events are made by rr_plan_reserve, never here
    if (!P->ev_first) return fail(RR_E_STATE, "route: the plan's events were not reserved");
    HIPCHK(hipEventRecord(P->ev_first, stream));
    return RR_OK;
}

// Opens a routing call on the plan: open exactly when session_setup set all of it up.
int session_begin(rr_plan *P, Mode mode, int64_t T, int64_t nsub, const Rows &io, hipStream_t stream,
                  const double *ghost_series, double *export_series)
{
    if (P->ses.open) return fail(RR_E_STATE, "a routing call is already open on this plan (rr_stream_end it first)");
    const int rc = session_setup(P, mode, T, nsub, io, stream, ghost_series, export_series);
    P->ses.open = rc == RR_OK;
    return rc;
}

// A skeleton position's carried value `state` (TileSet::sq or ::sqch) back into the params-order array the lanes kept.
void launch_skel_state_out(const TileSet &ks, double *dst, const DevBuf<double> &state, hipStream_t stream)
{
    if (ks.tp->np > 0) hipLaunchKernelGGL(k_skel_state_out, grid1(ks.tp->np), dim3(kBlock), 0, stream, dst, (const double *)state, ks.perm.get(), ks.pmeta.get(), (int32_t)ks.tp->np);
}

// params order <-> engine order through the two-phase tiled permutation (k_perm_a / k_perm_b); mrows holds nrows x n intermediate values
void permute_rows_via(rr_plan *P, int which, const RowView &src, const RowView &dst, int64_t t0, int nrows, double *mrows, hipStream_t stream)
{
    const int64_t n = P->h.n;
    constexpr int E = kPermE;
    const int64_t tile = (int64_t)E * kPermThreads;
    const int rpb = (int)std::max<int64_t>(1, P->perm_rows_per_block);
    dim3 g((unsigned)((n + tile - 1) / tile), (unsigned)((nrows + rpb - 1) / rpb));
    const size_t lds_bytes = (size_t)tile * sizeof(double);
    hipLaunchKernelGGL(k_perm_a<E>, g, dim3(kPermThreads), lds_bytes, stream, src, mrows, n,
                       (const uint16_t *)P->d_slot_a[which], (const int32_t *)P->d_m_index[which], t0, nrows, rpb);
    hipLaunchKernelGGL(k_perm_b<E>, g, dim3(kPermThreads), lds_bytes, stream, dst, (const double *)mrows, n,
                       (const uint16_t *)P->d_slot_b[which], t0, nrows, rpb);
}

// the same through the plan's work rows, on the open session's stream
void permute_rows(rr_plan *P, int which, const RowView &src, const RowView &dst, int64_t t0, int nrows)
{
    permute_rows_via(P, which, src, dst, t0, nrows, P->d_mrows, P->ses.stream);
}

int session_load_rows(rr_plan *P, int64_t r0, int64_t r1)   // params order -> ring
{
    Session &S = P->ses;
    if (S.in_place || !S.has_in) return RR_OK;
    const int64_t n = P->h.n, C = std::max<int64_t>(1, P->chunk_rows);
    const int nrows = (int)(r1 - r0);
    const RowView ring_view{P->d_ring, n, 0, (uint32_t)std::max<int64_t>(1, S.ring_rows)};
    if (S.io.host_in) {
        HIPCHK(hipMemcpyAsync(P->d_stage, S.io.host_in + r0 * n, (size_t)nrows * n * sizeof(double),
                              hipMemcpyHostToDevice, S.stream));
        permute_rows(P, 0, RowView{P->d_stage, n, r0, (uint32_t)C}, ring_view, r0, nrows);
        HIPCHK(hipStreamSynchronize(S.stream));   // the stage is reused by the next chunk
    } else {
        permute_rows(P, 0, RowView{const_cast<double *>(S.io.dev_in), n, 0, (uint32_t)S.io.rows_in}, ring_view, r0, nrows);
    }
    return RR_OK;
}

int session_store_rows(rr_plan *P, int64_t r0, int64_t r1)   // ring -> params order
{
    Session &S = P->ses;
    if (S.in_place) return RR_OK;
    const int64_t n = P->h.n, C = std::max<int64_t>(1, P->chunk_rows);
    const RowView ring_view{P->d_ring, n, 0, (uint32_t)std::max<int64_t>(1, S.ring_rows)};
    for (int64_t b0 = r0; b0 < r1; b0 += C) {
        const int nrows = (int)std::min<int64_t>(C, r1 - b0);
        if (S.io.host_out) {
            permute_rows(P, 1, ring_view, RowView{P->d_stage, n, b0, (uint32_t)C}, b0, nrows);
            HIPCHK(hipMemcpyAsync(S.io.host_out + b0 * n, P->d_stage, (size_t)nrows * n * sizeof(double),
                                  hipMemcpyDeviceToHost, S.stream));
            HIPCHK(hipStreamSynchronize(S.stream));
        } else {
            permute_rows(P, 1, ring_view, RowView{S.io.dev_out, n, 0, (uint32_t)S.io.rows_out}, b0, nrows);
        }
    }
    return RR_OK;
}

// The engine positions [p_lo, p_hi) with work at tick tau of a call of `total` sub-steps: the lags with tau - total < lag <= tau.
// False when there is none.
inline bool tick_window(const rr::HostPlan &H, int64_t tau, int64_t total, int64_t &p_lo, int64_t &p_hi)
{
    p_lo = H.lag_start[std::max<int64_t>(0, tau - total + 1)];
    p_hi = H.lag_start[std::min<int64_t>(tau, H.depth - 1) + 1];
    return p_hi > p_lo;
}

typedef void (*tick_unit_kernel_t)(const UnitTickArgs);
typedef void (*tick_kernel_t)(const TickArgs);
tick_unit_kernel_t tick_unit_kernel(bool one) { return one ? (tick_unit_kernel_t)k_tick_unit<true> : (tick_unit_kernel_t)k_tick_unit<false>; }
tick_kernel_t tick_kernel(bool lat, bool one)      // lat: RapidMuskingum's lateral term; one: one sub-step per row
{
    return lat ? (one ? (tick_kernel_t)k_tick<true, true> : (tick_kernel_t)k_tick<true, false>) : (one ? (tick_kernel_t)k_tick<false, true> : (tick_kernel_t)k_tick<false, false>);
}

int session_launch_tick(rr_plan *P, int64_t tau)
{
    Session &S = P->ses;
    const int64_t n = P->h.n;
    int64_t p_lo, p_hi;
    if (!tick_window(P->h, tau, S.total, p_lo, p_hi)) return RR_OK;
    TickArgs &a = S.a;
    a.p_lo = (int32_t)p_lo; a.p_hi = (int32_t)p_hi; a.tau = tau;
    a.xc = P->d_x + (tau % 3) * n;
    a.xa = P->d_x + ((tau + 2) % 3) * n;
    a.xb = P->d_x + ((tau + 1) % 3) * n;
    // sampling: every sample_every-th launch opens a bracket of kSampleGroup consecutive launches, so the
    // event overhead (~5 us per pair) is amortised and the figure is comparable with rocprofv3's per-kernel time
    const int64_t phase = S.max_samples > 0 ? P->prof_launches % P->sample_every : -1;
    if (phase == 0 && !S.bracket_open && (size_t)P->prof_brackets < S.max_samples) {
        HIPCHK(hipEventRecord(P->ev[2 * P->prof_brackets], S.stream));
        S.bracket_open = true;
    }
    const dim3 g = grid1(p_hi - p_lo);
    const bool one = S.nsub == 1;
    if (S.mode == Mode::Unit) {
        UnitTickArgs ua{};
        ua.t = a; ua.hw_children = P->d_hwc; ua.qch = P->d_qch;
        ua.a2 = P->unit_general ? P->d_a2 : nullptr; ua.c1own = P->d_c1own;
        if (P->unit_general) { ua.t.c1row = nullptr; ua.zc = P->d_z + (tau % 3) * n; ua.za = P->d_z + ((tau + 2) % 3) * n; }
        hipLaunchKernelGGL(tick_unit_kernel(one), g, dim3(kBlock), 0, S.stream, ua);
    } else {
        hipLaunchKernelGGL(tick_kernel(S.mode == Mode::Rapid, one), g, dim3(kBlock), 0, S.stream, a);
    }
    if (S.bracket_open) {
        S.bracket_reaches += p_hi - p_lo;
        ++P->prof_samples;
        if (P->prof_samples % kSampleGroup == 0) {
            HIPCHK(hipEventRecord(P->ev[2 * P->prof_brackets + 1], S.stream));
            ++P->prof_brackets;
            P->ev_reaches.push_back(S.bracket_reaches);
            S.bracket_reaches = 0;
            S.bracket_open = false;
        }
    }
    ++P->prof_launches;
    return RR_OK;
}

typedef void (*tile_kernel_t)(const TileArgs);

// Tile = one position per thread, 512 threads, two workgroups per CU: 16 waves per CU whose two record buffers fill the register
// file, and while the waves of one workgroup wait to issue their record loads the other one ticks (368 ms per year at 1M reaches
// against 391 with one 1,024-thread workgroup and 382 with four 256-thread ones; smaller tiles for smaller networks do not pay
// either: profiles/r03_tile_size_sweep.txt).
constexpr int kTileThreads = 512;
tile_kernel_t tile_kernel(bool unit, bool sub, bool lean = false, bool nolat = false)
{
    constexpr int T = kTileThreads;
    if (lean && nolat && !unit && !sub) return (tile_kernel_t)k_tile<T, false, false, true, true>;      // channel-only routing, one sub-step per row: the short tick without a lateral term
    return unit ? (sub ? (tile_kernel_t)k_tile<T, true, true> : (lean ? (tile_kernel_t)k_tile<T, true, false, true> : (tile_kernel_t)k_tile<T, true, false>))
                : (sub ? (tile_kernel_t)k_tile<T, false, true> : (lean ? (tile_kernel_t)k_tile<T, false, false, true> : (tile_kernel_t)k_tile<T, false, false>));
}

// RapidMuskingum's k_tile forms, member-batched: the general tick, with or without sub-steps.  (The short tick's member-batched form needs 72
// bytes of scratch at 128 VGPRs -- the member's chunk and position offsets tip it over -- so an ensemble with one sub-step per row runs the
// general tick on every tile, as RR_TILE_LEAN=0 does: the same multiply-adds on the same sums, which can differ only in the sign of a zero.)
// mcoef: a coefficient set per member (k_tile<..., MCOEF>): the same two forms over the members' table.
tile_kernel_t tile_ens_kernel(bool sub, bool mcoef = false)
{
    constexpr int T = kTileThreads;
    if (mcoef) return sub ? (tile_kernel_t)k_tile<T, false, true, false, false, true, true> : (tile_kernel_t)k_tile<T, false, false, false, false, true, true>;
    return sub ? (tile_kernel_t)k_tile<T, false, true, false, false, true> : (tile_kernel_t)k_tile<T, false, false, false, false, true>;
}

// Launch d of the time-tiled schedule: the tasks (tile, macro-chunk d - level) of every tile whose macro-chunk exists.
// Tiles are stored by level, so they are one contiguous range; a tile with no active position returns at once.
// ts: the plan's own tiles, or the skeleton of the direct row path (its levels start at 1); coef_unit: the coefficients of UnitMuskingum's short tick.
int launch_tile_diag(rr_plan *P, const TileSet &ts, TileArgs &w, const double *coef_unit, int64_t d, bool sampled)
{
    Session &S = P->ses;
    const rr::TilePlan &TP = *ts.tp;
    const int64_t l_lo = std::max<int64_t>(0, d - (S.n_macro - 1)), l_hi = std::min<int64_t>(TP.n_levels - 1, d);
    if (l_hi < l_lo) return RR_OK;
    int64_t t_lo = TP.level_start[l_lo], t_hi = TP.level_start[l_hi + 1];
    // tiles are sorted by their smallest lag inside a level; while the pipeline fills, the tiles of level 0 that
    // have not started yet are a suffix of it
    const int64_t K = (int64_t)w.KC * kRec;      // (the skeleton of the direct row path may run shorter tasks than its lanes)
    if (l_lo == 0) {
        const int64_t end0 = TP.level_start[1];
        int64_t hi = std::min<int64_t>(t_hi, end0);
        while (hi > t_lo && (d + 1) * K <= TP.tile_lag_lo[hi - 1]) --hi;
        if (t_hi <= end0) t_hi = hi;     // only level 0 in this launch: trim; otherwise the idle ones just return
    }
    if (t_hi <= t_lo) return RR_OK;
    w.diag = (int32_t)d; w.t_first = (int32_t)t_lo; w.t_last = (int32_t)t_hi - 1;
    // every fourth launch is bracketed by HIP events, full or not (fill and drain launches run fewer tiles), so the
    // sampled average is the average rocprofv3 reports for the kernel; the position-ticks of a sample are those of the
    // tiles that run a task in it
    const bool sample = sampled && S.max_samples > 0 && (P->prof_launches % 4) == 0 && (size_t)P->prof_brackets < S.max_samples;
    if (sample) HIPCHK(hipEventRecord(P->ev[2 * P->prof_brackets], S.stream));
    // one workgroup per resident slot (16 waves per CU); each walks its share of the launch's tiles
    const dim3 g((unsigned)std::min<int64_t>(t_hi - t_lo, (int64_t)P->cu_count * (1024 / P->wave_threads)));
    const size_t lds_bytes = tile_lds_bytes(P->wave_threads);
    // With one sub-step per row every mode runs the short tick (k_tile<..., LEAN>), and beside it the general kernel for
    // the tiles the short tick does not take (a reach with more than three upstream reaches); RR_TILE_LEAN=0: the general one
    const bool unit = S.mode == Mode::Unit;
    const bool lean = S.nsub == 1 && P->lean_enabled;      // every router's default (dt_routing = dt_runoff); sub-steps keep the general tick
    if (S.members > 0) {
        // An ensemble (k_tile<..., ENS>): the tasks of every member, member on the grid's second dimension.  The workgroups of one member walk its tiles as k_tile's do;
        // together the members' take the slots one member's would (fewer tiles each: the card fills with (tile, member) tasks however few tiles the network has).
        const dim3 ge((unsigned)std::min<int64_t>(t_hi - t_lo, std::max<int64_t>(1, ((int64_t)P->cu_count * (1024 / kTileThreads) + S.members - 1) / S.members)), (unsigned)S.members);
        const bool mcoef = S.io.member_coeffs;      // a parameter ensemble: member m's coefficients at 3 m np doubles of the members' table
        w.tile_filter = 0; w.coef = mcoef ? P->d_mcoef.get() : ts.coef.get();      // (member m's ring: chunks [m C, (m + 1) C); its state: positions [m np, (m + 1) np))
        hipLaunchKernelGGL(tile_ens_kernel(S.nsub > 1, mcoef), ge, dim3((unsigned)kTileThreads), tile_lds_bytes(kTileThreads), S.stream, w);
    } else {
        w.tile_filter = lean ? 1 : 0;
        w.coef = (lean && unit) ? coef_unit : ts.coef.get();
        const int4 *const pos = w.pos;
        if (lean && S.hw) {      // (S.hw: the plan's own tiles) the in-pass headwaters are published, not stored: their flag and, RapidMuskingum, zero coefficients
            w.pos = P->d_pmeta_hw;
            if (!unit) w.coef = P->d_coef_hw;
        }
        hipLaunchKernelGGL(tile_kernel(unit, S.nsub > 1, lean, S.mode == Mode::Muskingum), g, dim3((unsigned)P->wave_threads), lds_bytes, S.stream, w);
        w.pos = pos;      // (no in-pass headwater in a tile the general kernel takes)
        if (lean && ts.n_wide > 0) {
            w.tile_filter = 2; w.coef = ts.coef;
            hipLaunchKernelGGL(tile_kernel(unit, false, false), g, dim3((unsigned)P->wave_threads), lds_bytes, S.stream, w);
        }
    }
    if (sample) {
        HIPCHK(hipEventRecord(P->ev[2 * P->prof_brackets + 1], S.stream));
        // position-ticks of the sample: the tiles that run a task in this launch (k_tile's select(): the macro-chunk exists and
        // some position is active in it); a tile that returns at once moves nothing -- in a short call most of a launch's tiles
        int64_t moved = 0;
        for (int64_t c = t_lo; c < t_hi; ++c) {
            const int64_t m = d - TP.tile_level[c];
            if (m < 0 || m >= S.n_macro || m * K >= TP.tile_lag_hi[c] + S.total || (m + 1) * K <= TP.tile_lag_lo[c]) continue;
            moved += TP.tile_ptr[c + 1] - TP.tile_ptr[c];
        }
        P->ev_reaches.push_back(moved * K * std::max<int64_t>(1, S.members));
        P->prof_samples += K;
        ++P->prof_brackets;
    }
    return RR_OK;
}

// Whether launch d of a tile plan has any tile to run (launch_tile_diag returns early otherwise).
bool tile_diag_launches(const rr_plan *P, const rr::TilePlan &TP, int64_t d)
{
    const Session &S = P->ses;
    const int64_t l_lo = std::max<int64_t>(0, d - (S.n_macro - 1)), l_hi = std::min<int64_t>(TP.n_levels - 1, d);
    return l_hi >= l_lo && TP.level_start[l_hi + 1] > TP.level_start[l_lo];
}

// What every record pass of the open call hands its kernel, whichever columns it is over: the ring and its positions, the call's length,
// the float32 rows' format.  The passes add their columns (n, colmeta, cols), their rows and what only they have.
RecPermArgs rec_args(const rr_plan *P, int64_t batch)
{
    const Session &S = P->ses;
    RecPermArgs ra{};
    ra.in32_sel = P->in32_big_endian ? kSelSwap : kSelNative; ra.out32_sel = P->out32_big_endian ? kSelSwap : kSelNative;
    ra.rec = P->d_ring; ra.rec_chunks = Div32((uint32_t)S.rec_chunks); ra.np = tiles_of(P, S.kernel).tp->np;
    ra.T = S.T; ra.total = S.total; ra.batch = batch; ra.nsub = Div32((uint32_t)S.nsub);
    ra.factor = Div32((uint32_t)std::max<int64_t>(1, S.io.out_factor));
    return ra;
}

// Boundary inflow of a partitioned network: the ghost series (total sub-steps x ghosts, row = sub-step) is a matrix of
// tick-rows like the lateral rows, and its columns become the records of the ghost positions by the same pass.
void launch_ghost_permute(rr_plan *P, int64_t batch)
{
    Session &S = P->ses;
    RecPermArgs ra = rec_args(P, batch);
    ra.T = S.total; ra.nsub = Div32(1u);      // a row is a sub-step
    // (direct row path: the ghosts' records are those of the skeleton's positions that mirror them)
    ra.n = P->n_ghost; ra.colmeta = S.kernel == Kernel::Direct ? P->d_kghostmeta : P->d_ghostmeta;
    ra.rows = RowView{const_cast<double *>(S.ghost_series), P->n_ghost, 0, (uint32_t)S.total};
    hipLaunchKernelGGL(k_rec_in<false>, dim3((unsigned)((P->n_ghost + kRecInCols - 1) / kRecInCols)), dim3(kRecInThreads), 0, rec_stream(P), ra);
}

typedef void (*rec_in_uh_t)(const RecPermArgs, const UhArgs);
constexpr int kUhFusedMaxTaps = 64;
int uh_padded_taps(int64_t n_ks) { return n_ks <= 16 ? 16 : (n_ks <= 48 ? 48 : 64); }
rec_in_uh_t rec_in_uh_kernel(bool sub, int64_t n_ks, int batches, bool in32 = false)
{
    const int nk = uh_padded_taps(n_ks);
#define RR_UHIN_IN(NK_, B_, S_) (in32 ? (rec_in_uh_t)k_rec_in_uh<S_, NK_, B_, true> : (rec_in_uh_t)k_rec_in_uh<S_, NK_, B_, false>)
#define RR_UHIN_SUB(NK_, B_) (sub ? RR_UHIN_IN(NK_, B_, true) : RR_UHIN_IN(NK_, B_, false))
#define RR_UHIN_PICK(NK_) (batches == 2 ? RR_UHIN_SUB(NK_, 2) : RR_UHIN_SUB(NK_, 1))
    return nk == 16 ? RR_UHIN_PICK(16) : (nk == 48 ? RR_UHIN_PICK(48) : RR_UHIN_PICK(64));
#undef RR_UHIN_PICK
#undef RR_UHIN_SUB
#undef RR_UHIN_IN
}

// The record passes' forms.  (The casts settle each form where it stands: kernels lie in the code object in the order they are first named.)
typedef void (*rec_kernel_t)(const RecPermArgs);
typedef void (*rec_ens_kernel_t)(const RecEnsArgs);
typedef void (*rec_in_runoff_t)(const RecPermArgs, const RunoffArgs);
rec_kernel_t rec_out_kernel(bool sub, bool f32)
{
    return f32 ? (sub ? (rec_kernel_t)k_rec_out<true, true> : (rec_kernel_t)k_rec_out<false, true>) : (sub ? (rec_kernel_t)k_rec_out<true, false> : (rec_kernel_t)k_rec_out<false, false>);
}
rec_ens_kernel_t rec_in_ens_kernel(bool sub, bool in32)      // member-batched
{
    return in32 ? (sub ? (rec_ens_kernel_t)k_rec_in<true, true, true> : (rec_ens_kernel_t)k_rec_in<false, true, true>) : (sub ? (rec_ens_kernel_t)k_rec_in<true, false, true> : (rec_ens_kernel_t)k_rec_in<false, false, true>);
}
rec_ens_kernel_t rec_out_ens_kernel(bool sub, bool f32)
{
    return f32 ? (sub ? (rec_ens_kernel_t)k_rec_out<true, true, true> : (rec_ens_kernel_t)k_rec_out<false, true, true>) : (sub ? (rec_ens_kernel_t)k_rec_out<true, false, true> : (rec_ens_kernel_t)k_rec_out<false, false, true>);
}
rec_in_runoff_t rec_in_runoff_kernel(bool f32) { return f32 ? (rec_in_runoff_t)k_rec_in_runoff<float> : (rec_in_runoff_t)k_rec_in_runoff<double>; }
rec_kernel_t rec_in_kernel(bool sub, bool in32, bool hw)      // hw (the in-pass routes the flagged headwaters): only with one sub-step per row
{
    if (in32) return sub ? (rec_kernel_t)k_rec_in<true, true> : (hw ? (rec_kernel_t)k_rec_in<false, true, false, true> : (rec_kernel_t)k_rec_in<false, true>);
    return sub ? (rec_kernel_t)k_rec_in<true> : (hw ? (rec_kernel_t)k_rec_in<false, false, false, true> : (rec_kernel_t)k_rec_in<false>);
}

// The out-pass over ra.n columns (the plan's, or the holes' of the direct row path).
void launch_rec_out(const RecPermArgs &ra, bool sub, hipStream_t st)
{
    hipLaunchKernelGGL(rec_out_kernel(sub, ra.rows32 != nullptr), dim3((unsigned)((ra.n + kRecOutCols - 1) / kRecOutCols)), dim3(kRecOutThreads), 0, st, ra);
}

// `count` batches from `batch` on (session_advance_tile): up to Session::rec_nb for k_rec_in / k_rec_out, up to 2 for the fused
// convolution, 1 for gridded runoff
void launch_rec_permute(rr_plan *P, bool in, int64_t batch, int count = 1)
{
    Session &S = P->ses;
    const int64_t n = P->h.n;
    RecPermArgs ra = rec_args(P, batch);
    ra.batches = count;
    ra.n = n; ra.colmeta = P->d_colmeta;
    ra.scale = (in && S.mode == Mode::Rapid) ? P->d_c4_params : nullptr;
    if (in) { ra.rows = RowView{const_cast<double *>(S.io.dev_in), n, 0, (uint32_t)S.io.rows_in}; ra.rows_in32 = S.io.dev_in32; }
    else { ra.rows = RowView{S.io.dev_out, n, 0, (uint32_t)std::max<int64_t>(1, S.io.rows_out)}; ra.rows32 = S.io.dev_out32; }
    ra.clamp = S.nsub > 1 ? 0 : (S.mode == Mode::Unit ? 2 : 1);
    // The out-pass walks its column tiles in XCD-contiguous order (xcd_swizzle): where the row pitch is not a whole number
    // of 128-byte lines neighbouring tiles write parts of the same lines, and on one XCD those meet in its L2 (1.25M-reach
    // part with an odd column count: 522 -> 473 ms per year; 1% - 2% with an aligned pitch too).  The in-pass gains
    // nothing from it (its shared lines are reads) and the two together were slower: profiles/r02_rec_swizzle.txt.
    ra.swizzle = in ? 0 : 1;
    // one column tile per workgroup, dispatched in address order: a persistent grid with the next tile's loads in flight was no
    // faster (427 / 469 us per 128 rows against 419 / 434-448 at 1M reaches; a plain copy shows the same, profiles/r03_hbm_probe_*.txt)
    static_assert(kRecInCols == kRecOutCols && kRecInThreads == kRecOutThreads, "one grid for the member-batched in- and out-pass");
    const unsigned tiles = (unsigned)((n + kRecInCols - 1) / kRecInCols);
    const bool sub = S.nsub > 1, in32 = ra.rows_in32 != nullptr;
    const bool hw = in && S.hw && S.mode == Mode::Rapid;      // k_rec_in<..., HW>: the flagged columns leave as discharge
    if (hw) { ra.hw_coef = P->d_hwcoef; ra.hw_carry = P->d_hwq; }
    hipStream_t st = rec_stream(P);
    const int aux = aux_begin(P, in ? 0 : 1, st);
    if (S.members > 0) {      // an ensemble: every member's rows in one launch, member on the grid's second dimension
        RecEnsArgs e{ra, S.ring_stride, in ? S.io.in_pitch : S.io.out_pitch, 0};      // (in32 / out32 rows: the pitch counts float32 elements)
        if (in && S.io.member_coeffs) { e.scale = P->d_mc4; e.scale_pitch = n; }      // a parameter ensemble: the member's own c4dt
        hipLaunchKernelGGL(in ? rec_in_ens_kernel(sub, in32) : rec_out_ens_kernel(sub, ra.rows32 != nullptr), dim3(tiles, (unsigned)S.members), dim3(kRecInThreads), 0, st, e);
    } else if (!in) {
        launch_rec_out(ra, sub, st);
    } else if (S.io.runoff) {
        const dim3 gr((unsigned)((n + kRunoffInThreads - 1) / kRunoffInThreads), (unsigned)kRecBatch);
        hipLaunchKernelGGL(rec_in_runoff_kernel(S.io.runoff->is_f32), gr, dim3(kRunoffInThreads), 0, st, ra, *S.io.runoff);
    } else if (S.io.uh_kernel) {
        UhArgs ua{S.io.uh_kernel, S.io.uh_state, (int32_t)S.io.uh_nks};
        hipLaunchKernelGGL(rec_in_uh_kernel(sub, S.io.uh_nks, count, in32), dim3((unsigned)((n + kUhCols - 1) / kUhCols)), dim3(uh_threads(count)),
                           rec_in_uh_lds_bytes(uh_padded_taps(S.io.uh_nks), count), st, ra, ua);
    } else {
        hipLaunchKernelGGL(rec_in_kernel(sub, in32, hw), dim3(tiles), dim3(kRecInThreads), 0, st, ra);
    }
    aux_end(P, aux, st);
}

// Whether the ring slots batch j of an in-pass writes are free: a slot is recycled only after every tick-row it can hold has left.  Batch j writes, for a position of lag L,
// the records whose last tick-row lies in the batch -- chunks up to (R (j + 1) + L) / 16, R = kRecRows (the boundary in-pass: whole records, zeros past the call's end).
// One ring revolution earlier that slot held the same position's tick-rows up to R (j + 1) - 16 rec_chunks + 15, whatever L is: those must have left.
bool slot_free(const Session &S, int64_t j)
{
    const int64_t must_have_left = kRecRows * (j + 1) + kRec - kRec * S.rec_chunks;
    return must_have_left <= 0 || S.ticks_stored >= std::min(S.total, must_have_left);
}

// Time-tiled schedule: batches of kRecRows (128) tick-rows become records as soon as their rows are there and their ring slots
// are free, launches run while their input is present, finished batches leave.
int session_advance_tile(rr_plan *P, int64_t rows_ready, int64_t ghost_ready, int64_t *export_ready)
{
    Session &S = P->ses;
    const int64_t dmax = P->h.depth - 1, levels = P->tp.n_levels, K = S.KC * kRec;
    const int64_t ticks_ready = std::min(rows_ready, S.T) * S.nsub;
    for (;;) {
        bool progressed = false;
        // one batch of tick-rows -> records; a record slot is recycled only after every tick-row it can hold has left.
        // Lateral rows and boundary sub-steps (the ghost series of a partitioned network) advance separately: a ghost in a
        // tile of level l at lag L is first read (l K + L) ticks into the schedule, so the boundary may trail the rows.
        if (S.has_in && S.in_batches < S.n_in_batches && ticks_ready >= std::min(kRecRows * (S.in_batches + 1), S.total) && slot_free(S, S.in_batches)) {
            // the next batches along while their rows and ring slots are there too (less to read per value): up to rec_nb for k_rec_in,
            // two for the fused convolution, one batch a launch for gridded runoff
            const int max_count = S.io.runoff ? 1 : (S.io.uh_kernel ? (P->uh_pairs ? 2 : 1) : (int)S.rec_nb);
            int count = 1;
            while (count < max_count && S.in_batches + count < S.n_in_batches &&
                   ticks_ready >= std::min(kRecRows * (S.in_batches + count + 1), S.total) && slot_free(S, S.in_batches + count)) ++count;
            launch_rec_permute(P, true, S.in_batches, count);
            S.in_batches += count;
            progressed = true;
        }
        if (P->n_ghost > 0 && S.ghost_batches < S.n_in_batches && (!S.has_in || S.ghost_batches < S.in_batches) &&      // after the lateral batch: that one writes zeros into the ghosts' records
            ghost_ready >= std::min(kRecRows * (S.ghost_batches + 1), S.total) && slot_free(S, S.ghost_batches)) {
            launch_ghost_permute(P, S.ghost_batches);
            ++S.ghost_batches;
            progressed = true;
        }
        auto loaded_ticks = [&](int64_t batches) { return batches >= S.n_in_batches ? S.total : std::max<int64_t>(0, kRecRows * batches - 15); };
        const int64_t have = S.has_in ? loaded_ticks(S.in_batches) : S.total;
        const int64_t have_ghost = P->n_ghost > 0 ? loaded_ticks(S.ghost_batches) : S.total;
        S.rows_loaded = have / S.nsub;
        // launch d runs macro-chunk d of the tiles of level 0: ticks below (d + 1) K need the tick-rows below that
        int64_t launched = 0;
        const int64_t batch = std::max<int64_t>(1, kRecRows / K);
        while (S.diag < S.n_diags && launched < batch) {
            const int64_t need_ticks = std::min((S.diag + 1) * K, S.total);
            if (have < need_ticks) break;
            if (have_ghost < std::min(std::max<int64_t>(0, (S.diag + 1) * K - S.ghost_slack), S.total)) break;
            // the tasks of this launch overwrite records in place: nothing they write may still be waiting to leave from
            // one ring revolution earlier (their chunks are at most (d + 1) KC - 1)
            const int64_t top = std::min(std::min(S.diag + 1, S.n_macro) * S.KC - 1, (S.total_ticks - 1) / kRec);      // (a task longer than what is left of the call -- RR_WAVE_K -- ends with the call's last chunk)
            if (top >= S.rec_chunks && S.ticks_stored < std::min(S.total, kRec * (top - S.rec_chunks + 1))) break;
            int rc = launch_tile_diag(P, P->ts, S.ta, P->d_coef_unit, S.diag, true);
            ++P->prof_launches;
            if (rc) return rc;
            ++S.diag; ++launched;
            progressed = true;
        }
        // the tiles of the last level have finished macro-chunk diag - levels; every other tile is further along
        const int64_t m_done = S.diag - levels;
        int64_t done = 0;
        if (S.diag >= S.n_diags) done = S.total;
        else if (m_done >= 0) done = std::max<int64_t>(0, (m_done + 1) * K - dmax);
        done = std::min(done, S.total);
        // finished batches leave rec_nb at a time; fewer at the end of the call, and when nothing else can move -- so every call and every
        // rr_stream_advance returns with all its finished batches out, as with one batch per launch (choose_schedule: the ring holds the rest)
        auto out_ready = [&](int64_t j) {
            const int64_t end = std::min(kRecRows * (j + 1), S.total);
            return done >= end && (end + S.nsub - 1) / S.nsub <= S.out_limit;
        };
        while (S.out_batches < S.n_out_batches) {
            int count = 0;
            while (count < S.rec_nb && S.out_batches + count < S.n_out_batches && out_ready(S.out_batches + count)) ++count;
            if (count == 0 || (count < S.rec_nb && S.out_batches + count < S.n_out_batches && progressed)) break;
            launch_rec_permute(P, false, S.out_batches, count);
            S.out_batches += count;
            S.ticks_stored = std::min(S.total, kRecRows * S.out_batches);
            progressed = true;
        }
        if (!progressed) break;
    }
    S.rows_stored = S.ticks_stored / S.nsub;
    if (S.diag >= S.n_diags) S.tau = S.total_ticks;
    if (export_ready) {
        const int64_t e = S.diag >= S.n_diags ? S.total : S.diag * K - S.export_skew;
        *export_ready = std::max<int64_t>(0, std::min(e, S.total));
    }
    return RR_OK;
}

// The direct row path (rr_kernels_direct.hpp).  Launch d: k_direct routes rows [d K, (d + 1) K) of every small subtree straight from
// and to the caller's rows, forwarding the skeleton's lateral inflow and the subtrees' outflow into the skeleton's records; then
// the skeleton's tiles of level l run macro-chunk d - l on those records (levels start at 1: what they read was written by an
// earlier launch); rows all of whose skeleton reaches are final get their holes patched from the records (k_rec_out over the
// holes' columns), 128 rows at a time, which also frees their ring slots.
// (The skeleton's launches and the out-pass on a second stream beside the direct launches, with or without CUs set aside for them,
// changed nothing -- 212 to 226 ms per year against 212: profiles/r04_direct_second_stream_ab.txt -- the out-pass's scattered
// 8-byte stores, 5 % of the columns, compete for the same memory system.)
int session_advance_direct(rr_plan *P, int64_t rows_ready, int64_t ghost_ready, int64_t *export_ready)
{
    Session &S = P->ses;
    const rr::TilePlan &TP = P->dp.skel;
    const int64_t dmax = P->h.depth - 1, levels = TP.n_levels, K = S.KC * kRec, Kt = K * S.nsub, KS = S.KS * kRec, per = Kt / KS, n = P->h.n;      // K rows = Kt ticks per direct task
    rows_ready = std::min(rows_ready, S.T);
    const bool skel = TP.n_tiles > 0, ghosts = skel && P->n_ghost > 0;
    for (;;) {
        bool progressed = false;
        while (S.d_done < S.n_tasks) {
            const int64_t d = S.d_done;
            if (rows_ready < std::min((d + 1) * K, S.T)) break;
            if (skel) {      // this launch writes record slots up to tick (d + 1) K + dmax: whatever they held one revolution earlier must have left
                const int64_t top = std::min((d + 1) * Kt + dmax, S.total_ticks) / kRec;
                if (top >= S.rec_chunks && S.ticks_stored < std::min(S.total, kRec * (top - S.rec_chunks + 1))) break;
            }
            const bool sample = S.max_samples > 0 && (size_t)P->prof_brackets < S.max_samples;
            if (sample) HIPCHK(hipEventRecord(P->ev[2 * P->prof_brackets], S.stream));
            S.da.m = (int32_t)d;
            const dim3 g((unsigned)std::min<int64_t>(P->dp.n_tiles, (int64_t)P->cu_count));
            hipLaunchKernelGGL(direct_kernel(S.io.dev_in32 != nullptr && S.has_in, S.da.out32 != nullptr, S.nsub > 1, S.mode == Mode::Unit), g, dim3(kDirectThreads), direct_lds_bytes(P->direct_window), S.stream, S.da);
            if (sample) {
                HIPCHK(hipEventRecord(P->ev[2 * P->prof_brackets + 1], S.stream));
                P->ev_reaches.push_back(n * (std::min((d + 1) * K, S.T) - d * K));
                P->prof_samples += K;
                ++P->prof_brackets;
            }
            ++P->prof_launches;
            ++S.d_done;
            progressed = true;
        }
        const int64_t rows_routed = S.d_done >= S.n_tasks ? S.T : S.d_done * K;      // by the lanes
        const int64_t ticks_routed = rows_routed * S.nsub;
        S.rows_loaded = rows_routed;
        // The boundary series of a partitioned network becomes the records of the skeleton's ghosts that mirror the boundary reaches,
        // 128 tick-rows at a time (k_rec_in's batches), never ahead of the rows the lanes have routed: the ring's slots up to there are free.
        while (ghosts && S.ghost_batches < S.n_in_batches) {
            const int64_t need = std::min(kRecRows * (S.ghost_batches + 1), S.total);
            if (ghost_ready < need || need > ticks_routed || !slot_free(S, S.ghost_batches)) break;
            launch_ghost_permute(P, S.ghost_batches);
            ++S.ghost_batches;
            progressed = true;
        }
        const int64_t ghost_loaded = !ghosts || S.ghost_batches >= S.n_in_batches ? S.total : std::max<int64_t>(0, kRecRows * S.ghost_batches - 15);
        // The skeleton's launch j runs its tiles of level l (from 1) on macro-chunk j - l, KS ticks each: what they read -- the records the
        // lanes forwarded and the boundary records, ticks below j KS -- is there once the lanes have routed that many rows.
        while (skel && S.diag < S.n_diags) {
            const int64_t j = S.diag;
            if (S.d_done < S.n_tasks && j > S.d_done * per - 1) break;
            if (ghost_loaded < std::min(S.total, j * KS)) break;
            if (tile_diag_launches(P, TP, j)) {      // (an empty bracket would be counted as a launch of the skeleton)
                const int aux = aux_begin(P, 2, S.stream);
                int rc = launch_tile_diag(P, P->ks, S.ta, P->ks.coef, j, false);
                aux_end(P, aux, S.stream);      // before rc is looked at: rr_plan_profile_aux reads both events of every sample
                if (rc) return rc;
            }
            ++S.diag;
            progressed = true;
        }
        // rows the direct tiles have written, and of those the rows whose skeleton reaches are final too
        int64_t done = ticks_routed;      // in sub-steps
        if (skel) {
            const int64_t m_done = S.diag - levels;      // the tiles of the last level have finished macro-chunk diag - levels
            int64_t sk = S.diag >= S.n_diags ? S.total : (m_done >= 0 ? std::max<int64_t>(0, (m_done + 1) * KS - dmax) : 0);
            done = std::min(done, std::min(sk, S.total));
            while (S.out_batches < S.n_out_batches && done >= std::min(kRecRows * (S.out_batches + 1), S.total)) {
                RecPermArgs ra = rec_args(P, S.out_batches);
                ra.n = P->n_kholes; ra.colmeta = P->d_kholemeta; ra.cols = P->d_kholecol;
                ra.rows = RowView{S.io.dev_out, n, 0, (uint32_t)std::max<int64_t>(1, S.io.rows_out)}; ra.rows32 = S.io.dev_out32;
                ra.clamp = S.nsub > 1 ? 0 : 1;
                const int aux = aux_begin(P, 3, S.stream);
                if (P->n_kholes > 0) launch_rec_out(ra, S.nsub > 1, S.stream);
                aux_end(P, aux, S.stream);
                ++S.out_batches;
                S.ticks_stored = std::min(S.total, kRecRows * S.out_batches);
                progressed = true;
            }
            S.rows_stored = S.ticks_stored / S.nsub;
        } else {
            S.ticks_stored = done; S.rows_stored = done / S.nsub;
        }
        if (!progressed) break;
    }
    if (S.d_done >= S.n_tasks && S.diag >= S.n_diags) S.tau = S.total_ticks;
    if (export_ready) {      // a lane's export is final with its row; a skeleton reach's once its tile's level has passed the tick
        int64_t e = S.d_done >= S.n_tasks ? S.total : S.d_done * Kt;
        if (S.export_skel) e = std::min(e, S.diag >= S.n_diags ? S.total : S.diag * KS - S.export_skew);
        *export_ready = P->n_export > 0 ? std::max<int64_t>(0, std::min(e, S.total)) : S.total;
    }
    return RR_OK;
}

// Runs every tick whose inputs are present: lateral rows [0, rows_ready) and ghost sub-steps [0, ghost_ready).
// On return *export_ready = number of leading sub-steps of the export series that are final.
int session_advance(rr_plan *P, int64_t rows_ready, int64_t ghost_ready, int64_t *export_ready)
{
    Session &S = P->ses;
    if (!S.open) return fail(RR_E_STATE, "no routing call is open on this plan");
    const int64_t n = P->h.n, dmax = P->h.depth - 1, C = std::max<int64_t>(1, P->chunk_rows);
    if (export_ready) *export_ready = 0;
    if (n == 0 || S.total == 0) { if (export_ready) *export_ready = S.total; return RR_OK; }
    if (S.kernel == Kernel::Tile) return session_advance_tile(P, rows_ready, std::min(ghost_ready, S.total), export_ready);
    if (S.kernel == Kernel::Direct) return session_advance_direct(P, rows_ready, std::min(ghost_ready, S.total), export_ready);
    rows_ready = std::min(rows_ready, S.T);
    ghost_ready = std::min(ghost_ready, S.total);
    // a ghost at lag L is read at tick tau for sub-step tau - L: ticks below ghost_ready + min lag are safe
    const int64_t ghost_limit = (P->n_ghost == 0 || ghost_ready >= S.total) ? S.total_ticks
                                                                            : ghost_ready + P->ghost_min_lag;
    for (;;) {
        bool progressed = false;
        if (S.has_in && S.rows_loaded < rows_ready) {
            const int64_t r1 = std::min(rows_ready, S.rows_loaded + C);
            int rc = session_load_rows(P, S.rows_loaded, r1);
            if (rc) return rc;
            S.rows_loaded = r1;
            progressed = true;
        }
        const int64_t have_rows = S.has_in ? S.rows_loaded : rows_ready;
        const int64_t lat_limit = have_rows < S.T ? have_rows * S.nsub : S.total_ticks;
        // without lateral rows to pace the loop, run the ticks in chunk-sized batches so finished rows leave the ring
        const int64_t batch_limit = S.has_in ? S.total_ticks : S.tau + C * S.nsub;
        const int64_t tau_end = std::min(std::min(lat_limit, ghost_limit), std::min(batch_limit, S.total_ticks));
        for (; S.tau < tau_end; ++S.tau) {
            int rc = session_launch_tick(P, S.tau);
            if (rc) return rc;
            progressed = true;
        }
        // row t is final once the outlet-most reaches passed it: tick (t+1)*nsub - 1 + dmax
        int64_t done = S.tau >= S.total_ticks ? S.T : (S.tau - dmax < 0 ? 0 : (S.tau - dmax) / S.nsub);
        done = std::min(done, S.T);
        if (done > S.rows_stored) {
            int rc = session_store_rows(P, S.rows_stored, done);
            if (rc) return rc;
            S.rows_stored = done;
            progressed = true;
        }
        if (!progressed) break;
    }
    if (export_ready) {
        const int64_t e = S.tau >= S.total_ticks ? S.total : S.tau - P->export_max_lag;
        *export_ready = std::max<int64_t>(0, std::min(e, S.total));
    }
    return RR_OK;
}

int session_end(rr_plan *P)
{
    Session &S = P->ses;
    if (!S.open) return fail(RR_E_STATE, "no routing call is open on this plan");
    const bool complete = P->h.n == 0 || S.total == 0 || (S.tau >= S.total_ticks && S.rows_stored >= S.T);
    S.open = false;
    if (!complete && getenv("RR_VERBOSE"))
        fprintf(stderr, "rr: incomplete call: T=%lld total=%lld tau=%lld/%lld rows_loaded=%lld rows_stored=%lld | direct=%d tasks %lld/%lld diag %lld/%lld in_batches %lld ghost_batches %lld/%lld out_batches %lld/%lld "
                        "ticks_stored=%lld K=%lld KS=%lld chunks=%lld macro=%lld\n", (long long)S.T, (long long)S.total, (long long)S.tau, (long long)S.total_ticks, (long long)S.rows_loaded, (long long)S.rows_stored,
                (int)(S.kernel == Kernel::Direct), (long long)S.d_done, (long long)S.n_tasks, (long long)S.diag, (long long)S.n_diags, (long long)S.in_batches, (long long)S.ghost_batches, (long long)S.n_in_batches,
                (long long)S.out_batches, (long long)S.n_out_batches, (long long)S.ticks_stored, (long long)(S.KC * kRec), (long long)(S.KS * kRec), (long long)S.rec_chunks, (long long)S.n_macro);
    if (!complete) return fail(RR_E_STATE, "routing call closed before all of its time steps were routed");
    if (P->h.n == 0 || S.total == 0) return RR_OK;
    if (S.bracket_open) P->prof_samples -= P->prof_samples % kSampleGroup;   // incomplete bracket: not counted
    HIPCHK(hipEventRecord(P->ev_last, S.stream));
    HIPCHK(hipGetLastError());
    return RR_OK;
}

// The whole call at once: what the reference's kernel boundary does.
int route_core(rr_plan *P, Mode mode, int64_t T, int64_t nsub, const Rows &io, hipStream_t stream)
{
    if (P->n_ghost > 0 || P->n_export > 0)
        return fail(RR_E_STATE, "plan has boundary reaches: use rr_stream_begin / rr_stream_advance / rr_stream_end");
    int rc = session_begin(P, mode, T, nsub, io, stream, nullptr, nullptr);
    if (rc) return rc;
    rc = session_advance(P, T, T * nsub, nullptr);
    if (rc) { P->ses.open = false; return rc; }
    return session_end(P);
}

int check_route_args(rr_plan *P, bool need_c4, int64_t T, int64_t nsub)
{
    int rc = need_device(P);
    if (rc) return rc;
    if (!P->coeffs_set) return fail(RR_E_STATE, "route called before rr_plan_set_coeffs");
    if (!P->boundary_whole) return fail(RR_E_STATE, "route called after a failed rr_plan_set_boundary: repeat that call first");
    if (need_c4 && !P->has_c4) return fail(RR_E_STATE, "rr_rapid_route needs c4_dt (rr_plan_set_coeffs got NULL)");
    if (T < 0 || nsub < 1) return fail(RR_E_INVALID, "route: need num steps >= 0 and sub-steps >= 1");
    if (nsub > 0x7FFFFFFF) return fail(RR_E_INVALID, "route: too many sub-steps");
    return RR_OK;
}

int launch_state_in(rr_plan *P, const double *d_q, hipStream_t stream)
{
    const int64_t n = P->h.n;
    if (P->sch.kernel != Kernel::Tick) {      // positions and ghosts as k_tile wants them (direct row path: the skeleton's; the lanes carry their discharge in params order)
        const bool d = P->sch.kernel == Kernel::Direct;
        const TileSet &ts = tiles_of(P, P->sch.kernel);
        const int64_t np = ts.tp->np;
        if (d) HIPCHK(hipMemcpyAsync(P->d_dq, d_q, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, stream));
        if (!d && P->hw_inpass) HIPCHK(hipMemcpyAsync(P->d_hwq, d_q, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, stream));      // k_rec_in's carry starts from the call's state
        if (np > 0)
            hipLaunchKernelGGL(k_tile_state_in, grid1(np), dim3(kBlock), 0, stream, ts.sq.get(), ts.ss.get(), ts.si.get(), d_q, ts.perm.get(), ts.pmeta.get(), (int32_t)np);
        return RR_OK;
    }
    hipLaunchKernelGGL(k_state_in, grid1(n), dim3(kBlock), 0, stream, P->d_x, P->d_x + n, P->d_x + 2 * n, d_q,
                       P->d_perm, (int32_t)n);
    return RR_OK;
}

void launch_state_out(rr_plan *P, double *d_q, int64_t total, hipStream_t stream)
{
    const int64_t n = P->h.n;
    if (P->sch.kernel == Kernel::Direct) {
        (void)hipMemcpyAsync(d_q, P->d_dq, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, stream);
        launch_skel_state_out(P->ks, d_q, P->ks.sq, stream);
        return;
    }
    if (P->sch.kernel == Kernel::Tile) {
        hipLaunchKernelGGL(k_tile_state_out, grid1(n), dim3(kBlock), 0, stream, d_q, (const double *)P->ts.sq, P->d_tinv,
                           (int32_t)n);
        return;
    }
    hipLaunchKernelGGL(k_state_out, grid1(n), dim3(kBlock), 0, stream, d_q, (const double *)P->d_x, n,
                       P->d_lag, P->d_inv, (int32_t)n, total);
}

void parallel_copy(double *dst, const double *src, size_t count, int threads, std::vector<std::thread> &pool)
{
    const size_t per = ((count + threads - 1) / threads + 511) / 512 * 512;
    for (int t = 0; t < threads; ++t) {
        const size_t o = (size_t)t * per;
        if (o >= count) break;
        pool.emplace_back([=] { std::memcpy(dst + o, src + o, std::min(per, count - o) * sizeof(double)); });
    }
}

int host_pipe_prepare(rr_plan *P)
{
    HostPipe &H = P->pipe;
    const int64_t n = P->h.n;
    // chunks of about half a gigabyte: long enough for the DMA engines to reach their rate, short enough to pipeline
    H.chunk_rows = std::max<int64_t>(16, std::min<int64_t>(4096, ((H.chunk_mib << 20) / (n * 8) + 15) / 16 * 16));
    if (n * 8 * 64 <= (int64_t{1} << 30)) H.chunk_rows = std::max<int64_t>(H.chunk_rows, 64);
    H.ring_chunks = std::max<int64_t>(8, (2 * kRecRows + 15) / H.chunk_rows + 6);      // a batch of rows + its 15-row overlap stays readable
    const int64_t pin_need = H.chunk_rows * n, dev_need = H.ring_chunks * H.chunk_rows * n;
    if (H.pin_cap < pin_need || H.dev_in.count() < dev_need) {
        H.destroy();
        for (int k = 0; k < HostPipe::kPinned; ++k) {
            if (hipHostMalloc((void **)&H.pin_in[k], (size_t)pin_need * 8, hipHostMallocDefault) != hipSuccess ||
                hipHostMalloc((void **)&H.pin_out[k], (size_t)pin_need * 8, hipHostMallocDefault) != hipSuccess) {
                (void)hipGetLastError(); H.destroy();
                return fail(RR_E_ALLOC, "host pipeline: pinned staging buffers could not be allocated");
            }
        }
        if (H.dev_in.alloc(dev_need) != RR_OK || H.dev_out.alloc(dev_need) != RR_OK) {
            (void)hipGetLastError(); H.destroy();
            return fail(RR_E_ALLOC, "host pipeline: device staging rings could not be allocated");
        }
        H.pin_cap = pin_need;
    }
    if (!H.s_h2d) { HIPCHK(hipStreamCreateWithFlags(&H.s_h2d, hipStreamNonBlocking)); HIPCHK(hipStreamCreateWithFlags(&H.s_d2h, hipStreamNonBlocking)); }
    return RR_OK;
}

// Routes T rows between host arrays (host_in may be NULL: channel-only) through the pipeline above.  State arrays are
// already on the device and the tile state is loaded; returns when host_out is complete.
int route_host_pipelined(rr_plan *P, Mode mode, int64_t T, int64_t nsub, const double *host_in, double *host_out, hipStream_t stream)
{
    int rc = host_pipe_prepare(P);
    if (rc) return rc;
    HostPipe &H = P->pipe;
    constexpr int kPinned = HostPipe::kPinned;
    const int64_t n = P->h.n, C = H.chunk_rows, NR = H.ring_chunks, nchunks = (T + C - 1) / C;
    auto grow = [&](std::vector<hipEvent_t> &v, size_t count) {
        while (v.size() < count) { hipEvent_t e; if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return false; v.push_back(e); }
        return true;
    };
    if (!grow(H.ev_h2d, (size_t)nchunks) || !grow(H.ev_d2h, (size_t)nchunks) || !grow(H.ev_adv, (size_t)4 * nchunks + 64))
        return fail(RR_E_HIP, "host pipeline: event creation failed");
    Rows io;
    io.dev_in = host_in ? H.dev_in : nullptr; io.rows_in = NR * C; io.dev_out = H.dev_out; io.rows_out = NR * C;
    rc = session_begin(P, mode, T, nsub, io, stream, nullptr, nullptr);
    if (rc) return rc;
    Session &S = P->ses;
    auto rows_of = [&](int64_t c) { return std::min(C, T - c * C); };
    std::vector<int64_t> adv_loaded;      // rows that were records after the a-th advance (ev_adv[a] marks it on the stream)
    int64_t filled = 0, h2d_issued = 0, d2h_issued = 0, copied_out = 0;      // chunks through each stage
    std::vector<std::thread> pool;
    auto bail = [&](int code, const std::string &msg) {
        for (auto &t : pool) t.join();
        (void)hipStreamSynchronize(H.s_h2d); (void)hipStreamSynchronize(H.s_d2h); (void)hipStreamSynchronize(stream);
        P->ses.open = false;
        return fail(code, msg);
    };
#define RR_PIPE(expr) do { hipError_t e__ = (expr); if (e__ != hipSuccess) return bail(RR_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e__)); } while (0)
    // One iteration: the copy threads fill the next pinned input chunk and empty the oldest downloaded output chunk while
    // this thread enqueues the upload of the chunk filled last time, the routing it enables and the downloads it completes.
    double t_join = 0.0, t_wait = 0.0;      // RR_VERBOSE: seconds this thread waited for the copy threads / for events
    auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    while (copied_out < nchunks) {
        pool.clear();
        bool progressed = false;
        const bool fill = host_in && filled < nchunks && filled < h2d_issued + kPinned;
        if (fill) {
            if (filled >= kPinned) { const double t0 = now(); RR_PIPE(hipEventSynchronize(H.ev_h2d[filled - kPinned])); t_wait += now() - t0; }      // the buffer's previous chunk has left
            parallel_copy(H.pin_in[filled % kPinned], host_in + filled * C * n, (size_t)(rows_of(filled) * n), H.copy_threads, pool);
        }
        bool empty = false;
        if (copied_out < d2h_issued) {      // only a download that HAS arrived: waiting for one here would stall the uploads behind it
            const hipError_t q = hipEventQuery(H.ev_d2h[copied_out]);
            if (q == hipSuccess) empty = true;
            else if (q != hipErrorNotReady) return bail(RR_E_HIP, std::string("hipEventQuery: ") + hipGetErrorString(q));
        }
        if (empty) {
            parallel_copy(host_out + copied_out * C * n, H.pin_out[copied_out % kPinned], (size_t)(rows_of(copied_out) * n), H.copy_threads, pool);
        }
        // upload of a chunk filled earlier, into the ring slot whose previous occupant has become records
        if (host_in && h2d_issued < filled) {
            const int64_t c = h2d_issued;
            bool slot_ready = true;
            if (c >= NR) {
                const int64_t need = std::min(T, (c - NR + 1) * C);
                size_t a = 0;
                while (a < adv_loaded.size() && adv_loaded[a] < need) ++a;
                if (a < adv_loaded.size()) RR_PIPE(hipStreamWaitEvent(H.s_h2d, H.ev_adv[a], 0));
                else slot_ready = false;      // the routing has to get further first (see the advance below)
            }
            if (slot_ready) {
                RR_PIPE(hipMemcpyAsync(H.dev_in + (c % NR) * C * n, H.pin_in[c % kPinned], (size_t)(rows_of(c) * n) * 8, hipMemcpyHostToDevice, H.s_h2d));
                RR_PIPE(hipEventRecord(H.ev_h2d[c], H.s_h2d));
                RR_PIPE(hipStreamWaitEvent(stream, H.ev_h2d[c], 0));
                ++h2d_issued;
                progressed = true;
            }
        }
        // route what has arrived; output rows land in the device ring at row % (NR * C), so no batch may be written before
        // the rows it overwrites are on their way to the host
        if (S.tau < S.total_ticks || S.rows_stored < T) {
            const int64_t ready = host_in ? std::min(T, h2d_issued * C) : T;
            S.out_limit = std::min(T, d2h_issued * C) + NR * C;
            if (d2h_issued > 0) RR_PIPE(hipStreamWaitEvent(stream, H.ev_d2h[d2h_issued - 1], 0));
            const int64_t before_diag = S.diag, before_in = S.in_batches, before_out = S.out_batches;
            rc = session_advance(P, ready, S.total, nullptr);
            if (rc) { for (auto &t : pool) t.join(); P->ses.open = false; return rc; }
            if (S.diag != before_diag || S.in_batches != before_in || S.out_batches != before_out) {
                progressed = true;
                if (adv_loaded.size() < H.ev_adv.size() - 1) {
                    RR_PIPE(hipEventRecord(H.ev_adv[adv_loaded.size()], stream));
                    adv_loaded.push_back(S.rows_loaded);
                }
            }
        }
        // downloads of the output chunks that are complete; a pinned buffer is free once the copy threads have emptied it
        while (d2h_issued < nchunks && std::min(T, (d2h_issued + 1) * C) <= S.rows_stored && d2h_issued < copied_out + kPinned) {
            const int64_t k = d2h_issued;
            RR_PIPE(hipEventRecord(H.ev_adv.back(), stream));      // everything enqueued so far on the routing stream
            RR_PIPE(hipStreamWaitEvent(H.s_d2h, H.ev_adv.back(), 0));
            RR_PIPE(hipMemcpyAsync(H.pin_out[k % kPinned], H.dev_out + (k % NR) * C * n, (size_t)(rows_of(k) * n) * 8, hipMemcpyDeviceToHost, H.s_d2h));
            RR_PIPE(hipEventRecord(H.ev_d2h[k], H.s_d2h));
            ++d2h_issued;
            progressed = true;
        }
        { const double t0 = now(); for (auto &t : pool) t.join(); t_join += now() - t0; }
        if (fill) ++filled;
        if (empty) ++copied_out;
        if (!progressed && !fill && !empty) {
            if (copied_out < d2h_issued) { const double t0 = now(); RR_PIPE(hipEventSynchronize(H.ev_d2h[copied_out])); t_wait += now() - t0; }      // nothing else to do but wait for it
            else return bail(RR_E_STATE, "host pipeline: no stage can make progress");
        }
    }
#undef RR_PIPE
    if (getenv("RR_VERBOSE"))
        fprintf(stderr, "rr: host pipeline: %lld chunks of %lld rows, %d copy threads per direction; waited %.1f ms for the copy threads, %.1f ms for transfers\n",
                (long long)nchunks, (long long)C, H.copy_threads, t_join * 1e3, t_wait * 1e3);
    S.out_limit = std::numeric_limits<int64_t>::max();
    return session_end(P);
}

// Host rows on the time-tiled kernel go through the PCIe pipeline; every other call is one session (route_core).
int route_rows(rr_plan *P, Mode mode, int64_t T, int64_t nsub, const Rows &io, hipStream_t stream)
{
    if ((io.host_in || io.host_out) && P->sch.kernel == Kernel::Tile) return route_host_pipelined(P, mode, T, nsub, io.host_in, io.host_out, stream);
    return route_core(P, mode, T, nsub, io, stream);
}

// The state arrays of a route call: device arrays as given, or (on_host: the host-pointer entry points) staged in one device buffer
// for the call, `count` doubles each; out() copies them back.
struct CallState {
    std::vector<double *> host, dev;
    DevBuf<double> tmp;
    int64_t count = 0;
    hipStream_t stream = nullptr;
    int in(bool on_host, std::vector<double *> arrays, int64_t count_, hipStream_t stream_)
    {
        host = dev = arrays; count = count_; stream = stream_;
        const int64_t each = std::max<int64_t>(count, 1);
        if (!on_host) return RR_OK;
        if (int rc = tmp.alloc((int64_t)host.size() * each)) return rc;
        hipError_t e = hipSuccess;
        for (size_t i = 0; i < host.size() && e == hipSuccess; ++i)
            e = hipMemcpyAsync(dev[i] = tmp + i * each, host[i], count * sizeof(double), hipMemcpyHostToDevice, stream);
        return e == hipSuccess ? RR_OK : fail(RR_E_HIP, hipGetErrorString(e));
    }
    int out()
    {
        hipError_t e = hipSuccess;
        for (size_t i = 0; tmp && i < host.size() && e == hipSuccess; ++i) e = hipMemcpyAsync(host[i], dev[i], count * sizeof(double), hipMemcpyDeviceToHost, stream);
        if (tmp && e == hipSuccess) e = hipStreamSynchronize(stream);
        return e == hipSuccess ? RR_OK : fail(RR_E_HIP, hipGetErrorString(e));
    }
    ~CallState() { if (tmp) (void)hipStreamSynchronize(stream); }      // (before tmp goes)
};

// RapidMuskingum / channel-only Muskingum.  `who` names the entry point in the errors of prepare_call.
int rapid_like(rr_plan *P, Mode mode, double *q_t, const Rows &io, int64_t T, int64_t nsub, hipStream_t stream, bool q_on_host, const char *who)
{
    if (P->h.n == 0 || T == 0) return RR_OK;
    int rc = prepare_call(P, call_shape(mode, T, nsub, io), who);
    CallState q;
    if (!rc) rc = q.in(q_on_host, {q_t}, P->h.n, stream);
    if (!rc) rc = launch_state_in(P, q.dev[0], stream);
    if (!rc) rc = route_rows(P, mode, T, nsub, io, stream);
    if (!rc) {
        launch_state_out(P, q.dev[0], T * nsub, stream);
        rc = q.out();
    }
    return rc;
}

// UnitMuskingum state (channel discharge and full discharge of the reaches that have upstream reaches) into the layout of the
// kernel this call runs, and back.
int unit_state_in(rr_plan *P, const double *d_qch, const double *d_qfull, hipStream_t stream)
{
    const int64_t n = P->h.n, ni = (int64_t)P->h.inner_pos.size();
    hipError_t e0 = hipSuccess;
    if (P->sch.kernel != Kernel::Tick) {
        // q_full / q_ch scattered to params order (zeros on headwaters: the direct row path's lanes carry them so), then gathered position by
        // position as k_tile<UNIT> wants them (on the direct row path: the skeleton's positions)
        const TileSet &ts = tiles_of(P, P->sch.kernel);
        const int64_t np = ts.tp->np;
        e0 = hipMemsetAsync(P->d_full, 0, n * sizeof(double), stream);
        if (e0 == hipSuccess) e0 = hipMemsetAsync(P->d_chan, 0, n * sizeof(double), stream);
        if (e0 == hipSuccess && ni > 0)
            hipLaunchKernelGGL(k_unit_scatter, grid1(ni), dim3(kBlock), 0, stream, P->d_full, P->d_chan, d_qfull, d_qch, P->d_inner_idx, (int32_t)ni);
        if (e0 == hipSuccess && np > 0)
            hipLaunchKernelGGL(k_tile_unit_state_in, grid1(np), dim3(kBlock), 0, stream, ts.sq.get(), ts.ss.get(), ts.si.get(), ts.sqch.get(),
                               (const double *)P->d_full, (const double *)P->d_chan, ts.perm.get(), ts.pmeta.get(), (int32_t)np);
    } else {
        e0 = hipMemsetAsync(P->d_x, 0, 3 * n * sizeof(double), stream);
        if (e0 == hipSuccess && ni > 0)
            hipLaunchKernelGGL(k_unit_state_in, grid1(ni), dim3(kBlock), 0, stream, P->d_x, P->d_x + n, P->d_x + 2 * n,
                               P->d_qch, d_qch, d_qfull, P->d_inner_pos, (int32_t)ni);
    }
    return e0 == hipSuccess ? RR_OK : fail(RR_E_HIP, hipGetErrorString(e0));
}

void unit_state_out(rr_plan *P, double *d_qch, double *d_qfull, int64_t total, hipStream_t stream)
{
    const int64_t n = P->h.n, ni = (int64_t)P->h.inner_pos.size();
    if (ni == 0) return;
    if (P->sch.kernel == Kernel::Direct) {      // the skeleton's reaches back into the params-order arrays the lanes kept, then the inner reaches' pairs
        launch_skel_state_out(P->ks, P->d_full, P->ks.sq, stream);
        launch_skel_state_out(P->ks, P->d_chan, P->ks.sqch, stream);
        hipLaunchKernelGGL(k_unit_gather, grid1(ni), dim3(kBlock), 0, stream, d_qch, d_qfull, (const double *)P->d_chan, (const double *)P->d_full, P->d_inner_idx, (int32_t)ni);
    } else if (P->sch.kernel == Kernel::Tile)
        hipLaunchKernelGGL(k_tile_unit_state_out, grid1(ni), dim3(kBlock), 0, stream, d_qch, d_qfull,
                           (const double *)P->ts.sq, (const double *)P->ts.sqch, P->d_inner_idx, P->d_tinv, (int32_t)ni);
    else
        hipLaunchKernelGGL(k_unit_state_out, grid1(ni), dim3(kBlock), 0, stream, d_qch, d_qfull,
                           (const double *)P->d_x, n, (const double *)P->d_qch, P->d_lag, P->d_inner_pos, (int32_t)ni, total);
}

// Carry-over state of the unit-hydrograph convolution, in place, enqueued after every pass that reads the old one (same stream).
template <typename TIn> using uh_tail_t = void (*)(const double *, double *, const TIn *, int64_t, int32_t, int64_t, uint32_t);
template <typename TIn>
uh_tail_t<TIn> uh_tail_kernel(int64_t n_ks)      // (0: any number of taps, from memory)
{
    return n_ks <= 16 ? (uh_tail_t<TIn>)k_uh_tail<16, TIn> : (n_ks <= 48 ? (uh_tail_t<TIn>)k_uh_tail<48, TIn> : (uh_tail_t<TIn>)k_uh_tail<0, TIn>);
}
template <typename TIn>
void launch_uh_tail(const double *kernel, double *state, const TIn *rows, int64_t T, int64_t n_ks, int64_t n, hipStream_t stream, uint32_t sel)
{
    hipLaunchKernelGGL(uh_tail_kernel<TIn>(n_ks), dim3((unsigned)((n + kUhTailThreads - 1) / kUhTailThreads)), dim3(kUhTailThreads), 0, stream, kernel, state, rows, T, (int32_t)n_ks, n, sel);
}

template <typename TIn>
int uh_convolve_core(const double *d_kernel, double *d_state, const TIn *d_lateral, double *d_out, int64_t T, int64_t n_ks, int64_t n, hipStream_t stream, uint32_t sel);

// UnitMuskingum.  `who` names the entry point in the errors of prepare_call.
int unit_like(rr_plan *P, double *q_ch, double *q_full, const Rows &io_in, int64_t T, int64_t nsub, hipStream_t stream, bool q_on_host,
              const char *who, double *d_q_final = nullptr, double *uh_state_inout = nullptr)
{
    const int64_t n = P->h.n, ni = (int64_t)P->h.inner_pos.size();
    if (n == 0 || T == 0) return RR_OK;
    Rows io = io_in;
    int rc = prepare_call(P, call_shape(Mode::Unit, T, nsub, io), who);
    const Kernel kernel = P->sch.kernel;
    const uint32_t sel32 = P->in32_big_endian ? kSelSwap : kSelNative;
    CallState q;
    if (!rc) rc = q.in(q_on_host, {q_ch, q_full}, ni, stream);
    if (!rc) rc = unit_state_in(P, q.dev[0], q.dev[1], stream);
    if (!rc && kernel == Kernel::Direct && io.uh_kernel) {
        // the direct row path: the convolution first, into the work rows (choose_schedule: uh), carry-over state updated in place;
        // the lanes then route those rows
        if (T * n > P->d_mrows.count()) rc = fail(RR_E_STATE, "route: the convolved rows of the direct row path were not reserved");
        else if (io.dev_in32) rc = uh_convolve_core<float>(io.uh_kernel, uh_state_inout, io.dev_in32, P->d_mrows, T, io.uh_nks, n, stream, sel32);
        else rc = uh_convolve_core<double>(io.uh_kernel, uh_state_inout, io.dev_in, P->d_mrows, T, io.uh_nks, n, stream, kSelNative);
        io.dev_in = P->d_mrows; io.dev_in32 = nullptr; io.rows_in = T; io.uh_kernel = nullptr; io.uh_state = nullptr;
    }
    if (!rc) rc = route_rows(P, Mode::Unit, T, nsub, io, stream);
    if (!rc && kernel == Kernel::Tile && d_q_final)      // every reach: a headwater's state is its last lateral inflow, an inner reach's q_full
        hipLaunchKernelGGL(k_tile_state_out, grid1(n), dim3(kBlock), 0, stream, d_q_final, (const double *)P->ts.sq, P->d_tinv, (int32_t)n);
    if (!rc && kernel == Kernel::Direct && d_q_final) {      // the lanes' columns hold exactly that; the skeleton's reaches join them
        launch_skel_state_out(P->ks, P->d_full, P->ks.sq, stream);
        (void)hipMemcpyAsync(d_q_final, P->d_full, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, stream);
    }
    if (!rc && io.uh_kernel && uh_state_inout) {      // carry-over state of the fused convolution, after every batch has read the old one
        if (io.dev_in32) launch_uh_tail<float>(io.uh_kernel, uh_state_inout, io.dev_in32, T, io.uh_nks, n, stream, sel32);
        else launch_uh_tail<double>(io.uh_kernel, uh_state_inout, io.dev_in, T, io.uh_nks, n, stream, kSelNative);
    }
    if (!rc && ni > 0) {
        unit_state_out(P, q.dev[0], q.dev[1], T * nsub, stream);
        rc = q.out();
    }
    return rc;
}

template <typename TIn>
int uh_convolve_core(const double *d_kernel, double *d_state, const TIn *d_lateral, double *d_out, int64_t T,
                     int64_t n_ks, int64_t n, hipStream_t stream, uint32_t sel)
{
    if (T < 1 || n_ks < 1 || n < 0) return fail(RR_E_INVALID, "rr_uh_convolve: need T >= 1, n_ks >= 1, n >= 0");
    if (n == 0) return RR_OK;
    if (n_ks > 0x7FFFFFFF || T > 0x7FFFFFFFLL * 8) return fail(RR_E_INVALID, "rr_uh_convolve: sizes out of range");
    constexpr int TB = 8;
    if (n_ks <= 57 && T >= 64) {
        // long series: register-resident taps + LDS window; split time only as far as needed to fill the chip
        const int64_t blocks_x = (n + kUhThreads - 1) / kUhThreads;
        int64_t segs = std::max<int64_t>(1, std::min<int64_t>(T / 256, (2048 + blocks_x - 1) / blocks_x));
        const int64_t seg_rows = ((T + segs - 1) / segs + 63) / 64 * 64;      // segments start at multiples of every NK
        segs = (T + seg_rows - 1) / seg_rows;
        dim3 g((unsigned)blocks_x, (unsigned)segs);
#define RR_UH_LAUNCH(NK_, NT_, R_, D_)                                                                             \
        do {                                                                                                       \
            const size_t lds = (size_t)NK_ * kUhThreads * sizeof(double);                                          \
            (void)hipFuncSetAttribute((const void *)k_uh_convolve_ring<NK_, NT_, R_, D_, TIn>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
            hipLaunchKernelGGL((k_uh_convolve_ring<NK_, NT_, R_, D_, TIn>), g, dim3(kUhThreads), lds, stream, d_kernel, (const double *)d_state,     \
                               d_lateral, d_out, T, (int32_t)n_ks, n, seg_rows, sel);                              \
        } while (0)
        if (n_ks <= 5) RR_UH_LAUNCH(8, 5, 4, 2);            // NK >= NT + R - 1 window slots
        else if (n_ks <= 13) RR_UH_LAUNCH(16, 13, 4, 2);
        else if (n_ks <= 24) RR_UH_LAUNCH(32, 24, 8, 2);
        else if (n_ks <= 29) RR_UH_LAUNCH(32, 29, 4, 2);
        else if (n_ks <= 48) RR_UH_LAUNCH(64, 48, 8, 2);
        else RR_UH_LAUNCH(64, 57, 8, 2);
#undef RR_UH_LAUNCH
    } else {
        dim3 g((unsigned)((n + kBlock - 1) / kBlock), (unsigned)((T + TB - 1) / TB));
        hipLaunchKernelGGL((k_uh_convolve<TB, TIn>), g, dim3(kBlock), 0, stream, d_kernel, (const double *)d_state, d_lateral,
                           d_out, T, (int32_t)n_ks, n, sel);
    }
    // carry-over state, in place, after the rows above have read the old one (same stream)
    launch_uh_tail<TIn>(d_kernel, d_state, d_lateral, T, n_ks, n, stream, sel);
    HIPCHK(hipGetLastError());
    return RR_OK;
}

}  // namespace
