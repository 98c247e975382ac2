// rr_engine.hip -- gfx950 kernels, the streaming executor and the C ABI of librr_hip.so.
//
// The math (river_route/routers/_numba_kernels.py:63-84 in gather form):
//   q+[i] = c3[i] q[i] + c4dt[i] ql[t,i] + c2[i] * sum_{u in up(i)} q[u] + sum_{u in up(i)} c1[i] q+[u]
// The second sum is a sparse triangular solve down the river tree.  Instead of sweeping the tree level by
// level inside one time step, the engine PIPELINES time down the tree: at routing tick tau the reach at
// engine position p advances its own sub-step  ts = tau - lag[p]  (lag = levels between p and the farthest
// headwater of the whole network).  Because lag(down) = lag(up) + 1 on every edge, the upstream values a
// reach needs -- q+[u] at ts and q[u] at ts-1 -- are exactly what its upstream reaches wrote one and two
// ticks ago.  Every tick is therefore one dependency-free, fully coalesced streaming kernel over all
// reaches; there are T*nsub + depth - 1 ticks in a call.  State lives in three rotating buffers X[tau % 3].
//
// Layout: rr_plan.hpp.  No CPU fallback anywhere in this file.
//
// The routing translation unit: the plan and everything that works on one, the runoff and unit-hydrograph calls that share its
// kernels' headers, and the device helpers of the C ABI.  In this order: rr_common.hpp
// (constants, index helpers), rr_kernels_tick.hpp, rr_kernels_tile.hpp, rr_kernels_uh.hpp, rr_kernels_rec.hpp, rr_kernels_runoff.hpp,
// rr_kernels_direct.hpp, rr_kernels_adjoint.hpp, rr_kernels_adjoint_unit.hpp (device code), rr_exec.hpp (plan object, executor),
// then the C ABI below; rr_adjoint.hpp (the adjoints' host side) and rr_kernels_runoff_adjoint.hpp (the adjoint of the
// gridded-runoff inflow, device code) are included where their entry points are.  The skill scores, their adjoint and the overlap
// areas take a device index and no plan: they are rr_scores.hip, a translation unit and a code object of their own, so this
// unit's code object does not notice what happens to them.
#include "rr_common.hpp"
#include "rr_kernels_tick.hpp"
#include "rr_kernels_tile.hpp"
#include "rr_kernels_uh.hpp"
#include "rr_kernels_rec.hpp"
#include "rr_kernels_runoff.hpp"
#include "rr_kernels_direct.hpp"
#include "rr_kernels_adjoint.hpp"
#include "rr_kernels_adjoint_unit.hpp"
#include "rr_exec.hpp"

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------

static thread_local std::string g_err;      // what rr::fail (rr_common.hpp) sets, in whichever translation unit, and rr_last_error reads

int rr::fail(int code, const std::string &msg) { g_err = msg; return code; }

extern "C" {

int rr_version(void) { return RR_VERSION_NUM; }

const char *rr_last_error(void) { return g_err.c_str(); }

int rr_device_count(void)
{
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess) return 0;
    return c;
}

void rr_plan_destroy(rr_plan *P)
{
    if (!P) return;
    if (P->device >= 0 && hipSetDevice(P->device) == hipSuccess) {      // (the device arrays go with the plan: they are DevBufs)
        P->pipe.destroy();
        for (hipEvent_t e : P->ev) (void)hipEventDestroy(e);
        for (hipEvent_t e : P->aux_ev) (void)hipEventDestroy(e);
        if (P->ev_first) (void)hipEventDestroy(P->ev_first);
        if (P->ev_last) (void)hipEventDestroy(P->ev_last);
    }
    delete P;
}

int rr_plan_create(int64_t n, const int32_t *csc_indptr, const int32_t *csc_indices, int device, rr_plan **out)
{
    if (!out) return fail(RR_E_INVALID, "rr_plan_create: null out");
    *out = nullptr;
    rr_plan *P = new (std::nothrow) rr_plan();
    if (!P) return fail(RR_E_ALLOC, "rr_plan_create: out of memory");
    // Run-time switches, all for tests (each is exercised by tests/test_gpu_*.py): RR_WAVE=0 the streaming kernel for every call,
    // =1 the time-tiled one wherever it applies; RR_WAVE_K ticks per task; RR_TILE_BLOCK tile capacity (many small tiles);
    // RR_TILE_LEAN=0 the general tick; RR_UH_PAIRS=0 one record batch per fused-convolution launch; RR_REC_BATCHES=N N record batches
    // per launch of k_rec_in / k_rec_out in every call (1: one, as before multi-batch launches); RR_DIRECT=0 records also where the
    // params order would allow the direct row path; RR_HW_INPASS=0 headwaters routed and stored by k_tile, as every other reach; RR_VERBOSE=1
    // logs the schedule; RR_ALLOC_FAIL_AT=k the k-th device allocation the process makes from here on, whoever makes it, is refused once
    // (as the device refuses one: RR_E_ALLOC, NULL; the message says "(injected)").
    if (const char *e = getenv("RR_HW_INPASS")) P->hw_inpass = atoi(e) != 0;
    if (const char *e = getenv("RR_ALLOC_FAIL_AT")) rr::g_dev_fail_in = std::max(0, atoi(e));
    if (const char *e = getenv("RR_WAVE")) { P->wave_enabled = atoi(e) != 0; P->wave_forced = atoi(e) == 1; }
    if (const char *e = getenv("RR_REC_BATCHES")) { P->rec_batches = std::max(1, std::min(kRecMaxLaunchBatches, atoi(e))); P->rec_batches_forced = true; }
    if (const char *e = getenv("RR_WAVE_K")) P->wave_K = std::max(kRec, atoi(e) / kRec * kRec);
    std::string err;
    int rc = rr::build_host_plan(n, csc_indptr, csc_indices, P->h, err);
    if (rc) { delete P; return fail(rc, err); }
    if (device != RR_DEVICE_NONE) {      // the tile size below depends on the card's CU count
        int count = rr_device_count(), cus = 0;
        if (device >= 0 && device < count && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) P->cu_count = cus;
    }
    {   // Time-tiled schedule: one position per thread, tiles of at most kTileThreads positions (rr_exec.hpp: tile_kernel)
        P->wave_threads = kTileThreads;
        int32_t block = P->wave_threads;
        if (const char *e = getenv("RR_TILE_BLOCK")) block = std::max(8, std::min(block, atoi(e)));     // tests: many small tiles
        std::vector<int32_t> lag_of((size_t)n);
        for (int64_t i = 0; i < n; ++i) lag_of[i] = P->h.lag[P->h.inv[i]];
        rr::build_tile_plan(P->h.down, lag_of, block, P->tp);
        // the direct row path where the params order numbers small subtrees contiguously (any depth-first post-order); `why` says why not
        if (const char *e = getenv("RR_DIRECT")) P->direct_enabled = atoi(e) != 0;
        P->direct_block = block;
        rr::build_direct_plan(P->h.down, lag_of, std::min<int32_t>(kDirectLanes, block), kDirectMaxWindow - 2, block, P->dp);
        P->direct_window = 3;
        for (int32_t sp : P->dp.tile_span) P->direct_window = std::max(P->direct_window, sp + 3);
    }
    if (device != RR_DEVICE_NONE) {
        int count = rr_device_count();
        if (device < 0 || device >= count) {
            delete P;
            return fail(RR_E_NO_DEVICE, "rr_plan_create: HIP device " + std::to_string(device) + " not available (" +
                                            std::to_string(count) + " visible)");
        }
        hipError_t e = hipSetDevice(device);
        if (e != hipSuccess) { delete P; return fail(RR_E_HIP, hipGetErrorString(e)); }
        P->device = device;
        {
            size_t free_b = 0, total_b = 0;
            if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) P->dev_total_bytes = total_b;
        }
        if (const char *e2 = getenv("RR_TILE_LEAN")) P->lean_enabled = atoi(e2) != 0;
        for (int v = 0; v < 7; ++v)    // > 64 KiB of dynamic LDS needs an explicit opt-in per kernel (v = 4, 5, 6: the short ticks of Rapid, Unit, channel-only)
            if (hipFuncSetAttribute((const void *)tile_kernel(v < 4 ? (v & 1) != 0 : v == 5, v < 4 && (v & 2) != 0, v >= 4, v == 6), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)tile_lds_bytes(P->wave_threads)) != hipSuccess) {
                (void)hipGetLastError();
                P->wave_enabled = false;
            }
        for (int v = 0; v < 4; ++v)    // the same for the member-batched forms (ensembles; v = 2, 3: with a coefficient set per member)
            if (hipFuncSetAttribute((const void *)tile_ens_kernel((v & 1) != 0, v >= 2), hipFuncAttributeMaxDynamicSharedMemorySize, (int)tile_lds_bytes(kTileThreads)) != hipSuccess) {
                (void)hipGetLastError();
                P->ens_enabled = false;
            }
        if (const char *e2 = getenv("RR_UH_PAIRS")) P->uh_pairs = atoi(e2) != 0;
        for (int v = 0; v < 4; ++v)
            (void)hipFuncSetAttribute((const void *)rec_in_uh_kernel((v & 1) != 0, 64, 1 + (v >> 1)), hipFuncAttributeMaxDynamicSharedMemorySize, (int)rec_in_uh_lds_bytes(64, 1 + (v >> 1)));
        (void)hipGetLastError();
        const rr::HostPlan &H = P->h;
        const int64_t ni = (int64_t)H.inner_pos.size();
        rc = P->d_child_ptr.alloc(n + 1);      // (their uploads come last, as they always did: the order of a plan's allocations and uploads is kept)
        for (DevBuf<int32_t> *col : {&P->d_lag, &P->d_perm, &P->d_inv}) if (!rc) rc = col->alloc(n);
        if (!rc) rc = P->d_inner_pos.alloc(ni);
        if (!rc) rc = P->d_hwc.alloc(n);
        if (!rc) rc = P->d_bidx.alloc(n);
        if (!rc) rc = P->d_c4_params.alloc(n);
        if (!rc && P->tp.ok) {      // tile layout of the time-tiled kernel
            const rr::TilePlan &TP = P->tp;
            const int64_t np = TP.np;
            std::vector<int32_t> inner_idx;
            inner_idx.reserve(ni);
            for (int64_t i = 0; i < n; ++i) if (H.child_ptr[H.inv[i] + 1] > H.child_ptr[H.inv[i]]) inner_idx.push_back((int32_t)i);
            rc = assign(P->d_inner_idx, inner_idx);
            if (!rc) rc = upload_tile_meta(P, TP.lag, TP.xpos, TP.tile_flags);      // (and the column metadata of the record passes)
            if (!rc) rc = assign(P->ts.perm, TP.perm);
            if (!rc) rc = assign(P->d_tinv, TP.inv);
            for (DevBuf<double> *coef : {&P->ts.coef, &P->d_coef_unit, &P->d_coef_hw}) if (!rc) rc = coef->alloc(3 * np);
            if (!rc) rc = P->d_hwcoef.alloc(3 * n);
            if (!rc) rc = P->d_hwq.alloc(n);
            for (DevBuf<double> *state : {&P->ts.sq, &P->ts.ss, &P->ts.si, &P->ts.sqch}) if (!rc) rc = state->alloc(np);
            if (!rc) rc = P->d_full.alloc(n);
            if (!rc) rc = P->d_chan.alloc(n);
        }
        if (!rc) rc = upload_direct_plan(P);      // direct row path: per-column constants, the skeleton's tile arrays, the holes' out-pass
        for (DevBuf<double> *row : {&P->d_w, &P->d_c1row_h, &P->d_c2, &P->d_c3, &P->d_c4}) if (!rc) rc = row->alloc(n);
        if (!rc) rc = P->d_x.alloc(3 * n);
        if (!rc) rc = P->d_isum.alloc(n);
        if (!rc) rc = P->d_qch.alloc(n);
        if (!rc) rc = dev_upload(P->d_child_ptr, H.child_ptr);
        if (!rc) rc = dev_upload(P->d_lag, H.lag);
        if (!rc) rc = dev_upload(P->d_perm, H.perm);
        if (!rc) rc = dev_upload(P->d_inv, H.inv);
        if (!rc) rc = dev_upload(P->d_inner_pos, H.inner_pos);
        if (!rc) rc = dev_upload(P->d_hwc, H.hw_children);
        if (rc) { rr_plan_destroy(P); return rc; }
    }
    *out = P;
    return RR_OK;
}

int rr_plan_info(const rr_plan *P, int64_t info[8])
{
    if (!P || !info) return fail(RR_E_INVALID, "rr_plan_info: null argument");
    info[0] = P->h.n; info[1] = P->h.n_edges; info[2] = P->h.depth; info[3] = P->h.widest_level;
    info[4] = P->h.n_headwaters; info[5] = P->h.n_outlets; info[6] = P->h.identity ? 1 : 0; info[7] = P->device;
    return RR_OK;
}

int rr_plan_layout(const rr_plan *P, int32_t *perm, int32_t *lag, int32_t *child_ptr)
{
    if (!P) return fail(RR_E_INVALID, "rr_plan_layout: null plan");
    const size_t n = (size_t)P->h.n;
    if (perm && n) std::memcpy(perm, P->h.perm.data(), n * sizeof(int32_t));
    if (lag && n) std::memcpy(lag, P->h.lag.data(), n * sizeof(int32_t));
    if (child_ptr) std::memcpy(child_ptr, P->h.child_ptr.data(), (n + 1) * sizeof(int32_t));
    return RR_OK;
}

int rr_plan_tile_info(const rr_plan *P, int64_t info[8])
{
    if (!P || !info) return fail(RR_E_INVALID, "rr_plan_tile_info: null argument");
    const rr::TilePlan &T = P->tp;
    info[0] = T.ok ? 1 : 0; info[1] = T.block; info[2] = T.np; info[3] = T.n_ghost; info[4] = T.n_tiles; info[5] = T.n_levels;
    info[6] = P->wave_threads; info[7] = kRecRows;
    return RR_OK;
}

int rr_plan_inpass_info(const rr_plan *P, int64_t info[5])
{
    if (!P || !info) return fail(RR_E_INVALID, "rr_plan_inpass_info: null argument");
    for (int k = 0; k < 5; ++k) info[k] = 0;
    info[0] = P->hw_inpass ? 1 : 0;
    if (!P->tp.ok) return RR_OK;
    std::vector<int32_t> lag(P->tp.lag);      // with the boundary ghosts of a partitioned network, as rr_plan_set_boundary flags them
    for (int32_t i : P->ghost_reach) lag[P->tp.inv[i]] |= kGhostBit;
    std::vector<uint8_t> elig;
    rr::mark_inpass_headwaters(P->tp, lag, kGhostBit, elig, info + 1, P->h_coef.empty() ? nullptr : P->h_coef.data());
    return RR_OK;
}

int rr_plan_tile_layout(const rr_plan *P, int32_t *tile_ptr, int32_t *tile_level, int32_t *perm, int32_t *lag, int32_t *cfirst,
                        uint32_t *ccnt, int32_t *xpos)
{
    if (!P) return fail(RR_E_INVALID, "rr_plan_tile_layout: null plan");
    const rr::TilePlan &T = P->tp;
    if (!T.ok) return fail(RR_E_UNSUPPORTED, "rr_plan_tile_layout: this network does not tile (a reach has more upstream reaches than a tile holds)");
    auto copy = [](auto *dst, const auto &src) { if (dst && !src.empty()) std::memcpy(dst, src.data(), src.size() * sizeof(src[0])); };
    copy(tile_ptr, T.tile_ptr); copy(tile_level, T.tile_level); copy(perm, T.perm); copy(lag, T.lag); copy(cfirst, T.cfirst);
    copy(ccnt, T.ccnt); copy(xpos, T.xpos);
    return RR_OK;
}

int rr_plan_direct_info(const rr_plan *P, int64_t info[8], char *why, int64_t why_cap)
{
    if (!P || !info) return fail(RR_E_INVALID, "rr_plan_direct_info: null argument");
    const rr::DirectPlan &D = P->dp;
    info[0] = D.ok ? 1 : 0; info[1] = D.n_tiles; info[2] = D.n_holes; info[3] = D.n_exports; info[4] = D.skel.np; info[5] = D.skel.n_tiles;
    info[6] = D.skel.n_levels; info[7] = P->direct_window;
    if (why && why_cap > 0) { std::strncpy(why, D.why.c_str(), (size_t)why_cap - 1); why[why_cap - 1] = 0; }
    return RR_OK;
}

int rr_plan_direct_layout(const rr_plan *P, int32_t *tile_c0, int32_t *tile_nc, int32_t *tile_lag_lo, int32_t *tile_span, int32_t *delay, int32_t *up3, int32_t *xinfo)
{
    if (!P) return fail(RR_E_INVALID, "rr_plan_direct_layout: null plan");
    const rr::DirectPlan &D = P->dp;
    if (!D.ok) return fail(RR_E_UNSUPPORTED, "rr_plan_direct_layout: the direct row path does not apply to this plan: " + D.why);
    auto copy = [](auto *dst, const auto &src) { if (dst && !src.empty()) std::memcpy(dst, src.data(), src.size() * sizeof(src[0])); };
    copy(tile_c0, D.tile_c0); copy(tile_nc, D.tile_nc); copy(tile_lag_lo, D.tile_lag_lo); copy(tile_span, D.tile_span);
    copy(delay, D.delay); copy(up3, D.up3); copy(xinfo, D.xinfo);
    return RR_OK;
}

int rr_plan_last_kernel(const rr_plan *P)
{
    if (!P) return -1;
    return P->ses.members > 0 ? RR_KERNEL_TILE_ENSEMBLE : (int)P->ses.kernel;
}

int rr_plan_set_options(rr_plan *P, int64_t rows_per_chunk, int64_t sample_every)
{
    if (!P) return fail(RR_E_INVALID, "rr_plan_set_options: null plan");
    if (rows_per_chunk > 0) P->chunk_rows = rows_per_chunk;
    if (sample_every >= 0) P->sample_every = sample_every;
    return RR_OK;
}

int rr_plan_set_row_format(rr_plan *P, int in32_big_endian, int out32_big_endian)
{
    if (!P) return fail(RR_E_INVALID, "rr_plan_set_row_format: null plan");
    if (P->ses.open) return fail(RR_E_STATE, "rr_plan_set_row_format: a routing call is open");
    P->in32_big_endian = in32_big_endian != 0; P->out32_big_endian = out32_big_endian != 0;
    return RR_OK;
}

int rr_plan_set_coeffs(rr_plan *P, const double *lhs_off_data, const double *c2, const double *c3, const double *c4_dt)
{
    int rc = need_device(P);
    if (rc) return rc;
    const rr::HostPlan &H = P->h;
    const int64_t n = H.n;
    if (n > 0 && (!c2 || !c3 || (H.n_edges > 0 && !lhs_off_data)))
        return fail(RR_E_INVALID, "rr_plan_set_coeffs: null coefficient array");
    // the plan's coefficient set; the time-tiled kernel keeps ONE upstream weight per reach: per-edge weights (never produced by the
    // reference's callers) fall back to the streaming kernel
    rr::LagCoef L;
    std::vector<double> c1row((size_t)n);      // per reach
    P->weights_uniform = rr::lag_coef(H, lhs_off_data, c2, c3, c4_dt, L, c1row.data()) < 0;
    rc = dev_upload(P->d_w, L.w);
    if (!rc) rc = dev_upload(P->d_c1row_h, L.c1row);
    if (!rc && P->tp.ok) {
        lay_tile_coef(P, rr::ReachCoef{c1row.data(), c2, c3, 1});
        // which headwaters the in-pass routes depends on their coefficients: the position tables and column metadata again, then the coefficients
        if (!P->meta_lag.empty()) rc = upload_tile_meta(P, P->meta_lag, P->meta_xpos, P->meta_flags);
        if (!rc) rc = upload_tile_coef(P);
    }
    P->h_reach_coef.resize(4 * (size_t)n);      // the plan's one host copy of the set: rr_plan_set_boundary lays tables out from it again
    rr::reach_coef(n, c1row.data(), c2, c3, c4_dt, P->h_reach_coef.data());
    if (!rc) rc = upload_direct_coef(P);
    if (!rc) rc = dev_upload(P->d_c2, L.c2);
    if (!rc) rc = dev_upload(P->d_c3, L.c3);
    if (!rc) rc = dev_upload(P->d_c4, L.c4);
    if (!rc && c4_dt && n > 0) {
        hipError_t e = hipMemcpy(P->d_c4_params, c4_dt, (size_t)n * sizeof(double), hipMemcpyHostToDevice);
        if (e != hipSuccess) rc = fail(RR_E_HIP, hipGetErrorString(e));
    }
    if (rc) return rc;
    P->coeffs_set = true;
    P->has_c4 = c4_dt != nullptr;
    return RR_OK;
}

int rr_plan_set_unit_weights(rr_plan *P, const double *c1, const double *a_data)
{
    int rc = need_device(P);
    if (rc) return rc;
    if (P->ses.open) return fail(RR_E_STATE, "rr_plan_set_unit_weights: a routing call is open");
    if (!c1 && !a_data) { P->unit_general = false; return RR_OK; }
    const rr::HostPlan &H = P->h;
    const int64_t n = H.n;
    if (!c1 || (H.n_edges > 0 && !a_data)) return fail(RR_E_INVALID, "rr_plan_set_unit_weights: give both arrays, or neither to go back to unit weights");
    if (P->n_ghost > 0 || P->n_export > 0) return fail(RR_E_UNSUPPORTED, "rr_plan_set_unit_weights: general edge data on a partitioned network is not supported");
    std::vector<double> a2(n, 0.0), own(n, 0.0);
    for (int64_t p = 0; p < n; ++p) {
        const int32_t i = H.perm[p], e = H.edge_of[i];
        a2[p] = e >= 0 ? a_data[e] : 0.0;
        own[p] = c1[i];
    }
    rc = assign(P->d_a2, a2);
    if (!rc) rc = assign(P->d_c1own, own);
    if (!rc) rc = P->d_z.reserve(std::max<int64_t>(1, 3 * n));
    if (rc) return rc;
    P->unit_general = true;
    return RR_OK;
}

int rr_plan_reserve(rr_plan *P, int mode, int64_t T, int64_t nsub, int host_rows, int64_t info[8])
{
    int rc = need_device(P);
    if (rc) return rc;
    if (mode < RR_MODE_RAPID || mode > RR_MODE_UNIT || T < 0 || nsub < 1) return fail(RR_E_INVALID, "rr_plan_reserve: unknown mode, negative step count or sub-steps < 1");
    if (!P->coeffs_set) return fail(RR_E_STATE, "rr_plan_reserve before rr_plan_set_coeffs (per-edge weights decide which kernel routes)");
    if (P->ses.open) return fail(RR_E_STATE, "rr_plan_reserve: a routing call is open");
    const Mode m = mode == RR_MODE_RAPID ? Mode::Rapid : (mode == RR_MODE_MUSKINGUM ? Mode::Muskingum : Mode::Unit);
    CallShape shape;      // (the other place a CallShape is built: call_shape)
    shape.mode = m; shape.T = T; shape.nsub = nsub;
    shape.host = (host_rows & 1) != 0;
    shape.dev_rows = !shape.host && (host_rows & RR_ROWS_NOT_PLAIN) == 0;      // device rows the direct row path reads as they are
    shape.out32 = (host_rows & RR_ROWS_F32_OUT) != 0;
    shape.uh = (host_rows & RR_ROWS_UH) != 0;
    Schedule sch;
    rc = reserve_core(P, shape, &sch);
    if (rc) return rc;
    if (info) {
        const bool piped = shape.host && sch.kernel == Kernel::Tile;
        const int64_t levels = sch.kernel == Kernel::Direct ? P->dp.skel.n_levels : (sch.kernel == Kernel::Tile ? P->tp.n_levels : 0);
        info[0] = (int)sch.kernel; info[1] = sch.kernel != Kernel::Tick ? sch.KC * kRec : 1; info[2] = sch.chunks;
        info[3] = (P->d_ring.count() + P->d_mrows.count() + P->d_stage.count()) * (int64_t)sizeof(double);
        info[4] = piped ? 2 * P->pipe.dev_in.count() * (int64_t)sizeof(double) : 0;
        info[5] = piped ? 2 * HostPipe::kPinned * P->pipe.pin_cap * (int64_t)sizeof(double) : 0;
        info[6] = P->h.depth - 1 + levels * sch.KC * kRec;      // pipeline depth in ticks
        info[7] = sch.ring * (int64_t)sizeof(double);
    }
    return RR_OK;
}

// ---- ensembles (rr_rapid_route_ensemble_dev) ----

// Why an ensemble call of this shape does not get the time-tiled kernel, or NULL (record rings that do not fit: ensemble_member_cap).
// member_coeffs: the call routes the members' own coefficient sets, which have one weight per reach each (rr_plan_set_member_coeffs).
static const char *ensemble_unsupported(const rr_plan *P, int64_t T, int64_t nsub, bool member_coeffs = false)
{
    if (!member_coeffs && !P->weights_uniform) return "per-edge weights (the time-tiled kernel keeps one upstream weight per reach)";
    if (T * nsub < 32) return "fewer than 32 routing sub-steps (T x nsub) in a call";
    if (P->n_ghost > 0 || P->n_export > 0) return "the plan has boundary reaches (a partitioned network)";
    if (!P->tp.ok || !P->wave_enabled || !P->ens_enabled || P->wave_threads != kTileThreads || P->export_inside || P->tp.np >= (int64_t{1} << 25)) return "the network does not take the time-tiled kernel";
    return nullptr;
}

static CallShape ensemble_shape(int64_t members, int64_t T, int64_t nsub, bool in32, bool out32, int64_t factor)
{
    CallShape s;
    s.mode = Mode::Rapid; s.T = T; s.nsub = nsub; s.in32 = in32; s.out32 = out32; s.factor = factor; s.members = members;
    return s;
}

// The largest member count whose record rings fit the card at this shape (choose_schedule keeps to the time-tiled kernel: the ring
// only grows with the members).
static int64_t ensemble_member_cap(const rr_plan *P, CallShape s)
{
    int64_t lo = 0, hi = 65535;      // (the member is blockIdx.y)
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) / 2;
        s.members = mid;
        const Schedule sch = choose_schedule(P, s);      // (k_tile<..., ENS> addresses member m's ring chunks and state positions in 32 bits)
        if (sch.kernel == Kernel::Tile && mid * sch.chunks < (int64_t{1} << 32) && mid * P->tp.np < (int64_t{1} << 31)) lo = mid; else hi = mid - 1;
    }
    return lo;
}

int rr_plan_reserve_ensemble(rr_plan *P, int64_t members, int64_t T, int64_t nsub, int flags, int64_t info[9])
{
    int rc = need_device(P);
    if (rc) return rc;
    if (members < 1 || members > 65535 || T < 0 || nsub < 1) return fail(RR_E_INVALID, "rr_plan_reserve_ensemble: need 1 <= members <= 65535, T >= 0 and sub-steps >= 1");
    if (!P->coeffs_set && P->mc_sets == 0) return fail(RR_E_STATE, "rr_plan_reserve_ensemble before rr_plan_set_coeffs (or rr_plan_set_member_coeffs)");
    if (P->ses.open) return fail(RR_E_STATE, "rr_plan_reserve_ensemble: a routing call is open");
    if (info) for (int k = 0; k < 9; ++k) info[k] = 0;
    if (P->h.n == 0 || T == 0) return RR_OK;
    // (the work memory of a call is the same whichever coefficients it routes with: with member sets on the plan the reservation is theirs too)
    if (const char *why = ensemble_unsupported(P, T, nsub, P->mc_sets > 0)) return fail(RR_E_UNSUPPORTED, std::string("rr_plan_reserve_ensemble: ") + why);
    CallShape shape = ensemble_shape(members, T, nsub, (flags & RR_ROWS_F32_IN) != 0, (flags & RR_ROWS_F32_OUT) != 0, 1);
    shape.member_coeffs = P->mc_sets > 0;
    const int64_t cap = ensemble_member_cap(P, shape);
    if (info) info[8] = cap;
    if (members > cap)
        return fail(RR_E_UNSUPPORTED, "rr_plan_reserve_ensemble: the record rings of " + std::to_string(members) + " members do not fit the card at this shape; at most " +
                                          std::to_string(cap) + " per call");
    Schedule sch;
    rc = reserve_core(P, shape, &sch);
    if (rc) return rc;
    if (P->ens_cap < members) {      // the members' carried state, np apart
        reset_all(P->d_esq, P->d_ess, P->d_esi);      // all three before any of the larger ones
        P->ens_cap = 0;
        const int64_t count = members * P->tp.np;
        rc = P->d_esq.alloc(count);
        if (!rc) rc = P->d_ess.alloc(count);
        if (!rc) rc = P->d_esi.alloc(count);
        if (rc) return rc;
        P->ens_cap = members;
    }
    if (info) {
        info[0] = (int)sch.kernel; info[1] = sch.KC * kRec; info[2] = sch.chunks;
        info[3] = (P->d_ring.count() + P->d_mrows.count() + P->d_stage.count()) * (int64_t)sizeof(double);
        info[6] = P->h.depth - 1 + P->tp.n_levels * sch.KC * kRec;
        info[7] = sch.ring * (int64_t)sizeof(double);
        info[8] = cap;
    }
    return RR_OK;
}

int rr_plan_profile(rr_plan *P, double prof[10])
{
    if (!P || !prof) return fail(RR_E_INVALID, "rr_plan_profile: null argument");
    for (int k = 0; k < 10; ++k) prof[k] = 0.0;
    prof[0] = (double)P->prof_launches;
    prof[8] = (double)P->prof_brackets;
    prof[9] = P->ses.kernel != Kernel::Tick ? (double)(P->ses.KC * kRec) : 1.0;
    prof[7] = (double)P->prof_reach_steps;
    if (P->device < 0 || !P->ev_first || P->prof_launches == 0) return RR_OK;
    HIPCHK(hipSetDevice(P->device));
    HIPCHK(hipEventSynchronize(P->ev_last));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, P->ev_first, P->ev_last));
    prof[6] = ms;
    double sum = 0, mn = 1e300, mx = 0, reaches = 0;
    const double per = P->prof_brackets ? (double)P->prof_samples / (double)P->prof_brackets : 1.0;   // ticks per bracket
    for (int64_t k = 0; k < P->prof_brackets; ++k) {
        HIPCHK(hipEventElapsedTime(&ms, P->ev[2 * k], P->ev[2 * k + 1]));
        sum += ms; mn = std::min<double>(mn, ms / per); mx = std::max<double>(mx, ms / per);
        reaches += (double)P->ev_reaches[k];
    }
    prof[1] = (double)P->prof_samples; prof[2] = sum; prof[3] = P->prof_samples ? mn : 0.0; prof[4] = mx;
    prof[5] = reaches;
    return RR_OK;
}

int rr_plan_profile_aux(rr_plan *P, double aux[12])
{
    if (!P || !aux) return fail(RR_E_INVALID, "rr_plan_profile_aux: null argument");
    for (int k = 0; k < 12; ++k) aux[k] = 0.0;
    for (int k = 0; k < rr_plan::kAuxKinds; ++k) aux[3 * k] = (double)P->aux_launches[k];
    if (P->device < 0 || P->aux_kind.empty()) return RR_OK;
    HIPCHK(hipSetDevice(P->device));
    if (P->ev_last) HIPCHK(hipEventSynchronize(P->ev_last));
    for (size_t i = 0; i < P->aux_kind.size(); ++i) {
        float ms = 0.f;
        HIPCHK(hipEventSynchronize(P->aux_ev[2 * i + 1]));
        HIPCHK(hipEventElapsedTime(&ms, P->aux_ev[2 * i], P->aux_ev[2 * i + 1]));
        aux[3 * P->aux_kind[i] + 1] += 1.0;
        aux[3 * P->aux_kind[i] + 2] += ms;
    }
    return RR_OK;
}

// ---- partitioned networks: boundary reaches + streaming calls ----

int rr_plan_set_boundary(rr_plan *P, int64_t n_ghost, const int64_t *ghost_reaches, int64_t n_export,
                         const int64_t *export_reaches)
{
    if (!P) return fail(RR_E_INVALID, "null plan");
    const bool host_only = P->device < 0;      // a host-only plan takes the boundary too: its layouts can be inspected (rr_plan_direct_info)
    int rc = host_only ? RR_OK : need_device(P);
    if (rc) return rc;
    const rr::HostPlan &H = P->h;
    const int64_t n = H.n;
    if (n_ghost < 0 || n_export < 0 || (n_ghost > 0 && !ghost_reaches) || (n_export > 0 && !export_reaches))
        return fail(RR_E_INVALID, "rr_plan_set_boundary: bad argument");
    if (P->ses.open) return fail(RR_E_STATE, "rr_plan_set_boundary: a routing call is open");
    std::vector<int32_t> lag(H.lag), bidx(n, 0);
    int64_t gmin = H.depth, emax = 0;
    for (int64_t g = 0; g < n_ghost; ++g) {
        const int64_t i = ghost_reaches[g];
        if (i < 0 || i >= n) return fail(RR_E_INVALID, "rr_plan_set_boundary: ghost reach out of range");
        const int32_t p = H.inv[i];
        if (lag[p] & kGhostBit) return fail(RR_E_INVALID, "rr_plan_set_boundary: a ghost reach is listed twice");
        lag[p] |= kGhostBit;
        bidx[p] = (int32_t)g;
        gmin = std::min<int64_t>(gmin, H.lag[p]);
    }
    for (int64_t e = 0; e < n_export; ++e) {
        const int64_t i = export_reaches[e];
        if (i < 0 || i >= n) return fail(RR_E_INVALID, "rr_plan_set_boundary: export reach out of range");
        const int32_t p = H.inv[i];
        if (lag[p] & (kGhostBit | kExportBit))
            return fail(RR_E_INVALID, "rr_plan_set_boundary: an export reach must be a real reach, listed once");
        lag[p] |= kExportBit;
        bidx[p] = (int32_t)e;
        emax = std::max<int64_t>(emax, H.lag[p]);
    }
    P->boundary_whole = false;      // until everything below has succeeded
    if (!host_only) {
        rc = dev_upload(P->d_lag, lag);
        if (!rc) rc = dev_upload(P->d_bidx, bidx);
        if (rc) return rc;
    }
    P->n_ghost = n_ghost; P->n_export = n_export;
    P->ghost_min_lag = n_ghost ? gmin : 0;
    P->export_max_lag = n_export ? emax : 0;
    P->ghost_reach.assign(n_ghost, 0); P->export_reach.assign(n_export, 0);
    for (int64_t g = 0; g < n_ghost; ++g) P->ghost_reach[g] = (int32_t)ghost_reaches[g];
    for (int64_t e = 0; e < n_export; ++e) P->export_reach[e] = (int32_t)export_reaches[e];
    {   // the direct row path, laid out again around the boundary reaches: a ghost's column is passed through (its series becomes the record
        // of the skeleton's ghost that mirrors it), an export is stored by the skeleton's kernel or by its lane (rr_plan.hpp: build_direct_plan)
        std::vector<uint8_t> gmask((size_t)n, 0);
        std::vector<int32_t> eslot((size_t)n, -1), lag_of((size_t)n);
        for (int64_t g = 0; g < n_ghost; ++g) gmask[ghost_reaches[g]] = 1;
        for (int64_t e = 0; e < n_export; ++e) eslot[export_reaches[e]] = (int32_t)e;
        for (int64_t i = 0; i < n; ++i) lag_of[i] = H.lag[H.inv[i]];
        rr::build_direct_plan(H.down, lag_of, std::min<int32_t>(kDirectLanes, P->direct_block), kDirectMaxWindow - 2, P->direct_block, P->dp,
                              n_ghost ? &gmask : nullptr, n_export ? &eslot : nullptr);
        rc = upload_direct_plan(P);
        if (!rc) rc = upload_direct_coef(P);
        if (rc) return rc;
    }
    if (!host_only && P->tp.ok) {      // the same flags and slots in the tile layout
        const rr::TilePlan &TP = P->tp;
        // flags in the tile layout; an export reach's slot in the export series travels in xpos[], the word a reach mirrored
        // by another tile's ghost uses for that ghost's position -- an export is normally an outlet of its part and has no
        // such ghost; where it has one, the plan keeps to the streaming kernel
        std::vector<int32_t> tlag(TP.lag), txpos(TP.xpos);
        P->export_inside = false;
        for (int64_t g = 0; g < n_ghost; ++g) { const int32_t p = TP.inv[ghost_reaches[g]]; tlag[p] |= kGhostBit; }
        for (int64_t e = 0; e < n_export; ++e) {
            const int32_t p = TP.inv[export_reaches[e]];
            if (tlag[p] & kTileExportBit) P->export_inside = true;
            tlag[p] |= kExportBit; txpos[p] = (int32_t)e;
        }
        std::vector<int32_t> tflags(TP.tile_flags);      // a tile with a boundary export stores it tick by tick
        for (int64_t e = 0; e < n_export; ++e) tflags[TP.tile_of[TP.inv[export_reaches[e]]]] |= kTileExports;
        if (!P->h_reach_coef.empty()) lay_tile_coef(P, rr::table_rows(P->h_reach_coef.data()));      // zeros at the new boundary ghosts
        rc = upload_tile_meta(P, tlag, P->export_inside ? TP.xpos : txpos, tflags);
        if (!rc) rc = upload_tile_coef(P);
        std::vector<int2> gm((size_t)n_ghost);
        for (int64_t g = 0; g < n_ghost; ++g) { const int32_t p = TP.inv[ghost_reaches[g]]; gm[g] = make_int2(p, TP.lag[p] & kLagMask); }
        DevBuf<int2> ghostmeta;      // the plan keeps the table it has until this one is whole
        if (!rc) rc = ghostmeta.alloc(n_ghost);
        if (!rc) rc = dev_upload(ghostmeta, gm);
        if (rc) return rc;
        P->d_ghostmeta = std::move(ghostmeta);
    }
    P->boundary_whole = true;
    return RR_OK;
}

int rr_stream_begin(rr_plan *P, int has_lateral, const double *q_t, const double *lateral, int64_t lat_rows,
                    double *discharge, int64_t out_rows, int64_t T, int64_t nsub, const double *ghost_series,
                    double *export_series, void *stream)
{
    int rc = check_route_args(P, has_lateral != 0, T, nsub);
    if (rc) return rc;
    if (P->h.n > 0 && T > 0 && (!q_t || !discharge || out_rows < 1 || (has_lateral && (!lateral || lat_rows < 1))))
        return fail(RR_E_INVALID, "rr_stream_begin: null array or empty row count");
    Rows io; io.dev_in = has_lateral ? lateral : nullptr; io.rows_in = lat_rows; io.dev_out = discharge; io.rows_out = out_rows;
    const Mode mode = has_lateral ? Mode::Rapid : Mode::Muskingum;
    if (P->ses.open) return fail(RR_E_STATE, "a routing call is already open on this plan (rr_stream_end it first)");
    rc = prepare_call(P, call_shape(mode, T, nsub, io, true), "rr_stream_begin");
    if (rc) return rc;
    if (P->h.n > 0 && T > 0) {
        rc = launch_state_in(P, q_t, (hipStream_t)stream);
        if (rc) return rc;
    }
    return session_begin(P, mode, T, nsub, io, (hipStream_t)stream, ghost_series, export_series);
}

int rr_stream_begin_unit(rr_plan *P, const double *q_ch, const double *q_full, const double *lateral, int64_t lat_rows,
                         double *discharge, int64_t out_rows, int64_t T, int64_t nsub, const double *ghost_series,
                         double *export_series, void *stream)
{
    int rc = check_route_args(P, false, T, nsub);
    if (rc) return rc;
    const int64_t ni = (int64_t)P->h.inner_pos.size();
    if (P->h.n > 0 && T > 0 && (!lateral || !discharge || lat_rows < 1 || out_rows < 1 || (ni > 0 && (!q_ch || !q_full))))
        return fail(RR_E_INVALID, "rr_stream_begin_unit: null array or empty row count");
    Rows io; io.dev_in = lateral; io.rows_in = lat_rows; io.dev_out = discharge; io.rows_out = out_rows;
    if (P->ses.open) return fail(RR_E_STATE, "a routing call is already open on this plan (rr_stream_end_unit it first)");
    if (P->unit_general) return fail(RR_E_UNSUPPORTED, "rr_stream_begin_unit: general edge data (rr_plan_set_unit_weights) on a partitioned network is not supported");
    rc = prepare_call(P, call_shape(Mode::Unit, T, nsub, io, true), "rr_stream_begin_unit");
    if (rc) return rc;
    if (P->h.n > 0 && T > 0) {
        rc = unit_state_in(P, q_ch, q_full, (hipStream_t)stream);
        if (rc) return rc;
    }
    return session_begin(P, Mode::Unit, T, nsub, io, (hipStream_t)stream, ghost_series, export_series);
}

int rr_stream_end_unit(rr_plan *P, double *q_ch, double *q_full)
{
    int rc = need_device(P);
    if (rc) return rc;
    if (P->ses.open && P->ses.mode != Mode::Unit) return fail(RR_E_STATE, "rr_stream_end_unit: the open call is not a UnitMuskingum call");
    const int64_t total = P->ses.total;
    hipStream_t stream = P->ses.stream;
    rc = session_end(P);
    if (rc) return rc;
    if (P->h.n > 0 && total > 0 && q_ch && q_full) unit_state_out(P, q_ch, q_full, total, stream);
    return RR_OK;
}

int rr_stream_advance(rr_plan *P, int64_t lateral_rows_ready, int64_t ghost_substeps_ready, int64_t *export_substeps_ready)
{
    int rc = need_device(P);
    if (rc) return rc;
    return session_advance(P, lateral_rows_ready, ghost_substeps_ready, export_substeps_ready);
}

int rr_stream_end(rr_plan *P, double *q_t)
{
    int rc = need_device(P);
    if (rc) return rc;
    const int64_t total = P->ses.total;
    hipStream_t stream = P->ses.stream;
    rc = session_end(P);
    if (rc) return rc;
    if (P->h.n > 0 && total > 0 && q_t) launch_state_out(P, q_t, total, stream);
    return RR_OK;
}

int rr_partition_forest(int64_t n, const int32_t *csc_indptr, const int32_t *csc_indices, int32_t n_parts,
                        int32_t *part_of, int64_t *part_sizes)
{
    if (!part_of || n_parts < 1) return fail(RR_E_INVALID, "rr_partition_forest: bad argument");
    rr::HostPlan H;
    std::string err;
    int rc = rr::build_host_plan(n, csc_indptr, csc_indices, H, err);
    if (rc) return fail(rc, err);
    std::vector<int32_t> down(n, -1);
    for (int64_t i = 0; i < n; ++i) if (H.edge_of[i] >= 0) down[i] = csc_indices[H.edge_of[i]];
    std::vector<int64_t> sizes;
    rr::partition_forest(down, n_parts, part_of, sizes);
    if (part_sizes) for (int32_t k = 0; k < n_parts; ++k) part_sizes[k] = k < (int32_t)sizes.size() ? sizes[k] : 0;
    return RR_OK;
}

int rr_postorder(int64_t n, const int64_t *down_index, int64_t *order)
{
    if (n < 0 || (n > 0 && (!down_index || !order))) return fail(RR_E_INVALID, "rr_postorder: bad argument");
    if (!rr::postorder(down_index, n, order)) return fail(RR_E_INVALID, "rr_postorder: a downstream index is out of range, or the network has a cycle");
    return RR_OK;
}

// ---- device-pointer entry points ----

// The output of a *_dev route call: float64 rows (out_rows of them) or float32 rows, each the mean of `factor` routed rows (prepare_call
// checks factor).  False unless exactly one of the two arrays is given, and float64 rows have rows.
static bool dev_output(Rows &io, double *discharge, int64_t out_rows, float *discharge32, int64_t factor, int64_t T)
{
    if (discharge32) { io.dev_out32 = discharge32; io.out_factor = factor; io.rows_out = factor >= 1 ? T / factor : 0; }
    else { io.dev_out = discharge; io.rows_out = out_rows; }
    return (discharge != nullptr) != (discharge32 != nullptr) && (discharge32 || out_rows >= 1);
}

int rr_rapid_route_dev(rr_plan *P, double *q_t, const double *qlateral, int64_t ql_rows, double *discharge,
                       int64_t out_rows, int64_t T, int64_t nsub, void *stream)
{
    int rc = check_route_args(P, true, T, nsub);
    if (rc) return rc;
    Rows io; io.dev_in = qlateral; io.rows_in = ql_rows;
    const bool out = dev_output(io, discharge, out_rows, nullptr, 1, T);
    if (P->h.n > 0 && T > 0 && (!q_t || !qlateral || ql_rows < 1 || !out))
        return fail(RR_E_INVALID, "rr_rapid_route_dev: null array or empty row count");
    return rapid_like(P, Mode::Rapid, q_t, io, T, nsub, (hipStream_t)stream, false, "rr_rapid_route_dev");
}

int rr_muskingum_route_dev(rr_plan *P, double *q_t, double *discharge, int64_t out_rows, int64_t n_out,
                           int64_t n_per_out, void *stream)
{
    int rc = check_route_args(P, false, n_out, n_per_out);
    if (rc) return rc;
    Rows io;
    const bool out = dev_output(io, discharge, out_rows, nullptr, 1, n_out);
    if (P->h.n > 0 && n_out > 0 && (!q_t || !out))
        return fail(RR_E_INVALID, "rr_muskingum_route_dev: null array or empty row count");
    return rapid_like(P, Mode::Muskingum, q_t, io, n_out, n_per_out, (hipStream_t)stream, false, "rr_muskingum_route_dev");
}

int rr_unit_route_dev(rr_plan *P, double *q_ch, double *q_full, const double *conv, int64_t conv_rows,
                      double *discharge, int64_t out_rows, int64_t T, int64_t nsub, void *stream)
{
    int rc = check_route_args(P, false, T, nsub);
    if (rc) return rc;
    Rows io; io.dev_in = conv; io.rows_in = conv_rows;
    const bool out = dev_output(io, discharge, out_rows, nullptr, 1, T);
    if (P->h.n > 0 && T > 0 && (!conv || conv_rows < 1 || !out || (!P->h.inner_pos.empty() && (!q_ch || !q_full))))
        return fail(RR_E_INVALID, "rr_unit_route_dev: null array or empty row count");
    return unit_like(P, q_ch, q_full, io, T, nsub, (hipStream_t)stream, false, "rr_unit_route_dev");
}

// float32 output fused into the out-pass (k_rec_out, or the direct row path's lanes): applies when the call gets the time-tiled kernel or the
// direct row path and factor x sub-steps divides the tick-rows of a batch (128); otherwise RR_E_UNSUPPORTED (prepare_call) and the caller
// uses the float64 form + rr_resample_cast_dev.
int rr_rapid_route_f32_dev(rr_plan *P, double *q_t, const double *qlateral, int64_t ql_rows, float *discharge32, int64_t T,
                           int64_t nsub, int64_t factor, void *stream)
{
    int rc = check_route_args(P, true, T, nsub);
    if (rc) return rc;
    Rows io; io.dev_in = qlateral; io.rows_in = ql_rows;
    const bool out = dev_output(io, nullptr, 0, discharge32, factor, T);
    if (P->h.n > 0 && T > 0 && (!q_t || !qlateral || !out || ql_rows < 1))
        return fail(RR_E_INVALID, "rr_rapid_route_f32_dev: null array or empty row count");
    return rapid_like(P, Mode::Rapid, q_t, io, T, nsub, (hipStream_t)stream, false, "rr_rapid_route_f32_dev");
}

int rr_rapid_route_f32in_dev(rr_plan *P, double *q_t, const float *qlateral32, int64_t ql_rows, double *discharge, int64_t out_rows,
                             float *discharge32, int64_t factor, int64_t T, int64_t nsub, void *stream)
{
    int rc = check_route_args(P, true, T, nsub);
    if (rc) return rc;
    Rows io; io.dev_in32 = qlateral32; io.rows_in = ql_rows;
    const bool out = dev_output(io, discharge, out_rows, discharge32, factor, T);
    if (P->h.n > 0 && T > 0 && (!q_t || !qlateral32 || ql_rows < 1 || !out))
        return fail(RR_E_INVALID, "rr_rapid_route_f32in_dev: null array, empty row count, or both or neither output");
    return rapid_like(P, Mode::Rapid, q_t, io, T, nsub, (hipStream_t)stream, false, "rr_rapid_route_f32in_dev");
}

// An ensemble call on the time-tiled kernel: with the plan's coefficients for every member (rr_rapid_route_ensemble_dev), or with the
// members' own sets (member_coeffs: rr_rapid_route_members_dev, where a lateral pitch of 0 shares one forcing).  The caller has checked the plan.
static int ensemble_route(rr_plan *P, const char *who, bool member_coeffs, int64_t members, double *q_t, int64_t q_pitch, const void *lateral, int lateral_is_f32,
                          int64_t lateral_member_pitch, void *discharge, int discharge_is_f32, int64_t discharge_member_pitch,
                          int64_t factor, int64_t T, int64_t nsub, void *stream)
{
    const std::string name(who);
    const int64_t n = P->h.n;
    if (members < 1 || members > 65535) return fail(RR_E_INVALID, name + ": need 1 <= members <= 65535");
    if (n == 0 || T == 0) return RR_OK;
    if (!q_t || !lateral || !discharge) return fail(RR_E_INVALID, name + ": null array");
    if (discharge_is_f32 && (factor < 1 || T % factor != 0))
        return fail(RR_E_INVALID, name + ": float32 output: the number of rows must be a multiple of factor >= 1");
    const int64_t out_rows = discharge_is_f32 ? T / factor : T;
    const bool shared_lateral = member_coeffs && lateral_member_pitch == 0;
    if (q_pitch < n || (!shared_lateral && lateral_member_pitch < T * n) || discharge_member_pitch < out_rows * n)
        return fail(RR_E_INVALID, name + ": a pitch is shorter than a member (q_pitch >= n, lateral pitch >= T n" + (member_coeffs ? " or 0: one forcing for all" : "") +
                                      ", discharge pitch >= rows x n)");
    if (member_coeffs && members > P->mc_sets)
        return fail(RR_E_STATE, name + ": " + std::to_string(members) + " members but " + std::to_string(P->mc_sets) + " coefficient sets: call rr_plan_set_member_coeffs(plan, " +
                                    std::to_string(members) + ", ...) first");
    if (const char *why = ensemble_unsupported(P, T, nsub, member_coeffs)) return fail(RR_E_UNSUPPORTED, name + ": " + why);
    Rows io;
    if (lateral_is_f32) io.dev_in32 = (const float *)lateral; else io.dev_in = (const double *)lateral;
    io.rows_in = T;
    if (discharge_is_f32) { io.dev_out32 = (float *)discharge; io.out_factor = factor; } else io.dev_out = (double *)discharge;
    io.rows_out = out_rows;
    io.members = members; io.in_pitch = lateral_member_pitch; io.out_pitch = discharge_member_pitch; io.member_coeffs = member_coeffs;
    const CallShape shape = call_shape(Mode::Rapid, T, nsub, io);
    if (members > ensemble_member_cap(P, shape))
        return fail(RR_E_UNSUPPORTED, name + ": the record rings of " + std::to_string(members) + " members do not fit the card; route fewer per call "
                                      "(rr_plan_reserve_ensemble's info[8])");
    int rc = prepare_call(P, shape, who);
    if (rc) return rc;
    if (P->ens_cap < members)
        return fail(RR_E_STATE, "the carried state of " + std::to_string(members) + " members was not reserved: call rr_plan_reserve_ensemble(plan, " + std::to_string(members) +
                                ", " + std::to_string(T) + ", " + std::to_string(nsub) + ", ...) first; " + name + " only enqueues work");
    const hipStream_t st = (hipStream_t)stream;
    const int64_t np = P->tp.np;
    hipLaunchKernelGGL(k_tile_state_in_ens, dim3((unsigned)((np + kBlock - 1) / kBlock), (unsigned)members), dim3(kBlock), 0, st, P->d_esq, P->d_ess, P->d_esi,
                       (const double *)q_t, q_pitch, (const int32_t *)P->ts.perm, (const int4 *)P->ts.pmeta, (int32_t)np);
    rc = route_core(P, Mode::Rapid, T, nsub, io, st);
    if (rc) return rc;
    hipLaunchKernelGGL(k_tile_state_out_ens, dim3((unsigned)((n + kBlock - 1) / kBlock), (unsigned)members), dim3(kBlock), 0, st, q_t, q_pitch,
                       (const double *)P->d_esq, np, (const int32_t *)P->d_tinv, (int32_t)n);
    HIPCHK(hipGetLastError());
    return RR_OK;
}

int rr_rapid_route_ensemble_dev(rr_plan *P, int64_t members, double *q_t, int64_t q_pitch, const void *lateral, int lateral_is_f32,
                                int64_t lateral_member_pitch, void *discharge, int discharge_is_f32, int64_t discharge_member_pitch,
                                int64_t factor, int64_t T, int64_t nsub, void *stream)
{
    int rc = check_route_args(P, true, T, nsub);
    if (rc) return rc;
    return ensemble_route(P, "rr_rapid_route_ensemble_dev", false, members, q_t, q_pitch, lateral, lateral_is_f32, lateral_member_pitch, discharge, discharge_is_f32,
                          discharge_member_pitch, factor, T, nsub, stream);
}

// ---- parameter ensembles: a coefficient set per member (rr_plan_set_member_coeffs, rr_rapid_route_members_dev) ----

int rr_plan_set_member_coeffs(rr_plan *P, int64_t members, const double *lhs_off_data, int64_t lhs_pitch, const double *c2, const double *c3, const double *c4_dt,
                              int64_t pitch)
{
    int rc = need_device(P);
    if (rc) return rc;
    if (P->ses.open) return fail(RR_E_STATE, "rr_plan_set_member_coeffs: a routing call is open");
    const rr::HostPlan &H = P->h;
    const rr::TilePlan &TP = P->tp;
    const int64_t n = H.n;
    if (members < 1 || members > 65535) return fail(RR_E_INVALID, "rr_plan_set_member_coeffs: need 1 <= members <= 65535");
    if (!c2 || !c3 || !c4_dt || (H.n_edges > 0 && !lhs_off_data)) return fail(RR_E_INVALID, "rr_plan_set_member_coeffs: null coefficient array (c4_dt included: the members are RapidMuskingum's)");
    if (pitch < n || (members > 1 && lhs_pitch < H.n_edges))
        return fail(RR_E_INVALID, "rr_plan_set_member_coeffs: a pitch is shorter than a member (pitch >= n, lhs_pitch >= the number of edges)");
    if (!TP.ok) return fail(RR_E_UNSUPPORTED, "rr_plan_set_member_coeffs: the network does not take the time-tiled kernel");
    const size_t staged = (size_t)(members * 3 * TP.np);
    std::unique_ptr<double[]> coef;      // the members' tile-order tables, 3 np apart (not filled here: tile_coef writes every position)
    std::vector<double> c1row, w;        // one member's c1row per reach; its edge weights in lag order
    try { coef.reset(new double[staged]); c1row.resize((size_t)n); }
    catch (const std::bad_alloc &) { return fail(RR_E_ALLOC, "rr_plan_set_member_coeffs: out of host memory for the members' tables"); }
    for (int64_t m = 0; m < members; ++m) {
        const int64_t i = rr::tributary_weight(H, lhs_off_data ? lhs_off_data + m * lhs_pitch : nullptr, w, c1row.data());
        if (i >= 0) return fail(RR_E_UNSUPPORTED, "rr_plan_set_member_coeffs: member " + std::to_string(m) + " has per-edge weights (two tributaries of reach " + std::to_string(i) +
                                              " differ): the time-tiled kernel keeps one upstream weight per reach, and a parameter ensemble has no streaming fallback");
        rr::tile_coef(TP, rr::ReachCoef{c1row.data(), c2 + m * pitch, c3 + m * pitch, 1}, kTileGhostBit, P->ghost_reach, coef.get() + m * 3 * TP.np);
    }
    P->mc_sets = 0;      // until both tables are whole
    rc = P->d_mcoef.reserve(members * 3 * TP.np);
    if (!rc) rc = P->d_mc4.reserve(members * n);
    if (!rc) rc = dev_upload(P->d_mcoef.get(), coef.get(), staged);
    if (!rc && n > 0) {
        const hipError_t e = hipMemcpy2D(P->d_mc4, (size_t)n * sizeof(double), c4_dt, (size_t)pitch * sizeof(double), (size_t)n * sizeof(double), (size_t)members, hipMemcpyHostToDevice);
        if (e != hipSuccess) rc = fail(RR_E_HIP, hipGetErrorString(e));
    }
    if (rc) return rc;
    P->mc_sets = members;
    return RR_OK;
}

int rr_rapid_route_members_dev(rr_plan *P, int64_t members, double *q_t, int64_t q_pitch, const void *lateral, int lateral_is_f32,
                               int64_t lateral_member_pitch, void *discharge, int discharge_is_f32, int64_t discharge_member_pitch,
                               int64_t factor, int64_t T, int64_t nsub, void *stream)
{
    int rc = need_device(P);      // (check_route_args without the plan's own coefficients: the call needs none)
    if (rc) return rc;
    if (!P->boundary_whole) return fail(RR_E_STATE, "rr_rapid_route_members_dev after a failed rr_plan_set_boundary: repeat that call first");
    if (T < 0 || nsub < 1 || nsub > 0x7FFFFFFF) return fail(RR_E_INVALID, "rr_rapid_route_members_dev: need num steps >= 0 and 1 <= sub-steps < 2^31");
    return ensemble_route(P, "rr_rapid_route_members_dev", true, members, q_t, q_pitch, lateral, lateral_is_f32, lateral_member_pitch, discharge, discharge_is_f32,
                          discharge_member_pitch, factor, T, nsub, stream);
}

int rr_muskingum_route_f32_dev(rr_plan *P, double *q_t, float *discharge32, int64_t n_out, int64_t n_per_out, void *stream)
{
    int rc = check_route_args(P, false, n_out, n_per_out);
    if (rc) return rc;
    Rows io;
    const bool out = dev_output(io, nullptr, 0, discharge32, 1, n_out);
    if (P->h.n > 0 && n_out > 0 && (!q_t || !out)) return fail(RR_E_INVALID, "rr_muskingum_route_f32_dev: null array");
    return rapid_like(P, Mode::Muskingum, q_t, io, n_out, n_per_out, (hipStream_t)stream, false, "rr_muskingum_route_f32_dev");
}

int rr_unit_route_f32_dev(rr_plan *P, double *q_ch, double *q_full, const double *conv, int64_t conv_rows, float *discharge32,
                          int64_t T, int64_t nsub, int64_t factor, void *stream)
{
    int rc = check_route_args(P, false, T, nsub);
    if (rc) return rc;
    Rows io; io.dev_in = conv; io.rows_in = conv_rows;
    const bool out = dev_output(io, nullptr, 0, discharge32, factor, T);
    if (P->h.n > 0 && T > 0 && (!conv || !out || conv_rows < 1 || (!P->h.inner_pos.empty() && (!q_ch || !q_full))))
        return fail(RR_E_INVALID, "rr_unit_route_f32_dev: null array or empty row count");
    return unit_like(P, q_ch, q_full, io, T, nsub, (hipStream_t)stream, false, "rr_unit_route_f32_dev");
}

int rr_rapid_route_runoff_dev(rr_plan *P, double *q_t, int64_t n_points, const int32_t *indptr, const int32_t *indices,
                              const double *weights, const void *runoff, int runoff_is_f32, int64_t stride_t, int64_t stride_p,
                              const double *area, int flags, double *discharge, float *discharge32, int64_t factor, int64_t T,
                              void *stream)
{
    int rc = check_route_args(P, true, T, 1);
    if (rc) return rc;
    const RunoffArgs ga{indptr, indices, weights, area, runoff, stride_t, stride_p, (int32_t)flags, runoff_is_f32 ? 1 : 0};
    Rows io; io.runoff = &ga;      // no lateral rows: the in-pass makes them
    const bool out = dev_output(io, discharge, T, discharge32, factor, T);
    if (P->h.n > 0 && T > 0 && (!q_t || !indptr || !indices || !weights || !runoff || !out))
        return fail(RR_E_INVALID, "rr_rapid_route_runoff_dev: null array, or both or neither output");
    if (n_points < 0 || stride_t < 0 || stride_p < 0) return fail(RR_E_INVALID, "rr_rapid_route_runoff_dev: negative size or stride");
    return rapid_like(P, Mode::Rapid, q_t, io, T, 1, (hipStream_t)stream, false, "rr_rapid_route_runoff_dev");
}

int rr_unit_route_uh_dev(rr_plan *P, double *q_ch, double *q_full, double *q_final, const double *uh_kernel, double *uh_state,
                         int64_t n_ks, const double *depth, double *discharge, float *discharge32, int64_t factor, int64_t T,
                         int64_t nsub, void *stream)
{
    int rc = check_route_args(P, false, T, nsub);
    if (rc) return rc;
    Rows io; io.dev_in = depth; io.rows_in = T; io.uh_kernel = uh_kernel; io.uh_state = uh_state; io.uh_nks = n_ks;
    const bool out = dev_output(io, discharge, T, discharge32, factor, T);
    if (P->h.n > 0 && T > 0 && (!depth || !uh_kernel || !uh_state || !out || n_ks < 1 || (!P->h.inner_pos.empty() && (!q_ch || !q_full))))
        return fail(RR_E_INVALID, "rr_unit_route_uh_dev: null array, both or neither output, or n_ks < 1");
    if (P->h.n > 0 && T > 0 && n_ks > kUhFusedMaxTaps) return fail(RR_E_UNSUPPORTED, "rr_unit_route_uh_dev: more than 64 kernel steps: convolve with rr_uh_convolve_dev, then rr_unit_route_dev");
    return unit_like(P, q_ch, q_full, io, T, nsub, (hipStream_t)stream, false, "rr_unit_route_uh_dev", q_final, uh_state);
}

int rr_unit_route_uh_f32in_dev(rr_plan *P, double *q_ch, double *q_full, double *q_final, const double *uh_kernel, double *uh_state,
                               int64_t n_ks, const float *depth32, double *discharge, float *discharge32, int64_t factor, int64_t T,
                               int64_t nsub, void *stream)
{
    int rc = check_route_args(P, false, T, nsub);
    if (rc) return rc;
    Rows io; io.dev_in32 = depth32; io.rows_in = T; io.uh_kernel = uh_kernel; io.uh_state = uh_state; io.uh_nks = n_ks;
    const bool out = dev_output(io, discharge, T, discharge32, factor, T);
    if (P->h.n > 0 && T > 0 && (!depth32 || !uh_kernel || !uh_state || !out || n_ks < 1 || (!P->h.inner_pos.empty() && (!q_ch || !q_full))))
        return fail(RR_E_INVALID, "rr_unit_route_uh_f32in_dev: null array, both or neither output, or n_ks < 1");
    if (P->h.n > 0 && T > 0 && n_ks > kUhFusedMaxTaps) return fail(RR_E_UNSUPPORTED, "rr_unit_route_uh_f32in_dev: more than 64 kernel steps: convert the rows, convolve with rr_uh_convolve_dev, then rr_unit_route_dev");
    return unit_like(P, q_ch, q_full, io, T, nsub, (hipStream_t)stream, false, "rr_unit_route_uh_f32in_dev", q_final, uh_state);
}

int rr_uh_convolve_dev(int device, const double *kernel, double *state, const double *lateral, double *out,
                       int64_t T, int64_t n_ks, int64_t n, void *stream)
{
    if (device < 0 || device >= rr_device_count()) return fail(RR_E_NO_DEVICE, "rr_uh_convolve: no such HIP device");
    HIPCHK(hipSetDevice(device));
    if (n > 0 && (!kernel || !state || !lateral || !out)) return fail(RR_E_INVALID, "rr_uh_convolve: null array");
    return uh_convolve_core<double>(kernel, state, lateral, out, T, n_ks, n, (hipStream_t)stream, kSelNative);
}

// ---- host-pointer entry points (the reference's kernel boundary) ----

int rr_rapid_route(rr_plan *P, double *q_t, const double *qlateral, double *discharge, int64_t T, int64_t nsub)
{
    int rc = check_route_args(P, true, T, nsub);
    if (rc) return rc;
    if (P->h.n > 0 && T > 0 && (!q_t || !qlateral || !discharge)) return fail(RR_E_INVALID, "rr_rapid_route: null array");
    Rows io; io.host_in = qlateral; io.host_out = discharge;
    rc = rapid_like(P, Mode::Rapid, q_t, io, T, nsub, nullptr, true, "rr_rapid_route");
    if (rc == RR_OK) HIPCHK(hipStreamSynchronize(nullptr));
    return rc;
}

int rr_muskingum_route(rr_plan *P, double *q_t, double *discharge, int64_t n_out, int64_t n_per_out)
{
    int rc = check_route_args(P, false, n_out, n_per_out);
    if (rc) return rc;
    if (P->h.n > 0 && n_out > 0 && (!q_t || !discharge)) return fail(RR_E_INVALID, "rr_muskingum_route: null array");
    Rows io; io.host_out = discharge;
    rc = rapid_like(P, Mode::Muskingum, q_t, io, n_out, n_per_out, nullptr, true, "rr_muskingum_route");
    if (rc == RR_OK) HIPCHK(hipStreamSynchronize(nullptr));
    return rc;
}

int rr_unit_route(rr_plan *P, double *q_ch, double *q_full, const double *conv, double *discharge, int64_t T,
                  int64_t nsub)
{
    int rc = check_route_args(P, false, T, nsub);
    if (rc) return rc;
    if (P->h.n > 0 && T > 0 && (!conv || !discharge || (!P->h.inner_pos.empty() && (!q_ch || !q_full))))
        return fail(RR_E_INVALID, "rr_unit_route: null array");
    Rows io; io.host_in = conv; io.host_out = discharge;
    rc = unit_like(P, q_ch, q_full, io, T, nsub, nullptr, true, "rr_unit_route");
    if (rc == RR_OK) HIPCHK(hipStreamSynchronize(nullptr));
    return rc;
}

int rr_uh_convolve(int device, const double *kernel, double *state, const double *lateral, double *out, int64_t T,
                   int64_t n_ks, int64_t n)
{
    if (device < 0 || device >= rr_device_count()) return fail(RR_E_NO_DEVICE, "rr_uh_convolve: no such HIP device");
    HIPCHK(hipSetDevice(device));
    if (T < 1 || n_ks < 1 || n < 0) return fail(RR_E_INVALID, "rr_uh_convolve: need T >= 1, n_ks >= 1, n >= 0");
    if (n == 0) return RR_OK;
    if (!kernel || !state || !lateral || !out) return fail(RR_E_INVALID, "rr_uh_convolve: null array");
    DevBuf<double> d_k, d_s, d_l, d_o;
    int rc = d_k.alloc(n_ks * n);
    if (!rc) rc = d_s.alloc(n_ks * n);
    if (!rc) rc = d_l.alloc(T * n);
    if (!rc) rc = d_o.alloc(T * n);
    hipError_t e = hipSuccess;
    if (!rc) {
        e = hipMemcpy(d_k, kernel, (size_t)n_ks * n * sizeof(double), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(d_s, state, (size_t)n_ks * n * sizeof(double), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(d_l, lateral, (size_t)T * n * sizeof(double), hipMemcpyHostToDevice);
        if (e != hipSuccess) rc = fail(RR_E_HIP, hipGetErrorString(e));
    }
    if (!rc) rc = uh_convolve_core<double>(d_k.get(), d_s.get(), d_l.get(), d_o.get(), T, n_ks, n, nullptr, kSelNative);
    if (!rc) {
        e = hipMemcpy(out, d_o, (size_t)T * n * sizeof(double), hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(state, d_s, (size_t)n_ks * n * sizeof(double), hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(RR_E_HIP, hipGetErrorString(e));
    }
    return rc;
}

int rr_resample_cast_dev(int device, const double *discharge, int64_t num_rows, int64_t n, int64_t factor, float *out,
                         void *stream)
{
    if (device < 0 || device >= rr_device_count()) return fail(RR_E_NO_DEVICE, "rr_resample_cast_dev: no such HIP device");
    HIPCHK(hipSetDevice(device));
    if (num_rows < 0 || n < 0 || factor < 1 || factor > 0x7FFFFFFF || (factor > 0 && num_rows % factor != 0))
        return fail(RR_E_INVALID, "rr_resample_cast_dev: rows must be a multiple of factor >= 1");
    const int64_t out_rows = num_rows / factor;
    if (out_rows == 0 || n == 0) return RR_OK;
    if (!discharge || !out) return fail(RR_E_INVALID, "rr_resample_cast_dev: null array");
    if (out_rows > 65535) {   // grid.y limit: go in slabs
        for (int64_t o0 = 0; o0 < out_rows; o0 += 65535) {
            const int64_t rows = std::min<int64_t>(65535, out_rows - o0);
            dim3 g((unsigned)((n + kBlock - 1) / kBlock), (unsigned)rows);
            hipLaunchKernelGGL(k_resample_cast, g, dim3(kBlock), 0, (hipStream_t)stream, discharge + o0 * factor * n,
                               out + o0 * n, n, rows, (int32_t)factor);
        }
    } else {
        dim3 g((unsigned)((n + kBlock - 1) / kBlock), (unsigned)out_rows);
        hipLaunchKernelGGL(k_resample_cast, g, dim3(kBlock), 0, (hipStream_t)stream, discharge, out, n, out_rows,
                           (int32_t)factor);
    }
    HIPCHK(hipGetLastError());
    return RR_OK;
}

int rr_runoff_to_qlateral_dev(int device, int64_t n_rivers, int64_t n_points, int64_t T, const int32_t *indptr,
                              const int32_t *indices, const double *weights, const void *runoff, int runoff_is_f32,
                              int64_t stride_t, int64_t stride_p, const double *area, int flags, double *qlateral, void *stream)
{
    if (device < 0 || device >= rr_device_count()) return fail(RR_E_NO_DEVICE, "rr_runoff_to_qlateral_dev: no such HIP device");
    HIPCHK(hipSetDevice(device));
    if (n_rivers < 0 || n_points < 0 || T < 0 || n_rivers > 0x7FFFFFFFLL || n_points > 0x7FFFFFFFLL)
        return fail(RR_E_INVALID, "rr_runoff_to_qlateral_dev: sizes out of range");
    if (n_rivers == 0 || T == 0) return RR_OK;
    if (!indptr || !indices || !weights || !runoff || !qlateral) return fail(RR_E_INVALID, "rr_runoff_to_qlateral_dev: null array");
    const int64_t chunks = (T + kRunoffRows - 1) / kRunoffRows;
    if (chunks > 65535) return fail(RR_E_UNSUPPORTED, "rr_runoff_to_qlateral_dev: more than 1,048,560 time steps in one call");
    dim3 g((unsigned)((n_rivers + kBlock - 1) / kBlock), (unsigned)chunks);
    const bool vec = stride_t == 1 && stride_p % kRunoffRows == 0 && ((uintptr_t)runoff & 15) == 0;
#define RR_RUNOFF_LAUNCH(RT_, VEC_)                                                                                \
    hipLaunchKernelGGL((k_runoff_to_qlateral<RT_, VEC_>), g, dim3(kBlock), 0, (hipStream_t)stream, indptr, indices, weights,  \
                       (const RT_ *)runoff, stride_t, stride_p, area, flags, qlateral, n_rivers, T)
    if (runoff_is_f32) { if (vec) RR_RUNOFF_LAUNCH(float, true); else RR_RUNOFF_LAUNCH(float, false); }
    else { if (vec) RR_RUNOFF_LAUNCH(double, true); else RR_RUNOFF_LAUNCH(double, false); }
#undef RR_RUNOFF_LAUNCH
    HIPCHK(hipGetLastError());
    return RR_OK;
}

int rr_runoff_to_qlateral(int device, int64_t n_rivers, int64_t n_points, int64_t T, const int32_t *indptr,
                          const int32_t *indices, const double *weights, const void *runoff, int runoff_is_f32,
                          int64_t stride_t, int64_t stride_p, const double *area, int flags, double *qlateral)
{
    if (device < 0 || device >= rr_device_count()) return fail(RR_E_NO_DEVICE, "rr_runoff_to_qlateral: no such HIP device");
    HIPCHK(hipSetDevice(device));
    if (n_rivers < 0 || n_points < 0 || T < 0) return fail(RR_E_INVALID, "rr_runoff_to_qlateral: negative size");
    if (n_rivers == 0 || T == 0) return RR_OK;
    if (!indptr || !indices || !weights || !runoff || !qlateral) return fail(RR_E_INVALID, "rr_runoff_to_qlateral: null array");
    // the runoff block spans max over (t, p) of t * stride_t + p * stride_p elements
    if (stride_t < 0 || stride_p < 0) return fail(RR_E_INVALID, "rr_runoff_to_qlateral: negative stride");
    const int64_t nnz = indptr[n_rivers];
    // point-major blocks may pad their rows (stride_p > T): the whole padded image is copied
    const int64_t elems = stride_t == 1 && stride_p >= T ? std::max<int64_t>(1, n_points) * stride_p
                                                        : (T - 1) * stride_t + (n_points > 0 ? (n_points - 1) * stride_p : 0) + 1;
    const size_t esz = runoff_is_f32 ? sizeof(float) : sizeof(double);
    DevBuf<int32_t> d_indptr, d_indices;
    DevBuf<double> d_w, d_area, d_out;
    DevBuf<char> d_runoff;      // float32 or float64 values
    int rc = d_indptr.alloc(n_rivers + 1);
    if (!rc) rc = d_indices.alloc(nnz);
    if (!rc) rc = d_w.alloc(nnz);
    if (!rc && area) rc = d_area.alloc(n_rivers);
    if (!rc) rc = d_out.alloc(T * n_rivers);
    if (!rc && d_runoff.alloc(elems * (int64_t)esz) != RR_OK) rc = fail(RR_E_ALLOC, "rr_runoff_to_qlateral: device allocation failed");
    if (rc) return rc;
    hipError_t e = hipMemcpy(d_indptr, indptr, (size_t)(n_rivers + 1) * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess && nnz > 0) e = hipMemcpy(d_indices, indices, (size_t)nnz * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess && nnz > 0) e = hipMemcpy(d_w, weights, (size_t)nnz * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess && area) e = hipMemcpy(d_area, area, (size_t)n_rivers * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_runoff, runoff, (size_t)elems * esz, hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(RR_E_HIP, hipGetErrorString(e));
    rc = rr_runoff_to_qlateral_dev(device, n_rivers, n_points, T, d_indptr, d_indices, d_w, d_runoff, runoff_is_f32, stride_t,
                                   stride_p, d_area, flags, d_out, nullptr);
    if (!rc) {
        e = hipMemcpy(qlateral, d_out, (size_t)(T * n_rivers) * sizeof(double), hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(RR_E_HIP, hipGetErrorString(e));
    }
    return rc;
}

// ---- adjoints of RapidMuskingum and UnitMuskingum routing (rr_adjoint.hpp) ----

}  // extern "C"

#include "rr_adjoint.hpp"      // here, not at the top: templated kernels land in the code object in the order of their first launch

extern "C" {

int rr_rapid_adjoint_work_bytes(rr_plan *P, int64_t T, int64_t nsub, int64_t *bytes) { return adjoint_work_bytes(kRapidAdjoint, P, T, nsub, bytes); }

int rr_rapid_adjoint_dev(rr_plan *P, const double *q0, const double *lateral, int64_t lat_rows, const double *discharge,
                         const double *grad_out, const double *grad_qfinal, double *grad_lateral, double *grad_q0, double *grad_coef,
                         void *work, int64_t work_bytes, int64_t T, int64_t nsub, void *stream)
{
    AdjointCall c{P, lateral, lat_rows, discharge, grad_out, work, work_bytes, T, nsub, (hipStream_t)stream};
    return rapid_adjoint("rr_rapid_adjoint_dev", kRapidAdjoint, c, q0, grad_qfinal, grad_lateral, grad_q0, grad_coef);
}

int rr_rapid_adjoint_batch_work_bytes(rr_plan *P, int64_t members, int64_t T, int64_t nsub, int64_t *bytes)
{
    return adjoint_work_bytes(kRapidAdjointBatch, P, T, nsub, bytes, members);
}

int rr_rapid_adjoint_batch_dev(rr_plan *P, int64_t members, const double *q0, int64_t q0_pitch, const double *lateral, int64_t lat_rows,
                               int64_t lat_pitch, const double *discharge, const double *grad_out, int64_t out_pitch, const double *grad_qfinal,
                               double *grad_lateral, double *grad_q0, double *grad_coef, void *work, int64_t work_bytes, int64_t T, int64_t nsub,
                               void *stream)
{
    AdjointCall c{P, lateral, lat_rows, discharge, grad_out, work, work_bytes, T, nsub, (hipStream_t)stream, members, q0_pitch, lat_pitch, out_pitch};
    return rapid_adjoint("rr_rapid_adjoint_batch_dev", kRapidAdjointBatch, c, q0, grad_qfinal, grad_lateral, grad_q0, grad_coef);
}

int rr_rapid_adjoint_gauges_work_bytes(rr_plan *P, int64_t members, int64_t n_gauges, int64_t T, int64_t nsub, int with_grad_lateral, int64_t *bytes)
{
    return adjoint_work_bytes(kRapidAdjointGauges, P, T, nsub, bytes, members, n_gauges, with_grad_lateral != 0);
}

int rr_rapid_adjoint_gauges_dev(rr_plan *P, int64_t members, int64_t n_gauges, const int32_t *gauges, const double *q0, int64_t q0_pitch,
                                const double *lateral, int64_t lat_rows, int64_t lat_pitch, const double *discharge_g, const double *grad_out_g,
                                int64_t gauge_pitch, const double *grad_qfinal, double *grad_lateral, double *grad_q0, double *grad_coef, void *work,
                                int64_t work_bytes, int64_t T, int64_t nsub, void *stream)
{
    AdjointCall c{P, lateral, lat_rows, discharge_g, grad_out_g, work, work_bytes, T, nsub, (hipStream_t)stream, members, q0_pitch, lat_pitch,
                  gauge_pitch, 0, n_gauges, gauges, grad_lateral != nullptr};
    return rapid_adjoint("rr_rapid_adjoint_gauges_dev", kRapidAdjointGauges, c, q0, grad_qfinal, grad_lateral, grad_q0, grad_coef);
}

int rr_unit_adjoint_work_bytes(rr_plan *P, int64_t T, int64_t nsub, int64_t *bytes) { return adjoint_work_bytes(kUnitAdjoint, P, T, nsub, bytes); }

int rr_unit_adjoint_dev(rr_plan *P, const double *q_ch0, const double *q_full0, const double *lateral, int64_t lat_rows,
                        const double *discharge, const double *grad_out, const double *grad_qch_final, const double *grad_qfull_final,
                        double *grad_lateral, double *grad_qch0, double *grad_qfull0, double *grad_coef, void *work, int64_t work_bytes,
                        int64_t T, int64_t nsub, void *stream)
{
    AdjointCall c{P, lateral, lat_rows, discharge, grad_out, work, work_bytes, T, nsub, (hipStream_t)stream};
    return unit_adjoint("rr_unit_adjoint_dev", kUnitAdjoint, c, q_ch0, q_full0, grad_qch_final, grad_qfull_final, grad_lateral, grad_qch0, grad_qfull0,
                        grad_coef);
}

int rr_unit_adjoint_batch_work_bytes(rr_plan *P, int64_t members, int64_t T, int64_t nsub, int64_t *bytes)
{
    return adjoint_work_bytes(kUnitAdjointBatch, P, T, nsub, bytes, members);
}

int rr_unit_adjoint_batch_dev(rr_plan *P, int64_t members, const double *q_ch0, const double *q_full0, int64_t state_pitch, const double *lateral,
                              int64_t lat_rows, int64_t lat_pitch, const double *discharge, const double *grad_out, int64_t out_pitch,
                              const double *grad_qch_final, const double *grad_qfull_final, double *grad_lateral, double *grad_qch0,
                              double *grad_qfull0, double *grad_coef, void *work, int64_t work_bytes, int64_t T, int64_t nsub, void *stream)
{
    AdjointCall c{P, lateral, lat_rows, discharge, grad_out, work, work_bytes, T, nsub, (hipStream_t)stream, members, 0, lat_pitch, out_pitch, state_pitch};
    return unit_adjoint("rr_unit_adjoint_batch_dev", kUnitAdjointBatch, c, q_ch0, q_full0, grad_qch_final, grad_qfull_final, grad_lateral, grad_qch0,
                        grad_qfull0, grad_coef);
}

int rr_unit_adjoint_gauges_work_bytes(rr_plan *P, int64_t members, int64_t n_gauges, int64_t T, int64_t nsub, int with_grad_lateral, int64_t *bytes)
{
    return adjoint_work_bytes(kUnitAdjointGauges, P, T, nsub, bytes, members, n_gauges, with_grad_lateral != 0);
}

int rr_unit_adjoint_gauges_dev(rr_plan *P, int64_t members, int64_t n_gauges, const int32_t *gauges, const double *q_ch0, const double *q_full0,
                               int64_t state_pitch, const double *lateral, int64_t lat_rows, int64_t lat_pitch, const double *discharge_g,
                               const double *grad_out_g, int64_t gauge_pitch, const double *grad_qch_final, const double *grad_qfull_final,
                               double *grad_lateral, double *grad_qch0, double *grad_qfull0, double *grad_coef, void *work, int64_t work_bytes,
                               int64_t T, int64_t nsub, void *stream)
{
    AdjointCall c{P, lateral, lat_rows, discharge_g, grad_out_g, work, work_bytes, T, nsub, (hipStream_t)stream, members, 0, lat_pitch,
                  gauge_pitch, state_pitch, n_gauges, gauges, grad_lateral != nullptr};
    return unit_adjoint("rr_unit_adjoint_gauges_dev", kUnitAdjointGauges, c, q_ch0, q_full0, grad_qch_final, grad_qfull_final, grad_lateral,
                        grad_qch0, grad_qfull0, grad_coef);
}

// ---- adjoint of the unit-hydrograph convolution (rr_kernels_adjoint_unit.hpp) ----

namespace {

constexpr int kUhAdjRows = 16;      // rows per thread of k_uh_adjoint_depth
constexpr int kUhAdjTaps = 16;      // taps per thread of k_uh_adjoint_kernel

struct UhAdjointLayout { int64_t tap_blocks, splits, rows_per_split; };

UhAdjointLayout uh_adjoint_layout(int64_t T, int64_t n_ks, int64_t n)
{
    UhAdjointLayout L{};
    L.tap_blocks = (n_ks + kUhAdjTaps - 1) / kUhAdjTaps;
    const int64_t blocks = std::max<int64_t>(1, ((n + kBlock - 1) / kBlock) * L.tap_blocks);
    const int64_t want = std::max<int64_t>(1, (kAdjTargetBlocks + blocks - 1) / blocks);
    L.splits = std::max<int64_t>(1, std::min(want, T));
    L.rows_per_split = (T + L.splits - 1) / L.splits;
    L.splits = (T + L.rows_per_split - 1) / L.rows_per_split;
    return L;
}

}  // namespace

int rr_uh_adjoint_work_bytes(int64_t T, int64_t n_ks, int64_t n, int64_t *bytes)
{
    if (!bytes) return fail(RR_E_INVALID, "rr_uh_adjoint_work_bytes: null argument");
    *bytes = 0;
    if (T < 1 || n_ks < 1 || n < 0 || n_ks > 0x7FFFFFFF) return fail(RR_E_INVALID, "rr_uh_adjoint_work_bytes: need T >= 1, n_ks >= 1, n >= 0");
    const UhAdjointLayout L = uh_adjoint_layout(T, n_ks, n);
    if (L.splits > 1) *bytes = L.splits * n_ks * n * (int64_t)sizeof(double);
    return RR_OK;
}

int rr_uh_adjoint_dev(int device, const double *kernel, const double *depth, const double *grad_convolved, const double *grad_state_out,
                      double *grad_depth, double *grad_kernel, double *grad_state, void *work, int64_t work_bytes, int64_t T,
                      int64_t n_ks, int64_t n, void *stream)
{
    if (device < 0 || device >= rr_device_count()) return fail(RR_E_NO_DEVICE, "rr_uh_adjoint_dev: no such HIP device");
    HIPCHK(hipSetDevice(device));
    if (T < 1 || n_ks < 1 || n < 0 || n_ks > 0x7FFFFFFF) return fail(RR_E_INVALID, "rr_uh_adjoint_dev: need T >= 1, n_ks >= 1, n >= 0");
    if (n == 0 || (!grad_depth && !grad_kernel && !grad_state)) return RR_OK;
    if (grad_depth && !kernel) return fail(RR_E_INVALID, "rr_uh_adjoint_dev: grad_depth needs the kernel");
    if (grad_kernel && !depth) return fail(RR_E_INVALID, "rr_uh_adjoint_dev: grad_kernel needs the depth rows");
    const UhAdjointLayout L = uh_adjoint_layout(T, n_ks, n);
    const int64_t need = L.splits > 1 ? L.splits * n_ks * n * (int64_t)sizeof(double) : 0;
    if (grad_kernel && need > 0 && (!work || work_bytes < need))
        return fail(RR_E_INVALID, "rr_uh_adjoint_dev: work memory smaller than rr_uh_adjoint_work_bytes (" + std::to_string(need) + " bytes)");
    const hipStream_t st = (hipStream_t)stream;
    const UhGrad G{grad_convolved, grad_state_out, T, n, T + n_ks - 1};
    const unsigned col_blocks = (unsigned)((n + kBlock - 1) / kBlock);
    if (grad_depth) {
        const int64_t row_blocks = (T + kUhAdjRows - 1) / kUhAdjRows;
        if (row_blocks > 65535) return fail(RR_E_INVALID, "rr_uh_adjoint_dev: too many rows for one call: split the series into windows");
        hipLaunchKernelGGL(k_uh_adjoint_depth<kUhAdjRows>, dim3(col_blocks, (unsigned)row_blocks), dim3(kBlock), 0, st, kernel, G, grad_depth, (int32_t)n_ks);
    }
    if (grad_kernel) {
        if (L.tap_blocks > 65535) return fail(RR_E_INVALID, "rr_uh_adjoint_dev: too many kernel steps");
        double *slab = L.splits > 1 ? static_cast<double *>(work) : grad_kernel;
        hipLaunchKernelGGL(k_uh_adjoint_kernel<kUhAdjTaps>, dim3(col_blocks, (unsigned)L.splits, (unsigned)L.tap_blocks), dim3(kBlock), 0, st, depth, G,
                           slab, (int32_t)n_ks, L.rows_per_split);
        if (L.splits > 1) {
            const int64_t count = n_ks * n;
            hipLaunchKernelGGL(k_uh_adjoint_merge, dim3((unsigned)std::min<int64_t>((count + kBlock - 1) / kBlock, 8192)), dim3(kBlock), 0, st,
                               (const double *)slab, L.splits, count, grad_kernel);
        }
    }
    if (grad_state) {
        const int64_t count = n_ks * n;
        hipLaunchKernelGGL(k_uh_adjoint_state, dim3((unsigned)std::min<int64_t>((count + kBlock - 1) / kBlock, 8192)), dim3(kBlock), 0, st, G, grad_state, n_ks);
    }
    HIPCHK(hipGetLastError());
    return RR_OK;
}

// ---- device helpers ----

int rr_dev_malloc(int device, int64_t bytes, void **out)
{
    if (!out || bytes < 0) return fail(RR_E_INVALID, "rr_dev_malloc: bad argument");
    if (device < 0 || device >= rr_device_count()) return fail(RR_E_NO_DEVICE, "rr_dev_malloc: no such HIP device");
    HIPCHK(hipSetDevice(device));
    if (rr::dev_mem_alloc(out, (size_t)std::max<int64_t>(bytes, 1)) != RR_OK) return fail(RR_E_ALLOC, "hipMalloc: " + rr::g_dev_refusal);
    return RR_OK;
}

int rr_dev_free(int device, void *ptr)
{
    if (!ptr) return RR_OK;
    if (device < 0 || device >= rr_device_count()) return fail(RR_E_NO_DEVICE, "rr_dev_free: no such HIP device");
    HIPCHK(hipSetDevice(device));
    (void)hipGetLastError();
    rr::dev_mem_free(ptr);
    const hipError_t e = hipGetLastError();      // of the release in there; the message is the one this entry point always had
    if (e != hipSuccess) return fail(RR_E_HIP, std::string("hipFree" "(ptr): ") + hipGetErrorString(e));
    return RR_OK;
}

int rr_dev_alloc_stats(int64_t out[2])
{
    if (!out) return fail(RR_E_INVALID, "rr_dev_alloc_stats: null out");
    out[0] = rr::g_dev_live; out[1] = rr::g_dev_made;
    return RR_OK;
}

int rr_dev_upload(int device, void *dst_dev, const void *src_host, int64_t bytes)
{
    if (device < 0 || device >= rr_device_count()) return fail(RR_E_NO_DEVICE, "rr_dev_upload: no such HIP device");
    HIPCHK(hipSetDevice(device));
    if (bytes > 0) HIPCHK(hipMemcpy(dst_dev, src_host, (size_t)bytes, hipMemcpyHostToDevice));
    return RR_OK;
}

int rr_dev_download(int device, void *dst_host, const void *src_dev, int64_t bytes)
{
    if (device < 0 || device >= rr_device_count()) return fail(RR_E_NO_DEVICE, "rr_dev_download: no such HIP device");
    HIPCHK(hipSetDevice(device));
    if (bytes > 0) HIPCHK(hipMemcpy(dst_host, src_dev, (size_t)bytes, hipMemcpyDeviceToHost));
    return RR_OK;
}

int rr_copy_bandwidth(int device, int64_t bytes, int reps, double *gbps)
{
    if (!gbps || bytes < 1024 || reps < 1) return fail(RR_E_INVALID, "rr_copy_bandwidth: bad argument");
    if (device < 0 || device >= rr_device_count()) return fail(RR_E_NO_DEVICE, "rr_copy_bandwidth: no such HIP device");
    HIPCHK(hipSetDevice(device));
    const int64_t count = bytes / 16;
    DevBuf<double2> a, b;
    int rc = a.alloc(count);
    if (!rc) rc = b.alloc(count);
    hipEvent_t e0 = nullptr, e1 = nullptr;
    float ms = 0.f;
    if (!rc) {
        hipError_t e = hipMemset(a, 0, (size_t)count * 16);
        if (e == hipSuccess) e = hipEventCreate(&e0);
        if (e == hipSuccess) e = hipEventCreate(&e1);
        const dim3 g((unsigned)((count + kBlock - 1) / kBlock));      // one element per thread (count <= 2^31 x 256 elements)
        if (e == hipSuccess) {
            hipLaunchKernelGGL(k_copy16, g, dim3(kBlock), 0, nullptr, (const double2 *)a, b.get(), count);      // warm-up
            e = hipEventRecord(e0, nullptr);
            for (int r = 0; r < reps; ++r) hipLaunchKernelGGL(k_copy16, g, dim3(kBlock), 0, nullptr, (const double2 *)a, b.get(), count);
            if (e == hipSuccess) e = hipEventRecord(e1, nullptr);
            if (e == hipSuccess) e = hipEventSynchronize(e1);
            if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
            // the runtime's own device-to-device copy: whichever of the two is faster is "the achievable rate"
            float ms2 = 0.f;
            if (e == hipSuccess) e = hipMemcpyAsync(b, a, (size_t)count * 16, hipMemcpyDeviceToDevice, nullptr);
            if (e == hipSuccess) e = hipEventRecord(e0, nullptr);
            for (int r = 0; r < reps && e == hipSuccess; ++r) e = hipMemcpyAsync(b, a, (size_t)count * 16, hipMemcpyDeviceToDevice, nullptr);
            if (e == hipSuccess) e = hipEventRecord(e1, nullptr);
            if (e == hipSuccess) e = hipEventSynchronize(e1);
            if (e == hipSuccess) e = hipEventElapsedTime(&ms2, e0, e1);
            if (e == hipSuccess && ms2 > 0.f && ms2 < ms) ms = ms2;
        }
        if (e != hipSuccess) rc = fail(RR_E_HIP, hipGetErrorString(e));
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (rc) return rc;
    *gbps = 2.0 * (double)count * 16.0 * reps / ((double)ms * 1e-3) / 1e9;      // bytes read + bytes written
    return RR_OK;
}

// ---- rows between a file and the device (the routers' qlateral / discharge files) ----
//
// A (rows, row_bytes) block that lies in a file at `file_offset` with `file_pitch` bytes from row to row (NetCDF-3: a fixed variable is
// contiguous, a record variable has the other record variables of each record between its rows) goes to / comes from a device array without
// ever existing as a host array: reader threads pread() whole rows into three pinned chunks while the copy engine uploads the chunk
// before (downloads: the copy engine fills a chunk while writer threads pwrite() the one before).  Byte order is the device's business
// (rr_plan_set_row_format).  Returns when the block has moved.
namespace {
struct RowPipe {
    static constexpr int kChunks = 3, kThreads = 4;
    char *pin[kChunks] = {nullptr, nullptr, nullptr};
    hipEvent_t ev[kChunks] = {nullptr, nullptr, nullptr};
    hipStream_t st = nullptr;
    int64_t cap = 0;
    ~RowPipe()
    {
        for (int k = 0; k < kChunks; ++k) { if (pin[k]) (void)hipHostFree(pin[k]); if (ev[k]) (void)hipEventDestroy(ev[k]); }
        if (st) (void)hipStreamDestroy(st);
    }
    int prepare(int64_t bytes)
    {
        if (!st) HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        for (int k = 0; k < kChunks; ++k) if (!ev[k]) HIPCHK(hipEventCreateWithFlags(&ev[k], hipEventDisableTiming));
        if (cap >= bytes) return RR_OK;
        for (int k = 0; k < kChunks; ++k) {
            if (pin[k]) { (void)hipHostFree(pin[k]); pin[k] = nullptr; }
            if (hipHostMalloc((void **)&pin[k], (size_t)bytes, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); cap = 0; return fail(RR_E_ALLOC, "rr_rows_*: pinned staging could not be allocated"); }
        }
        cap = bytes;
        return RR_OK;
    }
};
thread_local RowPipe g_row_pipe;

// rows [r0, r1) of the file block <-> packed rows in `buf`, split over the threads; false on a short read / write
bool file_rows(int fd, bool write, char *buf, int64_t file_offset, int64_t file_pitch, int64_t row_bytes, int64_t r0, int64_t r1)
{
    const int64_t rows = r1 - r0;
    const int nt = (int)std::max<int64_t>(1, std::min<int64_t>(RowPipe::kThreads, rows));
    std::vector<std::thread> pool;
    std::vector<int> ok((size_t)nt, 1);
    for (int t = 0; t < nt; ++t)
        pool.emplace_back([&, t] {
            for (int64_t r = r0 + rows * t / nt; r < r0 + rows * (t + 1) / nt; ++r) {
                char *p = buf + (r - r0) * row_bytes;
                int64_t done = 0;
                while (done < row_bytes) {
                    const ssize_t got = write ? pwrite(fd, p + done, (size_t)(row_bytes - done), (off_t)(file_offset + r * file_pitch + done))
                                              : pread(fd, p + done, (size_t)(row_bytes - done), (off_t)(file_offset + r * file_pitch + done));
                    if (got <= 0) { ok[t] = 0; return; }
                    done += got;
                }
            }
        });
    for (auto &th : pool) th.join();
    for (int v : ok) if (!v) return false;
    return true;
}
}  // namespace

static int rows_transfer(int device, bool upload, void *dev, int64_t dev_pitch, const char *path, int64_t file_offset, int64_t file_pitch, int64_t row_bytes,
                         int64_t n_rows, void *stream)
{
    if (device < 0 || device >= rr_device_count()) return fail(RR_E_NO_DEVICE, "rr_rows_*: no such HIP device");
    if (!dev || !path || row_bytes < 1 || n_rows < 0 || dev_pitch < row_bytes || file_pitch < row_bytes || file_offset < 0) return fail(RR_E_INVALID, "rr_rows_*: bad argument");
    if (n_rows == 0) return RR_OK;
    HIPCHK(hipSetDevice(device));
    const int fd = open(path, upload ? O_RDONLY : O_WRONLY);
    if (fd < 0) return fail(RR_E_INVALID, std::string("rr_rows_*: cannot open ") + path);
    RowPipe &R = g_row_pipe;
    const int64_t chunk_rows = std::max<int64_t>(1, (int64_t{64} << 20) / row_bytes);      // 64 MB: long enough for the copy engine, short enough to overlap
    int rc = R.prepare(chunk_rows * row_bytes);
    const int64_t n_chunks = (n_rows + chunk_rows - 1) / chunk_rows;
    hipError_t e = hipSuccess;
    if (!rc) {      // the block is used by / comes from work on the caller's stream (NULL: the default stream)
        hipEvent_t fence = nullptr;
        e = hipEventCreateWithFlags(&fence, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventRecord(fence, (hipStream_t)stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(R.st, fence, 0);
        if (fence) (void)hipEventDestroy(fence);
    }
    bool io_ok = true;
    if (!rc && e == hipSuccess) {
        if (upload) {
            for (int64_t c = 0; c < n_chunks && io_ok && e == hipSuccess; ++c) {
                const int k = (int)(c % RowPipe::kChunks);
                const int64_t r0 = c * chunk_rows, r1 = std::min(n_rows, r0 + chunk_rows);
                if (c >= RowPipe::kChunks) e = hipEventSynchronize(R.ev[k]);      // the chunk that used this buffer has left
                if (e != hipSuccess) break;
                io_ok = file_rows(fd, false, R.pin[k], file_offset, file_pitch, row_bytes, r0, r1);
                if (!io_ok) break;
                e = hipMemcpy2DAsync((char *)dev + r0 * dev_pitch, (size_t)dev_pitch, R.pin[k], (size_t)row_bytes, (size_t)row_bytes, (size_t)(r1 - r0), hipMemcpyHostToDevice, R.st);
                if (e == hipSuccess) e = hipEventRecord(R.ev[k], R.st);
            }
            if (e == hipSuccess) e = hipStreamSynchronize(R.st);
        } else {
            // chunk c is downloaded while chunk c - 1 is written
            auto fetch = [&](int64_t c) {
                const int k = (int)(c % RowPipe::kChunks);
                const int64_t r0 = c * chunk_rows, r1 = std::min(n_rows, r0 + chunk_rows);
                hipError_t ee = hipMemcpy2DAsync(R.pin[k], (size_t)row_bytes, (const char *)dev + r0 * dev_pitch, (size_t)dev_pitch, (size_t)row_bytes, (size_t)(r1 - r0), hipMemcpyDeviceToHost, R.st);
                if (ee == hipSuccess) ee = hipEventRecord(R.ev[k], R.st);
                return ee;
            };
            e = fetch(0);
            for (int64_t c = 0; c < n_chunks && io_ok && e == hipSuccess; ++c) {
                const int k = (int)(c % RowPipe::kChunks);
                if (c + 1 < n_chunks) e = fetch(c + 1);      // (buffer (c + 1) % 3 was written out two iterations ago)
                if (e == hipSuccess) e = hipEventSynchronize(R.ev[k]);
                if (e != hipSuccess) break;
                const int64_t r0 = c * chunk_rows, r1 = std::min(n_rows, r0 + chunk_rows);
                io_ok = file_rows(fd, true, R.pin[k], file_offset, file_pitch, row_bytes, r0, r1);
            }
        }
    }
    (void)close(fd);
    if (R.st && (rc || e != hipSuccess || !io_ok)) (void)hipStreamSynchronize(R.st);      // a failed transfer leaves no copy in flight behind: the caller may free the rows
    if (rc) return rc;
    if (e != hipSuccess) return fail(RR_E_HIP, std::string("rr_rows_*: ") + hipGetErrorString(e));
    if (!io_ok) return fail(RR_E_INVALID, std::string("rr_rows_*: short read or write on ") + path);
    return RR_OK;
}

int rr_rows_upload(int device, void *dst_dev, int64_t dst_pitch, const char *path, int64_t file_offset, int64_t file_pitch, int64_t row_bytes, int64_t n_rows, void *stream)
{
    return rows_transfer(device, true, dst_dev, dst_pitch, path, file_offset, file_pitch, row_bytes, n_rows, stream);
}

int rr_rows_download(int device, const void *src_dev, int64_t src_pitch, const char *path, int64_t file_offset, int64_t file_pitch, int64_t row_bytes, int64_t n_rows, void *stream)
{
    return rows_transfer(device, false, const_cast<void *>(src_dev), src_pitch, path, file_offset, file_pitch, row_bytes, n_rows, stream);
}

int rr_dev_synchronize(int device)
{
    if (device < 0 || device >= rr_device_count()) return fail(RR_E_NO_DEVICE, "rr_dev_synchronize: no such HIP device");
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipDeviceSynchronize());
    return RR_OK;
}

}  // extern "C"

// ---- adjoint of gridded runoff -> catchment inflow (rr_kernels_runoff_adjoint.hpp) ----

#include "rr_kernels_runoff_adjoint.hpp"      // here, at the end: the kernels above keep their place in the code object

extern "C" {

int rr_runoff_adjoint_work_bytes(int64_t n_rivers, int64_t n_points, int64_t T, int64_t *bytes)
{
    if (!bytes) return fail(RR_E_INVALID, "rr_runoff_adjoint_work_bytes: null out");
    *bytes = 0;
    if (n_rivers < 0 || n_points < 0 || T < 0 || n_rivers > 0x7FFFFFFFLL || n_points > 0x7FFFFFFFLL)
        return fail(RR_E_INVALID, "rr_runoff_adjoint_work_bytes: sizes out of range");
    const int64_t t_pad = (T + kRunoffRows - 1) / kRunoffRows * kRunoffRows;
    *bytes = n_rivers * t_pad * (int64_t)sizeof(double);      // Gs, river-major
    return RR_OK;
}

int rr_runoff_adjoint_dev(int device, int64_t n_rivers, int64_t n_points, int64_t T, const int32_t *indptr, const int32_t *indices,
                          const double *weights, const int32_t *t_indptr, const int32_t *t_pairs, const void *runoff, int runoff_is_f32,
                          int64_t stride_t, int64_t stride_p, const double *area, int flags, const double *grad_qlateral, void *grad_runoff,
                          int64_t grad_stride_t, double *grad_weights, void *work, int64_t work_bytes, void *stream)
{
    // what the arguments alone decide comes first, so that it is refused with or without a GPU
    if (n_rivers < 0 || n_points < 0 || T < 0 || n_rivers > 0x7FFFFFFFLL || n_points > 0x7FFFFFFFLL)
        return fail(RR_E_INVALID, "rr_runoff_adjoint_dev: sizes out of range");
    if (flags & RR_RUNOFF_KEEP_NAN) return fail(RR_E_INVALID, "rr_runoff_adjoint_dev: RR_RUNOFF_KEEP_NAN has no adjoint (the NaN fill is part of the mask)");
    if (!grad_runoff && !grad_weights) return fail(RR_E_INVALID, "rr_runoff_adjoint_dev: neither grad_runoff nor grad_weights is asked for");
    if (!indptr || !indices || !weights || !t_indptr || !t_pairs) return fail(RR_E_INVALID, "rr_runoff_adjoint_dev: null structure array");
    if (stride_t < 0 || stride_p < 0 || (grad_runoff && grad_stride_t < n_points))
        return fail(RR_E_INVALID, "rr_runoff_adjoint_dev: negative stride, or grad_stride_t shorter than n_points");
    if (device < 0 || device >= rr_device_count()) return fail(RR_E_NO_DEVICE, "rr_runoff_adjoint_dev: no such HIP device");
    HIPCHK(hipSetDevice(device));
    if (T == 0) return RR_OK;
    if (!runoff || !grad_qlateral) return fail(RR_E_INVALID, "rr_runoff_adjoint_dev: null array");
    const int64_t chunks = (T + kRunoffRows - 1) / kRunoffRows, t_pad = chunks * kRunoffRows;
    if (chunks > 65535) return fail(RR_E_UNSUPPORTED, "rr_runoff_adjoint_dev: more than 1,048,560 time steps in one call");
    const int64_t need = n_rivers * t_pad * (int64_t)sizeof(double);
    if (need > 0 && (!work || work_bytes < need))
        return fail(RR_E_STATE, "rr_runoff_adjoint_dev: work memory smaller than rr_runoff_adjoint_work_bytes (" + std::to_string(need) + " bytes)");
    if ((uintptr_t)work & 15) return fail(RR_E_INVALID, "rr_runoff_adjoint_dev: work memory must be 16-byte aligned");
    const hipStream_t st = (hipStream_t)stream;
    double *gs = static_cast<double *>(work);
    const unsigned river_blocks = (unsigned)((n_rivers + kBlock - 1) / kBlock), point_blocks = (unsigned)((n_points + kBlock - 1) / kBlock);
    const bool vec = stride_t == 1 && stride_p % kRunoffRows == 0 && stride_p >= t_pad && ((uintptr_t)runoff & 15) == 0;
    if (n_rivers > 0) {
#define RR_RUNOFF_ADJ_RIVER(RT_, VEC_)                                                                                                        \
    hipLaunchKernelGGL((k_runoff_adjoint_river<RT_, VEC_>), dim3(river_blocks, (unsigned)chunks), dim3(kBlock), 0, st, indptr, indices, weights, \
                       (const RT_ *)runoff, stride_t, stride_p, area, flags, grad_qlateral, gs, n_rivers, T, t_pad)
        if (runoff_is_f32) { if (vec) RR_RUNOFF_ADJ_RIVER(float, true); else RR_RUNOFF_ADJ_RIVER(float, false); }
        else { if (vec) RR_RUNOFF_ADJ_RIVER(double, true); else RR_RUNOFF_ADJ_RIVER(double, false); }
#undef RR_RUNOFF_ADJ_RIVER
        HIPCHK(hipGetLastError());
    }
    if (grad_runoff && n_points > 0) {      // without rivers every column is empty and the pass writes the zeros
        const dim3 g(point_blocks, (unsigned)((chunks + kRunoffAdjChunks - 1) / kRunoffAdjChunks));
        if (runoff_is_f32)
            hipLaunchKernelGGL(k_runoff_adjoint_point<float>, g, dim3(kBlock), 0, st, indptr, weights, t_indptr, t_pairs, gs, (float *)grad_runoff,
                               grad_stride_t, n_rivers, n_points, T, t_pad);
        else
            hipLaunchKernelGGL(k_runoff_adjoint_point<double>, g, dim3(kBlock), 0, st, indptr, weights, t_indptr, t_pairs, gs, (double *)grad_runoff,
                               grad_stride_t, n_rivers, n_points, T, t_pad);
        HIPCHK(hipGetLastError());
    }
    if (grad_weights && n_rivers > 0) {
#define RR_RUNOFF_ADJ_WEIGHT(RT_, VEC_)                                                                                                       \
    hipLaunchKernelGGL((k_runoff_adjoint_weight<RT_, VEC_>), dim3(river_blocks), dim3(kBlock), 0, st, indptr, indices, (const RT_ *)runoff,      \
                       stride_t, stride_p, gs, grad_weights, n_rivers, T, t_pad)
        if (runoff_is_f32) { if (vec) RR_RUNOFF_ADJ_WEIGHT(float, true); else RR_RUNOFF_ADJ_WEIGHT(float, false); }
        else { if (vec) RR_RUNOFF_ADJ_WEIGHT(double, true); else RR_RUNOFF_ADJ_WEIGHT(double, false); }
#undef RR_RUNOFF_ADJ_WEIGHT
        HIPCHK(hipGetLastError());
    }
    return RR_OK;
}

}  // extern "C"
