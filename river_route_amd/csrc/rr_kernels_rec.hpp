// rr_kernels_rec.hpp -- the record passes: params-order rows <-> tick-indexed records, with the fused float32 / convolution forms, and the stand-alone resample-cast.
// Part of the one translation unit rr_engine.hip builds (included from there, in order; not a stand-alone header).
#pragma once

namespace {

// ---- record permutation (one pass each way), see k_tile ----
// Column i of the params-order rows is position p = inv[i] with lag L = 16 * sh + o.  Tick-row r of that column (tick-row =
// routing sub-step: runoff row r / nsub, sub-step r % nsub) is slot (r + L) % 16 of record (r + L) / 16, so with B = 8 records
// per batch the 128 tick-rows [128 j - o, 128 j + 128 - o) are exactly the records B j + sh .. B j + sh + B - 1.  k_rec_in
// reads the runoff rows behind the 143 tick-rows [128 j - 15, 128 j + 128) of a 32-column tile coalesced into LDS (all loads
// in flight before the first LDS write) and writes B whole 128-byte records per column (8 lanes x 16 B per record), every
// sub-step slot of a row holding the row's lateral value; k_rec_out reads B + 1 records per column the same way and writes
// the tile's rows of the batch coalesced: the slot of a row's LAST sub-step holds the row's mean discharge.  B = 16 halves
// the share of rows / records read twice at a batch's edge but needs 72 KB of LDS per workgroup: 1 % slower when every row
// comes from HBM (380 vs 384 ms per year), faster only while a short cyclic forcing array is found in a cache
// (profiles/r02_rec_batch.txt).  A workgroup walking several consecutive batches in the same LDS tile (a.batches) reads the
// edge once per launch instead: DESIGN.md section 4.
// Tile shapes, each the winner of an A/B on the GPU box: 256 threads (128 to 1,024: within 0.5 %, profiles/r03_rec_threads_ab.txt),
// 32 columns (16 to 64: the same, r03_rec_tile_width_ab.txt), one tile per workgroup (persistent workgroups with the next tile's
// loads in flight: 427 / 469 us per 128 rows against 419 / 434, r03_rec_persistent_ab.txt), 8 records per batch (r02_rec_batch.txt).
constexpr int kRecCols = 32, kRecBatch = 8, kRecThreads = 256;
constexpr int kRecInThreads = kRecThreads, kRecOutThreads = kRecThreads;      // workgroup sizes of k_rec_in / k_rec_out
constexpr int kRecInCols = kRecCols, kRecOutCols = kRecCols;                  // columns of a tile of k_rec_in / k_rec_out
constexpr int kRecRows = 16 * kRecBatch;    // tick-rows of one batch
// Batches one launch of k_rec_in / k_rec_out walks in a long call (rr_exec.hpp: choose_schedule, session_advance_tile): the rows and
// records at a batch's edge are read once per launch instead of once per batch, in the same LDS tile.  Eight by default: 259.8 against
// 263.9 ms per year at 1M reaches for 4.3 GB more ring, inside three times the parent's spread (profiles/r08_rec_stream_ab.txt): four.
constexpr int kRecLaunchBatches = 4, kRecMaxLaunchBatches = 8;

// Cache policy of the four access streams of k_rec_in / k_rec_out, one hint per stream: true = non-temporal (the `nt` bit of the
// global load / store: the line is marked for early eviction), false = the default policy.  Every row and every record of these
// passes is used once.  A hint changes the instruction's cache bits only, never what a wave issues or in what order (the batch loop
// of k_rec_in stays sixteen loads, eight stores, a barrier, vmcnt(23) ... vmcnt(8); registers, LDS and scratch are unchanged).  The
// fused convolution and gridded-runoff in-passes keep the default (kRecStreamsDefault).  Measured at 1M reaches, each hint alone and
// together (profiles/r08_rec_stream_ab.txt), per year against 263.9 ms:
//   in_recs   k_rec_in 86.3 -> 84.5 ms, the year -3.8 ms: the records no longer displace the row lines still to be read;
//   out_recs  k_rec_out 80.8 -> 74.8 ms, the year -5.8 ms, where the discharge goes to a short cyclic sink (bench.py's 128 rows, a
//             streaming caller's ring): the sink's lines stay in L2 and are overwritten there (273 -> 211 GB written back); with
//             4,096 sink rows nothing is rewritten in time and the hint changes nothing (293.5 against 292.7 ms);
//   both      -8.4 ms (255.5): kept.  in_rows: k_rec_in 86.3 -> 101.2 ms, out_rows: k_rec_out 80.8 -> 94.2 ms: both refused.
struct RecStreamPolicy {
    bool in_rows;       // k_rec_in: params-order rows, loaded
    bool in_recs;       // k_rec_in: records, stored
    bool out_recs;      // k_rec_out: records, loaded
    bool out_rows;      // k_rec_out: params-order rows (float64 or float32 means), stored
};
constexpr RecStreamPolicy kRecStreamsDefault{false, false, false, false};
constexpr RecStreamPolicy kRecStreams{false, true, true, false};      // (stream_load / stream_store: rr_common.hpp)

struct RecPermArgs {
    double *rec;
    Div32 rec_chunks;
    int64_t n, np, T, total, batch;   // T runoff rows, total = T * nsub tick-rows
    Div32 nsub;
    const int2 *colmeta;      // per params column: {position, lag}
    const double *scale;      // c4dt in PARAMS order (RapidMuskingum: the ring holds c4dt * lateral) or NULL
    RowView rows;             // params-order rows (source of k_rec_in, destination of k_rec_out)
    const float *rows_in32;   // k_rec_in<..., IN32>: the source rows are float32 (a qlateral file stored that way: 4 B read instead of 8, exact in float64); same shape as `rows`
    float *rows32;            // k_rec_out: float32 destination with `factor` rows averaged (router post-processing), or NULL
    Div32 factor;
    const int32_t *cols;      // k_rec_out: column of the destination rows each of the n records' columns goes to (the holes of the direct row path), or NULL: column i
    int32_t swizzle;          // column tiles in XCD-contiguous order (rr_common.hpp: xcd_swizzle)
    int32_t clamp;            // k_rec_out: 0 records hold final values (sub-steps), 1 clamp at zero, 2 clamp all but headwater columns (UnitMuskingum)
    uint32_t in32_sel, out32_sel;   // byte selectors of the float32 rows (rr_plan_set_row_format): kSelNative, or kSelSwap for a big-endian file's rows
    int32_t batches;          // k_rec_in / k_rec_out: consecutive batches from `batch` on, walked by each workgroup (0 or 1: one)
    // k_rec_in<..., HW>: the columns flagged kColInpass leave as DISCHARGE records (see k_rec_in)
    const double *hw_coef;    // per params column {c1row, c2, c3}: the coefficients k_tile's general table holds for the column's position (the walk reads c3)
    double *hw_carry;         // per params column: the discharge of the column's last routed row, from launch to launch (the call's initial state before the first)
};

// Ensembles (rr_kernels_tile.hpp: member_chunk0): member blockIdx.y has its rows at m * row_pitch elements from the first member's and its record
// ring at m * ring_stride doubles; the member-batched passes (ENS) are the single-member ones on those.  scale_pitch: member m's scale
// (c4dt in params order) at m * scale_pitch doubles -- a parameter ensemble's (rr_rapid_route_members_dev); 0: the plan's, shared.
struct RecEnsArgs : RecPermArgs {
    int64_t ring_stride, row_pitch, scale_pitch;
};
template <bool ENS> using RecArgsOf = typename std::conditional<ENS, RecEnsArgs, RecPermArgs>::type;
__device__ __forceinline__ const RecPermArgs &member_args(const RecPermArgs &a) { return a; }
__device__ __forceinline__ RecPermArgs member_args(const RecEnsArgs &e)      // the pass's rows: k_rec_in's source (float64 or float32), k_rec_out's destination
{
    RecPermArgs a = e;
    const int64_t m = blockIdx.y;
    a.rec += m * e.ring_stride;
    a.rows.base += m * e.row_pitch;
    if (a.rows_in32) a.rows_in32 += m * e.row_pitch;
    if (a.rows32) a.rows32 += m * e.row_pitch;
    if (a.scale) a.scale += m * e.scale_pitch;
    return a;
}

constexpr int32_t kColHeadwater = 1 << 30;      // colmeta[].y: lag | this flag
constexpr int32_t kColInpass = 1 << 29;         // colmeta[].y: a headwater the in-pass may route (rr_plan.hpp: mark_inpass_headwaters)

constexpr int kRecTileRows = 16 * kRecBatch + 15;      // tick-rows behind one batch of records
constexpr int kRecTileLd = kRecCols + 1;

// Ring chunk `first + ahead`, first < chunks and ahead = lag / 16 + a record of the batch: the ring is longer than the deepest
// lag plus two batches (rr_exec.hpp: choose_schedule), so one subtraction wraps it -- the division costs 12 VALU instructions,
// and the fused convolution is bound by those (profiles/r03_uh_diet.txt).
__device__ __forceinline__ uint32_t ring_chunk(const Div32 &chunks, uint32_t first, uint32_t ahead)
{
    const uint32_t c = first + ahead;
    return c >= chunks.d ? c - chunks.d : c;
}

// Second half of the in-pass: the LDS tile (row = runoff row - row_first, kRecTileLd doubles per row) becomes records.
// BATCH records per column of batch `batch`, from tick-row kRecRows * batch - 15 on (the fused convolution takes two batches at a time).
// smeta / sscale: the tile's column metadata and scale in LDS (k_rec_in keeps them there: loaded with the rows, no registers
// held across the stores), or NULL: read from the plan's arrays.
template <bool SUB, int THREADS = kRecThreads, int BATCH = kRecBatch, bool LDSMETA = false, int COLS = kRecCols, bool NT = kRecStreamsDefault.in_recs>
__device__ __forceinline__ void write_records(const RecPermArgs &a, const double *tile, int64_t col0, int64_t batch, int64_t tick_first, int64_t row_first,
                                              const int2 *smeta = nullptr, const double *sscale = nullptr)
{
    constexpr int R = 16 * BATCH + 15;
    const int tid = threadIdx.x;
    static_assert(COLS * BATCH * 8 % THREADS == 0, "records of a tile must divide among the threads");
    constexpr int IT = COLS * BATCH * 8 / THREADS;
    int2 meta[LDSMETA ? 1 : IT];
    double f[LDSMETA ? 1 : IT];
    if constexpr (!LDSMETA) {
#pragma unroll
        for (int it = 0; it < IT; ++it) {     // all metadata loads first: they are independent
            const int64_t i = col0 + (it * THREADS + tid) / (8 * BATCH);
            meta[it] = i < a.n ? a.colmeta[i] : make_int2(-1, 0);
        }
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int64_t i = col0 + (it * THREADS + tid) / (8 * BATCH);
            f[it] = (a.scale && i < a.n) ? a.scale[i] : 1.0;
        }
    }
    const uint32_t chunk_first = a.rec_chunks.mod((uint32_t)kRecBatch * (uint32_t)batch);
    // LDSMETA (k_rec_in): every column of the tile is one to store (a column past the end is a replica of the last), and without sub-steps
    // the stores are one straight run that no lane skips: the waits for loads issued before them can count them
#pragma unroll(LDSMETA ? (SUB ? 2 : IT) : IT)
    for (int it = 0; it < IT; ++it) {
        const int piece = it * THREADS + tid;       // (column, record, 16-byte part): 8 consecutive lanes = one record
        const int c = piece / (8 * BATCH), k = (piece >> 3) % BATCH, part = piece & 7;
        const int2 m = LDSMETA ? smeta[c] : meta[LDSMETA ? 0 : it];
        const double scale = LDSMETA ? sscale[c] : f[LDSMETA ? 0 : it];
        const int32_t p = m.x;
        if (!LDSMETA && p < 0) continue;
        const int32_t lag = m.y & kLagMask;
        const int o = lag & 15;
        const uint32_t chunk = ring_chunk(a.rec_chunks, chunk_first, (uint32_t)(lag >> 4) + k);
        const int r = 15 - o + 16 * k + 2 * part;       // tick-row tick_first + r
        double v0, v1;
        if (SUB) {
            const int64_t t0 = tick_first + r, t1 = t0 + 1;
            uint32_t s;
            const int r0 = t0 < 0 ? 0 : (int)((int64_t)a.nsub.div((uint32_t)t0, s) - row_first);
            const int r1 = t1 < 0 ? 0 : (int)((int64_t)a.nsub.div((uint32_t)t1, s) - row_first);
            v0 = tile[min(r0, R - 1) * (COLS + 1) + c] * scale; v1 = tile[min(r1, R - 1) * (COLS + 1) + c] * scale;
        } else {
            v0 = tile[r * (COLS + 1) + c] * scale; v1 = tile[(r + 1) * (COLS + 1) + c] * scale;
        }
        double2 *dst = reinterpret_cast<double2 *>(a.rec + rec_elem(chunk, a.np, p)) + part;
        typedef double d2 __attribute__((ext_vector_type(2)));
        stream_store<NT>(reinterpret_cast<d2 *>(dst), d2{v0, v1});
    }
}

// One column tile per workgroup: all of its row loads in flight before the first LDS write, the tile's column metadata and
// scale travelling with the rows into LDS (no registers held across the stores).  The rows alone read in 186 us per 128 rows at 1M
// reaches, the records alone store in 199 us, the pass takes 415: within 7 % of the two one after the other
// (profiles/r03_rec_probe.txt, r03_alias_kernel_times.txt).
// a.batches consecutive batches of the tile per workgroup (session_advance_tile: rr_plan::rec_batches where the rows and ring slots
// are there): the 15 tick-rows before a later batch are the last 15 of the one before it, still in LDS -- moved to the tile's top,
// not read from HBM again (131.75 rows read per 128 at four batches instead of 143).  A later batch's row loads are all in flight
// before the previous batch's records leave; the column metadata and scale stay in LDS for the whole walk.
// Nothing in the batch loop may wait for those stores before it has to (the memory counter retires loads and stores in the order
// they were issued, and hipcc counts only what it can prove was issued), so, without sub-steps, every load and store of the pass is
// issued by every lane on every path:
//   * a column past the network's end is a REPLICA of column n - 1 (its loads are clamped there anyway): same rows, metadata, scale and
//     walk, and the same records stored to the same addresses -- no lane skips a store, and only the last tile has replicas;
//   * the tile is padded to a whole number of row groups (144 rows), so the first batch's last load is written by every lane instead of
//     staying pending in the lanes past row 142 (a register with a load pending is waited for when it is next written: that was the
//     wait at the top of the batch loop's load block);
//   * the eight record stores of a batch are one straight run, so the waits for the next batch's sixteen loads count them: the first
//     row is waited for with 23 operations still outstanding, the last with the eight stores.
// What a thread derives from its number (column, row group, addresses) is rebuilt from fresh_tid(tid) where it is used: kept across the batch
// loop those were 34 registers of hoisted row numbers, and the spills they caused were reloaded inside the loop -- a reload is a memory
// operation too and returns behind every store before it.
// HW (RapidMuskingum, one sub-step per row, the short tick): a headwater's discharge q+ = fma(c3, q, c4dt ql) depends on its own column
// only, and the whole column of the batch is here in LDS.  One thread per flagged column (kColInpass) walks the column's 128 tick-rows of
// the batch in time order and replaces the scaled lateral by the discharge, so the record k_tile receives is final: the position has zero
// coefficients and a ghost's flag in k_tile's tables of this mode, publishes the slot and never stores the record (DESIGN.md section
// 3c).  The arithmetic is the tick's own, q+ = fma(c1row, 0.0, fma(c2, 0.0, r)) with r = fma(c3, q, x) and the sums of a reach without
// upstream reaches (0.0) written out, evaluated as q+ = r + 0.0 -- the same double, bit for bit, for the columns the plan flags
// (mark_inpass_headwaters: c1row is +0.0 and c2 is finite, both tested on the bits):
//   c2 finite: c2 * 0.0 is a zero of either sign, so the inner fma is r + (+-0.0): r itself when r is not a zero (an infinity stays, a
//   NaN stays a NaN), a zero of some sign when r is one.  c1row = +0.0: c1row * 0.0 = +0.0, so the outer fma adds +0.0 to that: unchanged
//   when it is not a zero, and +0.0 when it is (round to nearest: -0.0 + +0.0 = +0.0).  r + 0.0 is r when r is not a zero and +0.0 when it is.
// Two dependent operations per row instead of three; nothing else is reassociated.  q is carried from batch to batch in LDS and from launch
// to launch in a.hw_carry; the call's first row starts from the caller's state, which the call puts there.  Rows outside the call keep what
// every column gets (0.0 * scale).  The rows a later batch of the walk keeps at the tile's top are exactly those the column has not routed
// yet (tile rows from 143 - o on, o = lag % 16).
__device__ __forceinline__ int32_t fresh_tid(int32_t v) { asm volatile("" : "+v"(v)); return v; }      // (rr_kernels_tile.hpp: fresh)

template <bool SUB, bool IN32 = false, bool ENS = false, bool HW = false>
__global__ __launch_bounds__(kRecInThreads, 4) void k_rec_in(const RecArgsOf<ENS> args)
{
    static_assert(!HW || (!SUB && !ENS), "headwaters are routed by the in-pass only with one sub-step per row, single member");
    const RecPermArgs &a = member_args(args);
    constexpr int R = kRecTileRows, G = kRecInThreads / kRecInCols;      // G rows of the tile loaded at once
    constexpr int RPT = (R + G - 1) / G;
    static_assert((kRecInCols & (kRecInCols - 1)) == 0 && (G & (G - 1)) == 0, "column and row group of a thread are bit fields of its number");
    __shared__ double tile[RPT * G * (kRecInCols + 1)];      // R rows and the padding of the last row group
    __shared__ int2 smeta[kRecInCols];
    __shared__ double sscale[kRecInCols];
    __shared__ double shw[3][HW ? kRecInCols : 1];      // HW: c3, q, and the scale write_records applies (1.0 to a routed column)
    const int tid = threadIdx.x;
    auto first_row = [&](int64_t tick_first) -> int64_t {      // runoff row of the tile's first tick-row
        uint32_t sub_unused;
        return SUB ? (int64_t)a.nsub.div((uint32_t)(tick_first < 0 ? 0 : tick_first), sub_unused) : tick_first;
    };
    int64_t tick_first = kRecRows * a.batch - 15;                 // may be negative in the first batch
    int64_t row_first = first_row(tick_first);
    const int need = SUB ? (int)((uint32_t)(R - 1) / a.nsub.d) + 2 : R;     // runoff rows behind the batch's tick-rows
    const uint32_t n_tiles = (uint32_t)((a.n + kRecInCols - 1) / kRecInCols);
    if (blockIdx.x >= n_tiles) return;
    const int64_t col0 = (int64_t)(a.swizzle ? xcd_swizzle(blockIdx.x, n_tiles) : blockIdx.x) * kRecInCols;
    // branch-free: out-of-range rows are clamped here and zeroed on the way into LDS; a column past the end is column n - 1 once more
    auto col_of = [&](int t) -> int64_t { return min(col0 + (t & (kRecInCols - 1)), a.n - 1); };
    auto group_of = [](int t) -> int { return (t / kRecInCols) & (G - 1); };
    auto load = [&](int64_t t, int64_t i) -> double {
        const int64_t off = a.rows.offset(t < 0 ? 0 : (t >= a.T ? a.T - 1 : t)) + i;
        if constexpr (IN32) return (double)f32_from_file(stream_load<kRecStreams.in_rows>(a.rows_in32 + off), a.in32_sel);
        else return stream_load<kRecStreams.in_rows>(a.rows.base + off);
    };
    {
        const int c = tid & (kRecInCols - 1), r0 = group_of(tid);
        const int64_t i = col_of(tid);
        double v[RPT];
        // the column's words first, by every thread (the row loads' waits then cover them on every path); thread c puts them into LDS
        const int2 cm = a.colmeta[i];
        const double cs = a.scale ? a.scale[i] : 1.0;
        double hc3 = 0.0, hq = 0.0;
        if constexpr (HW) { hc3 = a.hw_coef[3 * i + 2]; hq = a.hw_carry[i]; }      // (params order: these loads wait for nothing)
#pragma unroll
        for (int q = 0; q < RPT; ++q) v[q] = load(row_first + min(r0 + q * G, need - 1), i);
#pragma unroll
        for (int q = 0; q < RPT; ++q) {
            const int r = r0 + q * G;
            const int64_t row = row_first + r;
            tile[r * (kRecInCols + 1) + c] = (row >= 0 && row < a.T) ? v[q] : 0.0;      // (r < RPT * G: the padding is written, never read)
        }
        if (tid < kRecInCols) {
            smeta[c] = cm; sscale[c] = cs;
            if constexpr (HW) { shw[0][c] = hc3; shw[1][c] = hq; shw[2][c] = (cm.y & kColInpass) ? 1.0 : cs; }
        }
    }
    __syncthreads();
    // HW: the flagged columns of the batch in the tile, lateral -> discharge.  Eight rows at a time through registers, so that the
    // serial chain is a multiply-add and an add per row and not an LDS round trip.
    auto route_headwaters = [&](int64_t first) {      // first: tick-row of the tile's row 0
        const int t = fresh_tid(tid);
        if (t >= kRecInCols) return;
        const int2 m = smeta[t];
        if (!(m.y & kColInpass)) return;
        const double c3 = shw[0][t], sc = sscale[t];
        double q = shw[1][t];
        const int r_first = 15 - (m.y & 15);      // the column's rows of the batch: [r_first, r_first + 128)
        double *col = tile + r_first * (kRecInCols + 1) + t;
        const int64_t t_first = first + r_first;
        constexpr int kBlk = 8;      // rows per register block
#pragma unroll 1
        for (int b = 0; b < kRecRows; b += kBlk) {
            double x[kBlk];
#pragma unroll
            for (int k = 0; k < kBlk; ++k) x[k] = col[(b + k) * (kRecInCols + 1)] * sc;
            const int64_t t0 = t_first + b;
            if (t0 >= 0 && t0 + kBlk <= a.T) {
#pragma unroll
                for (int k = 0; k < kBlk; ++k) { q = __builtin_fma(c3, q, x[k]) + 0.0; x[k] = q; }
            } else {      // the call's first and last rows: a row outside the call is not routed
#pragma unroll
                for (int k = 0; k < kBlk; ++k) {
                    const bool in = t0 + k >= 0 && t0 + k < a.T;
                    const double qn = __builtin_fma(c3, q, x[k]) + 0.0;
                    q = in ? qn : q; x[k] = in ? qn : x[k];
                }
            }
#pragma unroll
            for (int k = 0; k < kBlk; ++k) col[(b + k) * (kRecInCols + 1)] = x[k];
        }
        shw[1][t] = q;
    };
    const double *wscale = HW ? shw[2] : sscale;      // the scale on the way out
    // (routed as soon as a batch's tile is whole, before the next batch's loads are issued: beside sixteen loads in flight the walk's
    // registers do not fit)
    if constexpr (HW) { route_headwaters(tick_first); __syncthreads(); }
    const int nb = a.batches > 1 ? a.batches : 1;
    for (int b = 1; b < nb; ++b) {
        // the next batch's tile, rows [row_next, row_next + need): its first `keep` rows are this tile's last -- 15 without sub-steps, with
        // them at most 17 (a tile spans 142 / nsub + 2 rows, the next starts at least 113 / nsub - 1 rows further: KPT * G = 24 is room enough)
        constexpr int NPT = kRecRows / G, KPT = 3;      // new rows (at most 128) / kept rows per thread
        const int64_t tick_next = tick_first + kRecRows, row_next = first_row(tick_next);
        const int shift = (int)(row_next - row_first), keep = max(need - shift, 0);
        const int t = fresh_tid(tid), c = t & (kRecInCols - 1), r0 = group_of(t);
        double v[NPT], kv[KPT];
        {
            const int64_t i = col_of(t);
#pragma unroll
            for (int q = 0; q < NPT; ++q) {
                const int r = keep + r0 + q * G;      // without sub-steps 15 + r0 + 8 q < 143: every lane loads
                if (!SUB || r < need) v[q] = load(row_next + r, i);
            }
        }
        write_records<SUB, kRecInThreads, kRecBatch, true, kRecInCols, kRecStreams.in_recs>(a, tile, col0, a.batch + b - 1, tick_first, row_first, smeta, wscale);
#pragma unroll
        for (int q = 0; q < KPT; ++q) {
            const int r = r0 + q * G;
            if (r < keep) kv[q] = tile[(shift + r) * (kRecInCols + 1) + c];
        }
        __syncthreads();      // every record of the batch has been read out of the tile
#pragma unroll
        for (int q = 0; q < KPT; ++q) {
            const int r = r0 + q * G;
            if (r < keep) tile[r * (kRecInCols + 1) + c] = kv[q];
        }
#pragma unroll
        for (int q = 0; q < NPT; ++q) {
            const int r = keep + r0 + q * G;
            const int64_t row = row_next + r;
            if (!SUB || r < need) tile[r * (kRecInCols + 1) + c] = (row >= 0 && row < a.T) ? v[q] : 0.0;
        }
        __syncthreads();
        tick_first = tick_next; row_first = row_next;
        if constexpr (HW) { route_headwaters(tick_first); __syncthreads(); }
    }
    if constexpr (HW) {
        const int t = fresh_tid(tid);
        if (t < kRecInCols && col0 + t < a.n && (smeta[t].y & kColInpass)) a.hw_carry[col0 + t] = shw[1][t];      // (written by this thread; a replica writes nothing)
    }
    write_records<SUB, kRecInThreads, kRecBatch, true, kRecInCols, kRecStreams.in_recs>(a, tile, col0, a.batch + nb - 1, tick_first, row_first, smeta, wscale);
}

// The in-pass with the unit-hydrograph convolution fused in (UnitHydrograph.py:93-107, direct form): the tile is COMPUTED
// from the runoff-depth rows instead of loaded, so the convolved lateral never exists as (T, n) rows in HBM (written by the
// convolution kernel, read again by k_rec_in: 16 B per value).  The block loads the depth rows behind its 143 tick-rows plus
// the n_ks - 1 before them and the kernel's taps into LDS; thread (column, group of 18 rows) pulls its window of 18 + NK - 1
// depth values into registers and accumulates 18 outputs x NK taps with static indices (NK = n_ks padded with zero taps);
// the outputs replace the depth tile in LDS and leave as records.  out[t] = [t < n_ks] state[t] + sum_k kernel[k] depth[t - k].
struct UhArgs {
    const double *kernel, *state;     // (n_ks, n) taps and carried-in state, params order
    int32_t n_ks;
};
// Columns of a tile of the fused convolution: 16 (128-byte row pieces) against the 32 of the plain passes: 52.6 against 55.2 ms
// for BASELINE config 4 (profiles/r03_small_networks_and_uh16.txt).
// BATCH = batches of kRecBatch records (128 tick-rows) per launch, 1 or 2: the n_ks - 1 depth rows before a tile and the taps
// are read once per tile, so the pair moves 19.4 B per value where the single batch moves 22.9 (n_ks = 48); a workgroup has
// 32 threads per record: 16 columns x (2 x records) groups of 9 rows.
constexpr int kUhCols = 16, kUhTileLd = kUhCols + 1;
constexpr int kUhMaxBatches = 2;
constexpr int uh_threads(int batches) { return 32 * kRecBatch * batches; }
constexpr int uh_tile_rows(int batches) { return 16 * kRecBatch * batches + 15; }
constexpr int uh_groups(int batches) { return uh_threads(batches) / kUhCols; }
constexpr int uh_rows_per_thread(int batches) { return (uh_tile_rows(batches) + uh_groups(batches) - 1) / uh_groups(batches); }
constexpr int uh_win_rows(int batches) { return uh_groups(batches) * uh_rows_per_thread(batches); }      // rows the windows start in: one more than the tile has
// depth rows [win_rows + nk - 1] (the last ones are padding: the windows of the threads past the tile's end reach them) | taps [nk]
constexpr size_t rec_in_uh_lds_bytes(int nk, int batches) { return (size_t)((uh_win_rows(batches) + nk - 1) + nk) * kUhTileLd * sizeof(double); }

// The kernel issues 432 multiply-adds per thread at NK = 48 and used to issue 670 other vector instructions around them: a
// division per cyclic row and record, clamps and 64-bit compares per LDS access (SQ_INSTS_VALU, profiles/r03_b_sq_counters_*);
// at 16 lanes per cycle that was 450 of its 770 us.  Now: LDS accesses at compile-time offsets from one address per thread
// (the tile is padded instead of the indices clamped), the cyclic rows stepped from one division, 32-bit range tests, the
// carried-in state behind a branch the whole launch takes the same way.
template <bool SUB, int NK, int BATCHES, bool IN32 = false>      // IN32: the depth rows are float32 (a.rows_in32, the shape of a.rows)
__global__ __launch_bounds__(uh_threads(BATCHES)) void k_rec_in_uh(const RecPermArgs a, const UhArgs u)
{
    constexpr int R = uh_tile_rows(BATCHES), G = uh_groups(BATCHES), RP = uh_rows_per_thread(BATCHES);
    constexpr int ROWS = uh_win_rows(BATCHES) + NK - 1, DATA = R + NK - 1;      // depth rows in LDS / those that hold data
    extern __shared__ __attribute__((aligned(16))) double uh_lds[];
    double *dt = uh_lds;                          // [ROWS][kUhTileLd] depth rows row_first - (NK - 1) ...
    double *tp = uh_lds + ROWS * kUhTileLd;      // [NK][kUhTileLd] taps
    const int tid = threadIdx.x, c = tid % kUhCols, g = tid / kUhCols;
    const int64_t col0 = (int64_t)(a.swizzle ? xcd_swizzle(blockIdx.x, gridDim.x) : blockIdx.x) * kUhCols;
    const int64_t tick_first = kRecRows * a.batch - 15;
    uint32_t sub_unused;
    const int64_t row_first = SUB ? (int64_t)a.nsub.div((uint32_t)(tick_first < 0 ? 0 : tick_first), sub_unused) : tick_first;
    const int need = SUB ? (int)((uint32_t)(R - 1) / a.nsub.d) + 2 : R;
    const int64_t i = min(col0 + c, a.n - 1);
    const bool live = col0 + c < a.n;
    const int32_t tb = (int32_t)row_first - (NK - 1) + g;      // depth row of this thread's first load (negative in a call's first launch); T < 2^31
    {   // all loads in flight first (branch-free: rows outside the call and columns past the end load something valid and are zeroed afterwards)
        constexpr int DPT = (ROWS + G - 1) / G, TPT = (NK + G - 1) / G;
        double dv[DPT], tv[TPT];
        if constexpr (SUB) {
#pragma unroll
            for (int q = 0; q < DPT; ++q) {
                const int64_t t = row_first - (NK - 1) + min(g + q * G, need + NK - 2);
                const int64_t off = a.rows.offset(t < 0 ? 0 : (t >= a.T ? a.T - 1 : t)) + i;
                dv[q] = IN32 ? (double)f32_from_file(a.rows_in32[off], a.in32_sel) : a.rows.base[off];
            }
        } else {
            // load q reads the cyclic row (tb + G q - t0) mod rows: one division, for the first q whose row cannot be negative,
            // and steps of G mod rows either way from there (a row before the call's first steps to some row of the array: loaded, not used)
            constexpr int QM = (NK - 1 + 15 + G - 1) / G;
            static_assert(QM < DPT, "the tile is longer than the rows before it");
            const uint32_t d = a.rows.rows.d, step = a.rows.rows.mod((uint32_t)G);
            uint32_t m[DPT];
            m[QM] = a.rows.rows.mod((uint32_t)(tb + G * QM - (int32_t)a.rows.t0));
#pragma unroll
            for (int q = QM + 1; q < DPT; ++q) { const uint32_t x = m[q - 1] + step; m[q] = x >= d ? x - d : x; }
#pragma unroll
            for (int q = QM - 1; q >= 0; --q) m[q] = m[q + 1] >= step ? m[q + 1] - step : m[q + 1] + d - step;
#pragma unroll
            for (int q = 0; q < DPT; ++q) {
                const int64_t off = (int64_t)m[q] * a.rows.ld + i;
                dv[q] = IN32 ? (double)f32_from_file(a.rows_in32[off], a.in32_sel) : a.rows.base[off];
            }
        }
#pragma unroll
        for (int q = 0; q < TPT; ++q) tv[q] = u.kernel[(int64_t)min(g + q * G, u.n_ks - 1) * a.n + i];
#pragma unroll
        for (int q = 0; q < DPT; ++q) {
            const int r = g + q * G;
            const bool inside = (uint32_t)(tb + q * G) < (uint32_t)a.T;      // 0 <= row < T in one test
            if (r < ROWS) dt[r * kUhTileLd + c] = (live && inside && r < DATA) ? dv[q] : 0.0;
        }
#pragma unroll
        for (int q = 0; q < TPT; ++q) {
            const int k = g + q * G;
            if (k < NK) tp[k * kUhTileLd + c] = (live && k < u.n_ks) ? tv[q] : 0.0;
        }
    }
    __syncthreads();
    const int rb = g * RP;      // first output row of this thread
    const bool mine = !SUB || rb < need;
    double acc[RP];
    if (mine) {
        const double *wp = dt + rb * kUhTileLd + c;       // depth row (row_first + rb + q - (NK - 1)) at wp[q * kUhTileLd]: rb + W - 1 < ROWS
        if (row_first < (int64_t)u.n_ks) {      // the carried-in state reaches the first n_ks rows of a call: a few launches, all of whose workgroups come here
#pragma unroll
            for (int j = 0; j < RP; ++j) {
                const int64_t t = row_first + rb + j;
                acc[j] = (live && t >= 0 && t < u.n_ks && t < a.T) ? u.state[t * a.n + i] : 0.0;
            }
        } else {
#pragma unroll
            for (int j = 0; j < RP; ++j) acc[j] = 0.0;
        }
        // Half of the taps in registers at a time and the window streamed past them (each depth value meets the taps it is
        // multiplied with while it is in one register): 24 taps + 9 sums instead of a 56-value window, 90 registers instead of
        // 142, five workgroups per CU instead of three.  Every sum still adds its products in the order k = 0, 1, ...
        const double *kp = tp + c;
        constexpr int KH = NK / 2;
        static_assert(NK % 2 == 0, "taps are padded to an even count");
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            double tap[KH];
#pragma unroll
            for (int k = 0; k < KH; ++k) tap[k] = kp[(h * KH + k) * kUhTileLd];
#pragma unroll
            for (int w = RP - 1 + NK - 1 - h * KH; w >= NK - 1 - h * KH - (KH - 1); --w) {      // window index j + NK - 1 - k, k ascending for each j
                const double x = wp[w * kUhTileLd];
#pragma unroll
                for (int j = 0; j < RP; ++j) {
                    const int k = j + NK - 1 - w - h * KH;
                    if (k >= 0 && k < KH) acc[j] = __builtin_fma(tap[k], x, acc[j]);
                }
            }
        }
    }
    __syncthreads();      // every window is in registers: the depth tile's space now takes the outputs
    if (mine) {
        double *op = dt + rb * kUhTileLd + c;
#pragma unroll
        for (int j = 0; j < RP; ++j) op[j * kUhTileLd] = acc[j];      // rb + j < win_rows: the rows past the tile's end are written and never read
    }
    __syncthreads();
    write_records<SUB, uh_threads(BATCHES), kRecBatch * BATCHES, false, kUhCols>(a, dt, col0, a.batch, tick_first, row_first);
}

// OUT32: the router's post-processing fused in (TransformMuskingum.py:128-142): mean over `factor` consecutive rows
// (sequential sum, one division, as numpy reduces a strided axis) and the float32 cast; 128 % (factor * nsub) == 0.
// One column tile per workgroup, every record read of it in flight at once.
// a.batches consecutive batches per workgroup, as k_rec_in: a later batch reads its eight new records only -- its first is the one
// before's ninth, still in LDS (moved to the front) -- 8.25 records read per batch at four batches instead of 9.  Its record loads
// are all in flight before the previous batch's rows leave; the column metadata stays in LDS.
template <bool SUB, bool OUT32, bool ENS = false>
__global__ __launch_bounds__(kRecOutThreads) void k_rec_out(const RecArgsOf<ENS> args)
{
    const RecPermArgs &a = member_args(args);
    constexpr int S = 16 * (kRecBatch + 1);
    __shared__ double recs[kRecOutCols][S + 1];
    __shared__ int2 smeta[kRecOutCols];
    const int tid = threadIdx.x;
    static_assert(kRecOutCols * (kRecBatch + 1) * 8 % kRecOutThreads == 0, "record pieces of a tile must divide among the threads");
    static_assert(kRecOutCols * 8 == kRecOutThreads, "one 16-byte piece of the records kept between batches per thread");
    constexpr int IT = kRecOutCols * (kRecBatch + 1) * 8 / kRecOutThreads, ITN = kRecOutCols * kRecBatch * 8 / kRecOutThreads;
    const uint32_t n_tiles = (uint32_t)((a.n + kRecOutCols - 1) / kRecOutCols);
    if (blockIdx.x >= n_tiles) return;
    const int64_t col0 = (int64_t)(a.swizzle ? xcd_swizzle(blockIdx.x, n_tiles) : blockIdx.x) * kRecOutCols;
    typedef double d2 __attribute__((ext_vector_type(2)));
    {
        d2 v[IT];
        const uint32_t chunk_first = a.rec_chunks.mod((uint32_t)kRecBatch * (uint32_t)a.batch);
        {   // a column past the end reads position 0 and is not written
            int2 meta[IT];
#pragma unroll
            for (int it = 0; it < IT; ++it) {      // every metadata load first: the record loads depend on them, one wait for all
                const int64_t i = col0 + (it * kRecOutThreads + tid) / ((kRecBatch + 1) * 8);
                meta[it] = i < a.n ? a.colmeta[i] : make_int2(0, 0);
            }
#pragma unroll
            for (int it = 0; it < IT; ++it) {
                const int piece = it * kRecOutThreads + tid;
                const int k = (piece >> 3) % (kRecBatch + 1), part = piece & 7;
                const uint32_t chunk = ring_chunk(a.rec_chunks, chunk_first, (uint32_t)((meta[it].y & kLagMask) >> 4) + k);
                v[it] = stream_load<kRecStreams.out_recs>(reinterpret_cast<const d2 *>(a.rec + rec_elem(chunk, a.np, meta[it].x)) + part);
            }
        }
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int piece = it * kRecOutThreads + tid;
            const int c = piece / ((kRecBatch + 1) * 8), k = (piece >> 3) % (kRecBatch + 1), part = piece & 7;
            recs[c][16 * k + 2 * part] = v[it].x;
            recs[c][16 * k + 2 * part + 1] = v[it].y;
        }
    }
    const int c = tid % kRecOutCols;
    const int64_t i = col0 + c;
    const bool live = i < a.n;
    const int2 cm = live ? a.colmeta[i] : make_int2(0, 0);
    if (tid < kRecOutCols) smeta[c] = cm;
    __syncthreads();
    const int32_t my = cm.y;
    const int o = my & 15;
    const int64_t io = !live ? 0 : (a.cols ? a.cols[i] : i);      // destination column; the float32 rows' pitch is the float64 rows' (rows.ld)
    // single sub-step: the records hold the unclamped discharge (a ghost's record is a copy of its reach's); the reference's
    // clip at zero (_numba_kernels.py:80) happens here.  UnitMuskingum leaves its headwaters' lateral inflow as it is (:122-123).
    const bool clamp = !SUB && (a.clamp == 1 || (a.clamp == 2 && !(my & kColHeadwater)));
    auto out = [&](double x) { return clamp && !(x > 0.0) ? 0.0 : x; };
    auto write_rows = [&](int64_t tick0) {      // the tile's rows of the batch from tick-row tick0 on; a column past the end writes nothing
        if (!live) return;
        if (OUT32) {
            // output row q averages runoff rows [q * factor, (q + 1) * factor), each the slot of its last sub-step
            const int step = (int)(a.factor.d * (SUB ? a.nsub.d : 1u));          // tick-rows per output row, divides 128
            const int64_t q0 = tick0 / step;
            for (int q = tid / kRecOutCols; q < kRecRows / step; q += kRecOutThreads / kRecOutCols) {
                if ((q0 + q + 1) * step > a.total) break;
                const int nsub = SUB ? (int)a.nsub.d : 1;
                double acc = out(recs[c][o + q * step + nsub - 1]);
                for (int j = 1; j < (int)a.factor.d; ++j) acc += out(recs[c][o + q * step + j * nsub + nsub - 1]);
                stream_store<kRecStreams.out_rows>(a.rows32 + ((q0 + q) * a.rows.ld + io), f32_to_file((float)(a.factor.d > 1 ? acc / (double)a.factor.d : acc), a.out32_sel));
            }
        } else {
            for (int r = tid / kRecOutCols; r < kRecRows; r += kRecOutThreads / kRecOutCols) {
                const int64_t tick = tick0 + r;
                if (tick >= a.total) break;
                if (SUB) {
                    uint32_t sub;
                    const uint32_t row = a.nsub.div((uint32_t)tick, sub);
                    if (sub + 1 == a.nsub.d) stream_store<kRecStreams.out_rows>(a.rows.row(row) + io, recs[c][o + r]);
                } else {
                    stream_store<kRecStreams.out_rows>(a.rows.row(tick) + io, out(recs[c][o + r]));
                }
            }
        }
    };
    const int nb = a.batches > 1 ? a.batches : 1;
    for (int b = 1; b < nb; ++b) {
        d2 v[ITN];
        const uint32_t chunk_first = a.rec_chunks.mod((uint32_t)kRecBatch * (uint32_t)(a.batch + b));
#pragma unroll
        for (int it = 0; it < ITN; ++it) {      // records 1 .. kRecBatch of the batch
            const int piece = it * kRecOutThreads + tid;
            const int2 m = smeta[piece / (kRecBatch * 8)];
            const int k = 1 + (piece >> 3) % kRecBatch, part = piece & 7;
            const uint32_t chunk = ring_chunk(a.rec_chunks, chunk_first, (uint32_t)((m.y & kLagMask) >> 4) + k);
            v[it] = stream_load<kRecStreams.out_recs>(reinterpret_cast<const d2 *>(a.rec + rec_elem(chunk, a.np, m.x)) + part);
        }
        write_rows(kRecRows * (a.batch + b - 1));
        const int kc = tid >> 3, kp = tid & 7;      // the piece of the last record this thread moves to the front
        const double k0 = recs[kc][16 * kRecBatch + 2 * kp], k1 = recs[kc][16 * kRecBatch + 2 * kp + 1];
        __syncthreads();      // every row of the batch has been read out of the records
        recs[kc][2 * kp] = k0;
        recs[kc][2 * kp + 1] = k1;
#pragma unroll
        for (int it = 0; it < ITN; ++it) {
            const int piece = it * kRecOutThreads + tid;
            const int cc = piece / (kRecBatch * 8), k = 1 + (piece >> 3) % kRecBatch, part = piece & 7;
            recs[cc][16 * k + 2 * part] = v[it].x;
            recs[cc][16 * k + 2 * part + 1] = v[it].y;
        }
        __syncthreads();
    }
    write_rows(kRecRows * (a.batch + nb - 1));
}

// Router post-processing on the device (TransformMuskingum.py:128-142): mean over `factor` consecutive rows
// (sequential sum then one division, as numpy's reduction over a strided axis does) and the float32 cast.
__global__ __launch_bounds__(kBlock) void k_resample_cast(const double *__restrict__ src, float *__restrict__ dst,
                                                          int64_t n, int64_t out_rows, int32_t factor)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t o = blockIdx.y;
    if (i >= n || o >= out_rows) return;
    const double *p = src + o * factor * n + i;
    double acc = p[0];
    for (int32_t j = 1; j < factor; ++j) acc += p[(int64_t)j * n];
    dst[o * n + i] = (float)(factor > 1 ? acc / (double)factor : acc);
}

}  // namespace
