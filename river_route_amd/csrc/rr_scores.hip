// rr_scores.hip -- the entry points of librr_hip.so that take a device index and no plan: the per-column skill scores
// (rr_kernels_metrics.hpp), their adjoint (rr_kernels_metrics_adjoint.hpp) and the catchment / grid-cell overlap areas
// (rr_kernels_overlap.hpp).  A translation unit and a code object of their own: nothing here refers to the plan, the executor or a
// routing kernel, and the code object of rr_engine.hip does not change when a kernel here is added, templated or merged
// (DESIGN.md section 9b).  No CPU fallback anywhere in this file.
//
// Shared with rr_engine.hip: rr::fail (one error string for rr_last_error, rr_common.hpp), rr::dev_mem_alloc / rr::dev_mem_free
// (behind DevBuf, rr_devbuf.hpp) and rr_device_count.
#include "rr_common.hpp"
#include "rr_devbuf.hpp"
#include "rr_kernels_metrics.hpp"
#include "rr_kernels_metrics_adjoint.hpp"
#include "rr_kernels_overlap.hpp"

using rr::DevBuf;

namespace {

// The eight forms of a scores kernel, by the call's skip_missing, true_is_f32 and pred_is_f32: LAUNCH_(MISSING, TT, TP).
#define RR_SCORES_DISPATCH(LAUNCH_)                                                        \
    switch ((skip_missing ? 4 : 0) | (true_is_f32 ? 2 : 0) | (pred_is_f32 ? 1 : 0)) {       \
    case 0: LAUNCH_(false, double, double); break;                                         \
    case 1: LAUNCH_(false, double, float); break;                                          \
    case 2: LAUNCH_(false, float, double); break;                                          \
    case 3: LAUNCH_(false, float, float); break;                                           \
    case 4: LAUNCH_(true, double, double); break;                                          \
    case 5: LAUNCH_(true, double, float); break;                                           \
    case 6: LAUNCH_(true, float, double); break;                                           \
    default: LAUNCH_(true, float, float); break;                                           \
    }

// One update of the scores' state, behind rr_metrics_update_dev, rr_metrics_update_missing_dev (members = 1, member pitches 0) and
// rr_metrics_update_members_dev (by_members: sized by rr_metrics_members_work_bytes).  `who` names the entry point in every refusal.
int metrics_update(const char *who, bool by_members, int device, int64_t n, int64_t members, int64_t rows, const void *y_true, int true_is_f32,
                   int64_t true_pitch, int64_t true_member_pitch, const void *y_pred, int pred_is_f32, int64_t pred_pitch,
                   int64_t pred_member_pitch, const int32_t *pred_columns, int skip_missing, double *state, void *work, int64_t work_bytes,
                   void *stream)
{
    const std::string fn(who);
    if (device < 0 || device >= rr_device_count()) return fail(RR_E_NO_DEVICE, fn + ": no such HIP device");
    HIPCHK(hipSetDevice(device));
    int64_t need = 0;
    if (int rc = by_members ? rr_metrics_members_work_bytes(n, members, rows, &need) : rr_metrics_work_bytes(n, rows, &need)) return rc;
    if (n == 0 || rows == 0) return RR_OK;
    if (!y_true || !y_pred || !state) return fail(RR_E_INVALID, fn + ": null array");
    const int64_t pred_width = pred_columns ? 1 : n;
    if (true_pitch < n || pred_pitch < pred_width) return fail(RR_E_INVALID, fn + ": row pitch shorter than the columns read");
    if (members > 1) {      // (one member: its pitches are never used)
        // no real pitch is this long; refusing it keeps the products below in range
        if (true_pitch > (INT64_MAX >> 1) / rows || pred_pitch > (INT64_MAX >> 1) / rows) return fail(RR_E_INVALID, fn + ": row pitch out of range");
        if (pred_member_pitch < (rows - 1) * pred_pitch + pred_width ||
            (true_member_pitch != 0 && true_member_pitch < (rows - 1) * true_pitch + n))
            return fail(RR_E_INVALID, fn + ": member pitch shorter than the rows one member spans");
    }
    if (!work || work_bytes < need)
        return fail(RR_E_INVALID, fn + ": work memory smaller than " + (by_members ? "rr_metrics_members_work_bytes" : "rr_metrics_work_bytes") +
                                      " (" + std::to_string(need) + " bytes)");
    int64_t splits, rows_per_split;
    metrics_split(n, rows, splits, rows_per_split, members);
    double *slab = static_cast<double *>(work);
    const int64_t col_blocks = (n + kBlock - 1) / kBlock, total = members * n;
    const dim3 g((unsigned)(members * col_blocks), (unsigned)splits);
#define RR_METRICS_LAUNCH(MISSING_, TT_, TP_)                                                                                          \
    hipLaunchKernelGGL((k_metrics_partial<MISSING_, TT_, TP_>), g, dim3(kBlock), 0, (hipStream_t)stream, (const TT_ *)y_true, true_pitch, \
                       true_member_pitch, (const TP_ *)y_pred, pred_pitch, pred_member_pitch, pred_columns, n, col_blocks, members, rows, \
                       rows_per_split, slab)
    RR_SCORES_DISPATCH(RR_METRICS_LAUNCH)
#undef RR_METRICS_LAUNCH
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_metrics_merge, grid1(total), dim3(kBlock), 0, (hipStream_t)stream, slab, splits, total, state);
    HIPCHK(hipGetLastError());
    return RR_OK;
}

// The gradient of a loss through the scores, behind rr_metrics_adjoint_dev and rr_metrics_adjoint_missing_dev.
int metrics_adjoint(const char *who, int device, int64_t n, int64_t rows, const void *y_true, int true_is_f32, int64_t true_pitch,
                    const void *y_pred, int pred_is_f32, int64_t pred_pitch, const double *state, const double *grad_scores, int64_t n_distinct,
                    const int32_t *order, const int32_t *distinct_columns, const int32_t *segments, void *grad_pred, int64_t grad_pitch,
                    void *work, int64_t work_bytes, void *stream, int skip_missing)
{
    const std::string fn(who);
    if (device < 0 || device >= rr_device_count()) return fail(RR_E_NO_DEVICE, fn + ": no such HIP device");
    HIPCHK(hipSetDevice(device));
    int64_t need = 0;
    if (int rc = rr_metrics_adjoint_work_bytes(n, &need)) return rc;
    if (rows < 0) return fail(RR_E_INVALID, fn + ": sizes out of range");
    if (n == 0 || rows == 0) return RR_OK;
    if (!y_true || !y_pred || !state || !grad_scores || !grad_pred) return fail(RR_E_INVALID, fn + ": null array");
    const bool mapped = order || distinct_columns || segments;
    if (mapped && !(order && distinct_columns && segments))
        return fail(RR_E_INVALID, fn + ": order, distinct_columns and segments come together or not at all");
    if (mapped ? (n_distinct < 1 || n_distinct > n) : n_distinct != n)
        return fail(RR_E_INVALID, fn + ": n_distinct must be n without a column map and 1 .. n with one");
    if (true_pitch < n || pred_pitch < (mapped ? 1 : n) || grad_pitch < (mapped ? 1 : n))
        return fail(RR_E_INVALID, fn + ": row pitch shorter than the columns read or written");
    if (!work || work_bytes < need)
        return fail(RR_E_INVALID, fn + ": work memory smaller than rr_metrics_adjoint_work_bytes (" + std::to_string(need) + " bytes)");
    double *coef = static_cast<double *>(work);
    hipLaunchKernelGGL(k_metrics_adjoint_coef, grid1(n), dim3(kBlock), 0, (hipStream_t)stream, state, grad_scores, n, coef);
    HIPCHK(hipGetLastError());
    int64_t splits, rows_per_split;
    metrics_split(n_distinct, rows, splits, rows_per_split);      // the forward's row ranges: narrow inputs still fill the card
    const dim3 g((unsigned)((n_distinct + kBlock - 1) / kBlock), (unsigned)splits);
#define RR_METRICS_ADJ_LAUNCH(MISSING_, TT_, TP_)                                                                                          \
    hipLaunchKernelGGL((k_metrics_adjoint_rows<MISSING_, TT_, TP_>), g, dim3(kBlock), 0, (hipStream_t)stream, (const TT_ *)y_true, true_pitch, \
                       (const TP_ *)y_pred, pred_pitch, (const double *)coef, n, order, distinct_columns, segments, n_distinct, rows,         \
                       rows_per_split, (TP_ *)grad_pred, grad_pitch)
    RR_SCORES_DISPATCH(RR_METRICS_ADJ_LAUNCH)
#undef RR_METRICS_ADJ_LAUNCH
    HIPCHK(hipGetLastError());
    return RR_OK;
}

#undef RR_SCORES_DISPATCH

}  // namespace

extern "C" {

// ---- skill scores (rr_kernels_metrics.hpp; DESIGN.md sections 9, 9c) ----

int rr_metrics_work_bytes(int64_t n, int64_t rows, int64_t *bytes)
{
    if (!bytes) return fail(RR_E_INVALID, "rr_metrics_work_bytes: null out");
    if (n < 0 || rows < 0 || n > 0x7FFFFFFFLL) return fail(RR_E_INVALID, "rr_metrics_work_bytes: sizes out of range");
    *bytes = 0;
    if (n == 0 || rows == 0) return RR_OK;
    int64_t splits, rows_per_split;
    metrics_split(n, rows, splits, rows_per_split);
    *bytes = splits * RR_METRICS_STATE * n * (int64_t)sizeof(double);
    return RR_OK;
}

int rr_metrics_members_work_bytes(int64_t n, int64_t members, int64_t rows, int64_t *bytes)
{
    if (!bytes) return fail(RR_E_INVALID, "rr_metrics_members_work_bytes: null out");
    if (n < 0 || rows < 0 || members < 1 || n > 0x7FFFFFFFLL || (n > 0 && members > 0x7FFFFFFFLL / n))
        return fail(RR_E_INVALID, "rr_metrics_members_work_bytes: sizes out of range (members >= 1, members * n <= 2^31 - 1)");
    *bytes = 0;
    if (n == 0 || rows == 0) return RR_OK;
    int64_t splits, rows_per_split;
    metrics_split(n, rows, splits, rows_per_split, members);
    *bytes = splits * RR_METRICS_STATE * members * n * (int64_t)sizeof(double);
    return RR_OK;
}

int rr_metrics_update_dev(int device, int64_t n, int64_t rows, const void *y_true, int true_is_f32, int64_t true_pitch,
                          const void *y_pred, int pred_is_f32, int64_t pred_pitch, const int32_t *pred_columns, double *state,
                          void *work, int64_t work_bytes, void *stream)
{
    return metrics_update("rr_metrics_update_dev", false, device, n, 1, rows, y_true, true_is_f32, true_pitch, 0, y_pred, pred_is_f32, pred_pitch,
                          0, pred_columns, 0, state, work, work_bytes, stream);
}

int rr_metrics_update_missing_dev(int device, int64_t n, int64_t rows, const void *y_true, int true_is_f32, int64_t true_pitch,
                                  const void *y_pred, int pred_is_f32, int64_t pred_pitch, const int32_t *pred_columns, double *state,
                                  void *work, int64_t work_bytes, void *stream)
{
    return metrics_update("rr_metrics_update_missing_dev", false, device, n, 1, rows, y_true, true_is_f32, true_pitch, 0, y_pred, pred_is_f32,
                          pred_pitch, 0, pred_columns, 1, state, work, work_bytes, stream);
}

int rr_metrics_update_members_dev(int device, int64_t n, int64_t members, int64_t rows, const void *y_true, int true_is_f32,
                                  int64_t true_pitch, int64_t true_member_pitch, const void *y_pred, int pred_is_f32, int64_t pred_pitch,
                                  int64_t pred_member_pitch, const int32_t *pred_columns, int skip_missing, double *state, void *work,
                                  int64_t work_bytes, void *stream)
{
    return metrics_update("rr_metrics_update_members_dev", true, device, n, members, rows, y_true, true_is_f32, true_pitch, true_member_pitch,
                          y_pred, pred_is_f32, pred_pitch, pred_member_pitch, pred_columns, skip_missing, state, work, work_bytes, stream);
}

int rr_metrics_finish_dev(int device, int64_t n, const double *state, double *out, void *stream)
{
    if (device < 0 || device >= rr_device_count()) return fail(RR_E_NO_DEVICE, "rr_metrics_finish_dev: no such HIP device");
    HIPCHK(hipSetDevice(device));
    if (n < 0 || n > 0x7FFFFFFFLL) return fail(RR_E_INVALID, "rr_metrics_finish_dev: sizes out of range");
    if (n == 0) return RR_OK;
    if (!state || !out) return fail(RR_E_INVALID, "rr_metrics_finish_dev: null array");
    hipLaunchKernelGGL(k_metrics_finish, grid1(n), dim3(kBlock), 0, (hipStream_t)stream, state, n, out);
    HIPCHK(hipGetLastError());
    return RR_OK;
}

// ---- adjoint of the skill scores (rr_kernels_metrics_adjoint.hpp) ----

int rr_metrics_adjoint_work_bytes(int64_t n, int64_t *bytes)
{
    if (!bytes) return fail(RR_E_INVALID, "rr_metrics_adjoint_work_bytes: null out");
    *bytes = 0;
    if (n < 0 || n > 0x7FFFFFFFLL) return fail(RR_E_INVALID, "rr_metrics_adjoint_work_bytes: sizes out of range");
    *bytes = kMetricsAdjCoef * n * (int64_t)sizeof(double);
    return RR_OK;
}

int rr_metrics_adjoint_dev(int device, int64_t n, int64_t rows, const void *y_true, int true_is_f32, int64_t true_pitch,
                           const void *y_pred, int pred_is_f32, int64_t pred_pitch, const double *state, const double *grad_scores,
                           int64_t n_distinct, const int32_t *order, const int32_t *distinct_columns, const int32_t *segments,
                           void *grad_pred, int64_t grad_pitch, void *work, int64_t work_bytes, void *stream)
{
    return metrics_adjoint("rr_metrics_adjoint_dev", device, n, rows, y_true, true_is_f32, true_pitch, y_pred, pred_is_f32, pred_pitch, state,
                           grad_scores, n_distinct, order, distinct_columns, segments, grad_pred, grad_pitch, work, work_bytes, stream, 0);
}

int rr_metrics_adjoint_missing_dev(int device, int64_t n, int64_t rows, const void *y_true, int true_is_f32, int64_t true_pitch,
                                   const void *y_pred, int pred_is_f32, int64_t pred_pitch, const double *state, const double *grad_scores,
                                   int64_t n_distinct, const int32_t *order, const int32_t *distinct_columns, const int32_t *segments,
                                   void *grad_pred, int64_t grad_pitch, void *work, int64_t work_bytes, void *stream)
{
    return metrics_adjoint("rr_metrics_adjoint_missing_dev", device, n, rows, y_true, true_is_f32, true_pitch, y_pred, pred_is_f32, pred_pitch,
                           state, grad_scores, n_distinct, order, distinct_columns, segments, grad_pred, grad_pitch, work, work_bytes, stream, 1);
}

// ---- catchment / grid-cell overlap areas (rr_kernels_overlap.hpp) ----

namespace {

int overlap_sizes(const char *fn, int64_t n_rows, int64_t n_rings, int64_t n_vertices, int64_t nx, int64_t ny, int64_t n_pairs)
{
    if (n_rows < 0 || n_rings < 0 || n_vertices < 0 || nx < 1 || ny < 1 || n_pairs < 0 || nx >= 0x7FFFFFFFLL ||
        ny >= 0x7FFFFFFFLL || n_rows >= 0x7FFFFFFFLL || n_pairs > (int64_t)0xFFFFFFFFLL * kOverlapWaves)
        return fail(RR_E_INVALID, std::string(fn) + ": sizes out of range");
    return RR_OK;
}

}  // namespace

int rr_grid_overlap_area_dev(int device, int64_t n_rows, int64_t n_rings, int64_t n_vertices, int64_t nx, int64_t ny, int64_t n_pairs,
                             const int64_t *row_rings, const int64_t *ring_offsets, const double *ring_weight, const double *lon,
                             const double *lat, const double *x_bounds, const double *y_bounds, const int32_t *row_cells,
                             const int64_t *pair_offsets, double *area, void *stream)
{
    if (device < 0 || device >= rr_device_count()) return fail(RR_E_NO_DEVICE, "rr_grid_overlap_area_dev: no such HIP device");
    HIPCHK(hipSetDevice(device));
    if (int rc = overlap_sizes("rr_grid_overlap_area_dev", n_rows, n_rings, n_vertices, nx, ny, n_pairs)) return rc;
    if (n_pairs == 0) return RR_OK;
    if (n_rows == 0) return fail(RR_E_INVALID, "rr_grid_overlap_area_dev: pairs without rows");
    if (!row_rings || !ring_offsets || !ring_weight || !lon || !lat || !x_bounds || !y_bounds || !row_cells || !pair_offsets || !area)
        return fail(RR_E_INVALID, "rr_grid_overlap_area_dev: null array");
    const int64_t blocks = (n_pairs + kOverlapWaves - 1) / kOverlapWaves;
    hipLaunchKernelGGL(k_overlap_area, dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, n_rows, n_pairs, row_rings,
                       ring_offsets, ring_weight, lon, lat, x_bounds, y_bounds, row_cells, pair_offsets, area);
    HIPCHK(hipGetLastError());
    return RR_OK;
}

int rr_grid_overlap_area(int device, int64_t n_rows, int64_t n_rings, int64_t n_vertices, int64_t nx, int64_t ny, int64_t n_pairs,
                         const int64_t *row_rings, const int64_t *ring_offsets, const double *ring_weight, const double *lon,
                         const double *lat, const double *x_bounds, const double *y_bounds, const int32_t *row_cells,
                         const int64_t *pair_offsets, double *area)
{
    const char *fn = "rr_grid_overlap_area";
    if (device < 0 || device >= rr_device_count()) return fail(RR_E_NO_DEVICE, "rr_grid_overlap_area: no such HIP device");
    HIPCHK(hipSetDevice(device));
    if (int rc = overlap_sizes(fn, n_rows, n_rings, n_vertices, nx, ny, n_pairs)) return rc;
    if (n_pairs == 0) return RR_OK;
    if (n_rows == 0) return fail(RR_E_INVALID, "rr_grid_overlap_area: pairs without rows");
    if (!row_rings || !ring_offsets || !ring_weight || !lon || !lat || !x_bounds || !y_bounds || !row_cells || !pair_offsets || !area)
        return fail(RR_E_INVALID, "rr_grid_overlap_area: null array");
    // every index the kernel follows, checked here so the device reads stay inside the arrays
    if (row_rings[0] != 0 || row_rings[n_rows] != n_rings || ring_offsets[0] != 0 || ring_offsets[n_rings] != n_vertices ||
        pair_offsets[0] != 0 || pair_offsets[n_rows] != n_pairs)
        return fail(RR_E_INVALID, "rr_grid_overlap_area: offsets must start at 0 and end at n_rings / n_vertices / n_pairs");
    for (int64_t r = 0; r < n_rows; ++r) {
        const int64_t cells = pair_offsets[r + 1] - pair_offsets[r];
        if (row_rings[r + 1] < row_rings[r] || cells < 0)
            return fail(RR_E_INVALID, "rr_grid_overlap_area: row " + std::to_string(r) + ": offsets decrease");
        if (cells == 0) continue;
        const int64_t cx = row_cells[3 * r], cy = row_cells[3 * r + 1], cny = row_cells[3 * r + 2];
        if (cny < 1 || cells % cny != 0 || cx < 0 || cy < 0 || cx + cells / cny > nx || cy + cny > ny || cells > 0x7FFFFFFFLL)
            return fail(RR_E_INVALID, "rr_grid_overlap_area: row " + std::to_string(r) + ": candidate cells outside the grid");
    }
    for (int64_t g = 0; g < n_rings; ++g)
        if (ring_offsets[g + 1] < ring_offsets[g])
            return fail(RR_E_INVALID, "rr_grid_overlap_area: ring " + std::to_string(g) + ": offsets decrease");
    for (int64_t i = 0; i < nx; ++i)
        if (!(x_bounds[i] < x_bounds[i + 1])) return fail(RR_E_INVALID, "rr_grid_overlap_area: x_bounds not strictly ascending");
    for (int64_t j = 0; j < ny; ++j)
        if (!(y_bounds[j] < y_bounds[j + 1])) return fail(RR_E_INVALID, "rr_grid_overlap_area: y_bounds not strictly ascending");

    DevBuf<int64_t> d_rr, d_ro, d_po;
    DevBuf<double> d_w, d_lon, d_lat, d_xb, d_yb, d_out;
    DevBuf<int32_t> d_rc;
    int rc = d_rr.alloc(n_rows + 1);
    if (!rc) rc = d_ro.alloc(n_rings + 1);
    if (!rc) rc = d_po.alloc(n_rows + 1);
    if (!rc) rc = d_w.alloc(n_rings);
    if (!rc) rc = d_lon.alloc(n_vertices);
    if (!rc) rc = d_lat.alloc(n_vertices);
    if (!rc) rc = d_xb.alloc(nx + 1);
    if (!rc) rc = d_yb.alloc(ny + 1);
    if (!rc) rc = d_rc.alloc(3 * n_rows);
    if (!rc) rc = d_out.alloc(n_pairs);
    if (rc) return rc;
    auto up = [](void *dst, const void *src, int64_t bytes) {
        return bytes > 0 ? hipMemcpy(dst, src, (size_t)bytes, hipMemcpyHostToDevice) : hipSuccess;
    };
    hipError_t e = up(d_rr, row_rings, (n_rows + 1) * 8);
    if (e == hipSuccess) e = up(d_ro, ring_offsets, (n_rings + 1) * 8);
    if (e == hipSuccess) e = up(d_po, pair_offsets, (n_rows + 1) * 8);
    if (e == hipSuccess) e = up(d_w, ring_weight, n_rings * 8);
    if (e == hipSuccess) e = up(d_lon, lon, n_vertices * 8);
    if (e == hipSuccess) e = up(d_lat, lat, n_vertices * 8);
    if (e == hipSuccess) e = up(d_xb, x_bounds, (nx + 1) * 8);
    if (e == hipSuccess) e = up(d_yb, y_bounds, (ny + 1) * 8);
    if (e == hipSuccess) e = up(d_rc, row_cells, 3 * n_rows * 4);
    if (e != hipSuccess) return fail(RR_E_HIP, hipGetErrorString(e));
    rc = rr_grid_overlap_area_dev(device, n_rows, n_rings, n_vertices, nx, ny, n_pairs, d_rr, d_ro, d_w, d_lon, d_lat, d_xb, d_yb,
                                  d_rc, d_po, d_out, nullptr);
    if (!rc) {
        e = hipMemcpy(area, d_out, (size_t)n_pairs * sizeof(double), hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(RR_E_HIP, hipGetErrorString(e));
    }
    return rc;
}

}  // extern "C"
