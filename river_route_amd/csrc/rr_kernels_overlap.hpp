// rr_kernels_overlap.hpp -- area of catchment polygons clipped to the cells of a regular grid (river_route/runoff.py:70-116:
// gpd.overlay of the grid's Voronoi cells with the catchments, then .to_crs({'proj': 'cea'}).area).
// Part of the translation unit rr_scores.hip builds (included from there, after rr_common.hpp; not a stand-alone header).
#pragma once

namespace {

// ---- cylindrical equal-area projection, PROJ's `+proj=cea` on its default ellipsoid (GRS80), lat_ts = 0 ----
// X = a lambda, Y = a q(phi) / 2 with PROJ's pj_qsfn form of q.  Both axes are monotone, so a lon/lat rectangle maps to a
// rectangle and a ring keeps its orientation.
constexpr double kCeaA = 6378137.0;
constexpr double kCeaF = 1.0 / 298.257222101;
constexpr double kCeaEs = 2.0 * kCeaF - kCeaF * kCeaF;      // e^2
constexpr double kDegToRad = 0.017453292519943295;          // pi / 180, as PROJ's DEG_TO_RAD
constexpr double kCeaXPerDeg = kCeaA * kDegToRad;

__device__ __forceinline__ double cea_y(double lat_deg)
{
    const double e = sqrt(kCeaEs);
    const double s = sin(lat_deg * kDegToRad);
    const double con = e * s;
    const double q = (1.0 - kCeaEs) * (s / (1.0 - con * con) - (0.5 / e) * log((1.0 - con) / (1.0 + con)));
    return 0.5 * q * kCeaA;
}

// Contribution of one straight lon/lat edge a -> b to the clipped area of a ring against the cell [x0, x1] x [y0, y1]
// (projected band [Y0, Y1]): the edge is clipped to the cell's longitude span, split where it crosses lat y0 or y1 (the
// crossing points computed in lon/lat, as the overlay computes the vertices of the intersection polygon), and each
// sub-piece u -> v scores (Xv - Xu) * (h(u) + h(v)) / 2 with h = clamp(Y, Y0, Y1) - Y0: 0 below the band, the band's height
// above it, the trapezoid to Y0 inside it.  A ring's clipped shoelace area is minus the sum over its edges.
__device__ __forceinline__ double overlap_edge(double ax, double ay, double bx, double by, double x0, double x1, double y0,
                                               double y1, double Y0, double Y1)
{
    if (ax == bx) return 0.0;                                    // vertical (or zero-length): no dX
    if (fmax(ay, by) <= y0) return 0.0;                          // wholly below the band
    const double lo = fmin(ax, bx), hi = fmax(ax, bx);
    if (hi <= x0 || lo >= x1) return 0.0;                        // outside the cell's longitude span
    // clip to [x0, x1] along the edge's own parameter; the clip points lie exactly on the cell's sides
    double px = ax, py = ay, qx = bx, qy = by;
    const double sx = (by - ay) / (bx - ax);
    if (ax < x0) { px = x0; py = ay + (x0 - ax) * sx; }
    else if (ax > x1) { px = x1; py = ay + (x1 - ax) * sx; }
    if (bx < x0) { qx = x0; qy = ay + (x0 - ax) * sx; }
    else if (bx > x1) { qx = x1; qy = ay + (x1 - ax) * sx; }
    const double H = Y1 - Y0;
    const double dX = (qx - px) * kCeaXPerDeg;
    if (fmin(py, qy) >= y1) return dX * H;                       // wholly above the band
    if (fmax(py, qy) <= y0) return 0.0;
    const double hp = py >= y1 ? H : (py <= y0 ? 0.0 : cea_y(py) - Y0);
    const double hq = qy >= y1 ? H : (qy <= y0 ? 0.0 : cea_y(qy) - Y0);
    // crossings of y0 / y1 strictly inside the piece, in the order the piece meets them
    const bool c0 = (py - y0) * (qy - y0) < 0.0, c1 = (py - y1) * (qy - y1) < 0.0;
    if (!c0 && !c1) return 0.5 * dX * (hp + hq);
    const double ix = (qx - px) / (qy - py);
    const double X0c = c0 ? (px + (y0 - py) * ix) * kCeaXPerDeg : 0.0;
    const double X1c = c1 ? (px + (y1 - py) * ix) * kCeaXPerDeg : 0.0;
    const double Xp = px * kCeaXPerDeg, Xq = qx * kCeaXPerDeg;
    if (c0 && c1) {
        // below -> inside -> above (rising) or above -> inside -> below (falling)
        return qy > py ? 0.5 * (X1c - X0c) * H + (Xq - X1c) * H : (X1c - Xp) * H + 0.5 * (X0c - X1c) * H;
    }
    if (c0) return qy > py ? 0.5 * (Xq - X0c) * hq : 0.5 * (X0c - Xp) * hp;          // the below part scores 0
    return qy > py ? 0.5 * (X1c - Xp) * (hp + H) + (Xq - X1c) * H                     // inside, then above
                   : (X1c - Xp) * H + 0.5 * (Xq - X1c) * (H + hq);                    // above, then inside
}

// Wave sum in a fixed butterfly order: every lane ends with the same bits, whatever the launch.
__device__ __forceinline__ double overlap_wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

constexpr int kOverlapWaves = kBlock / 64;

// One wave per (row, cell) pair; kOverlapWaves pairs per workgroup.  The wave finds its row in pair_offsets (a binary search
// on wave-uniform values), then sweeps the row's rings in order with its 64 lanes striding over each ring's edges; each lane
// keeps its own partial and the wave sums them in a fixed order.  No atomics: the same input gives the same bits.
// area[p] = sum over the row's rings r of ring_weight[r] * (signed area of ring r clipped to the cell, positive when the ring
// runs counter-clockwise).  Edge k of a ring runs from its vertex k to vertex k + 1 (the last one back to the first: a
// closed ring's repeated vertex gives a zero-length edge that scores 0).
__global__ __launch_bounds__(kBlock) void k_overlap_area(int64_t n_rows, int64_t n_pairs, const int64_t *__restrict__ row_rings,
                                                         const int64_t *__restrict__ ring_offsets, const double *__restrict__ ring_weight,
                                                         const double *__restrict__ lon, const double *__restrict__ lat,
                                                         const double *__restrict__ x_bounds, const double *__restrict__ y_bounds,
                                                         const int32_t *__restrict__ row_cells, const int64_t *__restrict__ pair_offsets,
                                                         double *__restrict__ area)
{
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * kOverlapWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (p >= n_pairs) return;
    // row = the last r with pair_offsets[r] <= p (rows without pairs are skipped: their offsets repeat)
    int64_t lo = 0, hi = n_rows - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (pair_offsets[mid] <= p) lo = mid; else hi = mid - 1;
    }
    const int64_t row = lo;
    const int32_t ny = row_cells[3 * row + 2];
    const int32_t k = (int32_t)(p - pair_offsets[row]);
    const int32_t ix = row_cells[3 * row] + k / ny, iy = row_cells[3 * row + 1] + k % ny;
    const double x0 = x_bounds[ix], x1 = x_bounds[ix + 1], y0 = y_bounds[iy], y1 = y_bounds[iy + 1];
    // boundaries past the poles (the outer cells reach the clip envelope) project as the pole: no vertex lies beyond it
    const double Y0 = cea_y(fmin(fmax(y0, -90.0), 90.0)), Y1 = cea_y(fmin(fmax(y1, -90.0), 90.0));

    double acc = 0.0;
    for (int64_t r = row_rings[row]; r < row_rings[row + 1]; ++r) {
        const int64_t v0 = ring_offsets[r], v1 = ring_offsets[r + 1];
        const double w = ring_weight[r];
        double ring = 0.0;
        for (int64_t v = v0 + lane; v < v1; v += 64) {
            const int64_t u = v + 1 < v1 ? v + 1 : v0;
            ring += overlap_edge(lon[v], lat[v], lon[u], lat[u], x0, x1, y0, y1, Y0, Y1);
        }
        acc -= w * ring;
    }
    acc = overlap_wave_sum(acc);
    if (lane == 0) area[p] = acc;
}

}  // namespace
