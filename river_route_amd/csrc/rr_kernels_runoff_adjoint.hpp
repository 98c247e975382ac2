// rr_kernels_runoff_adjoint.hpp -- the gradient of a loss through k_runoff_to_qlateral (rr_kernels_runoff.hpp) with respect to the
// gridded runoff and to the weights of the catchment / grid-cell table.
// Part of the one translation unit rr_engine.hip builds (included from there, in order; not a stand-alone header).
#pragma once

namespace {

// With S[t, r] = sum_k w[k] R[t, p_k] over the CSR row of river r, V = S[t] - S[t - 1] (cumulative input, t > 0) or S[t], and
// G = dL/dqlateral:
//   M[t, r]  = V is not NaN and (no clip or V >= 0)            -- torch.clamp's rule: an exactly dry catchment passes its gradient
//   Gb[t, r] = M ? G[t, r] * area[r] : 0
//   Gs[t, r] = Gb[t] - Gb[t + 1] (cumulative; the last row has no t + 1 term) or Gb[t]
//   dL/dR[t, p] = sum over the pairs k of point p, ascending, of w[k] * Gs[t, r_k]
//   dL/dw[k]    = sum over t, ascending, of Gs[t, r_k] * R[t, p_k]
// Terms whose Gs is exactly 0 are skipped: a NaN in the runoff makes Gb 0 at its row (and at the row after it, cumulative), so Gs
// is 0 there, and 0 * NaN must not reach a sum.  Every sum is one lane's serial loop in a fixed order: no atomics, the same bits on every call.

// The river a pair belongs to: the r with indptr[r] <= k < indptr[r + 1] (empty rows are stepped over).  The call carries no
// pair -> river table, so the point pass, which meets pairs out of row order, searches the row offsets: four-way, three pivots in
// flight per step, which halves the chain of dependent loads of a binary search (10 steps for a million rivers); the upper levels
// are the same few lines for every lane.
__device__ __forceinline__ int32_t runoff_pair_river(const int32_t *__restrict__ indptr, int32_t n_rivers, int32_t k)
{
    int32_t lo = 0, hi = n_rivers;      // indptr[lo] <= k < indptr[hi]
    while (hi - lo > 4) {
        const int32_t q = (hi - lo) >> 2, m1 = lo + q, m2 = m1 + q, m3 = m2 + q;
        const int32_t a = indptr[m1], b = indptr[m2], c = indptr[m3];
        if (k < a) hi = m1;
        else if (k < b) { lo = m1; hi = m2; }
        else if (k < c) { lo = m2; hi = m3; }
        else lo = m3;
    }
    while (hi - lo > 1) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (indptr[mid] <= k) lo = mid; else hi = mid;
    }
    return lo;
}

// River pass.  k_runoff_to_qlateral's geometry (one lane per river, a chunk of kRunoffRows rows, the same gather and the same
// rounding, so S and the mask are the forward's), with row t0 - 1 and, for cumulative input, row t0 + 16 beside the chunk: the
// mask of the row after the chunk enters Gs of the chunk's last row.  Gs leaves river-major, gs[r * t_pad + t], t_pad a multiple of
// kRunoffRows: one 128-byte run per lane, which the point and weight passes read back whole.  Rows t >= T of the last chunk are 0.
template <typename RT, bool VEC>
__global__ __launch_bounds__(kBlock) void k_runoff_adjoint_river(const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                                 const double *__restrict__ weights, const RT *__restrict__ runoff,
                                                                 int64_t stride_t, int64_t stride_p, const double *__restrict__ area,
                                                                 int flags, const double *__restrict__ grad_q, double *__restrict__ gs,
                                                                 int64_t n_rivers, int64_t T, int64_t t_pad)
{
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t t0 = (int64_t)blockIdx.y * kRunoffRows;
    if (r >= n_rivers) return;
    const int nt = (int)min((int64_t)kRunoffRows, T - t0);
    const bool cumulative = flags & RR_RUNOFF_CUMULATIVE, force_positive = flags & RR_RUNOFF_FORCE_POSITIVE;
    double acc[kRunoffRows + 2];        // slot 0: row t0 - 1, slot 17: row t0 + 16 (cumulative input only)
#pragma unroll
    for (int j = 0; j <= kRunoffRows + 1; ++j) acc[j] = 0.0;
    const bool need_prev = cumulative && t0 > 0, need_next = cumulative && t0 + kRunoffRows < T;
    for (int32_t k = indptr[r]; k < indptr[r + 1]; ++k) {
        const double w = weights[k];
        const RT *src = runoff + (int64_t)indices[k] * stride_p + (t0 - 1) * stride_t;
        if (VEC) {
            constexpr int VL = 16 / (int)sizeof(RT);      // elements per 16-byte load
            struct alignas(16) Vec { RT v[VL]; };
            const Vec *vsrc = reinterpret_cast<const Vec *>(src + 1);
            if (need_prev) acc[0] = __dadd_rn(acc[0], __dmul_rn(w, (double)src[0]));
#pragma unroll
            for (int q = 0; q < kRunoffRows / VL; ++q) {
                const Vec x = vsrc[q];                    // rows past T lie in the row padding: read, never used
#pragma unroll
                for (int e = 0; e < VL; ++e) acc[1 + q * VL + e] = __dadd_rn(acc[1 + q * VL + e], __dmul_rn(w, (double)x.v[e]));
            }
            if (need_next) acc[kRunoffRows + 1] = __dadd_rn(acc[kRunoffRows + 1], __dmul_rn(w, (double)src[kRunoffRows + 1]));
        } else {
#pragma unroll
            for (int j = 0; j <= kRunoffRows + 1; ++j) {
                if (j == 0 ? need_prev : (j == kRunoffRows + 1 ? need_next : j <= nt))
                    acc[j] = __dadd_rn(acc[j], __dmul_rn(w, (double)src[(int64_t)j * stride_t]));
            }
        }
    }
    const double a = area ? area[r] : 1.0;
    // Gb of rows t0 .. t0 + 16, last to first, so each row's Gs follows from the row after it (no break, no dynamic index: the
    // loops must unroll for acc[] to stay in registers)
    double out[kRunoffRows];
    double gb_next = 0.0;
#pragma unroll
    for (int j = kRunoffRows + 1; j >= 1; --j) {
        const int64_t t = t0 + j - 1;
        const bool live = j == kRunoffRows + 1 ? need_next : j <= nt;
        const double v = (cumulative && t > 0) ? acc[j] - acc[j - 1] : acc[j];
        const bool pass = live && v == v && (!force_positive || v >= 0.0);
        double gb = 0.0;
        if (pass) {
            const double g = grad_q[t * n_rivers + r];
            gb = area ? __dmul_rn(g, a) : g;      // rounded on its own: the difference below must not contract it into an fma
        }
        if (j <= kRunoffRows) out[j - 1] = cumulative ? __dsub_rn(gb, gb_next) : gb;
        gb_next = gb;
    }
    double2 *dst = reinterpret_cast<double2 *>(gs + r * t_pad + t0);      // t_pad and t0 are multiples of 16: 128-byte aligned
#pragma unroll
    for (int q = 0; q < kRunoffRows / 2; ++q) dst[q] = make_double2(out[2 * q], out[2 * q + 1]);
}

// Point pass.  One lane per grid point and kRunoffAdjChunks chunks of kRunoffRows rows, one after the other: the point's column of the
// transposed structure (t_pairs: the pair indices of the point, ascending), each pair's 16 values of Gs as one 128-byte run, 16 sums in
// registers, and grad_runoff[t, p] for the chunk, adjacent lanes writing adjacent p.  Finding a pair's river and weight costs more than
// its 16 multiply-adds, so a lane does it once for the first kRunoffAdjCache pairs of its column and keeps the results in its own
// column of LDS for all of the block's chunks (no barrier: no lane reads another's); longer columns search again beyond that.
// Every element of grad_runoff is written: a point no river uses gets 0.
constexpr int kRunoffAdjChunks = 8;
constexpr int kRunoffAdjCache = 8;

template <typename RT>
__global__ __launch_bounds__(kBlock) void k_runoff_adjoint_point(const int32_t *__restrict__ indptr, const double *__restrict__ weights,
                                                                 const int32_t *__restrict__ t_indptr, const int32_t *__restrict__ t_pairs,
                                                                 const double *__restrict__ gs, RT *__restrict__ grad_runoff,
                                                                 int64_t grad_stride_t, int64_t n_rivers, int64_t n_points, int64_t T,
                                                                 int64_t t_pad)
{
    __shared__ int32_t river_of[kRunoffAdjCache][kBlock];
    __shared__ double weight_of[kRunoffAdjCache][kBlock];
    const int tid = threadIdx.x;
    const int64_t p = (int64_t)blockIdx.x * kBlock + tid;
    if (p >= n_points) return;
    const int32_t c0 = t_indptr[p], c1 = t_indptr[p + 1];
    for (int j = 0; j < kRunoffAdjCache && c0 + j < c1; ++j) {
        const int32_t k = t_pairs[c0 + j];
        river_of[j][tid] = runoff_pair_river(indptr, (int32_t)n_rivers, k);
        weight_of[j][tid] = weights[k];
    }
    const int64_t first = (int64_t)blockIdx.y * kRunoffAdjChunks * kRunoffRows;
    for (int64_t t0 = first; t0 < min(T, first + (int64_t)kRunoffAdjChunks * kRunoffRows); t0 += kRunoffRows) {
        double acc[kRunoffRows];
#pragma unroll
        for (int j = 0; j < kRunoffRows; ++j) acc[j] = 0.0;
        for (int32_t c = c0; c < c1; ++c) {
            double w;
            int64_t r;
            if (c - c0 < kRunoffAdjCache) {
                w = weight_of[c - c0][tid];
                r = river_of[c - c0][tid];
            } else {
                const int32_t k = t_pairs[c];
                w = weights[k];
                r = runoff_pair_river(indptr, (int32_t)n_rivers, k);
            }
            const double2 *src = reinterpret_cast<const double2 *>(gs + r * t_pad + t0);
#pragma unroll
            for (int q = 0; q < kRunoffRows / 2; ++q) {
                const double2 g = src[q];
                acc[2 * q] = g.x != 0.0 ? __dadd_rn(acc[2 * q], __dmul_rn(w, g.x)) : acc[2 * q];
                acc[2 * q + 1] = g.y != 0.0 ? __dadd_rn(acc[2 * q + 1], __dmul_rn(w, g.y)) : acc[2 * q + 1];
            }
        }
#pragma unroll
        for (int j = 0; j < kRunoffRows; ++j)
            if (t0 + j < T) grad_runoff[(t0 + j) * grad_stride_t + p] = (RT)acc[j];      // float64 sums, rounded once here
    }
}

// Weight pass (only when grad_weights is asked for).  One lane per river, pair after pair of its CSR row (so the river of a pair and
// the number of pairs need no look-up: the call carries neither), each pair serial over the rows in ascending order; Gs[r, .] is read
// as contiguous 128-byte runs, from cache after the row's first pair; with the runoff point-major and padded (VEC, as in the river
// pass) its rows come as 16-byte vectors.
template <typename RT, bool VEC>
__global__ __launch_bounds__(kBlock) void k_runoff_adjoint_weight(const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                                  const RT *__restrict__ runoff, int64_t stride_t, int64_t stride_p,
                                                                  const double *__restrict__ gs, double *__restrict__ grad_weights,
                                                                  int64_t n_rivers, int64_t T, int64_t t_pad)
{
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r >= n_rivers) return;
    const double *row = gs + r * t_pad;
    for (int32_t k = indptr[r]; k < indptr[r + 1]; ++k) {
        const RT *col = runoff + (int64_t)indices[k] * stride_p;
        double acc = 0.0;
        for (int64_t t0 = 0; t0 < T; t0 += kRunoffRows) {
            double g[kRunoffRows], x[kRunoffRows];
#pragma unroll
            for (int q = 0; q < kRunoffRows / 2; ++q) {
                const double2 v = reinterpret_cast<const double2 *>(row + t0)[q];
                g[2 * q] = v.x; g[2 * q + 1] = v.y;
            }
            if (VEC) {
                constexpr int VL = 16 / (int)sizeof(RT);
                struct alignas(16) Vec { RT v[VL]; };
                const Vec *vsrc = reinterpret_cast<const Vec *>(col + t0);
#pragma unroll
                for (int q = 0; q < kRunoffRows / VL; ++q) {
                    const Vec v = vsrc[q];                    // rows past T lie in the row padding; their Gs is 0
#pragma unroll
                    for (int e = 0; e < VL; ++e) x[q * VL + e] = (double)v.v[e];
                }
            } else {
#pragma unroll
                for (int j = 0; j < kRunoffRows; ++j) x[j] = t0 + j < T ? (double)col[(t0 + j) * stride_t] : 0.0;
            }
#pragma unroll
            for (int j = 0; j < kRunoffRows; ++j) acc = g[j] != 0.0 ? __dadd_rn(acc, __dmul_rn(g[j], x[j])) : acc;
        }
        grad_weights[k] = acc;
    }
}

}  // namespace
