/*
 * rr_hip.h -- C ABI of librr_hip.so, the MI355X (gfx950) Muskingum routing engine.
 *
 * Drop-in boundary: these entry points replace the reference's kernel boundary, i.e. the three
 * numba functions and the UH convolution that the reference's routers call once per input file
 * (citations relative to the reference repository root):
 *
 *   rr_rapid_route      <- rapid_route      river_route/routers/_numba_kernels.py:49-84
 *                          (call site river_route/routers/RapidMuskingum.py:27-32)
 *   rr_muskingum_route  <- muskingum_route  river_route/routers/_numba_kernels.py:8-46
 *                          (call site river_route/routers/Muskingum.py:281-286)
 *   rr_unit_route       <- unit_route       river_route/routers/_numba_kernels.py:88-171
 *                          (call site river_route/routers/UnitMuskingum.py:82-92)
 *   rr_uh_convolve      <- UnitHydrograph.convolve  river_route/uhkernels/UnitHydrograph.py:77-107
 *                          (call site river_route/routers/UnitMuskingum.py:75)
 *   rr_unit_adjoint_dev <- the gradient of a loss through unit_route (same lines), rr_uh_adjoint_dev <- through
 *                          UnitHydrograph.convolve (same lines); rr_rapid_adjoint_dev <- through rapid_route;
 *                          rr_rapid_adjoint_batch_dev, rr_unit_adjoint_batch_dev <- through several such calls at once;
 *                          rr_rapid_adjoint_gauges_dev, rr_unit_adjoint_gauges_dev <- through rapid_route / unit_route with a loss
 *                          at gauged reaches only
 *   rr_plan_create      <- the CSC structure the routers take from tools.adjacency_matrix
 *                          (river_route/tools.py:75-109; river_route/routers/Muskingum.py:189-192)
 *   rr_plan_set_coeffs  <- the coefficient vectors of Muskingum._set_muskingum_coefficients
 *                          (river_route/routers/Muskingum.py:172-193) and c4_dt of RapidMuskingum.py:24
 *
 * Conventions
 *   - plain pointers and sizes only; all floating point is IEEE fp64; CSC indices are int32
 *     (what scipy hands the reference); hw/inner positions are implied by the adjacency.
 *   - every function returns RR_OK (0) or a negative RR_E_* code and never throws; the message of
 *     the last failure on the calling thread is rr_last_error().
 *   - arrays are C-contiguous; 2-D arrays are (time, reach) row-major in PARAMS-FILE reach order,
 *     exactly as the reference passes them.  The engine keeps its own permuted device layout.
 *   - `*_dev` variants take DEVICE pointers (valid on the plan's GPU) and a hipStream_t passed as
 *     void*; they only enqueue work: nothing in them allocates or synchronises (work memory comes
 *     from rr_plan_reserve -- a BREAK against the first versions of this ABI, see INTEGRATION.md: a
 *     `_dev` call or rr_stream_begin* without a reservation at least as large returns RR_E_STATE).  Every
 *     kernel of a call is enqueued on the caller's stream.  The un-suffixed variants take HOST pointers,
 *     copy in/out, and return when the results are in the caller's buffers.
 *   - a plan is bound to one GPU and is not thread-safe; use one plan per thread/stream.
 *   - there is NO CPU fallback: without a usable gfx950 device every compute call fails with
 *     RR_E_NO_DEVICE.  rr_plan_create(device = RR_DEVICE_NONE) builds a host-only plan whose
 *     layout can be inspected (rr_plan_info / rr_plan_layout) but which cannot compute.
 */
#ifndef RR_HIP_H
#define RR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RR_OK 0
#define RR_E_INVALID (-1)         /* bad argument (null pointer, negative size, malformed CSC) */
#define RR_E_NOT_TOPOLOGICAL (-2) /* a CSC entry has row <= column: reaches not sorted upstream -> downstream */
#define RR_E_HIP (-3)             /* HIP runtime failure; text in rr_last_error() */
#define RR_E_NO_DEVICE (-4)       /* no usable GPU, or host-only plan asked to compute */
#define RR_E_STATE (-5)           /* call order (e.g. route before rr_plan_set_coeffs) */
#define RR_E_ALLOC (-6)           /* host or device allocation failed */
#define RR_E_UNSUPPORTED (-7)     /* structure outside what the engine handles */

#define RR_DEVICE_NONE (-1)

typedef struct rr_plan rr_plan;

/* ---- library ---- */
int rr_version(void);             /* major*10000 + minor*100 + patch */
const char *rr_last_error(void);  /* thread-local, never NULL */
int rr_device_count(void);        /* number of visible HIP devices, 0 when there is none */

/* ---- plan: network structure analysis + device-resident layout ---- */

/* n reaches; CSC of A[down, up] = 1 with n columns: csc_indptr[n+1], csc_indices[csc_indptr[n]].
 * Validates what tools.adjacency_matrix guarantees (row > column for every entry).  device is a
 * HIP device ordinal or RR_DEVICE_NONE. */
int rr_plan_create(int64_t n, const int32_t *csc_indptr, const int32_t *csc_indices, int device, rr_plan **out);
void rr_plan_destroy(rr_plan *plan);

/* info[0]=n, [1]=edges, [2]=depth (reaches on the longest flow path), [3]=widest level,
 * [4]=headwaters, [5]=outlets, [6]=1 if the engine's order equals params order (no permutation pass),
 * [7]=device ordinal or -1. */
int rr_plan_info(const rr_plan *plan, int64_t info[8]);

/* Engine layout for inspection/tests (any pointer may be NULL): perm[n] params index held at each
 * engine position; lag[n] pipeline lag of each position (ticks behind the farthest headwater);
 * child_ptr[n+1] engine-position range [child_ptr[p], child_ptr[p+1]) of the reaches flowing into p. */
int rr_plan_layout(const rr_plan *plan, int32_t *perm, int32_t *lag, int32_t *child_ptr);

/* Layout of the time-tiled kernel (subtree tiles), for inspection/tests.
 * info[0]=1 if the network tiles (else the streaming kernel routes it), [1]=tile capacity in positions, [2]=positions
 * (reaches + ghosts), [3]=ghosts, [4]=tiles, [5]=tile levels, [6]=threads per workgroup, [7]=rows the passes between
 * params-order rows and the kernel's records move per launch (a cyclic discharge array with at least that many rows is never
 * written twice by one launch).
 * rr_plan_tile_layout (any pointer may be NULL): tile_ptr[tiles+1] first position of each tile; tile_level[tiles];
 * perm[np] params index of the reach at (or mirrored by) each position; lag[np] pipeline lag, bit 28 set on a ghost, bit 27 on
 * a reach that a ghost of another tile mirrors; cfirst[np] first upstream position; ccnt[np] upstream positions (low 16 bits)
 * and how many of them are headwaters (high 16 bits, they come first); xpos[np] position of the mirroring ghost / mirrored
 * reach, -1 elsewhere. */
int rr_plan_tile_info(const rr_plan *plan, int64_t info[8]);
/* Headwaters the in-pass routes: with one sub-step per row the record pass that turns lateral rows into
 * records also routes the headwaters among them, and the time-tiled kernel never writes their records back.  info[0]=1 unless
 * RR_HW_INPASS=0 switched it off, [1]=eligible positions of the tile layout, [2]=positions that own a reach without an upstream
 * position in their tile, [3]=of those, left out because a ghost of another tile mirrors them or they are boundary ghosts of a
 * partitioned network, [4]=left out because their tile holds a reach with more than three upstream reaches.  Once the plan has
 * coefficients, a headwater whose c2 is not finite is left out of [1] as well (it is counted in [2] only). */
int rr_plan_inpass_info(const rr_plan *plan, int64_t info[5]);
int rr_plan_tile_layout(const rr_plan *plan, int32_t *tile_ptr, int32_t *tile_level, int32_t *perm, int32_t *lag,
                        int32_t *cfirst, uint32_t *ccnt, int32_t *xpos);

/* Coefficients in params order.  lhs_off_data[e] is the off-diagonal of (I - diag(c1) A) for CSC entry e,
 * i.e. -c1[row(e)] (Muskingum.py:192); c2, c3 per reach; c4_dt per reach or NULL (channel-only / unit). */
int rr_plan_set_coeffs(rr_plan *plan, const double *lhs_off_data, const double *c2, const double *c3,
                       const double *c4_dt);

/* UnitMuskingum with general edge data: the reference's unit_route multiplies by a_inner_data[j] / a_hw_data[j] and
 * subtracts lhs_off_data[j] q_ch (river_route/routers/_numba_kernels.py:126-139, 159-162); its own callers pass ones and
 * -c1[row], which is what rr_plan_set_coeffs alone describes.  For other values: c1[n] per reach (params order, any value
 * on headwaters) and a_data per entry of the plan's CSC structure (a_inner_data / a_hw_data of that edge);
 * lhs_off_data of rr_plan_set_coeffs is then read for the edges between two reaches that have upstream reaches only.
 * Such a plan routes UnitMuskingum with the streaming kernel.  (NULL, NULL) goes back to unit weights. */
int rr_plan_set_unit_weights(rr_plan *plan, const double *c1, const double *a_data);

/* Work memory of the route calls to come, allocated up front: the *_dev entry points and rr_stream_begin* only enqueue
 * work and return RR_E_STATE (with the byte count in rr_last_error()) when a call needs more than has been reserved; the
 * host-pointer entry points, which synchronise anyway, reserve by themselves.  Reserve once per plan for the largest
 * call (T runoff rows x nsub sub-steps; rr_muskingum_route*: T = num_output_steps, nsub = num_routing_per_output), after
 * rr_plan_set_coeffs and rr_plan_set_boundary / rr_plan_set_options: one call per input file is the reference's pattern
 * (river_route/routers/TransformMuskingum.py:108-148), and the routers reserve in _hook_before_route.  Memory only
 * grows; a smaller call fits a larger reservation.  host_rows: bit 0 also prepares the staging of the host-pointer entry
 * points (pinned buffers and device rings of the PCIe pipeline); RR_ROWS_NOT_PLAIN: the call does not hand over lateral rows
 * in a device array (fused convolution, gridded runoff: rr_unit_route_uh*_dev, rr_rapid_route_runoff_dev), so the direct row path
 * -- which rr_rapid_route*_dev and rr_stream_begin take where the params order numbers small subtrees contiguously, see
 * rr_plan_direct_info -- does not apply and the record ring is needed; RR_ROWS_F32_OUT: the call writes float32 rows
 * (rr_*_route_f32*_dev: the direct task is then a multiple of 128 rows); RR_ROWS_UH: the call is rr_unit_route_uh*_dev (runoff
 * depths + unit-hydrograph kernel): on the direct row path -- which rr_unit_route*_dev take too, with up to four sub-steps per row and no
 * boundary reaches -- the convolution runs as a pass of its own into T rows of work memory, reserved here.
 * info (may be NULL): [0] 2 = direct row path, 1 = time-tiled kernel, 0 = streaming kernel; [1] routing ticks (rows) per launch K; [2] chunks of the
 * record ring (16 ticks each); [3] bytes of routing work memory now held on the device; [4] bytes of device staging and
 * [5] of pinned host staging of the host-pointer path; [6] depth of the routing pipeline in ticks (network depth + tile
 * levels x K: a call's first output row leaves this many ticks after its first input row entered); [7] bytes of the record
 * ring (or streaming work rows) this shape needs. */
#define RR_MODE_RAPID 0
#define RR_MODE_MUSKINGUM 1
#define RR_MODE_UNIT 2
#define RR_ROWS_NOT_PLAIN 2
#define RR_ROWS_F32_OUT 4
#define RR_ROWS_UH 8
int rr_plan_reserve(rr_plan *plan, int mode, int64_t T, int64_t nsub, int host_rows, int64_t info[8]);

/* The direct row path: where the params order numbers every small subtree contiguously -- any depth-first
 * post-order does (a valid order for tools.adjacency_matrix, river_route/tools.py:103-104) -- RapidMuskingum calls with one
 * sub-step per row on float64 device rows (rr_rapid_route_dev, rr_stream_begin) are routed straight from and to the caller's rows
 * by column-range tiles: no record ring and no permutation pass for 95 % of the columns.
 * info: [0] 1 = applies to this plan; [1] direct tiles; [2] holes (columns of skeleton reaches); [3] outlets that feed the
 * skeleton; [4] positions, [5] tiles, [6] tile levels of the skeleton; [7] rows of the LDS window.  why (may be NULL): the
 * reason it does not apply.  rr_plan_direct_layout: tile arrays [tiles], per-column arrays [n]; any pointer may be NULL. */
int rr_plan_direct_info(const rr_plan *plan, int64_t info[8], char *why, int64_t why_cap);
int rr_plan_direct_layout(const rr_plan *plan, int32_t *tile_c0, int32_t *tile_nc, int32_t *tile_lag_lo, int32_t *tile_span,
                          int32_t *delay, int32_t *up3, int32_t *xinfo);
/* The kernels around the routing kernel in the last call, sampled like it (every fourth launch between HIP events on the call's
 * stream, while rr_plan_set_options(sample_every >= 16) is in force): aux[3 k + 0] launches, [3 k + 1] launches sampled,
 * [3 k + 2] their milliseconds, for k = 0 the in-pass (params-order rows -> records), 1 the out-pass, 2 the skeleton's routing
 * launches of the direct row path, 3 its out-pass over the holes. */
int rr_plan_profile_aux(rr_plan *plan, double aux[12]);
/* Which routing kernel the last call on this plan ran. */
#define RR_KERNEL_TICK 0
#define RR_KERNEL_TILE 1
#define RR_KERNEL_DIRECT 2
#define RR_KERNEL_TILE_ENSEMBLE 3      /* rr_rapid_route_ensemble_dev: the time-tiled kernel over (tile, member) tasks */
int rr_plan_last_kernel(const rr_plan *plan);

/* Byte order of the FLOAT32 rows of the calls to come (rr_*_f32in_dev's lateral / depth rows, rr_*_f32*_dev's discharge rows): non-zero =
 * big-endian, as a NetCDF-3 file stores them, so that a file's bytes go to the device and come back from it as they are (rr_rows_upload /
 * rr_rows_download) and the conversion costs one instruction per value in the kernels that read or write the rows anyway.  Default: native. */
int rr_plan_set_row_format(rr_plan *plan, int in32_big_endian, int out32_big_endian);

/* Tuning / measurement.  rows_per_chunk: time rows moved per permutation launch of the streaming kernel (default 16).
 * sample_every >= 16: HIP-event brackets on the call's stream around sampled routing launches (every fourth launch of the
 * time-tiled kernel; every sample_every-th tick of the streaming kernel opens a bracket of 16 launches); 0 switches it off. */
int rr_plan_set_options(rr_plan *plan, int64_t rows_per_chunk, int64_t sample_every);

/* prof[0]=routing launches of the last route call, [1]=routing ticks inside brackets, [2]=sum of the bracket
 * durations (ms), [3]/[4]=smallest/largest per-launch mean of a bracket (ms), [5]=reaches updated by the
 * bracketed launches,
 * [6]=ms between the first and the last routing-step launch of the call (permutation passes included),
 * [7]=reach-steps of the call, [8]=number of brackets, [9]=routing ticks per launch (K of the time-tiled
 * kernel, 1 for the streaming kernel).  Synchronises the plan's last stream. */
int rr_plan_profile(rr_plan *plan, double prof[10]);

/* ---- routing, host pointers (the reference's kernel boundary) ---- */

/* q_t[n] in: initial state, out: state after the last sub-step.  qlateral[T*n], discharge[T*n].
 * discharge[t, i] = max(mean over the nsub sub-steps of step t of q[i], 0). */
int rr_rapid_route(rr_plan *plan, double *q_t, const double *qlateral, double *discharge,
                   int64_t num_runoff_steps, int64_t num_substeps);

/* discharge[num_output_steps * n]; each output row averages num_routing_per_output sub-steps. */
int rr_muskingum_route(rr_plan *plan, double *q_t, double *discharge,
                       int64_t num_output_steps, int64_t num_routing_per_output);

/* Plan built on the FULL adjacency; headwaters are the reaches with no upstream entry, inner reaches the
 * rest, both in ascending params order (UnitMuskingum.py:41-44).  q_ch[n_inner], q_full[n_inner] in/out;
 * convolved_lateral[T*n], discharge[T*n] over all n reaches. */
int rr_unit_route(rr_plan *plan, double *q_ch, double *q_full, const double *convolved_lateral,
                  double *discharge, int64_t num_runoff_steps, int64_t num_substeps);

/* kernel[n_ks*n], state[n_ks*n] in/out (carry-over), lateral[T*n] -> out[T*n].  No plan needed. */
int rr_uh_convolve(int device, const double *kernel, double *state, const double *lateral, double *out,
                   int64_t T, int64_t n_ks, int64_t n);

/* ---- routing, device pointers + stream ---- */

/* As above with device pointers.  qlateral has ql_rows rows and step t reads row t % ql_rows;
 * discharge has out_rows rows and step t writes row t % out_rows (pass T for plain arrays). */
int rr_rapid_route_dev(rr_plan *plan, double *q_t, const double *qlateral, int64_t ql_rows,
                       double *discharge, int64_t out_rows, int64_t num_runoff_steps, int64_t num_substeps,
                       void *stream);
int rr_muskingum_route_dev(rr_plan *plan, double *q_t, double *discharge, int64_t out_rows,
                           int64_t num_output_steps, int64_t num_routing_per_output, void *stream);
int rr_unit_route_dev(rr_plan *plan, double *q_ch, double *q_full, const double *convolved_lateral,
                      int64_t conv_rows, double *discharge, int64_t out_rows,
                      int64_t num_runoff_steps, int64_t num_substeps, void *stream);
int rr_uh_convolve_dev(int device, const double *kernel, double *state, const double *lateral, double *out,
                       int64_t T, int64_t n_ks, int64_t n, void *stream);

/* The same with the routers' post-processing (river_route/routers/TransformMuskingum.py:128-142) fused into the pass that
 * returns the rows to params order: discharge32[o, i] = (float) mean_{j < factor} discharge[o * factor + j, i], (T / factor, n)
 * rows, 4 bytes written per value instead of 8 + 8 + 4.  RR_E_UNSUPPORTED when the call is not time-tiled or factor x
 * sub-steps does not divide 128: use the float64 form and rr_resample_cast_dev then. */
int rr_rapid_route_f32_dev(rr_plan *plan, double *q_t, const double *qlateral, int64_t ql_rows, float *discharge32,
                           int64_t num_runoff_steps, int64_t num_substeps, int64_t factor, void *stream);
/* rr_rapid_route_dev with float32 lateral rows, as qlateral files store them: 4 bytes read per value instead of 8, and the
 * routers upload half the bytes; float32 -> float64 is exact, so the result equals rr_rapid_route_dev on the converted rows
 * bit for bit.  Exactly one of discharge (float64 rows, out_rows >= 1 cyclic) and discharge32 (float32 rows, `factor` routed
 * rows averaged, as rr_rapid_route_f32_dev).  Time-tiled kernel only (RR_E_UNSUPPORTED otherwise: convert and call
 * rr_rapid_route_dev). */
int rr_rapid_route_f32in_dev(rr_plan *plan, double *q_t, const float *qlateral32, int64_t ql_rows, double *discharge, int64_t out_rows,
                             float *discharge32, int64_t factor, int64_t T, int64_t nsub, void *stream);

/* Ensembles: `members` RapidMuskingum calls over the same period on one plan -- same network, coefficients and shape, each member
 * with its own lateral rows, discharge rows and initial state -- routed together on the time-tiled kernel.  One launch runs the
 * (tile, member) tasks of every member, so the pipeline's fill and drain (rr_plan_reserve's info[6] ticks) is paid once per group
 * instead of once per member, and a network of a few hundred tiles still fills the card.  Member m's results are bit for bit those of
 * rr_rapid_route_dev / _f32_dev / _f32in_dev on member m's rows (time-tiled) -- with one exception at one sub-step
 * per row: the batched call runs the general tick there where a single-member call runs the short one (RR_TILE_LEAN), whose sums of
 * three upstream values may differ in the sign of a zero (-0.0 against +0.0) when every term is a negative zero.
 * rr_plan_reserve_ensemble: the work memory of such calls (one record ring per member, and the members' carried state); flags:
 * RR_ROWS_F32_IN (float32 lateral rows) | RR_ROWS_F32_OUT (float32 discharge rows).  info as rr_plan_reserve's ([0] is 1), plus
 * [8] the largest member count whose record rings fit the card at this shape (reserve and route groups of at most that many).
 * rr_rapid_route_ensemble_dev only enqueues.  Rows are whole calls: member m's T lateral rows (float64, or float32 with lateral_is_f32)
 * start at lateral + m * lateral_member_pitch elements; its discharge rows at discharge + m * discharge_member_pitch elements: T float64
 * rows, or with discharge_is_f32 T / factor float32 rows, each the mean of `factor` routed rows (as rr_rapid_route_f32_dev).  q_t holds
 * member m's initial state at q_t + m * q_pitch on entry, its final state on return.  RR_E_INVALID: members < 1 (or > 65535), a null
 * array, a pitch shorter than a member; RR_E_STATE: more than was reserved (the message names the rr_plan_reserve_ensemble call to
 * make); RR_E_UNSUPPORTED, with the reason: the call would not get the time-tiled kernel -- per-edge weights, T x nsub < 32, a plan
 * with boundary reaches, or record rings too large for the card (fewer members per call). */
#define RR_ROWS_F32_IN 16
int rr_plan_reserve_ensemble(rr_plan *plan, int64_t members, int64_t T, int64_t nsub, int flags, int64_t info[9]);
int rr_rapid_route_ensemble_dev(rr_plan *plan, int64_t members, double *q_t, int64_t q_pitch, const void *lateral, int lateral_is_f32,
                                int64_t lateral_member_pitch, void *discharge, int discharge_is_f32, int64_t discharge_member_pitch,
                                int64_t factor, int64_t T, int64_t nsub, void *stream);
/* Parameter ensembles: the members of an ensemble call with a coefficient set each -- one basin, one forcing, `members` (k, x) sets: a
 * generation of a population-based calibration, the samples of a sensitivity analysis.
 * rr_plan_set_member_coeffs takes host arrays, as rr_plan_set_coeffs does: member m's lhs_off_data (n_edges values) at + m * lhs_pitch,
 * its c2, c3 and c4_dt (n values each, params order) at + m * pitch.  It builds per member what rr_plan_set_coeffs builds for the
 * time-tiled general tick -- {c1row, c2, c3} per position in tile order (zeros at tile ghosts) and c4dt in params order -- and keeps them
 * on the device beside the plan's own coefficient set, which it does not touch: every other call on the plan computes what it did.  A
 * later call replaces the tables.  RR_E_INVALID: members < 1 (or > 65535), a null array (c4_dt included), pitch < n, lhs_pitch < n_edges
 * with more than one member; RR_E_UNSUPPORTED: a member with two tributaries of one reach at different weights (the message names the
 * member; there is no streaming fallback here); RR_E_STATE: a routing call is open.
 * rr_rapid_route_members_dev is rr_rapid_route_ensemble_dev, argument for argument, with member m routed by coefficient set m.
 * lateral_member_pitch == 0: one forcing (T rows) shared by all members.  RR_E_STATE if fewer sets than `members` were set (the message
 * names the rr_plan_set_member_coeffs call to make).  Work memory: rr_plan_reserve_ensemble's, which either setter allows; the plan needs
 * no rr_plan_set_coeffs for this call.  Every member runs the general tick: member m's results are bit for bit those of
 * rr_plan_set_coeffs(member m's arrays) + a one-member rr_rapid_route_ensemble_dev.  rr_plan_last_kernel: RR_KERNEL_TILE_ENSEMBLE. */
int rr_plan_set_member_coeffs(rr_plan *plan, int64_t members,
                              const double *lhs_off_data, int64_t lhs_pitch,   /* member m: n_edges values at + m * lhs_pitch */
                              const double *c2, const double *c3, const double *c4_dt, int64_t pitch);   /* member m: n values at + m * pitch */
int rr_rapid_route_members_dev(rr_plan *plan, int64_t members, double *q_t, int64_t q_pitch,
                               const void *lateral, int lateral_is_f32, int64_t lateral_member_pitch,
                               void *discharge, int discharge_is_f32, int64_t discharge_member_pitch,
                               int64_t factor, int64_t T, int64_t nsub, void *stream);
int rr_muskingum_route_f32_dev(rr_plan *plan, double *q_t, float *discharge32, int64_t num_output_steps,
                               int64_t num_routing_per_output, void *stream);
int rr_unit_route_f32_dev(rr_plan *plan, double *q_ch, double *q_full, const double *convolved_lateral, int64_t conv_rows,
                          float *discharge32, int64_t num_runoff_steps, int64_t num_substeps, int64_t factor, void *stream);

/* RapidMuskingum fed by gridded runoff (river_route/routers/TransformMuskingum.py:38-51 -> runoff.py:288-332 -> RapidMuskingum.py:
 * 19-33 in one call, one sub-step per row): the weights product of rr_runoff_to_qlateral_dev (same arguments, device arrays;
 * pass area: the routers route volumes) runs inside the pass that builds the engine's records, so the catchment inflow never
 * exists as (T, n) rows.  Exactly one of discharge (float64, T rows) / discharge32 (float32, T / factor rows) is non-NULL.
 * RR_E_UNSUPPORTED where the call is not time-tiled (use rr_runoff_to_qlateral_dev + rr_rapid_route_dev). */
int rr_rapid_route_runoff_dev(rr_plan *plan, double *q_t, int64_t n_points, const int32_t *indptr, const int32_t *indices,
                              const double *weights, const void *runoff, int runoff_is_f32, int64_t stride_t, int64_t stride_p,
                              const double *area, int flags, double *discharge, float *discharge32, int64_t factor,
                              int64_t num_runoff_steps, void *stream);

/* UnitMuskingum with the unit-hydrograph convolution fused into the pass that turns rows into the engine's records
 * (river_route/routers/UnitMuskingum.py:72-98 in one call): depth[T*n] runoff depths, uh_kernel[n_ks*n], uh_state[n_ks*n]
 * in/out (carry-over, updated in place), n_ks <= 64.  Exactly one of discharge (float64, T rows) / discharge32 (float32,
 * T / factor rows, `factor` rows averaged) is non-NULL.  q_final[n] (may be NULL) receives the state the router keeps: the
 * last lateral inflow on headwaters, q_full on inner reaches.  The convolved lateral never exists as rows in memory.
 * RR_E_UNSUPPORTED where the call is not time-tiled (use rr_uh_convolve_dev + rr_unit_route_dev). */
int rr_unit_route_uh_dev(rr_plan *plan, double *q_ch, double *q_full, double *q_final, const double *uh_kernel, double *uh_state,
                         int64_t n_ks, const double *depth, double *discharge, float *discharge32, int64_t factor,
                         int64_t num_runoff_steps, int64_t num_substeps, void *stream);
/* The same with float32 runoff depths, as runoff files usually store them (4 bytes read and uploaded per value instead of 8;
 * float32 -> float64 is exact, so the results are those of the float64 copy, bit for bit). */
int rr_unit_route_uh_f32in_dev(rr_plan *plan, double *q_ch, double *q_full, double *q_final, const double *uh_kernel, double *uh_state,
                               int64_t n_ks, const float *depth32, double *discharge, float *discharge32, int64_t factor,
                               int64_t num_runoff_steps, int64_t num_substeps, void *stream);

/* ---- partitioned networks (multi-GPU): boundary reaches and streaming calls ----
 *
 * A network cut into parts (rr_partition_forest) is routed one part per GPU.  In the part that holds the
 * DOWNSTREAM end of a cut edge the upstream reach appears as a GHOST: a headwater column of the part's local
 * network whose discharge at every sub-step is prescribed from `ghost_series`; in the part that owns it the
 * reach is an EXPORT reach whose discharge after every sub-step is recorded in `export_series`.  Both series
 * are device arrays of shape (T * nsub, n_ghost) / (T * nsub, n_export), row = sub-step.  The streaming
 * calls keep the lag pipeline full while series arrive in batches (no drain between batches). */

/* Reaches are LOCAL params indices of this plan.  A ghost's value is prescribed, so whatever the local network puts upstream
 * of it is ignored.  UnitMuskingum distinguishes headwater tributaries from the others (_numba_kernels.py:150-156): a ghost
 * that mirrors a reach WITH upstream reaches must itself have one in the local network (a dummy headwater whose lateral
 * column is zero does), so that it falls on the same side of that distinction as the reach it mirrors, and it then has an
 * entry in the q_ch / q_full arrays, whose q_full is the mirrored reach's.
 * A call that fails after its arguments were accepted (RR_E_ALLOC, RR_E_HIP) leaves the plan between two boundaries: every route call
 * returns RR_E_STATE until rr_plan_set_boundary has been repeated and has succeeded; the plan can be destroyed as it is. */
int rr_plan_set_boundary(rr_plan *plan, int64_t n_ghost, const int64_t *ghost_reaches, int64_t n_export,
                         const int64_t *export_reaches);

/* Opens a routing call on device arrays (has_lateral = 1: RapidMuskingum, 0: channel-only Muskingum).
 * q_t[n]: initial state (ghost entries = the upstream reach's initial discharge).
 * lateral / discharge are read / written cyclically (step t: row t % lat_rows, row t % out_rows).  A caller that REFILLS a lateral
 * ring shorter than the call between two rr_stream_advance calls may announce at most lat_rows rows beyond those the engine has
 * taken; the engine takes them in whole batches -- 128 tick-rows (+ 15 of overlap) on the record path, K rows on the direct row path,
 * where K (rr_plan_reserve's info[1]) is capped to the largest multiple of 16 that fits BOTH rings (rings of fewer than 32 rows keep
 * to records) -- so a refilled ring must hold at least one such batch.  On the direct row path the columns of skeleton reaches are
 * patched into a discharge row info[6] (the pipeline's depth) rows after the row was first written: a cyclic discharge ring that the
 * caller drains while the call is open must be that long (or T rows), or the call must be reserved with RR_ROWS_NOT_PLAIN. */
int rr_stream_begin(rr_plan *plan, int has_lateral, const double *q_t, const double *lateral, int64_t lat_rows,
                    double *discharge, int64_t out_rows, int64_t T, int64_t nsub, const double *ghost_series,
                    double *export_series, void *stream);
/* Enqueues every routing tick whose inputs are present: lateral rows [0, lateral_rows_ready) and ghost
 * sub-steps [0, ghost_substeps_ready).  *export_substeps_ready = leading sub-steps of export_series that are
 * final once the enqueued work has run. */
int rr_stream_advance(rr_plan *plan, int64_t lateral_rows_ready, int64_t ghost_substeps_ready,
                      int64_t *export_substeps_ready);
/* Closes the call (all T steps must have been routed) and writes the final state to q_t[n] (may be NULL). */
int rr_stream_end(rr_plan *plan, double *q_t);

/* The same for UnitMuskingum (river_route/routers/_numba_kernels.py:88-171 on one part of a cut network): lateral = the
 * convolved runoff depths of this part's columns (rr_uh_convolve_dev; ghost columns are not read), q_ch / q_full over the
 * local reaches that have upstream reaches, ascending local index.  Export series hold the discharge a reach publishes
 * (q_full; the lateral inflow on a headwater).  Advance with rr_stream_advance. */
int rr_stream_begin_unit(rr_plan *plan, const double *q_ch, const double *q_full, const double *lateral, int64_t lat_rows,
                         double *discharge, int64_t out_rows, int64_t T, int64_t nsub, const double *ghost_series,
                         double *export_series, void *stream);
/* Closes the call and writes the final q_ch / q_full (both may be NULL). */
int rr_stream_end_unit(rr_plan *plan, double *q_ch, double *q_full);

/* Cuts a forest into at most n_parts balanced parts whose part graph is acyclic (boundary discharge flows one way):
 * main stems + the tributaries joining them farthest upstream in the last part, the other subtrees spread over the
 * rest (part graph of depth two); chain-like networks fall back to a nested min-max cut.
 * part_of[n] receives the part of every reach, parts are numbered upstream-first; part_sizes[n_parts] (may be NULL)
 * their sizes.  Host-only, needs no GPU. */
int rr_partition_forest(int64_t n, const int32_t *csc_indptr, const int32_t *csc_indices, int32_t n_parts,
                        int32_t *part_of, int64_t *part_sizes);

/* Depth-first post-order of a river network given as one downstream ROW index per reach (-1 at outlets), rows in ANY order:
 * order[k] = the row that comes k-th.  Every reach follows the whole sub-basin of each of its tributaries, so every sub-basin is a run
 * of consecutive rows -- still a valid order for river_route/tools.py:103-104 (upstream before downstream), and the one in which
 * rr_rapid_route_dev / rr_stream_begin route straight from and to the caller's rows (rr_plan_direct_info).  A reach's tributaries
 * are visited small sub-basins first (at most 256 reaches: what one tile of the direct row path holds; the largest of them first), then
 * the large ones, the largest last -- so the reaches of a main stem end up side by side behind the small sub-basins that join it, and the
 * 8-byte stores that patch them into the output rows share lines; outlets in ascending row index.  RR_E_INVALID for an index out of
 * range or a cycle.
 * Host-only, needs no GPU. */
int rr_postorder(int64_t n, const int64_t *down_index, int64_t *order);

/* ---- router post-processing on the device (river_route/routers/TransformMuskingum.py:128-142) ----
 * out[o, i] = (float) mean_{j < factor} discharge[o * factor + j, i]; num_rows must be a multiple of factor.
 * Halves (or better) the bytes that leave the GPU: the reference's routers hand float32 to their writer. */
int rr_resample_cast_dev(int device, const double *discharge, int64_t num_rows, int64_t n, int64_t factor, float *out,
                         void *stream);

/* ---- gridded runoff -> catchment lateral inflow (river_route/runoff.py:288-330) ----
 * qlateral[t, r] = sum over the CSR row r of weights[k] * runoff(t, indices[k]), then, in the reference's order:
 * RR_RUNOFF_CUMULATIVE input -> incremental (row t minus row t - 1, row 0 kept), RR_RUNOFF_FORCE_POSITIVE -> clip at 0,
 * NaN -> 0 (unless RR_RUNOFF_KEEP_NAN: the host resamples irregular time steps before filling), and, when
 * area != NULL, times area[r] (volumes, the routers' as_volumes=True).  weights = proportion * unit conversion.
 * runoff element (t, p) is at runoff[t * stride_t + p * stride_p] (float when runoff_is_f32, else double): pass the
 * block point-major (stride_t = 1, stride_p >= T) for contiguous gathers -- with stride_p a multiple of 16 and the rows
 * allocated in full (n_points * stride_p elements, 16-byte aligned) they are read as 16-byte vectors -- or as read
 * from the file (stride_p = 1).
 * The non-uniform-time resampling of the reference (pandas, runoff.py:313-325) stays on the host.
 * rr_runoff_to_qlateral takes host arrays; the _dev form takes device arrays and only enqueues on `stream`. */
#define RR_RUNOFF_CUMULATIVE 1
#define RR_RUNOFF_FORCE_POSITIVE 2
#define RR_RUNOFF_KEEP_NAN 4
int rr_runoff_to_qlateral(int device, int64_t n_rivers, int64_t n_points, int64_t T, const int32_t *indptr,
                          const int32_t *indices, const double *weights, const void *runoff, int runoff_is_f32,
                          int64_t stride_t, int64_t stride_p, const double *area, int flags, double *qlateral);
int rr_runoff_to_qlateral_dev(int device, int64_t n_rivers, int64_t n_points, int64_t T, const int32_t *indptr,
                              const int32_t *indices, const double *weights, const void *runoff, int runoff_is_f32,
                              int64_t stride_t, int64_t stride_p, const double *area, int flags, double *qlateral,
                              void *stream);

/* ---- skill scores of (time, reach) rows on the device (river_route/metrics.py; DESIGN.md section "Skill scores") ----
 * Per column j of n: y_true[r, j] against y_pred[r, pred_columns[j]] (pred_columns NULL: column j), r < rows.  Element (r, c)
 * of an array is at base[r * pitch + c] (pitch in elements, >= the columns read), float when *_is_f32, else double; both are
 * widened to double.  `state` is RR_METRICS_STATE x n doubles, field-major (state[k * n + j]), zero-filled by the caller
 * before the first update; each update merges its rows into it, so a series may arrive in row blocks (same inputs and
 * the same sequence of updates: bit-identical results).  An update needs rr_metrics_work_bytes bytes of work memory (0
 * when rows == 0).  rr_metrics_finish_dev writes out[5 * n]: out[k * n + j] = mean error, mean absolute error, mean
 * square error, Pearson r, KGE-2012 of column j, with the reference's NaN rules (a column without rows: all NaN).
 * The _dev calls only enqueue on `stream` and allocate nothing; pred_columns is not range-checked on the device. */
#define RR_METRICS_STATE 9
#define RR_METRICS_SCORES 5
int rr_metrics_work_bytes(int64_t n, int64_t rows, int64_t *bytes);
int rr_metrics_update_dev(int device, int64_t n, int64_t rows, const void *y_true, int true_is_f32, int64_t true_pitch,
                          const void *y_pred, int pred_is_f32, int64_t pred_pitch, const int32_t *pred_columns, double *state,
                          void *work, int64_t work_bytes, void *stream);
int rr_metrics_finish_dev(int device, int64_t n, const double *state, double *out, void *stream);

/* ---- catchment / grid-cell overlap areas (river_route/runoff.py:70-116) ----
 * The area in m^2 of each catchment row clipped to each candidate cell of a regular lon/lat grid, measured as the reference
 * measures it: intersected with straight edges in degrees, projected to the cylindrical equal-area projection (PROJ's
 * +proj=cea on GRS80, lat_ts 0), shoelace area.  Cells are the rectangles [x_bounds[i], x_bounds[i+1]] x [y_bounds[j],
 * y_bounds[j+1]], both bound arrays strictly ascending (nx + 1 and ny + 1 values, degrees; bounds past the poles are
 * measured at the pole).  Row r has the rings row_rings[r] .. row_rings[r+1] - 1; ring g has the vertices
 * ring_offsets[g] .. ring_offsets[g+1] - 1 of lon[] / lat[] (degrees; closed or not) and weight ring_weight[g]; row r's
 * candidate cells are the row_cells[3r+2] (= ny_r) -major block starting at cell (row_cells[3r], row_cells[3r+1]):
 * pair pair_offsets[r] + k is cell (row_cells[3r] + k / ny_r, row_cells[3r+1] + k % ny_r), and pair_offsets[n_rows] == n_pairs.
 * area[p] (one float64 per pair, provided by the caller) = sum over the row's rings of ring_weight[g] times the ring's
 * signed clipped area (positive counter-clockwise): +-1 by orientation and role turns exteriors positive and holes negative.
 * Deterministic: no atomics, the same input gives the same bits.  rr_grid_overlap_area takes host arrays and checks every
 * index; the _dev form takes device arrays, checks sizes only and only enqueues on `stream`. */
int rr_grid_overlap_area(int device, int64_t n_rows, int64_t n_rings, int64_t n_vertices, int64_t nx, int64_t ny, int64_t n_pairs,
                         const int64_t *row_rings, const int64_t *ring_offsets, const double *ring_weight, const double *lon,
                         const double *lat, const double *x_bounds, const double *y_bounds, const int32_t *row_cells,
                         const int64_t *pair_offsets, double *area);
int rr_grid_overlap_area_dev(int device, int64_t n_rows, int64_t n_rings, int64_t n_vertices, int64_t nx, int64_t ny, int64_t n_pairs,
                             const int64_t *row_rings, const int64_t *ring_offsets, const double *ring_weight, const double *lon,
                             const double *lat, const double *x_bounds, const double *y_bounds, const int32_t *row_cells,
                             const int64_t *pair_offsets, double *area, void *stream);

/* ---- adjoint of RapidMuskingum routing ----
 * The gradient of a scalar loss L through one rr_rapid_route_dev call (T rows, nsub sub-steps, S = T * nsub) with the coefficients
 * as last set by rr_plan_set_coeffs.  All rows are (time, reach) in params order on the plan's device:
 *   q0[n]              the state the forward call started from;
 *   lateral[lat_rows*n] its lateral rows (the first T are read; lat_rows >= T), or NULL for channel-only routing;
 *   discharge[T*n]     its discharge (the clamp mask: a value <= 0 passes no gradient); needed with grad_out;
 *   grad_out[T*n]      dL/d(discharge), or NULL;  grad_qfinal[n]  dL/d(final state), or NULL;
 * and it writes what is asked for (NULL: not computed):
 *   grad_lateral[T*n]  dL/d(lateral);  grad_q0[n]  dL/d(q0);
 *   grad_coef[4*n]     dL/dc1, dL/dc2, dL/dc3, dL/dc4dt per reach, c1 being the reach's own (the -lhs_off_data of the edges into it).
 * Work memory (caller-provided, rr_rapid_adjoint_work_bytes; the call allocates nothing and only enqueues on `stream`):
 *   8 n (2 S + 2 T + 2 depth + min(T, 16) + 4 splits + 2) bytes, splits = min(S, ceil(2048 / ceil(n / 256))) sub-step ranges of
 *   the reduction: the forward state tape and the adjoint tape (S + depth rows each), lateral and gradient rows in engine order.
 * rr_rapid_adjoint_work_bytes also readies the plan for adjoint calls (uploads its permutation tables once): call it before the first.
 * No atomics: the same inputs give the same bits.  RR_E_UNSUPPORTED for per-edge weights, a plan with boundary reaches
 * (rr_plan_set_boundary) and a host-only plan; RR_E_INVALID for a null or short argument or too little work memory. */
int rr_rapid_adjoint_work_bytes(rr_plan *plan, int64_t T, int64_t nsub, int64_t *bytes);
int rr_rapid_adjoint_dev(rr_plan *plan, const double *q0, const double *lateral, int64_t lat_rows, const double *discharge,
                         const double *grad_out, const double *grad_qfinal, double *grad_lateral, double *grad_q0, double *grad_coef,
                         void *work, int64_t work_bytes, int64_t T, int64_t nsub, void *stream);

/* ---- the same for several forcing series at once ----
 * `members` rr_rapid_route_dev calls on one plan with one coefficient set (a mini-batch of windows, the members of a forcing
 * ensemble), their gradients from one pair of sweeps: every reverse and replay tick is one launch over (positions, members), so the
 * tick launches number 2 (S + depth - 1) whatever the member count.  Member m's arrays lie m pitches (in doubles) behind member 0's:
 *   q0                 at q0_pitch (0: one q0[n] shared by every member; otherwise >= n);
 *   lateral, grad_lateral    at lat_pitch (>= T*n; lat_rows >= T rows per member);
 *   discharge, grad_out      at out_pitch (>= T*n);
 *   grad_qfinal, grad_q0     [members*n], dense;
 *   grad_coef[4*n]     the SUM over the members, folded in ascending member order (within a member its sub-step ranges in order).
 * NULL arguments mean what they mean in rr_rapid_adjoint_dev, for every member alike.  Each member's grad_lateral and grad_q0 are
 * the bits rr_rapid_adjoint_dev gives for that member alone; with members == 1 so is grad_coef.
 * Work memory (rr_rapid_adjoint_batch_work_bytes; caller-provided, the call allocates nothing and only enqueues on `stream`):
 *   8 n (members (2 S + 2 T + 2 depth + 4 splits + 2) + min(T, 16)) bytes, splits = min(S, ceil(2048 / (members ceil(n / 256)))):
 *   the single call's tapes, rows, partial sums and scratch rows once per member, the permutation's rows once.
 * rr_rapid_adjoint_batch_work_bytes readies the plan as rr_rapid_adjoint_work_bytes does.  No atomics.  Refused: what
 * rr_rapid_adjoint_dev refuses, then RR_E_INVALID for members < 1 or > 65535, for a pitch shorter than one member's rows, and for
 * too little work memory. */
int rr_rapid_adjoint_batch_work_bytes(rr_plan *plan, int64_t members, int64_t T, int64_t nsub, int64_t *bytes);
int rr_rapid_adjoint_batch_dev(rr_plan *plan, int64_t members, const double *q0, int64_t q0_pitch, const double *lateral, int64_t lat_rows,
                               int64_t lat_pitch, const double *discharge, const double *grad_out, int64_t out_pitch,
                               const double *grad_qfinal, double *grad_lateral, double *grad_q0, double *grad_coef, void *work,
                               int64_t work_bytes, int64_t T, int64_t nsub, void *stream);

/* ---- the same with dL/d(discharge) at gauged reaches only ----
 * rr_rapid_adjoint_batch_dev for a loss that reads the discharge at n_gauges reaches: no (T, n) cotangent is read, written or permuted.
 *   gauges[n_gauges]          device int32 reach indices in params order, distinct, in any order;
 *   discharge_g[T*n_gauges]   the forward call's discharge at those reaches, column j being reach gauges[j] (the clamp mask: a value
 *                             <= 0 passes no gradient, as in the dense call);
 *   grad_out_g[T*n_gauges]    dL/d(that discharge); both or neither (NULL: the loss reads the final state only);
 * member m's discharge_g and grad_out_g lie m * gauge_pitch doubles further on (gauge_pitch >= T*n_gauges; anything when members == 1).
 * Every other argument means what it means in rr_rapid_adjoint_batch_dev, NULLs included.  One call form: with members == 1 the
 * single-member kernels run and every output has the bits rr_rapid_adjoint_dev gives for the cotangent scattered to full width.
 * On the device a slot map (engine order, -1 or the gauge column) is built from gauges[] per call, the clamp mask and the 1 / nsub
 * mean are applied over the (T, n_gauges) blocks, and a reverse tick reads, per position, its slot and, at a gauge, one value of the
 * block.  gauges[] is not range-checked on the device: the caller vouches for distinct indices in [0, n).
 * Work memory (rr_rapid_adjoint_gauges_work_bytes; caller-provided, the call allocates nothing and only enqueues on `stream`):
 *   8 (n members (2 S + (with_grad_lateral ? 2 : 1) T + 2 depth + 4 splits + 2) + max(n min(T, 16), members T n_gauges)) bytes,
 *   splits as in rr_rapid_adjoint_batch_work_bytes: the batch call's memory without the engine-order gradient rows unless
 *   grad_lateral is asked for; the masked blocks share the permutation's rows, the slot map two scratch rows.
 * with_grad_lateral says which layout is meant: a non-NULL grad_lateral on work memory sized without it is refused (RR_E_INVALID, too
 * little work memory).  rr_rapid_adjoint_gauges_work_bytes readies the plan as rr_rapid_adjoint_work_bytes does.  No atomics.
 * Refused: what rr_rapid_adjoint_batch_dev refuses, then RR_E_INVALID for n_gauges < 1 or > n, a NULL gauges, discharge_g without
 * grad_out_g or the reverse, and a gauge_pitch shorter than T*n_gauges when members > 1. */
int rr_rapid_adjoint_gauges_work_bytes(rr_plan *plan, int64_t members, int64_t n_gauges, int64_t T, int64_t nsub, int with_grad_lateral,
                                       int64_t *bytes);
int rr_rapid_adjoint_gauges_dev(rr_plan *plan, int64_t members, int64_t n_gauges, const int32_t *gauges, const double *q0, int64_t q0_pitch,
                                const double *lateral, int64_t lat_rows, int64_t lat_pitch, const double *discharge_g,
                                const double *grad_out_g, int64_t gauge_pitch, const double *grad_qfinal, double *grad_lateral,
                                double *grad_q0, double *grad_coef, void *work, int64_t work_bytes, int64_t T, int64_t nsub, void *stream);

/* ---- adjoint of UnitMuskingum routing ----
 * The gradient of a scalar loss L through one rr_unit_route_dev call (unit_route, river_route/routers/_numba_kernels.py:88-171, with
 * the edge data of the reference's callers: a_inner_data = a_hw_data = 1, lhs_off_data = -c1 of the row) of T rows, nsub sub-steps,
 * S = T * nsub, with the coefficients as last set by rr_plan_set_coeffs.  Rows are (time, reach) in params order, states are indexed
 * by inner reach (ascending params order) as rr_unit_route_dev takes them, all on the plan's device:
 *   q_ch0, q_full0[n_inner]  the states the forward call started from (needed with grad_coef);
 *   lateral[lat_rows*n]      its convolved lateral rows (the first T are read; needed with grad_coef);
 *   discharge[T*n]           its discharge (the clamp mask of the inner reaches); needed with grad_out;
 *   grad_out[T*n]            dL/d(discharge), or NULL;  grad_qch_final, grad_qfull_final[n_inner]  dL/d(final states), or NULL;
 * and it writes what is asked for (NULL: not computed):
 *   grad_lateral[T*n];  grad_qch0, grad_qfull0[n_inner];
 *   grad_coef[3*n]           dL/dc1, dL/dc2, dL/dc3 per reach in params order, 0 at headwaters (their coefficients are never read).
 * Work memory (caller-provided, rr_unit_adjoint_work_bytes; the call allocates nothing and only enqueues on `stream`):
 *   8 n (2 S + 2 T + 2 depth + min(T, 16) + 3 splits + 6) bytes, splits = min(S, ceil(2048 / ceil(n / 256))): the forward tape of
 *   q_full (a headwater's slot holds its lateral inflow) and the adjoint tape of dL/dq_ch (S + depth rows each), lateral and gradient
 *   rows in engine order, the reduction's partial sums, six scratch rows.
 * rr_unit_adjoint_work_bytes also readies the plan for adjoint calls: call it before the first.  No atomics: the same inputs give the
 * same bits.  RR_E_UNSUPPORTED for general edge data (rr_plan_set_unit_weights), per-edge weights, a plan with boundary reaches and a
 * host-only plan; RR_E_INVALID for a null or short argument or too little work memory. */
int rr_unit_adjoint_work_bytes(rr_plan *plan, int64_t T, int64_t nsub, int64_t *bytes);
int rr_unit_adjoint_dev(rr_plan *plan, const double *q_ch0, const double *q_full0, const double *lateral, int64_t lat_rows,
                        const double *discharge, const double *grad_out, const double *grad_qch_final, const double *grad_qfull_final,
                        double *grad_lateral, double *grad_qch0, double *grad_qfull0, double *grad_coef, void *work, int64_t work_bytes,
                        int64_t T, int64_t nsub, void *stream);

/* ---- the same for several forcing series at once ----
 * `members` rr_unit_route_dev calls (unit_route, river_route/routers/_numba_kernels.py:88-171, call site
 * river_route/routers/UnitMuskingum.py:82-92) on one plan with one coefficient set, their gradients from one pair of sweeps: every
 * replay and reverse tick is one launch over (positions, members), so the tick launches number 2 (S + depth - 1) whatever the member
 * count.  Member m's arrays lie m pitches (in doubles) behind member 0's:
 *   q_ch0, q_full0           at state_pitch (0: one pair of states[n_inner] shared by every member; otherwise >= n_inner);
 *   lateral, grad_lateral    at lat_pitch (>= T*n; lat_rows >= T rows per member);
 *   discharge, grad_out      at out_pitch (>= T*n);
 *   grad_qch_final, grad_qfull_final, grad_qch0, grad_qfull0    [members*n_inner], dense;
 *   grad_coef[3*n]           the SUM over the members, folded in ascending member order (within a member its sub-step ranges in order).
 * NULL arguments mean what they mean in rr_unit_adjoint_dev, for every member alike.  Each member's grad_lateral, grad_qch0 and
 * grad_qfull0 are the bits rr_unit_adjoint_dev gives for that member alone; with members == 1 so is grad_coef.
 * Work memory (rr_unit_adjoint_batch_work_bytes; caller-provided, the call allocates nothing and only enqueues on `stream`):
 *   8 n (members (2 S + 2 T + 2 depth + 3 splits + 6) + min(T, 16)) bytes, splits = min(S, ceil(2048 / (members ceil(n / 256)))):
 *   the single call's tapes, rows, partial sums and six scratch rows once per member, the permutation's rows once.
 * rr_unit_adjoint_batch_work_bytes readies the plan as rr_unit_adjoint_work_bytes does.  No atomics.  Refused: what
 * rr_unit_adjoint_dev refuses, then RR_E_INVALID for members < 1 or > 65535, for a pitch shorter than one member's rows or states,
 * and for too little work memory. */
int rr_unit_adjoint_batch_work_bytes(rr_plan *plan, int64_t members, int64_t T, int64_t nsub, int64_t *bytes);
int rr_unit_adjoint_batch_dev(rr_plan *plan, int64_t members, const double *q_ch0, const double *q_full0, int64_t state_pitch,
                              const double *lateral, int64_t lat_rows, int64_t lat_pitch, const double *discharge, const double *grad_out,
                              int64_t out_pitch, const double *grad_qch_final, const double *grad_qfull_final, double *grad_lateral,
                              double *grad_qch0, double *grad_qfull0, double *grad_coef, void *work, int64_t work_bytes, int64_t T,
                              int64_t nsub, void *stream);

/* ---- the same with dL/d(discharge) at gauged reaches only ----
 * rr_unit_adjoint_batch_dev (unit_route, river_route/routers/_numba_kernels.py:88-171, call site
 * river_route/routers/UnitMuskingum.py:82-92) for a loss that reads the discharge at n_gauges reaches: no (T, n) cotangent is read,
 * written or permuted.
 *   gauges[n_gauges]          device int32 reach indices in params order, distinct, in any order, headwaters and inner reaches alike;
 *   discharge_g[T*n_gauges]   the forward call's discharge at those reaches, column j being reach gauges[j] (the clamp mask of an inner
 *                             reach: a value <= 0 passes no gradient, as in the dense call; a headwater's column is not read);
 *   grad_out_g[T*n_gauges]    dL/d(that discharge); both or neither (NULL: the loss reads the final states only);
 * member m's discharge_g and grad_out_g lie m * gauge_pitch doubles further on (gauge_pitch >= T*n_gauges; anything when members == 1).
 * Every other argument means what it means in rr_unit_adjoint_batch_dev, NULLs included.  One call form: with members == 1 the
 * single-member kernels run and every output has the bits rr_unit_adjoint_dev gives for the cotangent scattered to full width.
 * On the device a slot map (engine order, -1 or the gauge column) is built from gauges[] per call and the forward's output rule is
 * applied over the (T, n_gauges) blocks: an inner reach's column takes the clamp mask and the 1 / nsub mean, a headwater's passes as it
 * is.  A reverse tick reads, per position, its slot and, at a gauge, one value of the block; so does the row pass that writes
 * grad_lateral, where a headwater's cotangent arrives undivided.  gauges[] is not range-checked on the device: the caller vouches for
 * distinct indices in [0, n).
 * Work memory (rr_unit_adjoint_gauges_work_bytes; caller-provided, the call allocates nothing and only enqueues on `stream`):
 *   8 (n members (2 S + (with_grad_lateral ? 2 : 1) T + 2 depth + 3 splits + 6) + max(n min(T, 16), members T n_gauges)) bytes,
 *   splits as in rr_unit_adjoint_batch_work_bytes: the batch call's memory without the engine-order gradient rows unless
 *   grad_lateral is asked for; the masked blocks share the permutation's rows, the slot map the replay's first scratch row.
 * with_grad_lateral says which layout is meant: a non-NULL grad_lateral on work memory sized without it is refused (RR_E_INVALID, too
 * little work memory).  rr_unit_adjoint_gauges_work_bytes readies the plan as rr_unit_adjoint_work_bytes does.  No atomics.
 * Refused: what rr_unit_adjoint_batch_dev refuses (general edge data: RR_E_UNSUPPORTED), then RR_E_INVALID for n_gauges < 1 or > n, a
 * NULL gauges, discharge_g without grad_out_g or the reverse, and a gauge_pitch shorter than T*n_gauges when members > 1. */
int rr_unit_adjoint_gauges_work_bytes(rr_plan *plan, int64_t members, int64_t n_gauges, int64_t T, int64_t nsub, int with_grad_lateral,
                                      int64_t *bytes);
int rr_unit_adjoint_gauges_dev(rr_plan *plan, int64_t members, int64_t n_gauges, const int32_t *gauges, const double *q_ch0,
                               const double *q_full0, int64_t state_pitch, const double *lateral, int64_t lat_rows, int64_t lat_pitch,
                               const double *discharge_g, const double *grad_out_g, int64_t gauge_pitch, const double *grad_qch_final,
                               const double *grad_qfull_final, double *grad_lateral, double *grad_qch0, double *grad_qfull0,
                               double *grad_coef, void *work, int64_t work_bytes, int64_t T, int64_t nsub, void *stream);

/* ---- adjoint of the unit-hydrograph convolution ----
 * The gradient through one rr_uh_convolve_dev call (UnitHydrograph.convolve, river_route/uhkernels/UnitHydrograph.py:93-107):
 * buf = full convolution of depth[T*n] with kernel[n_ks*n] along time, buf[:n_ks] += state; convolved = buf[:T], the state it leaves
 * is buf[T:] in its first n_ks - 1 rows and 0 in its last.  With G = dL/dbuf (grad_convolved below T, grad_state_out above):
 *   grad_depth[t,i] = sum_j kernel[j,i] G[t+j,i];  grad_kernel[j,i] = sum_t depth[t,i] G[t+j,i];  grad_state[t',i] = G[t',i], t' < n_ks.
 * grad_convolved[T*n] and grad_state_out[n_ks*n] may be NULL (no gradient arrives there); a NULL output is not computed; depth is
 * needed with grad_kernel, kernel with grad_depth.  Work memory (rr_uh_adjoint_work_bytes): 8 n n_ks splits bytes, splits =
 * min(T, ceil(2048 / (ceil(n / 256) ceil(n_ks / 16)))) row ranges of grad_kernel merged in order, or none when splits = 1.
 * Enqueue only, no atomics.  RR_E_INVALID for a null or short argument. */
int rr_uh_adjoint_work_bytes(int64_t T, int64_t n_ks, int64_t n, int64_t *bytes);
int rr_uh_adjoint_dev(int device, const double *kernel, const double *depth, const double *grad_convolved, const double *grad_state_out,
                      double *grad_depth, double *grad_kernel, double *grad_state, void *work, int64_t work_bytes, int64_t T,
                      int64_t n_ks, int64_t n, void *stream);

/* ---- adjoint of the skill scores (river_route/metrics.py) ----
 * The gradient of a scalar loss L through the five scores of one rr_metrics_update_dev + rr_metrics_finish_dev pair over all `rows`
 * rows, with respect to y_pred.  y_true, y_pred, their pitches and types and n are those of the update; `state` is the
 * RR_METRICS_STATE x n state it left; grad_scores[5 * n] is dL/d(out) of rr_metrics_finish_dev (grad_scores[k * n + j]).  With
 * t = y_true[r, j], p = y_pred[r, c], c the column of y_pred that column j is scored against, column j adds to grad_pred[r, c]
 *   A + B (t - mean_true) + P (p - mean_pred) + S sign(t - p),  sign(0) = 0,
 * A, B, P, S following from the state and the five gradients.  A score whose gradient is exactly 0 adds
 * nothing; a score that is NaN by rr_metrics_finish_dev's rules with a gradient other than 0 makes the column's gradient NaN; r
 * passes no gradient where its unclipped value lies outside [-1, 1].  grad_pred has y_pred's element type, row r at
 * grad_pred + r * grad_pitch elements.
 * Without a column map (order, distinct_columns, segments NULL; n_distinct = n) c = j and every element of the n columns is written.
 * With one, the caller passes the map sorted: order[n] is a stable argsort of pred_columns, distinct_columns[n_distinct] its
 * distinct values ascending, segments[n_distinct + 1] the start of each value's run in `order` (segments[n_distinct] = n).
 * Column distinct_columns[u] of grad_pred receives the sum of the shares of the y_true columns order[segments[u]] ..
 * order[segments[u + 1] - 1], added in that order; other columns of grad_pred are not touched (the caller zero-fills them).
 * The maps are not range-checked on the device.  Work memory: rr_metrics_adjoint_work_bytes = 48 n bytes (six doubles per column).
 * Enqueue only, allocates nothing, no atomics: the same inputs give the same bits.  RR_E_INVALID for a null or short argument. */
int rr_metrics_adjoint_work_bytes(int64_t n, int64_t *bytes);
int rr_metrics_adjoint_dev(int device, int64_t n, int64_t rows, const void *y_true, int true_is_f32, int64_t true_pitch,
                           const void *y_pred, int pred_is_f32, int64_t pred_pitch, const double *state, const double *grad_scores,
                           int64_t n_distinct, const int32_t *order, const int32_t *distinct_columns, const int32_t *segments,
                           void *grad_pred, int64_t grad_pitch, void *work, int64_t work_bytes, void *stream);

/* ---- skill scores and their adjoint over records with gaps (DESIGN.md sections 9 and 12c, "Missing observations") ----
 * rr_metrics_update_missing_dev is rr_metrics_update_dev, and rr_metrics_adjoint_missing_dev is rr_metrics_adjoint_dev, with one
 * rule added: element (r, j) is MISSING when y_true[r, j], as stored (float or double), is NaN.  The pair (y_true[r, j],
 * y_pred[r, pred_columns[j]]) is then left out of every sum of column j, and y_pred there is never looked at (a NaN there changes
 * nothing).  Inf is not missing.  A NaN of y_pred at a KEPT row poisons the column as in rr_metrics_update_dev.  Each column is
 * scored over its own kept pairs: state[0 * n + j] (the count) is N_j, the number kept, and rr_metrics_finish_dev and the adjoint's
 * constants divide by it.  N_j = 0: all five scores NaN; N_j = 1: mean error, mean absolute error and mean square error finite,
 * Pearson r and KGE NaN; the constant-column and zero-mean rules are those of rr_metrics_finish_dev.
 * The argument lists, the refusals and the work memory (rr_metrics_work_bytes, rr_metrics_adjoint_work_bytes) are those of the two
 * calls without the rule; the state is finished by rr_metrics_finish_dev.  Updates with and without the rule may be mixed on one
 * state: the state then holds every pair of the plain updates (a NaN among them poisons the column) and the kept pairs of the
 * others, and its count is their sum.
 * Adjoint: `state` is the one rr_metrics_update_missing_dev left over the same rows.  At a kept element column j adds the share of
 * rr_metrics_adjoint_dev, with N_j and the kept pairs' moments in its constants; at a missing element its share is exactly 0.0,
 * never NaN, whatever the constants are.  With a column map every share is masked by its own y_true column, so a column of y_pred
 * scored twice gets the kept share alone where the other is missing.  Every element rr_metrics_adjoint_dev would write is
 * written.  "A NaN score with a gradient other than 0 makes the column's gradient NaN" holds at the kept rows; a column with
 * N_j = 0 adds zeros.  No atomics: the same inputs give the same bits. */
int rr_metrics_update_missing_dev(int device, int64_t n, int64_t rows, const void *y_true, int true_is_f32, int64_t true_pitch,
                                  const void *y_pred, int pred_is_f32, int64_t pred_pitch, const int32_t *pred_columns, double *state,
                                  void *work, int64_t work_bytes, void *stream);
int rr_metrics_adjoint_missing_dev(int device, int64_t n, int64_t rows, const void *y_true, int true_is_f32, int64_t true_pitch,
                                   const void *y_pred, int pred_is_f32, int64_t pred_pitch, const double *state, const double *grad_scores,
                                   int64_t n_distinct, const int32_t *order, const int32_t *distinct_columns, const int32_t *segments,
                                   void *grad_pred, int64_t grad_pitch, void *work, int64_t work_bytes, void *stream);

/* ---- skill scores of the members of an ensemble in one launch ----
 * rr_metrics_update_members_dev is rr_metrics_update_dev (skip_missing != 0: rr_metrics_update_missing_dev) for `members` blocks of
 * rows at once: member m's element (r, c) of y_pred is at y_pred[m * pred_member_pitch + r * pred_pitch + c], its observation at
 * y_true[m * true_member_pitch + r * true_pitch + c]; true_member_pitch == 0: one observation block that all members share.  All
 * pitches are in elements and every member offset is formed in 64 bits, so the members may lie more than 2^31 elements apart.
 * pred_columns[n] (may be NULL) is one map for all members.
 * `state` is RR_METRICS_STATE x (members * n) doubles, field-major over the flattened index m * n + j (state[k * members * n +
 * m * n + j]), zero-filled by the caller before the first update.  It is finished by rr_metrics_finish_dev(device, members * n, state,
 * out, stream), whose out[5 * members * n] then reads as (5, members, n); row 0 of the state is the pairs kept, (members, n).
 * The rows are cut by rr_metrics_update_dev's rule with members * ceil(n / 256) workgroups per row range in place of ceil(n / 256):
 * a function of (n, members, rows) only (same inputs and the same sequence of updates: bit-identical results), and with members == 1
 * the cut, and so every bit of the state, is that of rr_metrics_update_dev / rr_metrics_update_missing_dev (the member pitches are
 * then not looked at).  Wherever members * ceil(n / 256) * ceil(rows / 32) <= 2048, both calls cut the rows into the same 32-row
 * ranges and member m's columns of the state carry the bits of a single call on member m's rows.  Work memory:
 * rr_metrics_members_work_bytes = splits x RR_METRICS_STATE x members * n doubles (0 when n or rows is 0), folded in split order.
 * Enqueue only, allocates nothing, no atomics; pred_columns is not range-checked on the device.
 * RR_E_INVALID: what rr_metrics_update_dev refuses; members < 1; members * n > 2^31 - 1; with members > 1, pred_member_pitch <
 * (rows - 1) * pred_pitch + the columns read (n, or 1 with pred_columns), or a true_member_pitch other than 0 below
 * (rows - 1) * true_pitch + n.  A refused call leaves `state` as it was. */
int rr_metrics_members_work_bytes(int64_t n, int64_t members, int64_t rows, int64_t *bytes);
int rr_metrics_update_members_dev(int device, int64_t n, int64_t members, int64_t rows, const void *y_true, int true_is_f32,
                                  int64_t true_pitch, int64_t true_member_pitch, const void *y_pred, int pred_is_f32, int64_t pred_pitch,
                                  int64_t pred_member_pitch, const int32_t *pred_columns, int skip_missing, double *state, void *work,
                                  int64_t work_bytes, void *stream);

/* ---- adjoint of gridded runoff -> catchment inflow (rr.grad.runoff_to_qlateral) ----
 * The gradient of a scalar loss L through one rr_runoff_to_qlateral_dev call with respect to the runoff block and to the weights.
 * n_rivers, n_points, T, the CSR arrays, runoff with its type and strides, area and flags are those of the forward call;
 * grad_qlateral[T * n_rivers] is dL/dqlateral.  With S[t, r] = sum_k weights[k] runoff(t, indices[k]) over the CSR row of river r and
 * V = S[t] - S[t - 1] (RR_RUNOFF_CUMULATIVE, t > 0) or S[t], both rounded as the forward rounds them:
 *   M[t, r]  = V is not NaN and (no RR_RUNOFF_FORCE_POSITIVE or V >= 0)      -- V == 0 passes its gradient, as torch.clamp does
 *   Gb[t, r] = M ? grad_qlateral[t, r] * area[r] : 0                          -- area NULL: 1
 *   Gs[t, r] = Gb[t, r] - Gb[t + 1, r] (cumulative; row T - 1 has no t + 1 term), else Gb[t, r]
 *   grad_runoff[t, p] = sum over the pairs k with indices[k] = p, k ascending, of weights[k] * Gs[t, r_k]
 *   grad_weights[k]   = sum over t ascending of Gs[t, r_k] * runoff(t, indices[k])
 * in float64, each product and each sum rounded separately; terms with Gs == 0 are skipped, so a NaN in the runoff (whose Gs is 0)
 * poisons nothing and both gradients are finite whenever grad_qlateral is.  area gets no gradient.
 * t_indptr[n_points + 1], t_pairs[nnz]: the transposed (CSC) structure -- t_pairs[t_indptr[p] .. t_indptr[p + 1]) are the pair indices k
 * with indices[k] = p, ascending (a stable sort of the pairs by point).  Neither structure is range-checked on the device.
 * grad_runoff (may be NULL) has the runoff's element type, element (t, p) at grad_runoff[t * grad_stride_t + p], grad_stride_t >=
 * n_points; every element of its T x n_points is written (a point no river uses gets 0), the float64 sum rounded once on the store.
 * grad_weights (may be NULL) has nnz values.  An output that is NULL costs no pass; both NULL is RR_E_INVALID.
 * Work memory: rr_runoff_adjoint_work_bytes = 8 * n_rivers * T_pad bytes, T_pad = T rounded up to a multiple of 16 (Gs, river-major),
 * 16-byte aligned.  Enqueue only, allocates nothing, no atomics: the same inputs give the same bits.
 * RR_E_INVALID: a null structure array, a negative size or stride, RR_RUNOFF_KEEP_NAN, both outputs NULL (all refused before a
 * device is looked for); RR_E_STATE, with the byte count in rr_last_error(): work_bytes too small; RR_E_UNSUPPORTED: more than
 * 1,048,560 rows in one call. */
int rr_runoff_adjoint_work_bytes(int64_t n_rivers, int64_t n_points, int64_t T, int64_t *bytes);
int rr_runoff_adjoint_dev(int device, int64_t n_rivers, int64_t n_points, int64_t T, const int32_t *indptr, const int32_t *indices,
                          const double *weights, const int32_t *t_indptr, const int32_t *t_pairs, const void *runoff, int runoff_is_f32,
                          int64_t stride_t, int64_t stride_p, const double *area, int flags, const double *grad_qlateral,
                          void *grad_runoff, int64_t grad_stride_t, double *grad_weights, void *work, int64_t work_bytes, void *stream);

/* ---- small device helpers so a host language needs no HIP binding of its own ---- */
int rr_dev_malloc(int device, int64_t bytes, void **out);
int rr_dev_free(int device, void *ptr);
/* The engine's device allocations, process-wide: out[0] = alive now, out[1] = made since the process started (a plan's arrays, the
 * work memory of the host-pointer entry points and what rr_dev_malloc handed out alike).  For tests: a plan that is destroyed, and a
 * call that fails half-way, leave out[0] where it was (RR_ALLOC_FAIL_AT, read by rr_plan_create, makes the k-th allocation fail). */
int rr_dev_alloc_stats(int64_t out[2]);
int rr_dev_upload(int device, void *dst_dev, const void *src_host, int64_t bytes);
int rr_dev_download(int device, void *dst_host, const void *src_dev, int64_t bytes);
int rr_dev_synchronize(int device);
/* Measured device copy rate (GB/s, bytes read + bytes written) of a 16-byte-per-lane copy kernel over `bytes` bytes,
 * `reps` launches: the achievable HBM rate bench.py reports beside the nominal 8 TB/s. */
int rr_copy_bandwidth(int device, int64_t bytes, int reps, double *gbps);

/* Rows between a file and a device array, for the routers' qlateral / discharge files (river_route/routers/TransformMuskingum.py:30-36,
 * Muskingum.py:319-352): n_rows rows of row_bytes bytes that lie in `path` at file_offset, file_pitch bytes apart (a NetCDF-3 fixed variable:
 * file_pitch = row_bytes; a record variable: the record size), go to / come from device rows dev_pitch bytes apart through pinned staging
 * chunks (reader / writer threads beside the copy engine): the (time, river) block never exists as a host array.  Bytes move as they are:
 * a big-endian float32 variable is converted on the device (rr_plan_set_row_format).  stream (may be NULL): work already enqueued there
 * is finished before the rows move; the functions return when they have. */
int rr_rows_upload(int device, void *dst_dev, int64_t dst_pitch, const char *path, int64_t file_offset, int64_t file_pitch, int64_t row_bytes,
                   int64_t n_rows, void *stream);
int rr_rows_download(int device, const void *src_dev, int64_t src_pitch, const char *path, int64_t file_offset, int64_t file_pitch,
                     int64_t row_bytes, int64_t n_rows, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RR_HIP_H */
