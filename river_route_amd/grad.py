"""
Differentiable routing: torch autograd through the HIP engine.

    import river_route_amd as rr
    k = torch.tensor(k0, dtype=torch.float64, requires_grad=True)
    Q, q_final = rr.grad.rapid_route(plan, q0, qlateral, k, x, dt_routing=900.0, dt_runoff=3600.0)
    loss = ((Q[:, gauges] - observed) ** 2).mean()
    loss.backward()                     # k.grad: dL/dk of every reach, from one reverse sweep on the GPU

The forward is the production route call (rr_rapid_route_dev on torch's current stream), so the discharge is the one
Plan.rapid_route computes, bit for bit.  The backward is rr_rapid_adjoint_dev: it routes the forward again into a state tape and
runs the adjoint recurrence from the outlets upward and backward in time, then reduces the coefficient gradients per reach.
Torch chains from the coefficients to k and x (muskingum_coefficients), so any loss written in torch can sit on top.

UnitMuskingum has the same three layers: uh_convolve (UnitHydrograph.convolve; gradients to the kernel columns, the carried state
and the runoff depths), unit_route (unit_route on a convolved lateral; gradients to q_ch0, q_full0, the lateral rows, k and x) and
unit_muskingum, the two chained as the router chains them, in windows if asked:

    Q, q_ch, q_full, uh_state = rr.grad.unit_muskingum(plan, q_ch0, q_full0, depth, uh_kernel, uh_state0, k, x, 900.0, 3600.0)

Several forcing series on one network and one coefficient set (a mini-batch of windows, the members of a forcing ensemble) go
through rapid_route_batch: the forward is rapid_route's, member by member, and the backward is one
rr_rapid_adjoint_batch_dev call whose two sweeps launch once per tick for all members together; k and x get the sum over the members:

    Q, q_final = rr.grad.rapid_route_batch(plan, q0, qlateral, k, x, 900.0, 3600.0)      # qlateral[B, T, n] -> Q[B, T, n], q_final[B, n]

UnitMuskingum has the same: unit_route_batch (backward: rr_unit_adjoint_batch_dev), uh_convolve_batch (member
by member: the convolution's adjoint is a few launches per member, not one per tick) and unit_muskingum_batch, the two chained:

    Q, q_ch, q_full, uh_state = rr.grad.unit_muskingum_batch(plan, q_ch0, q_full0, depth, uh_kernel, uh_state0, k, x, 900.0, 3600.0)

A calibration reads the discharge at a few thousand gauged reaches of a large network.  rapid_route and rapid_route_batch take those
reaches as gauges=: they then return and keep the (T, G) gauge columns only, and the backward pass is
rr_rapid_adjoint_gauges_dev, which takes the (T, G) cotangent as it is -- no (T, n) cotangent is allocated, zero-filled or permuted:

    Qg, q_final = rr.grad.rapid_route(plan, q0, qlateral, k, x, 900.0, 3600.0, gauges=gauges)      # Qg[T, G], column j is reach gauges[j]
    (1 - rr.grad.scores(observed, Qg)['kge2012']).mean().backward()

unit_route, unit_route_batch, unit_muskingum and unit_muskingum_batch take gauges= in the same way (backward:
rr_unit_adjoint_gauges_dev, where a gauged headwater passes its cotangent to the lateral rows as it is).

Float64 rows, one plan on one GPU, the edge data of the reference's callers: float32 rows, partitioned plans and plans with
set_unit_weights edge data are refused, and so are 3-D rows everywhere but in the *_batch functions.

The loss a calibration minimises is a skill score at gauges, and `scores` is rr.metrics.scores with an autograd graph (DESIGN.md
section 12c): the same five values, bit for bit, and a backward pass that writes dL/dQ in one streaming pass on the GPU:

    kge = rr.grad.scores(observed, Q, columns=gauges)['kge2012']      # observed[T, n_gauges] against Q[:, gauges], no gather copy
    (1 - kge).mean().backward()

Gauge records have gaps; with skip_missing=True a NaN in `observed` is a missing observation, every gauge is scored over its own
kept pairs, a skipped element gets the gradient 0, and 'count' (no graph) says how many pairs each gauge kept:

    s = rr.grad.scores(observed, Q, columns=gauges, skip_missing=True)
    (1 - s['kge2012'][s['count'] >= 2]).mean().backward()

The router's chain starts one step before the catchment inflow when it is fed gridded runoff, and runoff_to_qlateral is that step with
a gradient: the forward is rr_runoff_to_qlateral_dev, bit for bit what engine.runoff_to_qlateral computes
(weights product, cumulative -> incremental, clip, NaN fill, area), the backward rr_runoff_adjoint_dev, which reaches the runoff field
and the weights of the catchment / grid-cell table; a RunoffMap holds the table's structure on the GPU for a whole training loop:

    rmap = rr.grad.RunoffMap.from_source(src)                          # src: rr.runoff.prepare_runoff(...)
    qlateral = rr.grad.runoff_to_qlateral(rmap, runoff * bias, weights, area, force_positive=True)      # runoff[T, n_points] -> [T, n]
"""
from __future__ import annotations

import numpy as np
import torch

from . import engine, metrics
from .engine import Plan

__all__ = ['muskingum_coefficients', 'RapidRoute', 'rapid_route', 'RapidRouteBatch', 'rapid_route_batch', 'UhConvolve', 'uh_convolve', 'UnitRoute', 'unit_route',
           'unit_muskingum', 'UnitRouteBatch', 'unit_route_batch', 'UhConvolveBatch', 'uh_convolve_batch', 'unit_muskingum_batch', 'Scores', 'scores',
           'RunoffMap', 'RunoffToQlateral', 'runoff_to_qlateral']


def muskingum_coefficients(k, x, dt_routing):
    """(c1, c2, c3) from k, x and the routing step as torch tensors: the operations of the routers' _set_muskingum_coefficients
    (river_route/routers/Muskingum.py:172-193) in the same order, so the values are the same bits and autograd can chain through
    them.  Raises ValueError when the coefficients do not sum to 1, as the reference does."""
    k = torch.as_tensor(k, dtype=torch.float64)
    x = torch.as_tensor(x, dtype=torch.float64)
    ratio = torch.full_like(k, float(dt_routing)) / k      # tensor / tensor: `scalar / tensor` is a reciprocal times the scalar in torch
    twice_x = 2 * x
    denom = ratio + (2 * (1 - x))
    c1 = (ratio - twice_x) / denom
    c2 = (ratio + twice_x) / denom
    c3 = ((2 * (1 - x)) - ratio) / denom
    total = (c1 + c2 + c3).detach()
    if not torch.allclose(total, torch.ones_like(total)):      # np.allclose(c1 + c2 + c3, 1): rtol 1e-5, atol 1e-8, NaN is not close
        raise ValueError('Muskingum coefficients do not sum to 1, check routing parameters and time step')
    return c1, c2, c3


def _host(c) -> np.ndarray:
    return np.ascontiguousarray(c.detach().to('cpu', torch.float64).numpy())


def _set_coeffs(plan: Plan, c1, c2, c3, c4dt, device: int) -> None:
    """Coefficients onto the plan.  rr_plan_set_coeffs copies synchronously: work already enqueued on torch's stream that reads the
    plan's coefficients finishes first."""
    torch.cuda.current_stream(device).synchronize()
    c1h = _host(c1)
    plan.set_coeffs(-c1h[plan._indices], _host(c2), _host(c3), None if c4dt is None else _host(c4dt))


def _route_backward(plan, coeffs, c4dt, device, grads, shapes, want_coef, need_coef, work_bytes, adjoint):
    """What the backward passes of RapidRoute and UnitRoute share.  The saved coefficients go back onto the plan (c4dt: what the forward
    set); `grads` become contiguous float64 (None stays None); one output per entry of `shapes` (None: not wanted) and, if want_coef,
    one row of coefficient gradients per entry of `coeffs` are allocated, and `work_bytes()` bytes of work memory (torch's allocator
    owns the tapes); adjoint(*grads, *outputs, g_coef, work, nbytes, stream) makes the engine's call on torch's stream.  Returns the
    outputs, then the coefficient rows need_coef asks for (None for the others)."""
    _set_coeffs(plan, *coeffs[:3], c4dt, plan.device)
    stream = torch.cuda.current_stream(plan.device).cuda_stream
    f64 = dict(dtype=torch.float64, device=device)
    grads = [None if g is None else g.to(**f64).contiguous() for g in grads]
    outs = [None if shape is None else torch.empty(shape, **f64) for shape in shapes]
    g_coef = torch.empty((len(coeffs), plan.n), **f64) if want_coef else None
    nbytes = work_bytes()
    work = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=device)
    adjoint(*grads, *outs, g_coef, work, nbytes, stream)
    coef = [g_coef[j].to(c.device) if want_coef and want else None for j, (c, want) in enumerate(zip(coeffs, need_coef))]
    return (*outs, *coef)


def _members_backward(plan, coeffs, c4dt, device, B, per_sweep, grads, shapes, want_coef, need_coef, work_bytes, adjoint):
    """_route_backward for the B members of RapidRouteBatch and UnitRouteBatch: `grads` and the outputs (one per entry of `shapes`, a
    member's shape) have a leading member axis.  The members go in groups of min(B, kMaxMembers, per_sweep) (per_sweep None: all) in
    ascending order: `work_bytes(group_size)` sizes the one work buffer for the largest group, adjoint(m0, m1, *grads[m0:m1],
    *outputs[m0:m1], part, work, nbytes, stream) makes the engine's call for members [m0, m1), and the groups' coefficient rows `part`
    are added in that order."""
    _set_coeffs(plan, *coeffs[:3], c4dt, plan.device)
    stream = torch.cuda.current_stream(plan.device).cuda_stream
    f64 = dict(dtype=torch.float64, device=device)
    grads = [None if g is None else g.to(**f64).contiguous() for g in grads]
    outs = [None if shape is None else torch.empty((B, *shape), **f64) for shape in shapes]
    group = min(B, kMaxMembers, B if per_sweep is None else int(per_sweep))
    nbytes = max(work_bytes(g) for g in {group, B % group or group})
    work = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=device)      # torch's allocator owns the tapes
    g_coef = None
    for m0 in range(0, B, group):
        m1 = min(B, m0 + group)
        part = torch.empty((len(coeffs), plan.n), **f64) if want_coef else None
        adjoint(m0, m1, *(None if t is None else t[m0:m1] for t in (*grads, *outs)), part, work, nbytes, stream)
        if want_coef:
            g_coef = part if g_coef is None else g_coef + part
    coef = [g_coef[j].to(c.device) if want_coef and want else None for j, (c, want) in enumerate(zip(coeffs, need_coef))]
    return (*outs, *coef)


class RapidRoute(torch.autograd.Function):
    """(discharge[T, n], q_final[n]) = RapidMuskingum routing of T rows of qlateral (None: channel-only, then `rows` gives T) from
    q0 with nsub sub-steps per row and per-reach coefficients c1, c2, c3, c4dt.  Forward: rr_rapid_route_dev (or
    rr_muskingum_route_dev); backward: rr_rapid_adjoint_dev, which rebuilds the state tape, so only q0 and references to the inputs
    and the discharge are kept between the two."""

    @staticmethod
    def forward(ctx, plan, nsub, rows, q0, qlateral, c1, c2, c3, c4dt):
        dev = plan.device
        T = int(rows)
        _set_coeffs(plan, c1, c2, c3, c4dt if qlateral is not None else None, dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        q = q0.detach().clone()
        discharge = torch.empty((T, plan.n), dtype=torch.float64, device=q0.device)
        if qlateral is not None:
            plan.rapid_route_dev(q, qlateral.detach(), T, discharge, T, T, nsub, stream)
        else:
            plan.muskingum_route_dev(q, discharge, T, T, nsub, stream)
        ctx.plan, ctx.nsub, ctx.rows = plan, int(nsub), T
        ctx.coeffs = (c1.detach(), c2.detach(), c3.detach(), None if c4dt is None else c4dt.detach())
        ctx.save_for_backward(q0, qlateral, discharge)
        ctx.set_materialize_grads(False)
        return discharge, q

    @staticmethod
    def backward(ctx, grad_discharge, grad_qfinal):
        plan, nsub, T = ctx.plan, ctx.nsub, ctx.rows
        q0, qlateral, discharge = ctx.saved_tensors
        need = ctx.needs_input_grad      # plan, nsub, rows, q0, qlateral, c1, c2, c3, c4dt
        want_q0, want_ql = need[3], need[4] and qlateral is not None
        want_coef = any(need[5:8]) or (need[8] and qlateral is not None)
        if (grad_discharge is None and grad_qfinal is None) or not (want_q0 or want_ql or want_coef):
            return (None,) * 9
        ql = None if qlateral is None else qlateral.detach()
        return (None, None, None, *_route_backward(
            plan, ctx.coeffs, ctx.coeffs[3] if qlateral is not None else None, q0.device, (grad_discharge, grad_qfinal),
            (plan.n if want_q0 else None, (T, plan.n) if want_ql else None), want_coef,
            [need[5 + j] and c is not None for j, c in enumerate(ctx.coeffs)], lambda: plan.rapid_adjoint_work_bytes(T, nsub),
            lambda g_out, g_fin, g_q0, g_ql, g_coef, work, nbytes, stream: plan.rapid_adjoint_dev(
                q0.detach(), ql, T, discharge, g_out, g_fin, g_ql, g_q0, g_coef, work, nbytes, T, nsub, stream)))


def _check_tensor(t, name, shape):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f'{name} must be a torch tensor')
    if t.dtype != torch.float64:
        raise TypeError(f'{name} must be float64 (the adjoint has no float32 rows)')
    if tuple(t.shape) != shape:
        raise ValueError(f'{name} has shape {tuple(t.shape)}, expected {shape}')
    if not t.is_contiguous():
        raise ValueError(f'{name} must be contiguous')


def _check_rows(t, name, n):
    if not isinstance(t, torch.Tensor) or t.ndim != 2:
        raise ValueError(f'{name} must be a 2-D (T, n) tensor (ensembles have no adjoint: route members one by one)')
    T = int(t.shape[0])
    if T < 1:
        raise ValueError(f'{name} has no rows')
    _check_tensor(t, name, (T, n))
    return T


def _check_call(plan, state_len, states, k, x, dt_routing, dt_runoff, rows_per_window):
    """The checks the routing functions share before their rows: the plan's type, the time steps, the state vectors (of plan.n or
    plan.n_inner values, as state_len names), k and x, rows_per_window.  Returns nsub."""
    if not isinstance(plan, Plan):
        raise TypeError('plan must be a river_route_amd.engine.Plan (one GPU; partitioned plans have no adjoint)')
    if not (float(dt_routing) > 0 and float(dt_runoff) > 0):
        raise ValueError('dt_routing and dt_runoff must be positive')
    nsub = int(round(float(dt_runoff) / float(dt_routing)))
    if nsub < 1 or nsub * float(dt_routing) != float(dt_runoff):
        raise ValueError(f'dt_runoff ({dt_runoff}) must be a whole number of routing steps ({dt_routing})')
    for t, name in states:
        _check_tensor(t, name, (getattr(plan, state_len),))
    for t, name in ((k, 'k'), (x, 'x')):
        _check_tensor(t, name, (plan.n,))
    if rows_per_window is not None and int(rows_per_window) < 1:
        raise ValueError('rows_per_window must be >= 1')
    return nsub


def _check_device(plan, pairs):
    """The last checks, so that the others are made before a device is needed: the plan has a GPU and every tensor given is on it."""
    if plan.device < 0:
        raise ValueError('plan is host-only (RR_DEVICE_NONE): the adjoint runs on the GPU only')
    for t, name in pairs:
        if t is not None and (t.device.type != 'cuda' or t.device.index != plan.device):
            raise ValueError(f"{name} must be on cuda:{plan.device}, the plan's device (it is on {t.device})")


def _in_windows(T, rows_per_window, state, route, axis=0):
    """Rows [0, T) in windows of rows_per_window rows (None: one window), chained through the state tuple: route(t0, t1, *state) returns the
    window's discharge rows followed by its final state.  Returns (discharge[T, n], *final state); `axis` is the discharge's time axis."""
    R = T if rows_per_window is None else min(T, int(rows_per_window))
    parts = []
    for t0 in range(0, T, R):
        d, *state = route(t0, min(T, t0 + R), *state)
        parts.append(d)
    return (parts[0] if len(parts) == 1 else torch.cat(parts, axis)), *state


def _check_gauges(gauges, n):
    """gauges= of the routing functions: a 1-D integer array or tensor of distinct params-order reach indices in [0, n).
    Returns them as an int64 host array; for a tensor on a GPU only its shape and type are checked, and None is returned: its values
    are read (by _gauge_values) after the device checks."""
    if isinstance(gauges, torch.Tensor):
        if gauges.dim() != 1 or gauges.is_floating_point() or gauges.is_complex() or gauges.dtype == torch.bool:
            raise ValueError('gauges must be a 1-D integer array or tensor of reach indices')
        if int(gauges.shape[0]) < 1:
            raise ValueError('gauges is empty')
        if gauges.device.type != 'cpu':
            return None
        gauges = gauges.detach().numpy()
    return _gauge_values(gauges, n)


def _gauge_values(gauges, n):
    g = np.asarray(gauges)
    if g.ndim != 1 or not np.issubdtype(g.dtype, np.integer):
        raise ValueError('gauges must be a 1-D integer array or tensor of reach indices')
    if g.size < 1:
        raise ValueError('gauges is empty')
    g = g.astype(np.int64)
    if g.min() < 0 or g.max() >= n:
        raise ValueError(f'gauges refers to reach {int(g.min() if g.min() < 0 else g.max())}: the plan has reaches 0 .. {n - 1}')
    if np.unique(g).size != g.size:
        raise ValueError('gauges holds a reach more than once (the indices must be distinct)')
    return g


def _upload_gauges(plan, gauges, host):
    """The gauge indices on the plan's device, once per call: (int32 for the adjoint, int64 for the forward's gather)."""
    if host is None:
        host = _gauge_values(gauges.detach().cpu().numpy(), plan.n)
    g32 = torch.from_numpy(host.astype(np.int32)).to(torch.device('cuda', plan.device))
    return g32, g32.long()


def rapid_route(plan, q0, qlateral, k, x, dt_routing, dt_runoff, rows_per_window=None, rows=None, gauges=None):
    """Differentiable RapidMuskingum routing: (discharge[T, n], q_final[n]) as torch tensors on the plan's device.

    q0[n] and qlateral[T, n] are float64 tensors on the plan's GPU (qlateral in the reference's volume units per runoff step;
    None routes channel-only, and then `rows` gives T); k and x are float64 tensors of n values on any device.  c1, c2, c3 come
    from muskingum_coefficients(k, x, dt_routing) and c4dt = (c1 + c2) / dt_runoff; dt_runoff must be a whole number of routing
    steps.  Gradients reach q0, qlateral, k and x (whichever require grad).  rows_per_window routes the series in windows chained
    through q_final -> q0, so the tape memory of the backward pass is one window's.

    gauges (a 1-D integer array or tensor of G distinct params-order reach indices) makes the first result discharge[T, G], column
    j being reach gauges[j], for a loss that reads gauged reaches only: the values and every gradient are those of the call without
    it and discharge[:, gauges], bit for bit, but only the gauge columns are kept for the backward pass, which takes the (T, G)
    cotangent as it is (rr_rapid_adjoint_gauges_dev), so nothing (T, n) is allocated for it unless qlateral requires grad.  Every
    argument is checked before the GPU is touched."""
    nsub = _check_call(plan, 'n', ((q0, 'q0'),), k, x, dt_routing, dt_runoff, rows_per_window)
    host_gauges = None if gauges is None else _check_gauges(gauges, plan.n)
    if qlateral is None:
        if rows is None or int(rows) < 1:
            raise ValueError('channel-only routing (qlateral=None) needs rows >= 1')
        T = int(rows)
    else:
        T = _check_rows(qlateral, 'qlateral', plan.n)
    _check_device(plan, ((q0, 'q0'), (qlateral, 'qlateral')))
    c1, c2, c3 = muskingum_coefficients(k, x, float(dt_routing))
    c4dt = (c1 + c2) / float(dt_runoff)
    if gauges is not None:      # the one-member case of the batched gauge call
        on_device = _upload_gauges(plan, gauges, host_gauges)
        d, q = _in_windows(T, rows_per_window, (q0.unsqueeze(0),), lambda t0, t1, q: RapidRouteBatch.apply(
            plan, nsub, t1 - t0, None, on_device, q, None if qlateral is None else qlateral[t0:t1].unsqueeze(0), c1, c2, c3, c4dt), axis=1)
        return d[0], q[0]
    return _in_windows(T, rows_per_window, (q0,), lambda t0, t1, q: RapidRoute.apply(
        plan, nsub, t1 - t0, q, None if qlateral is None else qlateral[t0:t1], c1, c2, c3, c4dt))


# ---- RapidMuskingum, several series at once ----

kMaxMembers = 65535      # members of one rr_rapid_adjoint_batch_dev / rr_unit_adjoint_batch_dev call


def _check_members_per_sweep(members_per_sweep):
    if members_per_sweep is not None and int(members_per_sweep) < 1:
        raise ValueError('members_per_sweep must be >= 1')


def _check_member_rows(t, name, n, single):
    """Rows of a batched call: a contiguous float64 (B, T, n) tensor (`single` names the function for one series).  Returns B, T."""
    if not isinstance(t, torch.Tensor) or t.ndim != 3:
        raise ValueError(f'{name} must be a 3-D (B, T, n) tensor (one series: {single})')
    B, T = int(t.shape[0]), int(t.shape[1])
    if T < 1:
        raise ValueError(f'{name} has no rows')
    _check_tensor(t, name, (B, T, n))
    if B < 1:
        raise ValueError('no members')
    return B, T


def _check_member_state(t, name, B, shape):
    """A state of a batched call: (B, *shape), or `shape` alone for one state shared by every member."""
    if not isinstance(t, torch.Tensor) or t.ndim not in (len(shape), len(shape) + 1):
        dims = ', '.join(('n_inner',) if len(shape) == 1 else ('n_ks', 'n'))
        raise ValueError(f'{name} must be a (B, {dims}) tensor, or ({dims}{"," if len(shape) == 1 else ""}) for one state shared by every member')
    _check_tensor(t, name, (B, *shape) if t.ndim == len(shape) + 1 else tuple(shape))


def _per_member(t, B, shape):
    """A shared state as B rows of pitch 0: autograd sums the members' rows into the one state."""
    return t.unsqueeze(0).expand(B, *shape) if t.ndim == len(shape) else t


class RapidRouteBatch(torch.autograd.Function):
    """(discharge[B, T, n], q_final[B, n]) = RapidRoute for B series at once: q0[B, n] (rows of n adjacent values, any pitch: an
    expanded (n,) q0 has pitch 0), qlateral[B, T, n] or None, one set of coefficients.  Forward: RapidRoute's call, member by member,
    so every member's values are RapidRoute's bits.  Backward: rr_rapid_adjoint_batch_dev on groups of `per_sweep` members (None: all) in
    ascending order, the groups' coefficient gradients added in that order.

    With `gauges` (None, or a pair of device tensors, int32 and int64, of G distinct params-order indices) the discharge is
    (B, T, G), at those reaches only: the forward routes every member into one (T, n) scratch tensor that is not kept and gathers the
    gauge columns out of it, so only q0, qlateral and the (B, T, G) gauge discharge are kept; the backward is
    rr_rapid_adjoint_gauges_dev, whose work memory has gradient rows only when qlateral requires grad."""

    @staticmethod
    def forward(ctx, plan, nsub, rows, per_sweep, gauges, q0, qlateral, c1, c2, c3, c4dt):
        dev = plan.device
        g32, g64 = (None, None) if gauges is None else gauges
        B, T = int(q0.shape[0]), int(rows)
        _set_coeffs(plan, c1, c2, c3, c4dt if qlateral is not None else None, dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        q = q0.detach().clone(memory_format=torch.contiguous_format)
        scratch = None if gauges is None else torch.empty((T, plan.n), dtype=torch.float64, device=q0.device)
        discharge = torch.empty((B, T, plan.n if gauges is None else int(g32.shape[0])), dtype=torch.float64, device=q0.device)
        ql = None if qlateral is None else qlateral.detach()
        for m in range(B):
            routed = discharge[m] if gauges is None else scratch
            if ql is not None:
                plan.rapid_route_dev(q[m], ql[m], T, routed, T, T, nsub, stream)
            else:
                plan.muskingum_route_dev(q[m], routed, T, T, nsub, stream)
            if gauges is not None:
                torch.index_select(scratch, 1, g64, out=discharge[m])
        ctx.plan, ctx.nsub, ctx.rows, ctx.per_sweep, ctx.g32 = plan, int(nsub), T, per_sweep, g32
        ctx.coeffs = (c1.detach(), c2.detach(), c3.detach(), None if c4dt is None else c4dt.detach())
        ctx.save_for_backward(q0, qlateral, discharge)
        ctx.set_materialize_grads(False)
        return discharge, q

    @staticmethod
    def backward(ctx, grad_discharge, grad_qfinal):
        plan, nsub, T, g32 = ctx.plan, ctx.nsub, ctx.rows, ctx.g32
        q0, qlateral, discharge = ctx.saved_tensors
        need = ctx.needs_input_grad      # plan, nsub, rows, per_sweep, gauges, q0, qlateral, c1, c2, c3, c4dt
        want_q0, want_ql = need[5], need[6] and qlateral is not None
        want_coef = any(need[7:10]) or (need[10] and qlateral is not None)
        if (grad_discharge is None and grad_qfinal is None) or not (want_q0 or want_ql or want_coef):
            return (None,) * 11
        B, n, G = int(q0.shape[0]), plan.n, int(discharge.shape[2])
        ql = None if qlateral is None else qlateral.detach()
        q0_pitch = int(q0.stride(0)) if B > 1 else n

        def work_bytes(members):
            if g32 is None:
                return plan.rapid_adjoint_batch_work_bytes(members, T, nsub)
            return plan.rapid_adjoint_gauges_work_bytes(members, G, T, nsub, want_ql)

        def adjoint(m0, m1, g_out, g_fin, g_q0, g_ql, g_coef, work, nbytes, stream):
            inputs = (q0.data_ptr() + 8 * m0 * q0_pitch, q0_pitch, None if ql is None else ql[m0:m1], T, T * n)
            rest = (g_fin, g_ql, g_q0, g_coef, work, nbytes, T, nsub, stream)
            if g32 is None:
                plan.rapid_adjoint_batch_dev(m1 - m0, *inputs, discharge[m0:m1], g_out, T * n, *rest)
            else:      # the gauge discharge goes with its cotangent only: the engine refuses one without the other
                plan.rapid_adjoint_gauges_dev(m1 - m0, G, g32, *inputs, None if g_out is None else discharge[m0:m1], g_out, T * G, *rest)

        return (None, None, None, None, None, *_members_backward(
            plan, ctx.coeffs, ctx.coeffs[3] if qlateral is not None else None, discharge.device, B, ctx.per_sweep,
            (grad_discharge, grad_qfinal), ((n,) if want_q0 else None, (T, n) if want_ql else None), want_coef,
            [need[7 + j] and c is not None for j, c in enumerate(ctx.coeffs)], work_bytes, adjoint))


def rapid_route_batch(plan, q0, qlateral, k, x, dt_routing, dt_runoff, rows_per_window=None, rows=None, members_per_sweep=None, gauges=None):
    """rapid_route for B forcing series on one network and one set of coefficients: (discharge[B, T, n], q_final[B, n]).

    qlateral[B, T, n] is a contiguous float64 tensor on the plan's GPU (None routes channel-only: then `rows` gives T and q0 gives B);
    q0 is (B, n), or (n,) for one initial state shared by every member, whose gradient is then the sum over the members; k and x are
    as in rapid_route and serve all members.  Every member's discharge and q_final are the bits rapid_route gives for that member
    alone (the forward is the same call, member by member), and so are its dL/dqlateral and dL/dq0; k and x get the sum over the
    members.  The backward pass is one rr_rapid_adjoint_batch_dev call: its tick launches do not grow with B.  members_per_sweep (None:
    all members in one sweep) bounds the tape memory: the backward then runs groups of that many members in ascending order and adds
    the groups' coefficient gradients in that order.  rows_per_window chains windows through q_final -> q0 as rapid_route does.
    gauges makes the first result discharge[B, T, G] at the reaches gauges[j], as in rapid_route: each member's values and gradients
    are those of rapid_route(..., gauges=gauges) for that member alone.  Every argument is checked before the GPU is touched."""
    nsub = _check_call(plan, 'n', (), k, x, dt_routing, dt_runoff, rows_per_window)
    n = plan.n
    host_gauges = None if gauges is None else _check_gauges(gauges, n)
    _check_members_per_sweep(members_per_sweep)
    if not isinstance(q0, torch.Tensor) or q0.ndim not in (1, 2):
        raise ValueError('q0 must be a (B, n) tensor, or (n,) for one state shared by every member')
    if qlateral is None:
        if q0.ndim != 2:
            raise ValueError('channel-only routing (qlateral=None) takes its member count from q0, which must be (B, n)')
        if rows is None or int(rows) < 1:
            raise ValueError('channel-only routing (qlateral=None) needs rows >= 1')
        B, T = int(q0.shape[0]), int(rows)
    else:
        B, T = _check_member_rows(qlateral, 'qlateral', n, 'rapid_route')
    if B < 1:
        raise ValueError('no members')
    _check_tensor(q0, 'q0', (B, n) if q0.ndim == 2 else (n,))
    _check_device(plan, ((q0, 'q0'), (qlateral, 'qlateral')))
    c1, c2, c3 = muskingum_coefficients(k, x, float(dt_routing))
    c4dt = (c1 + c2) / float(dt_runoff)
    if q0.ndim == 1:
        q0 = q0.unsqueeze(0).expand(B, n)      # autograd sums the members' rows into the one q0
    whole = rows_per_window is None or int(rows_per_window) >= T      # a window of the rows: its own contiguous copy
    on_device = None if gauges is None else _upload_gauges(plan, gauges, host_gauges)
    return _in_windows(T, rows_per_window, (q0,), lambda t0, t1, q: RapidRouteBatch.apply(
        plan, nsub, t1 - t0, members_per_sweep, on_device, q,
        None if qlateral is None else qlateral if whole else qlateral[:, t0:t1].contiguous(), c1, c2, c3, c4dt), axis=1)


# ---- UnitMuskingum ----

class UhConvolve(torch.autograd.Function):
    """(convolved[T, n], state_out[n_ks, n]) = UnitHydrograph.convolve of depth[T, n] with kernel[n_ks, n] from the carried state.
    Forward: rr_uh_convolve_dev on a copy of the state; backward: rr_uh_adjoint_dev."""

    @staticmethod
    def forward(ctx, kernel, state, depth):
        dev = depth.device.index
        n_ks, n = kernel.shape
        T = int(depth.shape[0])
        stream = torch.cuda.current_stream(dev).cuda_stream
        state_out = state.detach().clone()
        convolved = torch.empty((T, n), dtype=torch.float64, device=depth.device)
        engine.uh_convolve_dev(kernel.detach(), state_out, depth.detach(), convolved, T, n_ks, n, dev, stream)
        ctx.save_for_backward(kernel, depth)
        ctx.set_materialize_grads(False)
        return convolved, state_out

    @staticmethod
    def backward(ctx, grad_convolved, grad_state_out):
        kernel, depth = ctx.saved_tensors
        need = ctx.needs_input_grad      # kernel, state, depth
        if (grad_convolved is None and grad_state_out is None) or not any(need):
            return None, None, None
        dev = depth.device.index
        n_ks, n = kernel.shape
        T = int(depth.shape[0])
        f64 = dict(dtype=torch.float64, device=depth.device)
        g_c = None if grad_convolved is None else grad_convolved.to(**f64).contiguous()
        g_s = None if grad_state_out is None else grad_state_out.to(**f64).contiguous()
        g_kernel = torch.empty((n_ks, n), **f64) if need[0] else None
        g_state = torch.empty((n_ks, n), **f64) if need[1] else None
        g_depth = torch.empty((T, n), **f64) if need[2] else None
        nbytes = engine.uh_adjoint_work_bytes(T, n_ks, n) if need[0] else 0
        work = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=depth.device)
        engine.uh_adjoint_dev(kernel.detach(), depth.detach(), g_c, g_s, g_depth, g_kernel, g_state, work, nbytes, T, n_ks, n, dev,
                              torch.cuda.current_stream(dev).cuda_stream)
        return g_kernel, g_state, g_depth


class UnitRoute(torch.autograd.Function):
    """(discharge[T, n], q_ch[n_inner], q_full[n_inner]) = UnitMuskingum routing of T rows of convolved lateral inflow from q_ch0,
    q_full0 with nsub sub-steps per row and per-reach coefficients c1, c2, c3.  Forward: rr_unit_route_dev; backward:
    rr_unit_adjoint_dev, which rebuilds the state tape, so only references to the inputs and the discharge are kept between the two."""

    @staticmethod
    def forward(ctx, plan, nsub, q_ch0, q_full0, lateral, c1, c2, c3):
        dev = plan.device
        T = int(lateral.shape[0])
        _set_coeffs(plan, c1, c2, c3, None, dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        q_ch, q_full = q_ch0.detach().clone(), q_full0.detach().clone()
        discharge = torch.empty((T, plan.n), dtype=torch.float64, device=lateral.device)
        plan.unit_route_dev(q_ch, q_full, lateral.detach(), T, discharge, T, T, nsub, stream)
        ctx.plan, ctx.nsub = plan, int(nsub)
        ctx.coeffs = (c1.detach(), c2.detach(), c3.detach())
        ctx.save_for_backward(q_ch0, q_full0, lateral, discharge)
        ctx.set_materialize_grads(False)
        return discharge, q_ch, q_full

    @staticmethod
    def backward(ctx, grad_discharge, grad_qch, grad_qfull):
        plan, nsub = ctx.plan, ctx.nsub
        q_ch0, q_full0, lateral, discharge = ctx.saved_tensors
        T = int(lateral.shape[0])
        need = ctx.needs_input_grad      # plan, nsub, q_ch0, q_full0, lateral, c1, c2, c3
        want_coef = any(need[5:8])
        if (grad_discharge is None and grad_qch is None and grad_qfull is None) or not (any(need[2:5]) or want_coef):
            return (None,) * 8
        return (None, None, *_route_backward(
            plan, ctx.coeffs, None, lateral.device, (grad_discharge, grad_qch, grad_qfull),
            (plan.n_inner if need[2] else None, plan.n_inner if need[3] else None, (T, plan.n) if need[4] else None), want_coef, need[5:8],
            lambda: plan.unit_adjoint_work_bytes(T, nsub),
            lambda g_out, g_c, g_f, g_qch0, g_qfull0, g_lat, g_coef, work, nbytes, stream: plan.unit_adjoint_dev(
                q_ch0.detach(), q_full0.detach(), lateral.detach(), T, discharge, g_out, g_c, g_f, g_lat, g_qch0, g_qfull0, g_coef, work,
                nbytes, T, nsub, stream)))


def uh_convolve(kernel, state, depth):
    """Differentiable UnitHydrograph.convolve (river_route/uhkernels/UnitHydrograph.py:77-107): (convolved[T, n], state_out[n_ks, n])
    from kernel[n_ks, n], the carried state[n_ks, n] and depth[T, n], float64 tensors on one GPU.  The inputs are not modified;
    convolved is the array engine.uh_convolve_dev computes, bit for bit.  Gradients reach kernel, state and depth."""
    if not isinstance(kernel, torch.Tensor) or kernel.ndim != 2:
        raise ValueError('kernel must be a 2-D (n_ks, n) tensor')
    n_ks, n = (int(v) for v in kernel.shape)
    if n_ks < 1:
        raise ValueError('kernel has no steps')
    _check_tensor(kernel, 'kernel', (n_ks, n))
    _check_tensor(state, 'state', (n_ks, n))
    _check_rows(depth, 'depth', n)
    if depth.device.type != 'cuda':
        raise ValueError(f'depth must be on a GPU (it is on {depth.device})')
    for t, name in ((kernel, 'kernel'), (state, 'state')):
        if t.device != depth.device:
            raise ValueError(f'{name} must be on cuda:{depth.device.index} (it is on {t.device})')
    return UhConvolve.apply(kernel, state, depth)


def _unit_route_one(plan, nsub, on_device, q_ch, q_full, lateral, c1, c2, c3):
    """One series through UnitRoute or, with gauges on the device, through the one-member case of the batched gauge call."""
    if on_device is None:
        return UnitRoute.apply(plan, nsub, q_ch, q_full, lateral, c1, c2, c3)
    d, q_ch, q_full = UnitRouteBatch.apply(plan, nsub, None, on_device, q_ch.unsqueeze(0), q_full.unsqueeze(0), lateral.unsqueeze(0), c1, c2, c3)
    return d[0], q_ch[0], q_full[0]


def unit_route(plan, q_ch0, q_full0, lateral, k, x, dt_routing, dt_runoff, rows_per_window=None, gauges=None):
    """Differentiable unit_route (river_route/routers/_numba_kernels.py:88-171) on an already convolved lateral:
    (discharge[T, n], q_ch[n_inner], q_full[n_inner]) as torch tensors on the plan's device.

    q_ch0 and q_full0 (one value per reach with upstream reaches, ascending params order) and lateral[T, n] are float64 tensors on
    the plan's GPU; k and x are float64 tensors of n values on any device.  c1, c2, c3 come from muskingum_coefficients(k, x,
    dt_routing) and go onto the plan without c4; the forward is Plan.unit_route_dev, bit for bit.  Gradients reach q_ch0, q_full0,
    lateral, k and x (a headwater's k and x get 0: its coefficients are never read).  rows_per_window routes the series in windows
    chained through the states, so the tape memory of the backward pass is one window's.

    gauges (a 1-D integer array or tensor of G distinct params-order reach indices, headwaters and inner reaches alike) makes the
    first result discharge[T, G], column j being reach gauges[j], for a loss that reads gauged reaches only: the values and every
    gradient are those of the call without it and discharge[:, gauges], bit for bit, but only the gauge columns are kept for the
    backward pass, which takes the (T, G) cotangent as it is (rr_unit_adjoint_gauges_dev), so nothing (T, n) is allocated for it
    unless lateral requires grad.  Every argument is checked before the GPU is touched."""
    nsub = _check_call(plan, 'n_inner', ((q_ch0, 'q_ch0'), (q_full0, 'q_full0')), k, x, dt_routing, dt_runoff, rows_per_window)
    host_gauges = None if gauges is None else _check_gauges(gauges, plan.n)
    T = _check_rows(lateral, 'lateral', plan.n)
    _check_device(plan, ((q_ch0, 'q_ch0'), (q_full0, 'q_full0'), (lateral, 'lateral')))
    c1, c2, c3 = muskingum_coefficients(k, x, float(dt_routing))
    on_device = None if gauges is None else _upload_gauges(plan, gauges, host_gauges)
    return _in_windows(T, rows_per_window, (q_ch0, q_full0), lambda t0, t1, q_ch, q_full: _unit_route_one(
        plan, nsub, on_device, q_ch, q_full, lateral[t0:t1], c1, c2, c3))


def unit_muskingum(plan, q_ch0, q_full0, depth, uh_kernel, uh_state, k, x, dt_routing, dt_runoff, rows_per_window=None, gauges=None):
    """Differentiable UnitMuskingum (the router's _router, river_route/routers/UnitMuskingum.py:72-98): the runoff depths are
    convolved with the unit-hydrograph kernel (uh_convolve) and the result is routed (unit_route).  Returns (discharge[T, n],
    q_ch[n_inner], q_full[n_inner], uh_state_out[n_ks, n]); gradients reach q_ch0, q_full0, depth, uh_kernel, uh_state, k and x.
    With rows_per_window each window convolves its own rows and hands q_ch, q_full and the convolution's state to the next, as the
    router does from file to file.  gauges makes the first result discharge[T, G] at the reaches gauges[j], as in unit_route: the
    routing step keeps and differentiates the gauge columns only (each window gathers its own rows), the convolution is unchanged,
    and every value and gradient is that of the call without it and discharge[:, gauges], bit for bit."""
    nsub = _check_call(plan, 'n_inner', ((q_ch0, 'q_ch0'), (q_full0, 'q_full0')), k, x, dt_routing, dt_runoff, rows_per_window)
    host_gauges = None if gauges is None else _check_gauges(gauges, plan.n)
    T = _check_rows(depth, 'depth', plan.n)
    if not isinstance(uh_kernel, torch.Tensor) or uh_kernel.ndim != 2 or int(uh_kernel.shape[0]) < 1:
        raise ValueError('uh_kernel must be a 2-D (n_ks, n) tensor')
    n_ks = int(uh_kernel.shape[0])
    _check_tensor(uh_kernel, 'uh_kernel', (n_ks, plan.n))
    _check_tensor(uh_state, 'uh_state', (n_ks, plan.n))
    _check_device(plan, ((q_ch0, 'q_ch0'), (q_full0, 'q_full0'), (depth, 'depth'), (uh_kernel, 'uh_kernel'), (uh_state, 'uh_state')))
    c1, c2, c3 = muskingum_coefficients(k, x, float(dt_routing))
    on_device = None if gauges is None else _upload_gauges(plan, gauges, host_gauges)

    def route(t0, t1, q_ch, q_full, state):
        lateral, state = UhConvolve.apply(uh_kernel, state, depth[t0:t1])
        return (*_unit_route_one(plan, nsub, on_device, q_ch, q_full, lateral, c1, c2, c3), state)

    return _in_windows(T, rows_per_window, (q_ch0, q_full0, uh_state), route)


# ---- UnitMuskingum, several series at once ----

class UhConvolveBatch(torch.autograd.Function):
    """(convolved[B, T, n], state_out[B, n_ks, n]) = UhConvolve for B series at once: one kernel[n_ks, n], state[B, n_ks, n] (any member
    pitch: an expanded (n_ks, n) state has pitch 0), depth[B, T, n] whose members' rows are adjacent.  Forward and backward run member by
    member through rr_uh_convolve_dev and rr_uh_adjoint_dev, so every member's values are UhConvolve's bits; dL/dkernel is added in
    member order."""

    @staticmethod
    def forward(ctx, kernel, state, depth):
        dev = depth.device.index
        n_ks, n = kernel.shape
        B, T = int(depth.shape[0]), int(depth.shape[1])
        stream = torch.cuda.current_stream(dev).cuda_stream
        state_out = state.detach().clone(memory_format=torch.contiguous_format)
        convolved = torch.empty((B, T, n), dtype=torch.float64, device=depth.device)
        k, d = kernel.detach(), depth.detach()
        for m in range(B):
            engine.uh_convolve_dev(k, state_out[m], d[m], convolved[m], T, n_ks, n, dev, stream)
        ctx.save_for_backward(kernel, depth)
        ctx.set_materialize_grads(False)
        return convolved, state_out

    @staticmethod
    def backward(ctx, grad_convolved, grad_state_out):
        kernel, depth = ctx.saved_tensors
        need = ctx.needs_input_grad      # kernel, state, depth
        if (grad_convolved is None and grad_state_out is None) or not any(need):
            return None, None, None
        dev = depth.device.index
        n_ks, n = kernel.shape
        B, T = int(depth.shape[0]), int(depth.shape[1])
        f64 = dict(dtype=torch.float64, device=depth.device)
        g_c = None if grad_convolved is None else grad_convolved.to(**f64).contiguous()
        g_s = None if grad_state_out is None else grad_state_out.to(**f64).contiguous()
        g_state = torch.empty((B, n_ks, n), **f64) if need[1] else None
        g_depth = torch.empty((B, T, n), **f64) if need[2] else None
        nbytes = engine.uh_adjoint_work_bytes(T, n_ks, n) if need[0] else 0
        work = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=depth.device)
        stream = torch.cuda.current_stream(dev).cuda_stream
        k, d = kernel.detach(), depth.detach()
        g_kernel = None

        def member(t, m):
            return None if t is None else t[m]

        for m in range(B):
            part = torch.empty((n_ks, n), **f64) if need[0] else None
            engine.uh_adjoint_dev(k, d[m], member(g_c, m), member(g_s, m), member(g_depth, m), part, member(g_state, m), work, nbytes, T, n_ks,
                                  n, dev, stream)
            if need[0]:
                g_kernel = part if g_kernel is None else g_kernel + part
        return g_kernel, g_state, g_depth


class UnitRouteBatch(torch.autograd.Function):
    """(discharge[B, T, n], q_ch[B, n_inner], q_full[B, n_inner]) = UnitRoute for B series at once: q_ch0, q_full0[B, n_inner] (rows of
    n_inner adjacent values, any pitch: an expanded (n_inner,) state has pitch 0), lateral[B, T, n], one set of coefficients.  Forward:
    UnitRoute's call, member by member, so every member's values are UnitRoute's bits.  Backward: rr_unit_adjoint_batch_dev on groups of
    `per_sweep` members (None: all) in ascending order, the groups' coefficient gradients added in that order.

    With `gauges` (None, or a pair of device tensors, int32 and int64, of G distinct params-order indices) the discharge is
    (B, T, G), at those reaches only: the forward routes every member into one (T, n) scratch tensor that is not kept and gathers the
    gauge columns out of it, so only q_ch0, q_full0, lateral and the (B, T, G) gauge discharge are kept; the backward is
    rr_unit_adjoint_gauges_dev, whose work memory has gradient rows only when lateral requires grad."""

    @staticmethod
    def forward(ctx, plan, nsub, per_sweep, gauges, q_ch0, q_full0, lateral, c1, c2, c3):
        dev = plan.device
        g32, g64 = (None, None) if gauges is None else gauges
        B, T = int(lateral.shape[0]), int(lateral.shape[1])
        _set_coeffs(plan, c1, c2, c3, None, dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        q_ch = q_ch0.detach().clone(memory_format=torch.contiguous_format)
        q_full = q_full0.detach().clone(memory_format=torch.contiguous_format)
        scratch = None if gauges is None else torch.empty((T, plan.n), dtype=torch.float64, device=lateral.device)
        discharge = torch.empty((B, T, plan.n if gauges is None else int(g32.shape[0])), dtype=torch.float64, device=lateral.device)
        lat = lateral.detach()
        for m in range(B):
            plan.unit_route_dev(q_ch[m], q_full[m], lat[m], T, discharge[m] if gauges is None else scratch, T, T, nsub, stream)
            if gauges is not None:
                torch.index_select(scratch, 1, g64, out=discharge[m])
        ctx.plan, ctx.nsub, ctx.per_sweep, ctx.g32 = plan, int(nsub), per_sweep, g32
        ctx.coeffs = (c1.detach(), c2.detach(), c3.detach())
        ctx.save_for_backward(q_ch0, q_full0, lateral, discharge)
        ctx.set_materialize_grads(False)
        return discharge, q_ch, q_full

    @staticmethod
    def backward(ctx, grad_discharge, grad_qch, grad_qfull):
        plan, nsub, g32 = ctx.plan, ctx.nsub, ctx.g32
        q_ch0, q_full0, lateral, discharge = ctx.saved_tensors
        need = ctx.needs_input_grad      # plan, nsub, per_sweep, gauges, q_ch0, q_full0, lateral, c1, c2, c3
        want_coef, want_lat = any(need[7:10]), need[6]
        if (grad_discharge is None and grad_qch is None and grad_qfull is None) or not (any(need[4:7]) or want_coef):
            return (None,) * 10
        B, T, n, ni, G = int(lateral.shape[0]), int(lateral.shape[1]), plan.n, plan.n_inner, int(discharge.shape[2])
        lat = lateral.detach()
        # one pitch serves both states: one of them shared and the other not, or no inner reach at all, and they go as dense rows
        qc, qf = q_ch0.detach(), q_full0.detach()
        if ni == 0 or B == 1 or qc.stride(0) != qf.stride(0):
            qc, qf = qc.contiguous(), qf.contiguous()
        pitch = int(qc.stride(0)) if B > 1 and ni > 0 else ni

        def state(t, m0):
            return t.data_ptr() + 8 * m0 * pitch if ni > 0 else None

        def work_bytes(members):
            if g32 is None:
                return plan.unit_adjoint_batch_work_bytes(members, T, nsub)
            return plan.unit_adjoint_gauges_work_bytes(members, G, T, nsub, want_lat)

        def adjoint(m0, m1, g_out, g_c, g_f, g_qch0, g_qfull0, g_lat, g_coef, work, nbytes, stream):
            inputs = (state(qc, m0), state(qf, m0), pitch, lat[m0:m1], T, T * n)
            rest = (g_c, g_f, g_lat, g_qch0, g_qfull0, g_coef, work, nbytes, T, nsub, stream)
            if g32 is None:
                plan.unit_adjoint_batch_dev(m1 - m0, *inputs, discharge[m0:m1], g_out, T * n, *rest)
            else:      # the gauge discharge goes with its cotangent only: the engine refuses one without the other
                plan.unit_adjoint_gauges_dev(m1 - m0, G, g32, *inputs, None if g_out is None else discharge[m0:m1], g_out, T * G, *rest)

        return (None, None, None, None, *_members_backward(
            plan, ctx.coeffs, None, discharge.device, B, ctx.per_sweep, (grad_discharge, grad_qch, grad_qfull),
            ((ni,) if need[4] else None, (ni,) if need[5] else None, (T, n) if want_lat else None), want_coef, need[7:10],
            work_bytes, adjoint))


def _check_unit_batch(plan, q_ch0, q_full0, rows, rows_name, single, k, x, dt_routing, dt_runoff, rows_per_window, members_per_sweep):
    """The checks unit_route_batch and unit_muskingum_batch share.  Returns nsub, B, T."""
    nsub = _check_call(plan, 'n_inner', (), k, x, dt_routing, dt_runoff, rows_per_window)
    _check_members_per_sweep(members_per_sweep)
    B, T = _check_member_rows(rows, rows_name, plan.n, single)
    for t, name in ((q_ch0, 'q_ch0'), (q_full0, 'q_full0')):
        _check_member_state(t, name, B, (plan.n_inner,))
    return nsub, B, T


def uh_convolve_batch(kernel, state, depth):
    """uh_convolve for B series of runoff depths and one kernel: (convolved[B, T, n], state_out[B, n_ks, n]).

    kernel[n_ks, n] and depth[B, T, n] are contiguous float64 tensors on one GPU; state is (B, n_ks, n), or (n_ks, n) for one carried state
    shared by every member, whose gradient is then the sum over the members.  Every member's values and its dL/dstate and dL/ddepth are
    the bits uh_convolve gives for that member alone; dL/dkernel is the sum over the members, added in member order.  The calls run
    member by member (rr_uh_convolve_dev, rr_uh_adjoint_dev): the convolution's adjoint is a few launches per member, not one per tick,
    so there is nothing for a member dimension to save."""
    if not isinstance(kernel, torch.Tensor) or kernel.ndim != 2:
        raise ValueError('kernel must be a 2-D (n_ks, n) tensor')
    n_ks, n = (int(v) for v in kernel.shape)
    if n_ks < 1:
        raise ValueError('kernel has no steps')
    _check_tensor(kernel, 'kernel', (n_ks, n))
    B, _ = _check_member_rows(depth, 'depth', n, 'uh_convolve')
    _check_member_state(state, 'state', B, (n_ks, n))
    if depth.device.type != 'cuda':
        raise ValueError(f'depth must be on a GPU (it is on {depth.device})')
    for t, name in ((kernel, 'kernel'), (state, 'state')):
        if t.device != depth.device:
            raise ValueError(f'{name} must be on cuda:{depth.device.index} (it is on {t.device})')
    return UhConvolveBatch.apply(kernel, _per_member(state, B, (n_ks, n)), depth)


def unit_route_batch(plan, q_ch0, q_full0, lateral, k, x, dt_routing, dt_runoff, rows_per_window=None, members_per_sweep=None, gauges=None):
    """unit_route for B series of convolved lateral inflow on one network and one set of coefficients: (discharge[B, T, n],
    q_ch[B, n_inner], q_full[B, n_inner]).

    lateral[B, T, n] is a contiguous float64 tensor on the plan's GPU; q_ch0 and q_full0 are (B, n_inner), or (n_inner,) for one state
    shared by every member, whose gradient is then the sum over the members; k and x are as in unit_route and serve all members.  Every
    member's discharge, q_ch and q_full are the bits unit_route gives for that member alone (the forward is the same call, member by
    member), and so are its dL/dlateral, dL/dq_ch0 and dL/dq_full0; k and x get the sum over the members.  The backward pass is one
    rr_unit_adjoint_batch_dev call: its tick launches do not grow with B.  members_per_sweep (None: all members in one sweep) bounds the
    tape memory: the backward then runs groups of that many members in ascending order and adds the groups' coefficient gradients in
    that order.  rows_per_window chains windows through the states as unit_route does.  gauges makes the first result
    discharge[B, T, G] at the reaches gauges[j], as in unit_route: each member's values and gradients are those of unit_route(...,
    gauges=gauges) for that member alone (backward: rr_unit_adjoint_gauges_dev).  Every argument is checked before the GPU is touched."""
    nsub, B, T = _check_unit_batch(plan, q_ch0, q_full0, lateral, 'lateral', 'unit_route', k, x, dt_routing, dt_runoff, rows_per_window,
                                   members_per_sweep)
    host_gauges = None if gauges is None else _check_gauges(gauges, plan.n)
    _check_device(plan, ((q_ch0, 'q_ch0'), (q_full0, 'q_full0'), (lateral, 'lateral')))
    c1, c2, c3 = muskingum_coefficients(k, x, float(dt_routing))
    ni = plan.n_inner
    whole = rows_per_window is None or int(rows_per_window) >= T      # a window of the rows: its own contiguous copy
    on_device = None if gauges is None else _upload_gauges(plan, gauges, host_gauges)
    return _in_windows(T, rows_per_window, (_per_member(q_ch0, B, (ni,)), _per_member(q_full0, B, (ni,))),
                       lambda t0, t1, q_ch, q_full: UnitRouteBatch.apply(
                           plan, nsub, members_per_sweep, on_device, q_ch, q_full, lateral if whole else lateral[:, t0:t1].contiguous(),
                           c1, c2, c3), axis=1)


def unit_muskingum_batch(plan, q_ch0, q_full0, depth, uh_kernel, uh_state, k, x, dt_routing, dt_runoff, rows_per_window=None,
                         members_per_sweep=None, gauges=None):
    """unit_muskingum for B series of runoff depths: uh_convolve_batch and unit_route_batch chained per window, as unit_muskingum chains
    uh_convolve and unit_route.  depth is (B, T, n); uh_state is (B, n_ks, n), or (n_ks, n) for one shared by every member, as q_ch0 and
    q_full0 may be (n_inner,).  Returns (discharge[B, T, n], q_ch[B, n_inner], q_full[B, n_inner], uh_state_out[B, n_ks, n]); gradients
    reach q_ch0, q_full0, depth, uh_kernel, uh_state, k and x, the shared ones summed over the members.  gauges makes the first result
    discharge[B, T, G] at the reaches gauges[j], as in unit_route_batch; the convolution is unchanged."""
    nsub, B, T = _check_unit_batch(plan, q_ch0, q_full0, depth, 'depth', 'unit_muskingum', k, x, dt_routing, dt_runoff, rows_per_window,
                                   members_per_sweep)
    host_gauges = None if gauges is None else _check_gauges(gauges, plan.n)
    if not isinstance(uh_kernel, torch.Tensor) or uh_kernel.ndim != 2 or int(uh_kernel.shape[0]) < 1:
        raise ValueError('uh_kernel must be a 2-D (n_ks, n) tensor')
    n_ks, n, ni = int(uh_kernel.shape[0]), plan.n, plan.n_inner
    _check_tensor(uh_kernel, 'uh_kernel', (n_ks, n))
    _check_member_state(uh_state, 'uh_state', B, (n_ks, n))
    _check_device(plan, ((q_ch0, 'q_ch0'), (q_full0, 'q_full0'), (depth, 'depth'), (uh_kernel, 'uh_kernel'), (uh_state, 'uh_state')))
    c1, c2, c3 = muskingum_coefficients(k, x, float(dt_routing))

    on_device = None if gauges is None else _upload_gauges(plan, gauges, host_gauges)

    def route(t0, t1, q_ch, q_full, state):      # a member's rows of a window are adjacent: the convolution reads them in place
        lateral, state = UhConvolveBatch.apply(uh_kernel, state, depth[:, t0:t1])
        return (*UnitRouteBatch.apply(plan, nsub, members_per_sweep, on_device, q_ch, q_full, lateral, c1, c2, c3), state)

    return _in_windows(T, rows_per_window, (_per_member(q_ch0, B, (ni,)), _per_member(q_full0, B, (ni,)), _per_member(uh_state, B, (n_ks, n))),
                       route, axis=1)


# ---- skill scores as a loss ----

def _pitch(a) -> int:
    """Elements from one row of a 2-D tensor that metrics._Rows accepted to the next (one row: its width)."""
    return int(a.stride(0)) if a.shape[0] > 1 else int(a.shape[1])


def column_map_pointers(cols_dev, n, n_distinct):
    """Device addresses of (columns, order, distinct columns, segment starts) inside the one int32 tensor that
    np.concatenate(_sorted_columns(...)) uploads: n, n, n_distinct and n_distinct + 1 values.  None: four times None."""
    if cols_dev is None:
        return None, None, None, None
    base, size = cols_dev.data_ptr(), cols_dev.element_size()
    return tuple(base + k * size for k in (0, n, 2 * n, 2 * n + n_distinct))


class Scores(torch.autograd.Function):
    """out[5, n] = the scores of rr.metrics.SCORES per column of y_true[T, n] (the tensor of a metrics._Rows, a constant) against
    y_pred, a (T, m) or (T,) tensor.  Forward: rr_metrics_update_dev and rr_metrics_finish_dev, as rr.metrics.scores calls them.
    Backward: rr_metrics_adjoint_dev from the 9 x n state the forward left; beside it only the two inputs (saved tensors, read in
    place) and the sorted column map are kept.  cols is None or (columns, order, distinct columns, segment starts) as int32 host
    arrays.  skip_missing: both passes through rr_metrics_update_missing_dev / rr_metrics_adjoint_missing_dev, and out[6, n] with the
    kept pairs per column (row 0 of the state) as its last row, which `scores` returns detached."""

    @staticmethod
    def forward(ctx, y_pred, y_true, cols, skip_missing=False):
        t, p = y_true, metrics._Rows(y_pred.detach(), 'y_pred').tensor
        dev, where = p.device.index or 0, p.device
        T, n = (int(v) for v in t.shape)
        f32 = torch.float32
        stream = torch.cuda.current_stream(dev).cuda_stream
        cols_dev = None if cols is None else torch.from_numpy(np.concatenate(cols)).to(where)
        state = torch.zeros((engine.METRICS_STATE, n), dtype=torch.float64, device=where)
        nbytes = engine.metrics_work_bytes(n, T)
        work = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=where)
        n_distinct = n if cols is None else len(cols[2])
        update = engine.metrics_update_missing_dev if skip_missing else engine.metrics_update_dev
        update(n, T, t.data_ptr(), t.dtype == f32, _pitch(t), p.data_ptr(), p.dtype == f32, _pitch(p),
               column_map_pointers(cols_dev, n, n_distinct)[0], state, work, nbytes, device=dev, stream=stream)
        out = torch.empty((engine.METRICS_SCORES + (1 if skip_missing else 0), n), dtype=torch.float64, device=where)
        engine.metrics_finish_dev(n, state, out, device=dev, stream=stream)      # rows 0 .. 4
        if skip_missing:
            out[engine.METRICS_SCORES] = state[0]
        ctx.skip_missing = bool(skip_missing)
        ctx.save_for_backward(t, p, state, cols_dev)      # a change of the rows in place between the two passes is noticed
        ctx.n_distinct = n_distinct
        ctx.pred_shape = tuple(y_pred.shape)
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        if grad_out is None or not ctx.needs_input_grad[0]:
            return None, None, None, None
        t, p, state, cols_dev = ctx.saved_tensors
        dev, where, nd = p.device.index or 0, p.device, ctx.n_distinct
        T, n = (int(v) for v in t.shape)
        m = int(p.shape[1])
        f32 = torch.float32
        g = grad_out[:engine.METRICS_SCORES].to(dtype=torch.float64, device=where).contiguous()      # 'count' passes no gradient
        _, order, distinct, segments = column_map_pointers(cols_dev, n, nd)
        # unscored columns are zero and stay so: the kernel writes the scored ones only
        make = torch.empty if cols_dev is None else torch.zeros
        grad = make((T, m), dtype=p.dtype, device=where)
        nbytes = engine.metrics_adjoint_work_bytes(n)
        work = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=where)
        adjoint = engine.metrics_adjoint_missing_dev if ctx.skip_missing else engine.metrics_adjoint_dev
        adjoint(n, T, t.data_ptr(), t.dtype == f32, _pitch(t), p.data_ptr(), p.dtype == f32, _pitch(p), state, g, nd, order,
                distinct, segments, grad, m, work, nbytes, device=dev, stream=torch.cuda.current_stream(dev).cuda_stream)
        return grad.reshape(ctx.pred_shape), None, None, None


def _check_series(a, name):
    if not isinstance(a, torch.Tensor):
        raise TypeError(f'{name} must be a torch tensor on the GPU (rr.metrics.scores takes numpy arrays; it has no gradient)')
    if a.dtype not in (torch.float32, torch.float64):
        raise TypeError(f'{name} must be float32 or float64 (it is {a.dtype})')
    if a.dim() not in (1, 2):
        raise ValueError(f'{name} must be 1-D (time) or 2-D (time, column)')
    return int(a.shape[0]), (int(a.shape[1]) if a.dim() == 2 else 1)


def _sorted_columns(columns, n, m):
    """columns (host values) checked against n scored columns and y_pred's m, with the backward's segment map: (columns, a stable
    argsort, the distinct values, the start of each value's run) as int32, so a column scored several times adds its shares by
    ascending index."""
    c = np.asarray(columns)
    if c.shape != (n,) or not np.issubdtype(c.dtype, np.integer):
        raise ValueError(f'columns must be a 1-D integer array of length {n}')
    if c.min() < 0 or c.max() >= m:
        raise ValueError(f'columns refers to column {int(c.min() if c.min() < 0 else c.max())} of y_pred, which has {m} columns')
    if m > np.iinfo(np.int32).max:
        raise ValueError('y_pred has too many columns for a column map')
    order = np.argsort(c, kind='stable')
    distinct, starts = np.unique(c[order], return_index=True)
    return tuple(a.astype(np.int32) for a in (c, order, distinct, np.append(starts, n)))


def scores(y_true, y_pred, columns=None, skip_missing=False) -> dict:
    """rr.metrics.scores with autograd: {'me', 'mae', 'mse', 'pearson_r', 'kge2012'} -> (n,) float64 tensors on the GPU, the values
    rr.metrics.scores returns for the same tensors bit for bit, each carrying a graph to y_pred.

    y_true (T, n) or (T,) and y_pred (T, m) or (T,) are float32 or float64 tensors on one GPU; y_true is a constant (one that
    requires grad is refused).  columns: optional int array of length n, column j of y_true is scored against column columns[j]
    of y_pred (repeats allowed, no gather copy); without it m must equal n.  Views whose columns are adjacent and whose rows do
    not overlap are read in place, others are copied first.

    The backward pass writes dL/dy_pred (y_pred's shape and dtype) on the GPU from the per-column state the forward left: columns
    nobody scores get 0, a column scored several times the sum of its shares.  A score whose incoming gradient is exactly 0 for a
    column adds nothing there, so a constant series may sit in an mse loss although its pearson_r and kge2012 are NaN; a NaN score
    with a non-zero gradient makes the column's gradient NaN.  No atomics: two backward passes give the same bits.  Every argument
    is checked before the GPU is touched.

    skip_missing=True: a NaN in y_true is a missing observation, as in rr.metrics.scores(..., skip_missing=True): column j's pair at
    that row is left out of its sums, and the result has the key 'count' (the pairs kept per column, detached: no graph).  The
    gradient at a kept element is the same closed form with the kept pairs' count and moments; at a skipped element column j adds
    exactly 0.0, never NaN, and a column that keeps nothing adds zeros.  With repeats in columns= every share is masked by its own
    y_true column.  A NaN score with a non-zero gradient makes the gradient NaN at the column's kept rows."""
    T, n = _check_series(y_true, 'y_true')
    Tp, m = _check_series(y_pred, 'y_pred')
    if y_true.requires_grad:
        raise ValueError('y_true is a constant here: it must not require grad (detach it)')
    if T != Tp:
        raise ValueError(f'y_true has {T} rows, y_pred {Tp}')
    if T < 1:
        raise ValueError('y_true and y_pred have no rows')
    if n < 1:
        raise ValueError('y_true has no columns')
    cols = None
    if columns is None:
        if m != n:
            raise ValueError(f'y_pred has {m} columns, expected {n} (or pass columns=)')
    else:
        on_gpu = isinstance(columns, torch.Tensor) and columns.device.type != 'cpu'
        if on_gpu:      # its values are read after the device checks; shape and type need no device
            if columns.dim() != 1 or int(columns.shape[0]) != n or columns.is_floating_point() or columns.is_complex() or columns.dtype == torch.bool:
                raise ValueError(f'columns must be a 1-D integer array of length {n}')
        else:
            cols = _sorted_columns(columns, n, m)
    for a, name in ((y_true, 'y_true'), (y_pred, 'y_pred')):
        if a.device.type != 'cuda':
            raise ValueError(f'{name} must be on the GPU (it is on {a.device})')
    if y_true.device != y_pred.device:
        raise ValueError(f'y_true is on {y_true.device}, y_pred on {y_pred.device}')
    if columns is not None and cols is None:
        cols = _sorted_columns(columns.detach().cpu(), n, m)
    out = Scores.apply(y_pred, metrics._Rows(y_true, 'y_true').tensor, cols, bool(skip_missing))
    res = {k: out[i] for i, k in enumerate(metrics.SCORES)}
    if skip_missing:
        res['count'] = out[engine.METRICS_SCORES].detach()
    return res


class RunoffMap:
    """The structure of a catchment / grid-cell weight table for runoff_to_qlateral: the CSR arrays of rr_runoff_to_qlateral_dev
    (indptr[n + 1], indices[nnz]: river r owns the pairs indptr[r] .. indptr[r + 1] - 1, pair k reads grid point indices[k]) and the
    transposed (CSC) structure the backward pass walks, derived here once by a stable sort of the pairs by point: t_indptr[n_points + 1]
    and t_pairs[nnz], the pair indices of point p, ascending, at t_pairs[t_indptr[p] : t_indptr[p + 1]].  All four are int32 host arrays
    and attributes, with pair_river[nnz], n_rivers, n_points, nnz and device.  Building one needs no GPU; the device copy (one int32
    tensor) is uploaded by the first call that uses it and kept, so a training loop uploads the structure once."""

    def __init__(self, indptr, indices, n_points, device: int = 0):
        indptr, indices = np.asarray(indptr), np.asarray(indices)
        for a, name in ((indptr, 'indptr'), (indices, 'indices')):
            if a.ndim != 1 or not np.issubdtype(a.dtype, np.integer):
                raise ValueError(f'{name} must be a 1-D integer array')
        n_points = int(n_points)
        imax = np.iinfo(np.int32).max
        if indptr.shape[0] < 1 or indptr[0] != 0 or np.any(np.diff(indptr) < 0) or int(indptr[-1]) != indices.shape[0]:
            raise ValueError('indptr must start at 0, not decrease and end at len(indices)')
        if n_points < 0 or max(n_points, indptr.shape[0] - 1, indices.shape[0]) > imax:
            raise ValueError('n_points must be >= 0 and the table must fit int32 indices')
        if indices.shape[0] and (indices.min() < 0 or indices.max() >= n_points):
            bad = int(indices.min() if indices.min() < 0 else indices.max())
            raise ValueError(f'n_points is {n_points}, but indices refers to grid point {bad}')
        self.indptr = np.ascontiguousarray(indptr, dtype=np.int32)
        self.indices = np.ascontiguousarray(indices, dtype=np.int32)
        self.n_rivers, self.n_points, self.nnz, self.device = int(indptr.shape[0]) - 1, n_points, int(indices.shape[0]), int(device)
        self.t_pairs = np.argsort(self.indices, kind='stable').astype(np.int32)
        self.t_indptr = np.concatenate(([0], np.cumsum(np.bincount(self.indices, minlength=n_points)))).astype(np.int32)
        self.pair_river = np.repeat(np.arange(self.n_rivers, dtype=np.int32), np.diff(self.indptr))
        self._tables = None

    @classmethod
    def from_source(cls, src, device: int | None = None):
        """The map of a rr.runoff.RunoffSource (prepare_runoff): its CSR structure over the points of its runoff block."""
        return cls(src.indptr, src.indices, int(np.shape(src.runoff_tp)[1]), src.device if device is None else device)

    def device_pointers(self):
        """Device addresses of (indptr, indices, t_indptr, t_pairs), uploading them on the first call."""
        if self._tables is None:
            host = np.concatenate((self.indptr, self.indices, self.t_indptr, self.t_pairs))
            self._tables = torch.from_numpy(host).to(f'cuda:{self.device}')
        base, n, nnz = self._tables.data_ptr(), self.n_rivers + 1, self.nnz
        return tuple(base + 4 * k for k in (0, n, n + nnz, n + nnz + self.n_points + 1))


class RunoffToQlateral(torch.autograd.Function):
    """qlateral[T, n] = rr_runoff_to_qlateral_dev of runoff[T, n_points] (float32 or float64, any strides) with weights[nnz], area[n] or
    None and the RR_RUNOFF_* flags, on torch's current stream.  Backward: rr_runoff_adjoint_dev, which computes the weighted sums and
    the mask again, so beside references to the inputs only the point-major working copy of the runoff is kept (none where the runoff
    came point-major); an output nobody needs is passed as NULL and costs no pass."""

    @staticmethod
    def forward(ctx, rmap, flags, runoff, weights, area):
        dev = rmap.device
        T = int(runoff.shape[0])
        r, w = _vector_layout(runoff.detach()), weights.detach().contiguous()
        a = None if area is None else area.detach().contiguous()
        indptr, indices, _, _ = rmap.device_pointers()
        out = torch.empty((T, rmap.n_rivers), dtype=torch.float64, device=runoff.device)
        engine.runoff_to_qlateral_dev(rmap.n_rivers, rmap.n_points, T, indptr, indices, w, r.data_ptr(), r.dtype == torch.float32, r.stride(0),
                                      r.stride(1), a, flags, out, device=dev, stream=torch.cuda.current_stream(dev).cuda_stream)
        ctx.rmap, ctx.flags = rmap, int(flags)
        ctx.point_major = r if ctx.needs_input_grad[2] or ctx.needs_input_grad[3] else None      # the working copy, once for both passes
        ctx.save_for_backward(runoff, weights, area)      # a change of the runoff in place between the two passes is noticed
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_q):
        need = ctx.needs_input_grad      # rmap, flags, runoff, weights, area
        if grad_q is None or not (need[2] or need[3]):
            return (None,) * 5
        rmap, dev = ctx.rmap, ctx.rmap.device
        runoff, weights, area = ctx.saved_tensors
        T, P = int(runoff.shape[0]), rmap.n_points
        where = runoff.device
        r, w = ctx.point_major, weights.detach().contiguous()
        a = None if area is None else area.detach().contiguous()
        g = grad_q.to(dtype=torch.float64, device=where).contiguous()
        grad_runoff = torch.empty((T, P), dtype=runoff.dtype, device=where) if need[2] else None
        grad_weights = torch.empty(rmap.nnz, dtype=torch.float64, device=where) if need[3] else None
        nbytes = engine.runoff_adjoint_work_bytes(rmap.n_rivers, P, T)
        work = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=where)
        indptr, indices, t_indptr, t_pairs = rmap.device_pointers()
        engine.runoff_adjoint_dev(rmap.n_rivers, P, T, indptr, indices, w, t_indptr, t_pairs, r.data_ptr(), r.dtype == torch.float32, r.stride(0),
                                  r.stride(1), a, ctx.flags, g, grad_runoff, P, grad_weights, work, nbytes, device=dev,
                                  stream=torch.cuda.current_stream(dev).cuda_stream)
        return None, None, grad_runoff, grad_weights, None


def _vector_layout(r):
    """The (T, P) runoff as the kernels read it fastest: point-major with rows of a multiple of 16 elements, allocated in full and
    zero-padded (stride_t = 1), so each gathered grid point is a run of 16-byte vectors.  A tensor that already lies so is returned as
    it is; any other is copied once (sums in stored order do not depend on the layout: the values are the same bits)."""
    T, P = (int(v) for v in r.shape)
    t_pad = -(-T // 16) * 16
    if r.stride(0) == 1 and r.stride(1) % 16 == 0 and r.stride(1) >= t_pad and r.data_ptr() % 16 == 0:
        return r
    block = torch.empty((P, t_pad), dtype=r.dtype, device=r.device)
    block[:, T:] = 0
    block[:, :T] = r.t()
    return block[:, :T].t()


def runoff_to_qlateral(rmap, runoff, weights, area=None, *, cumulative: bool = False, force_positive: bool = False):
    """Gridded runoff -> catchment lateral inflow with autograd: qlateral (T, n) float64 on the GPU, bit for bit what
    engine.runoff_to_qlateral computes from the same data -- S[t, r] = sum_k weights[k] runoff[t, indices[k]] over river r's pairs in
    stored order, then cumulative -> incremental (row t minus row t - 1, row 0 kept), force_positive -> clip at 0, NaN -> 0, and
    times area[r] when area is given -- carrying a graph to runoff and weights, whichever require grad.

    rmap: a RunoffMap (the table's structure, uploaded once); runoff: (T, n_points) float32 or float64 tensor on the map's GPU, any
    strides (a point-major tensor whose rows are a multiple of 16 elements long and allocated in full, block[:, :T].T, is read in
    place; any other is copied into that layout once per call, which the kernels' vector path repays); weights: (nnz,) float64; area: None or (n,) float64, a constant (one that requires grad is refused).

    The backward pass (rr_runoff_adjoint_dev, on torch's current stream) writes dL/drunoff in runoff's dtype and dL/dweights in
    float64.  The clip passes the gradient where the unclipped value is >= 0 (torch.clamp's rule: an exactly dry catchment can be
    learned wet); a NaN of the runoff passes none and poisons nothing, so both gradients are finite whenever the incoming one is.
    Grid points no river uses get exact zeros.  No atomics: two backward passes give the same bits.  The irregular-time resampling of
    rr.runoff.runoff_to_qlateral stays on the host and is not part of this.  Every argument is checked before the GPU is touched."""
    if not isinstance(rmap, RunoffMap):
        raise TypeError('rmap must be a rr.grad.RunoffMap')
    for t, name, kinds in ((runoff, 'runoff', (torch.float32, torch.float64)), (weights, 'weights', (torch.float64,)), (area, 'area', (torch.float64,))):
        if t is None and name == 'area':
            continue
        if not isinstance(t, torch.Tensor):
            raise TypeError(f'{name} must be a torch tensor on the GPU')
        if t.dtype not in kinds:
            raise TypeError(f"{name} must be {' or '.join(str(k).replace('torch.', '') for k in kinds)} (it is {t.dtype})")
    if runoff.dim() != 2:
        raise ValueError('runoff must be a 2-D (time, points) tensor (members have no axis here: loop over them)')
    if int(runoff.shape[0]) < 1:
        raise ValueError('runoff has no rows')
    if int(runoff.shape[1]) != rmap.n_points or rmap.n_points < 1:
        raise ValueError(f'runoff has {int(runoff.shape[1])} grid points, rmap has {rmap.n_points} (at least one is needed)')
    if tuple(weights.shape) != (rmap.nnz,):
        raise ValueError(f'weights has shape {tuple(weights.shape)}, expected ({rmap.nnz},): one value per pair of rmap')
    if area is not None:
        if tuple(area.shape) != (rmap.n_rivers,):
            raise ValueError(f'area has shape {tuple(area.shape)}, expected ({rmap.n_rivers},): one value per river')
        if area.requires_grad:
            raise ValueError('area is a constant here: it must not require grad (detach it)')
    for t, name in ((runoff, 'runoff'), (weights, 'weights'), (area, 'area')):
        if t is not None and (t.device.type != 'cuda' or (t.device.index or 0) != rmap.device):
            raise ValueError(f"{name} must be on cuda:{rmap.device}, rmap's device (it is on {t.device})")
    flags = (engine.RUNOFF_CUMULATIVE if cumulative else 0) | (engine.RUNOFF_FORCE_POSITIVE if force_positive else 0)
    return RunoffToQlateral.apply(rmap, flags, runoff, weights, area)
