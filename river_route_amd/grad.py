"""
Differentiable RapidMuskingum routing: torch autograd through the HIP engine.

    import river_route_amd as rr
    k = torch.tensor(k0, dtype=torch.float64, requires_grad=True)
    Q, q_final = rr.grad.rapid_route(plan, q0, qlateral, k, x, dt_routing=900.0, dt_runoff=3600.0)
    loss = ((Q[:, gauges] - observed) ** 2).mean()
    loss.backward()                     # k.grad: dL/dk of every reach, from one reverse sweep on the GPU

The forward is the production route call (rr_rapid_route_dev on torch's current stream), so the discharge is the one
Plan.rapid_route computes, bit for bit.  The backward is rr_rapid_adjoint_dev: it routes the forward again into a state tape and
runs the adjoint recurrence from the outlets upward and backward in time, then reduces the coefficient gradients per reach.
Torch chains from the coefficients to k and x (muskingum_coefficients), so any loss written in torch can sit on top.

RapidMuskingum only, float64 rows, one plan on one GPU: UnitMuskingum, float32 rows, ensembles and partitioned plans are refused.
"""
from __future__ import annotations

import numpy as np
import torch

from .engine import Plan

__all__ = ['muskingum_coefficients', 'RapidRoute', 'rapid_route']


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
        none = (None,) * 9
        if (grad_discharge is None and grad_qfinal is None) or not (want_q0 or want_ql or want_coef):
            return none
        dev = plan.device
        c1, c2, c3, c4dt = ctx.coeffs
        _set_coeffs(plan, c1, c2, c3, c4dt if qlateral is not None else None, dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        device = q0.device
        f64 = dict(dtype=torch.float64, device=device)
        g_out = None if grad_discharge is None else grad_discharge.to(**f64).contiguous()
        g_fin = None if grad_qfinal is None else grad_qfinal.to(**f64).contiguous()
        g_ql = torch.empty((T, plan.n), **f64) if want_ql else None
        g_q0 = torch.empty(plan.n, **f64) if want_q0 else None
        g_coef = torch.empty((4, plan.n), **f64) if want_coef else None
        nbytes = plan.rapid_adjoint_work_bytes(T, nsub)
        work = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=device)       # torch's allocator owns the tapes
        plan.rapid_adjoint_dev(q0.detach(), None if qlateral is None else qlateral.detach(), T, discharge, g_out, g_fin, g_ql, g_q0,
                               g_coef, work, nbytes, T, nsub, stream)
        coef = [None] * 4
        if g_coef is not None:
            for j, c in enumerate((c1, c2, c3, c4dt)):
                if need[5 + j] and c is not None:
                    coef[j] = g_coef[j].to(c.device)
        return (None, None, None, g_q0, g_ql, *coef)


def _check_tensor(t, name, shape):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f'{name} must be a torch tensor')
    if t.dtype != torch.float64:
        raise TypeError(f'{name} must be float64 (the adjoint has no float32 rows)')
    if tuple(t.shape) != shape:
        raise ValueError(f'{name} has shape {tuple(t.shape)}, expected {shape}')
    if not t.is_contiguous():
        raise ValueError(f'{name} must be contiguous')


def rapid_route(plan, q0, qlateral, k, x, dt_routing, dt_runoff, rows_per_window=None, rows=None):
    """Differentiable RapidMuskingum routing: (discharge[T, n], q_final[n]) as torch tensors on the plan's device.

    q0[n] and qlateral[T, n] are float64 tensors on the plan's GPU (qlateral in the reference's volume units per runoff step;
    None routes channel-only, and then `rows` gives T); k and x are float64 tensors of n values on any device.  c1, c2, c3 come
    from muskingum_coefficients(k, x, dt_routing) and c4dt = (c1 + c2) / dt_runoff; dt_runoff must be a whole number of routing
    steps.  Gradients reach q0, qlateral, k and x (whichever require grad).  rows_per_window routes the series in windows chained
    through q_final -> q0, so the tape memory of the backward pass is one window's.  Every argument is checked before the GPU is
    touched."""
    if not isinstance(plan, Plan):
        raise TypeError('plan must be a river_route_amd.engine.Plan (one GPU; partitioned plans have no adjoint)')
    n = plan.n
    if not (float(dt_routing) > 0 and float(dt_runoff) > 0):
        raise ValueError('dt_routing and dt_runoff must be positive')
    nsub = int(round(float(dt_runoff) / float(dt_routing)))
    if nsub < 1 or nsub * float(dt_routing) != float(dt_runoff):
        raise ValueError(f'dt_runoff ({dt_runoff}) must be a whole number of routing steps ({dt_routing})')
    _check_tensor(q0, 'q0', (n,))
    if qlateral is None:
        if rows is None or int(rows) < 1:
            raise ValueError('channel-only routing (qlateral=None) needs rows >= 1')
        T = int(rows)
    else:
        if not isinstance(qlateral, torch.Tensor) or qlateral.ndim != 2:
            raise ValueError('qlateral must be a 2-D (T, n) tensor (ensembles have no adjoint: route members one by one)')
        T = int(qlateral.shape[0])
        if T < 1:
            raise ValueError('qlateral has no rows')
        _check_tensor(qlateral, 'qlateral', (T, n))
    for t, name in ((k, 'k'), (x, 'x')):
        _check_tensor(t, name, (n,))
    if rows_per_window is not None and int(rows_per_window) < 1:
        raise ValueError('rows_per_window must be >= 1')
    if plan.device < 0:
        raise ValueError('plan is host-only (RR_DEVICE_NONE): the adjoint runs on the GPU only')
    for t, name in ((q0, 'q0'), (qlateral, 'qlateral')):
        if t is not None and (t.device.type != 'cuda' or t.device.index != plan.device):
            raise ValueError(f"{name} must be on cuda:{plan.device}, the plan's device (it is on {t.device})")

    c1, c2, c3 = muskingum_coefficients(k, x, float(dt_routing))
    c4dt = (c1 + c2) / float(dt_runoff)
    R = T if rows_per_window is None else min(T, int(rows_per_window))
    q, parts = q0, []
    for t0 in range(0, T, R):
        t1 = min(T, t0 + R)
        ql = None if qlateral is None else qlateral[t0:t1]
        d, q = RapidRoute.apply(plan, nsub, t1 - t0, q, ql, c1, c2, c3, c4dt)
        parts.append(d)
    return (parts[0] if len(parts) == 1 else torch.cat(parts, 0)), q
