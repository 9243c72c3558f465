"""The batched solve and ``Mpc.mpcontrol`` as differentiable torch operations.

``solve(ctx, x_in, x_lin, x_ref, pf, C, mu=None) -> (u, x)`` runs
``Context.solve_device`` in fp64 and, under ``loss.backward()``, one adjoint
kernel at the solution's active set: ``Context.vjp_device`` (hmpc_vjp_batch,
DESIGN.md 4.9) for the gradients with respect to x_in, x_ref and pf, or, when
x_lin or mu requires a gradient, ``Context.kkt_device`` and
``Context.vjp_lin_device`` (hmpc_vjp_lin_batch), which returns
those two as well.  C is discrete (its gradient is None).

``mpcontrol(ctx, x_in, x_ref, pf, C, x_prev=None, init=False, mu=None) -> (u, x)``
is the reference's ``Mpc.mpcontrol`` around ``solve``: the linearisation point is
x_in in row 0 and the time-shifted previous solution (or, with ``init``, the
solution of a first solve linearised at the reference) below it, so the
gradients with respect to x_in, x_ref, pf, mu and x_prev include the terms
through x_lin.

``plant(ctx, X, U, pf, n_steps, dt, J) -> (X_next, x_out, X_hist)`` and
``convert(ctx, X) -> x`` are the Runner's plant (``n_steps`` of ``rk4_normalized``,
then ``convert``) and ``convert`` itself; their backward pass is one
``Context.plant_vjp_device`` call (hmpc_plant_vjp_batch).  With
them a Runner period, ``convert -> mpcontrol -> plant``, is differentiable end to
end: a loss on the closed-loop trajectory reaches x_ref, pf, mu and the start state.

All passes are HIP kernels on the current stream; there is no CPU or eager
fallback.
"""
from __future__ import annotations

import torch

import hmpc


class _Solve(torch.autograd.Function):
    @staticmethod
    def forward(fctx, ctx, x_in, x_lin, x_ref, pf, C, mu):
        out = ctx.solve_device(x_in, x_lin, x_ref, pf, C, mu=mu)
        bad = int((out['status'] != 0).sum())   # HMPC_SOLVED = 0; this waits for the solve
        if bad:
            raise hmpc.HmpcError(f'hmpc_autograd.solve: {bad} of {x_in.shape[0]} instances not HMPC_SOLVED')
        fctx.hmpc = ctx
        fctx.save_for_backward(x_in, x_lin, x_ref, pf, C, mu, out['u'], out['x'])
        return out['u'], out['x']

    @staticmethod
    def backward(fctx, g_u, g_x):
        x_in, x_lin, x_ref, pf, C, mu, u, x = fctx.saved_tensors
        names = ('x_in', 'x_lin', 'x_ref', 'pf', None, 'mu')   # forward's tensor arguments
        want = tuple(k for k, need in zip(names, fctx.needs_input_grad[1:]) if k and need)
        if not want:
            return (None,) * 7
        vjp = fctx.hmpc.vjp_lin_device if 'x_lin' in want or 'mu' in want else fctx.hmpc.vjp_device
        g = vjp(x_in, x_lin, x_ref, pf, C, u, x, g_u=None if g_u is None else g_u.contiguous(),
                g_x=None if g_x is None else g_x.contiguous(), mu=mu, want=want)
        return (None,) + tuple(g.get(k) if k else None for k in names)


class _Plant(torch.autograd.Function):
    @staticmethod
    def forward(fctx, ctx, X, U, pf, n_steps, dt, J):
        X0, U, pf = X.detach().contiguous(), U.detach().contiguous(), pf.detach().contiguous()
        Xn = X0.clone()   # plant_device steps its argument in place
        hist = torch.empty((X0.shape[0], n_steps, 13), dtype=torch.float64, device=X0.device)
        x_out = torch.empty((X0.shape[0], 12), dtype=torch.float64, device=X0.device)
        ctx.plant_device(Xn, U, 6, pf, 3 * n_steps, 3, n_steps, dt, J, X_hist=hist, x_out=x_out)
        fctx.hmpc, fctx.call = ctx, (n_steps, dt, J)
        fctx.save_for_backward(X0, hist, U, pf)
        return Xn, x_out, hist

    @staticmethod
    def backward(fctx, g_X, g_x_out, g_hist):
        X0, hist, U, pf = fctx.saved_tensors
        n_steps, dt, J = fctx.call
        want = tuple(k for k, need in zip(('X0', 'U', 'pf'), fctx.needs_input_grad[1:4]) if need)
        if not want:
            return (None,) * 7
        g = fctx.hmpc.plant_vjp_device(X0, hist, U, 6, pf, 3 * n_steps, 3, n_steps, dt, J,
                                       g_X=None if g_X is None else g_X.contiguous(),
                                       g_x_out=None if g_x_out is None else g_x_out.contiguous(),
                                       g_X_hist=None if g_hist is None else g_hist.contiguous(), want=want)
        return None, g['X0'], g['U'], g['pf'], None, None, None


class _Convert(torch.autograd.Function):
    @staticmethod
    def forward(fctx, ctx, X):
        X0 = X.detach().contiguous()
        x = torch.empty((X0.shape[0], 12), dtype=torch.float64, device=X0.device)
        ctx.convert_device(X0, x)
        fctx.hmpc = ctx
        fctx.save_for_backward(X0)
        return x

    @staticmethod
    def backward(fctx, g_x):
        (X0,) = fctx.saved_tensors
        # n_steps = 0: the adjoint of convert alone (U and pf are not read; any valid rows do)
        g = fctx.hmpc.plant_vjp_device(X0, None, X0, 13, X0, 13, 0, 0, 1.0, torch.eye(3).numpy(),
                                       g_x_out=g_x.contiguous(), want=('X0',))
        return None, g['X0']


def plant(ctx, X, U, pf, n_steps, dt, J):
    """(X_next, x_out, X_hist) of ``n_steps`` RK4 plant steps (src/robotrunner.py:126-164) from
    X (B,13) with the input U (B,6) held and the foot position pf (B,n_steps,3) per step:
    X_next (B,13), x_out = convert(X_next) (B,12) and every step's state X_hist (B,n_steps,13).
    X is left unchanged.  Differentiable with respect to X, U and pf (hmpc_plant_vjp_batch,
    DESIGN.md 4.11); pass ``u[:, 0]`` of ``mpcontrol`` as U and torch carries the gradient into u."""
    return _Plant.apply(ctx, X, U, pf, int(n_steps), float(dt), J)


def convert(ctx, X):
    """x (B,12) = convert(X (B,13)) (src/robotrunner.py:19-28), differentiable with respect to X
    away from the gimbal branch (the n_steps = 0 call of hmpc_plant_vjp_batch)."""
    return _Convert.apply(ctx, X)


def solve(ctx, x_in, x_lin, x_ref, pf, C, mu=None):
    """(u*, x*) of the batch, differentiable with respect to x_in, x_lin, x_ref, pf and mu.
    Raises HmpcError if any instance's status is not HMPC_SOLVED."""
    return _Solve.apply(ctx, x_in, x_lin, x_ref, pf, C, mu)


def mpcontrol(ctx, x_in, x_ref, pf, C, x_prev=None, init=False, mu=None):
    """(u*, x*) of ``Mpc.mpcontrol`` (src/mpc_cvx_euler_3f.py:41-69) for the batch.  init: a
    first solve linearised at (x_in; x_ref) gives the linearisation point of the second;
    otherwise it is (x_in; x_prev[2:]; x_prev[-1]), x_prev (B,N+1,12) being the previous
    call's x*.  Differentiable with respect to x_in, x_ref, pf, mu and x_prev."""
    if init:
        _, x_lin = solve(ctx, x_in, torch.cat([x_in[:, None], x_ref], 1), x_ref, pf, C, mu)
    else:
        x_lin = torch.cat([x_in[:, None], x_prev[:, 2:], x_prev[:, -1:]], 1)
    return solve(ctx, x_in, x_lin, x_ref, pf, C, mu)
