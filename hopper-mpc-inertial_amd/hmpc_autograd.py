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
