"""The batched solve as a differentiable torch operation.

``solve(ctx, x_in, x_lin, x_ref, pf, C, mu=None) -> (u, x)`` runs
``Context.solve_device`` in fp64 and, under ``loss.backward()``, one
``Context.vjp_device`` call (hmpc_vjp_batch): the gradients with
respect to x_in, x_ref and pf at the solution's active set.  x_lin, C and mu are
held fixed (their gradient is None).  Both passes are HIP kernels on the current
stream; there is no CPU or eager fallback.
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
        want = tuple(k for k, need in zip(('x_in', 'x_ref', 'pf'), (fctx.needs_input_grad[i] for i in (1, 3, 4)))
                     if need)
        if not want:
            return (None,) * 7
        g = fctx.hmpc.vjp_device(x_in, x_lin, x_ref, pf, C, u, x,
                                 g_u=None if g_u is None else g_u.contiguous(),
                                 g_x=None if g_x is None else g_x.contiguous(), mu=mu, want=want)
        return None, g['x_in'], None, g['x_ref'], g['pf'], None, None


def solve(ctx, x_in, x_lin, x_ref, pf, C, mu=None):
    """(u*, x*) of the batch, differentiable with respect to x_in, x_ref and pf.
    Raises HmpcError if any instance's status is not HMPC_SOLVED."""
    return _Solve.apply(ctx, x_in, x_lin, x_ref, pf, C, mu)
