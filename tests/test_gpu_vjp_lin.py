"""hmpc_vjp_lin_batch / Context.vjp_lin_device / hmpc_autograd.mpcontrol: the gradients of the
solve in x_lin (position 0:3 and yaw 5 of rows 0..N-1) and mu on the device against a dense
float64 reference, tests/test_gpu_vjp.py's: the Jacobian d z*/d theta at the held rows (SVD of
the rows + reduced Hessian; second route: lstsq on the full KKT matrix), then J' g.  Per column
c = dE'lam, D = -dE z with dE from the oracle's own matrices: exact one-unit differences in
position and mu (affine), the five-point central difference in yaw with h = 2e-4 (Ad, Bd are
trigonometric polynomials of degree <= 5 in the yaw: truncation h^4/30 5^5 = 1.7e-13 relative,
rounding 1.5 eps / h = 1.7e-12).

Inputs, cases and class bounds (TOL) are tests/test_gpu_vjp.py's; a case asserts
max(class bound, the two routes' disagreement in that case) on
max |gpu - ref| / max(1, max |ref|) per instance and output.  The reference builder asserts that
the cases are not empty: a held friction row and a non-zero grad_mu in every `mu` instance, a live
z row in `ride` and in `drop` for N >= 3 (N <= 2 has no stage that could hold one).  Worst values
of the first run (MI355X):
  class     x_lin        mu           ref vs ref   bound
  noz       7.349e-11    2.105e-10    2.455e-10    1.434e-09   (x_lin: 3f mu; mu: 3f plain)
  z2        4.549e-11    1.639e-15    9.081e-11    4.586e-10   (3f, N = 10 drop; grad_mu is 0 there)
  ride      5.673e-10    8.183e-12    6.204e-10    4.373e-09   (3f)
  mpcontrol 3.382e-12 (x_in, init) / 2.365e-11 (x_prev), bound 4.586e-10
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip('torch')

from test_gpu_kkt import mpc_params   # noqa: E402
from test_gpu_vjp import CASES, IDS, IDX, TOL, ctx_for, reference as vjp_reference   # noqa: E402

pytestmark = pytest.mark.gpu

H = 2e-4   # yaw step of the five-point difference
OUTS = ('x_lin', 'mu')
COLS = (0, 1, 2, 5)   # the entries of an x_lin row gen_dt_dynamics reads


def held_rows(qp, z, skip, tol=1e-8):
    A, l, u = qp['A'], qp['l'], qp['u']
    Az = A @ z
    act = l == u
    for bnd, slack in ((l, Az - l), (u, u - Az)):
        fin = np.isfinite(bnd)
        act |= fin & (np.where(fin, slack, 1.0) <= tol * (1 + np.abs(np.where(fin, bnd, 0.0))))
    act[list(skip)] = False
    return act


def dense_jac_lin(qp, N, z, act, dAd, dBd, dA_mu, route):
    """d z*/d (x_lin[k][0,1,2,5] for k < N, mu, x_in), [nz, 4 N + 13]: min 1/2 dz'P dz + c'dz s.t.
    E dz = D over the held rows E, with c = dE'lam and D = -dE z per column (x_in: D alone)."""
    P, E = qp['P'], qp['A'][act]
    nx, nz, m = (N + 1) * 12, len(z), E.shape[0]
    lam = np.linalg.lstsq(E.T, -(P @ z + qp['q']), rcond=None)[0]
    dyn = np.flatnonzero(np.count_nonzero(E[:, :nx], axis=1) >= 2).reshape(N, 12)   # the dynamics rows
    c, D = np.zeros((nz, 4 * N + 13)), np.zeros((m, 4 * N + 13))
    D[m - 12:, 4 * N + 1:] = np.eye(12)   # the x[0] == x_in rows
    for k in range(N):   # the rows are x[k+1] - Ad x[k] - Bd u[k] = Gd
        xs, us = slice(12 * k, 12 * k + 12), slice(nx + 6 * k, nx + 6 * k + 6)
        for j in range(4):
            c[xs, 4 * k + j] = -dAd[j][k].T @ lam[dyn[k]]
            c[us, 4 * k + j] = -dBd[j][k].T @ lam[dyn[k]]
            D[dyn[k], 4 * k + j] = dAd[j][k] @ z[xs] + dBd[j][k] @ z[us]
    c[:, 4 * N], D[:, 4 * N] = dA_mu[act].T @ lam, -dA_mu[act] @ z
    if route == 'svd':
        U, s, Vt = np.linalg.svd(E)
        r = int((s > 1e-10 * s[0]).sum())
        dzp = Vt[:r].T @ ((U[:, :r].T @ D) / s[:r, None])
        Z = Vt[r:].T
        return dzp - Z @ np.linalg.solve(Z.T @ P @ Z, Z.T @ (P @ dzp + c))
    kkt = np.block([[P, E.T], [E, np.zeros((m, m))]])
    return np.linalg.lstsq(kkt, np.vstack([-c, D]), rcond=1e-13)[0][:nz]


def instance_jac(variant, N, inst, i, x, u, route, x_lin=None, consts=None):
    """(J [nz, 4 N + 13], the number of held friction rows) of instance i at the primal (x, u)"""
    from oracle import hmpc_oracle as ho
    p = mpc_params(variant, N, float(inst['mu'][i]), consts)
    Gd = ho.constant_matrices(p)[2]
    dyn = lambda xl: ho.gen_dt_dynamics(p, xl, inst['pf'][i])   # noqa: E731
    qp_of = lambda q, AB: ho.build_qp(q, inst['x_in'][i], inst['x_ref'][i], *AB, Gd, inst['C'][i], 'per_stage')   # noqa: E731
    x_lin = inst['x_lin'][i] if x_lin is None else x_lin
    AB = dyn(x_lin)
    qp, z = qp_of(p, AB), np.concatenate([x.ravel(), u.ravel()])
    skip = ()   # the z row of stage 1 is fixed by x_0: active, it is dependent and dropped
    if N > 1 and x[1, 2] - 0.1 <= 1.1e-8:
        skip = [r for r in range(len(qp['l'])) if qp['l'][r] == 0.1 and qp['A'][r, 14] == 1.0]
    act = held_rows(qp, z, skip)
    e = lambda j, s: s * np.eye(12)[COLS[j]]   # noqa: E731
    dAd, dBd = [], []
    for j in range(4):
        if j < 3:
            d = [a1 - a0 for a1, a0 in zip(dyn(x_lin + e(j, 1.0)), AB)]
        else:
            m2, m1, p1, p2 = (dyn(x_lin + e(j, s * H)) for s in (-2, -1, 1, 2))
            d = [(a - 8 * b + 8 * c - dd) / (12 * H) for a, b, c, dd in zip(m2, m1, p1, p2)]
        dAd.append(d[0])
        dBd.append(d[1])
    dA_mu = qp_of(mpc_params(variant, N, float(inst['mu'][i]) + 1.0, consts), AB)['A'] - qp['A']
    return dense_jac_lin(qp, N, z, act, dAd, dBd, dA_mu, route), int(np.any(dA_mu[act] != 0, axis=1).sum())


@functools.lru_cache(maxsize=None)
def reference(variant, N, idx, mode, consts=None):
    """test_gpu_vjp's inputs, primal and cotangents, plus (route) -> per-instance dicts of the
    reference grad_x_lin [N+1,12] and grad_mu, and the per-instance count of held friction rows."""
    inst, ref = vjp_reference(variant, N, idx, mode, consts)
    lin = dict(fric=[])
    for i in range(len(idx)):
        g = np.concatenate([ref['g_x'][i].ravel(), ref['g_u'][i].ravel()])
        for route in ('svd', 'kkt'):
            J, nf = instance_jac(variant, N, inst, i, ref['x'][i], ref['u'][i], route, consts=consts)
            grad, gl = J.T @ g, np.zeros((N + 1, 12))
            gl[:N, COLS] = grad[:4 * N].reshape(N, 4)
            lin.setdefault(route, []).append(dict(x_lin=gl, mu=grad[4 * N:4 * N + 1]))
        lin['fric'].append(nf)
    live = (ref['x'][:, 2:N, 2] - 0.1 <= 1.1e-8).sum(axis=1)   # the z row of stage 1 is never live
    if mode == 'mu':
        assert min(lin['fric']) >= 1 and min(abs(r['mu'][0]) for r in lin['svd']) > 0.0
    if mode == 'ride' or (mode == 'drop' and N >= 3):   # N <= 2 has no stage that could hold a live row
        assert live.max() >= 1
    return inst, ref, lin


def figure(got, ref, outs=OUTS):
    return {o: max(np.abs(got[o][i] - r[o]).max() / max(1.0, np.abs(r[o]).max()) for i, r in enumerate(ref))
            for o in outs}


def bound(ref, lin):
    cls = 'ride' if ref['zrows'].max() > 2 else ('z2' if ref['zrows'].max() > 0 else 'noz')
    d_ref = max(figure({o: [a[o] for a in lin['kkt']] for o in OUTS}, lin['svd']).values())
    return cls, d_ref, max(TOL[cls], d_ref)


def run(ctx, inst, ref, reps=1, fn='vjp_lin_device', **kw):
    dev = {k: torch.from_numpy(np.ascontiguousarray(np.concatenate([v] * reps))).cuda()
           for k, v in dict(inst, u=ref['u'], x=ref['x'], g_u=ref['g_u'], g_x=ref['g_x']).items()}
    args = [dev[k] for k in ('x_in', 'x_lin', 'x_ref', 'pf', 'C', 'u', 'x')]
    if kw.pop('multipliers', False):
        kkt = ctx.kkt_device(*args, mu=dev['mu'])
        kw.update(nu=kkt['nu'], lam=kkt['lam'])
    out = getattr(ctx, fn)(*args, g_u=dev['g_u'], g_x=dev['g_x'], mu=dev['mu'], **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items() if v is not None}


@pytest.mark.parametrize('variant,N,idx,mode', CASES, ids=IDS)
def test_gradients_at_the_exact_primal(variant, N, idx, mode, consts=None):
    inst, ref, lin = reference(variant, N, idx, mode, consts)
    ctx = ctx_for(variant, N, consts)
    got, old = run(ctx, inst, ref), run(ctx, inst, ref, fn='vjp_device')
    assert all(np.array_equal(got[o], old[o]) for o in ('x_in', 'x_ref', 'pf', 'flags'))   # bit for bit
    assert np.array_equal(got['flags'] != 0, ref['singular'])
    assert got['x_lin'].shape == (len(idx), N + 1, 12) and got['mu'].shape == (len(idx),)
    dead = np.ones((N + 1, 12), bool)
    dead[:N, COLS] = False
    assert not got['x_lin'][:, dead].any()   # exactly 0.0 where gen_dt_dynamics reads nothing
    cls, d_ref, tol = bound(ref, lin)
    d = figure(dict(got, mu=got['mu'][:, None]), lin['svd'])
    print(f'LIN1 {variant} N={N} {mode} {cls} zrows={ref["zrows"]} fric={lin["fric"]} x_lin={d["x_lin"]:.3e} '
          f'mu={d["mu"]:.3e} refs={d_ref:.3e}')
    assert max(d.values()) <= tol


def test_partial_outputs_multipliers_and_the_launch_grid():
    inst, ref, lin = reference('3f', 3, IDX['3f'], 'drop')
    ctx = ctx_for('3f', 3)
    full, part = run(ctx, inst, ref), run(ctx, inst, ref, want=('x_lin',))
    assert set(part) == {'x_lin', 'flags'} and np.array_equal(part['x_lin'], full['x_lin'])
    given = run(ctx, inst, ref, multipliers=True)   # nu, lam from kkt_device by the caller
    assert all(np.array_equal(given[o], full[o]) for o in full)
    big = run(ctx, inst, ref, reps=343)   # B = 1029 > 1024 workgroups
    assert not big['flags'].any()
    assert all(np.array_equal(big[o][-3:], big[o][:3]) and np.array_equal(big[o][:3], full[o]) for o in full)


def mpcontrol_chain(variant, N, inst, i, g_u, consts=None):
    """Dense chain rule through Mpc.mpcontrol for the loss sum(g_u u): d/d x_in of the init call,
    d/d x_prev of a non-init call on x_prev = the init call's first solution; and that x_prev."""
    from oracle import hmpc_oracle as ho
    p = mpc_params(variant, N, float(inst['mu'][i]), consts)
    g = np.concatenate([np.zeros((N + 1) * 12), g_u.ravel()])

    def back(x_lin, g):   # the solve at x_lin: its x*, grad_x_lin [N+1,12] and grad_x_in of the cotangent g
        s = ho.solve_instance(p, inst['x_in'][i], x_lin, inst['x_ref'][i], inst['pf'][i], inst['C'][i], 'per_stage')
        assert s['status'] == 'solved'
        t = instance_jac(variant, N, inst, i, s['x'], s['u'], 'svd', x_lin=x_lin, consts=consts)[0].T @ g
        gl = np.zeros((N + 1, 12))
        gl[:N, COLS] = t[:4 * N].reshape(N, 4)
        return s['x'], gl, t[4 * N + 1:]

    x1 = back(np.vstack([inst['x_in'][i][None], inst['x_ref'][i]]), g)[0]
    _, gl2, gin2 = back(x1, g)   # the second solve is linearised at the first's x*
    _, gl1, gin1 = back(np.vstack([inst['x_in'][i][None], inst['x_ref'][i]]), np.concatenate([gl2.ravel(), 0 * g_u.ravel()]))
    _, gl3, _ = back(np.vstack([inst['x_in'][i][None], x1[2:], x1[-1:]]), g)
    g_prev = np.zeros((N + 1, 12))
    g_prev[2:] = gl3[1:N]   # x_lin[1:N] = x_prev[2:]; row N of x_lin is never read
    return gin2 + gin1 + gl1[0], g_prev, x1


@pytest.mark.parametrize('variant', ('3f', '2f'))
def test_mpcontrol(variant):
    import hmpc_autograd
    N = 3
    inst, ref, lin = reference(variant, N, IDX[variant], 'drop')
    tol = bound(ref, lin)[2]
    chains = [mpcontrol_chain(variant, N, inst, i, ref['g_u'][i]) for i in range(3)]
    dev = {k: torch.from_numpy(v).cuda() for k, v in dict(inst, g_u=ref['g_u']).items()}
    x_prev = torch.from_numpy(np.array([c[2] for c in chains])).cuda()
    for init, wrt, want in ((True, dev['x_in'], [c[0] for c in chains]), (False, x_prev, [c[1] for c in chains])):
        wrt.requires_grad_(True)
        u, x = hmpc_autograd.mpcontrol(ctx_for(variant, N), dev['x_in'], dev['x_ref'], dev['pf'], dev['C'],
                                       x_prev=x_prev, init=init, mu=dev['mu'])
        xp = x_prev.detach().clone()
        out = ctx_for(variant, N).mpcontrol_device(init, dev['x_in'].detach(), dev['x_ref'], dev['pf'], dev['C'], xp,
                                                   mu=dev['mu'])
        assert torch.equal(out['u'], u) and torch.equal(xp, x)   # a context that has run no other solve
        (grad,) = torch.autograd.grad((u * dev['g_u']).sum(), wrt)
        wrt.requires_grad_(False)
        d = max(np.abs(grad[i].cpu().numpy() - w).max() / max(1.0, np.abs(w).max()) for i, w in enumerate(want))
        print(f'LIN3 {variant} init={init} gpu={d:.3e} tol={tol:.3e}')
        assert d <= tol
        # the term through x_lin is live: solve with x_lin detached gives x_prev no gradient at all, and x_in another
        g0 = torch.zeros_like(grad)
        if init:
            xi = dev['x_in'].clone().requires_grad_(True)
            x1 = hmpc_autograd.solve(ctx_for(variant, N), xi, torch.cat([xi[:, None], dev['x_ref']], 1), dev['x_ref'],
                                     dev['pf'], dev['C'], mu=dev['mu'])[1].detach()
            u0, _ = hmpc_autograd.solve(ctx_for(variant, N), xi, x1, dev['x_ref'], dev['pf'], dev['C'], mu=dev['mu'])
            (g0,) = torch.autograd.grad((u0 * dev['g_u']).sum(), xi)
        assert (g0 - grad).abs().max() > 1e3 * tol


def test_arguments():
    import hmpc
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device='cuda')   # noqa: E731
    args = lambda N: (z(1, 12), z(1, N + 1, 12), z(1, N, 12), z(1, N, 3), z(1, N), z(1, N, 6),   # noqa: E731
                      z(1, N + 1, 12), z(1, N, 6), z(1, N + 1, 12))
    mult = lambda N: dict(nu=z(1, N), lam=z(1, N, 11))   # noqa: E731
    with pytest.raises(hmpc.HmpcError, match='hmpc_vjp_lin_batch failed: HMPC_ERR_UNSUPPORTED'):
        ctx_for('3f', 65).vjp_lin_device(*args(65), **mult(65))
    with pytest.raises(hmpc.HmpcError, match='hmpc_vjp_lin_batch failed: HMPC_ERR_UNSUPPORTED'):
        ctx_for('cas', 10).vjp_lin_device(*args(10), **mult(10))
    ctx = ctx_for('3f', 10)
    with pytest.raises(hmpc.HmpcError, match='HMPC_ERR_ARG'):
        ctx.vjp_lin_device(*args(10)[:7], **mult(10))   # both cotangents NULL
    with pytest.raises(hmpc.HmpcError, match='HMPC_ERR_ARG'):
        ctx.vjp_lin_device(*args(10), want=(), **mult(10))   # all five outputs NULL
    a = args(10)
    ptr = [t.data_ptr() for t in a[:5]] + [None] + [t.data_ptr() for t in a[5:7]]
    tail = [a[7].data_ptr(), a[8].data_ptr(), None, None, None, z(1, 11, 12).data_ptr(), None, None, None]
    for nu, lam in ((None, z(1, 10, 11).data_ptr()), (z(1, 10).data_ptr(), None)):   # a missing multiplier
        assert ctx._lib.hmpc_vjp_lin_batch(ctx._h, 1, *ptr, 1e-8, nu, lam, *tail) == -1
