"""hmpc_vjp_batch / Context.vjp_device / hmpc_autograd.solve: the reverse-mode
gradients (d z*/d theta)' g for theta = x_in, x_ref, pf on the device against a
dense float64 reference: the full Jacobian d z*/d theta at the active set (SVD of
the active rows + reduced Hessian; dA/dpf exact, A being affine in pf), then J' g.

Inputs and modes: the recipe of tests/test_gpu_sens.py (plain, drop, ride, mu,
stage1); cotangents are seeded standard normals.

Figure: max |gpu - ref| / max(1, max |ref|) per instance and output.  Worst values
of the first run (MI355X), next to the disagreement of the
reference's two routes (SVD / lstsq on the full KKT matrix); a case asserts
max(10 x its class's GPU figure, the two routes' disagreement in that case):
  class     gpu vs ref   ref vs ref
  noz       1.434e-10    1.783e-07   (no active z row; worst: 2f, N = 10, mu; lstsq's worst: 2f, N = 1)
  z2        4.586e-11    5.190e-10   (at most two live z rows; the stage1 case, the partial
                                      cotangents and autograd included)
  ride      4.373e-10    2.121e-09   (N = 64, up to 19 z rows; worst: 3f)
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip('torch')

from test_gpu_kkt import ctx_for as kkt_ctx_for, mpc_params, windows   # noqa: E402

pytestmark = pytest.mark.gpu

TOL = {'noz': 1.434e-9, 'z2': 4.586e-10, 'ride': 4.373e-9}   # 10 x the class's GPU figure
IDX = {'3f': (0, 5, 8), '2f': (0, 7, 15)}   # golden windows the oracle solves in every mode used
CASES = [(v, N, IDX[v], 'drop') for v in ('3f', '2f') for N in (1, 2, 3, 10)]
CASES += [(v, 10, IDX[v], 'plain') for v in ('3f', '2f')]
CASES += [('3f', 10, (5, 11, 5), 'mu'), ('2f', 10, (10, 15, 10), 'mu')]
CASES += [(v, 64, (4, 6, 7), 'ride') for v in ('3f', '2f')]
CASES += [('3f', 2, IDX['3f'], 'stage1')]
IDS = ['-'.join(map(str, (c[0], c[1], c[3]))) for c in CASES]
OUTS = ('x_in', 'x_ref', 'pf')
MODES = {'plain': (None,) * 3, 'mu': (None,) * 3, 'drop': (0.14, -1.0, 0.05), 'drop6': (0.14, -0.6, 0.05), 'ride': (0.104, -0.1, -2.0),
         'stage1': (0.102, -0.1, 0.05)}   # x_in z, vz and the z reference


def ctx_for(variant, N, consts=None):
    return kkt_ctx_for(variant, N, 'per_stage', consts)


def dense_jac(qp, N, z, skip, dB, route, tol=1e-8):
    """d z*/d (x_in, x_ref, pf), [nz, 12 + 15 N]: min 1/2 dz'P dz + c'dz s.t. E dz = D over the
    equality and active rows E, with c = dq + dE'lam and D = dd - dE z per column."""
    A, P, l, u = qp['A'], qp['P'], qp['l'], qp['u']
    Az = A @ z
    act = l == u
    for bnd, slack in ((l, Az - l), (u, u - Az)):
        fin = np.isfinite(bnd)
        act |= fin & (np.where(fin, slack, 1.0) <= tol * (1 + np.abs(np.where(fin, bnd, 0.0))))
    act[list(skip)] = False
    E = A[act]
    nx, nz, m = (N + 1) * 12, len(z), E.shape[0]
    lam = np.linalg.lstsq(E.T, -(P @ z + qp['q']), rcond=None)[0]
    dyn = np.flatnonzero(np.count_nonzero(E[:, :nx], axis=1) >= 2).reshape(N, 12)   # the dynamics rows
    c, D = np.zeros((nz, 12 + 15 * N)), np.zeros((m, 12 + 15 * N))
    D[m - 12:, :12] = np.eye(12)   # x_in: the x[0] == x_in rows
    for k in range(N):
        xs, us = slice(12 * (k + 1), 12 * (k + 2)), slice(nx + 6 * k, nx + 6 * k + 6)
        c[xs, 12 + 12 * k:24 + 12 * k] = -P[xs, xs]   # x_ref: dq / dx_ref[k]
        for j in range(3):   # pf: the rows are x[k+1] - Ad x[k] - Bd u[k] = Gd
            c[us, 12 + 12 * N + 3 * k + j] = -dB[j][k].T @ lam[dyn[k]]
            D[dyn[k], 12 + 12 * N + 3 * k + j] = dB[j][k] @ z[us]
    if route == 'svd':
        U, s, Vt = np.linalg.svd(E)
        r = int((s > 1e-10 * s[0]).sum())
        dzp = Vt[:r].T @ ((U[:, :r].T @ D) / s[:r, None])
        Z = Vt[r:].T
        return dzp - Z @ np.linalg.solve(Z.T @ P @ Z, Z.T @ (P @ dzp + c))
    kkt = np.block([[P, E.T], [E, np.zeros((m, m))]])
    return np.linalg.lstsq(kkt, np.vstack([-c, D]), rcond=1e-13)[0][:nz]


def split(grad, N):
    return dict(x_in=grad[:12], x_ref=grad[12:12 + 12 * N].reshape(N, 12), pf=grad[12 + 12 * N:].reshape(N, 3))


@functools.lru_cache(maxsize=None)
def reference(variant, N, idx, mode, consts=None):
    """Inputs [B, ...], the oracle's primal, the cotangents, the gradients by both routes for
    (g_u, g_x), (g_u, 0) and (0, g_x), the instances expected singular and the z-row counts."""
    from oracle import hmpc_oracle as ho
    inst = windows(variant, N, idx)
    inst['x_lin'] = inst['x_lin'][:, :N + 1]
    for k in ('x_ref', 'pf', 'C'):
        inst[k] = np.ascontiguousarray(inst[k][:, :N])
    if mode == 'mu':
        inst['mu'][:] = (0.5, 0.7, 0.9)
    z0, vz, zref = MODES[mode]
    if z0 is not None:
        inst['x_in'][:, 2], inst['x_in'][:, 8] = z0, vz
        inst['x_ref'][:, :, 2] = zref
    if mode == 'ride':
        inst['C'][:] = 1.0
    inst['x_lin'][:, 0] = inst['x_in']
    rng = np.random.default_rng(len(idx) * 1000 + N)
    ref = dict(u=[], x=[], g_u=rng.standard_normal((len(idx), N, 6)), g_x=rng.standard_normal((len(idx), N + 1, 12)))
    for i in range(len(idx)):
        p = mpc_params(variant, N, float(inst['mu'][i]), consts)
        s = ho.solve_instance(p, inst['x_in'][i], inst['x_lin'][i], inst['x_ref'][i], inst['pf'][i],
                              inst['C'][i], 'per_stage')
        assert s['status'] == 'solved', (variant, N, idx[i], mode)
        qp, z = s['qp'], np.concatenate([s['x'].ravel(), s['u'].ravel()])
        skip = ()   # the z row of stage 1 is fixed by x_0: active, it is dependent and dropped
        if N > 1 and s['x'][1, 2] - 0.1 <= 1.1e-8:
            skip = [r for r in range(len(qp['l'])) if qp['l'][r] == 0.1 and qp['A'][r, 14] == 1.0]
        dB = [ho.gen_dt_dynamics(p, inst['x_lin'][i], inst['pf'][i] + np.eye(3)[j])[1] - s['Bd'] for j in range(3)]
        gx, gu = ref['g_x'][i].ravel(), ref['g_u'][i].ravel()
        ref['u'].append(s['u'])
        ref['x'].append(s['x'])
        for route in ('svd', 'kkt'):
            J = dense_jac(qp, N, z, skip, dB, route)
            for key, g in (('full', np.concatenate([gx, gu])), ('gu', np.concatenate([0 * gx, gu])),
                           ('gx', np.concatenate([gx, 0 * gu]))):
                ref.setdefault((route, key), []).append(split(J.T @ g, N))
    ref['u'], ref['x'] = np.array(ref['u']), np.array(ref['x'])
    ref['singular'] = ref['x'][:, 1, 2] - 0.1 <= 1.1e-8 if N > 1 else np.zeros(len(idx), bool)
    ref['zrows'] = (ref['x'][:, 1:N, 2] - 0.1 <= 1.1e-8).sum(axis=1)
    return inst, ref


def figure(got, ref):
    """got: dict of [B, ...] arrays; ref: list of per-instance dicts"""
    return max(np.abs(got[o][i] - r[o]).max() / max(1.0, np.abs(r[o]).max())
               for i, r in enumerate(ref) for o in OUTS if o in got)


def run_vjp(ctx, inst, ref, g_u=True, g_x=True, reps=1, **kw):
    dev = {k: torch.from_numpy(np.ascontiguousarray(np.concatenate([v] * reps))).cuda()
           for k, v in dict(inst, u=ref['u'], x=ref['x'], g_u=ref['g_u'], g_x=ref['g_x']).items()}
    out = ctx.vjp_device(dev['x_in'], dev['x_lin'], dev['x_ref'], dev['pf'], dev['C'], dev['u'], dev['x'],
                         g_u=dev['g_u'] if g_u else None, g_x=dev['g_x'] if g_x else None, mu=dev['mu'], **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items() if v is not None}


def bound(ref, key='full'):
    cls = 'ride' if ref['zrows'].max() > 2 else ('z2' if ref['zrows'].max() > 0 else 'noz')
    d_ref = max(np.abs(a[o] - r[o]).max() / max(1.0, np.abs(r[o]).max())
                for a, r in zip(ref['kkt', key], ref['svd', key]) for o in OUTS)
    return cls, d_ref, max(TOL[cls], d_ref)


@pytest.mark.parametrize('variant,N,idx,mode', CASES, ids=IDS)
def test_gradients_at_the_exact_primal(variant, N, idx, mode, consts=None):
    inst, ref = reference(variant, N, idx, mode, consts)
    got = run_vjp(ctx_for(variant, N, consts), inst, ref)
    assert got['x_in'].shape == (len(idx), 12) and got['x_ref'].shape == (len(idx), N, 12)
    assert got['pf'].shape == (len(idx), N, 3)
    assert np.array_equal(got['flags'] != 0, ref['singular'])   # stage1: exactly the predicted instances
    cls, d_ref, tol = bound(ref)
    d = figure(got, ref['svd', 'full'])
    print(f'VJP1 {variant} N={N} {mode} {cls} zrows={ref["zrows"]} gpu={d:.3e} refs={d_ref:.3e}')
    assert d <= tol


def test_partial_cotangents_and_outputs():
    inst, ref = reference('2f', 10, IDX['2f'], 'drop')
    ctx = ctx_for('2f', 10)
    for key, kw in (('gu', dict(g_x=False)), ('gx', dict(g_u=False))):
        d = figure(run_vjp(ctx, inst, ref, **kw), ref['svd', key])
        print(f'VJP2 {key} gpu={d:.3e}')
        assert d <= bound(ref, key)[2]
    full, part = run_vjp(ctx, inst, ref), run_vjp(ctx, inst, ref, want=('x_ref',))
    assert set(part) == {'x_ref', 'flags'} and np.array_equal(part['x_ref'], full['x_ref'])


def test_batch_above_the_launch_grid():
    inst, ref = reference('3f', 3, IDX['3f'], 'drop')
    got = run_vjp(ctx_for('3f', 3), inst, ref, reps=343)   # B = 1029 > 1024 workgroups
    assert not got['flags'].any()
    assert figure(got, ref['svd', 'full'] * 343) <= bound(ref)[2]
    assert all(np.array_equal(got[o][-3:], got[o][:3]) for o in OUTS)


@pytest.mark.parametrize('variant', ('3f', '2f'))
def test_autograd_end_to_end(variant):
    import hmpc_autograd
    inst, ref = reference(variant, 10, IDX[variant], 'drop')
    dev = {k: torch.from_numpy(v).cuda() for k, v in dict(inst, g_u=ref['g_u'], g_x=ref['g_x']).items()}
    dev['x_ref'].requires_grad_(True)
    dev['pf'].requires_grad_(True)
    u, x = hmpc_autograd.solve(ctx_for(variant, 10), dev['x_in'], dev['x_lin'], dev['x_ref'], dev['pf'], dev['C'],
                               mu=dev['mu'])
    ((u * dev['g_u']).sum() + (x * dev['g_x']).sum()).backward()
    assert dev['x_in'].grad is None
    d = figure(dict(x_ref=dev['x_ref'].grad.cpu().numpy(), pf=dev['pf'].grad.cpu().numpy()), ref['svd', 'full'])
    print(f'VJP3 {variant} gpu={d:.3e}')
    assert d <= bound(ref)[2]


def test_arguments():
    import hmpc
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device='cuda')   # noqa: E731
    args = lambda N: (z(1, 12), z(1, N + 1, 12), z(1, N, 12), z(1, N, 3), z(1, N), z(1, N, 6),   # noqa: E731
                      z(1, N + 1, 12), z(1, N, 6), z(1, N + 1, 12))
    with pytest.raises(hmpc.HmpcError, match='HMPC_ERR_UNSUPPORTED'):
        ctx_for('3f', 65).vjp_device(*args(65))
    with pytest.raises(hmpc.HmpcError, match='HMPC_ERR_UNSUPPORTED'):
        ctx_for('cas', 10).vjp_device(*args(10))
    ctx = ctx_for('3f', 10)
    with pytest.raises(hmpc.HmpcError, match='HMPC_ERR_ARG'):
        ctx.vjp_device(*args(10)[:7])   # both cotangents NULL
    with pytest.raises(hmpc.HmpcError, match='HMPC_ERR_ARG'):
        ctx.vjp_device(*args(10), want=())   # all three outputs NULL
