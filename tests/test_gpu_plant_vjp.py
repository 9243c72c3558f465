"""hmpc_plant_vjp_batch / Context.plant_vjp_device / hmpc_autograd.plant, convert: the adjoint of the plant
(n_steps of rk4_normalized, then convert) on the device against torch.autograd.grad of a CPU float64 restatement
of oracle/hmpc_plant.py (regular atan2 branch only), whose forward test_gradients pins to the oracle's own
functions at 1e-12 absolute.  Figure: max |gpu - ref| / max(1, max |ref|) per output; TOL is 10 x the worst of the
first run on an MI355X: grad_X0 7.993e-16 (n = 2), grad_U 5.496e-16, grad_pf 8.788e-16 (n = 20).
One period convert -> mpcontrol -> plant: 1.442e-12 (3f) / 1.321e-12 (2f), the MPC chain's bound 4.586e-10."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')

from test_gpu_kkt import constants   # noqa: E402
from test_gpu_vjp_lin import IDX, bound, ctx_for, mpcontrol_chain, reference   # noqa: E402

pytestmark = pytest.mark.gpu

DT = 1e-3
TOL = dict(X0=7.993e-15, U=5.496e-15, pf=8.788e-15)
CASES = [(0, 3, 'x', 'dense'), (1, 1, 'X', 'dense'), (1, 65, 'x', 'dense'), (2, 3, 'Xxh', 'dense'),
         (20, 130, 'Xxh', 'dense'), (3, 4, 'h', 'dense'), (3, 5, 'Xxh', 'shared')]


def consts(c=None):
    """m, g, J, Jinv, rh of the plant: the Runner's, or those of test_gpu_kkt.constants(c) with J = inv(Jinv)"""
    c = constants(c)
    return dict(c, J=c['J'] if 'J' in c else np.linalg.inv(c['Jinv']))


mv = lambda M, a: (M @ a[..., None])[..., 0]   # noqa: E731


def rot(q):
    w, x, y, z = q.unbind(-1)
    return torch.stack([w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y),
                        2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z], -1).reshape(-1, 3, 3)


def dynamics_ct(X, U, pf, c):
    p, q, v, w = X[:, 0:3], X[:, 3:7], X[:, 7:10], X[:, 10:13]
    J, rh = torch.from_numpy(c['J']), torch.from_numpy(np.asarray(c['rh'], float))
    R, Fw = rot(q), U[:, 0:3]
    Rt = R.transpose(1, 2)
    Ftb = mv(Rt, Fw + torch.tensor([0.0, 0.0, -c['g'] * c['m']], dtype=torch.float64))
    tautb = U[:, 3:6] + torch.cross(rh + mv(Rt, pf - p), mv(Rt, Fw), dim=1)
    w0, w1, w2 = w.unbind(1)
    dq = 0.5 * torch.stack([-q[:, 1] * w0 - q[:, 2] * w1 - q[:, 3] * w2, q[:, 0] * w0 - q[:, 3] * w1 + q[:, 2] * w2,
                            q[:, 3] * w0 + q[:, 0] * w1 - q[:, 1] * w2, -q[:, 2] * w0 + q[:, 1] * w1 + q[:, 0] * w2], 1)
    dw = torch.linalg.solve(J, (tautb - torch.cross(w, mv(J, w), dim=1)).T).T
    return torch.cat([mv(R, v), dq, Ftb / c['m'] - torch.cross(w, v, dim=1), dw], 1)


def rk4_normalized(X, U, pf, h, c):
    f1 = dynamics_ct(X, U, pf, c)
    f2 = dynamics_ct(X + 0.5 * h * f1, U, pf, c)
    f3 = dynamics_ct(X + 0.5 * h * f2, U, pf, c)
    f4 = dynamics_ct(X + h * f3, U, pf, c)
    Xn = X + (h / 6.0) * (f1 + 2 * f2 + 2 * f3 + f4)
    return torch.cat([Xn[:, :3], Xn[:, 3:7] / Xn[:, 3:7].norm(dim=1, keepdim=True), Xn[:, 7:]], 1)


def convert(X):
    q = X[:, 3:7]
    M, R = rot(q) / (q * q).sum(1)[:, None, None], rot(q)   # quat2mat: s = 2 / |q|^2
    cy = torch.sqrt(M[:, 0, 0] ** 2 + M[:, 1, 0] ** 2)
    eul = torch.stack([torch.atan2(M[:, 2, 1], M[:, 2, 2]), torch.atan2(-M[:, 2, 0], cy),
                       torch.atan2(M[:, 1, 0], M[:, 0, 0])], 1)
    return torch.cat([X[:, :3], eul, mv(R, X[:, 7:10]), mv(R, X[:, 10:13])], 1)


def plant_ref(X0, U, pf, n, c):
    X, hist = X0, []
    for s in range(n):
        X = rk4_normalized(X, U, pf[:, s], DT, c)
        hist.append(X)
    return X, convert(X), torch.stack(hist, 1) if n else X0.new_zeros((X0.shape[0], 0, 13))


def inputs(n, B, seed):
    """test_plant_kernel_many_steps_matches_oracle's recipe with a per-robot pf; unit quaternions
    with |pitch| < 1.2; the last robot has |q0| = 1.1 and |w| = 8."""
    rng = np.random.default_rng(seed)
    X0 = np.concatenate([rng.uniform(-1, 1, (B, 3)), np.zeros((B, 4)), rng.uniform(-1, 1, (B, 6))], 1)
    for b in range(B):
        while True:
            q = rng.normal(size=4)
            q /= np.linalg.norm(q)
            if abs(np.arcsin(2 * (q[0] * q[2] - q[1] * q[3]))) < 1.2:
                break
        X0[b, 3:7] = q
    X0[-1, 3:7] *= 1.1
    X0[-1, 10:13] *= 8.0 / np.linalg.norm(X0[-1, 10:13])
    g = dict(X=rng.standard_normal((B, 13)), x=rng.standard_normal((B, 12)), h=rng.standard_normal((B, n, 13)))
    return X0, rng.uniform(-50, 150, (B, 6)), rng.uniform(-0.5, 0.5, (B, n, 3)), g


def ref_grads(X0, U, pf, n, g, cots, c):
    leaves = [torch.from_numpy(a).requires_grad_(True) for a in (X0, U, pf)]
    outs = plant_ref(*leaves, n, c)
    loss = sum((o * torch.from_numpy(g[k])).sum() for o, k in zip(outs, 'Xxh') if k in cots)
    grads = torch.autograd.grad(loss, leaves, allow_unused=True)
    return [o.detach().numpy() for o in outs], {k: (np.zeros_like(a) if gr is None else gr.numpy())
                                                for k, a, gr in zip(('X0', 'U', 'pf'), (X0, U, pf), grads)}


def gpu_grads(ctx, X0, U, pf, n, g, cots, c, layout='dense', **kw):
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    Ud, Us, pfd, pfs = cu(U), 6, cu(pf), (3 * n, 3)
    if layout == 'shared':   # U: row 0 of a (B,10,6) block; pf: one (n,3) plan for the batch
        Ud, Us, pfd, pfs = cu(np.concatenate([U[:, None], np.zeros((len(U), 9, 6))], 1)), 60, cu(pf[0]), (0, 3)
    X, hist = cu(X0), torch.empty((len(X0), n, 13), dtype=torch.float64, device='cuda')
    if n == 0:
        pfd = Ud   # no step reads pf; the ABI still wants a pointer
    else:
        ctx.plant_device(X, Ud, Us, pfd, *pfs, n, DT, c['J'], X_hist=hist)
    cot = {k: cu(g[k]) if k in cots else None for k in 'Xxh'}
    out = ctx.plant_vjp_device(cu(X0), hist if n >= 2 else None, Ud, Us, pfd, *pfs, n, DT, c['J'], g_X=cot['X'],
                               g_x_out=cot['x'], g_X_hist=cot['h'], **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items() if v is not None}


def figure(got, ref):
    return float(np.abs(got - ref).max() / max(1.0, np.abs(ref).max())) if ref.size else 0.0


@pytest.mark.parametrize('n,B,cots,layout', CASES, ids=[f'{c[0]}-{c[1]}-{c[2]}-{c[3]}' for c in CASES])
def test_gradients(n, B, cots, layout, cset=None):
    from oracle import hmpc_plant as pl
    c = consts(cset)
    X0, U, pf, g = inputs(n, B, 100 * n + B)
    if layout == 'shared':
        pf = np.repeat(pf[:1], B, 0)   # the dense layout of the shared plan: the reference's
    outs, ref = ref_grads(X0, U, pf, n, g, cots, c)
    for b in range(B):   # the reference's forward is the oracle's
        Xr = X0[b].copy()
        for s in range(n):
            Xr = pl.rk4_normalized(Xr, U[b], pf[b, s], DT, c['m'], c['g'], c['J'], c['rh'])
            assert np.abs(outs[2][b, s] - Xr).max() <= 1e-12
        assert np.abs(outs[1][b] - pl.convert(Xr)).max() <= 1e-12
    got = gpu_grads(ctx_for('3f', 10, cset), X0, U, pf, n, g, cots, c, layout, want=('X0', 'U', 'pf') if n else ('X0', 'U'))
    d = {k: figure(v, ref[k]) for k, v in got.items()}
    print(f'PVJP1 n={n} B={B} {cots} {layout} ' + ' '.join(f'{k}={v:.3e} (max {np.abs(ref[k]).max():.2e})'
                                                        for k, v in d.items()))
    assert all(v <= TOL[k] for k, v in d.items())


def test_partial_outputs():
    c, ctx = consts(), ctx_for('3f', 10)
    X0, U, pf, g = inputs(2, 3, 203)
    full, part = gpu_grads(ctx, X0, U, pf, 2, g, 'Xxh', c), gpu_grads(ctx, X0, U, pf, 2, g, 'Xxh', c, want=('U',))
    assert set(part) == {'U'} and np.array_equal(part['U'], full['U'])
    null, zero = gpu_grads(ctx, X0, U, pf, 2, g, 'xh', c), gpu_grads(ctx, X0, U, pf, 2, dict(g, X=0 * g['X']), 'Xxh', c)
    assert all(np.array_equal(null[k], zero[k]) for k in zero)


def test_autograd_wrappers():
    import hmpc_autograd
    c, ctx = consts(), ctx_for('3f', 10)
    X0, U, pf, _ = inputs(2, 2, 7)
    X, Ud, pfd = (torch.from_numpy(a).cuda().requires_grad_(True) for a in (X0, U, pf))
    kw = dict(eps=1e-6, atol=1e-6, rtol=1e-6)
    assert torch.autograd.gradcheck(lambda X, U, pf: hmpc_autograd.plant(ctx, X, U, pf, 2, DT, c['J'])[:2], (X, Ud, pfd), **kw)
    assert torch.autograd.gradcheck(lambda X: hmpc_autograd.convert(ctx, X), (X,), **kw)
    Xn, x_out, hist = hmpc_autograd.plant(ctx, X, Ud, pfd, 2, DT, c['J'])
    assert np.array_equal(X.detach().cpu().numpy(), X0)   # the caller's state survives the in-place plant
    Xd, xd = X.detach().clone(), torch.empty((2, 12), dtype=torch.float64, device='cuda')
    ctx.plant_device(Xd, Ud.detach(), 6, pfd.detach(), 6, 3, 2, DT, c['J'], x_out=xd)
    assert torch.equal(Xd, Xn) and torch.equal(xd, x_out) and torch.equal(hist[:, -1], Xn)
    ctx.convert_device(Xd, xd)
    assert torch.equal(hmpc_autograd.convert(ctx, Xd), xd)


@pytest.mark.parametrize('variant', ('3f', '2f'))
def test_one_period_closed_loop(variant):
    # L = <cw, x1>, x1 two plant steps under u[:, 0] of mpcontrol(convert(X0)): the direct term + the chain
    import hmpc_autograd
    N, c = 3, consts()
    inst, ref, lin = reference(variant, N, IDX[variant], 'drop')
    tol, ctx = bound(ref, lin)[2], ctx_for(variant, N)
    e, xi = 0.5 * inst['x_in'][:, 3:6], inst['x_in']   # 'rzyx' Euler angles (roll, pitch, yaw) -> quaternion
    (cr, cp, cy), (sr, sp, sy) = np.cos(e).T, np.sin(e).T
    q = np.stack([cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy,
                  cr * cp * sy - sr * sp * cy], 1)
    Rt = rot(torch.from_numpy(q)).transpose(1, 2)
    X0 = np.concatenate([xi[:, :3], q, mv(Rt, torch.from_numpy(xi[:, 6:9])).numpy(),
                         mv(Rt, torch.from_numpy(xi[:, 9:12])).numpy()], 1)
    cw = np.random.default_rng(11).standard_normal((3, 12))
    pf2 = np.ascontiguousarray(np.repeat(inst['pf'][:, :1], 2, 1))
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in dict(inst, X0=X0, cw=cw, pf2=pf2).items()}
    X = dev['X0'].requires_grad_(True)
    x_in = hmpc_autograd.convert(ctx, X)
    u, _ = hmpc_autograd.mpcontrol(ctx, x_in, dev['x_ref'], dev['pf'], dev['C'], init=True, mu=dev['mu'])
    _, x1, _ = hmpc_autograd.plant(ctx, X, u[:, 0], dev['pf2'], 2, DT, c['J'])
    (grad,) = torch.autograd.grad((x1 * dev['cw']).sum(), X)
    Xt, Ut = torch.from_numpy(X0).requires_grad_(True), u[:, 0].detach().cpu().requires_grad_(True)
    direct, g_U = torch.autograd.grad((plant_ref(Xt, Ut, torch.from_numpy(pf2), 2, c)[1] * torch.from_numpy(cw)).sum(), (Xt, Ut))
    inst = dict(inst, x_in=x_in.detach().cpu().numpy())
    g_u = np.zeros((3, N, 6))
    g_u[:, 0] = g_U.numpy()
    g_xin = np.array([mpcontrol_chain(variant, N, inst, i, g_u[i])[0] for i in range(3)])
    (via,) = torch.autograd.grad(convert(Xt), Xt, grad_outputs=torch.from_numpy(g_xin))
    want, got = (direct + via).numpy(), grad.cpu().numpy()
    d = max(figure(got[i], want[i]) for i in range(3))
    print(f'PVJP4 {variant} gpu={d:.3e} tol={tol:.3e} through the solve={np.abs(via.numpy()).max():.3e}')
    assert d <= tol
    assert np.abs(got - direct.numpy()).max() > 1e3 * tol   # the path through the solve is live


def test_arguments():
    ctx = ctx_for('3f', 10)
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device='cuda')   # noqa: E731
    Jh = np.eye(3).ravel()
    J = Jh.ctypes.data_as(ctx._lib.hmpc_plant_vjp_batch.argtypes[4])
    X0, Xh, U, pf, gX, gx, gh, o0, oU, op = (t.data_ptr() for t in (z(1, 13), z(1, 2, 13), z(1, 6), z(1, 2, 3), z(1, 13),
                                                                    z(1, 12), z(1, 2, 13), z(1, 13), z(1, 6), z(1, 2, 3)))
    call = lambda h=ctx._h, B=1, n=2, dt=DT, J=J, X0=X0, Xh=Xh, U=U, Us=6, pf=pf, pb=6, ps=3, gX=gX, gx=gx, gh=gh, o0=o0, oU=oU, op=op: \
        ctx._lib.hmpc_plant_vjp_batch(h, B, n, dt, J, X0, Xh, U, Us, pf, pb, ps, gX, gx, gh, o0, oU, op, None)   # noqa: E731
    assert call() == 0 and call(B=0) == 0 and call(n=1, Xh=None) == 0 and call(n=0, gh=None, op=None) == 0
    bad = [dict(h=None), dict(J=None), dict(X0=None), dict(U=None), dict(pf=None), dict(Us=-1), dict(pb=-1), dict(ps=-1),
           dict(B=-1), dict(n=-1), dict(dt=0.0), dict(gX=None, gx=None, gh=None), dict(o0=None, oU=None, op=None),
           dict(Xh=None), dict(n=0, gX=None, gx=None, gh=None, op=None), dict(n=0, op=None), dict(n=0, gh=None)]
    for kw in bad:
        assert call(**kw) == -1, kw
