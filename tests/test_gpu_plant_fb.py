"""hmpc_plant_fb_batch / Context.plant_fb_device / Runner(feedback=True): the plant under u_s = clip(U + K (convert(X_s)
- xbar_s)) against plain numpy fp64 around oracle/hmpc_plant.py's convert and rk4_normalized (fb_ref below: the law,
the clip and the count, no kernel code).  Figure: max |gpu - ref| / max(1, max |ref|) per output; TOL is 10 x the
worst of each class in the first run on an MI355X: states (X, X_hist, x_out) 5.844e-16 and inputs
(U_hist) 1.504e-14, both at n = 20, B = 130; the Runner replay with the real gains (max |K| 5.4e2) 2.181e-16 (2f).  With
K = 0 the kernel differs from plant_device by 4.144e-17."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')

from test_gpu_plant_vjp import consts, figure, inputs   # noqa: E402
from test_gpu_vjp_lin import ctx_for   # noqa: E402

pytestmark = pytest.mark.gpu

DT, STAGE, CLIP, INTERP = 1e-3, 20, 1, 2
TOL = dict(states=5.844e-15, inputs=1.504e-13, replay=2.181e-15)
CASES = [(1, 1, 0, 'dense'), (1, 65, CLIP, 'clipmix'), (3, 5, INTERP, 'strided'), (20, 130, CLIP | INTERP, 'dense'),
         (2, 3, 0, 'yaw'), (2, 4, CLIP, '2f')]
cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731


def fb_ref(X0, U, K, x_nom, pf, C0, mu, n, flags, fy_zero, c):
    """(X_hist, U_hist, x_out, sat, raw inputs, clip moves, yaw differences) of the law, robot by robot."""
    from oracle import hmpc_plant as pl
    B, tl = len(X0), np.array([7.78, 7.78, 4.0])
    Xh, Uh, raw, xo, sat, yaws = *(np.zeros((B, n, k)) for k in (13, 6, 6)), np.zeros((B, 12)), np.zeros(B, np.int32), []
    for b in range(B):
        X = X0[b].copy()
        for s in range(n):
            xbar = x_nom[b, 0] + (s / STAGE) * (x_nom[b, 1] - x_nom[b, 0]) if flags & INTERP else x_nom[b, 0]
            d = pl.convert(X) - xbar
            yaws.append(d[5])
            d[5] -= 2 * np.pi * np.rint(d[5] / (2 * np.pi))
            u = raw[b, s] = U[b] + K[b] @ d
            if flags & CLIP:
                v = np.concatenate([np.zeros(3), np.clip(u[3:], -tl, tl)])
                if C0[b] != 0:
                    v[2] = np.clip(u[2], 0.0, 206.0)
                    v[0] = np.clip(u[0], -mu[b] * v[2], mu[b] * v[2])
                    v[1] = 0.0 if fy_zero else np.clip(u[1], -mu[b] * v[2], mu[b] * v[2])
                sat[b] += (np.abs(v - u) > 1e-8 * (1 + np.abs(v))).any()   # a moved component sits on its bound
                u = v
            Uh[b, s] = u
            X = Xh[b, s] = pl.rk4_normalized(X, u, pf[b, s], DT, c['m'], c['g'], c['J'], c['rh'])
        xo[b] = pl.convert(X)
    return Xh, Uh, xo, sat, raw, np.abs(Uh - raw), np.array(yaws)


def case_inputs(n, B, flags, layout):
    from oracle import hmpc_plant as pl
    X0, U, pf, _ = inputs(n, B, 1000 * n + B)
    rng = np.random.default_rng(7 * n + B)
    C0, mu = np.ones(B), np.ones(B)
    if layout == 'clipmix':
        C0, mu = (np.arange(B) % 4 != 0).astype(float), np.array([0.5, 0.7, 1.0])[np.arange(B) % 3]
        U[::2] *= 2.0   # fz beyond 206
        U[::5, [0, 1, 3, 4, 5]] *= 0.02   # well inside the cone and the torque bounds: some robots do not clip
    if layout == 'strided':
        pf = np.repeat(pf[:1], B, 0)
    if layout == 'yaw':   # yaw +-3.1 against a nominal yaw of -+3.1: the difference wraps
        X0[0, 3:7], X0[1, 3:7] = [np.cos(1.55), 0, 0, np.sin(1.55)], [np.cos(1.55), 0, 0, -np.sin(1.55)]
    x0 = np.array([pl.convert(X) for X in X0]) + 1e-2 * rng.standard_normal((B, 12))
    if layout == 'yaw':
        x0[0, 5], x0[1, 5] = -3.1, 3.1
    return X0, U, rng.uniform(-50, 50, (B, 6, 12)), np.stack([x0, x0 + 1e-2], 1), pf, C0, mu


def gpu_fb(ctx, X0, U, K, x_nom, pf, C0, mu, n, flags, layout, c):
    B = len(X0)
    Ud, Us, Kd, Ks, xd, xs, pfd, pfs, kw = cu(U), 6, cu(K), 72, cu(x_nom), 24, cu(pf), (3 * n, 3), dict(C0=cu(C0), mu=cu(mu))
    if layout == 'strided':   # rows of wider blocks, one pf plan for the batch, no C0 and no mu
        pad = lambda a, w: cu(np.concatenate([a.reshape(B, -1), np.zeros((B, w - a[0].size))], 1))   # noqa: E731
        Ud, Us, Kd, Ks, xd, xs, pfd, pfs, kw = pad(U, 60), 60, pad(K, 144), 144, pad(x_nom, 132), 132, cu(pf[0]), (0, 3), {}
    X, f64 = cu(X0), dict(dtype=torch.float64, device='cuda')
    out = dict(X_hist=torch.empty((B, n, 13), **f64), U_hist=torch.empty((B, n, 6), **f64),
               x_out=torch.empty((B, 12), **f64), sat=torch.empty(B, dtype=torch.int32, device='cuda'))
    ctx.plant_fb_device(X, Ud, Us, Kd, Ks, xd, xs, pfd, *pfs, n, STAGE, DT, c['J'], C0_bstride=1, flags=flags, **kw, **out)
    torch.cuda.synchronize()
    return X.cpu().numpy(), {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize('n,B,flags,layout', CASES, ids=[f'{c[0]}-{c[1]}-{c[2]}-{c[3]}' for c in CASES])
def test_against_reference(n, B, flags, layout, cset=None):
    c, fy0 = consts(cset), layout == '2f'
    X0, U, K, x_nom, pf, C0, mu = case_inputs(n, B, flags, layout)
    Xh, Uh, xo, sat, raw, moves, yaws = fb_ref(X0, U, K, x_nom, pf, C0, mu, n, flags, fy0, c)
    # on the reference alone: no clip move and no yaw difference near where sat or the wrap could flip on rounding
    assert ((moves == 0) | (moves > 1e-5)).all() and (np.abs(np.abs(yaws) - np.pi) > 1e-3).all()
    if layout == 'clipmix':   # every kind of clip happens
        st, r, v = C0 == 1, raw[:, 0], Uh[:, 0]
        assert (np.abs(r[:, 3:]) > 7.78).any() and (r[st, 2] < 0).any() and (r[st, 2] > 206).any() and (C0 == 0).any()
        assert (v[st, 0] < r[st, 0]).any() and (v[st, 0] > r[st, 0]).any() and not sat.all()
    if layout == 'yaw':
        assert yaws[0] > 6 and yaws[n] < -6
    X, got = gpu_fb(ctx_for('2f' if fy0 else '3f', 10, cset), X0, U, K, x_nom, pf, C0, mu, n, flags, layout, c)
    d = dict(X=figure(X, Xh[:, -1]), X_hist=figure(got['X_hist'], Xh), x_out=figure(got['x_out'], xo),
             U_hist=figure(got['U_hist'], Uh))
    print(f'PFB1 n={n} B={B} flags={flags} {layout} ' + ' '.join(f'{k}={v:.3e}' for k, v in d.items())
          + f' (max |X| {np.abs(Xh).max():.2e} |U| {np.abs(Uh).max():.2e}) sat {sat.sum()}')
    assert max(d['X'], d['X_hist'], d['x_out']) <= TOL['states'] and d['U_hist'] <= TOL['inputs']
    assert np.array_equal(got['sat'], sat)


def test_zero_gain_is_the_plant():
    c, ctx = consts(), ctx_for('3f', 10)
    X0, U, K, x_nom, pf, C0, mu = case_inputs(3, 70, 0, 'dense')
    _, got = gpu_fb(ctx, X0, U, 0 * K, x_nom, pf, C0, mu, 3, 0, 'dense', c)
    X, hist = cu(X0), torch.empty((70, 3, 13), dtype=torch.float64, device='cuda')
    ctx.plant_device(X, cu(U), 6, cu(pf), 9, 3, 3, DT, c['J'], X_hist=hist)
    print(f"PFB2 zero gain against plant_device: {(d := figure(got['X_hist'], hist.cpu().numpy())):.3e}")
    assert d <= TOL['states'] and np.array_equal(got['U_hist'], np.repeat(U[:, None], 3, 1)) and not got['sat'].any()


@pytest.mark.parametrize('variant', ('3f', '2f'))
def test_runner_feedback(variant):
    import hmpc_runner
    c, worst = consts(), 0.0
    r = hmpc_runner.Runner(dyn=variant, N_run=60, N=10, batch=2, feedback=True)
    res = r.run(record=True)
    assert res['X_traj'].shape == (2, 61, 13) and res['sat'].shape == (3, 2) and (res['status'] == 0).all()
    for p, k in enumerate((0, 20, 40)):   # period by period from the recorded state: the real gains do not compound
        pf = np.repeat(res['pf_ref'][None, k:k + 20], 2, 0)
        Xh, Uh = fb_ref(res['X_traj'][:, k], res['U0'][p], res['K'][p], res['x_nom'][p], pf, res['C0'][p], np.ones(2),
                        20, CLIP | INTERP, variant == '2f', c)[:2]
        worst = max(worst, figure(res['X_traj'][:, k + 1:k + 21], Xh), figure(res['f_hist'][:, k:k + 20], Uh))
    print(f'PFB3 {variant} replay={worst:.3e} max |K| {np.abs(res["K"]).max():.2e} sat {res["sat"].ravel()}')
    assert worst <= TOL['replay']
    for _ in range(2):   # the capture's eager run, then a replay
        g = r.run(record=True, graph=True)
        assert all(np.array_equal(g[k], res[k]) for k in ('X_traj', 'f_hist', 'sat', 'K'))
    off, plain = (hmpc_runner.Runner(dyn=variant, N_run=60, N=10, batch=2, **kw).run() for kw in (dict(feedback=False), {}))
    assert all(np.array_equal(off[k], plain[k]) for k in plain) and 'sat' not in off


def test_arguments():
    ctx, c = ctx_for('3f', 10), consts()
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device='cuda')   # noqa: E731
    J = np.eye(3).ravel().ctypes.data_as(ctx._lib.hmpc_plant_fb_batch.argtypes[5])
    X2 = z(2, 13)
    X2[:, 3] = 1.0
    X, U, K, xn, pf = (t.data_ptr() for t in (X2, z(1, 6), z(1, 72), z(1, 24), z(2, 3)))
    call = lambda h=ctx._h, B=1, n=2, st=20, dt=DT, J=J, X=X, U=U, K=K, xn=xn, pf=pf, Us=6, fl=3: \
        ctx._lib.hmpc_plant_fb_batch(h, B, n, st, dt, J, X, U, Us, K, 72, xn, 24, pf, 6, 3, None, 0, None, fl, None, None, None, None, None)   # noqa: E731
    assert call() == 0 and call(B=0) == 0
    for kw in (dict(h=None), dict(X=None), dict(U=None), dict(K=None), dict(xn=None), dict(pf=None), dict(J=None),
               dict(n=0), dict(st=0), dict(fl=4), dict(fl=-1), dict(B=-1), dict(dt=0.0), dict(Us=-1)):
        assert call(**kw) == -1, kw
    a = dict(X=X2, U=z(2, 6), U_bstride=6, K=z(2, 72), K_bstride=72, x_nom=z(2, 24), xnom_bstride=24, pf=z(2, 3, 3),
             pf_bstride=9, pf_sstride=3, n_steps=3, stage_steps=20, dt=DT, J=c['J'], flags=CLIP | INTERP)
    ctx.plant_fb_device(**a)
    for kw in (dict(X=z(2, 12)), dict(U=z(1, 6)), dict(K=z(2, 71)), dict(x_nom=z(2, 23)), dict(pf=z(2, 2, 3)), dict(K=None),
               dict(C0=z(1), C0_bstride=1), dict(mu=z(3)), dict(U_hist=z(2, 3, 5)), dict(sat=z(2)), dict(K=z(2, 72).cpu()),
               dict(K_bstride=-1), dict(X_hist=z(2, 2, 13))):
        with pytest.raises(ValueError):
            ctx.plant_fb_device(**dict(a, **kw))
    torch.cuda.synchronize()
