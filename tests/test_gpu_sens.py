"""hmpc_sens_batch / Context.sens_device: S = d u* / d x_in on the device
against a dense float64 reference (SVD of the active rows + reduced Hessian).

Inputs: the recipe of tests/test_gpu_kkt.py -- golden qp_* windows truncated to
N (N = 64: hmpc_plan's sampler), the oracle's primal as the point (x, u), modes
  plain   as recorded: swing stages, saturated torques, an active friction row
  drop    x_in z = 0.14, vz = -1, z reference 0.05: one or two z rows, fz = 206,
          a stance stage with fz = 0
  zref    z reference 0.05 only (N = 64): a late z row
  ride    all-stance C, x_in z = 0.104, vz = -0.1, z reference -2 (N = 64): up to
          19 z rows at once
  mu      plain with mu = 0.5, 0.7, 0.9 over the batch (the context's default is
          1): windows with an active friction row in every instance
  stage1  x_in z = 0.102, vz = -0.1: x_1[2] = 0.1, a row fixed by x_0 and always
          dependent: HMPC_SENS_SINGULAR exactly there (predicted on the CPU); the
          reference is computed with that row removed.  2 cases.

Figure: max |S_gpu - S_ref| / max(1, max |S_ref|) per instance.  Worst values of
the first run (MI355X), next to the disagreement of the
reference's two routes (SVD / lstsq on the full KKT matrix); a case asserts
max(10 x its class's GPU figure, the two routes' disagreement in that case):
  class     gpu vs ref   ref vs ref
  noz       1.485e-10    1.782e-07   (no active z row; worst: 2f, N = 10, mu; 9.222e-11 at mu = 1;
                                      lstsq's worst: 2f, N = 1)
  z2        1.780e-11    8.167e-10   (at most two live z rows, stage1 cases included)
  ride      1.241e-11    2.212e-09   (N = 64, up to 19 z rows)
  e2e       1.241e-11    2.212e-09   (solve_device fp64, then sens_device)
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip('torch')

from test_gpu_kkt import ctx_for as kkt_ctx_for, mpc_params, windows   # noqa: E402

pytestmark = pytest.mark.gpu

TOL = {'noz': 1.5e-9, 'z2': 1.8e-10, 'ride': 1.25e-10, 'e2e': 1.25e-10}   # 10 x the class's GPU figure
IDX = {'3f': (0, 5, 8), '2f': (0, 7, 15)}   # golden windows the oracle solves in every mode used
CASES = [(v, N, IDX[v], 'drop') for v in ('3f', '2f') for N in (1, 2, 3, 10)]
CASES += [(v, 10, IDX[v], 'plain') for v in ('3f', '2f')]
CASES += [(v, 64, idx, mode) for v in ('3f', '2f')
          for idx, mode in (((0,), 'plain'), ((0, 1, 2), 'zref'), ((4, 6, 7), 'ride'))]
CASES += [('3f', 10, (5, 11, 5), 'mu'), ('2f', 10, (10, 15, 10), 'mu')]
CASES += [('3f', 2, IDX['3f'], 'stage1'), ('2f', 10, IDX['2f'], 'stage1')]
IDS = ['-'.join(map(str, (c[0], c[1], len(c[2]), c[3]))) for c in CASES]


def ctx_for(variant, N, consts=None):
    return kkt_ctx_for(variant, N, 'per_stage', consts)


def dense_sens(qp, N, z, skip, route, tol=1e-8):
    """min 1/2 dz'P dz  s.t.  E dz = D over the equality and active rows."""
    Az, l, u = qp['A'] @ z, qp['l'], qp['u']
    act = l == u
    for bnd, slack in ((l, Az - l), (u, u - Az)):
        fin = np.isfinite(bnd)
        act |= fin & (np.where(fin, slack, 1.0) <= tol * (1 + np.abs(np.where(fin, bnd, 0.0))))
    act[list(skip)] = False
    D = np.zeros((len(l), 12))
    D[-12:] = np.eye(12)   # d l / d x_in: the x[0] == x_in rows
    E, D, P = qp['A'][act], D[act], qp['P']
    if route == 'svd':
        U, s, Vt = np.linalg.svd(E)
        r = int((s > 1e-10 * s[0]).sum())
        dzp = Vt[:r].T @ ((U[:, :r].T @ D) / s[:r, None])
        Z = Vt[r:].T
        dz = dzp - Z @ np.linalg.solve(Z.T @ P @ Z, Z.T @ P @ dzp)
    else:
        n, m = P.shape[0], E.shape[0]
        kkt = np.block([[P, E.T], [E, np.zeros((m, m))]])
        dz = np.linalg.lstsq(kkt, np.vstack([np.zeros((n, 12)), D]), rcond=1e-13)[0][:n]
    return dz[(N + 1) * 12:].reshape(N, 6, 12)


@functools.lru_cache(maxsize=None)
def reference(variant, N, idx, mode, consts=None):
    """Inputs [B, ...], the oracle's primal, S by both routes, the instances
    expected singular and the z-row counts (computed once, shared)."""
    from oracle import hmpc_oracle as ho
    inst = windows(variant, N, idx)
    inst['x_lin'] = inst['x_lin'][:, :N + 1]
    for k in ('x_ref', 'pf', 'C'):
        inst[k] = np.ascontiguousarray(inst[k][:, :N])
    if mode == 'mu':
        inst['mu'][:] = (0.5, 0.7, 0.9)
    z0, vz, zref = {'plain': (None,) * 3, 'mu': (None,) * 3, 'drop': (0.14, -1.0, 0.05), 'drop6': (0.14, -0.6, 0.05),
                    'zref': (None, None, 0.05),
                    'ride': (0.104, -0.1, -2.0), 'stage1': (0.102, -0.1, 0.05)}[mode]
    if z0 is not None:
        inst['x_in'][:, 2], inst['x_in'][:, 8] = z0, vz
    if zref is not None:
        inst['x_ref'][:, :, 2] = zref
    if mode == 'ride':
        inst['C'][:] = 1.0
    inst['x_lin'][:, 0] = inst['x_in']
    ref = dict(u=[], x=[], S=[], S2=[])
    for i in range(len(idx)):
        p = mpc_params(variant, N, float(inst['mu'][i]), consts)
        s = ho.solve_instance(p, inst['x_in'][i], inst['x_lin'][i], inst['x_ref'][i], inst['pf'][i],
                              inst['C'][i], 'per_stage')
        assert s['status'] == 'solved', (variant, N, idx[i], mode)
        qp, z = s['qp'], np.concatenate([s['x'].ravel(), s['u'].ravel()])
        skip = ()   # the z row of stage 1 is fixed by x_0: active, it is dependent and dropped
        if N > 1 and s['x'][1, 2] - 0.1 <= 1.1e-8:
            skip = [r for r in range(len(qp['l'])) if qp['l'][r] == 0.1 and qp['A'][r, 14] == 1.0]
        for k, v in (('u', s['u']), ('x', s['x']), ('S', dense_sens(qp, N, z, skip, 'svd')),
                     ('S2', dense_sens(qp, N, z, skip, 'kkt'))):
            ref[k].append(v)
    ref = {k: np.array(v) for k, v in ref.items()}
    ref['d_ref'] = figure(ref['S2'], ref['S'])
    ref['singular'] = ref['x'][:, 1, 2] - 0.1 <= 1.1e-8 if N > 1 else np.zeros(len(idx), bool)
    ref['zrows'] = (ref['x'][:, 1:N, 2] - 0.1 <= 1.1e-8).sum(axis=1)
    return inst, ref


def figure(S, ref):
    return max(np.abs(a - r).max() / max(1.0, np.abs(r).max()) for a, r in zip(S, ref))


def run_sens(ctx, inst, u, x, n_stages=None, reps=1):
    dev = {k: torch.from_numpy(np.ascontiguousarray(np.concatenate([v] * reps))).cuda()
           for k, v in dict(inst, u=u, x=x).items()}
    out = ctx.sens_device(dev['x_in'], dev['x_lin'], dev['x_ref'], dev['pf'], dev['C'], dev['u'], dev['x'],
                          mu=dev['mu'], n_stages=n_stages)
    torch.cuda.synchronize()
    return out['S'].cpu().numpy(), out['flags'].cpu().numpy()


def test_inputs_cover_the_classes():
    """CPU only, from the oracle's points: per variant a swing stage, an active
    friction row, a saturated torque, fz = 206, a stance stage with fz = 0, a z
    row; 19 z rows at once somewhere."""
    refs = [(c, *reference(*c)) for c in CASES]
    assert max(r['zrows'].max() for _, _, r in refs) == 19
    for c, i, r in refs:   # per-instance mu: off the default, a live friction row in every instance
        if c[3] == 'mu':
            u, m = r['u'], i['mu'][:, None]
            fric = (i['C'] != 0) & (u[:, :, 2] > 1e-6) & (
                np.abs(np.abs(u[:, :, :2 if c[0] == '3f' else 1]) - (m * u[:, :, 2])[:, :, None]) <= 1e-8).any(axis=2)
            assert len(set(i['mu'])) == 3 and (i['mu'] != 1.0).all() and fric.any(axis=1).all()
    for v in ('3f', '2f'):
        mine = [(i, r['u'], r) for c, i, r in refs if c[0] == v]
        on = lambda f: any(f(i, u).any() for i, u, _ in mine)   # noqa: E731
        assert on(lambda i, u: i['C'] == 0)
        assert on(lambda i, u: (i['C'] != 0) & (u[:, :, 2] > 1e-6)
                  & (np.abs(np.abs(u[:, :, 0]) - i['mu'][:, None] * u[:, :, 2]) <= 1e-8))
        assert on(lambda i, u: np.abs(np.abs(u[:, :, 3:]) - np.array([7.78, 7.78, 4.0])) <= 1e-8)
        assert on(lambda i, u: np.abs(u[:, :, 2] - 206.0) <= 1e-6)
        assert on(lambda i, u: (i['C'] != 0) & (np.abs(u[:, :, 2]) <= 1e-8))
        assert any(0 < r['zrows'].max() <= 2 for _, _, r in mine)


@pytest.mark.parametrize('variant,N,idx,mode', CASES, ids=IDS)
def test_jacobian_at_the_exact_primal(variant, N, idx, mode, consts=None):
    inst, ref = reference(variant, N, idx, mode, consts)
    ctx = ctx_for(variant, N, consts)
    S, flags = run_sens(ctx, inst, ref['u'], ref['x'])
    S1, flags1 = run_sens(ctx, inst, ref['u'], ref['x'], n_stages=1)
    assert S.shape == (len(idx), N, 6, 12) and S1.shape == (len(idx), 1, 6, 12)
    assert np.array_equal(flags != 0, ref['singular']) and np.array_equal(flags, flags1)
    assert np.array_equal(S1[:, 0], S[:, 0])   # the gain K_0 is the first block
    cls = 'ride' if mode == 'ride' else ('z2' if ref['zrows'].max() > 0 else 'noz')
    d = figure(S, ref['S'])
    print(f'SENS1 {variant} N={N} {mode} {cls} zrows={ref["zrows"]} gpu={d:.3e} refs={ref["d_ref"]:.3e}')
    assert d <= max(TOL[cls], ref['d_ref'])


def test_batch_above_the_launch_grid():
    inst, ref = reference('3f', 3, IDX['3f'], 'drop')
    S, flags = run_sens(ctx_for('3f', 3), inst, ref['u'], ref['x'], reps=343)   # B = 1029 > 1024 workgroups
    assert not flags.any()
    assert figure(S, np.concatenate([ref['S']] * 343)) <= max(TOL['z2'], ref['d_ref'])
    assert np.array_equal(S[-3:], S[:3])


E2E = [(c, i) for c, i in zip(CASES, IDS) if c[1] in (10, 64) and c[3] in ('drop', 'ride')]


@pytest.mark.parametrize('variant,N,idx,mode', [c for c, _ in E2E], ids=[i for _, i in E2E])
def test_end_to_end(variant, N, idx, mode):
    inst, ref = reference(variant, N, idx, mode)
    ctx = ctx_for(variant, N)
    dev = {k: torch.from_numpy(v).cuda() for k, v in inst.items()}
    sol = ctx.solve_device(dev['x_in'], dev['x_lin'], dev['x_ref'], dev['pf'], dev['C'], mu=dev['mu'])
    out = ctx.sens_device(dev['x_in'], dev['x_lin'], dev['x_ref'], dev['pf'], dev['C'], sol['u'], sol['x'],
                          mu=dev['mu'])
    torch.cuda.synchronize()
    assert (sol['status'].cpu().numpy() == 0).all() and not out['flags'].cpu().numpy().any()
    d = figure(out['S'].cpu().numpy(), ref['S'])
    print(f'SENS2 {variant} N={N} {mode} gpu={d:.3e}')
    assert d <= max(TOL['e2e'], ref['d_ref'])


def test_arguments():
    import hmpc
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device='cuda')   # noqa: E731
    args = lambda N: (z(1, 12), z(1, N + 1, 12), z(1, N, 12), z(1, N, 3), z(1, N), z(1, N, 6),   # noqa: E731
                      z(1, N + 1, 12))
    with pytest.raises(hmpc.HmpcError, match='HMPC_ERR_UNSUPPORTED'):
        ctx_for('3f', 65).sens_device(*args(65))
    with pytest.raises(hmpc.HmpcError, match='HMPC_ERR_UNSUPPORTED'):
        ctx_for('cas', 10).sens_device(*args(10))
    ctx = ctx_for('3f', 10)
    for ns in (0, 11):
        with pytest.raises(hmpc.HmpcError, match='HMPC_ERR_ARG'):
            ctx.sens_device(*args(10), n_stages=ns)
    a = list(args(10))
    ptr = [t.data_ptr() for t in a[:5]] + [None] + [None, a[6].data_ptr()]   # mu may be NULL; u may not
    assert ctx._lib.hmpc_sens_batch(ctx._h, 1, *ptr, 1e-8, 1, z(1, 1, 6, 12).data_ptr(), None, None) == -1
