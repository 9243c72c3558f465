"""hmpc_kkt_batch / Context.kkt_device: multipliers and KKT certificate on the
device against the oracle's (exact IPM + polish, oracle/qp_exact.py).

Inputs: golden qp_* windows truncated to N (N = 64: hmpc_plan's sampler), every
one solved by the oracle.  No golden window has an active z row, so the
modes below change the inputs until the oracle holds x[k][2] >= 0.1:
  drop    x_in z = 0.14, vz = -1, z reference 0.05: one or two z rows
  zref    z reference 0.05 only (N = 64): a z row at stage 63 / 36
  ride    all-stance C, x_in z = 0.104, vz = -0.1, z reference -2 (N = 64): up
          to 19 z rows at once, stages 4 .. 63 (every eight-column block of the
          Gram row and of the elimination that 19 rows reach)
  stage1  x_in z = 0.102, vz = -0.1: x_1[2] = 0.1.  That row is fixed by x_0, so
          it is always dependent: HMPC_KKT_SINGULAR is expected exactly there
          (predicted on the CPU from the oracle's x), the instance's duals
          are not compared, its certificate is.  2 of the 24 cases: within
          the cap of one in ten (test_inputs_cover_the_classes).

At a stance stage with fz = 0 the five force rows are dependent and the
multipliers not unique (the oracle's polish returns another member than the
minimal split): those stages are compared through A_u' y, which is unique.

Measured on the first run (MI355X), recorded in DESIGN.md 4.7; the bounds
asserted here are 10x those figures:
  duals   worst |d| / (1 + max|y|)        1.263e-10 (2f, N = 64, 19 z rows; 8.5e-15 up to 2 rows)
  cert    worst |cert - oracle's cert|    1.593e-15 (worst entry there: 2.567e-15)
  end to end, worst certificate entry     2.802e-12 (complementarity, N = 64)
"""
import functools
import os

import numpy as np
import pytest

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')
DUAL_TOL = 1.3e-9
CERT_TOL = 1.6e-14
E2E_BOUND = 2.9e-11
KEYS = ('primal_eq', 'primal_ineq', 'dual_neg', 'stationarity', 'complementarity')
IDX = {'3f': (0, 5, 8), '2f': (0, 7, 15)}   # golden windows the oracle solves in every mode used
CASES = [(v, N, idx, uref, mode) for v in ('3f', '2f') for N in (1, 2, 3, 10)
         for idx, uref, mode in ((IDX[v][1:2], 'aliased', 'plain'), (IDX[v], 'per_stage', 'drop'))]
CASES += [(v, 64, idx, uref, mode) for v in ('3f', '2f') for idx, uref, mode in (
    ((0,), 'aliased', 'plain'), ((0, 1, 2), 'per_stage', 'zref'),
    ((4, 6, 7), 'per_stage', 'ride'))]
CASES += [('3f', 2, IDX['3f'], 'per_stage', 'stage1'), ('2f', 10, IDX['2f'], 'per_stage', 'stage1')]
IDS = ['-'.join(map(str, (c[0], c[1], len(c[2]), c[3], c[4]))) for c in CASES]


def constants(consts=None):
    """dict(t, m, g, Jinv, rh): the Runner's, or those of the hashable
    (t, m, g, Jinv[9] row-major, rh[3]) that the references below take as `consts`."""
    from oracle import hmpc_oracle as ho
    if consts is None:
        return ho.runner_constants()
    t, m, g, Jinv, rh = consts
    return dict(t=t, m=m, g=g, Jinv=np.array(Jinv, dtype=np.float64).reshape(3, 3), rh=np.array(rh, dtype=np.float64))


def mpc_params(variant, N, mu, consts=None):
    from oracle import hmpc_oracle as ho
    c = constants(consts)
    return ho.MpcParams(variant=variant, N=N, t=c['t'], m=c['m'], g=c['g'], mu=mu, Jinv=c['Jinv'], rh=c['rh'])


def windows(variant, N, idx):
    """The recorded golden windows (N <= 10, truncated to N) or hmpc_plan's sampler (longer horizons)."""
    import hmpc_plan
    if N > 10:
        d = hmpc_plan.sample_instances(max(idx) + 1, N, curve=True, seed=64)
    else:
        d = np.load(os.path.join(GOLDEN, f'qp_{variant}_N10_straight.npz'))
    return {k: np.array(d[k][list(idx)], dtype=np.float64) for k in ('x_in', 'x_lin', 'x_ref', 'pf', 'C', 'mu')}


def ctx_for(variant, N, uref='aliased', consts=None):
    import hmpc
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need an MI355X (torch.cuda.is_available() is False)')
    c = constants(consts)
    return hmpc.Context(variant, N, t=c['t'], m=c['m'], g=c['g'], mu=1.0, Jinv=c['Jinv'], rh=c['rh'],
                        uref_mode=uref)


def oracle_duals(variant, N, C, y):
    """info['y'] -> nu [N], lam [N,11] by the row order of build_qp."""
    nu, lam, r = np.zeros(N), np.zeros((N, 11)), 0
    for k in range(N):
        for c in range(3):
            lam[k, c] = y[r] + y[r + 1]
            r += 2
        if variant == '2f':
            lam[k, 9] = y[r]
            r += 1
        nu[k] = -y[r]
        r += 13
        if C[k] == 0:
            sl = (8, 10) if variant == '2f' else (8, 9, 10)
            lam[k, sl] = y[r:r + len(sl)]
            r += len(sl)
        else:
            nf = 2 if variant == '2f' else 4
            lam[k, 3:3 + nf] = y[r:r + nf]
            lam[k, 7] = y[r + nf] + y[r + nf + 1]
            r += nf + 2
    assert r + 12 == len(y)
    return nu, lam


@functools.lru_cache(maxsize=None)
def reference(variant, N, idx, uref, mode, consts=None):
    """Inputs [B, ...], the oracle's primal, duals and certificate, and the
    instances expected singular (computed once, shared by the tests)."""
    from oracle import hmpc_oracle as ho
    inst = windows(variant, N, idx)
    inst['x_lin'] = inst['x_lin'][:, :N + 1]
    for k in ('x_ref', 'pf', 'C'):
        inst[k] = np.ascontiguousarray(inst[k][:, :N])
    z0, vz, zref = {'plain': (None,) * 3, 'drop': (0.14, -1.0, 0.05), 'drop6': (0.14, -0.6, 0.05), 'zref': (None, None, 0.05),
                    'ride': (0.104, -0.1, -2.0), 'stage1': (0.102, -0.1, 0.05)}[mode]
    if z0 is not None:
        inst['x_in'][:, 2], inst['x_in'][:, 8] = z0, vz
    if zref is not None:
        inst['x_ref'][:, :, 2] = zref
    if mode == 'ride':
        inst['C'][:] = 1.0
    inst['x_lin'][:, 0] = inst['x_in']
    ref = dict(u=[], x=[], nu=[], lam=[], cert=[])
    for i in range(len(idx)):
        p = mpc_params(variant, N, float(inst['mu'][i]), consts)
        s = ho.solve_instance(p, inst['x_in'][i], inst['x_lin'][i], inst['x_ref'][i], inst['pf'][i],
                              inst['C'][i], uref)
        assert s['status'] == 'solved', (variant, N, idx[i], mode)   # the batch keeps its size
        nu, lam = oracle_duals(variant, N, inst['C'][i], s['info']['y'])
        for k, v in (('u', s['u']), ('x', s['x']), ('nu', nu), ('lam', lam),
                     ('cert', [s['info']['cert'][c] for c in KEYS])):
            ref[k].append(v)
    ref = {k: np.array(v) for k, v in ref.items()}
    # the z row of stage 1 is fixed by x_0: active, it is dependent
    ref['singular'] = ref['x'][:, 1, 2] - 0.1 <= 1.1e-8 if N > 1 else np.zeros(len(idx), bool)
    ref['zrows'] = (ref['x'][:, 1:N, 2] - 0.1 <= 1.1e-8).sum(axis=1)
    return inst, ref


def run_kkt(ctx, inst, u, x):
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in inst.items()}
    out = ctx.kkt_device(dev['x_in'], dev['x_lin'], dev['x_ref'], dev['pf'], dev['C'],
                         torch.from_numpy(np.ascontiguousarray(u)).cuda(),
                         torch.from_numpy(np.ascontiguousarray(x)).cuda(), mu=dev['mu'])
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def canon(lam, apex, mu):
    """Apex stages: slots 3..7 -> A_u' y (unique); other stages unchanged."""
    out = lam.copy()
    l = lam[apex]
    m = np.broadcast_to(mu[:, None], apex.shape)[apex]
    out[apex, 3:8] = np.stack([l[:, 3] - l[:, 4], l[:, 5] - l[:, 6], l[:, 7] - m * l[:, 3:7].sum(1),
                               0 * m, 0 * m], axis=1)
    return out


def test_inputs_cover_the_classes():
    """CPU only, from the oracle's active sets: singular cases within one in
    ten; per variant an active z row, apex, swing and torque / fz = 206 window."""
    refs = [(c, *reference(*c)) for c in CASES]
    assert sum(r['singular'].any() for _, _, r in refs) <= len(CASES) / 10
    assert max(r['zrows'].max() for _, _, r in refs) >= 17   # past two eight-column blocks
    for v in ('3f', '2f'):
        mine = [(i, r) for c, i, r in refs if c[0] == v]
        assert any((r['nu'] > 0).any() for _, r in mine)
        assert any(((i['C'] != 0) & (r['lam'][:, :, 7] < 0)).any() for i, r in mine)       # apex: fz >= 0 active
        assert any((i['C'] == 0).any() for i, _ in mine)
        assert any((r['lam'][:, :, :3] != 0).any() or (r['lam'][:, :, 7] > 0).any() for _, r in mine)
        assert max(r['zrows'].max() for _, r in mine) >= 8                                  # crosses a block


@pytest.mark.parametrize('variant,N,idx,uref,mode', CASES, ids=IDS)
def test_duals_from_the_exact_primal(variant, N, idx, uref, mode, consts=None):
    inst, ref = reference(variant, N, idx, uref, mode, consts)
    r = run_kkt(ctx_for(variant, N, uref, consts), inst, ref['u'], ref['x'])
    assert np.array_equal(r['flags'] != 0, ref['singular'])
    ok = ~ref['singular']   # flagged instances: the certificate only
    apex = (inst['C'] != 0) & (np.abs(ref['u'][:, :, 2]) <= 1e-8)
    scale = 1 + max(np.abs(ref['nu']).max(), np.abs(ref['lam']).max())
    dl = np.abs(canon(r['lam'], apex, inst['mu']) - canon(ref['lam'], apex, inst['mu']))
    d_dual = max(np.abs(r['nu'] - ref['nu'])[ok].max(initial=0), dl[ok].max(initial=0)) / scale
    d_cert = np.abs(r['cert'] - ref['cert']).max()
    print(f'KKT1 {variant} N={N} B={len(idx)} {uref} {mode} zrows={ref["zrows"]} dual={d_dual:.3e} '
          f'cert={d_cert:.3e} certmax={r["cert"].max():.3e}')
    assert d_dual <= DUAL_TOL and d_cert <= CERT_TOL


E2E = [(c, i) for c, i in zip(CASES, IDS) if len(c[2]) == 3]


@pytest.mark.parametrize('variant,N,idx,uref,mode', [c for c, _ in E2E], ids=[i for _, i in E2E])
def test_end_to_end_certificate(variant, N, idx, uref, mode):
    inst, ref = reference(variant, N, idx, uref, mode)
    ctx = ctx_for(variant, N, uref)
    dev = {k: torch.from_numpy(v).cuda() for k, v in inst.items()}
    sol = ctx.solve_device(dev['x_in'], dev['x_lin'], dev['x_ref'], dev['pf'], dev['C'], mu=dev['mu'])
    out = ctx.kkt_device(dev['x_in'], dev['x_lin'], dev['x_ref'], dev['pf'], dev['C'], sol['u'], sol['x'],
                         mu=dev['mu'])
    torch.cuda.synchronize()
    assert (sol['status'].cpu().numpy() == 0).all()
    assert np.array_equal(out['flags'].cpu().numpy() != 0, ref['singular'])
    cert = out['cert'].cpu().numpy()
    print(f'KKT2 {variant} N={N} {uref} {mode} cert={cert.max(axis=0)}')
    assert cert.max() <= E2E_BOUND


def test_detects_a_wrong_answer():
    from oracle import hmpc_oracle as ho
    variant, N = '3f', 10
    inst, ref = reference(variant, N, IDX['3f'], 'per_stage', 'plain')
    ctx = ctx_for(variant, N, 'per_stage')
    # a stance stage whose force rows are all inactive: every force component is free
    i, k = next((i, k) for i in range(len(ref['u'])) for k in range(N - 1)
                if inst['C'][i, k] != 0 and not ref['lam'][i, k, 3:8].any())
    p = ho.MpcParams.runner(variant, N, mu=float(inst['mu'][i]))
    Ad, Bd = ho.gen_dt_dynamics(p, inst['x_lin'][i], inst['pf'][i])
    Gd = ho.constant_matrices(p)[2]
    one = {kk: v[i:i + 1] for kk, v in inst.items()}
    for comp, delta, col in ((0, 1e-3, 3), (2, None, 1)):
        u = ref['u'][i].copy()
        u[k, comp] = u[k, comp] + delta if delta else -1e-3
        x = ho.rollout(p, inst['x_in'][i], u, Ad, Bd, Gd)
        cert = run_kkt(ctx, one, u[None], x[None])['cert'][0]
        print(f'KKT3 comp={comp} cert={cert}')
        assert cert[col] >= (100 * E2E_BOUND if col == 3 else 0.99e-3)


def test_arguments():
    import hmpc
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device='cuda')   # noqa: E731
    with pytest.raises(hmpc.HmpcError, match='HMPC_ERR_UNSUPPORTED'):
        ctx_for('3f', 65).kkt_device(z(1, 12), z(1, 66, 12), z(1, 65, 12), z(1, 65, 3), z(1, 65), z(1, 65, 6),
                                     z(1, 66, 12))
    with pytest.raises(hmpc.HmpcError, match='HMPC_ERR_UNSUPPORTED'):
        ctx_for('cas', 10).kkt_device(z(1, 12), z(1, 11, 12), z(1, 10, 12), z(1, 10, 3), z(1, 10), z(1, 10, 6),
                                      z(1, 11, 12))
    ctx = ctx_for('3f', 10)
    a = [z(1, 12), z(1, 11, 12), z(1, 10, 12), z(1, 10, 3), z(1, 10), None, z(1, 10, 6), z(1, 11, 12)]
    ptr = [None if t is None else t.data_ptr() for t in a]
    assert ctx._lib.hmpc_kkt_batch(ctx._h, 1, *ptr, 1e-8, None, None, None, None, None) == -1
