"""Every solve kernel at physical constants other than the Runner's, against
the C port (oracle/hmpc_port.c) called with the same constants.

hmpc_create takes t, m, g, mu, Jinv and rh from the caller; every other GPU
test creates its context from runner_constants(), whose Jinv is symmetric and
nearly diagonal and whose rh is millimetres: a transposed Jinv, a dropped
off-diagonal or a wrong sign in rh can stay below the 1e-6 asserted there.

The sets (SETS; c = runner_constants(), R = Rz(0.9) Ry(-0.7) Rx(0.5)):
  name        t      m     g      Jinv                                   rh
  light_fast  0.01   2.0   9.807  4 c['Jinv']                            c['rh']
  heavy       0.02   10.0  9.807  inv(R diag(0.02, 0.09, 0.2) R')        (0.03, -0.02, -0.05)
  mars_skew   0.025  11.0  3.72   inv(R diag(0.3, 0.05, 0.11) R') + K    (-0.04, 0.05, 0.02)
with K = 0.15 [[0, 1, -2], [-1, 0, 1.5], [2, -1.5, 0]]: mars_skew's Jinv is
not symmetric on purpose (hmpc.h: row-major; the reference forms
rz Jinv rz' from whatever it is given).

The cases (CASES), one context each, created with the set's constants:
  split-*      dense N = 10, the three classes of the split launch
               (test_gpu_ctg.three_classes, B = 256): every set, 3f and 2f;
               one more per set with uref_mode per_stage (2 m g reads m and g)
  short-*      no split, B = 64: N = 5 (dense) and N = 1 (S_N alone; the default
               build has no dense N = 1 kernel, the runtime-horizon Riccati runs)
  ric20-*      the Riccati default at N = 20; dense20-*: precision f64_dense
  n30-*        N = 30: ric_factor_kernel ahead of ric_kernel
  n60-*        N = 60, B = 64: the capacity-64 kernel; with heavy the overflow
               pass re-solves instances (optimal active sets above 64, counted
               on the CPU in test_inputs_can_catch_a_wrong_constant)
  generic      precision f64_generic at N = 10 (test_gpu_wide's recipe, B = 16)
  refined      precision f32_refined, five corrections (test_gpu_f32's bound)
  mu-default   the context's mu = 0.6 with mu = None in the call
and, outside the table, mpcontrol_device (init, then two shifted calls) and
the CAS variant against oracle/cas_oracle.

Bounds: all the project's own, unchanged -- test_gpu_swing.check (identical
statuses, |du| and |dx| <= 1e-6, relative objective <= 1e-9), equal iteration
counts where the dense kernels are held to them today (test_gpu_ctg.check_all),
test_gpu_f32's for f32_refined (the same figures), test_gpu_cas's for CAS.

test_inputs_can_catch_a_wrong_constant is the only test here without the gpu
mark: from the port alone it shows that the batches are solved (>= 90 %) and
that one wrong constant moves u* by at least 1e-3.
"""
import collections
import functools

import numpy as np
import pytest

torch = pytest.importorskip('torch')

from test_gpu_ctg import three_classes  # noqa: E402
from test_gpu_overflow import active_rows  # noqa: E402
from test_gpu_swing import KEYS, check, take  # noqa: E402

gpu = pytest.mark.gpu
NAMES = ('t', 'm', 'g', 'Jinv', 'rh')


def rot(ax, a):
    c, s = np.cos(a), np.sin(a)
    return {'x': np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), 'y': np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]),
            'z': np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])}[ax]


def constant_sets():
    from oracle import hmpc_oracle as ho
    c = ho.runner_constants()
    R = rot('z', 0.9) @ rot('y', -0.7) @ rot('x', 0.5)
    skew = 0.15 * np.array([[0, 1, -2], [-1, 0, 1.5], [2, -1.5, 0]])
    return {
        'light_fast': dict(t=0.01, m=2.0, g=9.807, Jinv=4 * c['Jinv'], rh=c['rh']),
        'heavy': dict(t=0.02, m=10.0, g=9.807, Jinv=np.linalg.inv(R @ np.diag([0.02, 0.09, 0.2]) @ R.T),
                      rh=np.array([0.03, -0.02, -0.05])),
        'mars_skew': dict(t=0.025, m=11.0, g=3.72, Jinv=np.linalg.inv(R @ np.diag([0.3, 0.05, 0.11]) @ R.T) + skew,
                          rh=np.array([-0.04, 0.05, 0.02])),
    }


SETS = constant_sets()


def frozen(name):
    """The set as the hashable (t, m, g, Jinv[9], rh[3]) that the `consts` argument of the
    post-solve and plant modules' helpers takes."""
    s = SETS[name]
    return (s['t'], s['m'], s['g'], tuple(map(float, np.ravel(s['Jinv']))), tuple(map(float, s['rh'])))


Case = collections.namedtuple('Case', 'set variant N B seed classes precision uref mu_ctx kernel iters')


def case(set_, variant, N, B, seed, kernel, classes=False, precision='f64', uref='aliased', mu_ctx=None, iters=False):
    return Case(set_, variant, N, B, seed, classes, precision, uref, mu_ctx, kernel, iters)


CASES = {}
for _s in SETS:
    for _v in ('3f', '2f'):
        CASES[f'split-{_s}-{_v}'] = case(_s, _v, 10, 256, 171, 'swing_kernel', classes=True, iters=True)
        for _N, _k in ((1, f'ric_kernel<{_v[0]}, 2, 0, 0, 0>'), (5, f'solve_kernel<{_v[0]}, 5, double')):
            CASES[f'short-{_s}-{_v}-N{_N}'] = case(_s, _v, _N, 64, 172 + _N, _k, iters=True)
        CASES[f'ric20-{_s}-{_v}'] = case(_s, _v, 20, 128, 174, f'ric_kernel<{_v[0]}, 2, 20')
        CASES[f'dense20-{_s}-{_v}'] = case(_s, _v, 20, 128, 175, f'solve_kernel<{_v[0]}, 20, double', precision='f64_dense')
        CASES[f'n30-{_s}-{_v}'] = case(_s, _v, 30, 64, 176, f'ric_factor_kernel<{_v[0]}')
    CASES[f'n60-{_s}-3f'] = case(_s, '3f', 60, 64, 177, 'ric_kernel<3, 1, 60, 64, 2>')
CASES['n60-mars_skew-2f'] = case('mars_skew', '2f', 60, 64, 177, 'ric_kernel<2, 1, 60, 64, 2>')
for _s, _v in (('light_fast', '3f'), ('heavy', '2f'), ('mars_skew', '3f')):
    CASES[f'split-{_s}-{_v}-per_stage'] = case(_s, _v, 10, 256, 178, 'swing_kernel', classes=True, uref='per_stage',
                                              iters=True)
CASES['generic-mars_skew'] = case('mars_skew', '3f', 10, 16, 77, 'wide_kernel<3, double>', precision='f64_generic')
CASES['refined-mars_skew'] = case('mars_skew', '3f', 10, 256, 93, 'float', precision='f32_refined')
# (a sampled batch, compared like test_gpu_parity's: no iteration equality -- instance 151 reaches the port's
# optimum, |du| = 8.9e-10, in 12 iterations against the port's 10, with mu passed or defaulted alike)
CASES['mu-default-heavy'] = case('heavy', '3f', 10, 256, 179, 'solve_kernel<3, 10, double', mu_ctx=0.6)
OVERFLOW = 'n60-heavy-3f'   # optimal active sets above the capacity-64 kernel's
CAP60 = 64


def port(name, variant, N, inst, mu='inst', **kw):
    from oracle import port as p
    s = SETS[name] if isinstance(name, str) else name
    return p.solve_batch(variant, N, *(inst[k] for k in KEYS[:5]), mu=inst['mu'] if mu == 'inst' else mu, nthreads=16,
                         **{k: s[k] for k in NAMES}, **kw)


@functools.lru_cache(maxsize=None)
def case_data(cid):
    """The case's batch and the port's solution of it (computed once, shared by
    the CPU test and the GPU test)."""
    import hmpc_plan
    k = CASES[cid]
    if k.classes:
        inst = three_classes(k.variant, True, k.seed)
    else:
        inst = take(hmpc_plan.sample_instances(k.B, k.N, curve=True, seed=k.seed, mu_sweep=(0.3, 1.2)), slice(0, k.B))
    assert len(inst['mu']) == k.B
    if k.mu_ctx is None:
        ref = port(k.set, k.variant, k.N, inst, uref_mode=k.uref)
    else:
        ref = port(k.set, k.variant, k.N, inst, mu=None, uref_mode=k.uref, mu_default=k.mu_ctx)
    return inst, ref


def mutations(name):
    """name -> the set with one constant wrong; a mutation that leaves the
    set's value unchanged is left out."""
    from oracle import hmpc_oracle as ho
    s, c, out = SETS[name], ho.runner_constants(), {}
    same = lambda a, b: np.allclose(a, b, rtol=1e-12, atol=0)   # noqa: E731
    for k in NAMES:
        out[f'{k}=runner'] = dict(s, **{k: c[k]})
    out['Jinv transposed'] = dict(s, Jinv=s['Jinv'].T.copy())
    out['diag(Jinv)'] = dict(s, Jinv=np.diag(np.diag(s['Jinv'])))
    for i in range(3):
        out[f'rh[{i}] sign'] = dict(s, rh=s['rh'] * np.where(np.arange(3) == i, -1.0, 1.0))
    return {k: v for k, v in out.items() if not all(same(v[n], s[n]) for n in NAMES)}


def test_inputs_can_catch_a_wrong_constant():
    """CPU only, from the port alone: every case's batch is solved (>= 90 %), the batches hold
    swing stages and fz = 206, the overflow case has optimal active sets above the kernel's
    capacity, and each single wrong constant moves u* of the N = 10 split batches by >= 1e-3."""
    for cid, k in CASES.items():
        inst, ref = case_data(cid)
        assert (ref['status'] == 0).mean() >= 0.9, (cid, (ref['status'] == 0).mean())
        assert k.N == 1 or ((inst['C'] == 0).any() and (inst['C'] != 0).any()), cid
    sat = {s: max((np.abs(case_data(cid)[1]['u'][..., 2] - 206.0) <= 1e-6).any(axis=1).mean()
                  for cid, k in CASES.items() if k.set == s) for s in SETS}
    print('CONST0 share of instances with fz = 206, worst case per set:', sat)
    assert sat['heavy'] > 0
    inst, ref = case_data(OVERFLOW)
    nact = np.array([active_rows(60, inst, ref, i, frozen('heavy')) if ref['status'][i] == 0 else 0
                     for i in range(len(ref['status']))])
    print(f'CONST0 {OVERFLOW}: optimal active sets up to {nact.max()}, iterations up to {ref["iters"].max()}')
    assert (nact > CAP60).any(), nact
    live = collections.Counter()
    for s in SETS:
        muts = mutations(s)
        for v in ('3f', '2f'):
            inst, ref = case_data(f'split-{s}-{v}')
            for name, wrong in muts.items():
                bad = port(wrong, v, 10, inst)
                ok = (ref['status'] == 0) & (bad['status'] == 0)
                du = np.abs(ref['u'][ok] - bad['u'][ok]).max()
                print(f'CONST0 {s} {v} {name}: max |du| = {du:.3e} over {ok.sum()} instances')
                assert ok.sum() >= 128 and du >= 1e-3, (s, v, name, du)
                live[name] += 1
    assert set(live) == {f'{k}=runner' for k in NAMES} | {'Jinv transposed', 'diag(Jinv)'} | {
        f'rh[{i}] sign' for i in range(3)}
    assert live['Jinv transposed'] == 2   # mars_skew alone: the other sets' Jinv is symmetric


@pytest.fixture(scope='module')
def hm():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need an MI355X (torch.cuda.is_available() is False)')
    import hmpc
    return hmpc


def context(hm, name, variant, N, **kw):
    s = SETS[name]
    return hm.Context(variant, N, **dict(dict(mu=1.0, **{k: s[k] for k in NAMES}), **kw))


@gpu
@pytest.mark.parametrize('cid', list(CASES))
def test_solve_vs_port(hm, cid):
    k = CASES[cid]
    inst, ref = case_data(cid)
    cx = context(hm, k.set, k.variant, k.N, uref_mode=k.uref, precision=k.precision,
                 **({} if k.mu_ctx is None else dict(mu=k.mu_ctx)))
    cx.set_order('index')   # (N = 10: the all-swing class at any batch size)
    if k.precision == 'f32_refined':
        cx.set_refinement(5)
    g = cx.solve_host(*(inst[n] for n in KEYS[:5]), mu=inst['mu'] if k.mu_ctx is None else None)
    name, cap, over = cx.kernel_name, cx.active_capacity, cx.overflow_total
    cx.close()
    ok = ref['status'] == 0
    print(f'CONST1 {cid} {name} solved={ok.mean():.3f} du={np.abs(g["u"][ok] - ref["u"][ok]).max():.3e} '
          f'dx={np.abs(g["x"][ok] - ref["x"][ok]).max():.3e} '
          f'dobj={(np.abs(g["obj"][ok] - ref["obj"][ok]) / np.abs(ref["obj"][ok])).max():.3e} '
          f'status={np.array_equal(g["status"], ref["status"])} cap={cap} overflow={over}')
    assert k.kernel in name, name
    check(g, ref, swing=False)
    if k.iters:
        assert np.array_equal(g['iters'], ref['iters'])
    if cid == OVERFLOW:
        assert cap == CAP60 and over >= 1, (cap, over)


@functools.lru_cache(maxsize=None)
def mpcontrol_reference(name, variant, N, B, seed):
    """OracleMpc.mpcontrol's recipe with the port as the solver: per call the x_lin built on the
    host by the reference's rule (3f :52-53 init, :59-62 shift), u and the x* kept for the next."""
    import hmpc_plan
    inst = take(hmpc_plan.sample_instances(B, N, curve=True, seed=seed, mu_sweep=(0.3, 1.2)), slice(0, B))
    calls, x_prev = [], None
    for init in (True, False, False):
        if init:
            r = port(name, variant, N, inst)   # x_guess = [x_in; x_ref]
            assert (r['status'] == 0).all()
            x_lin = r['x']
        else:
            x_lin = np.concatenate([inst['x_in'][:, None], x_prev[:, 2:], x_prev[:, -1:]], axis=1)
        r = port(name, variant, N, dict(inst, x_lin=np.ascontiguousarray(x_lin)))
        assert (r['status'] == 0).all()
        x_prev = r['x']
        calls.append((init, r['u'], r['x']))
    return inst, calls


@gpu
@pytest.mark.parametrize('variant', ['3f', '2f'])
def test_mpcontrol_device(hm, variant):
    N, B = 10, 8
    inst, calls = mpcontrol_reference('mars_skew', variant, N, B, 180)
    cx = context(hm, 'mars_skew', variant, N)
    d = {k: torch.from_numpy(inst[k]).cuda() for k in ('x_in', 'x_ref', 'pf', 'C', 'mu')}
    xp = torch.zeros((B, N + 1, 12), dtype=torch.float64, device='cuda')
    for n, (init, u, x) in enumerate(calls):
        o = cx.mpcontrol_device(init, d['x_in'], d['x_ref'], d['pf'], d['C'], xp, mu=d['mu'])
        torch.cuda.synchronize()
        du, dx = np.abs(o['u'].cpu().numpy() - u).max(), np.abs(xp.cpu().numpy() - x).max()
        print(f'CONST2 {variant} call {n} init={init} du={du:.3e} dx_prev={dx:.3e}')
        assert (o['status'].cpu().numpy() == 0).all()
        assert du <= 1e-6 and dx <= 1e-6
    cx.close()


@gpu
def test_cas_vs_oracle(hm):
    """test_gpu_cas.test_sampled_instances' comparison with heavy's constants."""
    import hmpc_plan
    from oracle import cas_oracle as co
    from test_gpu_cas import U_TOL, feasible, solve
    N, B, s = 10, 16, SETS['heavy']
    inst = hmpc_plan.sample_instances(B, N, curve=True, seed=5)
    cx = context(hm, 'heavy', 'cas', N)
    assert cx.kernel_name == 'hmpc::cas_kernel'
    r = solve(cx, inst['x_in'], inst['x_ref'], inst['C'])
    cx.close()
    assert (r['status'] == 0).all()
    for b in range(B):
        qp = co.build_qp(s['t'], N, s['m'], s['g'], 1.0, s['Jinv'], s['rh'], inst['x_in'][b], inst['x_ref'][b],
                         inst['C'][b])
        z = np.concatenate([r['x'][b].ravel(), r['u'][b].ravel()])
        assert feasible(qp, z, N), b
        obj = 0.5 * z @ qp['P'] @ z + qp['q'] @ z + qp['r']
        assert abs(obj - r['obj'][b]) <= 1e-9 * abs(obj)
        assert co.kkt_residual(qp, z, N) <= 1e-8, b
        ref = co.solve(qp, N)
        assert ref['status'] == 'solved', (b, ref['status'])
        assert np.abs(r['u'][b] - ref['u']).max() <= U_TOL, b
        assert abs(obj - ref['obj']) <= 1e-9 * abs(ref['obj'])
