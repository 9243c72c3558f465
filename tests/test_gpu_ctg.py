"""The dense and swing kernels with the cost-to-go's roll/pitch block in its
(a, p, q, c) form (hmpc_kernels.hip / hmpc_swing.hip phase 2; the algebra is
pinned on the CPU in test_ctg_structure.py), against the C port.

Each N = 10 batch holds the three classes of the split launch -- all-swing,
compacted (at most 48 free variables) and full -- chosen by contact pattern;
N = 5 and N = 1 (S_N alone) run the horizons without a split; one batch has
linearisation yaws that sweep through +-pi.  The comparison and its
tolerances are test_gpu_swing's.
"""
import numpy as np
import pytest

torch = pytest.importorskip('torch')

from test_gpu_swing import KEYS, check, take  # noqa: E402

pytestmark = pytest.mark.gpu

B = 256


@pytest.fixture(scope='module')
def hm():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need an MI355X (torch.cuda.is_available() is False)')
    import hmpc
    return hmpc


def solve(hm, variant, N, inst, order='index'):
    import hmpc_plan
    c = hmpc_plan.runner_constants()
    cx = hm.Context(variant, N, t=c['t'], m=c['m'], g=c['g'], mu=1.0, Jinv=c['Jinv'], rh=c['rh'])
    cx.set_order(order)
    r = cx.solve_host(*(inst[k] for k in KEYS[:5]), mu=inst['mu'])
    name = cx.kernel_name
    cx.close()
    return r, name


def port(variant, N, inst):
    from oracle import port as p
    return p.solve_batch(variant, N, *(inst[k] for k in KEYS[:5]), mu=inst['mu'], nthreads=16)


def check_all(g, ref):
    check(g, ref, swing=False)
    assert np.array_equal(g['iters'], ref['iters'])


def three_classes(variant, curve, seed):
    """B instances at N = 10: a third all-swing, a third with stance stages and
    at most 48 free variables, the rest above 48."""
    import hmpc_plan
    a = hmpc_plan.sample_instances(4096, 10, curve=curve, seed=seed, mu_sweep=(0.3, 1.2))
    nst = (a['C'] != 0).sum(1)
    nf = 30 + (3 if variant == '3f' else 2) * nst
    cls = [np.where(nst == 0)[0], np.where((nst > 0) & (nf <= 48))[0], np.where(nf > 48)[0]]
    n = [B // 3, B // 3, B - 2 * (B // 3)]
    for c, k in zip(cls, n):
        assert len(c) >= k >= 16
    idx = np.sort(np.concatenate([c[:k] for c, k in zip(cls, n)]))
    return take(a, idx)


@pytest.mark.parametrize('variant', ['3f', '2f'])
@pytest.mark.parametrize('curve', [True, False])
def test_three_classes_vs_port(hm, variant, curve):
    inst = three_classes(variant, curve, 71)
    g, name = solve(hm, variant, 10, inst)
    assert 'swing_kernel' in name, name   # the split ran, all-swing class included
    check_all(g, port(variant, 10, inst))


@pytest.mark.parametrize('variant', ['3f', '2f'])
@pytest.mark.parametrize('curve', [True, False])
@pytest.mark.parametrize('N', [5, 1])
def test_short_horizons_vs_port(hm, variant, curve, N):
    import hmpc_plan
    a = hmpc_plan.sample_instances(B, N, curve=curve, seed=72 + N, mu_sweep=(0.3, 1.2))
    inst = take(a, slice(0, B))
    g, _ = solve(hm, variant, N, inst)
    check_all(g, port(variant, N, inst))


@pytest.mark.parametrize('variant', ['3f', '2f'])
def test_yaw_through_pi(hm, variant):
    """Linearisation yaws that climb through +pi and come back wrapped near
    -pi: cos / sin of each stage's yaw are all the recursion sees."""
    inst = three_classes(variant, True, 73)
    k = np.arange(inst['x_lin'].shape[1])
    start = np.pi - np.linspace(0.02, 0.25, B)
    psi = start[:, None] + 0.03 * k[None, :]
    inst['x_lin'][:, :, 5] = (psi + np.pi) % (2 * np.pi) - np.pi
    assert (np.abs(np.diff(inst['x_lin'][:, :, 5], axis=1)) > 6.0).any(axis=1).sum() >= 16
    g, _ = solve(hm, variant, 10, inst)
    check_all(g, port(variant, 10, inst))
