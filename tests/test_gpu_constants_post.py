"""The post-solve kernels (kkt_device, sens_device, vjp_device, vjp_lin_device) and the plant kernels
(plant_device, plant_fb_device, plant_vjp_device) at physical constants other than the Runner's:
test_gpu_constants' sets `heavy` and `mars_skew` (the plant: `heavy`, whose Jinv is symmetric, with
the body inertia J = inv(Jinv) passed to the calls).

Post-solve cases (CASES): both sets x 3f, 2f x (N = 3 and 10: plain and drop6; N = 30: plain), three
windows each (IDX: windows the oracle solves with that set).  The references are the existing
modules' own, built from MpcParams of the set through their `consts` argument: the oracle's primal,
oracle_duals, dense_sens and the dense vjp Jacobians by both routes; each test below runs the
existing module's comparison with the set.  `drop6` is `drop` with vz = -0.6 instead of -1: with
x_in z = 0.14, vz = -1 the oracle solves none of the first 16 golden windows at these constants
(heavy at N = 10, mars_skew at N = 3 and 10: fz <= 206 cannot stop the heavier body above z = 0.1),
with vz = -0.6 it solves three per case and z rows are held at N = 10.
No case has x_1[2] = 0.1 (predicted on the CPU; no flag expected),
test_inputs_hold_what_the_modes_are_for checks on the CPU that z rows, fz = 206, a stance stage with
fz = 0 and swing stages occur.

Plant cases: n_steps 1, 3 (one plan shared by the batch, U strided) and 20, B <= 8.

Bounds: the project's own, unchanged -- test_gpu_kkt's DUAL_TOL / CERT_TOL, test_gpu_sens', test_gpu_vjp's
and test_gpu_vjp_lin's max(TOL[class], the two reference routes' disagreement in the case),
test_gpu_plant_vjp's and test_gpu_plant_fb's TOL, test_gpu_runner's 1e-11 (X_hist) and 1e-12 (x_out)
for plant_device.  None is a 10x first-run figure of this module.
"""
import numpy as np
import pytest

torch = pytest.importorskip('torch')

import test_gpu_kkt as kkt  # noqa: E402
import test_gpu_plant_fb as plant_fb  # noqa: E402
import test_gpu_plant_vjp as plant_vjp  # noqa: E402
import test_gpu_sens as sens  # noqa: E402
import test_gpu_vjp as vjp  # noqa: E402
import test_gpu_vjp_lin as vjp_lin  # noqa: E402
from test_gpu_constants import frozen  # noqa: E402

pytestmark = pytest.mark.gpu

IDX = {('heavy', '3f'): (0, 5, 9), ('heavy', '2f'): (0, 7, 15), ('mars_skew', '3f'): (5, 8, 11),
       ('mars_skew', '2f'): (5, 7, 15)}   # golden windows the oracle solves in drop6 with that set
CASES = [(s, v, N, IDX[s, v] if mode == 'drop6' else (0, 1, 2), mode) for s in ('heavy', 'mars_skew')
         for v in ('3f', '2f') for N, mode in ((3, 'plain'), (3, 'drop6'), (10, 'plain'), (10, 'drop6'), (30, 'plain'))]
IDS = ['-'.join(map(str, (c[0], c[1], c[2], c[4]))) for c in CASES]
UREF = {'plain': 'aliased', 'drop6': 'per_stage'}   # test_gpu_kkt's pairing of mode and u_ref semantics
post = pytest.mark.parametrize('cset,variant,N,idx,mode', CASES, ids=IDS)


def test_inputs_hold_what_the_modes_are_for():
    """CPU only, from the oracle's points (shared with the tests below)."""
    refs = [(c, *sens.reference(c[1], c[2], c[3], c[4], frozen(c[0]))) for c in CASES]
    assert not any(r['singular'].any() for _, _, r in refs)
    for s in ('heavy', 'mars_skew'):
        for v in ('3f', '2f'):
            mine = [(i, r) for c, i, r in refs if c[:2] == (s, v)]
            assert max(r['zrows'].max() for _, r in mine) >= 1
            assert any((np.abs(r['u'][:, :, 2] - 206.0) <= 1e-6).any() for _, r in mine)
            assert any(((i['C'] != 0) & (np.abs(r['u'][:, :, 2]) <= 1e-8)).any() for i, r in mine)
            assert any((i['C'] == 0).any() for i, _ in mine)


@post
def test_kkt(cset, variant, N, idx, mode):
    kkt.test_duals_from_the_exact_primal(variant, N, idx, UREF[mode], mode, frozen(cset))


@post
def test_sens(cset, variant, N, idx, mode):
    sens.test_jacobian_at_the_exact_primal(variant, N, idx, mode, frozen(cset))


@post
def test_vjp(cset, variant, N, idx, mode):
    vjp.test_gradients_at_the_exact_primal(variant, N, idx, mode, frozen(cset))


@post
def test_vjp_lin(cset, variant, N, idx, mode):
    vjp_lin.test_gradients_at_the_exact_primal(variant, N, idx, mode, frozen(cset))


@pytest.mark.parametrize('n,B,layout', [(1, 1, 'dense'), (3, 5, 'shared'), (20, 8, 'dense')])
def test_plant(n, B, layout):
    """plant_device against oracle/hmpc_plant.py's rk4_normalized and convert, robot by robot."""
    from oracle import hmpc_plant as pl
    c = plant_vjp.consts(frozen('heavy'))
    X0, U, pf, _ = plant_vjp.inputs(n, B, 300 * n + B)
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    Ud, Us, pfd, pfs = cu(U), 6, cu(pf), (3 * n, 3)
    if layout == 'shared':   # U: row 0 of a (B,10,6) block; pf: one (n,3) plan for the batch
        pf = np.repeat(pf[:1], B, 0)
        Ud, Us, pfd, pfs = cu(np.concatenate([U[:, None], np.zeros((B, 9, 6))], 1)), 60, cu(pf[0]), (0, 3)
    X, hist = cu(X0), torch.empty((B, n, 13), dtype=torch.float64, device='cuda')
    xo = torch.empty((B, 12), dtype=torch.float64, device='cuda')
    plant_vjp.ctx_for('3f', 10, frozen('heavy')).plant_device(X, Ud, Us, pfd, *pfs, n, plant_vjp.DT, c['J'], X_hist=hist,
                                                             x_out=xo)
    torch.cuda.synchronize()
    H, xo = hist.cpu().numpy(), xo.cpu().numpy()
    for b in range(B):
        Xr = X0[b].copy()
        for s in range(n):
            Xr = pl.rk4_normalized(Xr, U[b], pf[b, s], plant_vjp.DT, c['m'], c['g'], c['J'], c['rh'])
            np.testing.assert_allclose(H[b, s], Xr, rtol=0, atol=1e-11)
        np.testing.assert_allclose(xo[b], pl.convert(Xr), rtol=0, atol=1e-12)
    np.testing.assert_array_equal(X.cpu().numpy(), H[:, -1])


@pytest.mark.parametrize('n,B,cots,layout', [(1, 1, 'X', 'dense'), (3, 5, 'Xxh', 'shared'), (20, 8, 'Xxh', 'dense')])
def test_plant_vjp(n, B, cots, layout):
    plant_vjp.test_gradients(n, B, cots, layout, frozen('heavy'))


@pytest.mark.parametrize('n,B,flags,layout', [(1, 1, 0, 'dense'), (3, 5, plant_fb.INTERP, 'strided'),
                                              (20, 8, plant_fb.CLIP | plant_fb.INTERP, 'dense')])
def test_plant_fb(n, B, flags, layout):
    plant_fb.test_against_reference(n, B, flags, layout, frozen('heavy'))
