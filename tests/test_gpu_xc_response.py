"""'b88,' and 'lda,vwn' multigrid response on the device: the fused kernel isdf_gga_b88_fxc and isdf_xc_fxc_apply against their
numpy restatement (tests/test_xc_response.py), the response functions against derivatives of the SCF surface, the response
generators, and second-order SCF through them reaching the reference's Newton energies (pyscf/pbc/scf/test/test_newton.py)
quadratically."""
import numpy as np
import pytest
import scipy.linalg
from pyscf_isdf_amd import gto
from pyscf_isdf_amd import multigrid as pmg
import newton_helpers
import scf_helpers
from test_xc_response import (SYM4, b88_fxc, vwn_fxc, _sample_points, cell_he_split, check_b88_gamma, check_b88_kpts, check_vwn,
                              check_generators)

pytestmark = pytest.mark.gpu


def _device_df(cell, **kw):
    df = pmg.MultiGridFFTDF(cell, **kw)
    df.split = 'all'
    return df


@pytest.mark.parametrize('nset', [1, 3, 17])
def test_fused_b88_kernel_matches_numpy(nset):
    df = _device_df(cell_he_split())
    be = df.backend
    rho, grad = _sample_points()
    rng = np.random.default_rng(nset)
    G = 4096                                           # more than one block, and a ragged tail
    r = np.abs(rng.standard_normal(G)) * 2.0
    r[:rho.size] = rho
    r[rho.size:rho.size + 3] = [0.0, 1e-15, 1e-13]
    g = rng.standard_normal((3, G)) * r ** 1.2
    g[:, :rho.size] = grad
    G -= 37
    r, g = r[:G], g[:, :G]
    rho0 = np.ascontiguousarray(np.concatenate([r[None], g]))
    rho1 = rng.standard_normal((4, nset, G))
    f = b88_fxc(r, g)
    ref = np.einsum('xng,xyg->yng', rho1, f)
    d0, d1 = be.to_device(rho0), be.to_device(rho1)
    wv, f10 = be.empty((4, nset, G)), be.empty((10, G))
    be.gga_b88_fxc(d0, d1, wv, fxc=f10)
    wv = be.to_host(wv)
    for y in range(4):
        assert abs(wv[y] - ref[y]).max() <= 1e-12 * abs(ref[y]).max(), y
    f10 = be.to_host(f10)
    assert abs(f10[SYM4] - f).max() <= 1e-12 * abs(f).max()
    # the written-out components through the generic contraction give the same wv
    fd = be.to_device(np.ascontiguousarray(f10[SYM4]))
    wv2 = be.empty((4, nset, G))
    be.xc_fxc_apply(fd, d1, wv2)
    assert abs(be.to_host(wv2) - wv).max() <= 1e-13 * abs(wv).max()
    # strided views: every other response density, and accumulation
    wv3 = be.zeros((4, nset, G))
    be.xc_fxc_apply(fd, d1[:, ::2], wv3[:, ::2])
    be.xc_fxc_apply(fd, d1[:, ::2], wv3[:, ::2], accumulate=True)
    assert abs(be.to_host(wv3)[:, ::2] - 2 * wv[:, ::2]).max() <= 1e-13 * abs(wv).max()
    assert nset == 1 or abs(be.to_host(wv3)[:, 1::2]).max() == 0


def test_vwn_fxc_kernel_matches_numpy():
    df = _device_df(cell_he_split())
    be = df.backend
    rho = np.concatenate([[0.0, 1e-30, 1e-6, 1e-3], np.abs(np.random.default_rng(1).standard_normal(1000)) * 3])
    f = be.to_device(np.full(rho.size, 0.25))
    be.lda_vwn_fxc_add(be.to_device(rho), f)
    ref = 0.25 + vwn_fxc(rho)
    assert abs(be.to_host(f) - ref).max() <= 1e-13 * abs(ref).max()


def test_gpu_b88_response_gamma():
    cell = cell_he_split()
    check_b88_gamma(_device_df(cell), cell)


def test_gpu_b88_response_kpts():
    cell = cell_he_split()
    check_b88_kpts(_device_df(cell), cell)


def test_gpu_lda_vwn_response_and_refusals():
    cell = cell_he_split()
    check_vwn(_device_df(cell), cell)


def test_gpu_response_generators():
    cell = cell_he_split()
    check_generators(_device_df(cell), cell)


# ---- second-order SCF -------------------------------------------------------------------------------------------------------
def _diamond_newton_cell():
    # pyscf/pbc/scf/test/test_newton.py:25-44 (as tests/test_gpu_scf.py)
    return gto.Cell(unit='B', atom='C 0. 0. 0.; C 1.68506879 1.68506879 1.68506879',
                    a=[[0., 3.37013758, 3.37013758], [3.37013758, 0., 3.37013758], [3.37013758, 3.37013758, 0.]],
                    basis='gth-szv', pseudo='gth-pade', mesh=[19] * 3)


class _MF:
    def __init__(self, df, xc, kpts):
        self.with_df, self.xc, self.kpts = df, xc, kpts


def _rks_problem(cell, xc):
    """hcore, S, e_nuc, the converged 'lda,' orbitals, fock_energy and make_response of a Gamma-point RKS with ``xc``."""
    S, T = scf_helpers.overlap_kinetic_from_ft(cell)
    df = _device_df(cell)
    hcore = T + df.get_pp()
    e_nuc = scf_helpers.ewald_energy(cell)

    def veff(xc_):
        def fn(dm):
            n, exc, v = pmg.nr_rks(df, xc_, dm, with_j=True)
            return np.asarray(v), float(v.ecoul), float(exc)
        return fn
    _, dm = scf_helpers.rks(hcore, S, veff('lda,'), 4, e_nuc)
    C = scipy.linalg.eigh(hcore + veff('lda,')(dm)[0], S)[1]

    def fock_energy(D):
        n, exc, v = pmg.nr_rks(df, xc, D[0], with_j=True)
        return np.einsum('ij,ji', hcore, D[0]) + v.ecoul + exc + e_nuc, (hcore + np.asarray(v))[None]

    def make_response(D):
        vind = pmg._gen_rhf_response(_MF(df, xc, np.zeros((1, 3))), D[0], hermi=1)
        return lambda D1: vind(D1[:, 0])[:, None]
    return df, C, fock_energy, make_response


def _report(tag, hist):
    print('%s: %s' % (tag, ' '.join('E=%.12f |g|=%.2e' % h for h in hist)))


def test_newton_rks_b88_reaches_reference_quadratically():
    # pyscf/pbc/scf/test/test_newton.py:99-105: RKS 'b88,' through newton(), e_tot = -9.9355341416893559
    cell = _diamond_newton_cell()
    df, C, fock_energy, make_response = _rks_problem(cell, 'b88,')
    e, _, hist = newton_helpers.newton(newton_helpers.rotated(C[None], 4, KICK), 4, 2.0, 1, fock_energy, make_response, max_iter=6)
    _report('RKS b88', hist)
    newton_helpers.assert_quadratic(hist, c_max=NEWTON_C, g_start=5e-2)
    assert len(hist) <= NEWTON_STEPS + 1
    assert abs(e - (-9.9355341416893559)) < 5e-8


def test_newton_uks_b88_reaches_reference_quadratically():
    # test_newton.py:107-113: UKS 'b88,' of the same closed-shell cell, e_tot = -9.9355341416893559
    cell = _diamond_newton_cell()
    df, C, _, _ = _rks_problem(cell, 'b88,')
    S, T = scf_helpers.overlap_kinetic_from_ft(cell)
    hcore = T + df.get_pp()
    e_nuc = scf_helpers.ewald_energy(cell)

    def fock_energy(D):
        n, exc, v = pmg.nr_uks(df, 'b88,', D, with_j=True)
        return np.einsum('ij,sji->', hcore, D) + v.ecoul + exc + e_nuc, hcore + np.asarray(v)

    def make_response(D):
        vind = pmg._gen_uhf_response(_MF(df, 'b88,', np.zeros((1, 3))), D)

        def fn(D1):
            n = len(D1)
            v = vind(np.concatenate([D1[:, 0], D1[:, 1]]))
            return np.stack([v[:n], v[n:]], axis=1)
        return fn
    e, _, hist = newton_helpers.newton(newton_helpers.rotated(np.array([C, C]), 4, KICK), 4, 1.0, 1, fock_energy, make_response, max_iter=6)
    _report('UKS b88', hist)
    newton_helpers.assert_quadratic(hist, c_max=NEWTON_C, g_start=5e-2)
    assert len(hist) <= NEWTON_STEPS + 1
    assert abs(e - (-9.9355341416893559)) < 5e-8


def test_newton_krks_b88_reaches_reference_quadratically():
    # test_newton.py:151-157: KRKS 'b88,' with a [2,1,1] k-mesh, e_tot = -10.446717855794008
    cell = _diamond_newton_cell()
    kpts = cell.make_kpts([2, 1, 1])
    S, T = scf_helpers.overlap_kinetic_from_ft_kpts(cell, kpts)
    df = _device_df(cell, kpts=kpts)
    hcore = T + np.asarray(df.get_pp(kpts))
    e_nuc = scf_helpers.ewald_energy(cell)
    nk = len(kpts)

    def veff_lda(dms):
        n, exc, v = pmg.nr_rks(df, 'lda,', dms, kpts=kpts, with_j=True)
        return np.asarray(v), float(v.ecoul), float(exc)
    _, dms = scf_helpers.krks(hcore, S, veff_lda, 4, e_nuc)
    f = hcore + veff_lda(dms)[0]
    C = np.array([scipy.linalg.eigh(f[k], S[k])[1] for k in range(nk)])

    def fock_energy(D):
        n, exc, v = pmg.nr_rks(df, 'b88,', D, kpts=kpts, with_j=True)
        return np.einsum('kij,kji', hcore, D).real / nk + v.ecoul + exc + e_nuc, hcore + np.asarray(v)

    def make_response(D):
        return pmg._gen_rhf_response(_MF(df, 'b88,', kpts), D, hermi=1)
    e, _, hist = newton_helpers.newton(C, 4, 2.0, nk, fock_energy, make_response, max_iter=6)
    _report('KRKS b88', hist)
    newton_helpers.assert_quadratic(hist, c_max=NEWTON_C, g_start=5e-2)
    assert len(hist) <= NEWTON_STEPS + 1
    assert abs(e - (-10.446717855794008)) < 5e-8


def test_newton_rks_lda_vwn_reaches_reference():
    # RKS 'lda,vwn' on the cell of pyscf/pbc/dft/test/test_krks.py:59-71,112-119: e_tot = -10.221426445656439
    cell = gto.Cell(unit='A', atom='C 0. 0. 0.; C 0.8917 0.8917 0.8917', a=[[0., 1.7834, 1.7834], [1.7834, 0., 1.7834], [1.7834, 1.7834, 0.]],
                    basis='gth-szv', pseudo='gth-pade', mesh=[17] * 3)
    df, C, fock_energy, make_response = _rks_problem(cell, 'lda,vwn')
    e, _, hist = newton_helpers.newton(newton_helpers.rotated(C[None], 4, KICK), 4, 2.0, 1, fock_energy, make_response, max_iter=6)
    _report('RKS lda,vwn', hist)
    newton_helpers.assert_quadratic(hist, c_max=NEWTON_C, g_start=5e-2)
    assert abs(e - (-10.221426445656439)) < 5e-8


# Measured on MI355X (|g| at each visited point; the ratio is |g_(k+1)| / |g_k|^2):
#   RKS  b88      3.75e-02 -> 3.53e-05 -> 2.80e-11   (0.025, 0.022)
#   UKS  b88      1.63e-02 -> 1.89e-05 -> 1.84e-11   (0.071, 0.052)
#   KRKS b88      3.28e-02 -> 4.37e-05 -> 1.02e-10   (0.041, 0.053)
#   RKS  lda,vwn  3.79e-02 -> 2.80e-06 -> 3.98e-15   (0.002)
# C = 0.5 leaves a factor 7 over the largest ratio; a kernel that is not the exact second derivative converges linearly and fails it.
NEWTON_C = 0.5
NEWTON_STEPS = 2
KICK = 0.002            # start: the converged 'lda,' orbitals rotated by this much per element (|g| ~ 2e-2 .. 4e-2)
