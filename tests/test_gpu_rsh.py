"""CAM-B3LYP in the multigrid XC on the device (-m gpu): isdf_xc_fused_rsh alone against the float64 restatement
(tests/rsh_reference.py, itself pinned by the reference's CAM-B3LYP energies in tests/test_rsh.py), the ladder, the reference's
energies with hybrid_k, a p-shell SCF and the XC force."""
import numpy as np
import pytest
from pyscf_isdf_amd import gto
from pyscf_isdf_amd import multigrid as pmg
from oracle import multigrid as omg, pp as opp
import lyp_reference as lyp
import rsh_reference as rsh
import scf_helpers
import xc_grad_reference as xr
from test_multigrid import cell_he_split, cell_c2_orth, dense_ao4, make_dm
from test_lyp import memoised_collocation  # noqa: F401  (the fixture serves this module too)
from test_gpu_lyp import kernel_points, padded, rel_to_max, NPTS, SENTINEL
from test_xc_grad import cell_he_split_coarse
from test_rsh import check_cam_ladder, check_cam_kpts, check_hybrid_k, cell_he_reference, pair_eris, dense_hybrid_k, HE_PIN
from test_rsh import cam_restatement  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu

WEIGHT_SETS = {'camb3lyp': ((0.0, 0.35, 0.19, 0.81), 0.46), 'sr_b88': ((0.0, 0.0, 0.0, 0.0), 1.0)}
OMEGAS = (0.33, 0.15, 5.0, 1e-3)
_REFS = {}


def kernel_references(name, omega):
    """(float64 restatement, 30-digit evaluation) of (exc, vrho, w) on kernel_points(), computed once per case."""
    if (name, omega) not in _REFS:
        rho, grad = kernel_points()
        coeffs, csr = WEIGHT_SETS[name]
        _REFS[name, omega] = (rsh.xc_weighted_rsh(rho, grad, coeffs, 'V', csr, omega), rsh.xc_weighted_rsh_mp(rho, grad, coeffs, 'V', csr, omega))
    return _REFS[name, omega]


def run_rsh(be, d_rho, d_grad, gbuf, coeffs, rpa, csr, omega):
    e, v = be.empty((NPTS,)), be.empty((NPTS,))
    wbuf, w = padded(be, np.zeros((3, NPTS)))
    be.xc_fused_rsh(d_rho, d_grad, coeffs, rpa, csr, omega, e, v, w)
    assert (be.to_host(wbuf)[:, NPTS:] == SENTINEL).all() and (be.to_host(gbuf)[:, NPTS:] == SENTINEL).all()
    return be.to_host(e), be.to_host(v), be.to_host(w)


@pytest.fixture(scope='module')
def device_points():
    from pyscf_isdf_amd.backend import HipBackend
    be = HipBackend(0)
    rho, grad = kernel_points()
    gbuf, d_grad = padded(be, grad)
    return be, rho, grad, be.to_device(rho), d_grad, gbuf


@pytest.mark.parametrize('omega', OMEGAS)
@pytest.mark.parametrize('name', list(WEIGHT_SETS))
def test_gpu_fused_rsh_kernel_matches_the_restatement(device_points, name, omega):
    """isdf_xc_fused_rsh on the 1031 points of test_gpu_lyp.kernel_points() (five blocks of 256, the last partial; planes strided by
    NPTS + 7, a sentinel behind each, in and out) for the CAM-B3LYP weights and for the short-range B88 alone, omega = 0.33, 0.15,
    5.0 and 1e-3 (a from 1e-5 to 1e5: both forms of the attenuation).  The bound is the rule of the sibling tests: the float64
    restatement is measured against a 30-digit evaluation on these very points and the device gets 10 x that, relative to max|value|
    per output - and again on the 500 physical points alone, so that the extreme reduced gradients cannot hide them.
    Measured (profiles/r20_camb3lyp_pins_and_fused_rsh_kernel.log), (exc, vrho, w), all 1031 points: restatement against 30 digits
    2.0e-15 .. 2.2e-15 / 2.1e-15 .. 2.2e-15 / 9.0e-16 .. 1.0e-15 for the CAM-B3LYP sum at the four omegas (the values at the reduced
    gradients near 1e4, exc 2.7e4 and vrho 4.6e4, set the scale), device against restatement 9.4e-16 / 1.1e-15 / 7.9e-16 .. 9.0e-16;
    short-range B88 alone: restatement 2.0e-16 .. 1.2e-15 / 3.1e-16 .. 1.5e-15 / 4.1e-16 .. 1.1e-15, device 7.3e-17 .. 1.8e-15 / 3.9e-16 ..
    1.7e-15 / 4.1e-16 .. 2.0e-15; the closest case is exc of the short-range B88 at omega 0.33, 1.78e-15 under a bound of 1.19e-14.
    The 500 physical points: restatement 2.2e-16 .. 7.7e-16 (w at omega 5 alone: 2.6e-15), device 1.2e-16 .. 4.8e-16 (2.2e-15 there)."""
    be, rho, grad, d_rho, d_grad, gbuf = device_points
    coeffs, csr = WEIGHT_SETS[name]
    f64, mp = kernel_references(name, omega)
    got = run_rsh(be, d_rho, d_grad, gbuf, coeffs, False, csr, omega)
    for label, g, r, m in zip(('exc', 'vrho', 'w'), got, f64, mp):
        assert np.isfinite(g).all()
        for what, sel in (('all 1031', slice(None)), ('physical 500', slice(0, 500))):
            own, dev = rel_to_max(r[..., sel], m[..., sel]), rel_to_max(g[..., sel], r[..., sel])
            print('%-8s omega %-5g %-4s %-12s restatement vs 30 digits %.2e   device vs restatement %.2e   max|value| %.3e'
                  % (name, omega, label, what, own, dev, abs(m[..., sel]).max()))
            assert dev <= 10 * own, (name, omega, label, what, dev, own)
    if name == 'sr_b88':                                        # a pure GGA set: zero at and below the threshold
        below = rho <= 1e-14
        assert below.sum() > 20 and all(abs(g[..., below]).max() == 0.0 for g in got)


def test_gpu_fused_rsh_kernel_limits(device_points):
    """c_b88_sr = 0 is isdf_xc_fused bit for bit (B3LYP5, BLYP and Slater + VWN weights, whatever omega says); at omega = 1e-10 the
    short-range B88 alone is Becke-88 to within (8/3) sqrt(pi) max(a) relative to max|value| of each output (1 - F <= (8/3) sqrt(pi) a),
    with max(a) computed here from a = omega / (2 k).  Measured: max(a) 7.05e-7, bound 3.33e-6; exc 6.4e-10, vrho 3.7e-9, w 1.6e-6."""
    be, rho, grad, d_rho, d_grad, gbuf = device_points
    for coeffs, rpa in (((.08, .72, .19, .81), False), ((.08, .72, .19, .81), True), ((0, 1, 0, 1), False), ((1, 0, 1, 0), False)):
        got = run_rsh(be, d_rho, d_grad, gbuf, coeffs, rpa, 0.0, 0.33)
        e, v = be.empty((NPTS,)), be.empty((NPTS,))
        wbuf, w = padded(be, np.zeros((3, NPTS)))
        be.xc_fused(d_rho, d_grad, coeffs, rpa, e, v, w)
        for g, x in zip(got, (e, v, w)):
            assert np.array_equal(g, be.to_host(x))
    omega = 1e-10
    ok = rho > 1e-14
    G = -rho[ok] * lyp.b88_point(lyp._NP, rho[ok], (grad[:, ok] ** 2).sum(axis=0))[0] / (2 * (rho[ok] / 2) ** (4. / 3.))     # -G(x) = K / 2
    a_max = (omega / (2 * np.sqrt(9 * np.pi / (2 * G)) * np.cbrt(rho[ok] / 2))).max()
    bound = 8 * np.sqrt(np.pi) / 3 * a_max
    got = run_rsh(be, d_rho, d_grad, gbuf, (0, 0, 0, 0), False, 1.0, omega)
    e0, v0, w0 = be.empty((NPTS,)), be.empty((NPTS,)), be.empty((3, NPTS))
    be.gga_b88(d_rho, d_grad, e0, v0, w0)
    print('omega 1e-10: max(a) %.3e  bound %.3e  exc %.2e vrho %.2e w %.2e' % ((a_max, bound) + tuple(rel_to_max(g, be.to_host(x)) for g, x in zip(got, (e0, v0, w0)))))
    assert 1e-8 < a_max < 1e-4
    for g, x in zip(got, (e0, v0, w0)):
        assert 0 < rel_to_max(g, be.to_host(x)) <= bound


@pytest.mark.parametrize('mk', [cell_he_split, cell_c2_orth])
def test_gpu_multigrid_camb3lyp_ladder(mk):
    """The checks of test_rsh.check_cam_ladder on the device at the tolerance of test_gpu_multigrid_lyp_ladder (1e-9)."""
    cell = mk()
    df = pmg.MultiGridFFTDF(cell)
    df.split = 'all'
    check_cam_ladder(df, cell, 1e-9)
    assert not df._built


@pytest.mark.parametrize('mk', [cell_he_split, cell_c2_orth])
def test_gpu_multigrid_camb3lyp_kpts(mk):
    """The checks of test_rsh.check_cam_kpts on the device at 1e-9, on both cells (cell_c2_orth with the functional's own omega
    alone, as on the CPU: the reference side is the oracle's complex collocation of eight levels)."""
    cell = mk()
    df = pmg.MultiGridFFTDF(cell)
    df.split = 'all'
    check_cam_kpts(df, cell, 1e-9, (None, 0.15) if mk is cell_he_split else (None,))


@pytest.fixture(scope='module')
def he_device():
    """The He cell of pbc/dft/test/test_rks.py:28-36 at 69^3 with its analytic S and T, the device object (c_isdf = 2: the fit of two
    s functions' three pair products is exact) and hcore = T + get_nuc."""
    cell = cell_he_reference()
    S, T = scf_helpers.s_type_overlap_kinetic(cell)
    df = pmg.MultiGridFFTDF(cell, c_isdf=2, select='global')
    return cell, S, T + df.get_nuc(), df


@pytest.mark.parametrize('omega', [None, 0.15])
def test_gpu_he_camb3lyp_total_energy_matches_reference(he_device, omega):
    """RKS 'camb3lyp' on the reference's He cell (test_rks.py:135-143, test_krks.py:131-136; places=7): e_tot = -2.4745140703871877
    and, with omega = .15, -2.476617717375184, within 2e-7 (the bound test_gpu_scf.py uses for the same places).  XC and J from ONE
    nr_rks call, the exchange from hybrid_k (K and K_LR from the ISDF fit, both probe-charge terms).
    Measured (profiles/r20_camb3lyp_pins_and_fused_rsh_kernel.log): 2.65e-9 and 2.93e-9 Eh from the constants, the all-CPU SCF's own
    deviations (tests/test_rsh.py) to their last digit."""
    cell, S, hcore, df = he_device

    def veff(dm):
        n, exc, v = pmg.nr_rks(df, 'camb3lyp', dm, with_j=True, omega=omega)
        vx = pmg.hybrid_k(df, 'camb3lyp', dm, omega=omega)
        return np.asarray(v) - .5 * vx, float(v.ecoul), float(exc) - .25 * np.einsum('ij,ji', vx, dm)
    e_tot = scf_helpers.rks(hcore, S, veff, 1, scf_helpers.ewald_energy(cell))[0]
    print('He camb3lyp omega %s: e_tot %.10f  deviation %.2e' % (omega, e_tot, e_tot - HE_PIN[omega or 0.33]))
    assert abs(e_tot - HE_PIN[omega or 0.33]) < 2e-7


def test_gpu_hybrid_k_matches_the_dense_combination(he_device):
    cell, S, hcore, df = he_device
    check_hybrid_k(df, cell)


def test_gpu_diamond_camb3lyp_scf_matches_the_cpu_restatement():
    """'camb3lyp' on the diamond primitive cell of test_gpu_lyp.test_gpu_diamond_b3lyp5_scf_matches_the_cpu_restatement (gth-szv /
    gth-pade, 19^3; p shells): Fock = hcore + J + v_xc - hybrid_k / 2 from the device against an all-CPU SCF of the restatement
    (dense quadrature, J / K / K_LR from the 64 pair densities by FFT, both Madelung terms), at that test's 5e-8."""
    cell = gto.Cell(unit='B', atom='C 0. 0. 0.; C 1.68506879 1.68506879 1.68506879',
                    a=[[0., 3.37013758, 3.37013758], [3.37013758, 0., 3.37013758], [3.37013758, 3.37013758, 0.]],
                    basis='gth-szv', pseudo='gth-pade', mesh=[19] * 3)
    S, T = scf_helpers.overlap_kinetic_from_ft(cell)
    e_nuc = scf_helpers.ewald_energy(cell)
    omega, alpha, hyb = pmg.rsh_and_hybrid_coeff('camb3lyp')
    df = pmg.MultiGridFFTDF(cell, c_isdf=6, select='global')
    df.split = 'all'
    df.select_tol = 0.0
    hcore = T + df.get_pp()

    def veff_dev(dm):
        n, exc, v = pmg.nr_rks(df, 'camb3lyp', dm, with_j=True)
        vx = pmg.hybrid_k(df, 'camb3lyp', dm)
        return np.asarray(v) - .5 * vx, float(v.ecoul), float(exc) - .25 * np.einsum('ij,ji', vx, dm)
    e_dev = scf_helpers.rks(hcore, S, veff_dev, 4, e_nuc)[0]
    a, mesh = cell.lattice_vectors(), cell.mesh
    ao4 = dense_ao4(cell)
    ps = [cell._pseudo.get(cell.atom_symbol(i)) for i in range(cell.natm)]
    vpp = opp.get_pp(cell._atm, cell._bas, cell._env, cell.atom_coords(), cell.atom_charges(), ps, a, mesh,
                     cell.get_uniform_grids(), [ao4[0]], np.zeros((1, 3)))[0].real
    eri, eri_lr = pair_eris(ao4[0], a, mesh), pair_eris(ao4[0], a, mesh, omega)

    def veff_cpu(dm):
        vj = np.einsum('ijkl,lk->ij', eri, dm)
        vx = dense_hybrid_k(eri, eri_lr, dm, S, cell, omega, alpha, hyb)
        with lyp.oracle_gga(rsh.functional('camb3lyp')):
            n, exc, vxc = omg.nr_rks_b88_dense(ao4, dm, a, mesh)
        return vj + vxc - .5 * vx, 0.5 * np.einsum('ij,ji', vj, dm), exc - .25 * np.einsum('ij,ji', vx, dm)
    e_cpu = scf_helpers.rks(T + vpp, S, veff_cpu, 4, e_nuc)[0]
    print('diamond camb3lyp: device %.10f  cpu %.10f  diff %.2e' % (e_dev, e_cpu, e_dev - e_cpu))
    assert abs(e_dev - e_cpu) < 5e-8


def test_gpu_camb3lyp_force_and_matrix_match_the_restatement(cam_restatement):
    """xc_nuc_grad and get_vxc_e1 of 'camb3lyp' (and with omega = 0.15) on the device, one level, on the smallest force cell of
    tests/test_xc_grad.py, against the CPU restatement tests/test_rsh.py checks by central differences: 1e-9 of the largest entry,
    the tolerance of tests/test_gpu_xc_grad.py."""
    su = xr.CellSetup(cell_he_split_coarse())
    dm, ao10 = make_dm(su.cell), su.ao10()
    df = pmg.MultiGridFFTDF(su.cell)
    df.max_levels = 1
    rel = lambda x, ref: float(abs(x - ref).max() / abs(ref).max())
    for omega in (None, 0.15):
        tag = 'camb3lyp' if omega is None else 'camb3lyp@%s' % omega
        F, e1 = pmg.xc_nuc_grad(df, 'camb3lyp', dm, omega=omega), pmg.get_vxc_e1(df, 'camb3lyp', dm, omega=omega)
        Fr, er = xr.xc_nuc_grad(ao10, dm, tag, su.weight, su.aoslices), xr.get_vxc_e1(ao10, dm, tag, su.weight)
        print('camb3lyp omega %s: force %.3e, matrix %.3e' % (omega, rel(F, Fr), rel(e1, er)))
        assert len(df.tasks) == 1 and F.shape == Fr.shape and e1.shape == er.shape
        assert rel(F, Fr) < 1e-9 and rel(e1, er) < 1e-9
        assert rel(xr.contract_e1(e1, dm, su.aoslices), F) < 1e-9
