"""CAM-B3LYP in the multigrid XC: the short-range Becke-88 exchange, the hybrid K helper and the attenuated Madelung constant (CPU
half, -m "not gpu").

Trust chain, as for LYP: (1) the reference's CAM-B3LYP total energies of a one-atom He cell (pbc/dft/test/test_rks.py:135-143,
test_krks.py:131-136) pin the closed-form restatement tests/rsh_reference.py - the ITYH attenuation, the weights, VWN fit V, the
exact-exchange combination and the attenuated probe-charge term (libxc is not part of this tree); (2) the restatement pins the
device kernel (tests/test_gpu_rsh.py); (3) the ladder is compared with the dense quadrature.  Here: (1), the attenuation against 30
digits, the restatement's derivatives against central differences of the 30-digit energy density, and the product's orchestration on
the CPU checker backend."""
import numpy as np
import pytest
from scipy.special import erfc
from pyscf_isdf_amd import gto, kpts_symm
from pyscf_isdf_amd import multigrid as pmg
from oracle import multigrid as omg, pbc_tools as otools
import lyp_reference as lyp
import rsh_reference as rsh
import scf_helpers
import xc_grad_reference as xr
from test_multigrid import cell_he_split, cell_c2_orth, make_dm, as_tasks, dense_ao4, make_kpts_dms
from test_lyp import random_points, memoised_collocation  # noqa: F401  (the fixture serves this module too)
from test_xc_grad import coarse, H  # noqa: F401  (the displaced collocations of the smallest force cell)

CAM_CODES = ('camb3lyp', 'CAM-B3LYP', 'cam_b3lyp', 'HYB_GGA_XC_CAM_B3LYP', ' Cam B3lyp ')
HE_PIN = {0.33: -2.4745140703871877, 0.15: -2.476617717375184}        # test_rks.py:135-143 (places=7); the first also test_krks.py:131-136


# ---- the attenuation ---------------------------------------------------------------------------------------------------------------
def test_attenuation_matches_30_digits():
    """F and dF/da in float64 (direct form below a = 0.5, 16 series terms from there) against the closed form at 30 digits on 400
    log-spaced a from 1e-4 to 1e4: 1e-14 relative.  Measured: F 2.9e-15, dF/da 2.1e-15, both in the direct form just below the
    switch (the series part is at 3.3e-16; a switch at 0.75 would leave dF/da at 1.4e-14).  The first five series coefficients are
    the ones of the 60-digit expansion, and the two forms agree where they meet."""
    m, mpf = rsh._mp(30)
    a = np.logspace(-4, 4, 400)
    ref = [rsh.attenuation(m, mpf(float(x))) for x in a]
    F0, dF0 = np.array([float(r[0]) for r in ref]), np.array([float(r[1]) for r in ref])
    F, dF = rsh.attenuation(rsh._NP, a)
    eF, edF = abs(F / F0 - 1).max(), abs(dF / dF0 - 1).max()
    print('F %.2e  dF/da %.2e  (a < %.2f: %d points)' % (eF, edF, rsh.A_SWITCH, (a < rsh.A_SWITCH).sum()))
    assert eF < 1e-14 and edF < 1e-14
    assert (F > 0).all() and (dF < 0).all() and (np.diff(F) < 0).all()
    for n, den in zip(range(1, 6), (36, -960, 26880, -829440, 28385280)):
        assert abs(rsh.series_coefficient(n) * den - 1) < 4e-16
    s = np.array([rsh.A_SWITCH])
    for x, y in zip(rsh.attenuation_direct(rsh._NP, s), rsh.attenuation_series(rsh._NP, s)):
        assert abs(x / y - 1).max() < 1e-14
    # the limits: F(0) = 1 (the exponential underflows harmlessly), F -> 1/(36 a^2)
    F, dF = rsh.attenuation(rsh._NP, np.array([0.0, 1e-200, 1e4]))
    assert F[0] == 1.0 and F[1] == 1.0 and abs(dF[0] + 8 * np.sqrt(np.pi) / 3) < 1e-15 and abs(F[2] * 36e8 - 1) < 1e-9


@pytest.mark.parametrize('omega', [0.33, 0.15])
def test_short_range_b88_closed_form_derivatives(omega):
    """vrho and w of the short-range B88 on test_lyp.random_points() against central differences of the 30-digit energy density
    rho exc.  At 30 digits a step of 1e-8 of the variable leaves the quotient exact to about 1e-15, so the bound is the float64
    restatement's own rounding: 1e-12 relative to max|value|.  Measured: vrho 3e-16, w 2e-16 at both omegas."""
    rho, grad = random_points()
    g = np.sqrt((grad ** 2).sum(axis=0))
    exc, vrho, w = rsh.b88_sr_exchange(rho, grad, omega)
    m, mpf = rsh._mp(30)
    om = mpf(omega)

    def e(r, gg):
        return r * rsh.b88_sr_point(m, r, gg * gg, om)[0]
    fd_r, fd_g, e0 = np.empty(len(rho)), np.empty(len(rho)), np.empty(len(rho))
    for i in range(len(rho)):
        r, gg = mpf(float(rho[i])), mpf(float(g[i]))
        hr, hg = r * mpf('1e-8'), gg * mpf('1e-8')
        e0[i] = float(e(r, gg))
        fd_r[i] = float((e(r + hr, gg) - e(r - hr, gg)) / (2 * hr))
        fd_g[i] = float((e(r, gg + hg) - e(r, gg - hg)) / (2 * hg))
    wref = fd_g[None] * grad / g
    print('omega %.2f: e %.2e vrho %.2e w %.2e' % (omega, abs(rho * exc - e0).max() / abs(e0).max(), abs(vrho - fd_r).max() / abs(fd_r).max(),
                                                 abs(w - wref).max() / abs(wref).max()))
    assert abs(rho * exc - e0).max() < 1e-12 * abs(e0).max()
    assert abs(vrho - fd_r).max() < 1e-12 * abs(fd_r).max()
    assert abs(w - wref).max() < 1e-12 * abs(wref).max()
    # omega -> 0 is Becke-88 itself; below the threshold: zeros; the weighted sum adds the term
    b = omg.b88_exchange(rho, grad)
    for x, y in zip(rsh.b88_sr_exchange(rho, grad, 1e-14), b):                      # 1 - F = (8/3) sqrt(pi) a, a about omega
        assert abs(x - y).max() < 1e-11 * abs(y).max()
    out = rsh.b88_sr_exchange(np.array([0.0, -1e-3, 1e-14, 5e-15]), np.ones((3, 4)), omega)
    assert all(abs(o).max() == 0.0 for o in out)
    full = rsh.xc_weighted_rsh(rho, grad, (0, .35, .19, .81), 'V', .46, omega)
    base = lyp.xc_weighted(rho, grad, (0, .35, .19, .81), 'V')
    for x, y, z in zip(full, base, (exc, vrho, w)):
        assert np.array_equal(x, y + .46 * z)


# ---- the pin -----------------------------------------------------------------------------------------------------------------------
def cell_he_reference(mesh=69):
    """pbc/dft/test/test_rks.py:28-36: one He in a 4 A cube, two s primitives; 69^3 is the reference's mesh at its precision 1e-8
    (ke_cutoff 383.10)."""
    return gto.Cell(unit='A', a=np.eye(3) * 4, atom=[['He', (2., 2., 3.)]], basis=[[0, (4.0, 1.0)], [0, (1.0, 1.0)]], mesh=[mesh] * 3)


def pair_eris(ao, a, mesh, omega=None):
    """(ij|kl) of real AOs (G, nao) on the mesh, from the FFTs of the nao^2 pair densities with the Coulomb kernel (omega: its
    long-range part), G = 0 dropped."""
    G, nao = ao.shape
    pairs = np.einsum('gi,gj->ijg', ao, ao).reshape(nao * nao, G)
    vR = otools.ifft(otools.fft(pairs, mesh) * otools.get_coulG(a, mesh, omega=omega), mesh).real
    return (abs(np.linalg.det(a)) / G * pairs.dot(vR.T)).reshape(nao, nao, nao, nao)


def nuclear_attraction(cell, ao):
    """FFTDF.get_nuc (pbc/df/fft.py:39-62) in numpy."""
    a, mesh = cell.lattice_vectors(), cell.mesh
    Gv = otools.get_Gv(2 * np.pi * np.linalg.inv(a.T), mesh)
    rhoG = -np.asarray(cell.atom_charges(), dtype=float).dot(np.exp(-1j * cell.atom_coords().dot(Gv.T)))
    vR = np.fft.ifftn((rhoG * otools.get_coulG(a, mesh)).reshape(*mesh)).real.ravel()
    return ao.T.dot(vR[:, None] * ao)


def dense_hybrid_k(eri, eri_lr, dm, S, cell, omega, alpha, hyb, ewald=True):
    """hyb K + (alpha - hyb) K_LR from the dense integrals, each with its probe-charge term."""
    sds = S.dot(dm).dot(S) if ewald else 0.0
    vk = np.einsum('ikjl,kl->ij', eri, dm) + gto.madelung(cell) * sds
    vklr = np.einsum('ikjl,kl->ij', eri_lr, dm) + gto.madelung(cell, omega=omega) * sds
    return hyb * vk + (alpha - hyb) * vklr


def he_cpu_scf(cell, omega):
    """All-CPU closed-shell SCF of the He cell: the dense quadrature of the restatement, J, K and K_LR from the four AO pair
    densities by FFT, both Madelung terms with the analytic overlap (as the reference's get_k has them).  (e_tot, dm)."""
    a, mesh = cell.lattice_vectors(), cell.mesh
    S, T = scf_helpers.s_type_overlap_kinetic(cell)
    ao4 = dense_ao4(cell)
    eri, eri_lr = pair_eris(ao4[0], a, mesh), pair_eris(ao4[0], a, mesh, omega)
    _, _, _, om0, alpha, hyb = rsh.CAM_B3LYP

    def veff(dm):
        vj = np.einsum('ijkl,lk->ij', eri, dm)
        vx = dense_hybrid_k(eri, eri_lr, dm, S, cell, omega, alpha, hyb)
        with lyp.oracle_gga(rsh.functional('camb3lyp', omega)):
            n, exc, vxc = omg.nr_rks_b88_dense(ao4, dm, a, mesh)
        return vj + vxc - .5 * vx, .5 * np.einsum('ij,ji', vj, dm), exc - .25 * np.einsum('ij,ji', vx, dm)
    return scf_helpers.rks(T + nuclear_attraction(cell, ao4[0]), S, veff, 1, scf_helpers.ewald_energy(cell))


@pytest.mark.parametrize('omega', [0.33, 0.15])
def test_restatement_scf_reproduces_the_reference_camb3lyp_energies(omega):
    """'camb3lyp' on the He cell of test_rks.py at 69^3: e_tot = -2.4745140703871877 and, with mf.omega = .15, -2.476617717375184, to
    the reference's 7 places (5e-8).  Measured deviations: 2.6e-9 and 2.9e-9.  madelung = 0.3753582916854751,
    xi_0.33 = 0.3088965244914323, xi_0.15 = 0.16913976241701825."""
    cell = cell_he_reference()
    assert cell.nao_nr() == 2 and cell.nelectron == 2
    assert abs(gto.madelung(cell) - 0.3753582916854751) < 1e-12
    assert abs(gto.madelung(cell, omega=omega) - {0.33: 0.3088965244914323, 0.15: 0.16913976241701825}[omega]) < 1e-12
    e_tot = he_cpu_scf(cell, omega)[0]
    print('He camb3lyp omega %.2f: e_tot %.10f  deviation %.2e' % (omega, e_tot, e_tot - HE_PIN[omega]))
    assert abs(e_tot - HE_PIN[omega]) < 5e-8


# ---- madelung(omega) ---------------------------------------------------------------------------------------------------------------
def _madelung_cells():
    rng = np.random.default_rng(5)
    return [cell_he_reference(9), cell_he_split(), gto.Cell(a=np.eye(3) * 5.1 + rng.random((3, 3)), atom='He 0 0 0', unit='B',
                                                            basis=[[0, (1.0, 1.0)]], mesh=[9] * 3)]


@pytest.mark.parametrize('icell', [0, 1, 2])
def test_attenuated_madelung_is_the_ewald_split_at_eta_omega(icell):
    """madelung(cell) = xi_omega - sum_(T != 0) erfc(omega |T|) / |T| + pi / (omega^2 V): the Ewald split with eta = omega (madelung is
    -2 x the Ewald energy, whose real-space sum enters with +1/2 and whose background term with -pi / (2 eta^2 V)), to 1e-12, for a
    cubic, an orthorhombic and a triclinic cell, omega in {0.15, 0.33, 1.0}, nk = (1,1,1) and (2,2,2); omega = 0 is the old function
    bit for bit."""
    cell = _madelung_cells()[icell]
    for nk in ((1, 1, 1), (2, 2, 2)):
        a = np.einsum('xi,x->xi', cell.lattice_vectors(), np.asarray(nk, dtype=float))
        vol = abs(np.linalg.det(a))
        mad = gto.madelung(cell, nk)
        assert gto.madelung(cell, nk, omega=0.0) == mad and gto.madelung(cell, nk, 0) == mad
        for omega in (0.15, 0.33, 1.0):
            rmax = 9.5 / omega                                                          # erfc(9.5) = 4e-41
            n = np.ceil(rmax * np.linalg.norm(np.linalg.inv(a.T), axis=1)).astype(int) + 1
            r = np.linalg.norm(gto.cartesian_prod([np.arange(-k, k + 1) for k in n]).dot(a), axis=1)
            r = np.sort(r[(r > 1e-12) & (r < rmax)])[::-1]
            rhs = gto.madelung(cell, nk, omega=omega) - (erfc(omega * r) / r).sum() + np.pi / (omega ** 2 * vol)
            print(icell, nk, omega, mad, rhs - mad)
            assert abs(rhs - mad) < 1e-12
    with pytest.raises(ValueError):
        gto.madelung(cell, omega=-0.3)


# ---- the product on the checker backend --------------------------------------------------------------------------------------------
def _df(cell, **kw):
    from rsh_backend import RshOracleBackend
    df = pmg.MultiGridFFTDF(cell, backend=RshOracleBackend(), **kw)
    df.split = 'all'
    return df


def check_cam_ladder(df, cell, tol):
    """nr_rks('camb3lyp') against the restatement on the same ladder (tol, as test_lyp.check_lyp_ladder), the dense quadrature
    (1e-7) and the definition veff = dE_xc/dD; the omega override; the spellings."""
    a, mesh = cell.lattice_vectors(), cell.mesh
    dm = make_dm(cell)
    tasks = as_tasks(df.build_tasks())
    ao4 = dense_ao4(cell)
    vj = df.get_jk(dm, with_k=False)[0]
    results = {}
    for omega in (None, 0.15):
        n, e, veff = pmg.nr_rks(df, 'camb3lyp', dm, with_j=True, return_j=True, omega=omega)
        with lyp.oracle_gga(rsh.functional('camb3lyp', omega)):
            n0, e0, v0, ec0 = omg.nr_rks_b88(tasks, cell._atm, dm, a, mesh, with_j=True)
            nd, ed, vd = omg.nr_rks_b88_dense(ao4, dm, a, mesh)
        print('camb3lyp omega %s ladder: n %.1e e %.1e v %.1e' % (omega, abs(n - n0), abs(e - e0), abs(veff - v0).max()))
        assert abs(n - n0) < tol * 100 and abs(e - e0) < tol * 100 and abs(veff - v0).max() < tol * 10 and abs(veff.ecoul - ec0) < 1e-7
        assert abs(veff.vj - vj).max() < 1e-9
        vxc = pmg.nr_rks(df, 'CAM-B3LYP', dm, omega=omega)[2]
        print('camb3lyp omega %s dense: e %.1e v %.1e' % (omega, abs(e - ed), abs(vxc - vd).max()))
        assert abs(e - ed) < 1e-7 and abs(vxc - vd).max() < 1e-7 and abs(veff - vj - vxc).max() < 1e-9
        results[omega] = (e, np.asarray(vxc))
    assert abs(results[None][0] - results[0.15][0]) > 1e-3                       # the override changes the functional
    e33, v33 = pmg.nr_rks(df, 'camb3lyp', dm, omega=0.33)[1:]
    assert e33 == results[None][0] and np.array_equal(np.asarray(v33), results[None][1])
    rng = np.random.default_rng(4)
    d1 = rng.standard_normal(dm.shape) * 0.05
    d1 = d1 + d1.T
    eps = 1e-4
    fd = (pmg.nr_rks(df, 'camb3lyp', dm + eps * d1)[1] - pmg.nr_rks(df, 'camb3lyp', dm - eps * d1)[1]) / (2 * eps)
    assert abs(fd - np.einsum('ij,ji', results[None][1], d1)) < 1e-6 * max(1.0, abs(fd))
    for code in CAM_CODES[1:]:
        ec, vc = pmg.nr_rks(df, code, dm)[1:]
        assert ec == results[None][0] and np.array_equal(np.asarray(vc), results[None][1])
    with pytest.raises(ValueError, match='not range-separated'):
        pmg.nr_rks(df, 'b3lyp5', dm, omega=0.2)
    with pytest.raises(ValueError):
        pmg.nr_rks(df, 'camb3lyp', dm, omega=-0.2)


def check_cam_kpts(df, cell, tol, omegas=(None, 0.15)):
    """k-points, as test_lyp.check_lyp_kpts: nr_rks('camb3lyp', kpts=...) against the restatement on the same ladder."""
    a, mesh = cell.lattice_vectors(), cell.mesh
    kpts, dms = make_kpts_dms(cell)
    for omega in omegas:
        n, e, veff = pmg.nr_rks(df, 'camb3lyp', dms, kpts=kpts, with_j=True, omega=omega)
        with lyp.oracle_gga(rsh.functional('camb3lyp', omega)):
            n0, e0, v0 = omg.nr_rks_b88_kpts(as_tasks(df.tasks), cell._atm, dms, a, mesh, kpts, with_j=True)
        print('camb3lyp omega %s kpts: n %.1e e %.1e v %.1e' % (omega, abs(n - n0), abs(e - e0), abs(veff - v0).max()))
        assert veff.shape == dms.shape and abs(n - n0) < tol * 100 and abs(e - e0) < tol * 100 and abs(veff - v0).max() < tol * 10
        assert abs(veff - veff.conj().transpose(0, 2, 1)).max() < tol * 10


@pytest.mark.parametrize('mk', [cell_he_split, cell_c2_orth])
def test_product_camb3lyp_on_checker_backend(mk):
    """The orchestration for 'camb3lyp' on the CPU checker backend, at the tolerances of test_lyp.test_product_lyp_on_checker_backend."""
    cell = mk()
    df = _df(cell)
    check_cam_ladder(df, cell, 1e-10)
    assert not df._built


@pytest.mark.parametrize('mk', [cell_he_split, cell_c2_orth])
def test_product_camb3lyp_kpts_on_checker_backend(mk):
    """k-points on both cells; cell_c2_orth (p shells, the eight-level ladder under 48^3) with the functional's own omega alone: the
    oracle's complex collocation of its levels is most of the 100 s the case takes here, and the override is covered on cell_he_split
    and at Gamma."""
    cell = mk()
    df = _df(cell)
    check_cam_kpts(df, cell, 1e-10, (None, 0.15) if mk is cell_he_split else (None,))


def dense_hybrid_k_case(cell, dm):
    """The dense numbers of hybrid_k on ``cell``: integrals by FFT on the cell's mesh, the quadrature overlap.  Returns a function
    (omega, alpha, hyb, ewald) -> matrix."""
    a, mesh = cell.lattice_vectors(), cell.mesh
    ao = dense_ao4(cell)[0]
    S = cell.vol / len(ao) * ao.T.dot(ao)
    eri = pair_eris(ao, a, mesh)
    lr = {}

    def dense(omega, alpha, hyb, ewald=True):
        if omega not in lr:
            lr[omega] = pair_eris(ao, a, mesh, omega)
        return dense_hybrid_k(eri, lr[omega], dm, S, cell, omega, alpha, hyb, ewald)
    return dense


def check_hybrid_k(df, cell, tol=1e-8):
    """hybrid_k against the dense combination hyb (K + madelung S D S) + (alpha - hyb) (K_LR + xi_omega S D S) on a cell where the fit
    is exact (two s functions: three distinct pair products, c_isdf = 2 allows four points)."""
    dm = np.array([[1.1, -.3], [-.3, .7]])
    dense = dense_hybrid_k_case(cell, dm)
    for omega in (None, 0.15):
        vk = pmg.hybrid_k(df, 'camb3lyp', dm, omega=omega)
        ref = dense(omega or 0.33, 0.65, 0.19)
        print('hybrid_k omega %s: %.2e of %.3f' % (omega, abs(vk - ref).max(), abs(ref).max()))
        assert vk.shape == dm.shape and abs(vk - ref).max() < tol
    assert 3 <= len(df.ip) <= 4                                                  # the pick may stop at the rank: three distinct products
    assert abs(pmg.hybrid_k(df, 'camb3lyp', dm, exxdiv=None) - dense(0.33, 0.65, 0.19, ewald=False)).max() < tol
    stack = np.array([dm, dm[::-1, ::-1]])
    assert abs(pmg.hybrid_k(df, 'camb3lyp', stack)[0] - dense(0.33, 0.65, 0.19)).max() < tol
    # a global hybrid: hyb K; no exact exchange: zeros
    assert abs(pmg.hybrid_k(df, 'b3lyp5', dm) - 0.2 * df.get_jk(dm, with_j=False, exxdiv='ewald')[1]).max() < 1e-14
    assert abs(pmg.hybrid_k(df, 'blyp', dm)).max() == 0.0
    # get_jk keeps refusing omega with exxdiv='ewald'
    with pytest.raises(NotImplementedError):
        df.get_jk(dm, with_j=False, omega=0.33, exxdiv='ewald')
    with pytest.raises(ValueError, match='not range-separated'):
        pmg.hybrid_k(df, 'b3lyp5', dm, omega=0.2)


def test_hybrid_k_on_checker_backend():
    cell = cell_he_reference(15)
    df = _df(cell, c_isdf=2, select='global')
    check_hybrid_k(df, cell)


def test_coefficients_spellings_and_fences():
    for code in CAM_CODES:
        assert pmg.rsh_and_hybrid_coeff(code) == (0.33, 0.65, 0.19) and pmg.hybrid_coeff(code) == 0.19
        fn = pmg._functional(code)
        assert fn == (0.0, 0.35, 0.19, 'V', 0.81, 0.19) and (fn.c_b88_sr, fn.omega, fn.alpha) == (0.46, 0.33, 0.65)
    for code, hyb in (('b3lyp', 0.2), ('B3LYP5', 0.2), ('blyp', 0.0), ('lda,vwn', 0.0), ('b88,', 0.0)):
        assert pmg.rsh_and_hybrid_coeff(code) == (0, 0, hyb)
    assert pmg.rsh_and_hybrid_coeff((0, 1, 0, 'V', 1, 0.25)) == (0, 0, 0.25)
    assert pmg._functional('BLYP') == pmg._functional('b88, lyp') == (0.0, 1.0, 0.0, 'V', 1.0, 0.0)
    assert type(pmg._functional('BLYP')) is tuple and pmg._functional('b3lyp') == (0.08, 0.72, 0.19, 'RPA', 0.81, 0.2)
    for code in ('pbe,pbe', 'lda,pw', 'pbe0', 'b3pw91', 'wb97x', 'lc-blyp'):
        for f in (pmg._functional, pmg.hybrid_coeff, pmg.rsh_and_hybrid_coeff):
            with pytest.raises(NotImplementedError, match='no libxc'):
                f(code)


def test_refusals_fire_before_any_work():
    """Open shell (the spin-polarised VWN is not built), every response function, and hybrid_k away from the Gamma point or one
    process: NotImplementedError naming the case, nothing planned or built."""
    cell = cell_he_split()
    df = _df(cell)
    dm = make_dm(cell)
    pair = np.stack([dm, dm]) * .5

    class MF:
        with_df, kpts = df, np.zeros((1, 3))
    for code in CAM_CODES:
        MF.xc = code
        for call in (lambda: pmg.nr_uks(df, code, pair), lambda: pmg.xc_nuc_grad_uks(df, code, pair)):
            with pytest.raises(NotImplementedError, match='spin-polarised VWN'):
                call()
        for call in (lambda: pmg.nr_rks_fxc(df, code, dm, dm[None]), lambda: pmg.nr_rks_fxc_st(df, code, dm, dm[None]),
                     lambda: pmg.nr_rks_fxc_st(df, code, dm, dm[None], singlet=False), lambda: pmg.nr_uks_fxc(df, code, pair, pair),
                     lambda: pmg.cache_xc_kernel1(df, code, dm), lambda: pmg.cache_xc_kernel1(df, code, pair, spin=1),
                     lambda: pmg._gen_rhf_response(MF, dm), lambda: pmg._gen_rhf_response(MF, dm, singlet=True),
                     lambda: pmg._gen_uhf_response(MF, pair)):
            with pytest.raises(NotImplementedError, match='response'):
                call()
    kpt = np.array([[0.1, 0.2, 0.3]])
    dk = _df(cell, kpts=kpt)
    with pytest.raises(NotImplementedError, match='k-points'):
        pmg.hybrid_k(dk, 'camb3lyp', dm)
    sh = _df(cell)
    sh.force_sharded = True
    with pytest.raises(NotImplementedError, match='sharded'):
        pmg.hybrid_k(sh, 'camb3lyp', dm)
    ds = _df(cell)
    ds.kpts_symm = kpts_symm.make_kpts(cell, np.zeros((1, 3)))
    with pytest.raises(NotImplementedError, match='k-point symmetry'):
        pmg.hybrid_k(ds, 'camb3lyp', dm)
    for d in (df, dk, sh, ds):
        assert d.tasks is None and not d._built
    # the old fences
    for code in ('pbe,pbe', 'lda,pw'):
        with pytest.raises(NotImplementedError, match='no libxc'):
            pmg.nr_rks(df, code, dm)
    for code in ('b3lyp', 'b3lyp5', 'lda,vwn'):
        with pytest.raises(NotImplementedError):
            pmg.nr_uks(df, code, pair)
    with pytest.raises(NotImplementedError):
        pmg.nr_rks_fxc(df, 'blyp', dm, dm[None])
    assert df.tasks is None


# ---- forces ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def cam_restatement(monkeypatch):
    """tests/xc_grad_reference.py with 'camb3lyp' (and 'camb3lyp@omega') among its codes."""
    keep = xr.functional

    def functional(code):
        if code.startswith('camb3lyp'):
            return rsh.functional('camb3lyp', float(code.split('@')[1]) if '@' in code else None)
        return keep(code)
    monkeypatch.setattr(xr, 'functional', functional)
    return xr


def test_camb3lyp_force_restatement_and_product(coarse, cam_restatement):
    """The smallest cell of tests/test_xc_grad.py (cell_he_split on 20 x 21 x 20) by that file's method: every atom and direction, the
    restated 'camb3lyp' force against central differences of the restated E_xc at h = 2e-3 and 1e-3 Bohr, |F - FD(h/2)| <= 0.5 |FD(h) -
    FD(h/2)|; then xc_nuc_grad and get_vxc_e1 of the product on the checker backend (one level) against the restatement at 1e-10 of
    the largest, the matrix contracted with D giving the force, and the omega override."""
    from rsh_backend import RshGradOracleBackend
    su, code = coarse, 'camb3lyp'
    F = xr.xc_nuc_grad(su.ao10, su.dm, code, su.weight, su.aoslices)
    for ia in range(su.cell.natm):
        for x in range(3):
            fd = {h: (xr.exc_energy(su.displaced[ia, x, h, 1], su.dm, code, su.weight) -
                      xr.exc_energy(su.displaced[ia, x, h, -1], su.dm, code, su.weight)) / (2 * h) for h in (H, H / 2)}
            own, diff = abs(fd[H] - fd[H / 2]), abs(F[ia, x] - fd[H / 2])
            print('atom %d axis %d: analytic %+.10e  fd %+.10e  |diff| %.2e  |FD(h) - FD(h/2)| %.2e' % (ia, x, F[ia, x], fd[H / 2], diff, own))
            assert abs(F[ia, x]) > 1e-2
            assert diff <= 0.5 * own, (ia, x, diff, own)
    rel = lambda x, ref: float(abs(x - ref).max() / abs(ref).max())
    df = pmg.MultiGridFFTDF(su.cell, backend=RshGradOracleBackend())
    df.max_levels = 1
    for omega in (None, 0.15):
        tag = code if omega is None else '%s@%s' % (code, omega)
        Fp, e1 = pmg.xc_nuc_grad(df, code, su.dm, omega=omega), pmg.get_vxc_e1(df, code, su.dm, omega=omega)
        Fr, er = xr.xc_nuc_grad(su.ao10, su.dm, tag, su.weight, su.aoslices), xr.get_vxc_e1(su.ao10, su.dm, tag, su.weight)
        print('omega %s: force %.2e  matrix %.2e' % (omega, rel(Fp, Fr), rel(e1, er)))
        assert len(df.tasks) == 1 and Fp.shape == (su.cell.natm, 3) and e1.shape == (3,) + su.dm.shape
        assert rel(Fp, Fr) < 1e-10 and rel(e1, er) < 1e-10
        assert rel(xr.contract_e1(e1, su.dm, su.aoslices), Fp) < 1e-10
    assert rel(Fr, F) > 1e-4
    with pytest.raises(ValueError, match='not range-separated'):
        pmg.xc_nuc_grad(df, 'blyp', su.dm, omega=0.2)
