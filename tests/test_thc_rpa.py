"""Direct RPA from the ISDF factors (pyscf_isdf_amd/thc_rpa.py), CPU half (-m "not gpu"): the frequency grid, the identity with the
plasmon formula of the object's own integrals (any fit, good or poor), the second-order term against the direct MP2 energy and
against mp2_os, the deviation from the exact FFTDF integrals at full rank, the two-electron Be cell, and every refusal.  rpa runs
through the product's own orchestration on the checker backend of tests/rpa_backend.py.  The device half is
tests/test_gpu_thc_rpa.py, which imports the cases from here.

Every bound on a quadrature is ten times a deviation measured HERE on the CPU with a numpy restatement of the same frequency sum on
the same integrals in the (ia) basis (rpa_sum_from_integrals: no factor, no point basis), never looser than 1e-8 relative; the
measured values stand next to the constants and each test prints its own."""
import numpy as np
import pytest
from pyscf_isdf_amd import thc_rpa
from pyscf_isdf_amd import multigrid as pmg
from pyscf_isdf_amd.isdf import ISDF
from oracle import fftdf as offt
from cells import cell_diamond_prim
from test_multigrid import dense_ao
from test_thc_mp2 import IDENTITY_CASES, random_orbitals, be_df, be_rhf
from rpa_backend import RpaOracleBackend, thc_chi0_numpy

# max over D, D' in {0.25, 1, 5} of |sum_k w_k f(w_k) - pi / (2 (D + D'))| (2 (D + D') / pi) at nw = 40, x0 = 0.5
GRID_MEASURED = 5.80e-14
# |E(40-point sum) - E(plasmon)| / |E| of the numpy restatement on the object's own integrals, per identity case: e_corr, e_mp2_direct
QUAD_MEASURED = {'diamond-c6': (7.56e-12, 4.80e-15), 'diamond-c3': (5.57e-12, 5.12e-15), 'he_split-c4': (2.52e-12, 4.64e-15),
                 'he_split-c3-local': (2.59e-12, 4.52e-15)}
# |e_corr(factors at full rank) - plasmon(exact FFTDF integrals)| / |e_corr| on the diamond cell (the fit's error and the quadrature's)
FULL_RANK_MEASURED = 1.13e-11
# |E(40-point sum) - E(plasmon)| / |E| of the numpy restatement on the one exact integral of the Be cell
BE_QUAD_MEASURED = 7.42e-10


def bound(measured, P=0):
    """Ten times the measured deviation, never looser than 1e-8.  Where the measured value is itself rounding (the second-order
    sums: 20 eps), not below the rounding of the traces rpa takes over P^2 products, 2 P^2 eps in the worst case (the bound of
    isdf_trace_sq's own test)."""
    return min(max(10 * measured, 2 * P * P * np.finfo(float).eps), 1e-8)


FULL_RANK_BOUND = bound(FULL_RANK_MEASURED)


# ---- references ---------------------------------------------------------------------------------------------------------------------
def plasmon_energy(ovov, eo, ev):
    """Direct RPA correlation energy of a closed shell from the plasmon formula, 1/2 sum_n (Omega_n - A_nn) with A = D + 2 K,
    B = 2 K, K = (ia|jb): Omega^2 are the eigenvalues of (A - B)^1/2 (A + B) (A - B)^1/2 = D^1/2 (D + 4 K) D^1/2."""
    d = (ev[None, :] - eo[:, None]).ravel()
    r = np.sqrt(d)
    om = np.sqrt(np.linalg.eigvalsh(r[:, None] * (np.diag(d) + 4 * ovov) * r[None, :]))
    return 0.5 * float(om.sum() - d.sum() - 2 * np.trace(ovov))


def mp2_direct_from_integrals(ovov, eo, ev):
    """- 2 sum (ia|jb)^2 / (D_ia + D_jb): the direct (Coulomb-only) MP2 energy, twice the opposite-spin energy."""
    d = (ev[None, :] - eo[:, None]).ravel()
    return -2 * float((ovov ** 2 / (d[:, None] + d[None, :])).sum())


def rpa_sum_from_integrals(ovov, eo, ev, nw=40, x0=0.5):
    """The frequency sums of thc_rpa.rpa restated in the (ia) basis on explicit integrals: (e_corr, e_mp2_direct)."""
    d = (ev[None, :] - eo[:, None]).ravel()
    freqs, w = thc_rpa.frequency_grid(nw, x0)
    ec = e2 = 0.0
    for f, wk in zip(freqs, w):
        kd = ovov * (4 * d / (d ** 2 + f ** 2))[None, :]
        sign, logdet = np.linalg.slogdet(np.eye(len(d)) + kd)
        assert sign > 0
        ec += wk * (logdet - np.trace(kd))
        e2 -= wk * np.einsum('ij,ji->', kd, kd)
    return ec / (2 * np.pi), e2 / (4 * np.pi)


_CASES = {}


def rpa_case(name):
    """(df on the checker backend, C, e, occ, (ia|jb) from df.ao2mo), made once per identity case of tests/test_thc_mp2.py."""
    if name not in _CASES:
        mk, nocc, c_isdf, select = IDENTITY_CASES[name]
        cell = mk()
        df = ISDF(cell, c_isdf=c_isdf, select=select, backend=RpaOracleBackend())
        c, e, occ = random_orbitals(cell, nocc)
        co, cv = c[:, occ > 0], c[:, occ == 0]
        _CASES[name] = df, c, e, occ, df.ao2mo((co, cv, co, cv))
    return _CASES[name]


def exact_ovov(cell, c, occ):
    """(ia|jb) from the exact FFTDF integrals of the cell (oracle.fftdf.get_ao_eri_s4)."""
    nao = len(occ)
    s4 = offt.get_ao_eri_s4(dense_ao(cell), cell.lattice_vectors(), cell.mesh)
    idx = np.zeros((nao, nao), dtype=int)
    i, j = np.tril_indices(nao)
    idx[i, j] = idx[j, i] = np.arange(len(i))
    eri = s4[idx.ravel()][:, idx.ravel()].reshape(nao, nao, nao, nao)
    co, cv = c[:, occ > 0], c[:, occ == 0]
    return np.einsum('pqrs,pi,qa,rj,sb->iajb', eri, co, cv, co, cv, optimize=True).reshape(co.shape[1] * cv.shape[1], -1)


def be_case(df):
    """RHF orbitals of the Be cell from ``df`` (tests/test_thc_mp2.be_rhf), the plasmon energy of the cell's exact FFTDF integral
    (ia|ia) in them, and the bound for rpa's relative deviation from it: (C, e, occ, e_plasmon, bound).
    The bound has two parts.  The quadrature: ten times BE_QUAD_MEASURED.  The fit: with one pair E = (sqrt(D^2 + 4 K D) - D - 2 K)
    / 2 = - K^2 / D + O(K^3), so a relative error r in K is 2 r in E to first order; r is what the object's own ao2mo integral
    deviates from the exact one by (the rounding of a fit of three pair products on four points; c_isdf = 2 is exact but for
    that), and the bound takes 3 r."""
    e_scf, c, e, occ = be_rhf(df)
    eo, ev = e[occ > 0], e[occ == 0]
    k = exact_ovov(df.cell, c, occ)
    co, cv = c[:, occ > 0], c[:, occ == 0]
    r = float(abs(df.ao2mo((co, cv, co, cv)) - k).max() / abs(k).max())
    ref = plasmon_energy(k, eo, ev)
    own = rpa_sum_from_integrals(k, eo, ev)[0]
    print('Be: (ia|ia) %.6e, the fit deviates by %.2e relative; numpy sum against the plasmon formula %.2e (recorded %.2e)' %
          (k[0, 0], r, abs(own - ref) / abs(ref), BE_QUAD_MEASURED))
    return c, e, occ, ref, bound(BE_QUAD_MEASURED) + 3 * r


# ---- 1. the frequency grid ----------------------------------------------------------------------------------------------------------
def test_frequency_grid_integrates_the_products_of_two_lorentzians():
    """int_0^inf D D' / ((D^2 + w^2) (D'^2 + w^2)) dw = pi / (2 (D + D')): the integral behind every term of the second order, for
    gaps on both sides of x0."""
    freqs, w = thc_rpa.frequency_grid(40, 0.5)
    assert len(freqs) == 40 and (freqs > 0).all() and (w > 0).all() and (np.diff(freqs) > 0).all()
    assert (freqs < 0.5).sum() == 20
    worst = 0.0
    for d1 in (0.25, 1.0, 5.0):
        for d2 in (0.25, 1.0, 5.0):
            got = (w * d1 * d2 / ((d1 ** 2 + freqs ** 2) * (d2 ** 2 + freqs ** 2))).sum()
            worst = max(worst, abs(got * 2 * (d1 + d2) / np.pi - 1))
    print('frequency_grid(40, 0.5): worst relative deviation %.3e (asserted at 10 x %.3e)' % (worst, GRID_MEASURED))
    assert worst <= 10 * GRID_MEASURED
    f2, w2 = thc_rpa.frequency_grid(40, 2.0)
    assert np.allclose(f2, 4 * freqs, rtol=1e-14) and np.allclose(w2, 4 * w, rtol=1e-14)


def test_frequency_grid_rejects_bad_arguments():
    for args in ((0, 0.5), (40, 0.0), (40, -1.0), (40, np.inf)):
        with pytest.raises(ValueError):
            thc_rpa.frequency_grid(*args)


# ---- 2. identity with the object's own integrals ------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(IDENTITY_CASES))
def test_rpa_is_the_plasmon_energy_of_the_objects_own_integrals(name):
    """rpa against the plasmon formula with (ia|jb) from the same factors (df.ao2mo): they differ by the frequency quadrature alone,
    at any quality of the fit - c_isdf = 3 is a deliberately poor one.  The quadrature's own error is measured with the numpy
    restatement in the (ia) basis and the assertion is ten times the recorded value."""
    df, c, e, occ, ovov = rpa_case(name)
    eo, ev = e[occ > 0], e[occ == 0]
    ref = plasmon_energy(ovov, eo, ev)
    own = rpa_sum_from_integrals(ovov, eo, ev)[0]
    res = df.rpa(c, e, occ)
    rel = abs(res.e_corr - ref) / abs(ref)
    print('%s: e_corr %.12e  plasmon %.12e  relative %.2e  (numpy sum: %.2e; recorded %.2e)' %
          (name, res.e_corr, ref, rel, abs(own - ref) / abs(ref), QUAD_MEASURED[name][0]))
    assert res.e_corr < 0 and res.nw == len(res.terms) == len(res.freqs) == len(res.weights) == 40
    assert (res.terms <= 0).all()                                    # ln(1 + x) <= x for every eigenvalue x >= 0 of S W
    assert rel <= bound(QUAD_MEASURED[name][0], len(df.ip))


@pytest.mark.parametrize('name', list(IDENTITY_CASES))
def test_second_order_term_is_the_direct_mp2_energy(name):
    """e_mp2_direct against - 2 sum (ia|jb)^2 / (D + D') of the object's own integrals (the frequency quadrature alone, bounded as
    above), and against 2 e_os of mp2_os at rtol = 1e-10, whose own Laplace quadrature adds its contract of 1e-10 relative."""
    df, c, e, occ, ovov = rpa_case(name)
    eo, ev = e[occ > 0], e[occ == 0]
    ref = mp2_direct_from_integrals(ovov, eo, ev)
    own = rpa_sum_from_integrals(ovov, eo, ev)[1]
    res = df.rpa(c, e, occ)
    os2 = 2 * df.mp2_os(c, e, occ, rtol=1e-10).e_os
    rel, rel_os = abs(res.e_mp2_direct - ref) / abs(ref), abs(res.e_mp2_direct - os2) / abs(ref)
    print('%s: e_mp2_direct %.12e  integrals %.12e  relative %.2e  (numpy sum: %.2e; recorded %.2e)  against 2 e_os %.2e' %
          (name, res.e_mp2_direct, ref, rel, abs(own - ref) / abs(ref), QUAD_MEASURED[name][1], rel_os))
    assert rel <= bound(QUAD_MEASURED[name][1], len(df.ip))
    assert rel_os <= bound(QUAD_MEASURED[name][1], len(df.ip)) + 1e-10
    assert res.e_corr > res.e_mp2_direct                             # the ring sum beyond second order screens


def test_rpa_through_the_multigrid_object():
    """MultiGridFFTDF inherits rpa and builds its fit for it."""
    df, c, e, occ, ovov = rpa_case('diamond-c6')
    ref = plasmon_energy(ovov, e[occ > 0], e[occ == 0])
    mg = pmg.MultiGridFFTDF(df.cell, c_isdf=6, select='global', backend=RpaOracleBackend())
    assert abs(mg.rpa(c, e, occ).e_corr - ref) <= bound(QUAD_MEASURED['diamond-c6'][0]) * abs(ref)


def test_rpa_counts_its_buffers_against_max_device_memory():
    df, c, e, occ, ovov = rpa_case('diamond-c3')
    small = ISDF(df.cell, c_isdf=3, select='global', backend=RpaOracleBackend())
    small.build()
    small.max_device_memory = sum(b.numel() * 8 for b in small._bufs.values()) + 8 * len(small.ip) ** 2     # room for S, not for B
    with pytest.raises(MemoryError, match='max_device_memory'):
        small.rpa(c, e, occ)
    assert 'thc_A' not in small._bufs


# ---- 3. against exact integrals -----------------------------------------------------------------------------------------------------
def test_full_rank_fit_reproduces_the_plasmon_energy_of_the_exact_fftdf_integrals():
    """Diamond primitive cell, global selection to full rank (c_isdf = 6 offers 48 points for 36 pair products, select_tol = 0)
    against the plasmon formula of the exact FFTDF integrals.  What is left is the fit's error plus the quadrature's."""
    cell = cell_diamond_prim()
    df = ISDF(cell, c_isdf=6, select='global', backend=RpaOracleBackend())
    df.select_tol = 0.0
    c, e, occ = random_orbitals(cell, 4)
    ref = plasmon_energy(exact_ovov(cell, c, occ), e[occ > 0], e[occ == 0])
    res = df.rpa(c, e, occ)
    rel = abs(res.e_corr - ref) / abs(ref)
    print('full rank (P = %d): e_corr %.12e  exact %.12e  relative deviation %.2e  bound %.1e' % (len(df.ip), res.e_corr, ref, rel, FULL_RANK_BOUND))
    assert rel <= FULL_RANK_BOUND


def test_be_cell_matches_the_plasmon_formula_of_the_exact_integrals():
    """The two-electron Be cell of tests/golden/be_gth_cell.json (one occupied, one virtual orbital: S W is a rank-one update and
    the plasmon formula a single square root), RHF orbitals from the fit on the checker backend, against the plasmon formula of the
    cell's exact FFTDF integrals."""
    df = be_df(RpaOracleBackend())
    c, e, occ, ref, tol = be_case(df)
    res = df.rpa(c, e, occ)
    rel = abs(res.e_corr - ref) / abs(ref)
    print('Be: e_corr %.12e  plasmon %.12e  relative %.2e  bound %.1e' % (res.e_corr, ref, rel, tol))
    assert rel <= tol


# ---- 4. refusals --------------------------------------------------------------------------------------------------------------------
def _untouched(df):
    return not df._built and getattr(df, 'tasks', None) is None and 'thc_A' not in df._bufs


@pytest.mark.parametrize('cls', [ISDF, pmg.MultiGridFFTDF])
def test_rpa_refuses_what_it_does_not_do_before_any_work(cls):
    cell = cell_diamond_prim()
    c, e, occ = random_orbitals(cell, 4)

    def fresh(**kw):
        return cls(cell, c_isdf=3, select='local', backend=RpaOracleBackend(), **kw)
    dk = fresh(kpts=np.array([[.1, .2, .3]]))
    with pytest.raises(NotImplementedError, match='rpa at k-points'):
        dk.rpa(c, e, occ)
    assert _untouched(dk)
    db = fresh()
    db.kpts_band = np.array([[.1, 0, 0]])
    with pytest.raises(NotImplementedError, match='rpa at k-points'):
        db.rpa(c, e, occ)
    assert _untouched(db)
    ds = fresh()
    ds.kpts_symm = object()
    with pytest.raises(NotImplementedError, match='rpa with k-point symmetry'):
        ds.rpa(c, e, occ)
    assert _untouched(ds)
    sh = fresh()
    sh.force_sharded = True
    with pytest.raises(NotImplementedError, match='rpa on the grid-sharded'):
        sh.rpa(c, e, occ)
    assert _untouched(sh)
    do = fresh()
    do.pair_space = 'occ'
    with pytest.raises(NotImplementedError, match="rpa with pair_space='occ'"):
        do.rpa(c, e, occ)
    assert _untouched(do)
    df = fresh()
    for bad in (np.array([2., 2, 2, 1, 1, 0, 0, 0]), np.array([[1., 1, 1, 1, 0, 0, 0, 0]] * 2)):
        with pytest.raises(NotImplementedError, match='rpa for open shells'):
            df.rpa(c, e, bad)
    for eg in (np.concatenate([e[:3], [e[4]], e[4:]]), np.concatenate([e[:3], [e[4] + .1], e[4:]])):     # zero gap, negative gap
        with pytest.raises(ValueError, match='rpa needs a positive gap'):
            df.rpa(c, eg, occ)
    with pytest.raises(NotImplementedError, match='rpa with complex orbitals'):
        df.rpa(c + 1j * np.roll(c, 1, axis=0), e, occ)
    with pytest.raises(ValueError, match='frequency_grid'):
        df.rpa(c, e, occ, nw=0)
    assert _untouched(df)


def test_mp2_os_refusals_keep_their_wording():
    cell = cell_diamond_prim()
    c, e, occ = random_orbitals(cell, 4)
    df = ISDF(cell, c_isdf=3, select='local', backend=RpaOracleBackend(), kpts=np.array([[.1, .2, .3]]))
    with pytest.raises(NotImplementedError, match='^mp2_os at k-points is not implemented'):
        df.mp2_os(c, e, occ)


def test_rpa_refuses_an_indefinite_w():
    """W scaled by -alpha with alpha between the reciprocals of the two largest eigenvalues of W S at the first frequency: exactly
    one eigenvalue of 1 + W S is negative there, the determinant is negative, and the error names that frequency."""
    cell = cell_diamond_prim()
    c, e, occ = random_orbitals(cell, 4)
    df = ISDF(cell, c_isdf=6, select='global', backend=RpaOracleBackend())
    df.build()
    freqs = thc_rpa.frequency_grid()[0]
    aoP = df.aoP.numpy()
    delta = e[occ == 0][None, :] - e[occ > 0][:, None]
    s0 = thc_chi0_numpy(aoP.dot(c[:, occ > 0]), aoP.dot(c[:, occ == 0]), 4 * delta / (delta ** 2 + freqs[0] ** 2))
    mu = np.sort(np.linalg.eigvals(df.W.numpy().dot(s0)).real)[::-1]
    assert mu[1] > 1e-6 * mu[0] > 0
    df.W.mul_(-1 / np.sqrt(mu[0] * mu[1]))
    with pytest.raises(ValueError, match='not positive at the imaginary frequency %g ' % freqs[0]):
        df.rpa(c, e, occ)
