"""Opposite-spin MP2 from the ISDF factors (pyscf_isdf_amd/thc_mp2.py), CPU half (-m "not gpu"): the Laplace grid's contract, the
identity with the object's own integrals (any fit, good or poor), the deviation from the exact FFTDF integrals at full rank, the
reference's pinned KMP2 energy of a two-electron Be cell, and every refusal.  mp2_os runs through the product's own orchestration
on the checker backend of tests/thc_backend.py.  The device half is tests/test_gpu_thc_mp2.py, which imports the cases from here."""
import json
import os
import numpy as np
import pytest
import scipy.linalg
from pyscf_isdf_amd import gto, thc_mp2
from pyscf_isdf_amd import multigrid as pmg
from pyscf_isdf_amd.isdf import ISDF
from oracle import fftdf as offt, pp as opp
import scf_helpers
from cells import cell_diamond_prim
from test_multigrid import cell_he_split, dense_ao
from thc_backend import ThcOracleBackend

BE = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'be_gth_cell.json')))
# |e_os(factors) - e_os(exact integrals)| / |e_os| of the diamond cell at full rank: measured 4.64e-12 (test_full_rank_..., which prints it; the quadrature at rtol = 1e-10 is part of it), and
# the bound is 10 x that but never looser than 1e-6
FULL_RANK_MEASURED = 4.64e-12
FULL_RANK_BOUND = min(10 * FULL_RANK_MEASURED, 1e-6)


# ---- cases shared with the device half ----------------------------------------------------------------------------------------------
def random_orbitals(cell, nocc, seed=3, S=None):
    """Eigenvectors of a random symmetric matrix in the S metric (None: the cell's analytic overlap), and orbital energies with a
    gap: (C, e, occ)."""
    if S is None:
        S = scf_helpers.overlap_kinetic_from_ft(cell)[0]
    nao = len(S)
    rng = np.random.default_rng(seed)
    m = rng.standard_normal((nao, nao))
    c = scipy.linalg.eigh(m + m.T, S)[1]
    e = np.concatenate([np.sort(-1.3 + 0.8 * rng.random(nocc)), np.sort(0.25 + 2.5 * rng.random(nao - nocc))])
    occ = np.zeros(nao)
    occ[:nocc] = 2
    return c, e, occ


def e_os_from_integrals(ovov, eo, ev):
    """- sum (ia|jb)^2 / (e_a + e_b - e_i - e_j) with exact denominators; ovov (no nv, no nv)."""
    d = (ev[None, :] - eo[:, None]).ravel()
    return -float((ovov ** 2 / (d[:, None] + d[None, :])).sum())


def be_cell():
    """pbc/mp/test/test_kpoint.py:25-39: Be at the centre of a sheared 7 Bohr cell, gth-szv / gth-pade-q2, 12^3.  Neither table is
    bundled: both come from the fixture."""
    c = BE['cell']
    return gto.Cell(unit=c['unit'], atom=c['atom'], a=c['a'], mesh=c['mesh'], basis={'Be': BE['Be_SZV-GTH']},
                    pseudo={'Be': BE['Be_GTH-PADE-q2']})


def be_rhf(df, vpp=None):
    """RHF with exxdiv='ewald' on the Be cell through scf_helpers.rhf to 1e-12: (e_scf, C, e, occ).  vpp: the pseudopotential matrix
    (None: the object's own get_pp).  The Ewald term of the exchange is the reference's, madelung S D S with the ANALYTIC overlap
    (pyscf/pbc/df/df_jk.py:1446-1452), added here to the object's K without it: the object's own exxdiv='ewald' takes S by
    quadrature on the FFT grid (ISDF.overlap), and on this deliberately coarse 12^3 mesh that S is off by 0.3 in the sharp
    function's diagonal, which moves e_scf by 1.7e-4 Eh."""
    cell = df.cell
    S, T = scf_helpers.overlap_kinetic_from_ft(cell)
    hcore = T + (df.get_pp() if vpp is None else vpp)
    mad = gto.madelung(cell)

    def jk(dm):
        vj, vk = df.get_jk(dm, exxdiv=None)
        return vj, vk + mad * S.dot(dm).dot(S)
    e_scf, dm = scf_helpers.rhf(hcore, S, jk, 1, scf_helpers.ewald_energy(cell), max_cycle=100, conv=1e-12)
    vj, vk = jk(dm)
    e, c = scipy.linalg.eigh(hcore + vj - .5 * vk, S)
    return e_scf, c, e, np.array([2.] + [0.] * (len(e) - 1))


def be_df(backend=None):
    """Two s functions have three pair products: c_isdf = 2 (four points, the selection stops at rank 3) fits them exactly."""
    df = ISDF(be_cell(), c_isdf=2, select='global', backend=backend)
    df.select_tol = 0.0
    return df


def check_be_pin(df, vpp=None):
    e_scf, c, e, occ = be_rhf(df, vpp)
    res = df.mp2_os(c, e, occ, rtol=1e-9)
    print('Be: e_scf %.12f (deviation %.2e)  e_os %.12e (deviation %.2e)  ngrid %d' %
          (e_scf, e_scf - BE['e_scf'], res.e_os, res.e_os - BE['e_corr'], res.ngrid))
    assert abs(e_scf - BE['e_scf']) < 5e-8
    assert abs(res.e_os - BE['e_corr']) < 5e-10
    return res, (c, e, occ)


# ---- 1. the quadrature --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rtol', [1e-6, 1e-8, 1e-10])
@pytest.mark.parametrize('dmin,dmax', [(0.3, 0.3), (0.5, 5), (0.05, 50), (0.01, 100)])
def test_laplace_grid_meets_its_contract(dmin, dmax, rtol):
    tau, w = thc_mp2.laplace_grid(dmin, dmax, rtol)
    x = np.exp(np.linspace(np.log(dmin), np.log(dmax), 4001))
    err = abs(x * (w[None, :] * np.exp(-np.outer(x, tau))).sum(axis=1) - 1).max()
    print('laplace_grid(%g, %g, %g): %d points, max relative error %.2e' % (dmin, dmax, rtol, len(tau), err))
    assert err <= rtol
    assert (w > 0).all() and (tau > 0).all()
    assert len(tau) <= 160


def test_laplace_grid_rejects_bad_ranges():
    for args in ((0.0, 1.0), (-1.0, 1.0), (2.0, 1.0), (1.0, np.inf)):
        with pytest.raises(ValueError):
            thc_mp2.laplace_grid(*args)
    with pytest.raises(ValueError):
        thc_mp2.laplace_grid(1.0, 2.0, rtol=1e-15)


# ---- 2. identity with the object's own integrals ------------------------------------------------------------------------------------
IDENTITY_CASES = {'diamond-c6': (lambda: cell_diamond_prim(), 4, 6, 'global'), 'diamond-c3': (lambda: cell_diamond_prim(), 4, 3, 'global'),
                  'he_split-c4': (cell_he_split, 2, 4, 'global'), 'he_split-c3-local': (cell_he_split, 2, 3, 'local')}
_IDENTITY = {}


def identity_case(name):
    """(df on the checker backend, C, e, occ, -sum (ia|jb)^2 / Delta from df.ao2mo), made once per case."""
    if name not in _IDENTITY:
        mk, nocc, c_isdf, select = IDENTITY_CASES[name]
        cell = mk()
        df = ISDF(cell, c_isdf=c_isdf, select=select, backend=ThcOracleBackend())
        c, e, occ = random_orbitals(cell, nocc)
        co, cv = c[:, occ > 0], c[:, occ == 0]
        ref = e_os_from_integrals(df.ao2mo((co, cv, co, cv)), e[occ > 0], e[occ == 0])
        _IDENTITY[name] = df, c, e, occ, ref
    return _IDENTITY[name]


@pytest.mark.parametrize('rtol', [1e-6, 1e-9])
@pytest.mark.parametrize('name', list(IDENTITY_CASES))
def test_mp2_os_is_the_energy_of_the_objects_own_integrals(name, rtol):
    """mp2_os against - sum (ia|jb)^2 / Delta with (ia|jb) from the same factors (df.ao2mo) and exact denominators: they differ by the
    quadrature alone, whose relative error in the energy is <= rtol (all terms have one sign); 2 rtol with the rounding.  Holds at
    any quality of the fit - c_isdf = 3 is a deliberately poor one."""
    df, c, e, occ, ref = identity_case(name)
    res = df.mp2_os(c, e, occ, rtol=rtol)
    print('%s rtol %g: e_os %.12e  integrals %.12e  relative %.2e  ngrid %d' % (name, rtol, res.e_os, ref, abs(res.e_os - ref) / abs(ref), res.ngrid))
    assert res.e_os < 0 and res.ngrid == len(res.terms) == len(res.tau) and res.rtol == rtol
    assert abs(res.e_os - ref) <= 2 * rtol * abs(ref)
    assert res.e_sos == 1.3 * res.e_os and df.mp2_os(c, e, occ, rtol=rtol, c_os=1.0).e_sos == res.e_os


def test_mp2_os_through_the_multigrid_object():
    """MultiGridFFTDF inherits mp2_os and builds its fit for it."""
    df, c, e, occ, ref = identity_case('diamond-c6')
    mg = pmg.MultiGridFFTDF(df.cell, c_isdf=6, select='global', backend=ThcOracleBackend())
    assert abs(mg.mp2_os(c, e, occ, rtol=1e-9).e_os - ref) <= 2e-9 * abs(ref)


def test_mp2_os_counts_its_buffers_against_max_device_memory():
    df, c, e, occ, ref = identity_case('diamond-c3')
    small = ISDF(df.cell, c_isdf=3, select='global', backend=ThcOracleBackend())
    small.build()
    small.max_device_memory = sum(b.numel() * 8 for b in small._bufs.values()) + 8 * len(small.ip) ** 2     # room for A, not for B
    with pytest.raises(MemoryError, match='max_device_memory'):
        small.mp2_os(c, e, occ)
    assert 'thc_A' not in small._bufs


# ---- 3. against exact integrals -----------------------------------------------------------------------------------------------------
def test_full_rank_fit_reproduces_the_exact_fftdf_energy():
    """Diamond primitive cell, global selection to full rank (c_isdf = 6 offers 48 points for 36 pair products, select_tol = 0)
    against - sum (ia|jb)^2 / Delta from the exact FFTDF integrals (oracle.fftdf.get_ao_eri_s4).  What is left is the fit's error
    plus the quadrature's (rtol = 1e-10)."""
    cell = cell_diamond_prim()
    df = ISDF(cell, c_isdf=6, select='global', backend=ThcOracleBackend())
    df.select_tol = 0.0
    c, e, occ = random_orbitals(cell, 4)
    nao = len(e)
    s4 = offt.get_ao_eri_s4(dense_ao(cell), cell.lattice_vectors(), cell.mesh)
    idx = np.zeros((nao, nao), dtype=int)
    i, j = np.tril_indices(nao)
    idx[i, j] = idx[j, i] = np.arange(len(i))
    eri = s4[idx.ravel()][:, idx.ravel()].reshape(nao, nao, nao, nao)
    co, cv = c[:, occ > 0], c[:, occ == 0]
    ovov = np.einsum('pqrs,pi,qa,rj,sb->iajb', eri, co, cv, co, cv, optimize=True).reshape(co.shape[1] * cv.shape[1], -1)
    ref = e_os_from_integrals(ovov, e[occ > 0], e[occ == 0])
    res = df.mp2_os(c, e, occ, rtol=1e-10)
    rel = abs(res.e_os - ref) / abs(ref)
    print('full rank (P = %d): e_os %.12e  exact %.12e  relative deviation %.2e  bound %.1e' % (len(df.ip), res.e_os, ref, rel, FULL_RANK_BOUND))
    assert rel <= FULL_RANK_BOUND


# ---- 4. the reference's pin ---------------------------------------------------------------------------------------------------------
def test_be_cell_reproduces_the_reference_kmp2_energy():
    """pbc/mp/test/test_kpoint.py:85-89 (KRHF + KMP2 at one k-point, FFTDF): e_scf = -1.2061049658473704 to the reference's 7 places
    (5e-8) and e_corr = -5.44597932944397e-06 to its 9 (5e-10).  The cell has two electrons, so one occupied orbital: the same-spin
    term sum (ia|ib) [(ia|ib) - (ib|ia)] / Delta vanishes identically because (ia|ib) = (ib|ia), and e_corr = sum (ia|ib)
    [2 (ia|ib) - (ib|ia)] / Delta is the opposite-spin energy alone.  The orbital energies carry the Ewald shift of exxdiv='ewald',
    as the reference's do.  Pseudopotential matrix from the oracle, J and K from the fit on the checker backend."""
    df = be_df(ThcOracleBackend())
    cell = df.cell
    vpp = opp.get_pp(cell._atm, cell._bas, cell._env, cell.atom_coords(), cell.atom_charges(), [cell._pseudo['Be']],
                     cell.lattice_vectors(), cell.mesh, cell.get_uniform_grids(), [dense_ao(cell)], np.zeros((1, 3)))[0].real
    check_be_pin(df, vpp)


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------------
def _untouched(df):
    return not df._built and getattr(df, 'tasks', None) is None and 'thc_A' not in df._bufs


@pytest.mark.parametrize('cls', [ISDF, pmg.MultiGridFFTDF])
def test_mp2_os_refuses_what_it_does_not_do_before_any_work(cls):
    cell = cell_diamond_prim()
    c, e, occ = random_orbitals(cell, 4)

    def fresh(**kw):
        return cls(cell, c_isdf=3, select='local', backend=ThcOracleBackend(), **kw)
    dk = fresh(kpts=np.array([[.1, .2, .3]]))
    with pytest.raises(NotImplementedError, match='k-points'):
        dk.mp2_os(c, e, occ)
    assert _untouched(dk)
    db = fresh()
    db.kpts_band = np.array([[.1, 0, 0]])
    with pytest.raises(NotImplementedError, match='k-points'):
        db.mp2_os(c, e, occ)
    assert _untouched(db)
    ds = fresh()
    ds.kpts_symm = object()
    with pytest.raises(NotImplementedError, match='k-point symmetry'):
        ds.mp2_os(c, e, occ)
    assert _untouched(ds)
    sh = fresh()
    sh.force_sharded = True
    with pytest.raises(NotImplementedError, match='sharded'):
        sh.mp2_os(c, e, occ)
    assert _untouched(sh)
    do = fresh()
    do.pair_space = 'occ'
    with pytest.raises(NotImplementedError, match="pair_space='occ'"):
        do.mp2_os(c, e, occ)
    assert _untouched(do)
    df = fresh()
    for bad in (np.array([2., 2, 2, 1, 1, 0, 0, 0]), np.array([[1., 1, 1, 1, 0, 0, 0, 0]] * 2)):
        with pytest.raises(NotImplementedError, match='open shells'):
            df.mp2_os(c, e, bad)
    for eg in (np.concatenate([e[:3], [e[4]], e[4:]]), np.concatenate([e[:3], [e[4] + .1], e[4:]])):     # zero gap, negative gap
        with pytest.raises(ValueError, match='positive gap'):
            df.mp2_os(c, eg, occ)
    assert _untouched(df)
