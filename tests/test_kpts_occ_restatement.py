"""The (AO x occupied) pair space of the k-point ISDF exchange: the numpy restatement
(tests/kocc_reference.py) against oracle.kisdf and the exact k-point exchange, and the host driver's orchestration
(pair_space='occ' at k-points) on the CPU checker backend.  No GPU."""
import warnings
import numpy as np
import pytest
import torch
import cells
import kocc_reference as kr
from pyscf_isdf_amd import gto
from oracle import ao as oao, fftdf, kisdf
from oracle_backend import OracleBackend


class OccKBackend(OracleBackend):
    """The checker backend plus the two k-point (AO x occupied) products, restated in numpy."""

    def gram_prod_cplx(self, aoP, nh, psiP, npsi_h, A):
        A.copy_(torch.from_numpy(kr.gram_occ(aoP.numpy(), psiP.numpy())))

    def pair_prod_rows_cplx(self, aoP, nh, psiP, npsi_h, ao, psi, ng, B):
        B[:, :ng] = torch.from_numpy(kr.rows_occ(aoP.numpy(), psiP.numpy(), ao.numpy()[:, :ng], psi.numpy()[:, :ng]))


def _he2(mesh=None, nk=2, nocc=2, seed=11):
    cell = cells.cell_he2_triclinic()
    if mesh is not None:
        cell.mesh = np.asarray(mesh)
    coords = cell.get_uniform_grids()
    rcut = gto.estimate_rcut_per_shell(cell)
    Ls = gto.get_lattice_Ls(cell, rcut=rcut.max())
    rng = np.random.default_rng(seed)
    kpts = rng.random((nk, 3)) * 0.6
    kpts[0] = 0.0
    aos = [np.asarray(x, dtype=complex) for x in
           oao.eval_ao(cell._atm, cell._bas, cell._env, coords, Ls, rcut, kpts=kpts, rule='point')]
    nao = cell.nao_nr()
    c = rng.standard_normal((nk, nao, nocc)) + 1j * rng.standard_normal((nk, nao, nocc))
    dms = np.einsum('kpi,kqi->kpq', c, c.conj())
    return cell, coords, kpts, aos, c, dms


def test_identity_orbitals_reduce_to_the_ao_pair_fit():
    """C^k = I (every AO occupied with weight 1): psi~ = u, and the occupied-pair Gram matrix and Theta are those of the Bloch
    AO pairs (oracle.kisdf.fit_theta, A = |S|^2)."""
    cell, coords, kpts, aos, c, dms = _he2()
    nao = cell.nao_nr()
    X = kisdf.periodic_stack(aos, coords, kpts)
    Psi = kr.occupied_stack(X, nao, [np.eye(nao)] * len(kpts))
    assert abs(Psi - X).max() < 1e-14 * abs(X).max()
    ip, _ = kisdf.select_ip(X, 40)
    theta, A = kr.fit_theta_occ(X, Psi, ip, reg_rel=1e-12)
    Xp, Xr = X[:, ip], np.vstack([X[X.shape[0] // 2:], -X[:X.shape[0] // 2]])
    A_ao = Xp.T.dot(Xp) ** 2 + Xr[:, ip].T.dot(Xp) ** 2
    theta_ao = kisdf.fit_theta(X, ip, reg_rel=1e-12)
    assert abs(A - A_ao).max() <= 1e-12 * abs(A_ao).max()
    assert abs(theta - theta_ao).max() <= 1e-12 * abs(theta_ao).max()


def test_every_grid_point_reproduces_the_exact_exchange():
    """All G grid points as interpolation points: the fit reproduces every pair function on the grid, so K is the exact
    k-point exchange on that grid (oracle.fftdf.get_jk_kpts) up to the fit's diagonal shift.  The pair space (16 Bloch AOs x
    4 occupied orbitals) spans less than the 125 grid points, so A_PP is singular and needs the shift reg_rel * max(diag):
    the shift damps the pair components along A's small eigenvalues, and the error in K follows it linearly (measured
    4.4e-8, 4.4e-10, 4.4e-12 of |K| ~ 3 for reg_rel 1e-10, 1e-12, 1e-14).  Bound: 1e-8 at the default reg_rel = 1e-12, and the
    error must fall with the shift."""
    cell, coords, kpts, aos, c, dms = _he2(mesh=[5, 5, 5])
    nao = cell.nao_nr()
    a, mesh = cell.lattice_vectors(), cell.mesh
    X = kisdf.periodic_stack(aos, coords, kpts)
    Psi = kr.occupied_stack(X, nao, list(c))
    ip = np.arange(len(coords))
    vk_ref = fftdf.get_jk_kpts(aos, dms, a, mesh, coords, kpts)[1]
    errs = []
    for reg in (1e-10, 1e-12):
        theta, _ = kr.fit_theta_occ(X, Psi, ip, reg_rel=reg)
        errs.append(abs(kr.get_k_occ(theta, ip, aos, coords, kpts, a, mesh, dms) - vk_ref).max())
    assert errs[1] < 1e-8, errs
    assert errs[1] < 0.05 * errs[0], errs


# ---- the host driver on the checker backend ------------------------------------------------------------------------
def _diamond(nk=(2, 1, 1), mesh=(9, 9, 9), seed=5):
    cell = cells.cell_diamond_prim(mesh=mesh)
    kpts = cell.make_kpts(list(nk))
    nao = cell.nao_nr()
    rng = np.random.default_rng(seed)
    mo = []
    for k in range(len(kpts)):
        z = rng.standard_normal((nao, nao)) + 1j * rng.standard_normal((nao, nao))
        mo.append(np.linalg.qr(z)[0])
    mo = np.array(mo)
    occ = np.zeros((len(kpts), nao))
    occ[:, :2] = 2.0
    dms = np.einsum('kpi,ki,kqi->kpq', mo, occ, mo.conj())
    return cell, kpts, mo, occ, dms


def _tag(dms, mo, occ):
    from pyscf_isdf_amd._common import tag_array
    return tag_array(dms, mo_coeff=mo, mo_occ=occ)


def _df(cell, kpts, space, select='refined', c_isdf=3):
    from pyscf_isdf_amd.isdf import ISDF
    df = ISDF(cell, kpts=kpts, c_isdf=c_isdf, select=select, backend=OccKBackend())
    df.pair_space = space
    return df


@pytest.mark.parametrize('select', ['refined', 'local'])
def test_host_driver_fits_the_occupied_pairs_at_k_points(select):
    """pair_space='occ' at k-points: build() stops after the per-atom candidates; get_jk with a per-k tagged density picks the
    points from the occupied-pair Gram matrix of the candidates ('refined'), fits in that pair space and returns the
    restatement's K on those points; J is the pair_space='ao' object's J bit for bit."""
    cell, kpts, mo, occ, dms = _diamond()
    df = _df(cell, kpts, 'occ', select)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        df.build()
    assert df._fit_pending and df._Wq is None
    vj, vk = df.get_jk(_tag(dms, mo, occ), kpts=kpts)
    assert not df._fit_pending
    orbs = [mo[k][:, :2] * np.sqrt(2.0) for k in range(len(kpts))]
    k_ref, X, Psi = kr.restated_k(df, cell, kpts, orbs, dms)
    assert abs(vk - k_ref).max() < 1e-10 * abs(k_ref).max()
    if select == 'refined':
        cand = np.concatenate(df._ksel['per_atom'])
        want = kr.refine_pick_occ(X, Psi, cand, int(df._ksel['nip_final'].sum()), tol=df.select_tol, tie_rtol=df.tie_rtol)
        assert sorted(want) == sorted(df.ip)
    ref = _df(cell, kpts, 'ao', select)
    vj_ao, vk_ao = ref.get_jk(dms, kpts=kpts)
    assert np.array_equal(vj, vj_ao)
    assert abs(vk - vk_ao).max() > 1e-9                  # a different fit
    # untagged: the same occupied space through the eigenvectors - no refit
    fits = df.timings['S3_fit']
    vk2 = df.get_jk(dms, kpts=kpts, with_j=False)[1]
    assert df.timings['S3_fit'] == fits and abs(vk2 - vk).max() < 1e-12


def test_host_driver_refit_rules_and_ao_pair_fallbacks():
    """A full-rank response density and get_ao_eri take the Bloch AO pairs (the pair_space='ao' result); occ_refit='once' keeps
    the first fit; another occupied space refits under 'always' and drops the range-separated W^q; nset = 2 puts both sets'
    orbitals side by side."""
    cell, kpts, mo, occ, dms = _diamond()
    nao = cell.nao_nr()
    nk = len(kpts)
    ao = _df(cell, kpts, 'ao')
    df = _df(cell, kpts, 'occ')
    rng = np.random.default_rng(3)
    z = rng.standard_normal((nk, nao, nao)) + 1j * rng.standard_normal((nk, nao, nao))
    resp = z + z.conj().transpose(0, 2, 1)                      # Hermitian, indefinite, full rank
    vk_ao = ao.get_jk(resp, kpts=kpts, with_j=False)[1]
    vk = df.get_jk(resp, kpts=kpts, with_j=False)[1]
    assert abs(vk - vk_ao).max() < 1e-12 * abs(vk_ao).max()
    assert df._fit_dm is None
    # an MO-tagged density now refits ('always'); the omega W^q of the AO fit are dropped
    df.get_jk(_tag(dms, mo, occ), kpts=kpts, with_j=False, omega=0.4)
    assert list(df._W_omega) == [0.4]
    occ2 = np.zeros_like(occ)
    occ2[:, 1:3] = 2.0
    dms2 = np.einsum('kpi,ki,kqi->kpq', mo, occ2, mo.conj())
    vk2 = df.get_jk(_tag(dms2, mo, occ2), kpts=kpts, with_j=False)[1]
    assert df._W_omega == {}
    orbs2 = [mo[k][:, 1:3] * np.sqrt(2.0) for k in range(nk)]
    assert abs(vk2 - kr.restated_k(df, cell, kpts, orbs2, dms2)[0]).max() < 1e-10 * abs(vk2).max()
    # 'once': the fit for dms2 stays
    df.occ_refit = 'once'
    ip = df.ip.copy()
    vk3 = df.get_jk(_tag(dms, mo, occ), kpts=kpts, with_j=False)[1]
    assert np.array_equal(ip, df.ip)
    assert abs(vk3 - kr.restated_k(df, cell, kpts, orbs2, dms)[0]).max() < 1e-10 * abs(vk3).max()
    # nset = 2 (spins): tags (nset, nk, N, nmo), the orbitals of both sets side by side at every k-point
    df2 = _df(cell, kpts, 'occ')
    occa = np.zeros_like(occ); occa[:, :2] = 1.0
    occb = np.zeros_like(occ); occb[:, :1] = 1.0
    dma = np.einsum('kpi,ki,kqi->kpq', mo, occa, mo.conj())
    dmb = np.einsum('kpi,ki,kqi->kpq', mo, occb, mo.conj())
    vks = df2.get_jk(_tag(np.array([dma, dmb]), np.array([mo, mo]), np.array([occa, occb])), kpts=kpts, with_j=False)[1]
    orbs = [np.hstack([mo[k][:, :2], mo[k][:, :1]]) for k in range(nk)]
    for s, d in enumerate((dma, dmb)):
        assert abs(vks[s] - kr.restated_k(df2, cell, kpts, orbs, d)[0]).max() < 1e-10 * abs(vks[s]).max()
    # get_ao_eri: the Bloch AO pairs
    df3 = _df(cell, kpts, 'occ')
    eri = df3.get_ao_eri(kpts=kpts[1:2])
    assert abs(eri - ao.get_ao_eri(kpts=kpts[1:2])).max() < 1e-12 * abs(eri).max()


def test_unsupported_settings_keep_the_ao_pairs_and_warn():
    """robust_k, the block-Jacobi route and select='global' keep today's behaviour: a warning, then the Bloch AO pairs."""
    cell, kpts, mo, occ, dms = _diamond()
    for setting in ('fit_route', 'global'):
        df = _df(cell, kpts, 'occ', select='global' if setting == 'global' else 'refined')
        ref = _df(cell, kpts, 'ao', select='global' if setting == 'global' else 'refined')
        if setting == 'fit_route':
            df.fit_route = ref.fit_route = 'blockjacobi'
        with pytest.warns(UserWarning, match="pair_space='occ'"):
            vk = df.get_jk(_tag(dms, mo, occ), kpts=kpts, with_j=False)[1]
        vk_ao = ref.get_jk(dms, kpts=kpts, with_j=False)[1]
        assert np.array_equal(vk, vk_ao)
