"""pair_space='occ' at k-points on the GPU: the two (AO x occupied) products of the C ABI against numpy,
and the k-point exchange of a converged KRKS density against the numpy restatement (tests/kocc_reference.py) and the exact
exchange."""
import warnings
import numpy as np
import pytest
import torch
import cells
import kocc_reference as kr
import scf_helpers
from pyscf_isdf_amd import gto
from pyscf_isdf_amd._common import tag_array

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def be():
    from pyscf_isdf_amd.backend import HipBackend
    return HipBackend(0)


@pytest.mark.parametrize('P,nh,npsi_h,ng,pad', [(37, 10, 1, 1000, 3), (37, 10, 7, 65536 + 301, 0), (1100, 16, 5, 130001, 1)])
def test_occupied_pair_products_match_numpy(be, P, nh, npsi_h, ng, pad):
    """isdf_gram_prod_cplx and isdf_pair_prod_rows_cplx against numpy, 1e-12 relative: P not a multiple of any tile, ng across
    the column chunks (65536 and 60928 columns here), leading dimensions > ng (odd ones: the combine's 8-byte path), nocc = 1."""
    from pyscf_isdf_amd import lib
    assert lib.ABI_VERSION == 21 and lib.load().isdf_abi_version() == 21
    rng = np.random.default_rng(P + ng)
    X = rng.standard_normal((2 * nh, ng + pad))
    Psi = rng.standard_normal((2 * npsi_h, ng + pad))
    aoP = np.ascontiguousarray(rng.standard_normal((P, 2 * nh)))
    psiP = np.ascontiguousarray(rng.standard_normal((P, 2 * npsi_h)))
    A = be.empty((P, P))
    be.gram_prod_cplx(be.to_device(aoP), nh, be.to_device(psiP), npsi_h, A)
    A_ref = kr.gram_occ(aoP, psiP)
    assert abs(be.to_host(A) - A_ref).max() <= 1e-12 * abs(A_ref).max()
    Bfull = be.zeros((P, ng + 2 * pad + 1))
    B = Bfull[:, pad:pad + ng]
    be.pair_prod_rows_cplx(be.to_device(aoP), nh, be.to_device(psiP), npsi_h, be.to_device(X)[:, :ng], be.to_device(Psi)[:, :ng],
                           ng, B)
    B_ref = kr.rows_occ(aoP, psiP, X[:, :ng], Psi[:, :ng])
    got = be.to_host(Bfull)
    assert abs(got[:, pad:pad + ng] - B_ref).max() <= 1e-12 * abs(B_ref).max()
    assert not got[:, :pad].any() and not got[:, pad + ng:].any()          # nothing written outside the columns


def _newton_cell():
    # pyscf/pbc/scf/test/test_newton.py:25-44
    return gto.Cell(unit='B', atom='C 0. 0. 0.; C 1.68506879 1.68506879 1.68506879',
                    a=[[0., 3.37013758, 3.37013758], [3.37013758, 0., 3.37013758], [3.37013758, 3.37013758, 0.]],
                    basis='gth-szv', pseudo='gth-pade', mesh=[19] * 3)


@pytest.fixture(scope='module')
def krks():
    """Converged KRKS 'lda,' on the diamond primitive cell, 2x1x1 k-mesh (as tests/test_gpu_scf.py), then the orbitals of the
    final Fock matrix: the density tagged per k-point as PySCF's make_rdm1 tags it."""
    from pyscf_isdf_amd import multigrid as pmg
    cell = _newton_cell()
    kpts = cell.make_kpts([2, 1, 1])
    S, T = scf_helpers.overlap_kinetic_from_ft_kpts(cell, kpts)
    mg = pmg.MultiGridFFTDF(cell, kpts=kpts)
    mg.split = 'all'
    hcore = T + np.asarray(mg.get_pp(kpts))
    e_nuc = scf_helpers.ewald_energy(cell)

    def veff(dms):
        n, exc, v = pmg.nr_rks(mg, 'lda,', dms, kpts=kpts, with_j=True)
        return np.asarray(v), float(v.ecoul), float(exc)
    e_tot, dms = scf_helpers.krks(hcore, S, veff, 4, e_nuc)
    assert abs(e_tot - (-10.307756038726733)) < 5e-8
    import scipy.linalg
    f = hcore + veff(dms)[0]
    nao = cell.nao_nr()
    mo, occ = [], []
    for k in range(len(kpts)):
        c = scipy.linalg.eigh(f[k], S[k])[1]
        mo.append(c)
        o = np.zeros(nao)
        o[:4] = 2.0
        occ.append(o)
    mo, occ = np.array(mo), np.array(occ)
    dms = np.einsum('kpi,ki,kqi->kpq', mo, occ, mo.conj())
    return cell, kpts, mo, occ, dms


def _isdf(cell, kpts, space, c_isdf, **kw):
    from pyscf_isdf_amd.isdf import ISDF
    df = ISDF(cell, kpts=kpts, c_isdf=c_isdf, select='refined')
    df.pair_space = space
    for k, v in kw.items():
        setattr(df, k, v)
    return df


def _orbs(mo, occ):
    return [m[:, o > 0] * np.sqrt(o[o > 0]) for m, o in zip(mo, occ)]


def test_krks_density_occupied_pairs_match_restatement(krks):
    """(b) The exchange of the tagged KRKS density with pair_space='occ' equals the restatement's on the same points (1e-8
    of |K|); J is bit for bit the pair_space='ao' object's J."""
    cell, kpts, mo, occ, dms = krks
    df = _isdf(cell, kpts, 'occ', 4)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        vj, vk = df.get_jk(tag_array(dms, mo_coeff=mo, mo_occ=occ), kpts=kpts)
    k_ref = kr.restated_k(df, cell, kpts, _orbs(mo, occ), dms)[0]
    err = abs(vk - k_ref).max()
    print('occ pairs vs restatement: max|dK| = %.2e (|K| %.2f), P = %d' % (err, abs(k_ref).max(), len(df.ip)))
    assert err < 1e-8 * abs(k_ref).max()
    ref = _isdf(cell, kpts, 'ao', 4)
    vj_ao, vk_ao = ref.get_jk(dms, kpts=kpts)
    assert np.array_equal(vj, vj_ao)
    assert abs(vk - vk_ao).max() > 1e-9


def test_occupied_pairs_beat_ao_pairs_at_equal_points(krks):
    """(c) At equal c_isdf (4: 64 points), against the exact k-point exchange (get_k_exact): the (AO x occupied) fit's |dE_K| is
    at least 2x smaller than the Bloch AO pairs' (measured 3.5e-3 against 4.0e-2 Eh: 11.6x), and its max|dK| is no worse
    within 25 % (measured 2.13e-2 against 2.31e-2: the element-wise error does not follow the energy)."""
    cell, kpts, mo, occ, dms = krks
    tagged = tag_array(dms, mo_coeff=mo, mo_occ=occ)
    nk = len(kpts)
    out = {}
    for space in ('ao', 'occ'):
        df = _isdf(cell, kpts, space, 4)
        vk = df.get_jk(tagged, kpts=kpts, with_j=False)[1]
        if space == 'ao':
            k_ex = df.get_k_exact(tagged)
        dk = vk - k_ex
        out[space] = (abs(dk).max(), abs(np.einsum('kij,kji', dms, dk).real) / (4 * nk))
    print('c = 4: ao max|dK| %.2e dE_K %.2e | occ max|dK| %.2e dE_K %.2e | ratios %.1f %.1f' %
          (out['ao'] + out['occ'] + (out['ao'][0] / out['occ'][0], out['ao'][1] / out['occ'][1])))
    assert out['occ'][1] * 2 < out['ao'][1]
    assert out['occ'][0] < 1.25 * out['ao'][0]


def test_occupied_pair_semantics(krks):
    """(d) An untagged density gives the tagged result; nset = 2; a band k-point matches the restatement; a full-rank response
    density gives the pair_space='ao' K; occ_refit='once' keeps the first fit."""
    cell, kpts, mo, occ, dms = krks
    nk, nao = len(kpts), cell.nao_nr()
    tagged = tag_array(dms, mo_coeff=mo, mo_occ=occ)
    df = _isdf(cell, kpts, 'occ', 3)
    vk = df.get_jk(tagged, kpts=kpts, with_j=False)[1]
    df_u = _isdf(cell, kpts, 'occ', 3)
    vk_u = df_u.get_jk(dms, kpts=kpts, with_j=False)[1]
    assert abs(vk_u - vk).max() < 1e-10 * abs(vk).max()
    # nset = 2: the spins of a KUHF-like density, tags (nset, nk, N, nmo)
    occa = np.zeros_like(occ)                                  # 2 + 1 orbitals side by side: rank 3 <= N/2 at every k-point
    occa[:, :2] = 1.0
    occb = np.zeros_like(occ)
    occb[:, :1] = 1.0
    dma = np.einsum('kpi,ki,kqi->kpq', mo, occa, mo.conj())
    dmb = np.einsum('kpi,ki,kqi->kpq', mo, occb, mo.conj())
    df2 = _isdf(cell, kpts, 'occ', 3)
    vks = df2.get_jk(tag_array(np.array([dma, dmb]), mo_coeff=np.array([mo, mo]), mo_occ=np.array([occa, occb])), kpts=kpts,
                     with_j=False)[1]
    orbs = [np.hstack([a, b]) for a, b in zip(_orbs(mo, occa), _orbs(mo, occb))]
    for s, d in enumerate((dma, dmb)):
        ref = kr.restated_k(df2, cell, kpts, orbs, d)[0]
        assert abs(vks[s] - ref).max() < 1e-8 * abs(ref).max()
    # a band k-point off the mesh
    kb = np.array([[0.1, 0.2, -0.05]])
    df3 = _isdf(cell, kpts, 'occ', 3)
    vkb = df3.get_jk(tagged, kpts=kpts, kpts_band=kb, with_j=False)[1]
    ref = kr.restated_k(df3, cell, kpts, _orbs(mo, occ), dms, kpts_band=kb)[0]
    assert abs(np.asarray(vkb).reshape(ref.shape) - ref).max() < 1e-8 * abs(ref).max()
    # a full-rank response density: the Bloch AO pairs
    rng = np.random.default_rng(2)
    z = rng.standard_normal((nk, nao, nao)) + 1j * rng.standard_normal((nk, nao, nao))
    resp = z + z.conj().transpose(0, 2, 1)
    vk_r = df.get_jk(resp, kpts=kpts, with_j=False)[1]
    vk_ao = _isdf(cell, kpts, 'ao', 3).get_jk(resp, kpts=kpts, with_j=False)[1]
    assert abs(vk_r - vk_ao).max() < 1e-12 * abs(vk_ao).max()
    # occ_refit='once': the first fit (for the tagged density) stays for another occupied space
    df4 = _isdf(cell, kpts, 'occ', 3, occ_refit='once')
    df4.get_jk(tagged, kpts=kpts, with_j=False)
    occ2 = np.zeros_like(occ)
    occ2[:, 1:5] = 2.0
    dm2 = np.einsum('kpi,ki,kqi->kpq', mo, occ2, mo.conj())
    vk2 = df4.get_jk(tag_array(dm2, mo_coeff=mo, mo_occ=occ2), kpts=kpts, with_j=False)[1]
    ref = kr.restated_k(df4, cell, kpts, _orbs(mo, occ), dm2)[0]
    assert abs(vk2 - ref).max() < 1e-8 * abs(ref).max()


class _AlwaysComm:
    """A one-rank communicator that issues its collectives (the multi-rank code path's switch), the collectives no-ops."""
    rank, size, local_rank, always = 0, 1, 0, True

    def all_reduce_sum(self, t):
        return t

    def agree_max(self, x):
        return x


@pytest.mark.parametrize('kind', ['multirank', 'robust_k'])
def test_unsupported_settings_warn_and_keep_ao_pairs(krks, kind):
    """(d) A multi-rank-style object and robust_k keep today's behaviour: the warning, then the Bloch AO pairs."""
    from pyscf_isdf_amd.isdf import ISDF
    cell, kpts, mo, occ, dms = krks
    tagged = tag_array(dms, mo_coeff=mo, mo_occ=occ)
    out = []
    for space in ('occ', 'ao'):
        df = ISDF(cell, kpts=kpts, c_isdf=3, select='refined', comm=_AlwaysComm() if kind == 'multirank' else None)
        df.pair_space = space
        df.robust_k = kind == 'robust_k'
        if space == 'occ':
            with pytest.warns(UserWarning, match="pair_space='occ'"):
                out.append(df.get_jk(tagged, kpts=kpts, with_j=False)[1])
        else:
            out.append(df.get_jk(dms, kpts=kpts, with_j=False)[1])
    assert abs(out[0] - out[1]).max() <= 1e-12 * abs(out[1]).max()
