"""get_k_nuc_grad / get_jk_nuc_grad (pyscf_isdf_amd/jk_e1.py) on the CPU, checker backend: the contracted exchange force against
the host contraction of get_k_e1 (existing code), against the half-fitted formula written directly, in the exact limit against
the exact restatement and finite differences of the oracle's exchange energy, then the orchestration and the refusals.

Setup of tests/test_jk_e1.py: diamond primitive cell, gth-szv, 12^3 (8 AOs, G = 1728), c_isdf = 3 'local' (P = 24), robust_k.

Measured on the checker backend (relative to max|f|): contracted route against the matrix route 4.2e-15 (low rank), 5.5e-15 (full
rank), 6.1e-15 (non-symmetric), 4.6e-15 (stack), 6.8e-15 ('occ'); against the formula written directly 6.7e-15, 7.8e-15 and
1.3e-14.  The bound is ten times the largest, 1.3e-13: far below the 1e-10 at which a mismatch would be a defect.
Exact limit ('global', c_isdf = 5): plain K mismatch 3.4e-15 of max|K|, force against the exact restatement contracted 1.9e-14
(inside ten times the K mismatch).  c_isdf = 3: the force's error against the exact restatement is 1.3e-1 of max|f| (first order
in the fit error, and the force sums many matrix entries of either sign; printed, not bounded)."""
import numpy as np
import pytest
from pyscf_isdf_amd import gto
from pyscf_isdf_amd.isdf import ISDF
from oracle import isdf as oisdf, fftdf
import e1_reference as e1
from k_grad_backend import KGradOracleBackend, KGradPlainBackend
from test_jk_e1 import _Setup, EXACT_C

ROUTE_BOUND = 1.3e-13          # 10 x the largest measured mismatch of the two float64 orders of one sum (module docstring)


def _df(su, backend=None, c=3, select='local', robust=True, pair_space='ao'):
    df = ISDF(su.cell, c_isdf=c, select=select, backend=backend or KGradOracleBackend())
    df.robust_k, df.pair_space = robust, pair_space
    return df


def contract(cell, vk, dm):
    """2 sum_(mu in A) sum_nu vk[x, mu, nu] dm_sym[nu, mu] on the host: (natm, 3), or (nset, natm, 3) for vk (3, nset, nao, nao)."""
    d = np.asarray(dm, dtype=float)
    d = 0.5 * (d + d.swapaxes(-1, -2))
    rows = 2.0 * np.einsum('x...mn,...nm->...xm', vk, d)
    f = np.stack([rows[..., int(p0):int(p1)].sum(axis=-1) for p0, p1 in cell.aoslice_by_atom()[:, :2]], axis=-1)
    return f.swapaxes(-1, -2)


def _rel(x, ref):
    return float(abs(x - ref).max() / abs(ref).max())


@pytest.fixture(scope='module')
def su():
    return _Setup()


@pytest.fixture(scope='module')
def built(su):
    df = _df(su)
    fk = df.get_k_nuc_grad(su.dm)
    theta = oisdf.fit_theta_global_chol(su.aoT, df.ip, reg_rel=df.reg_used)
    return df, fk, theta


def _full_rank(su):
    rng = np.random.default_rng(5)
    x = rng.standard_normal((su.nao, su.nao))
    return x + x.T


# ---- (a) the contracted route is the matrix route -------------------------------------------------------------------------------
def test_contracted_route_equals_the_matrix_route(su, built):
    df, fk, theta = built
    natm = su.cell.natm
    assert fk.shape == (natm, 3) and fk.dtype == np.float64
    assert len(df.backend.nn_had_calls) > 0 and 'S8_get_k_nuc_grad' in df.timings
    worst = 0.0
    for name, dm in (('low rank', su.dm), ('full rank', _full_rank(su)), ('non-symmetric', su.dn)):
        sym = 0.5 * (dm + dm.T)
        f = df.get_k_nuc_grad(dm)
        ref = contract(su.cell, df.get_k_e1(sym), sym)
        direct = contract(su.cell, e1.get_k_e1_isdf(su.aoT, su.dao, df.ip, theta, sym, su.a, su.mesh), sym)
        print('%-14s |contracted - matrix| / max = %.3e   |contracted - formula| / max = %.3e' % (name, _rel(f, ref), _rel(f, direct)))
        worst = max(worst, _rel(f, ref), _rel(f, direct))
        assert _rel(f, ref) <= ROUTE_BOUND and _rel(f, direct) <= ROUTE_BOUND
    stack = np.array([su.dm, su.dn])
    fs = df.get_k_nuc_grad(stack)
    assert fs.shape == (2, natm, 3)
    sym = 0.5 * (stack + stack.transpose(0, 2, 1))
    ref = contract(su.cell, df.get_k_e1(sym), sym)
    assert ref.shape == fs.shape
    print('stack          |contracted - matrix| / max = %.3e' % _rel(fs, ref))
    worst = max(worst, _rel(fs, ref))
    assert _rel(fs, ref) <= ROUTE_BOUND
    assert _rel(fs[0], fk) <= 1e-13 and _rel(fs[1], df.get_k_nuc_grad(su.dn)) <= 1e-13
    print('largest mismatch of (a): %.3e' % worst)


def test_occ_pair_space():
    """pair_space='occ' on gth-dzvp at c_isdf = 4: the force goes through _ensure_fit(dm) and uses that fit's V."""
    so = _Setup('gth-dzvp')
    df = _df(so, c=4, pair_space='occ')
    f = df.get_k_nuc_grad(so.dm)
    assert df._fit_dm is not None
    ref = contract(so.cell, df.get_k_e1(so.dm), so.dm)
    print('occ pair space |contracted - matrix| / max = %.3e' % _rel(f, ref))
    assert _rel(f, ref) <= ROUTE_BOUND


# ---- (b) the exact limit ----------------------------------------------------------------------------------------------------------
def test_exact_limit_and_finite_differences(su, built):
    df = _df(su, c=EXACT_C, select='global')
    f = df.get_k_nuc_grad(su.dm)
    k_isdf = oisdf.get_k(df.backend.to_host(df.aoP), df.backend.to_host(df.W), su.dm)
    k_exact = fftdf.get_k(su.ao4[0], su.dm, su.a, su.mesh)
    mismatch = _rel(k_isdf, k_exact)
    ref = contract(su.cell, su.vk_ref, su.dm)
    err = _rel(f, ref)
    print('c_isdf = %d global: P = %d, plain K mismatch %.3e, force mismatch %.3e' % (EXACT_C, len(df.ip), mismatch, err))
    print('c_isdf = 3: |force - exact| / max = %.3e' % _rel(built[1], ref))
    assert mismatch < 1e-9
    assert err <= 10 * mismatch
    # d[1/2 tr(K D)] / dR_(1, x) by central differences of the oracle, the rule of test_restatement_matches_finite_differences_of_the_oracle
    cell, dm = su.cell, su.dm
    ptr = int(np.asarray(cell._atm)[1, gto.PTR_COORD])

    def energy(env):
        return 0.5 * np.einsum('ij,ji', fftdf.get_k(su.collocate(env)[0], dm, su.a, su.mesh), dm)

    for x in range(3):
        fd = {}
        for h in (2e-3, 1e-3):
            ep, em = np.array(cell._env, dtype=float), np.array(cell._env, dtype=float)
            ep[ptr + x] += h
            em[ptr + x] -= h
            fd[h] = (energy(ep) - energy(em)) / (2 * h)
        own = abs(fd[2e-3] - fd[1e-3])
        diff = abs(f[1, x] - fd[1e-3])
        print('axis %d: analytic %.10e  fd %.10e  |diff| %.2e  fd own error %.2e' % (x, f[1, x], fd[1e-3], diff, own))
        assert own > 0 and diff <= 10 * own, (x, diff, own)


# ---- (c) orchestration ------------------------------------------------------------------------------------------------------------
def test_chunks_row_batches_composition_and_the_pair_of_calls(su, built):
    df, fk, theta = built
    be = df.backend
    assert df.k_grad_fused is True and df.e1_grid_chunk == 65536 and df.e1_row_batch is None
    del be.nn_had_calls[:]
    assert _rel(df.get_k_nuc_grad(su.dm), fk) == 0.0
    assert be.nn_had_calls == [0.0]                                   # one chunk, one batch of 24 points
    assert _rel(df.get_k_nuc_grad(su.dm, exxdiv='ewald'), fk) == 0.0    # the G = 0 term has no gradient
    df.e1_grid_chunk = 500                                            # 1728 = 3 * 500 + 228
    try:
        sizes = [s1 - s0 for s0, s1, _ in df._e1_chunks()]
        assert sizes == [500, 500, 500, 228]
        del be.nn_had_calls[:]
        fc = df.get_k_nuc_grad(su.dm)
        assert be.nn_had_calls == [0.0] * 4
        df.e1_row_batch = 7                                           # 24 = 3 * 7 + 3: beta = 0 on the first batch, 1 after
        del be.nn_had_calls[:]
        fb = df.get_k_nuc_grad(su.dn)
        assert be.nn_had_calls == [0.0, 1.0, 1.0, 1.0] * 4
    finally:
        df.e1_grid_chunk, df.e1_row_batch = 65536, None
    assert _rel(fc, fk) <= 1e-13 and _rel(fb, df.get_k_nuc_grad(su.dn)) <= 1e-13
    del be.nn_had_calls[:]
    df.k_grad_fused = False
    try:
        assert _rel(df.get_k_nuc_grad(su.dm), fk) <= 1e-13 and be.nn_had_calls == []
    finally:
        df.k_grad_fused = True
    df.k_grad_fused_max_rank = 3                                      # D has 4 occupied orbitals: above the knob, the composition
    try:
        assert _rel(df.get_k_nuc_grad(su.dm), fk) <= 1e-13 and be.nn_had_calls == []
    finally:
        df.k_grad_fused_max_rank = 256
    plain = _df(su, backend=KGradPlainBackend())                     # a backend without gemm_nn_had: the composition
    assert not hasattr(plain.backend, 'gemm_nn_had')
    assert _rel(plain.get_k_nuc_grad(su.dm), fk) <= 1e-13
    fj, fk2 = df.get_jk_nuc_grad(su.dm)
    assert np.array_equal(fj, df.get_j_nuc_grad(su.dm))               # the J half, operation by operation
    assert _rel(fk2, fk) == 0.0
    sj, sk = df.get_jk_nuc_grad(np.array([su.dm, su.dn]))
    assert sj.shape == sk.shape == (2, su.cell.natm, 3)
    assert np.array_equal(sj, df.get_j_nuc_grad(np.array([su.dm, su.dn])))
    assert _rel(sk[0], fk) <= 1e-13


def test_multigrid_object_gives_the_same_force(su, built):
    from pyscf_isdf_amd import multigrid as pmg
    df = pmg.MultiGridFFTDF(su.cell, c_isdf=3, select='local', backend=KGradOracleBackend())
    df.robust_k = True
    assert _rel(df.get_k_nuc_grad(su.dm), built[1]) <= 1e-13
    assert len(df.backend.nn_had_calls) > 0


# ---- (d) refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_a_build(su):
    dm = su.dm
    kpt = np.array([[0.1, 0.2, 0.3]])
    for name in ('get_k_nuc_grad', 'get_jk_nuc_grad'):
        df = _df(su)
        with pytest.raises(NotImplementedError, match='k-points'):
            getattr(df, name)(dm, kpts=kpt)
        for ex in ('vcut_sph', 'vcut_ws', 'None'):
            with pytest.raises(NotImplementedError, match='exxdiv'):
                getattr(df, name)(dm, exxdiv=ex)
        with pytest.raises(ValueError, match='real density matrix'):
            getattr(df, name)(dm + 1j * su.dn)
        assert not df._built
        dk = ISDF(su.cell, kpts=kpt, backend=KGradOracleBackend())
        dk.robust_k = True
        with pytest.raises(NotImplementedError, match='k-points'):
            getattr(dk, name)(dm)
        assert not dk._built
        db = _df(su)
        db.kpts_band = kpt
        with pytest.raises(NotImplementedError, match='kpts_band'):
            getattr(db, name)(dm)
        assert not db._built
        ds = _df(su)
        ds.kpts_symm = object()
        with pytest.raises(NotImplementedError, match='k-point symmetry'):
            getattr(ds, name)(dm)
        assert not ds._built
        sh = _df(su)
        sh.force_sharded = True
        with pytest.raises(NotImplementedError, match='sharded'):
            getattr(sh, name)(dm)
        assert not sh._built
        om = _df(su)
        with om.range_coulomb(0.3) as rdf:
            with pytest.raises(NotImplementedError, match='omega'):
                getattr(rdf, name)(dm)
        assert not om._built
        norob = _df(su, robust=False)
        with pytest.raises(RuntimeError, match='robust_k needs a build with robust_k=True'):
            getattr(norob, name)(dm)
        assert not norob._built
