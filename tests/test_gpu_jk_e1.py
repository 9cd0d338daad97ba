"""isdf_gemm_nt_had3 and get_j_e1 / get_k_e1 / get_jk_e1 on the device.

Kernel sweep, in the manner of test_gpu_gemm_sweep.py's exact reference: small-integer operands (entries in [-4, 4], alpha and
beta powers of two: every partial sum is an integer far below 2^53, so numpy's float64 result IS the answer), np.array_equal.
M in {1, 15, 16, 17, 127, 128, 129, 300} x N in {1, 13, 128, 130} x K in {3, 16, 31, 32, 48, 2047, 6160}, with and without H;
lda = K + 2, ldh = K + 4, ldb = K + 6, the three B and the three C more than one matrix apart; NaN in every padding of A, H and
B, a sentinel around and between the C that must stay bit-unchanged; (alpha, beta) = (1, 0) onto NaN, (0.5, -2), (-1, 1).  What
ran is read from the profiling labels: the one-launch kernel for K % 16 == 0 (one chunk, a pair, a pair and an odd one, and
K = 6160 in three slabs of 129 / 129 / 127 chunks, run twice bit-identically), the composition (hadamard_rows + three NT
products) for the odd K, whose lda is odd, and for an A base off by one double.

Rounding: Gaussian data, one case per path (one launch direct, one launch in slabs, composition), against an np.longdouble
product under test_gpu_gemm_sweep's ROUNDING_FACTOR rule.  Measured on an MI355X, device error / numpy error per component:
4.42 / 3.83 / 2.64 (one launch, 129 x 65 x 2048), 2.38 / 3.50 / 2.29 (three slabs, K = 6160), 3.02 / 3.60 / 2.75 (composition,
K = 2047) - inside the 4.69 that module's factor of 32 was derived from.

Product: the checks of tests/test_jk_e1.py on the device - the K side at 1e-8 of max (the bound of
test_robust_k_matches_oracle_and_reduces_the_error), the J side at 1e-10 (the bound of the get_j parity tests) - the exact
limit, and one (AO x occupied) pair-space case."""
import numpy as np
import pytest
import cells
from pyscf_isdf_amd import gto
from oracle import ao as oao, isdf as oisdf, fftdf
import e1_reference as e1
from test_gpu_gemm_sweep import ROUNDING_FACTOR, SENTINEL, REDUCE, _ints, _profiled, _rel_err

gpu = pytest.mark.gpu

HAD3 = {True: 'gemm_nt_had3_kernel<true>[flop]', False: 'gemm_nt_had3_kernel<false>[flop]'}
HADAMARD = 'hadamard_rows_kernel[byte]'
SWEEP_M = (1, 15, 16, 17, 127, 128, 129, 300)
SWEEP_N = (1, 13, 128, 130)
SWEEP_K = (3, 16, 31, 32, 48, 2047, 6160)
SCALARS = ((1.0, 0.0), (0.5, -2.0), (-1.0, 1.0))
PAD = 2


@pytest.fixture(scope='module')
def be():
    from pyscf_isdf_amd.backend import HipBackend
    b = HipBackend(0)
    b.prof_enable(True)
    yield b
    b.prof_enable(False)
    b.prof_reset()
    b.release_workspace()


def _window(buf, first, shape, strides):
    return np.lib.stride_tricks.as_strided(buf[first:], shape=shape, strides=tuple(8 * s for s in strides))


class _Had3Run:
    """One isdf_gemm_nt_had3 case: operands embedded in NaN (A, H, B) or the sentinel (C), PAD rows before and after."""

    def __init__(self, be, M, N, K, had, alpha, beta, rng, off_a=0, gaussian=False):
        self.be, self.M, self.N, self.K, self.had, self.alpha, self.beta = be, M, N, K, had, alpha, beta
        draw = (lambda shape: rng.standard_normal(shape)) if gaussian else (lambda shape: _ints(rng, shape, 4))
        lda, ldh, ldb, ldc = K + 2, K + 4, K + 6, N + 3
        bstride, cstride = (N + 3) * ldb, (M + 2) * ldc + 1
        self.A, self.H, self.B = draw((M, K)), (draw((M, K)) if had else None), draw((3, N, K))
        self.C0 = np.full((3, M, N), np.nan) if beta == 0.0 else draw((3, M, N))

        def dev(mat, shape, strides, span, fill, off=0):
            buf = np.full(off + 2 * PAD * strides[-2] + span, fill)
            first = off + PAD * strides[-2]
            _window(buf, first, shape, strides)[...] = mat
            d = be.to_device(buf)
            return buf, d, d.as_strided(shape, strides, first)
        _, _, self.dA = dev(self.A, (M, K), (lda, 1), M * lda, np.nan, off_a)
        self.dH = dev(self.H, (M, K), (ldh, 1), M * ldh, np.nan)[2] if had else None
        _, _, self.dB = dev(self.B, (3, N, K), (bstride, ldb, 1), 3 * bstride, np.nan)
        self.c_layout = ((3, M, N), (cstride, ldc, 1), 3 * cstride)
        self._dev = dev
        assert self.dA.data_ptr() % 16 == 8 * (off_a % 2) and self.dB.data_ptr() % 16 == 0
        self.fused = K % 16 == 0 and off_a % 2 == 0               # lda = K + 2 is even exactly when K is

    def launch(self):
        shape, strides, span = self.c_layout
        self.c_host, self.c_dev, self.dC = self._dev(self.C0, shape, strides, span, SENTINEL)
        self.be.gemm_nt_had3(self.dA, self.dH, self.dB, self.dC, alpha=self.alpha, beta=self.beta)

    def fetch(self):
        """(the three windows, whether everything around them is bit-unchanged)."""
        shape, strides, _ = self.c_layout
        after, before = self.be.to_host(self.c_dev), self.c_host.copy()
        first = PAD * strides[-2]
        win = _window(after, first, shape, strides).copy()
        for buf in (after, before):
            _window(buf, first, shape, strides)[...] = 0.0
        return win, np.array_equal(after.view(np.int64), before.view(np.int64))

    def ref(self, cast=lambda x: x):
        ah = cast(self.A) * cast(self.H) if self.had else cast(self.A)
        out = [cast(self.alpha) * ah.dot(cast(self.B[x]).T) + (cast(self.beta) * cast(self.C0[x]) if self.beta != 0.0 else 0)
               for x in range(3)]
        return np.array(out)

    def check_labels(self, prof, bad):
        """The one-launch kernel (with the slab reduction exactly when K is cut), or the composition: no had3 label, three NT
        launches, the Hadamard pass exactly when there is an H."""
        M, N, K = self.M, self.N, self.K
        nt = sum(v['launches'] for k, v in prof.items() if k.startswith('gemm_nt_mfma_kernel'))
        if self.fused:
            nslab = 3 if K >= 6144 else 1
            want = {HAD3[self.had]} | ({REDUCE} if nslab > 1 else set())
            if set(prof) != want:
                bad.append('ran %s, expected %s' % (sorted(prof), sorted(want)))
            elif nslab > 1 and int(round(prof[REDUCE]['work'] / (24.0 * M * N))) - 1 != nslab:
                bad.append('slab reduction work %r is not that of %d slabs' % (prof[REDUCE]['work'], nslab))
        else:
            if any(k in prof for k in HAD3.values()) or nt != 3 or (HADAMARD in prof) != self.had:
                bad.append('expected the composition, ran %s' % sorted(prof))
        return self.fused and K >= 6144


def _sweep_case(be, M, N, K, had, alpha, beta, off_a=0):
    run = _Had3Run(be, M, N, K, had, alpha, beta, np.random.default_rng([M, N, K, int(had)]), off_a=off_a)
    bad = []
    prof = _profiled(be, run.launch)
    multi = run.check_labels(prof, bad)
    win, clean = run.fetch()
    if not clean:
        bad.append('sentinel around C overwritten')
    r = run.ref()
    if not np.array_equal(win, r):
        x, i, j = np.argwhere(win != r)[0]
        bad.append('%d of %d entries differ, first at (%d, %d, %d): got %r, exact %r' % ((win != r).sum(), r.size, x, i, j,
                                                                                         win[x, i, j], r[x, i, j]))
    if multi:
        run.launch()
        again, _ = run.fetch()
        if not np.array_equal(win.view(np.int64), again.view(np.int64)):
            bad.append('two runs on the same inputs differ')
    return bad


@gpu
@pytest.mark.parametrize('K', SWEEP_K)
def test_had3_exact_sweep(be, K):
    fails, n = [], 0
    for M in SWEEP_M:
        for N in SWEEP_N:
            for had in (True, False):
                alpha, beta = SCALARS[n % 3]
                n += 1
                bad = _sweep_case(be, M, N, K, had, alpha, beta)
                if bad:
                    fails.append(('%dx%dx%d had=%s alpha=%g beta=%g' % (M, N, K, had, alpha, beta), bad))
    for name, bad in fails:
        print('FAILED %s: %s' % (name, '; '.join(bad)))
    assert not fails, fails


@gpu
@pytest.mark.parametrize('had', [True, False])
def test_had3_unaligned_base_takes_the_composition(be, had):
    """An aligned shape of the one-launch kernel with the A base off by one double: the labels say composition, the numbers are
    the same exact product."""
    for alpha, beta in SCALARS:
        assert not _sweep_case(be, 129, 130, 32, had, alpha, beta)                   # aligned: one launch
        bad = _sweep_case(be, 129, 130, 32, had, alpha, beta, off_a=1)
        assert not bad, bad


W = 0.7
ROUNDING_CASES = [(129, 65, 2048, W, 0.0), (129, 65, 6160, -1.0, 1.0), (129, 65, 2047, W, 0.0)]


@gpu
@pytest.mark.parametrize('M,N,K,alpha,beta', ROUNDING_CASES)
def test_had3_rounding_against_longdouble(be, M, N, K, alpha, beta):
    """Gaussian operands with H: the device's error against an np.longdouble product may exceed the error of numpy's float64
    evaluation of the same inputs against the same reference by ROUNDING_FACTOR at most (one launch direct, one launch in three
    slabs, composition)."""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63
    run = _Had3Run(be, M, N, K, True, alpha, beta, np.random.default_rng([M, N, K]), gaussian=True)
    bad = []
    prof = _profiled(be, run.launch)
    run.check_labels(prof, bad)
    assert not bad, bad
    win, clean = run.fetch()
    assert clean and np.isfinite(win).all()
    ref = run.ref(lambda x: np.asarray(x, dtype=np.longdouble))
    f64 = run.ref()
    for x in range(3):
        dev, host = _rel_err(win[x], ref[x]), _rel_err(f64[x], ref[x])
        print('rounding had3 %dx%dx%d %s component %d: device %.2e, numpy %.2e, ratio %.2f' %
              (M, N, K, 'one launch' if run.fused else 'composition', x, dev, host, dev / host))
        assert host > 0.0 and dev <= ROUNDING_FACTOR * host, ((M, N, K), dev, host, dev / host)


# ---- the product ----------------------------------------------------------------------------------------------------------------
def _rel(x, ref):
    return float(abs(x - ref).max() / abs(ref).max())


class _Product:
    def __init__(self, basis, c, select='local', pair_space='ao'):
        from pyscf_isdf_amd.isdf import ISDF
        self.cell = cell = cells.cell_diamond_prim(basis, (12, 12, 12))
        self.nao = nao = cell.nao_nr()
        self.a, self.mesh = cell.lattice_vectors(), cell.mesh
        rcut = gto.estimate_rcut_per_shell(cell)
        Ls = gto.get_lattice_Ls(cell, rcut=rcut.max())
        self.ao4 = oao.eval_ao_deriv1(cell._atm, cell._bas, cell._env, cell.get_uniform_grids(), Ls, rcut)
        self.aoT = np.ascontiguousarray(self.ao4[0].T)
        self.dao = np.ascontiguousarray(self.ao4[1:].transpose(0, 2, 1))
        rng = np.random.default_rng(11)
        self.c = np.linalg.qr(rng.standard_normal((nao, nao)))[0]
        self.occ = np.zeros(nao)
        self.occ[:cell.nelectron // 2] = 2
        self.dm = (self.c * self.occ).dot(self.c.T)
        self.dn = self.dm + 0.1 * rng.standard_normal((nao, nao))
        self.df = df = ISDF(cell, c_isdf=c, select=select)
        df.robust_k, df.pair_space = True, pair_space
        df.backend.prof_enable(True)
        df.backend.prof_reset()
        self.vj, self.vk = df.get_jk_e1(self.dm)
        self.labels = set(df.backend.prof_results())
        df.backend.prof_enable(False)


@pytest.fixture(scope='module')
def prod():
    p = _Product('gth-szv', 3)
    p.theta = oisdf.fit_theta_global_chol(p.aoT, p.df.ip, reg_rel=p.df.reg_used)
    return p


@gpu
def test_device_k_e1_is_the_half_fitted_formula_and_j_e1_the_restatement(prod):
    p, df = prod, prod.df
    assert p.vj.shape == p.vk.shape == (3, p.nao, p.nao)
    assert HAD3[True] in p.labels, sorted(p.labels)               # 1728 columns = 108 chunks of 16, aligned: the one launch ran
    assert _rel(p.vk, e1.get_k_e1_isdf(p.aoT, p.dao, df.ip, p.theta, p.dm, p.a, p.mesh)) < 1e-8
    assert _rel(p.vj, e1.get_j_e1(p.ao4, p.dm, p.a, p.mesh)) < 1e-10
    print('c_isdf = 3 on the device: |vk_e1 - exact| / max = %.3e' % _rel(p.vk, e1.get_k_e1(p.ao4, p.dm, p.a, p.mesh)))
    assert 'S8_get_j_e1' in df.timings and 'S8_get_k_e1' in df.timings


@gpu
def test_device_non_symmetric_stack_complex_chunks_and_composition(prod):
    p, df = prod, prod.df
    kn, jn = df.get_k_e1(p.dn), df.get_j_e1(p.dn)
    assert _rel(kn, e1.get_k_e1_isdf(p.aoT, p.dao, df.ip, p.theta, p.dn, p.a, p.mesh)) < 1e-8
    assert _rel(jn, e1.get_j_e1(p.ao4, p.dn, p.a, p.mesh)) < 1e-10
    sj, sk = df.get_jk_e1(np.array([p.dm, p.dn]))
    assert sj.shape == sk.shape == (3, 2, p.nao, p.nao)
    assert _rel(sk[:, 0], p.vk) < 1e-8 and _rel(sk[:, 1], kn) < 1e-8 and _rel(sj[:, 0], p.vj) < 1e-10 and _rel(sj[:, 1], jn) < 1e-10
    cj, ck = df.get_jk_e1(p.dm + 1j * p.dn)
    assert _rel(cj, p.vj + 1j * jn) < 1e-10 and _rel(ck, p.vk + 1j * kn) < 1e-8
    assert _rel(df.get_j_e1(p.dm), p.vj) < 1e-10 and _rel(df.get_k_e1(p.dm, exxdiv='ewald'), p.vk) < 1e-8
    df.e1_grid_chunk = 500                                        # 1728 = 3 * 500 + 228; 500 and 228 are no multiples of 16
    try:
        cj, ck = df.get_jk_e1(p.dm)
        df.e1_row_batch = 7
        cn = df.get_k_e1(p.dn)
    finally:
        df.e1_grid_chunk, df.e1_row_batch = 65536, None
    assert _rel(cj, p.vj) < 1e-10 and _rel(ck, p.vk) < 1e-8 and _rel(cn, kn) < 1e-8
    df.e1_fused = False
    try:
        assert _rel(df.get_k_e1(p.dm), p.vk) < 1e-8
    finally:
        df.e1_fused = True
    with pytest.raises(NotImplementedError, match='k-points'):
        df.get_jk_e1(p.dm, kpts=np.array([[0.1, 0.2, 0.3]]))
    with pytest.raises(NotImplementedError, match='exxdiv'):
        df.get_k_e1(p.dm, exxdiv='vcut_sph')
    with df.range_coulomb(0.3) as rdf:
        with pytest.raises(NotImplementedError, match='omega'):
            rdf.get_jk_e1(p.dm)


@gpu
def test_device_exact_limit():
    """select='global', c_isdf = 5 on gth-szv (tests/test_jk_e1.py): every AO pair is interpolated, the plain K of the build meets
    the exact exchange to 1e-9 of max, and get_k_e1 the exact restatement within 10 x that measured mismatch."""
    from test_jk_e1 import EXACT_C
    p = _Product('gth-szv', EXACT_C, select='global')
    df = p.df
    k_isdf = oisdf.get_k(df.backend.to_host(df.aoP), df.backend.to_host(df.W), p.dm)
    mismatch = _rel(k_isdf, fftdf.get_k(p.ao4[0], p.dm, p.a, p.mesh))
    err = _rel(p.vk, e1.get_k_e1(p.ao4, p.dm, p.a, p.mesh))
    print('device, c_isdf = %d global: P = %d, plain K mismatch %.3e, vk_e1 mismatch %.3e' % (EXACT_C, len(df.ip), mismatch, err))
    assert mismatch < 1e-9
    assert err <= 10 * mismatch


@gpu
def test_device_occ_pair_space():
    """pair_space='occ' on gth-dzvp, c_isdf = 4: the fit follows the density (_ensure_fit), and the same formula holds with that
    fit's Theta and V."""
    p = _Product('gth-dzvp', 4, pair_space='occ')
    df = p.df
    assert df._fit_dm is not None and df._psi is not None
    psi = oisdf.occupied_on_grid(p.aoT, p.c, p.occ)
    theta = oisdf.fit_theta_occ_chol(p.aoT, psi, df.ip, reg_rel=df.reg_used)
    assert _rel(p.vk, e1.get_k_e1_isdf(p.aoT, p.dao, df.ip, theta, p.dm, p.a, p.mesh)) < 1e-8
    assert _rel(p.vj, e1.get_j_e1(p.ao4, p.dm, p.a, p.mesh)) < 1e-10
