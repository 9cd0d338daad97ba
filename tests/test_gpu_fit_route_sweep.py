"""Sweep of the Cholesky fit route: the non-solve entry points of csrc/fit.hip (gathers, the Gram products of the three pair spaces,
the factorisations with their shift ladders) and the two-sided finishing solves through the left-looking drivers of csrc/trsm.hip.

The older tests (test_gpu_parity.py, test_gpu_kpts.py) run these calls on one physical cell or one Gaussian shape each, at the 1e-7
to 1e-10 that conditioning allows.  This module takes its cases from a restatement of the host-side chunking (fit_route_cases.py:
8192 columns per pass of the complex-mode second product, prod_chunk(P) columns of the occupied-pair product, 1024 rows per block of
tri_left / tri_right, 512-row panels and 64-row blocks of the substitution twin) and, where the library labels its launches
(rocblas_dtrsm, rocsolver_dpotrf, mul_rows_kernel, prod_combine_kernel, the own NN kernel), compares the launch count with it.

  gathers        isdf_gather_aoP and the gather of isdf_fit_prepare (P in {1, 255, 256, 257} x nao in {1, 9, 300}, ld = ng + 3, an
                 unsorted index list with repeats, 0 and ng - 1); isdf_gather_T (k in {1, 255, 256, 257}, ldL > m).
  Gram products  isdf_gram_sq (real; complex nh in {1, 5}; P in {1, 37, 256, 257}); isdf_pair_gram_rows real with both values of
                 gemm_nn_own on a shape the own kernel takes and one it refuses; complex P in {3, 37} over ng in {1, 8191, 8192,
                 8193, 16384, 16392}; isdf_fit_apply_cplx(forward_only) on the same ng with a unit bidiagonal factor;
                 isdf_gram_prod; isdf_pair_prod_rows over ng in {65535, 65536, 65537, 131077}; the two k-point forms with an odd
                 ldb and an output base that is not 16-byte aligned.  The row-chunk loops of isdf_gram_prod and isdf_gram_prod_cplx
                 take a second pass only from P of about 16384 and 9460 on - gigabytes of Gram matrix - and are out of scope.
  solves         isdf_factor_solve and isdf_factor_solve_half (P in {1, 63, 64, 65, 512, 513, 1024, 1025, 2049} x n in {1, 37,
                 257}), isdf_W_from_factor (kinds 0, 2, 2 then 0, and 1; P in {1, 65, 513, 1025}; ldm = P + 3),
                 isdf_fit_from_chol, isdf_bj_probe_vectors, isdf_fit_apply (both values of forward_only), isdf_fit_global, all on
                 factors the library did not make: integer lower triangular with diagonal in {1, 2, 4} and NaN above it.
  factorisations isdf_chol_inplace on A = L0 L0^T, with and without a caller's scratch; the five-rung ladders of isdf_fit_prepare,
                 isdf_fit_prepare_cplx and isdf_chol_inplace on an exactly singular integer Gram matrix; the ISDF_ERR_NUM exit;
                 isdf_shift_diag; isdf_block_chol with a singular, a healthy and an empty block.
  refusals       2 nh != nao, ldt / ldb < ng, ldm < P, kind 3, P = 0, blk_off[nblk] != P: an error, every output bit-unchanged.

Layouts, for every case: each operand with a leading dimension gets a larger one (odd where the entry point allows) with NaN in
the padding and around it; outputs sit in a sentinel-filled buffer with sentinel rows before and after; operands must be
bit-unchanged after the call, and so must everything around a result.

Two references.  Exact: integer operands stored as doubles, int64 numpy references (fit_route_cases.py; test_fit_route_cases.py
bounds every partial sum below 2^53), np.array_equal, no tolerance - all of the gathers, Gram products and refusals, and the solves
under option trsm_substitution, where every intermediate is an exact integer and the device must return X_true bit for bit.
Rounding: the default rocBLAS path (inverted diagonal blocks) on the same integer inputs, rocsolver_dpotrf, and one Gaussian case
per path against np.longdouble: the device's error relative to max|ref| over the error of numpy's float64 evaluation of the same
operation on the same inputs (one unit roundoff where numpy is exact) may not exceed ROUNDING_FACTOR.

Measured on an MI355X (profiles/r21_fit_route_sweep_ratios.log), device error / numpy error:

  path                                                            ratio
  rocblas_dtrsm, one block (Gaussian, P = 300, n = 37)            0.79 (L^-1), 2.59 (L^-T)
  rocblas_dtrsm, left-looking over three blocks (P = 2100, n = 8) 1.71 (L^-1), 1.96 (L^-T)
  rocsolver_dpotrf (Gaussian, P = 200)                            2.55
  rocsolver_dpotrf after the ladder (singular case, residual)     1.77 (request 0, reg_used 1e-14), 3.45 (request 1e-10)
  rocsolver_dpotrf inside isdf_block_chol (singular block)        1.84
  every default-path case on integer inputs                       0: the device returned X_true, W_true and Theta bit for bit in
                                                                  all 81 + 12 + 4 + 6 + 4 + 6 cases, while numpy's LU solve is off
                                                                  by 1e-13 to 4e-2 of max|X| on the one-sided systems and by more
                                                                  than max|W| on the two-sided ones of 513 rows and up: on these
                                                                  inputs the measure only catches gross errors (the K = jb - 1
                                                                  mutation below), the Gaussian cases carry the rounding check

The device errors are 2.2e-16 to 1.1e-15 of max|ref|, numpy's 7.5e-17 to 4.8e-16.  The largest ratio is 3.45; 4 x 3.45 = 13.8, so
ROUNDING_FACTOR = 16.  isdf_chol_inplace on A = L0 L0^T returned L0 with error 0 at every P, so that test asserts equality.  The
requests of 0 on the singular matrix stopped at the first rung, 1e-14, through all three entry points and isdf_block_chol.

Found and fixed: nothing.  All 62 GPU tests pass against the unchanged kernels (7 s for the module, the slowest test 0.6 s).

Mutations tried on a scratch copy (not committed), all in bounds, all seven noticed:
  - isdf_pair_gram_rows(nh > 0) reading d_ao instead of d_ao + c0: the pair_gram_rows cases of 8193, 16384 and 16392 columns fail
    from column 8192 on, at both P; the cases of 1, 8191 and 8192 columns pass, and have to.
  - isdf_fit_apply_cplx folding every chunk into d_theta instead of d_theta + c0: the same three ng fail for fit_apply_cplx.
  - isdf_pair_prod_rows reading d_psi instead of d_psi + c0: ng = 65537 and 131077 fail from column 65536 on.
  - stack_rot_kernel with [Im | Re]: both k-point products fail in 97 % of their entries.
  - isdf_chol_inplace without the restore between rungs: the request of 0 on the singular matrix ends in ISDF_ERR_NUM.
  - gather_T_kernel with s > t: isdf_gather_T, every kind 1 case and isdf_fit_from_chol fail.
  - tri_left's update of block jb one column short (K = jb - 1): the default-path solves of 1025 and 2049 rows, kind 2 at 1025
    rows and the Gaussian three-block case fail with ratios of 3e5 to 5e10.
"""
import ctypes
import functools
import numpy as np
import pytest

import fit_route_cases as fc
from test_gpu_gemm_sweep import _embed, _view, _profiled, _report, SENTINEL, PAD_ROWS, NN_LABEL, plan_nn
from test_gpu_fit_solve_sweep import _bits_equal, _first_diff, _offsets, SUBST

pytestmark = pytest.mark.gpu

DTRSM = 'rocblas_dtrsm[flop]'
DGEMM = 'rocblas_dgemm[flop]'
DPOTRF = 'rocsolver_dpotrf[flop]'
MUL_ROWS = 'mul_rows_kernel[byte]'
COMBINE = 'prod_combine_kernel[byte]'
WATCHED = (DTRSM, DPOTRF, MUL_ROWS, COMBINE, NN_LABEL[False], NN_LABEL[True], SUBST[False], SUBST[True])

# The smallest power of two at or above 4 x the largest device / numpy error ratio measured on an MI355X, capped at 64.
ROUNDING_FACTOR = 16.0


@pytest.fixture(scope='module')
def be():
    from pyscf_isdf_amd.backend import HipBackend
    b = HipBackend(0)
    b.prof_enable(True)
    yield b
    b.prof_enable(False)
    b.prof_reset()
    for key in ('gemm_nn_own', 'trsm_substitution'):
        b.set_option(key, 0)
    b.release_workspace()


def _odd(n):
    """A leading dimension above n, odd."""
    return n + 3 if n % 2 == 0 else n + 4


class _Buf:
    """The (nrow, ncol) window of a flat device buffer: ``off`` doubles, PAD_ROWS rows, the matrix in rows of ld, PAD_ROWS rows;
    NaN everywhere else for an operand, the sentinel for an output (out=True)."""

    def __init__(self, be, mat, ld=None, out=False, off=0):
        mat = np.asarray(mat, dtype=np.float64)
        self.be, (self.nrow, self.ncol), self.off = be, mat.shape, off
        self.ld = self.ncol + 3 if ld is None else ld
        self.host = _embed(mat, self.ld, off=off, fill=SENTINEL if out else np.nan)
        self.dev = be.to_device(self.host)
        self.view = _view(self.dev, self.nrow, self.ncol, self.ld, off=off)
        assert self.view.stride(1) == 1 and (self.nrow == 1 or self.view.stride(0) == self.ld)

    def _win(self, flat):
        return flat[self.off:].reshape(-1, self.ld)[PAD_ROWS:PAD_ROWS + self.nrow, :self.ncol]

    def unchanged(self):
        return _bits_equal(self.be.to_host(self.dev), self.host)

    def fetch(self):
        """(the window, whether everything around it is bit-unchanged)."""
        after = self.be.to_host(self.dev)
        win = self._win(after).copy()
        before = self.host.copy()
        self._win(after)[:] = 0.0
        self._win(before)[:] = 0.0
        return win, _bits_equal(after, before)


def _watched(prof):
    return {k: v['launches'] for k, v in prof.items() if k in WATCHED}


def _check_gemms(bad, prof, want):
    """The updates of the blocked walks: launches and summed flop of rocblas_dgemm against fc.solve_gemms (exact: every product's
    flop is an integer, the sum far below 2^53)."""
    ran = prof.get(DGEMM, dict(launches=0, work=0.0))
    ran = dict(launches=ran['launches'], work=ran['work'])
    if ran != want:
        bad.append('%s ran %s, the restatement says %s' % (DGEMM, ran, want))


def _check(bad, out, ref, operands, prof=None, want=None):
    """One exact case: the window equals ref, its surroundings and every operand are bit-unchanged, the watched labels ran as
    restated."""
    got, clean = out.fetch()
    if not clean:
        bad.append('sentinel or padding around the result overwritten')
    ref = np.asarray(ref, dtype=np.float64)
    if not np.array_equal(got, ref):
        bad.append(_first_diff(got, ref))
    for name, op in operands.items():
        if not op.unchanged():
            bad.append('operand %s changed' % name)
    if want is not None and _watched(prof) != want:
        bad.append('ran %s, the restatement says %s' % (_watched(prof), want))
    return got


def _finish(title, n, fails):
    _report('%s: %d cases' % (title, n), fails)
    assert not fails, fails


def _dev_ip(be, ip):
    import torch
    return be.to_device(np.asarray(ip, dtype=np.int64), dtype=torch.int64)


RATIOS = []


def _ratio(tag, got, host, ref):
    """Record and return the rounding measure of one case."""
    dev, hst = fc.rel_err(got, ref), fc.rel_err(host, ref)
    r = fc.rounding_ratio(dev, hst)
    RATIOS.append((tag, dev, hst, r))
    print('ratio %-58s device %.2e numpy %.2e ratio %.2f' % (tag, dev, hst, r))
    return r


# ---- A. gathers -------------------------------------------------------------------------------------------------------------
def test_gather_aoP_exact(be):
    """isdf_gather_aoP and the gather inside isdf_fit_prepare (requested shift 1e-6, so that the repeated points factorise at
    the first rung and the call returns exactly that shift): aoP == ao[:, ip]^T."""
    fails, ng = [], fc.GATHER_NG
    for P in fc.GATHER_P:
        for nao in fc.GATHER_NAO:
            rng = np.random.default_rng([P, nao])
            vals = fc.ints(rng, (nao, ng), 3)
            vals[vals == 0] = 1                                  # no all-zero point: its Gram matrix would be 0
            ao = _Buf(be, vals, ld=ng + 3)
            ip = fc.index_list(rng, P, ng)
            d_ip = _dev_ip(be, ip)
            ref = ao._win(ao.host)[:, ip].T
            for entry in ('gather_aoP', 'fit_prepare'):
                bad = []
                out = _Buf(be, np.full((P, nao), np.nan), ld=nao, out=True)
                if entry == 'gather_aoP':
                    be.gather_aoP(ao.view, d_ip, out.view)
                else:
                    chol = _Buf(be, np.full((P, P), np.nan), ld=P, out=True)
                    reg = be.fit_prepare(ao.view, d_ip, 1e-6, out.view, chol.view)
                    if reg != 1e-6:
                        bad.append('reg_used %r for a request of 1e-6' % reg)
                    if not chol.fetch()[1]:
                        bad.append('sentinel around the factor overwritten')
                _check(bad, out, ref, dict(ao=ao))
                if not np.array_equal(be.to_host(d_ip), ip):
                    bad.append('ip changed')
                if bad:
                    fails.append(('%s P=%d nao=%d' % (entry, P, nao), bad))
    _finish('gather aoP', 2 * len(fc.GATHER_P) * len(fc.GATHER_NAO), fails)


def test_gather_T_exact(be):
    """isdf_gather_T: the upper triangle is L[t, piv[s]], the strict lower triangle +0.0, bit for bit."""
    fails = []
    for k in fc.GATHER_T_K:
        rng = np.random.default_rng(k)
        m = k + 5
        L = _Buf(be, fc.ints(rng, (k, m), 3), ld=m + 3)
        piv = rng.permutation(m)[:k].astype(np.int64)
        d_piv = _dev_ip(be, piv)
        out = _Buf(be, np.full((k, k), np.nan), ld=k, out=True)
        be.gather_T(L.view, k, d_piv, out.view)
        bad = []
        ref = np.triu(L._win(L.host)[:, piv])
        got = _check(bad, out, ref, dict(L=L))
        if not _bits_equal(got, ref):
            bad.append('a zero of the lower triangle is not +0.0')
        if bad:
            fails.append(('k=%d' % k, bad))
    _finish('gather T', len(fc.GATHER_T_K), fails)


# ---- B. Gram products -------------------------------------------------------------------------------------------------------
def test_gram_sq_exact(be):
    """isdf_gram_sq, real and complex mode: (aoP aoP^T)^2 (+ (rot aoP^T)^2 with rot = [Im | -Re]) in int64."""
    fails = []
    for P in fc.GRAM_P:
        for nh in (0,) + fc.GRAM_NH:
            aoP = fc.gram_sq_operand(P, nh)
            d_aoP = _Buf(be, aoP, ld=aoP.shape[1])
            out = _Buf(be, np.full((P, P), np.nan), ld=P, out=True)
            prof = _profiled(be, lambda: be.gram_sq(d_aoP.view, out.view, nh=nh))
            bad = []
            _check(bad, out, fc.gram_sq_ref(aoP, nh), dict(aoP=d_aoP), prof, {})
            if bad:
                fails.append(('P=%d nh=%d' % (P, nh), bad))
    _finish('gram_sq', len(fc.GRAM_P) * 3, fails)


def test_pair_gram_rows_real_exact(be):
    """isdf_pair_gram_rows in real mode with both values of option gemm_nn_own, on a shape the own NN kernel takes (P = 256,
    nao = 32, even ld) and one it refuses (P = 37, nao = 9): the label against plan_nn, the same exact (aoP ao)^2."""
    fails, seen, ng = [], set(), fc.ROWS_REAL_NG
    for P, nao in fc.ROWS_REAL:
        for own in (0, 1):
            rng = np.random.default_rng([P, nao, own])
            aoP, ao = fc.ints(rng, (P, nao), 3), fc.ints(rng, (nao, ng), 3)
            d_aoP, d_ao = _Buf(be, aoP, ld=nao), _Buf(be, ao, ld=ng + 4)
            out = _Buf(be, np.full((P, ng), np.nan), ld=_odd(ng), out=True)
            plan = plan_nn(P, ng, nao, True, own=bool(own), lda=nao, ldb=d_ao.ld)
            want = {NN_LABEL[True]: 1} if plan.kern == 'nn' else {}
            be.set_option('gemm_nn_own', own)
            try:
                prof = _profiled(be, lambda: be.pair_gram_rows(d_aoP.view, d_ao.view, ng, out.view))
            finally:
                be.set_option('gemm_nn_own', 0)
            bad = []
            _check(bad, out, fc.pair_rows_ref(aoP, ao), dict(aoP=d_aoP, ao=d_ao), prof, want)
            seen.add((own, plan.kern))
            if bad:
                fails.append(('P=%d nao=%d own=%d' % (P, nao, own), bad))
    _finish('pair_gram_rows, real mode', 4, fails)
    assert seen == {(0, 'rocblas'), (1, 'rocblas'), (1, 'nn')}, seen


@pytest.mark.parametrize('P', fc.CPLX_P)
def test_complex_rows_across_the_column_chunk_exact(be, P):
    """isdf_pair_gram_rows(nh = 5) and isdf_fit_apply_cplx(forward_only) over ng on, below and above one and two chunks of 8192
    columns: (aoP ao)^2 + (rot ao)^2, and Y = L^-1 of it for a unit bidiagonal integer factor under option trsm_substitution."""
    fails, nh = [], fc.CPLX_NH
    for ng in fc.CPLX_NG:
        rng = np.random.default_rng([P, ng])
        aoP, ao = fc.complex_operands(rng, P, nh, ng)
        L, Linv = fc.bidiagonal_factor(rng, P)
        B = fc.pair_rows_ref(aoP, ao, nh)
        d_aoP, d_ao = _Buf(be, aoP, ld=2 * nh), _Buf(be, ao, ld=_odd(ng))
        d_L = _Buf(be, fc.nan_upper(L), ld=P)
        for entry in ('pair_gram_rows', 'fit_apply_cplx'):
            out = _Buf(be, np.full((P, ng), np.nan), ld=_odd(ng) + 2, out=True)
            bad = []
            if entry == 'pair_gram_rows':
                prof = _profiled(be, lambda: be.pair_gram_rows(d_aoP.view, d_ao.view, ng, out.view, nh=nh))
                _check(bad, out, B, dict(aoP=d_aoP, ao=d_ao), prof, {})
            else:
                be.set_option('trsm_substitution', 1)
                try:
                    prof = _profiled(be, lambda: be.fit_apply_cplx(d_L.view, d_aoP.view, nh, d_ao.view, ng, out.view, forward_only=True))
                finally:
                    be.set_option('trsm_substitution', 0)
                _check(bad, out, Linv.dot(B), dict(aoP=d_aoP, ao=d_ao, chol=d_L), prof, {SUBST[False]: fc.cdiv(P, fc.SUBST_BLOCK)})
            if bad:
                fails.append(('%s ng=%d (%d chunks)' % (entry, ng, len(fc.chunks(ng, fc.CPLX_CHUNK))), bad))
    _finish('complex-mode rows, P = %d' % P, 2 * len(fc.CPLX_NG), fails)


def test_gram_prod_exact(be):
    """isdf_gram_prod: (aoP aoP^T) o (psiP psiP^T)."""
    fails = []
    for P in fc.PROD_P:
        for nocc in fc.PROD_NOCC:
            rng = np.random.default_rng([P, nocc])
            aoP, psiP = fc.ints(rng, (P, fc.PROD_NAO), 3), fc.ints(rng, (P, nocc), 3)
            d_aoP, d_psiP = _Buf(be, aoP, ld=fc.PROD_NAO), _Buf(be, psiP, ld=nocc)
            out = _Buf(be, np.full((P, P), np.nan), ld=P, out=True)
            be.gram_prod(d_aoP.view, d_psiP.view, out.view)
            bad = []
            _check(bad, out, fc.gram_prod_ref(aoP, psiP), dict(aoP=d_aoP, psiP=d_psiP))
            if bad:
                fails.append(('P=%d nocc=%d' % (P, nocc), bad))
    _finish('gram_prod', len(fc.PROD_P) * len(fc.PROD_NOCC), fails)


@pytest.mark.parametrize('P', fc.PROD_ROWS_P)
def test_pair_prod_rows_across_the_column_chunk_exact(be, P):
    """isdf_pair_prod_rows over ng below, on and above one chunk of prod_chunk(P) = 65536 columns and above two, ld, ldpsi and
    ldb above ng: (aoP ao) o (psiP psi), mul_rows_kernel launched once per chunk."""
    fails, nao = [], fc.PROD_NAO
    ch = fc.prod_chunk(P)
    for ng in fc.PROD_ROWS_NG:
        for nocc in fc.PROD_NOCC:
            rng = np.random.default_rng([P, ng, nocc])
            aoP, psiP = fc.ints(rng, (P, nao), 3), fc.ints(rng, (P, nocc), 3)
            ao, psi = fc.ints(rng, (nao, ng), 3), fc.ints(rng, (nocc, ng), 3)
            d_aoP, d_psiP = _Buf(be, aoP, ld=nao), _Buf(be, psiP, ld=nocc)
            d_ao, d_psi = _Buf(be, ao, ld=_odd(ng)), _Buf(be, psi, ld=_odd(ng) + 2)
            out = _Buf(be, np.full((P, ng), np.nan), ld=_odd(ng) + 4, out=True)
            prof = _profiled(be, lambda: be.pair_prod_rows(d_aoP.view, d_psiP.view, d_ao.view, d_psi.view, ng, out.view))
            bad = []
            _check(bad, out, fc.pair_prod_rows_ref(aoP, psiP, ao, psi), dict(aoP=d_aoP, psiP=d_psiP, ao=d_ao, psi=d_psi), prof,
                   {MUL_ROWS: len(fc.chunks(ng, ch))})
            if bad:
                fails.append(('ng=%d nocc=%d' % (ng, nocc), bad))
    _finish('pair_prod_rows, P = %d' % P, len(fc.PROD_ROWS_NG) * len(fc.PROD_NOCC), fails)


def test_kpoint_pair_products_exact_on_the_8_byte_path(be):
    """isdf_gram_prod_cplx (P = 37: odd rows of A) and isdf_pair_prod_rows_cplx (odd ldb), both with an output base one double
    past a 16-byte boundary, on integers: prod_combine_kernel's 8-byte loads and stores."""
    P, nh, npsi_h, ng = 37, fc.CPLX_NH, 2, 701
    rng = np.random.default_rng(12)
    aoP, ao = fc.complex_operands(rng, P, nh, ng)
    psiP, psi = fc.complex_operands(rng, P, npsi_h, ng)
    d_aoP, d_psiP = _Buf(be, aoP, ld=2 * nh), _Buf(be, psiP, ld=2 * npsi_h)
    d_ao, d_psi = _Buf(be, ao, ld=_odd(ng)), _Buf(be, psi, ld=_odd(ng) + 2)
    fails = []
    out = _Buf(be, np.full((P, P), np.nan), ld=P, out=True, off=1)
    assert out.view.data_ptr() % 16 == 8
    prof = _profiled(be, lambda: be.gram_prod_cplx(d_aoP.view, nh, d_psiP.view, npsi_h, out.view))
    bad = []
    _check(bad, out, fc.gram_prod_cplx_ref(aoP, nh, psiP, npsi_h), dict(aoP=d_aoP, psiP=d_psiP), prof, {COMBINE: 1})
    if bad:
        fails.append(('gram_prod_cplx', bad))
    out = _Buf(be, np.full((P, ng), np.nan), ld=_odd(ng) + 4, out=True, off=1)
    assert out.view.data_ptr() % 16 == 8 and out.ld % 2 == 1
    prof = _profiled(be, lambda: be.pair_prod_rows_cplx(d_aoP.view, nh, d_psiP.view, npsi_h, d_ao.view, d_psi.view, ng, out.view))
    bad = []
    _check(bad, out, fc.pair_prod_rows_cplx_ref(aoP, nh, psiP, npsi_h, ao, psi),
           dict(aoP=d_aoP, psiP=d_psiP, ao=d_ao, psi=d_psi), prof, {COMBINE: 1})
    if bad:
        fails.append(('pair_prod_rows_cplx', bad))
    _finish('k-point pair products', 2, fails)


# ---- C. solves with a caller's factor ---------------------------------------------------------------------------------------
N_MAX = max(fc.SOLVE_N)


@functools.lru_cache(maxsize=2)
def _solve_data(P):
    """Per P: the factor, X_true (P, 257) (a case of n columns takes the first n), the right-hand sides of the three entry points in
    exact integers, and numpy's float64 solutions of them."""
    L, _ = fc.factor_pair(P, 0)
    Xt = fc.ints(np.random.default_rng([P, 41]), (P, N_MAX), 4).astype(np.float64)
    Xt[0, 0] = 3.0                                           # max|X_true| > 0 for every n, P = 1 included
    rhs = {'half0': fc.exact_dot(L, Xt), 'half1': fc.exact_dot(L.T, Xt)}
    rhs['solve'] = fc.exact_dot(L, rhs['half1'])
    host = {'half0': np.linalg.solve(L, rhs['half0']), 'half1': np.linalg.solve(L.T, rhs['half1'])}
    host['solve'] = np.linalg.solve(L.T, np.linalg.solve(L, rhs['solve']))
    return L, Xt, rhs, host


def _launch_solve(be, entry, d_L, X):
    if entry == 'solve':
        be.factor_solve(d_L, X)
    else:
        be.factor_solve_half(d_L, entry == 'half1', X)


def _subst_launches(P, passes):
    return fc.cdiv(P, fc.SUBST_BLOCK) * passes


@pytest.mark.parametrize('subst', [1, 0])
@pytest.mark.parametrize('P', fc.SOLVE_P)
def test_factor_solves(be, P, subst):
    """isdf_factor_solve and isdf_factor_solve_half (backward 0 and 1) across the 64-row blocks, the 512-row panels and the
    1024-row blocks of the left-looking form, n in {1, 37, 257}, ldx = n + 3.  Option trsm_substitution: X_true bit for bit.
    Default: one rocblas_dtrsm per block of 1024 rows and pass, the rounding measure against X_true."""
    L, Xt, rhs, host = _solve_data(P)
    d_L = _Buf(be, fc.nan_upper(L), ld=P)
    fails = []
    be.set_option('trsm_substitution', subst)
    try:
        for n in fc.SOLVE_N:
            for entry in ('solve', 'half0', 'half1'):
                X = _Buf(be, rhs[entry][:, :n], ld=n + 3, out=True)
                prof = _profiled(be, lambda: _launch_solve(be, entry, d_L.view, X.view))
                passes = {'solve': (False, True), 'half0': (False,), 'half1': (True,)}[entry]
                bad = []
                _check_gemms(bad, prof, fc.solve_gemms(P, n, [not trans for trans in passes], subst))    # L^-1 X walks upwards
                if subst:
                    want = {SUBST[t]: _subst_launches(P, 1) for t in passes}
                    _check(bad, X, Xt[:, :n], dict(fac=d_L), prof, want)
                else:
                    got, clean = X.fetch()
                    if not clean:
                        bad.append('sentinel or padding around X overwritten')
                    if not d_L.unchanged():
                        bad.append('the factor changed')
                    want = {DTRSM: fc.trsm_calls(P) * len(passes)}
                    if _watched(prof) != want:
                        bad.append('ran %s, the restatement says %s' % (_watched(prof), want))
                    r = _ratio('%s P=%d n=%d (integers)' % (entry, P, n), got, host[entry][:, :n], Xt[:, :n])
                    if not (np.isfinite(got).all() and r <= ROUNDING_FACTOR):
                        bad.append('rounding ratio %.2f above %g' % (r, ROUNDING_FACTOR))
                if bad:
                    fails.append(('%s n=%d' % (entry, n), bad))
    finally:
        be.set_option('trsm_substitution', 0)
    _finish('factor solves, P = %d, substitution = %d' % (P, subst), 9, fails)


def _sym_ints(rng, P):
    W = np.triu(fc.ints(rng, (P, P), 4))
    return (W + np.triu(W, 1).T).astype(np.float64)


@pytest.mark.parametrize('subst', [1, 0])
@pytest.mark.parametrize('P', fc.W_P)
def test_W_from_factor_kinds_0_and_2(be, P, subst):
    """isdf_W_from_factor on M = op(L) W_true op(L)^T in exact integers, ldm = P + 3 with the sentinel in the padding: kind 0
    (L^-T M L^-1), kind 2 (L^-1 M L^-T) and kind 2 followed by kind 0 (A^-1 M A^-1)."""
    L, _ = fc.factor_pair(P, 0)
    Wt = _sym_ints(np.random.default_rng([P, 43]), P)
    d_L = _Buf(be, fc.nan_upper(L), ld=P)
    M0 = fc.exact_dot(fc.exact_dot(L.T, Wt), L)
    M2 = fc.exact_dot(fc.exact_dot(L, Wt), L.T)
    M20 = fc.exact_dot(fc.exact_dot(L, M0), L.T)
    solveL = lambda X: np.linalg.solve(L, X)                                   # L^-1 X
    solveLt = lambda X: np.linalg.solve(L.T, X)                                # L^-T X
    two_sided = {0: lambda M: solveLt(solveLt(M).T).T, 2: lambda M: solveL(solveL(M).T).T}
    fails = []
    be.set_option('trsm_substitution', subst)
    try:
        for tag, M, kinds in (('kind 0', M0, (0,)), ('kind 2', M2, (2,)), ('kind 2 then 0', M20, (2, 0))):
            X = _Buf(be, M, ld=P + 3, out=True)
            prof = _profiled(be, lambda: [be.W_from_factor(d_L.view, k, X.view) for k in kinds])
            bad = []
            # two walks per kind, both upwards for kind 2 (L^-1 M, then M L^-T) and both downwards for kind 0
            _check_gemms(bad, prof, fc.solve_gemms(P, P, [k == 2 for k in kinds for _ in range(2)], subst))
            if subst:
                # a right-sided solve is the left-sided one of the other op on X^T: kind 0 runs L^-T twice, kind 2 L^-1 twice
                _check(bad, X, Wt, dict(fac=d_L), prof, {SUBST[k == 0]: _subst_launches(P, 2) for k in kinds})
            else:
                got, clean = X.fetch()
                if not clean:
                    bad.append('sentinel in the ldm padding or around M overwritten')
                if not d_L.unchanged():
                    bad.append('the factor changed')
                want = {DTRSM: fc.trsm_calls(P, two_sided=True) * len(kinds)}
                if _watched(prof) != want:
                    bad.append('ran %s, the restatement says %s' % (_watched(prof), want))
                hst = M
                for k in kinds:
                    hst = two_sided[k](hst)
                r = _ratio('W_from_factor %s P=%d (integers)' % (tag, P), got, hst, Wt)
                if not (np.isfinite(got).all() and r <= ROUNDING_FACTOR):
                    bad.append('rounding ratio %.2f above %g' % (r, ROUNDING_FACTOR))
            if bad:
                fails.append((tag, bad))
    finally:
        be.set_option('trsm_substitution', 0)
    _finish('W_from_factor, P = %d, substitution = %d' % (P, subst), 3, fails)


@pytest.mark.parametrize('P', fc.W_P)
def test_W_from_factor_kind_1(be, P):
    """Kind 1 with T from isdf_gather_T of integer rows (T = L^T of an integer factor at permuted pivot columns, NaN where the
    gather must write zeros): M = T W_true T^T, ldm = P + 3.  rocBLAS only: two dtrsm in one label, the rounding measure."""
    L, _ = fc.factor_pair(P, 0)
    rng = np.random.default_rng([P, 47])
    Wt = _sym_ints(rng, P)
    m = P + 4
    piv = rng.permutation(m)[:P].astype(np.int64)
    rows = fc.ints(rng, (P, m), 3).astype(np.float64)
    rows[:, piv] = fc.nan_upper(L).T                       # NaN below the diagonal of T
    d_rows = _Buf(be, rows, ld=m + 3)
    d_T = _Buf(be, np.full((P, P), np.nan), ld=P, out=True)
    be.gather_T(d_rows.view, P, _dev_ip(be, piv), d_T.view)
    T = L.T
    bad = []
    _check(bad, d_T, T, dict(rows=d_rows))
    X = _Buf(be, fc.exact_dot(fc.exact_dot(T, Wt), T.T), ld=P + 3, out=True)
    keep = be.to_host(d_T.dev)
    prof = _profiled(be, lambda: be.W_from_factor(d_T.view, 1, X.view))
    got, clean = X.fetch()
    if not clean:
        bad.append('sentinel in the ldm padding or around M overwritten')
    if not _bits_equal(be.to_host(d_T.dev), keep):
        bad.append('T changed')
    if _watched(prof) != {DTRSM: 2}:
        bad.append('ran %s, the restatement says %s' % (_watched(prof), {DTRSM: 2}))
    M = X._win(X.host)
    hst = np.linalg.solve(T, np.linalg.solve(T, M).T).T
    r = _ratio('W_from_factor kind 1 P=%d (integers)' % P, got, hst, Wt)
    assert not bad, bad
    assert np.isfinite(got).all() and r <= ROUNDING_FACTOR, r


def test_fit_from_chol_identity_at_the_pivots(be):
    """isdf_fit_from_chol on integer rows whose pivot columns form a unit upper bidiagonal T, ldL = m + 3: the pivot columns come
    back as the identity exactly, the whole of Theta = T^-1 L within the rounding measure."""
    fails = []
    for k, m in fc.FROM_CHOL:
        c = fc.from_chol_case(k, m)
        X = _Buf(be, c['L'], ld=m + 3, out=True)
        d_piv = _dev_ip(be, c['piv'])
        be.fit_from_chol(X.view, k, m, d_piv)
        got, clean = X.fetch()
        bad = [] if clean else ['sentinel or padding around L overwritten']
        if not np.array_equal(be.to_host(d_piv), c['piv']):
            bad.append('piv changed')
        if not np.array_equal(got[:, c['piv']], np.eye(k)):
            bad.append('the pivot columns are not the identity')
        hst = np.linalg.solve(c['T'].astype(np.float64), c['L'].astype(np.float64))
        r = _ratio('fit_from_chol k=%d m=%d (integers)' % (k, m), got, hst, c['Theta'])
        if not (np.isfinite(got).all() and r <= ROUNDING_FACTOR):
            bad.append('rounding ratio %.2f above %g' % (r, ROUNDING_FACTOR))
        if bad:
            fails.append(('k=%d m=%d' % (k, m), bad))
    _finish('fit_from_chol', len(fc.FROM_CHOL), fails)


@pytest.mark.parametrize('subst', [1, 0])
def test_bj_probe_vectors(be, subst):
    """isdf_bj_probe_vectors: rows t^T <- t^T D^-T L^-T L^-1 with D block diagonal (NaN outside the blocks and above every
    diagonal), on T = E_true L L^T D^T in exact integers.  P = 37 in blocks of 10, 0, 16, 11 rows and P = 600 in 130 + 470."""
    fails = []
    be.set_option('trsm_substitution', subst)
    try:
        for n, sizes in fc.PROBE_CASES:
            off = _offsets(sizes)
            P = int(off[-1])
            L, _ = fc.factor_pair(P, 0)
            D = np.full((P, P), np.nan)
            Dz = np.zeros((P, P))
            for b, s in enumerate(sizes):
                o = int(off[b])
                D[o:o + s, o:o + s] = fc.nan_upper(fc.factor_pair(s, 2)[0]) if s else 0.0
                Dz[o:o + s, o:o + s] = fc.factor_pair(s, 2)[0] if s else 0.0
            Et = fc.ints(np.random.default_rng([n, P]), (n, P), 4).astype(np.float64)
            T0 = fc.exact_dot(fc.exact_dot(fc.exact_dot(Et, L), L.T), Dz.T)
            d_L, d_D = _Buf(be, fc.nan_upper(L), ld=P), _Buf(be, D, ld=P)
            X = _Buf(be, T0, ld=P, out=True)
            be.bj_probe_vectors(X.view, d_L.view, d_D.view, off)
            bad = []
            if subst:
                _check(bad, X, Et, dict(fac=d_L, D=d_D))
            else:
                got, clean = X.fetch()
                if not (clean and d_L.unchanged() and d_D.unchanged()):
                    bad.append('an operand or the surroundings of T changed')
                hst = np.linalg.solve(L.T, np.linalg.solve(L, np.linalg.solve(Dz, T0.T))).T
                r = _ratio('bj_probe_vectors n=%d P=%d (integers)' % (n, P), got, hst, Et)
                if not (np.isfinite(got).all() and r <= ROUNDING_FACTOR):
                    bad.append('rounding ratio %.2f above %g' % (r, ROUNDING_FACTOR))
            if bad:
                fails.append(('n=%d P=%d' % (n, P), bad))
    finally:
        be.set_option('trsm_substitution', 0)
    _finish('bj_probe_vectors, substitution = %d' % subst, len(fc.PROBE_CASES), fails)


@pytest.mark.parametrize('subst', [1, 0])
def test_fit_apply_real_mode(be, subst):
    """isdf_fit_apply with integer aoP, ao and a unit bidiagonal integer factor, both values of forward_only: Y = L^-1 (aoP ao)^2
    and Theta = L^-T Y are integers; bit for bit under option trsm_substitution, the rounding measure on the default path."""
    fails = []
    be.set_option('trsm_substitution', subst)
    try:
        for ng in fc.APPLY_NG:
            c = fc.apply_case(ng)
            P = fc.APPLY_P
            d_aoP, d_ao = _Buf(be, c['aoP'], ld=fc.APPLY_NAO), _Buf(be, c['ao'], ld=_odd(ng))
            d_L = _Buf(be, fc.nan_upper(c['L']), ld=P)
            Lf, Bf = c['L'].astype(np.float64), c['B'].astype(np.float64)
            for fwd in (True, False):
                ref = c['Y'] if fwd else c['Theta']
                out = _Buf(be, np.full((P, ng), np.nan), ld=_odd(ng) + 2, out=True)
                prof = _profiled(be, lambda: be.fit_apply(d_L.view, d_aoP.view, d_ao.view, ng, out.view, forward_only=fwd))
                bad = []
                ops = dict(aoP=d_aoP, ao=d_ao, chol=d_L)
                if subst:
                    _check(bad, out, ref, ops, prof, {SUBST[False]: 1} if fwd else {SUBST[False]: 1, SUBST[True]: 1})
                else:
                    got, clean = out.fetch()
                    if not clean or not all(op.unchanged() for op in ops.values()):
                        bad.append('an operand or the surroundings of theta changed')
                    if _watched(prof) != {DTRSM: 1 if fwd else 2}:
                        bad.append('ran %s, the restatement says %d dtrsm' % (_watched(prof), 1 if fwd else 2))
                    hst = np.linalg.solve(Lf, Bf)
                    hst = hst if fwd else np.linalg.solve(Lf.T, hst)
                    r = _ratio('fit_apply ng=%d forward_only=%d (integers)' % (ng, fwd), got, hst, ref)
                    if not (np.isfinite(got).all() and r <= ROUNDING_FACTOR):
                        bad.append('rounding ratio %.2f above %g' % (r, ROUNDING_FACTOR))
                if bad:
                    fails.append(('ng=%d forward_only=%d' % (ng, fwd), bad))
    finally:
        be.set_option('trsm_substitution', 0)
    _finish('fit_apply, substitution = %d' % subst, 2 * len(fc.APPLY_NG), fails)


def test_fit_global_is_prepare_then_apply(be):
    """isdf_fit_global against isdf_fit_prepare followed by isdf_fit_apply on the same integer inputs: theta, aoP and the shift
    bit for bit."""
    c = fc.singular_case(seed=21)
    ao, ip = c['ao'].copy(), c['ip']
    ao[:, ip[1]] = fc.ints(np.random.default_rng(5), (fc.SING_NAO,), 2)           # no duplicated point: a healthy matrix
    P, nao, ng = fc.SING_P, fc.SING_NAO, fc.SING_NG
    d_ao, d_ip = _Buf(be, ao, ld=_odd(ng)), _dev_ip(be, ip)
    th1 = _Buf(be, np.full((P, ng), np.nan), ld=_odd(ng) + 2, out=True)
    aoP1 = _Buf(be, np.full((P, nao), np.nan), ld=nao, out=True)
    reg1 = be.fit_global(d_ao.view, ng, d_ip, 1e-10, th1.view, aoP1.view)
    th2 = _Buf(be, np.full((P, ng), np.nan), ld=_odd(ng) + 2, out=True)
    aoP2 = _Buf(be, np.full((P, nao), np.nan), ld=nao, out=True)
    chol = _Buf(be, np.full((P, P), np.nan), ld=P, out=True)
    reg2 = be.fit_prepare(d_ao.view, d_ip, 1e-10, aoP2.view, chol.view)
    be.fit_apply(chol.view, aoP2.view, d_ao.view, ng, th2.view)
    assert reg1 == reg2 == 1e-10
    (t1, c1), (t2, c2), (a1, c3), (a2, c4) = th1.fetch(), th2.fetch(), aoP1.fetch(), aoP2.fetch()
    assert c1 and c2 and c3 and c4 and d_ao.unchanged()
    assert np.isfinite(t1).all() and _bits_equal(t1, t2) and _bits_equal(a1, a2) and np.array_equal(a1, ao[:, ip].T)


# ---- D. factorisations and the ladders --------------------------------------------------------------------------------------
def _chol_residual(Lrm, Ashift, md):
    """max |L L^T - A| / maxdiag in np.longdouble."""
    L = np.tril(Lrm).astype(np.longdouble)
    return float(abs(L.dot(L.T) - Ashift.astype(np.longdouble)).max() / md)


def _chol_ratio(tag, got, Ashift, md):
    dev, hst = _chol_residual(got, Ashift, md), _chol_residual(np.linalg.cholesky(Ashift), Ashift, md)
    r = fc.rounding_ratio(dev, hst)
    RATIOS.append((tag, dev, hst, r))
    print('ratio %-58s device %.2e numpy %.2e ratio %.2f' % (tag, dev, hst, r))
    return r


@pytest.mark.parametrize('P', fc.CHOL_P)
def test_chol_inplace_healthy(be, P):
    """isdf_chol_inplace (requested shift 0) on A = L0 L0^T with an integer L0: returns 0.0 after one rocsolver_dpotrf, the strict
    upper triangle keeps A, a caller's scratch changes no bit.  The lower triangle is L0: the device's error measured on an MI355X
    is 0 at every P (every pivot is an exact square, every quotient an exact integer), so this asserts equality."""
    A, L0 = fc.healthy_matrix(P)
    results = []
    for scratch in (False, True):
        X = _Buf(be, A, ld=P, out=True)
        d_s = _Buf(be, np.full((P, P), np.nan), ld=P, out=True) if scratch else None
        box = []
        prof = _profiled(be, lambda: box.append(be.chol_inplace(X.view, 0.0, scratch=d_s.view if scratch else None)))
        got, clean = X.fetch()
        assert box == [0.0] and clean and _watched(prof) == {DPOTRF: 1}, (box, clean, _watched(prof))
        assert d_s is None or d_s.fetch()[1]
        assert np.array_equal(np.triu(got, 1), np.triu(A, 1))
        results.append(got)
    assert _bits_equal(results[0], results[1])
    got = np.tril(results[0])
    hst = np.linalg.cholesky(A)
    _ratio('chol_inplace healthy P=%d (integers)' % P, got, hst, L0)
    assert np.array_equal(got, L0), _first_diff(got, L0)


def _ladder_checks(tag, bad, request, reg, prof, got, A, md):
    """The shift a ladder returned, its dpotrf count and the factor it left, for a request of 0 or 1e-10 on the singular case."""
    if request == 0.0:
        if reg not in (1e-14, 1e-12):
            bad.append('reg_used %r, expected the first rung 1e-14 (1e-12 allowed)' % reg)
        want = {DPOTRF: {1e-14: 2, 1e-12: 3}.get(reg, -1)}
    else:
        if reg != request:
            bad.append('reg_used %r for a request of %r' % (reg, request))
        want = {DPOTRF: 1}
    if _watched(prof) != want:
        bad.append('ran %s, the restatement says %s' % (_watched(prof), want))
    if not np.isfinite(np.tril(got)).all():
        bad.append('the factor is not finite')
        return
    # against the ORIGINAL matrix with one shift: a rung that did not start from the unshifted matrix shows here
    r = _chol_ratio('%s request %g' % (tag, request), got, fc.shifted(A, reg, md), md)
    if not r <= ROUNDING_FACTOR:
        bad.append('residual ratio %.2f above %g' % (r, ROUNDING_FACTOR))


@pytest.mark.parametrize('request_', [0.0, 1e-10])
def test_shift_ladders_on_a_singular_matrix(be, request_):
    """An integer aoP whose rows 0 and 1 coincide makes the second pivot of A = (aoP aoP^T)^2 exactly 0.  isdf_fit_prepare,
    isdf_fit_prepare_cplx (the same rows as [Re | Im] with Im = 0) and isdf_chol_inplace (with and without a caller's scratch):
    a request of 0 climbs to 1e-14 (1e-12 allowed), a request of 1e-10 is kept; L L^T = A + reg_used maxdiag I against the
    unshifted A; d_aoP equals the gathered rows."""
    c = fc.singular_case()
    A, md, P, nao, ng = c['A'].astype(np.float64), c['maxdiag'], fc.SING_P, fc.SING_NAO, fc.SING_NG
    d_ip = _dev_ip(be, c['ip'])
    fails = []
    for tag in ('fit_prepare', 'fit_prepare_cplx'):
        cplx = tag.endswith('cplx')
        ao = np.concatenate([c['ao'], np.zeros_like(c['ao'])]) if cplx else c['ao']
        d_ao = _Buf(be, ao, ld=_odd(ng))
        aoP = _Buf(be, np.full((P, ao.shape[0]), np.nan), ld=ao.shape[0], out=True)
        chol = _Buf(be, np.full((P, P), np.nan), ld=P, out=True)
        box = []
        if cplx:
            prof = _profiled(be, lambda: box.append(be.fit_prepare_cplx(d_ao.view, nao, d_ip, request_, aoP.view, chol.view)))
        else:
            prof = _profiled(be, lambda: box.append(be.fit_prepare(d_ao.view, d_ip, request_, aoP.view, chol.view)))
        bad = []
        _check(bad, aoP, ao[:, c['ip']].T, dict(ao=d_ao))
        got, clean = chol.fetch()
        if not clean:
            bad.append('sentinel around the factor overwritten')
        _ladder_checks(tag, bad, request_, box[0], prof, got, A, md)
        if bad:
            fails.append((tag, bad))
    for scratch in (False, True):
        tag = 'chol_inplace%s' % (' with scratch' if scratch else '')
        X = _Buf(be, A, ld=P, out=True)
        d_s = _Buf(be, np.full((P, P), np.nan), ld=P, out=True) if scratch else None
        box = []
        prof = _profiled(be, lambda: box.append(be.chol_inplace(X.view, request_, scratch=d_s.view if scratch else None)))
        got, clean = X.fetch()
        bad = [] if clean else ['sentinel around A overwritten']
        if scratch and not d_s.fetch()[1]:
            bad.append('sentinel around the scratch overwritten')
        _ladder_checks(tag, bad, request_, box[0], prof, got, A, md)
        if bad:
            fails.append((tag, bad))
    _finish('shift ladders, request %g' % request_, 4, fails)


def test_chol_inplace_failure_exit_and_recovery(be):
    """diag(1, -1, 1, 1, 1) is indefinite at every rung: the backend raises, isdf_last_error names the last shift tried (1e-8),
    and the next call on the same handle, a healthy factorisation, gives the bits it gave before the failure."""
    from pyscf_isdf_amd.lib import IsdfError
    A, _ = fc.healthy_matrix(65)

    def healthy():
        X = _Buf(be, A, ld=65, out=True)
        assert be.chol_inplace(X.view, 0.0) == 0.0
        got, clean = X.fetch()
        assert clean
        return got
    before = healthy()
    X = _Buf(be, np.diag([1.0, -1.0, 1.0, 1.0, 1.0]), ld=5, out=True)
    be.prof_reset()
    with pytest.raises(IsdfError) as err:
        be.chol_inplace(X.view, 0.0)
    assert '1e-08' in str(err.value), str(err.value)
    be.synchronize()
    assert _watched(be.prof_results()) == {DPOTRF: 5}, _watched(be.prof_results())
    assert X.fetch()[1]
    assert _bits_equal(healthy(), before)


def test_shift_diag_exact(be):
    """isdf_shift_diag on an integer matrix: a shift of 0 changes no bit; 2^-10 with max diag 64 adds exactly 2^-4 to the diagonal
    and touches nothing else."""
    for P in (1, 37, 257):
        rng = np.random.default_rng(P)
        A = fc.ints(rng, (P, P), 60).astype(np.float64)
        A[P // 2, P // 2] = 64.0
        X = _Buf(be, A, ld=P, out=True)
        be.shift_diag(X.view, 0.0)
        assert _bits_equal(be.to_host(X.dev), X.host)
        be.shift_diag(X.view, 2.0 ** -10)
        got, clean = X.fetch()
        assert clean and np.array_equal(got, A + 2.0 ** -4 * np.eye(P)), P


def test_block_chol_ladder_of_one_block(be):
    """isdf_block_chol with the duplicated-point block next to a healthy block and an empty one (NaN outside the diagonal
    blocks): shift_used is the singular block's rung, the healthy block's factor is bit-identical to the one a call without the
    singular block gives, everything outside the blocks is +0.0."""
    c = fc.singular_case()
    S = c['A'].astype(np.float64)
    H, _ = fc.healthy_matrix(65)
    ns = S.shape[0]

    def run(blocks):
        sizes = [b.shape[0] for b in blocks]
        off = _offsets(sizes)
        P = int(off[-1])
        A = np.full((P, P), np.nan)
        for b, blk in enumerate(blocks):
            o = int(off[b])
            A[o:o + blk.shape[0], o:o + blk.shape[0]] = blk
        d_A = _Buf(be, A, ld=P)
        D = _Buf(be, np.full((P, P), np.nan), ld=P, out=True)
        used = be.block_chol(d_A.view, off, 0.0, D.view)
        got, clean = D.fetch()
        assert clean and d_A.unchanged()
        return used, got, off
    used, got, off = run([S, np.zeros((0, 0)), H])
    used_h, got_h, _ = run([np.zeros((0, 0)), H])
    assert used in (1e-14, 1e-12) and used_h == 0.0, (used, used_h)
    assert _bits_equal(got[ns:, ns:], got_h)
    outside = got.copy()
    outside[:ns, :ns] = 0.0
    outside[ns:, ns:] = 0.0
    assert _bits_equal(outside, np.zeros_like(outside))
    md = max(c['maxdiag'], H.diagonal().max())
    r = _chol_ratio('block_chol singular block', got[:ns, :ns], fc.shifted(S, used, md), md)
    assert r <= ROUNDING_FACTOR, r


# ---- E. rounding cases ------------------------------------------------------------------------------------------------------
def _gauss_factor(rng, P):
    M = rng.standard_normal((P, P))
    return np.linalg.cholesky(M.dot(M.T) + P * np.eye(P))


@pytest.mark.parametrize('P,n,backward', [(300, 37, 0), (300, 37, 1), (2100, 8, 0), (2100, 8, 1)])
def test_dtrsm_rounding_against_longdouble(be, P, n, backward):
    """rocBLAS dtrsm as one block (P = 300) and left-looking over three blocks (P = 2100) through isdf_factor_solve_half on a
    Gaussian factor and right-hand side, against substitution in np.longdouble."""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63
    rng = np.random.default_rng([P, n, backward])
    L, B = _gauss_factor(rng, P), rng.standard_normal((P, n))
    d_L = _Buf(be, fc.nan_upper(L), ld=P)
    X = _Buf(be, B, ld=n + 3, out=True)
    prof = _profiled(be, lambda: be.factor_solve_half(d_L.view, bool(backward), X.view))
    got, clean = X.fetch()
    assert clean and d_L.unchanged() and _watched(prof) == {DTRSM: fc.trsm_calls(P)}, _watched(prof)
    ref = fc.solve_lower_longdouble(L, B, trans=bool(backward))
    hst = np.linalg.solve(np.tril(L).T if backward else np.tril(L), B)
    r = _ratio('dtrsm %d block(s) P=%d n=%d backward=%d (Gaussian)' % (fc.trsm_calls(P), P, n, backward), got, hst, ref)
    assert np.isfinite(got).all() and r <= ROUNDING_FACTOR, r


def _chol_longdouble(A):
    A = np.asarray(A, dtype=np.longdouble)
    P = A.shape[0]
    L = np.zeros((P, P), dtype=np.longdouble)
    for j in range(P):
        L[j, j] = np.sqrt(A[j, j] - L[j, :j].dot(L[j, :j]))
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j].dot(L[j, :j])) / L[j, j]
    return L


def test_dpotrf_rounding_against_longdouble(be):
    """rocsolver_dpotrf through isdf_chol_inplace on a Gaussian M M^T + P I (P = 200), against a Cholesky factorisation in
    np.longdouble."""
    P = 200
    M = np.random.default_rng(8).standard_normal((P, P))
    A = M.dot(M.T) + P * np.eye(P)
    A = (A + A.T) / 2
    X = _Buf(be, A, ld=P, out=True)
    assert be.chol_inplace(X.view, 0.0) == 0.0
    got, clean = X.fetch()
    assert clean
    r = _ratio('dpotrf P=%d (Gaussian)' % P, np.tril(got), np.linalg.cholesky(A), _chol_longdouble(A))
    assert np.isfinite(np.tril(got)).all() and r <= ROUNDING_FACTOR, r


# ---- F. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_leave_every_output_unchanged(be):
    """2 nh != nao, ldt < ng, ldb < ng, ldm < P, kind 3, P = 0 and blk_off[nblk] != P: an error, no watched label, every output
    bit-unchanged; the handle works afterwards."""
    from pyscf_isdf_amd.lib import IsdfError
    rng = np.random.default_rng(6)
    P, nao, ng = 7, 6, 20
    aoP, ao = _Buf(be, fc.ints(rng, (P, nao), 3), ld=nao), _Buf(be, fc.ints(rng, (nao, ng), 3), ld=_odd(ng))
    psiP, psi = _Buf(be, fc.ints(rng, (P, 2), 3), ld=2), _Buf(be, fc.ints(rng, (2, ng), 3), ld=_odd(ng))
    L = _Buf(be, fc.nan_upper(fc.factor_pair(P, 0)[0]), ld=P)
    d_ip = _dev_ip(be, np.arange(P))
    call, p = be.handle.call, be._p
    reg = ctypes.c_double(-1.0)
    fails = []

    def refused(name, outs, fn):
        be._stream()
        be.prof_reset()
        bad = []
        try:
            fn()
            bad.append('the call was accepted')
        except IsdfError:
            pass
        be.synchronize()
        if _watched(be.prof_results()):
            bad.append('a refused call recorded %s' % _watched(be.prof_results()))
        for o in outs:
            if not o.unchanged():
                bad.append('an output changed')
        if bad:
            fails.append((name, bad))

    def fresh(nrow, ncol, ld=None):
        return _Buf(be, fc.ints(rng, (nrow, ncol), 4), ld=ld, out=True)

    A, B, aoP_out = fresh(P, P, P), fresh(P, ng), fresh(P, nao, nao)
    refused('gram_sq 2 nh != nao', [A], lambda: be.gram_sq(aoP.view, A.view, nh=2))
    refused('pair_gram_rows 2 nh != nao', [B], lambda: be.pair_gram_rows(aoP.view, ao.view, ng, B.view, nh=2))
    refused('fit_prepare_cplx 2 nh != nao', [A, aoP_out], lambda: be.fit_prepare_cplx(ao.view, 2, d_ip, 0.0, aoP_out.view, A.view))
    refused('fit_apply_cplx 2 nh != nao', [B], lambda: be.fit_apply_cplx(L.view, aoP.view, 2, ao.view, ng, B.view))
    refused('gram_prod_cplx 2 nh != nao', [A], lambda: be.gram_prod_cplx(aoP.view, 2, psiP.view, 1, A.view))
    refused('fit_apply ldt < ng', [B], lambda: call('isdf_fit_apply', p(L.view), p(aoP.view), P, nao, p(ao.view), ng, ao.ld, 0,
                                                    p(B.view), ng - 1))
    refused('pair_gram_rows ldb < ng', [B], lambda: call('isdf_pair_gram_rows', p(aoP.view), P, nao, 0, p(ao.view), ng, ao.ld,
                                                         p(B.view), ng - 1))
    refused('pair_prod_rows ldb < ng', [B], lambda: call('isdf_pair_prod_rows', p(aoP.view), P, nao, p(psiP.view), 2, p(ao.view),
                                                         ao.ld, p(psi.view), psi.ld, ng, p(B.view), ng - 1))
    refused('W_from_factor ldm < P', [A], lambda: call('isdf_W_from_factor', p(L.view), P, 0, p(A.view), P - 1))
    refused('W_from_factor kind 3', [A], lambda: be.W_from_factor(L.view, 3, A.view))
    refused('gram_sq P = 0', [A], lambda: call('isdf_gram_sq', p(aoP.view), 0, nao, 0, p(A.view)))
    refused('gather_aoP P = 0', [aoP_out], lambda: call('isdf_gather_aoP', p(ao.view), nao, ao.ld, p(d_ip), 0, p(aoP_out.view)))
    refused('factor_solve P = 0', [B], lambda: call('isdf_factor_solve', p(L.view), 0, p(B.view), ng, B.ld))
    refused('chol_inplace P = 0', [A], lambda: call('isdf_chol_inplace', p(A.view), 0, 0.0, None, ctypes.byref(reg)))
    refused('block_chol blk_off[nblk] != P', [A], lambda: be.block_chol(L.view, np.array([0, 3, P - 1]), 0.0, A.view))
    for o in (aoP, ao, psiP, psi, L):
        assert o.unchanged()
    assert reg.value == -1.0
    _finish('refusals', 15, fails)
    out = _Buf(be, np.full((P, P), np.nan), ld=P, out=True)
    be.gram_sq(aoP.view, out.view)
    a = aoP._win(aoP.host).astype(np.int64)
    assert np.array_equal(out.fetch()[0], fc.gram_sq_ref(a))
