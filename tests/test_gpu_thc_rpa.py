"""Direct RPA from the ISDF factors on the device (-m gpu): isdf_thc_chi0 on integer data (exact in FP64 whatever the order of the
sums, so equality is exact) and on random reals, isdf_logdet_lu against numpy.linalg.slogdet, then rpa end to end against the same
orchestration on the CPU checker backend (tests/rpa_backend.py) and against the plasmon formula on the Be cell.  Cases and helpers
come from tests/test_thc_rpa.py and tests/test_gpu_thc_mp2.py."""
import ctypes
import numpy as np
import pytest
import scipy.linalg
from pyscf_isdf_amd.isdf import ISDF
from pyscf_isdf_amd.lib import IsdfError
from test_thc_mp2 import random_orbitals, be_df
from test_thc_rpa import be_case
from test_gpu_thc_mp2 import E2E, PS, _padded
from rpa_backend import RpaOracleBackend

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps


@pytest.fixture(scope='module')
def be():
    from pyscf_isdf_amd.backend import HipBackend
    return HipBackend(0)


@pytest.mark.parametrize('no,nv', [(1, 1), (3, 4), (4, 7), (5, 9), (17, 68)])
def test_gpu_thc_chi0_is_exact_on_integers(be, no, nv):
    """S = sum_ia (Xo_i Xv_a) d_ia (Xo_i Xv_a)^T with |X| <= 2 and d a power of two in 2^-3 .. 2^3 against int64 arithmetic
    (|8 S| <= 16 * 64 * no nv < 2^21: far below 2^53), for P below, at and past the 16-row MFMA edge and the 128-row tile edge (200:
    two tile rows, an off-diagonal tile stored twice), pair counts of every residue mod 4, past one 16-deep chunk in the virtual index
    (68) and one 16-wide block in the occupied one (17).  Three layouts per shape: even leading dimensions on 16-byte aligned rows
    (vector loads), odd leading dimensions, and even ones on a base that is off by one element (both element-wise).  The padding of
    every operand is NaN; S's must stay NaN, and S must equal its transpose bit for bit."""
    rng = np.random.default_rng(1000 * no + nv)
    for P in PS:
        xo = rng.integers(-2, 3, (P, no)).astype(float)
        xv = rng.integers(-2, 3, (P, nv)).astype(float)
        d = 2.0 ** rng.integers(-3, 4, (no, nv))
        y = (xo.astype(np.int64)[:, :, None] * xv.astype(np.int64)[:, None, :]).reshape(P, -1)
        ref = (y * (8 * d).astype(np.int64).reshape(-1)) @ y.T
        for ldo, ldv, ldd, lead in ((no + 2 + (no & 1), nv + 4 + (nv & 1), nv + 2, 0), (no + 1 + (no & 1), nv + 3 + (nv & 1), nv + 1, 0),
                                    (no + 2 + (no & 1), nv + 4 + (nv & 1), nv, 1)):
            bo, d_xo = _padded(be, xo, ldo, lead)
            bv, d_xv = _padded(be, xv, ldv, lead)
            bd, d_d = _padded(be, d, ldd, lead)
            lds = P + 3
            sbuf = be.to_device(np.full((P, lds), np.nan))
            be.thc_chi0(d_xo, d_xv, d_d, sbuf[:, :P])
            got = be.to_host(sbuf)
            assert np.isnan(got[:, P:]).all(), (P, ldo, ldv, lead)
            assert np.array_equal(got[:, :P] * 8, ref.astype(float)), (P, ldo, ldv, lead)
            assert np.array_equal(got[:, :P].view(np.int64), got[:, :P].T.copy().view(np.int64)), (P, ldo, ldv, lead)


def test_gpu_thc_chi0_is_symmetric_to_the_bit_on_real_data(be):
    """On random reals y_P (d y_Q) and y_Q (d y_P) differ in the last bit: S = S^T to the bit only because each value is stored
    twice.  Against numpy: each side is a sum of no nv terms, each term a product of five numbers (4 roundings) - error
    <= (no nv + 4) eps sum |terms| per side to first order."""
    rng = np.random.default_rng(6)
    P, no, nv = 333, 13, 51
    xo, xv = rng.standard_normal((P, no)), rng.standard_normal((P, nv))
    d = rng.random((no, nv)) + 0.1
    S = be.empty((P, P))
    be.thc_chi0(be.to_device(xo), be.to_device(xv), be.to_device(d), S)
    got = be.to_host(S)
    y = (xo[:, :, None] * xv[:, None, :]).reshape(P, -1)
    ref = (y * d.reshape(-1)).dot(y.T)
    assert np.array_equal(got.view(np.int64), got.T.copy().view(np.int64))
    tol = 2 * (no * nv + 5) * EPS * (abs(y) * d.reshape(-1)).dot(abs(y).T)
    print('thc_chi0 on reals: max |got - numpy| / tol = %.3f' % (abs(got - ref) / tol).max())
    assert (abs(got - ref) <= tol).all()


def test_gpu_thc_chi0_and_logdet_lu_refuse_short_leading_dimensions_and_zero_sizes(be):
    x = be.zeros((8, 4))
    d = be.zeros((4, 4))
    S = be.zeros((8, 8))
    p = be._p
    for args in ((8, p(x), 3, 4, p(x), 4, 4, p(d), 4, p(S), 8), (8, p(x), 4, 4, p(x), 3, 4, p(d), 4, p(S), 8),
                 (8, p(x), 4, 4, p(x), 4, 4, p(d), 3, p(S), 8), (8, p(x), 4, 4, p(x), 4, 4, p(d), 4, p(S), 7),
                 (0, p(x), 4, 4, p(x), 4, 4, p(d), 4, p(S), 8), (8, p(x), 4, 0, p(x), 4, 4, p(d), 4, p(S), 8),
                 (8, p(x), 4, 4, p(x), 4, 0, p(d), 4, p(S), 8)):
        with pytest.raises(IsdfError, match=r'status 1\)'):            # ISDF_ERR_ARG
            be.handle.call('isdf_thc_chi0', *args)
    la, sg = ctypes.c_double(0.0), ctypes.c_int(0)
    for args in ((8, p(S), 7, 0.0, ctypes.byref(la), ctypes.byref(sg)), (0, p(S), 8, 0.0, ctypes.byref(la), ctypes.byref(sg))):
        with pytest.raises(IsdfError, match=r'status 1\)'):
            be.handle.call('isdf_logdet_lu', *args)


def test_gpu_logdet_lu_refuses_a_singular_matrix(be):
    a = np.arange(16.0).reshape(4, 4)
    a[2] = 0.0
    with pytest.raises(IsdfError, match=r'status 4\)'):                # ISDF_ERR_NUM
        be.logdet_lu(be.to_device(a))


@pytest.mark.parametrize('n', [1, 31, 64, 65, 200])
def test_gpu_logdet_lu_matches_slogdet(be, n):
    """ln|det| and the sign against numpy.linalg.slogdet on M = n I + U(-1, 1)^{n x n} (dominant by rows and by columns: growth
    factor rho <= 2), on M with its rows in an odd permutation (the pivot searches swap them back: the sign comes from the parity
    alone), on that with one row negated (a negative pivot and an odd parity: positive again) and on M with one row negated.
    ld = n + 3 with NaN padding, which must stay; the shift argument adds the n I.
    Bound: partial pivoting is backward stable, L U = A + E with ||E|| <= n eps rho ||A|| to first order (Higham, Accuracy and
    Stability, Thm 9.3 with |L| <= 1), and d ln|det A| = Tr(A^-1 E), so |error| <= n ||A^-1|| ||E|| <= n^2 eps rho cond_2(A); the
    sum of n logarithms adds (n + 1) eps sum |ln|u_ii||.  Both sides carry it: twice that."""
    rng = np.random.default_rng(n)
    m0 = rng.uniform(-1, 1, (n, n))
    perm = np.arange(n)
    if n > 1:
        perm[[0, n - 1]] = perm[[n - 1, 0]]                            # one transposition: odd
        if n > 4:
            perm[1:4] = perm[[2, 3, 1]]                                # and a 3-cycle: even
    neg = np.ones(n)
    neg[n // 2] = -1
    for name, rows, scale, shift in (('dominant', np.arange(n), np.ones(n), float(n)), ('permuted', perm, np.ones(n), 0.0),
                                     ('permuted, negated', perm, neg, 0.0), ('negated', np.arange(n), neg, 0.0)):
        m = m0 + n * np.eye(n)
        full = (scale[:, None] * m)[rows]
        given = full - shift * np.eye(n)                               # what the call gets: it adds shift I itself
        buf, A = _padded(be, given, n + 3)
        logabs, sign = be.logdet_lu(A, shift)
        rsign, rlog = np.linalg.slogdet(full)
        u = np.diag(scipy.linalg.lu(full)[2])
        tol = 2 * (n * n * EPS * 2 * np.linalg.cond(full) + (n + 1) * EPS * abs(np.log(abs(u))).sum())
        print('logdet_lu n %d %s: %.15e  numpy %.15e  |diff| %.2e  tol %.2e  sign %d' % (n, name, logabs, rlog, abs(logabs - rlog), tol, sign))
        assert sign == int(rsign), (n, name)
        assert abs(logabs - rlog) <= tol, (n, name)
        got = be.to_host(buf).reshape(n, n + 3)
        assert np.isnan(got[:, n:]).all() and np.isfinite(got[:, :n]).all()
        buf2, A2 = _padded(be, given, n + 3)
        assert be.logdet_lu(A2, shift) == (logabs, sign)               # the same bits again
    if n > 1:
        assert int(np.linalg.slogdet(m[perm])[0]) == -1


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(E2E))
def test_gpu_rpa_matches_the_checker_backend(name):
    """rpa on the device against the same orchestration on the CPU checker backend (each on its own build of the factors) to 1e-10
    relative in e_corr and e_mp2_direct; a second run on the device returns the same bits in e_corr and in every term."""
    mk, nocc, c_isdf = E2E[name]
    cell = mk()
    c, e, occ = random_orbitals(cell, nocc, S=np.eye(cell.nao_nr()))
    dev = ISDF(cell, c_isdf=c_isdf, select='global')
    cpu = ISDF(cell, c_isdf=c_isdf, select='global', backend=RpaOracleBackend())
    r1 = dev.rpa(c, e, occ)
    r2 = dev.rpa(c, e, occ)
    ref = cpu.rpa(c, e, occ)
    assert np.array_equal(dev.ip, cpu.ip)
    rel = abs(r1.e_corr - ref.e_corr) / abs(ref.e_corr)
    rel2 = abs(r1.e_mp2_direct - ref.e_mp2_direct) / abs(ref.e_mp2_direct)
    print('%s: P %d  device %.14e  checker %.14e  relative %.2e  second order %.14e relative %.2e  loop %.3f s' %
          (name, len(dev.ip), r1.e_corr, ref.e_corr, rel, r1.e_mp2_direct, rel2, r1.seconds))
    assert r1.nw == ref.nw == 40 and rel <= 1e-10 and rel2 <= 1e-10
    assert r1.e_corr == r2.e_corr and np.array_equal(r1.terms, r2.terms) and r1.e_mp2_direct == r2.e_mp2_direct


def test_gpu_be_cell_matches_the_plasmon_formula():
    """tests/test_thc_rpa.py::test_be_cell_matches_the_plasmon_formula_of_the_exact_integrals with everything from the device."""
    df = be_df()
    c, e, occ, ref, tol = be_case(df)
    assert df.backend.name.startswith('hip')
    res = df.rpa(c, e, occ)
    rel = abs(res.e_corr - ref) / abs(ref)
    print('Be on the device: e_corr %.12e  plasmon %.12e  relative %.2e  bound %.1e' % (res.e_corr, ref, rel, tol))
    assert rel <= tol
    assert df.rpa(c, e, occ).e_corr == res.e_corr
