"""Opposite-spin MP2 from the ISDF factors on the device (-m gpu): isdf_thc_pair and isdf_trace_sq alone on integer data (exact in
FP64 whatever the order of the sums, so equality is exact), then mp2_os end to end against the same orchestration on the CPU checker
backend (tests/thc_backend.py) and against the reference's pinned Be energy.  Cases and helpers come from tests/test_thc_mp2.py."""
import ctypes
import numpy as np
import pytest
from pyscf_isdf_amd import gto
from pyscf_isdf_amd.isdf import ISDF
from pyscf_isdf_amd.lib import IsdfError
from test_thc_mp2 import random_orbitals, be_df, check_be_pin
from cells import cell_diamond_prim
from thc_backend import ThcOracleBackend

pytestmark = pytest.mark.gpu

PS = (1, 15, 16, 17, 63, 64, 65, 129, 200)


@pytest.fixture(scope='module')
def be():
    from pyscf_isdf_amd.backend import HipBackend
    return HipBackend(0)


def _padded(be, a, ld, lead=0):
    """a (rows, k) on the device inside a NaN-filled buffer with leading dimension ld, starting ``lead`` elements into it: (buffer, view)."""
    rows, k = a.shape
    buf = be.to_device(np.full(lead + rows * ld, np.nan))
    view = buf[lead:].view(rows, ld)[:, :k]
    view.copy_(be.to_device(a))
    return buf, view


@pytest.mark.parametrize('no,nv', [(1, 1), (3, 4), (4, 7), (5, 9), (17, 68)])
def test_gpu_thc_pair_is_exact_on_integers(be, no, nv):
    """A = (Xo diag(so) Xo^T) o (Xv diag(sv) Xv^T) with |X| <= 3 and scales that are powers of two against int64 arithmetic, for P
    below, at and past the 16-row MFMA edge and the 128-row tile edge (200: two tile rows, an off-diagonal tile stored twice) and K
    tails of every residue mod 4 and past one 16-deep chunk.  Three layouts per shape: even leading dimensions on 16-byte aligned
    rows (vector loads), odd leading dimensions, and even ones on a base that is off by one element (both element-wise): the kernel
    takes every leading dimension >= K, so none is refused for its alignment.  The padding of every operand is NaN; A's must stay
    NaN, and A must equal its transpose bit for bit."""
    rng = np.random.default_rng(100 * no + nv)
    for P in PS:
        xo = rng.integers(-3, 4, (P, no)).astype(float)
        xv = rng.integers(-3, 4, (P, nv)).astype(float)
        ko, kv = rng.integers(-3, 4, no), rng.integers(-3, 4, nv)
        so, sv = 2.0 ** ko, 2.0 ** kv
        # exact: 8 so and 8 sv are integers
        ref = ((xo.astype(np.int64) * (8 * so).astype(np.int64)) @ xo.astype(np.int64).T) * \
              ((xv.astype(np.int64) * (8 * sv).astype(np.int64)) @ xv.astype(np.int64).T)
        for ldo, ldv, lead in ((no + 2 + (no & 1), nv + 4 + (nv & 1), 0), (no + 1 + (no & 1), nv + 3 + (nv & 1), 0),
                               (no + 2 + (no & 1), nv + 4 + (nv & 1), 1)):
            bo, d_xo = _padded(be, xo, ldo, lead)
            bv, d_xv = _padded(be, xv, ldv, lead)
            lda = P + 3
            abuf = be.to_device(np.full((P, lda), np.nan))
            A = abuf[:, :P]
            be.thc_pair(d_xo, be.to_device(so), d_xv, be.to_device(sv), A)
            got = be.to_host(abuf)
            assert np.isnan(got[:, P:]).all(), (P, ldo, ldv, lead)
            assert np.array_equal(got[:, :P] * 64, ref.astype(float)), (P, ldo, ldv, lead)
            assert np.array_equal(got[:, :P].view(np.int64), got[:, :P].T.copy().view(np.int64)), (P, ldo, ldv, lead)


def test_gpu_thc_pair_is_symmetric_to_the_bit_on_real_data(be):
    """On random reals a_p (s a_q) and a_q (s a_p) differ in the last bit: A = A^T to the bit only because each value is stored
    twice.  Against numpy to the rounding of sums of no + nv products."""
    rng = np.random.default_rng(5)
    P, no, nv = 333, 13, 51
    xo, xv = rng.standard_normal((P, no)), rng.standard_normal((P, nv))
    so, sv = rng.random(no), rng.random(nv)
    A = be.empty((P, P))
    be.thc_pair(be.to_device(xo), be.to_device(so), be.to_device(xv), be.to_device(sv), A)
    got = be.to_host(A)
    ref = (xo * so).dot(xo.T) * (xv * sv).dot(xv.T)
    assert np.array_equal(got.view(np.int64), got.T.copy().view(np.int64))
    # each factor is a sum of K products (error <= (K + 2) eps sum |terms|), once here and once in numpy, then one product
    tol = 2 * (no + nv + 5) * np.finfo(float).eps * (abs(xo) * so).dot(abs(xo).T) * (abs(xv) * sv).dot(abs(xv).T)
    assert (abs(got - ref) <= tol).all()


def test_gpu_thc_pair_and_trace_sq_refuse_short_leading_dimensions(be):
    x = be.zeros((8, 4))
    s = be.zeros((4,))
    A = be.zeros((8, 8))
    out = ctypes.c_double(0.0)
    p = be._p
    for args in ((8, p(x), 3, 4, p(s), p(x), 4, 4, p(s), p(A), 8), (8, p(x), 4, 4, p(s), p(x), 3, 4, p(s), p(A), 8),
                 (8, p(x), 4, 4, p(s), p(x), 4, 4, p(s), p(A), 7), (0, p(x), 4, 4, p(s), p(x), 4, 4, p(s), p(A), 8),
                 (8, p(x), 4, 0, p(s), p(x), 4, 4, p(s), p(A), 8)):
        with pytest.raises(IsdfError, match=r'status 1\)'):            # ISDF_ERR_ARG
            be.handle.call('isdf_thc_pair', *args)
    for args in ((8, p(A), 7, ctypes.byref(out)), (0, p(A), 8, ctypes.byref(out))):
        with pytest.raises(IsdfError, match=r'status 1\)'):
            be.handle.call('isdf_trace_sq', *args)


@pytest.mark.parametrize('n', [1, 31, 32, 33, 65, 200])
def test_gpu_trace_sq_is_exact_on_integers_and_repeats_to_the_bit(be, n):
    """sum_ij B_ij B_ji on integers |B| <= 3 (|sum| <= 9 n^2: exact) with ld > n and NaN in the padding, at, below and past the 32 x 32
    tile edge; then on random reals twice: the same bits, and the value of the float64 einsum to the rounding of n^2 terms."""
    rng = np.random.default_rng(n)
    b = rng.integers(-3, 4, (n, n))
    buf, B = _padded(be, b.astype(float), n + 5)
    assert be.trace_sq(B) == float((b * b.T).sum())
    r = rng.standard_normal((n, n))
    buf, B = _padded(be, r, n + 1)
    t1, t2 = be.trace_sq(B), be.trace_sq(B)
    assert t1 == t2
    assert abs(t1 - np.einsum('ij,ji->', r, r)) <= 2 * n * n * np.finfo(float).eps * abs(r * r.T).sum()      # two sums of n^2 terms, worst case


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
def _diamond222():
    """Diamond 2 x 2 x 2, gth-szv (64 AOs) on 24^3; with c_isdf = 6 P = 384: three tile rows of the pair kernel, and W A crosses
    isdf_gemm_nt's tile edges."""
    return gto.diamond_supercell(2, basis='gth-szv', mesh=(24, 24, 24))


E2E = {'diamond-prim': (lambda: cell_diamond_prim(), 4, 3), 'diamond-222': (_diamond222, 32, 6)}


@pytest.mark.parametrize('name', list(E2E))
def test_gpu_mp2_os_matches_the_checker_backend(name):
    """mp2_os on the device against the same orchestration on the CPU checker backend (each on its own build of the factors) to
    1e-10 relative, the bound of the product-vs-checker comparisons; and a second run on the device returns the same bits."""
    mk, nocc, c_isdf = E2E[name]
    cell = mk()
    c, e, occ = random_orbitals(cell, nocc, S=np.eye(cell.nao_nr()))       # any C serves here; the analytic S of 64 AOs takes seconds
    dev = ISDF(cell, c_isdf=c_isdf, select='global')
    cpu = ISDF(cell, c_isdf=c_isdf, select='global', backend=ThcOracleBackend())
    r1 = dev.mp2_os(c, e, occ)
    r2 = dev.mp2_os(c, e, occ)
    ref = cpu.mp2_os(c, e, occ)
    assert np.array_equal(dev.ip, cpu.ip)
    rel = abs(r1.e_os - ref.e_os) / abs(ref.e_os)
    print('%s: P %d  ngrid %d  device %.14e  checker %.14e  relative %.2e' % (name, len(dev.ip), r1.ngrid, r1.e_os, ref.e_os, rel))
    assert r1.ngrid == ref.ngrid and rel <= 1e-10
    assert r1.e_os == r2.e_os and np.array_equal(r1.terms, r2.terms)
    A = dev.backend.to_host(dev._bufs['thc_A'][:len(dev.ip) ** 2].view(len(dev.ip), -1))
    assert np.array_equal(A, A.T)


def test_gpu_be_cell_reproduces_the_reference_kmp2_energy():
    """The pin of tests/test_thc_mp2.py::test_be_cell_reproduces_the_reference_kmp2_energy with everything from the device: get_pp,
    J, K and mp2_os.  Two runs return the same bits."""
    df = be_df()
    res, orbitals = check_be_pin(df)
    assert df.backend.name.startswith('hip')
    assert df.mp2_os(*orbitals, rtol=1e-9).e_os == res.e_os
