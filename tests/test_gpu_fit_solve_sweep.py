"""Sweep of the fit's solve kernels (csrc/trsm.hip, skinny_rows_kernel of csrc/fit.hip) over every form, edge and stride.

The older tests (test_gpu_parity.py: test_block_invert_and_mfma_block_apply, test_block_solve_*, test_gpu_row_frontier.py) reach
block_apply_reg_kernel<8,2> and <16,1> only, give every workgroup exactly one column tile, and compare Gaussian data at 1e-10 to
1e-11.  This module chooses its cases from a restatement of the host dispatch of block_apply_inverse (plan_apply below: the four
register forms by nt = ceil(mmax / 16), the older kernel's tile width by its LDS rule, the refusal, and the persistent grid
gx = min(ntile, ceil(CUs * block_apply_waves / nblk))) and reads what really ran from the profiling label, which names the
instantiation.  A case whose label or work differs from the restatement fails and names both.

  block apply    isdf_block_apply (SQ off) and isdf_pair_rows_block_apply (SQ on: integer aoP, ao in [-2, 2], nao = 9; with option
                 gemm_nn_own and nao = 32 the product squares in its epilogue and the apply runs with SQ off) on
                 - block maxima 1, 15, 16, 17, 127, 128, 129, 130, 156, 160, 161, 182, 192, 193, 234, 255, 256, 257: every bin
                   edge of the register forms and the step to the older kernel, each call with further blocks of 0, 1, 7, 16 and 33
                   rows (empty blocks, blocks below one row tile, wave pairs whose two row tiles are both past m);
                 - the older block_apply_mfma_kernel<64 / 32 / 16> (option block_apply_reg 0) at 16, 96, 97, 288, 289, 1100, 1120;
                 - the persistent column-tile loop of each register form: block_apply_waves 1 and 320 blocks (one of 128 / 156 /
                   182 / 234 rows and small fillers, 830 to 940 rows) make gx = 1 on any device of up to 320 CUs, with n = 5 tiles + 7
                   columns, exactly 4 tiles and 1 column, and ceil(CUs / 2) blocks make gx = 2 with 7 tiles (the last, ragged one
                   taken by one workgroup only); every such case runs twice and must repeat bit for bit;
                 - refusals (1121 rows, all blocks empty, n = 0, ldx < n): an error, X bit-unchanged.
  forward solve  isdf_block_solve(side 0, trans 0) (block_forward_kernel): blocks of 1, 63, 0, 64, 65, 128, 129, 200 rows in one
                 call, n in {1, 255, 256, 257}; isdf_block_invert on the same blocks.
  substitution   option trsm_substitution: subst_kernel<false / true> and transpose_kernel through isdf_block_solve, all four
                 (side, trans), blocks of 1, 64, 0, 65, 512, 513, 577 rows (across the 64-row blocks and the 512-row panels), n = 37.
  rows combine   isdf_rows_combine (skinny_rows_kernel): n in 1..8 (n = 9 must carry the rocBLAS label), rows in {1, 63, 64, 65,
                 129}, ng in {1, 255, 256, 257, 700}, E a column slice of a wider matrix, both values of accumulate.

Layouts, seen by every case: ldx = n + 3 with NaN and a sentinel in the padding; sentinel rows before the first block's row and
after blk_off[nblk]; Dinv / D a diagonal sub-block view of a larger matrix (ldd > P) that holds NaN everywhere outside the diagonal
blocks (for the factors D also above the diagonal inside a block), so a read outside a block or past n poisons the result;
everything around the result must be bit-unchanged.

Two references.
  Exact.  Operands are small integers stored as doubles.  Block apply: Dinv lower triangular in [-3, 3] with exact zeros above the
  diagonal, X in [-4, 4]; every partial sum is an integer far below 2^53 (test_exact_cases_stay_below_2_53), so the int64 numpy
  product IS the answer whatever the summation order.  Solves: L integer lower triangular with diagonal in {1, -1, 2, 4}, X_true
  in [-4, 4], B = op(L) X_true formed in int64 - every intermediate of a substitution is an exact integer and every division is
  exact, so the device must return X_true.  Inverse: D = (I + N1) S (I + N2) with N1^2 = N2^2 = 0 and S a signed unit
  bidiagonal; its inverse (I - N2) S^-1 (I - N1) is an integer matrix, D Dinv == I is checked in int64 on the CPU, and the device's
  Dinv must equal it bit for bit, the zeros above the diagonal and outside the blocks included (rows past blk_off[nblk] keep the
  identity the inverse starts from).  np.array_equal, no tolerance.
  Rounding.  Exact small integers survive a lower-precision path, so one Gaussian case per label and SQ value: Dinv the real
  inverse of the Cholesky factor of M M^T + m I, X Gaussian, against an np.longdouble triangular product.  The measure is the
  error of numpy's float64 product of the same inputs against the same reference, relative to max|ref|; the device may exceed it
  by ROUNDING_FACTOR, the smallest power of two at or above 4 x the largest device / numpy ratio measured on an MI355X, capped
  at 64.

Measured on an MI355X (256 CUs), device error / numpy error, both against the longdouble product:

  label                                 SQ off                SQ on (device / numpy error 1.0: both carry the squared
                                                              product's own rounding, which dominates)
  block_apply_reg_kernel<8,2>           1.55 (128 rows)       1.00
  block_apply_reg_kernel<10,2>          1.62 (156 rows)       1.36
  block_apply_reg_kernel<12,2>          2.24 (182 rows)       1.00
  block_apply_reg_kernel<16,1>          1.65 (234 rows)       1.00
  block_apply_mfma_kernel<64>           1.90 (96 rows)        1.00
  block_apply_mfma_kernel<32>           2.34 (288 rows)       1.00
  block_apply_mfma_kernel<16>           3.25 (289 rows)       1.00

numpy's own error is 6.0e-17 to 3.3e-16 of max|ref| on these cases, the device's 1.4e-16 to 3.3e-16: a row of the result is one
sequential chain of up to 320 fused multiply-adds in the MFMA accumulator where BLAS sums in blocks.  The largest ratio is 3.25;
4 x 3.25 = 13, so ROUNDING_FACTOR = 16.

Found and fixed: nothing.  All 29 GPU tests passed on the first run against the unchanged kernels (3.1 s for the module); the one
source change is the profiling label of block_apply_inverse, which now names the instantiation that runs.

Mutations tried on a scratch copy (not committed):
  - prefetching tile + 1 instead of tile + gridDim.x in block_apply_reg_kernel: the 8 gx = 2 cases fail the exact test (about 60 % of
    the entries).  The 24 gx = 1 cases pass, and have to: with one workgroup per block the two expressions are the same tile.
  - the guard k0 + j < m on the A fragments of block_apply_reg_kernel loosened to <= m (one column past the block, NaN there, inside
    the same allocation): 34 of the 36 edge cases (all but the two of 257 rows, which the older kernel takes), all 32 persistent
    cases, 3 of the 4 own-product cases and the 8 register-form rounding cases fail.  The single block of 256 rows passes, and has to:
    the fragments of NT = 16 end at k = 255, so k = m is never formed.  (Dropping the guard altogether reads up to 16 NT + 32 columns
    past the last block, which in the small cases is past the allocation: not run.)
  - kend one chunk short in block_apply_mfma_kernel: all 14 older-kernel cases, the two edge cases of 257 rows and the 6 older-kernel
    rounding cases fail.
  - the coupling loop of block_forward_kernel stopping 8 finished rows early: all 4 forward-solve cases (first wrong row 192: row 64 of
    the 65-row block, the first row whose coupling to a finished sub-block is cut) and the inverse fail.
  - the panel update of trsm_lower_left one column short (K = r0 - 1): the two substitution cases that reach subst_kernel<false>
    across a 512-row panel, (side, trans) = (0, 0) and (1, 1), fail in the 513- and 577-row blocks; the other two solve with
    the transposed branch, which the mutation leaves alone.
  - skinny_rows_kernel staging E without p0: 31 of the 36 distinct rows-combine cases with more than 64 rows fail.  The other five
    pass, and have to: four have n = 9, which rocBLAS takes, and in (n = 5, rows = 65, ng = 1) the only row of Y that meets a wrong
    E entry, Y[64, 0], was drawn as 0.
"""
import ctypes
import itertools
import numpy as np
import pytest

gpu = pytest.mark.gpu

# ---- restatement of the host-side dispatch of block_apply_inverse (trsm.hip) ------------------------------------------------
REG_LABEL = {8: 'block_apply_reg_kernel<8,2>[byte]', 10: 'block_apply_reg_kernel<10,2>[byte]',
             12: 'block_apply_reg_kernel<12,2>[byte]', 16: 'block_apply_reg_kernel<16,1>[byte]'}
OLD_LABEL = {64: 'block_apply_mfma_kernel<64>[byte]', 32: 'block_apply_mfma_kernel<32>[byte]',
             16: 'block_apply_mfma_kernel<16>[byte]'}
ALL_LABELS = set(REG_LABEL.values()) | set(OLD_LABEL.values())
ROCBLAS_GEMM = 'rocblas_dgemm[flop]'
NN_SQ = 'gemm_nn_mfma_kernel<true>[flop]'
SKINNY = 'skinny_rows_kernel[byte]'
FORWARD = 'block_forward_kernel[byte]'
SUBST = {False: 'trsm_subst_kernel<false>[flop]', True: 'trsm_subst_kernel<true>[flop]'}
CPU_TEST_CUS = 256
DEFAULT_WAVES = 16


def cdiv(a, b):
    return -(-a // b)


class Plan(dict):
    __getattr__ = dict.__getitem__


def plan_apply(sizes, n, ncu, reg=True, waves=DEFAULT_WAVES):
    """block_apply_inverse: the label of the instantiation that runs (None: the call is refused), and for the register forms the
    tile width, the tile count, gx and the fewest / most loop steps a workgroup of a non-empty block takes."""
    nblk = len(sizes)
    mmax = max(sizes) if sizes else 0
    if nblk <= 0 or n <= 0 or mmax <= 0:
        return Plan(label=None)
    mpad = (mmax + 31) & ~31
    if reg and mmax <= 256:
        nt = cdiv(mmax, 16)
        NT, NCT = (8, 2) if nt <= 8 else (10, 2) if nt <= 10 else (12, 2) if nt <= 12 else (16, 1)
        TN = 16 * NCT
        ntile = cdiv(n, TN)
        gx = max(1, min(ntile, cdiv(ncu * waves, nblk)))
        return Plan(label=REG_LABEL[NT], kind='reg', NT=NT, TN=TN, ntile=ntile, gx=gx, steps_min=ntile // gx, steps_max=cdiv(ntile, gx))
    if mpad * (64 + 2) * 8 <= 52 * 1024:
        TN = 64
    elif mpad * (32 + 2) * 8 <= 80 * 1024:
        TN = 32
    elif mpad * (16 + 2) * 8 <= 160 * 1024:
        TN = 16
    else:
        return Plan(label=None)
    return Plan(label=OLD_LABEL[TN], kind='old', TN=TN, ntile=cdiv(n, TN), gx=cdiv(n, TN), steps_min=1, steps_max=1)


# ---- the case lists ---------------------------------------------------------------------------------------------------------
EDGE_MMAX = (1, 15, 16, 17, 127, 128, 129, 130, 156, 160, 161, 182, 192, 193, 234, 255, 256, 257)
OLD_MMAX = (16, 96, 97, 288, 289, 1100, 1120)
MIXED = (0, 1, 7, 16, 33)                          # the other blocks of a call
PERSIST_M = {8: 128, 10: 156, 12: 182, 16: 234}    # the block of the size under test, per register form
PERSIST_NBLK = 320
FILLER = (1, 2, 0, 3, 1, 5, 2, 0, 7, 1)            # the filler blocks of the persistent cases, cycled
N_PLAIN = 70                                       # 2 tiles of 32 + 6, 4 of 16 + 6, 1 of 64 + 6
NAO = 9
OWN_NAO = 32


class Case(dict):
    __getattr__ = dict.__getitem__

    def name(self):
        return '%s mmax=%d nblk=%d n=%d%s%s%s%s' % (self.tag, max(self.sizes), len(self.sizes), self.n, ' SQ' if self.sq else '',
                                                   '' if self.reg else ' reg=0', ' waves=%d' % self.waves if self.waves != DEFAULT_WAVES else '',
                                                   ' own' if self.own else '')


def _case(tag, sizes, n, sq, reg=True, waves=DEFAULT_WAVES, own=False):
    return Case(tag=tag, sizes=tuple(int(s) for s in sizes), n=int(n), sq=bool(sq), reg=bool(reg), waves=int(waves), own=bool(own))


def mixed_sizes(mmax):
    """The largest block decides the form; around it the blocks of MIXED that do not exceed it (an empty one always)."""
    small = [s for s in MIXED if s <= mmax]
    return small[:3] + [mmax] + small[3:] + [0]


def edge_cases():
    return [_case('edge', mixed_sizes(m), N_PLAIN, sq) for m in EDGE_MMAX for sq in (False, True)]


def old_cases():
    return [_case('older', mixed_sizes(m), N_PLAIN, sq, reg=False) for m in OLD_MMAX for sq in (False, True)]


def persist_sizes(m, nblk):
    """nblk blocks: the one of m rows in the middle, fillers of 0 to 7 rows around it."""
    sizes = [FILLER[i % len(FILLER)] for i in range(nblk)]
    sizes[nblk // 2] = m
    return sizes


def gx2_nblk(ncu):
    return cdiv(ncu, 2)


def persist_cases(NT, ncu):
    """gx = 1: 5 tiles + 7 columns, exactly 4 tiles, 1 column (a single step: listed with the loop because it shares the grid);
    gx = 2 (3 for a CU count just above a multiple of nblk): 6 tiles + 7 columns."""
    TN = 32 if NT != 16 else 16
    m = PERSIST_M[NT]
    out = []
    for sq in (False, True):
        for n in (5 * TN + 7, 4 * TN, 1):
            out.append(_case('gx1', persist_sizes(m, PERSIST_NBLK), n, sq, waves=1))
        out.append(_case('gx2', persist_sizes(m, gx2_nblk(ncu)), 6 * TN + 7, sq, waves=1))
    return out


def own_cases():
    """isdf_pair_rows_block_apply with option gemm_nn_own and operands the own NN kernel takes (P > 128 rows filling a 256-row tile
    to 87 %, nao = 32, even ng and leading dimensions): the square rides the product, the apply runs with SQ off."""
    return [_case('own', (130, 0, 33, 93), 70, True, own=True), _case('own', (256,), 70, True, own=True),
            _case('own', (182, 41), 70, True, own=True), _case('own', (97, 128), 70, True, own=True)]


def apply_worst_partial_sum(c):
    """Upper bound of |any partial sum| of a block-apply case: m terms of |Dinv| <= 3 times |X| <= 4 (SQ: (nao * 2 * 2)^2)."""
    xmax = (((OWN_NAO if c.own else NAO) * 4) ** 2) if c.sq else 4
    return max(c.sizes) * 3 * xmax


FORWARD_SIZES = (1, 63, 0, 64, 65, 128, 129, 200)
FORWARD_N = (1, 255, 256, 257)
SUBST_SIZES = (1, 64, 0, 65, 512, 513, 577)
SUBST_N = 37
COMBINE_ROWS = (1, 63, 64, 65, 129)
COMBINE_NG = (1, 255, 256, 257, 700)
TAIL_ROWS = 4                                      # rows of the matrices past blk_off[nblk]


def combine_cases():
    """(n, rows, ng, accumulate): every (rows, ng) pair with both values of accumulate and n walking 1..9, then every n at
    (65, 257); n = 9 is rocBLAS's."""
    out = []
    for i, (rows, ng) in enumerate(itertools.product(COMBINE_ROWS, COMBINE_NG)):
        for acc in (0, 1):
            out.append((1 + (2 * i + acc) % 9, rows, ng, acc))
    for n in range(1, 10):
        for acc in (0, 1):
            out.append((n, 65, 257, acc))
    return out


def _ints(rng, shape, m):
    return rng.integers(-m, m + 1, size=shape).astype(np.int64)


def int_factor(rng, m):
    """Integer lower triangular L (m x m): diagonal in {1, -1, 2, 4}, below it [-3, 3]."""
    L = np.tril(_ints(rng, (m, m), 3), -1)
    L[np.arange(m), np.arange(m)] = rng.choice(np.array([1, -1, 2, 4]), size=m)
    return L


def int_unit_pair(rng, m):
    """(D, Dinv), integer lower triangular with unit diagonal, D Dinv = I: D = (I + N1) S (I + N2), N1 / N2 nonzero only in rows
    from h1 / h2 on and columns before them (so N^2 = 0 and (I + N)^-1 = I - N), sparse with entries in [-2, 2]; S = I + the
    sub-diagonal s in {-1, 1}, whose inverse has entries (-1)^(i-j) s_j+1 ... s_i."""
    eye = np.eye(m, dtype=np.int64)
    if m <= 1:
        return eye.copy(), eye.copy()

    def nil(h):
        N = np.zeros((m, m), dtype=np.int64)
        blk = _ints(rng, (m - h, h), 2)
        blk[rng.random((m - h, h)) < 0.7] = 0
        N[h:, :h] = blk
        return N
    N1, N2 = nil(max(1, m // 3)), nil(max(1, (2 * m) // 3))
    s = rng.choice(np.array([-1, 1]), size=m - 1)
    S = eye + np.diag(s, -1)
    Sinv = eye.copy()
    for j in range(m):
        p = 1
        for i in range(j + 1, m):
            p *= -s[i - 1]
            Sinv[i, j] = p
    D = (eye + N1).dot(S).dot(eye + N2)
    Dinv = (eye - N2).dot(Sinv).dot(eye - N1)
    return D, Dinv


def invert_blocks(seed=11):
    rng = np.random.default_rng(seed)
    return [int_unit_pair(rng, m) for m in FORWARD_SIZES]


# ---- CPU-side checks of the case table ----------------------------------------------------------------------------------------
def test_plan_reaches_every_label_with_both_sq():
    """The restated dispatch at 256 CUs over the case lists: all seven labels, each with SQ off and on; every bin edge lands where
    it was written for; the refused shapes are refused."""
    ncu = CPU_TEST_CUS
    seen = set()
    cases = edge_cases() + old_cases() + [c for NT in PERSIST_M for c in persist_cases(NT, ncu)]
    for c in cases:
        p = plan_apply(c.sizes, c.n, ncu, c.reg, c.waves)
        assert p.label is not None, c.name()
        seen.add((p.label, c.sq))
    assert seen == {(l, sq) for l in ALL_LABELS for sq in (False, True)}, seen
    want = {1: 8, 15: 8, 16: 8, 17: 8, 127: 8, 128: 8, 129: 10, 130: 10, 156: 10, 160: 10, 161: 12, 182: 12, 192: 12, 193: 16, 234: 16,
            255: 16, 256: 16}
    for m in EDGE_MMAX:
        p = plan_apply(mixed_sizes(m), N_PLAIN, ncu)
        assert p.label == (REG_LABEL[want[m]] if m in want else OLD_LABEL[32]), (m, p)
    for m, TN in zip(OLD_MMAX, (64, 64, 32, 32, 16, 16, 16)):
        assert plan_apply(mixed_sizes(m), N_PLAIN, ncu, reg=False).label == OLD_LABEL[TN], m
    for NT, m in PERSIST_M.items():
        assert plan_apply([m], 1, ncu).NT == NT
    assert plan_apply([1121], N_PLAIN, ncu).label is None and plan_apply([1121], N_PLAIN, ncu, reg=False).label is None
    assert plan_apply([0, 0], N_PLAIN, ncu).label is None and plan_apply([5], 0, ncu).label is None
    for c in own_cases():                                        # the own NN kernel's conditions (gemm_nn_f64_supported)
        P = sum(c.sizes)
        assert P > 128 and cdiv(P, 256) * 256 <= 1.15 * P and c.n % 2 == 0 and OWN_NAO % 32 == 0
    assert {plan_apply(c.sizes, c.n, ncu).label for c in own_cases()} == set(REG_LABEL.values())
    # the mixed blocks: an empty block, one below a row tile, and (m = 33 under NT >= 8) a wave pair with both row tiles past m
    for m in EDGE_MMAX:
        s = mixed_sizes(m)
        assert max(s) == m and 0 in s and (m < 33 or {1, 7, 16, 33} <= set(s))


def test_persistent_cases_walk_the_loop():
    """Every persistent case makes at least 3 loop steps in every workgroup (the n = 1 cases are the single-tile edge and make
    one); the gx = 1 cases do so for any CU count up to 320, the gx = 2 cases have 2 or 3 workgroups per block and a last round
    that only some of them take."""
    for NT in PERSIST_M:
        for ncu in list(range(1, PERSIST_NBLK + 1)):
            for c in persist_cases(NT, ncu):
                if c.tag != 'gx1':
                    continue
                p = plan_apply(c.sizes, c.n, ncu, c.reg, c.waves)
                assert p.NT == NT and p.gx == 1 and len(c.sizes) == PERSIST_NBLK and 800 <= sum(c.sizes) <= 1000, (c.name(), p)
                assert p.steps_min == p.ntile == {5 * p.TN + 7: 6, 4 * p.TN: 4, 1: 1}[c.n], (c.name(), p)
        for ncu in (64, 80, 104, 110, 228, 256, 304):
            for c in persist_cases(NT, ncu):
                if c.tag != 'gx2':
                    continue
                p = plan_apply(c.sizes, c.n, ncu, c.reg, c.waves)
                assert p.NT == NT and p.gx in (2, 3) and p.ntile == 7 and p.steps_min >= 3, (c.name(), p)
                assert p.ntile % p.gx != 0 and p.steps_max == p.steps_min + 1


def test_exact_cases_stay_below_2_53():
    """The worst partial sum of every exact case, bounded by (terms) x max|a| x max|b|, is far below 2^53; the integer inverse
    pairs satisfy D Dinv == I in int64 and their substitution's partial sums stay below 2^53 as well."""
    lim = 2 ** 53
    cases = edge_cases() + old_cases() + own_cases() + [c for NT in PERSIST_M for c in persist_cases(NT, CPU_TEST_CUS)]
    assert max(apply_worst_partial_sum(c) for c in cases) < 2 ** 34 < lim
    assert max(FORWARD_SIZES) * 4 * 4 < lim and max(SUBST_SIZES) * 4 * 4 < lim        # |L| <= 4, |X_true| <= 4
    assert max(COMBINE_ROWS) * 4 * 4 + 4 < lim
    for (D, Dinv), m in zip(invert_blocks(), FORWARD_SIZES):
        assert D.shape == (m, m) and np.array_equal(D.dot(Dinv), np.eye(m, dtype=np.int64))
        assert np.array_equal(D, np.tril(D)) and np.array_equal(Dinv, np.tril(Dinv))
        assert m == 0 or (np.diag(D) == 1).all()
        assert m == 0 or int(np.abs(D).dot(np.abs(Dinv)).max()) < 2 ** 40 < lim
    ns = [c[0] for c in combine_cases()]
    assert set(ns) == set(range(1, 10)) and {(c[0], c[3]) for c in combine_cases()} == set(itertools.product(range(1, 10), (0, 1)))
    assert {(c[1], c[2], c[3]) for c in combine_cases()} >= set(itertools.product(COMBINE_ROWS, COMBINE_NG, (0, 1)))


# ---- device side ------------------------------------------------------------------------------------------------------------
SENTINEL = -777.25
PAD_ROWS = 2
D0 = 5                                             # first row / column of the diagonal sub-block view inside its matrix


@pytest.fixture(scope='module')
def be():
    from pyscf_isdf_amd.backend import HipBackend
    b = HipBackend(0)
    b.prof_enable(True)
    yield b
    b.prof_enable(False)
    b.prof_reset()
    for key, value in (('gemm_nn_own', 0), ('block_apply_reg', 1), ('block_apply_waves', DEFAULT_WAVES), ('trsm_substitution', 0)):
        b.set_option(key, value)
    b.release_workspace()


@pytest.fixture(scope='module')
def ncu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def _profiled(be, fn):
    be.prof_reset()
    fn()
    return be.prof_results()


def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


def _first_diff(got, ref):
    bad = np.argwhere(~(got == ref))
    i, j = bad[0]
    return '%d of %d entries differ, first at (%d, %d): got %r, exact %r' % (len(bad), ref.size, i, j, got[i, j], ref[i, j])


class _Rows:
    """A row-major operand that a kernel overwrites: the (nrow, ncol) window of a buffer with PAD_ROWS sentinel rows before and
    after it and ld = ncol + 3, the padding columns holding NaN, the sentinel, NaN."""

    def __init__(self, be, mat, ld=None):
        self.be = be
        self.nrow, self.ncol = mat.shape
        self.ld = self.ncol + 3 if ld is None else ld
        host = np.full((self.nrow + 2 * PAD_ROWS, self.ld), SENTINEL)
        host[:, self.ncol::2] = np.nan
        host[PAD_ROWS:PAD_ROWS + self.nrow, :self.ncol] = mat
        self.host = host
        self.dev = be.to_device(host)
        self.view = self.dev[PAD_ROWS:PAD_ROWS + self.nrow, :self.ncol]
        assert self.view.stride(0) == self.ld and self.view.stride(1) == 1

    def fetch(self):
        """(the window, whether everything around it is bit-unchanged)."""
        after = self.be.to_host(self.dev)
        win = after[PAD_ROWS:PAD_ROWS + self.nrow, :self.ncol].copy()
        before = self.host.copy()
        for buf in (after, before):
            buf[PAD_ROWS:PAD_ROWS + self.nrow, :self.ncol] = 0.0
        return win, _bits_equal(after, before)


def _embed_blocks(be, blocks, off, tail=TAIL_ROWS):
    """The (P + tail)^2 diagonal sub-block view, first element (D0, D0), of a NaN-filled device matrix with the blocks on its
    diagonal: (view, its leading dimension)."""
    P = int(off[-1]) + tail
    ld = P + D0 + 3
    big = np.full((ld, ld), np.nan)
    for b, blk in enumerate(blocks):
        o = D0 + int(off[b])
        big[o:o + blk.shape[0], o:o + blk.shape[0]] = blk
    dev = be.to_device(big)
    view = dev[D0:D0 + P, D0:D0 + P]
    assert view.stride(0) == ld > P
    return view, ld


class _ApplyRun:
    """One block-apply case on the device.  Dinv: per block np.tril of integers in [-3, 3] (Gaussian: the inverse of a Cholesky
    factor) inside the NaN-filled larger matrix; X (or, SQ, aoP and ao) as the case asks; rows [0, P) of the result window are the
    blocks', TAIL_ROWS more rows belong to the window and must stay as they are."""

    def __init__(self, be, c, rng, gaussian=False):
        self.be, self.c = be, c
        self.off = _offsets(c.sizes)
        self.P = P = int(self.off[-1])
        n = c.n
        if gaussian:
            self.blocks = []
            for m in c.sizes:
                M = rng.standard_normal((m, m))
                self.blocks.append(np.tril(np.linalg.inv(np.linalg.cholesky(M.dot(M.T) + m * np.eye(m)))) if m else np.zeros((0, 0)))
        else:
            self.blocks = [np.tril(_ints(rng, (m, m), 3)) for m in c.sizes]
        self.dD, self.ldd = _embed_blocks(be, [np.asarray(b, dtype=np.float64) for b in self.blocks], self.off)
        self.dD = self.dD[:P, :P] if c.sq else self.dD
        if c.sq:
            nao = OWN_NAO if c.own else NAO
            self.aoP = rng.standard_normal((P, nao)) if gaussian else _ints(rng, (P, nao), 2)
            self.ao = rng.standard_normal((nao, n)) if gaussian else _ints(rng, (nao, n), 2)
            self.d_aoP = be.to_device(np.asarray(self.aoP, dtype=np.float64))
            ld = n + 4 if c.own else n + 3                       # the own NN kernel wants 16-byte aligned rows
            ao_host = np.full((nao + 2, ld), np.nan)
            ao_host[1:1 + nao, :n] = self.ao
            self.d_ao = be.to_device(ao_host)[1:1 + nao]
            self.X0 = None
        else:
            self.X0 = rng.standard_normal((P, n)) if gaussian else _ints(rng, (P, n), 4)
        self.rows = None

    def launch(self):
        be, c = self.be, self.c
        if c.sq:
            start = np.full((self.P, c.n), np.nan)               # the product overwrites every entry
            self.rows = _Rows(be, start, ld=c.n + 4 if c.own else None)
        else:
            start = np.full((self.P + TAIL_ROWS, c.n), SENTINEL)
            start[:self.P] = self.X0
            self.rows = _Rows(be, start)
        be.set_option('block_apply_reg', int(c.reg))
        be.set_option('block_apply_waves', c.waves)
        be.set_option('gemm_nn_own', int(c.own))
        try:
            if c.sq:
                be.pair_rows_block_apply(self.d_aoP, self.d_ao, c.n, self.dD, self.off, self.rows.view)
            else:
                be.block_apply(self.dD, self.off, self.rows.view)
        finally:
            be.set_option('block_apply_reg', 1)
            be.set_option('block_apply_waves', DEFAULT_WAVES)
            be.set_option('gemm_nn_own', 0)

    def ref(self, cast=lambda x: np.asarray(x, dtype=np.int64)):
        """Dinv_b X_b per block (SQ: X = (aoP ao)^2) in the number type ``cast`` converts to."""
        if self.c.sq:
            X = cast(self.aoP).dot(cast(self.ao))
            X = X * X
        else:
            X = cast(self.X0)
        out = np.zeros(X.shape, dtype=X.dtype)
        for b, blk in enumerate(self.blocks):
            o, e = int(self.off[b]), int(self.off[b + 1])
            if e > o:
                out[o:e] = cast(blk).dot(X[o:e])
        return out

    def fetch(self, bad):
        win, clean = self.rows.fetch()
        if not clean:
            bad.append('sentinel or padding around the rows overwritten')
        if not self.c.sq and not _bits_equal(win[self.P:], np.full((TAIL_ROWS, self.c.n), SENTINEL)):
            bad.append('rows past blk_off[nblk] changed')
        return win[:self.P]

    def expected_labels(self, plan):
        c = self.c
        return sorted([plan.label] + ([NN_SQ] if c.own else [ROCBLAS_GEMM] if c.sq else []))


def _run_apply_exact(be, c, ncu, twice=False):
    plan = plan_apply(c.sizes, c.n, ncu, c.reg, c.waves)
    run = _ApplyRun(be, c, np.random.default_rng([len(c.sizes), max(c.sizes), c.n, int(c.sq), int(c.reg), c.waves]))
    bad = []
    prof = _profiled(be, run.launch)
    want = run.expected_labels(plan)
    if sorted(prof) != want:
        bad.append('ran %s, the restatement says %s' % (sorted(prof), want))
    elif prof[plan.label]['work'] != 16.0 * run.P * c.n or prof[plan.label]['launches'] != 1:
        bad.append('work %r in %d launch(es), expected 16 * %d * %d' % (prof[plan.label]['work'], prof[plan.label]['launches'], run.P, c.n))
    got = run.fetch(bad)
    ref = run.ref().astype(np.float64)
    if not np.array_equal(got, ref):
        bad.append(_first_diff(got, ref))
    if twice:
        run.launch()
        if not _bits_equal(got, run.fetch(bad)):
            bad.append('two runs on the same inputs differ')
    label = next((k for k in prof if k in ALL_LABELS), None)
    return label, plan, bad


def _report(title, fails, cover=None):
    print('\n' + title)
    for key in sorted(cover or {}, key=str):
        print('  %-44s %s' % (key, ', '.join(sorted(cover[key]))))
    for name, bad in fails:
        print('  FAILED %s: %s' % (name, '; '.join(bad)))


def _sweep_apply(be, ncu, cases, title, twice=False):
    fails, cover = [], {}
    for c in cases:
        label, plan, bad = _run_apply_exact(be, c, ncu, twice)
        if label is not None:
            cover.setdefault('%s SQ=%d' % (label, c.sq and not c.own), set()).add('%s %d' % (c.tag, max(c.sizes)))
        if bad:
            fails.append((c.name(), bad))
    _report('%s on %d CUs: %d cases' % (title, ncu, len(cases)), fails, cover)
    assert not fails, fails
    return set(cover)


@gpu
def test_block_apply_edges_exact(be, ncu):
    """Every mmax-side dispatch edge with the register form on, SQ off (isdf_block_apply) and on (isdf_pair_rows_block_apply),
    mixed blocks in every call: label and work against the restatement, the exact integer product, sentinels, NaN outside the
    blocks of Dinv and in the padding; the four register forms and the step to block_apply_mfma_kernel<32> are all seen."""
    seen = _sweep_apply(be, ncu, edge_cases(), 'block apply, dispatch edges')
    assert seen == {'%s SQ=%d' % (l, sq) for l in list(REG_LABEL.values()) + [OLD_LABEL[32]] for sq in (0, 1)}, seen


@gpu
def test_block_apply_older_kernel_exact(be, ncu):
    """block_apply_mfma_kernel<64 / 32 / 16> (option block_apply_reg 0) at both sides of its two tile-width edges, at 16 rows and
    at the largest blocks it takes (1100, 1120), SQ off and on."""
    seen = _sweep_apply(be, ncu, old_cases(), 'block apply, older kernel')
    assert seen == {'%s SQ=%d' % (l, sq) for l in OLD_LABEL.values() for sq in (0, 1)}, seen


@gpu
@pytest.mark.parametrize('NT', sorted(PERSIST_M))
def test_block_apply_persistent_loop_exact(be, ncu, NT):
    """One register form with block_apply_waves 1: gx = 1 (320 blocks) over 6 tiles with a ragged last one, exactly 4 tiles and a
    single column, gx = 2 over 7 tiles; SQ off and on; every case twice, bit-identical."""
    cases = persist_cases(NT, ncu)
    for c in cases:
        p = plan_apply(c.sizes, c.n, ncu, c.reg, c.waves)
        assert p.NT == NT and (p.gx == 1 if c.tag == 'gx1' else p.gx in (2, 3) and p.steps_max >= 3), (c.name(), p)
    seen = _sweep_apply(be, ncu, cases, 'block apply, persistent loop of NT = %d' % NT, twice=True)
    assert seen == {'%s SQ=%d' % (REG_LABEL[NT], sq) for sq in (0, 1)}, seen


@gpu
def test_block_apply_after_own_squared_product(be, ncu):
    """isdf_pair_rows_block_apply with option gemm_nn_own on operands the own NN kernel takes: gemm_nn_mfma_kernel<true> squares,
    the block apply (each register form once) runs with SQ off, the result is the same exact Dinv_b (aoP ao)^2."""
    seen = _sweep_apply(be, ncu, own_cases(), 'block apply after the own squared product')
    assert seen == {'%s SQ=0' % l for l in REG_LABEL.values()}, seen


@gpu
def test_block_apply_refusals_leave_x_unchanged(be, ncu):
    """1121 rows (both settings of block_apply_reg), all blocks empty, n = 0 and ldx < n: an error, no label, X bit-unchanged."""
    from pyscf_isdf_amd.lib import IsdfError
    rng = np.random.default_rng(3)
    fails = []

    def refused(name, sizes, n, call, reg=True):
        off = _offsets(sizes)
        P = max(int(off[-1]), 8)
        dD, _ = _embed_blocks(be, [np.tril(_ints(rng, (m, m), 3)).astype(np.float64) for m in sizes], off, tail=P - int(off[-1]))
        rows = _Rows(be, _ints(rng, (P, max(n, 4)), 4).astype(np.float64))
        be.set_option('block_apply_reg', int(reg))
        be.prof_reset()
        try:
            call(dD, off, rows)
            fails.append((name, ['the call was accepted']))
        except IsdfError:
            pass
        finally:
            be.set_option('block_apply_reg', 1)
        be.synchronize()
        if be.prof_results():
            fails.append((name, ['a refused call recorded %s' % sorted(be.prof_results())]))
        if not _bits_equal(be.to_host(rows.dev), rows.host):
            fails.append((name, ['X changed']))

    plain = lambda dD, off, rows: be.block_apply(dD, off, rows.view)
    assert plan_apply([1121], N_PLAIN, ncu).label is None
    refused('1121 rows', [1121], 40, plain)
    refused('1121 rows, reg = 0', [1121], 40, plain, reg=False)
    refused('all blocks empty', [0, 0, 0], 40, plain)
    refused('n = 0', [7, 16], 0, lambda dD, off, rows: be.block_apply(dD, off, rows.view[:, :0]))

    def short_ld(dD, off, rows):
        be._stream()
        be.handle.call('isdf_block_apply', be._p(dD), dD.stride(0), len(off) - 1, off.ctypes.data_as(ctypes.c_void_p),
                       be._p(rows.view), 40, 39)
    refused('ldx < n', [7, 16], 40, short_ld)
    _report('block apply refusals', fails)
    assert not fails, fails
    # and the handle still works after the refusals
    label, _, bad = _run_apply_exact(be, _case('after refusal', [33, 7], 40, False), ncu)
    assert label == REG_LABEL[8] and not bad, (label, bad)


# ---- rounding ---------------------------------------------------------------------------------------------------------------
# The smallest power of two at or above 4 x the largest device / numpy error ratio measured on an MI355X (module docstring); it may
# not exceed 64 whatever a later measurement says.
ROUNDING_FACTOR = 16.0
ROUNDING_CASES = [(REG_LABEL[8], 128, True), (REG_LABEL[10], 156, True), (REG_LABEL[12], 182, True), (REG_LABEL[16], 234, True),
                  (OLD_LABEL[64], 96, False), (OLD_LABEL[32], 288, False), (OLD_LABEL[16], 289, False)]


def _rel_err(x, ref):
    return float(abs(x.astype(np.longdouble) - ref).max() / abs(ref).max())


@gpu
@pytest.mark.parametrize('sq', [False, True])
@pytest.mark.parametrize('label,mmax,reg', ROUNDING_CASES)
def test_block_apply_rounding_against_longdouble(be, ncu, label, mmax, reg, sq):
    """Gaussian X (SQ: Gaussian aoP, ao) under the inverse of a Cholesky factor of M M^T + m I: the device's error against the
    np.longdouble triangular product may exceed the error of numpy's float64 product of the same inputs by ROUNDING_FACTOR."""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63
    c = _case('rounding', [33, mmax, 7], N_PLAIN, sq, reg=reg)
    plan = plan_apply(c.sizes, c.n, ncu, c.reg, c.waves)
    assert plan.label == label
    run = _ApplyRun(be, c, np.random.default_rng([mmax, int(sq), int(reg)]), gaussian=True)
    prof = _profiled(be, run.launch)
    assert sorted(prof) == run.expected_labels(plan), (sorted(prof), plan)
    bad = []
    got = run.fetch(bad)
    assert not bad, bad
    ref = run.ref(lambda x: np.asarray(x, dtype=np.longdouble))
    f64 = run.ref(lambda x: np.asarray(x, dtype=np.float64))
    dev, host = _rel_err(got, ref), _rel_err(f64, ref)
    print('rounding %-36s SQ=%d mmax %d: device %.2e, numpy %.2e, ratio %.2f' % (label, sq, mmax, dev, host, dev / host))
    assert np.isfinite(got).all() and host > 0.0
    assert dev <= ROUNDING_FACTOR * host, (label, sq, dev, host, dev / host)


# ---- forward solve, inverse, substitution -----------------------------------------------------------------------------------
def _nan_upper(L):
    """The factor as the device sees it: NaN above the diagonal."""
    out = np.asarray(L, dtype=np.float64).copy()
    out[np.triu_indices(out.shape[0], 1)] = np.nan
    return out


def _solve_case(be, sizes, n, side, trans, seed):
    """isdf_block_solve on integer factors: returns (labels, got, X_true, clean).  side 0: X (P + tail, n), side 1: X (n, P + tail),
    the tail rows / columns past blk_off[nblk] hold the sentinel."""
    rng = np.random.default_rng([seed, n, side, trans])
    off = _offsets(sizes)
    P = int(off[-1])
    Ls = [int_factor(rng, m) for m in sizes]
    dD, _ = _embed_blocks(be, [_nan_upper(L) for L in Ls], off)
    Xt = _ints(rng, (P, n), 4)
    B = np.zeros((P, n), dtype=np.int64)
    for b, L in enumerate(Ls):
        o, e = int(off[b]), int(off[b + 1])
        # side 0: op(L) x = b per column; side 1 solves x^T op(L) = b^T, i.e. op(L)^T x = b
        op = L.T if (trans != 0) != (side == 1) else L
        B[o:e] = op.dot(Xt[o:e])
    start = np.full((P + TAIL_ROWS, n), SENTINEL)
    start[:P] = B
    rows = _Rows(be, start if side == 0 else np.ascontiguousarray(start.T))
    prof = _profiled(be, lambda: be.block_solve(dD, off, side, trans, rows.view))
    win, clean = rows.fetch()
    win = win if side == 0 else win.T
    clean = clean and _bits_equal(win[P:], np.full((TAIL_ROWS, n), SENTINEL))
    return sorted(prof), win[:P], Xt.astype(np.float64), clean


@gpu
def test_block_forward_solve_exact(be):
    """block_forward_kernel through isdf_block_solve(side 0, trans 0): blocks of 1, 63, 0, 64, 65, 128, 129 and 200 rows in one
    call, n in {1, 255, 256, 257}, integer factors with NaN above the diagonal and outside the blocks, B = L X_true in int64: the
    device returns X_true exactly; ldx padding, the rows before and the rows past blk_off[nblk] < P bit-unchanged."""
    fails = []
    for n in FORWARD_N:
        labels, got, Xt, clean = _solve_case(be, FORWARD_SIZES, n, 0, 0, 21)
        bad = [] if labels == [FORWARD] else ['ran %s, expected %s' % (labels, FORWARD)]
        if not clean:
            bad.append('sentinel or padding around X overwritten')
        if not np.array_equal(got, Xt):
            bad.append(_first_diff(got, Xt))
        if bad:
            fails.append(('n = %d' % n, bad))
    _report('block forward solve: %d cases' % len(FORWARD_N), fails)
    assert not fails, fails


@gpu
def test_block_invert_exact(be):
    """isdf_block_invert on integer unit-diagonal factors with a known integer inverse: bit equality with blockdiag(D_b^-1), the
    exact zeros above the diagonal and outside the blocks included; rows past blk_off[nblk] keep the identity."""
    pairs = invert_blocks()
    off = _offsets(FORWARD_SIZES)
    P = int(off[-1]) + TAIL_ROWS
    D = np.full((P, P), np.nan)
    want = np.eye(P)
    for b, (Db, Dib) in enumerate(pairs):
        o, e = int(off[b]), int(off[b + 1])
        D[o:e, o:e] = _nan_upper(Db)
        want[o:e, o:e] = Dib
    dD = be.to_device(D)
    dI = be.to_device(np.full((P, P), np.nan))
    prof = _profiled(be, lambda: be.block_invert(dD, off, dI))
    got = be.to_host(dI)
    assert sorted(prof) == [FORWARD], sorted(prof)
    assert np.array_equal(got, want), _first_diff(got, want)
    assert _bits_equal(got, want)                             # no negative zeros either


@gpu
@pytest.mark.parametrize('side,trans', [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_substitution_solve_exact(be, side, trans):
    """Option trsm_substitution: subst_kernel<false / true>, the rocBLAS updates between the 64-row blocks and 512-row panels and
    (side 1) transpose_kernel, blocks of 1, 64, 0, 65, 512, 513 and 577 rows, n = 37 with a row stride: X_true exactly."""
    be.set_option('trsm_substitution', 1)
    try:
        labels, got, Xt, clean = _solve_case(be, SUBST_SIZES, SUBST_N, side, trans, 31)
    finally:
        be.set_option('trsm_substitution', 0)
    kernel = SUBST[(trans != 0) != (side == 1)]                # a right-sided solve is the left-sided one of the other op on X^T
    assert labels == sorted([kernel, ROCBLAS_GEMM]), labels
    assert clean, 'sentinel or padding around X overwritten'
    assert np.array_equal(got, Xt), _first_diff(got, Xt)


# ---- skinny rows ------------------------------------------------------------------------------------------------------------
@gpu
def test_rows_combine_exact(be):
    """isdf_rows_combine on integers: n in 1..8 through skinny_rows_kernel, n = 9 through rocBLAS, rows in {1, 63, 64, 65, 129},
    ng in {1, 255, 256, 257, 700}, E a column slice of a wider NaN-filled matrix, Y with NaN in its padding, both values of
    accumulate, the sentinel in the ldf padding and around F."""
    fails = []
    for n, rows, ng, acc in combine_cases():
        rng = np.random.default_rng([n, rows, ng, acc])
        E, Y, F0 = _ints(rng, (n, rows), 4), _ints(rng, (rows, ng), 4), _ints(rng, (n, ng), 4)
        wide = np.full((n, rows + 5), np.nan)
        wide[:, 3:3 + rows] = E
        dE = be.to_device(wide)[:, 3:3 + rows]
        ypad = np.full((rows + 1, ng + 2), np.nan)
        ypad[:rows, :ng] = Y
        dY = be.to_device(ypad)[:rows, :ng]
        out = _Rows(be, F0.astype(np.float64) if acc else np.full((n, ng), np.nan))
        prof = _profiled(be, lambda: be.rows_combine(dE, dY, out.view, accumulate=bool(acc)))
        got, clean = out.fetch()
        ref = (E.dot(Y) + (F0 if acc else 0)).astype(np.float64)
        want = ROCBLAS_GEMM if n > 8 else SKINNY
        bad = [] if sorted(prof) == [want] else ['ran %s, expected %s' % (sorted(prof), want)]
        if not clean:
            bad.append('sentinel or padding around F overwritten')
        if not np.array_equal(got, ref):
            bad.append(_first_diff(got, ref))
        if bad:
            fails.append(('n=%d rows=%d ng=%d accumulate=%d' % (n, rows, ng, acc), bad))
    _report('rows combine: %d cases' % len(combine_cases()), fails)
    assert not fails, fails
