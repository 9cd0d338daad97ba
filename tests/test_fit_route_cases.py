"""CPU-side checks of the case table of the fit route sweep (fit_route_cases.py): what test_gpu_fit_route_sweep.py takes for granted
when it compares the device with np.array_equal."""
import numpy as np
import pytest

import fit_route_cases as fc
from test_gpu_fit_solve_sweep import int_unit_pair

LIMIT = fc.LIMIT


def test_exact_dot_is_the_int64_product():
    rng = np.random.default_rng(1)
    for shape in ((1, 1, 1), (65, 130, 37), (200, 200, 9)):
        a, b = fc.ints(rng, shape[:2], 4), fc.ints(rng, shape[1:], 4)
        got = fc.exact_dot(a, b)
        assert got.dtype == np.float64 and np.array_equal(got, a.dot(b))
    with pytest.raises(AssertionError):
        fc.exact_dot(np.full((1, 2), 2.0 ** 27), np.full((2, 1), 2.0 ** 26))


def test_gram_references_stay_below_2_53():
    """Bounds of every partial sum of sections A and B (entries in [-3, 3]), and the references really reach no further."""
    worst = max([fc.gram_bound(fc.GRAM_NAO, 3), fc.gram_bound(2 * max(fc.GRAM_NH), 3, cplx=True), fc.gram_bound(32, 3),
                 fc.gram_bound(2 * fc.CPLX_NH, 3, cplx=True), fc.gram_bound(fc.PROD_NAO, 3, max(fc.PROD_NOCC), 3),
                 fc.gram_bound(2 * fc.CPLX_NH, 3, 2 * 2, 3, cplx=True)])
    assert worst < 2 ** 20 < LIMIT
    rng = np.random.default_rng(2)
    aoP, ao = fc.complex_operands(rng, 37, fc.CPLX_NH, 300)
    assert abs(fc.pair_rows_ref(aoP, ao, fc.CPLX_NH)).max() <= fc.gram_bound(2 * fc.CPLX_NH, 3, cplx=True)
    assert abs(fc.gram_sq_ref(aoP, fc.CPLX_NH)).max() <= fc.gram_bound(2 * fc.CPLX_NH, 3, cplx=True)


@pytest.mark.parametrize('nh', fc.GRAM_NH)
def test_rot_sign_shows_in_the_integer_result(nh):
    """(aoP aoP^T)^2 + (rot aoP^T)^2 with rot = [Im | -Re]: [Im | Re] gives another integer matrix on the inputs of the sweep, for
    every P (at P = 1 the only entry gains (2 Re . Im)^2 under the wrong sign, which row 0 of the operand keeps away from 0)."""
    for P in fc.GRAM_P:
        aoP = fc.gram_sq_operand(P, nh)
        good, wrong = fc.gram_sq_ref(aoP, nh), fc.gram_sq_ref(aoP, nh, wrong_sign=True)
        assert np.array_equal(good, good.T)
        assert not np.array_equal(good, wrong), (P, nh)
        assert np.array_equal(fc.gram_sq_ref(aoP, nh).diagonal(), (aoP * aoP).sum(axis=1) ** 2)   # Im S has a zero diagonal


def test_integer_factors_have_the_stated_inverse():
    """L Linv = I exactly for every factor of the solve cases; L is lower triangular with diagonal in {1, 2, 4}; the worst
    partial sum of L X_true, of the substitution and of L W L^T stays below 2^53."""
    for P in sorted(set(fc.SOLVE_P + fc.W_P + fc.CHOL_P)):
        for seed in ((0,) if P in fc.SOLVE_P + fc.W_P else ()) + ((1,) if P in fc.CHOL_P else ()):      # solves: 0, healthy_matrix: 1
            L, Linv = fc.factor_pair(P, seed)
            assert np.array_equal(L, np.tril(L)) and np.array_equal(Linv, np.tril(Linv)) and np.array_equal(L, np.rint(L))
            assert set(np.unique(L.diagonal())) <= {1.0, 2.0, 4.0}
            # |L| |Linv| below 2^53 / 4: Linv holds multiples of 1/4, so 4 L Linv is an integer product with the same bound
            assert np.array_equal(4 * Linv, np.rint(4 * Linv))
            assert np.array_equal(fc.exact_dot(L, 4 * Linv), 4 * np.eye(P))
            assert abs(L).max() <= 64 and abs(Linv).max() <= 4096
            # X_true in [-4, 4]: |L| 4 summed over a row; two-sided: |L| |W| |L|^T with |W| <= 4
            row = abs(L).sum(axis=1).max()
            assert 4 * row * row < 2 ** 40 < LIMIT
    for P in (1, 2, 65, 200):                                   # the same construction as the solve sweep's builder
        D, Dinv = fc.unit_pair(np.random.default_rng(P), P)
        D0, D0inv = int_unit_pair(np.random.default_rng(P), P)
        assert np.array_equal(D, D0) and np.array_equal(Dinv, D0inv)
    for sizes in {sizes for _, sizes in fc.PROBE_CASES}:        # isdf_bj_probe_vectors: the factor (seed 0) and the blocks (seed 2)
        for P, seed in [(sum(sizes), 0)] + [(m, 2) for m in sizes if m]:
            L, Linv = fc.factor_pair(P, seed)
            assert np.array_equal(fc.exact_dot(L, 4 * Linv), 4 * np.eye(P)) and np.array_equal(L, np.tril(L))
            assert 4 * abs(L).sum(axis=1).max() ** 3 < 2 ** 45 < LIMIT                 # E L L^T D^T with |E| <= 4
    L, Linv = fc.bidiagonal_factor(np.random.default_rng(4), 40)
    assert np.array_equal(L.dot(Linv), np.eye(40, dtype=np.int64)) and abs(Linv).max() == 1
    assert np.array_equal(np.abs(np.tril(L, -1)).sum(axis=1)[1:], np.ones(39, dtype=np.int64))


def test_fit_apply_and_from_chol_cases_are_integers():
    for ng in fc.APPLY_NG:
        for nh in (0,):
            c = fc.apply_case(ng, nh)
            assert np.array_equal(c['L'].dot(c['Y']), c['B']) and np.array_equal(c['L'].T.dot(c['Theta']), c['Y'])
            # |Linv| = 1 on the lower triangle: every partial sum is below P max|B| (P^2 max|B| for Theta)
            assert fc.APPLY_P ** 2 * int(abs(c['B']).max()) < 2 ** 30 < LIMIT
    for k, m in fc.FROM_CHOL:
        c = fc.from_chol_case(k, m)
        T = c['L'][:, c['piv']]
        assert np.array_equal(T, np.triu(T)) and (T.diagonal() == 1).all() and np.array_equal(T, c['T'])
        assert np.array_equal(T.dot(c['Theta']), c['L']) and np.array_equal(c['Theta'][:, c['piv']], np.eye(k, dtype=np.int64))
        assert len(set(c['piv'].tolist())) == k and k * 3 * k < LIMIT


def test_singular_case_fails_at_rung_0_and_passes_at_1e_14():
    c = fc.singular_case()
    A, md = c['A'], c['maxdiag']
    assert A[0, 0] == A[0, 1] == A[1, 1] == 16 and np.array_equal(c['ao'][:, c['ip']], c['aoP'].T)
    assert len(set(c['ip'].tolist())) == fc.SING_P and abs(c['aoP']).max() <= 2
    keep = [0] + list(range(2, fc.SING_P))
    assert np.linalg.cond(A[np.ix_(keep, keep)].astype(np.float64)) < 1e4          # well conditioned without the duplicate
    with pytest.raises(np.linalg.LinAlgError):
        np.linalg.cholesky(A.astype(np.float64))
    piv = np.linalg.cholesky(fc.shifted(A, 1e-14, md)).diagonal() ** 2 / md
    assert piv.argmin() == 1 and 1.5e-14 < piv[1] < 2.5e-14, piv[:3]
    piv = np.linalg.cholesky(fc.shifted(A, 1e-10, md)).diagonal() ** 2 / md
    assert piv.argmin() == 1 and 1.9e-10 < piv[1] < 2.1e-10
    # the failure exit: diag(1, -1, 1, 1, 1) is indefinite at every rung up to 1e-8
    with pytest.raises(np.linalg.LinAlgError):
        np.linalg.cholesky(np.diag([1.0, -1.0, 1.0, 1.0, 1.0]) + 1e-8 * np.eye(5))


def test_healthy_matrices_are_exact_integers():
    for P in fc.CHOL_P:
        A, L0 = fc.healthy_matrix(P)
        assert np.array_equal(A, A.T) and np.array_equal(A, np.rint(A)) and abs(A).max() < 2 ** 30
        assert (L0.diagonal() > 0).all()


def _enumerate_walk(m, n, sizes, up):
    """The gemm_rm calls of a walk by direct enumeration: the rows are solved 64, 512 or 1024 at a time (sizes, innermost
    first: a block of a level never crosses a boundary of the level above, and every level counts from row 0 of its parent);
    whenever a group of rows at some level starts on rows that the same parent has finished, one product couples the two."""
    calls = []

    def solve(lo, hi, level):                                  # rows [lo, hi) with everything outside the parent done
        if level < 0:
            return
        nb = sizes[level]
        starts = list(range(lo, hi, nb))
        finished = []
        for j0 in (starts if up else starts[::-1]):
            rows = list(range(j0, min(hi, j0 + nb)))
            if finished:
                calls.append(2 * len(rows) * n * len(finished))
            solve(rows[0], rows[-1] + 1, level - 1)
            finished += rows
    solve(0, m, len(sizes) - 1)
    return len(calls), sum(calls)


def test_walk_gemms_is_the_enumeration_of_the_blocks():
    """walk_gemms / solve_gemms against the enumeration above on every shape of the solve sweeps, both directions: cdiv(P, 1024)
    - 1 products per pass on the default path, cdiv(P, 64) - 1 under trsm_substitution (64 divides 512), and the flop of a pass
    is 2 n times the sum over pairs of blocks of the product of their sizes - the same upwards and downwards."""
    for P in sorted(set(fc.SOLVE_P + fc.W_P)):
        for n in fc.SOLVE_N + (P,):
            for up in (True, False):
                plain = fc.walk_gemms(P, n, fc.TRSM_NB, up)
                assert plain == _enumerate_walk(P, n, (fc.TRSM_NB,), up) and plain[0] == fc.cdiv(P, fc.TRSM_NB) - 1
                sub = fc.walk_gemms(P, n, fc.SUBST_PANEL, up, fc.SUBST_BLOCK)
                assert sub == _enumerate_walk(P, n, (fc.SUBST_BLOCK, fc.SUBST_PANEL), up)
                assert sub[0] == fc.cdiv(P, fc.SUBST_BLOCK) - 1
                sizes = [rows for _, rows in fc.chunks(P, fc.TRSM_NB)]
                pairs = sum(a * b for i, a in enumerate(sizes) for b in sizes[i + 1:])
                assert plain[1] == 2 * n * pairs
            for subst in (0, 1):
                got = fc.solve_gemms(P, n, (True, False), subst)
                nb = (fc.SUBST_PANEL, fc.SUBST_BLOCK) if subst else (fc.TRSM_NB, None)
                both = [fc.walk_gemms(P, n, nb[0], up, nb[1]) for up in (True, False)]
                assert got == dict(launches=both[0][0] + both[1][0], work=float(both[0][1] + both[1][1]))
                assert got['work'] < LIMIT
    assert fc.walk_gemms(2049, 37, fc.TRSM_NB, True) == (2, 2 * 37 * (1024 * 1024 + 2048 * 1))
    assert fc.walk_gemms(2049, 37, fc.TRSM_NB, False) == (2, 2 * 37 * (1024 * 1 + 1024 * 1025))
    assert fc.walk_gemms(1024, 37, fc.TRSM_NB, True) == (0, 0) and fc.walk_gemms(65, 1, 512, False, 64) == (1, 2 * 64)


def _straddles(values, edge):
    return edge in values and any(v < edge for v in values) and any(v > edge for v in values)


def test_case_lists_straddle_every_chunk_edge():
    assert _straddles(fc.CPLX_NG, fc.CPLX_CHUNK) and _straddles(fc.CPLX_NG, 2 * fc.CPLX_CHUNK)
    assert [len(fc.chunks(ng, fc.CPLX_CHUNK)) for ng in fc.CPLX_NG] == [1, 1, 1, 2, 2, 3]
    for P in fc.PROD_ROWS_P:
        ch = fc.prod_chunk(P)
        assert ch == 65536
        assert _straddles(fc.PROD_ROWS_NG, ch) and max(fc.PROD_ROWS_NG) > 2 * ch
        assert [len(fc.chunks(ng, ch)) for ng in fc.PROD_ROWS_NG] == [1, 1, 2, 3]
    assert fc.prod_chunk(1) == 65536 and fc.prod_chunk(4096) == 65536 and fc.prod_chunk(4097) == 65280
    assert fc.prod_chunk(65535) == 4096 and fc.prod_chunk(1 << 20) == 1024
    for edge in (fc.SUBST_BLOCK, fc.SUBST_PANEL, fc.TRSM_NB):
        assert _straddles(fc.SOLVE_P, edge)
    assert max(fc.SOLVE_P) > 2 * fc.TRSM_NB and fc.trsm_calls(2049) == 3 and fc.trsm_calls(1024) == 1
    assert min(fc.W_P) < fc.SUBST_BLOCK < 65 in fc.W_P and 513 in fc.W_P and fc.TRSM_NB + 1 in fc.W_P    # one row past each edge
    for values in (fc.GATHER_P, fc.GATHER_T_K, fc.GRAM_P + (255,)):
        assert _straddles(values, 256)                          # the 256-lane blocks of the gather and square kernels
    for ng in (1, 8191, 8192, 8193):
        assert sum(n for _, n in fc.chunks(ng, fc.CPLX_CHUNK)) == ng
