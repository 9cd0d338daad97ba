"""Case builders and exact references of the Cholesky fit route sweep (test_gpu_fit_route_sweep.py).  Plain numpy, no GPU import:
test_fit_route_cases.py checks in the CPU suite what the GPU module takes for granted - that every exact reference is an integer
below 2^53 in every partial sum, that every integer factor has the stated inverse, that the singular matrix is singular in the
way the ladder tests need, and that the case lists straddle every chunk edge of the restated host dispatch.

Exact references are int64 numpy.  The one exception is the product with a factor of up to 2049 rows, where numpy's int64 matmul
takes seconds: exact_dot runs it in float64 after bounding |a| |b| (a sum of non-negative terms is monotone, so a final value below
2^53 bounds every partial sum in any order, and a float64 sum of integers below 2^53 is exact); the CPU suite checks it against the
int64 product.
"""
import functools
import numpy as np
from test_gpu_fit_solve_sweep import _ints as ints, cdiv

LIMIT = 2 ** 53

# ---- restatement of the host-side chunking (csrc/fit.hip) -------------------------------------------------------------------
CPLX_CHUNK = 8192                                   # pair_rows (isdf_fit_apply_cplx, isdf_pair_gram_rows), nh > 0: columns per pass
TRSM_NB = 1024                                      # TRSM_NB of trsm.hip: rows per block of blocked_walk under tri_left / tri_right
SUBST_PANEL, SUBST_BLOCK = 512, 64                  # trsm_lower_left: rows per panel of blocked_walk, per block of the walk inside it


def prod_chunk(P):
    """Columns per pass of isdf_pair_prod_rows (rows per pass of isdf_gram_prod)."""
    ch = (1 << 28) // max(P, 1)
    ch = max(1024, min(65536, ch))
    return ch // 256 * 256


def chunks(n, ch):
    """(start, length) of every pass of a loop over n in pieces of ch."""
    return [(c0, min(ch, n - c0)) for c0 in range(0, n, ch)]


def trsm_calls(P, two_sided=False):
    """rocblas_dtrsm calls of one tri_left / tri_right on P rows (default path): one per block of TRSM_NB rows."""
    return cdiv(P, TRSM_NB) * (2 if two_sided else 1)


def walk_gemms(m, n, nb, up, inner=None):
    """(count, summed flop) of the gemm_rm calls of one blocked_walk (csrc/trsm.hip) over m rows with n right-hand sides: blocks
    of nb from row 0, taken upwards (up: L^-1 X, X L^-T) or downwards (L^-T X, X L^-1); every block but the first taken is
    updated from all finished rows in one product of 2 (its rows) n (the finished rows) flop.  inner: the block's diagonal solve
    is itself a walk over blocks of `inner` rows in the same direction (trsm_lower_left)."""
    count, flop = 0, 0
    for j0, rows in chunks(m, nb):
        done = j0 if up else m - (j0 + rows)
        if done > 0:
            count, flop = count + 1, flop + 2 * rows * n * done
        if inner:
            c, f = walk_gemms(rows, n, inner, up)
            count, flop = count + c, flop + f
    return count, flop


def solve_gemms(P, n, ups, subst):
    """rocblas_dgemm[flop] as dict(launches, work) of the walks of one call on a P-row factor, one walk per entry of ups (its
    direction): tri_left / tri_right on the default path, their substitution twins (a right-sided solve is the left-sided one
    of the other op on the transpose: same direction, same products) under trsm_substitution."""
    nb, inner = (SUBST_PANEL, SUBST_BLOCK) if subst else (TRSM_NB, None)
    walks = [walk_gemms(P, n, nb, up, inner) for up in ups]
    return dict(launches=sum(c for c, _ in walks), work=float(sum(f for _, f in walks)))


# ---- the case lists ---------------------------------------------------------------------------------------------------------
GATHER_P = (1, 255, 256, 257)
GATHER_NAO = (1, 9, 300)
GATHER_NG = 300
GATHER_T_K = (1, 255, 256, 257)
GRAM_P = (1, 37, 256, 257)
GRAM_NH = (1, 5)
GRAM_NAO = 9
ROWS_REAL = ((256, 32), (37, 9))                    # (P, nao): the own NN kernel takes the first and refuses the second
ROWS_REAL_NG = 70
CPLX_P = (3, 37)
CPLX_NH = 5
CPLX_NG = (1, 8191, 8192, 8193, 16384, 16385 + 7)
PROD_P = (1, 37, 257)
PROD_NOCC = (1, 4)
PROD_ROWS_P = (2, 37)
PROD_ROWS_NG = (65535, 65536, 65537, 131072 + 5)
PROD_NAO = 5
SOLVE_P = (1, 63, 64, 65, 512, 513, 1024, 1025, 2049)
SOLVE_N = (1, 37, 257)
W_P = (1, 65, 513, 1025)
FROM_CHOL = tuple((k, m) for k in (1, 64, 65) for m in (k, 700))
PROBE_CASES = tuple((n, sizes) for n in (1, 8) for sizes in ((10, 0, 16, 11), (130, 470)))
APPLY_P, APPLY_NAO, APPLY_NG = 40, 9, (1, 255, 300)
CHOL_P = (1, 64, 65, 257, 1025)
SING_P, SING_NAO, SING_NG, SING_SEED = 40, 9, 50, 3


def exact_dot(a, b):
    """a b for integer a, b, computed in float64 and proven exact (module docstring); float64 holding integers."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    bound = float(np.abs(a).dot(np.abs(b)).max()) if a.size and b.size else 0.0
    assert bound < LIMIT, bound
    return a.dot(b)


def index_list(rng, P, ng):
    """P grid indices: unsorted, with repeats (from P = 3 on), containing 0 and ng - 1 (from P = 2 on)."""
    ip = rng.integers(0, ng, size=P)
    if P >= 2:
        ip[P // 2], ip[0] = 0, ng - 1
    if P >= 3:
        ip[-1] = ip[0]
    return ip.astype(np.int64)


# ---- integer factors --------------------------------------------------------------------------------------------------------
def unit_pair(rng, m):
    """(D, Dinv) as float64 integers, lower triangular with unit diagonal, D Dinv = I: the construction of int_unit_pair of
    test_gpu_fit_solve_sweep.py, D = (I + N1) S (I + N2) with N1^2 = N2^2 = 0 and S = I + a sub-diagonal of signs, without its
    O(m^2) Python loop and int64 m^3 products (which take a minute at 2049 rows)."""
    eye = np.eye(m)
    if m <= 1:
        return eye.copy(), eye.copy()

    def nil(h):
        N = np.zeros((m, m))
        blk = ints(rng, (m - h, h), 2).astype(np.float64)
        blk[rng.random((m - h, h)) < 0.7] = 0
        N[h:, :h] = blk
        return N
    N1, N2 = nil(max(1, m // 3)), nil(max(1, (2 * m) // 3))
    s = rng.choice(np.array([-1.0, 1.0]), size=m - 1)
    c = np.concatenate([[1.0], np.cumprod(-s)])             # S^-1[i, j] = (-s_j+1) ... (-s_i) = c_i c_j for i >= j
    S = eye + np.diag(s, -1)
    Sinv = np.tril(np.outer(c, c))
    D = exact_dot(exact_dot(eye + N1, S), eye + N2)
    Dinv = exact_dot(exact_dot(eye - N2, Sinv), eye - N1)
    return D, Dinv


@functools.lru_cache(maxsize=None)
def factor_pair(P, seed=0, unit=False):
    """(L, Linv): L = D diag(d) integer lower triangular with diagonal d in {1, 2, 4} (unit: all 1), Linv = diag(1 / d) Dinv
    its exact inverse, whose entries are small dyadic numbers.  Cached: the arrays are shared and must not be written."""
    rng = np.random.default_rng([P, seed, 77])
    D, Dinv = unit_pair(rng, P)
    d = np.ones(P) if unit else rng.choice(np.array([1.0, 2.0, 4.0]), size=P)
    L, Linv = D * d[None, :], Dinv / d[:, None]
    for a in (L, Linv):
        a.setflags(write=False)
    return L, Linv


def bidiagonal_factor(rng, P):
    """Unit lower bidiagonal integer factor with +-1 below the diagonal, and its (integer, +-1 lower triangle) inverse."""
    s = rng.choice(np.array([-1, 1]), size=max(P - 1, 0)).astype(np.int64)
    c = np.concatenate([[1], np.cumprod(-s)]).astype(np.int64)
    return np.eye(P, dtype=np.int64) + np.diag(s, -1), np.tril(np.outer(c, c))


def nan_upper(L):
    """The factor as the device gets it: NaN above the diagonal."""
    out = np.array(L, dtype=np.float64)
    out[np.triu_indices(out.shape[0], 1)] = np.nan
    return out


# ---- Gram references (int64) --------------------------------------------------------------------------------------------------
def rot(x, nh, wrong_sign=False):
    """[Im | -Re] of rows stored [Re | Im] (wrong_sign: [Im | Re], for the CPU suite's check that the sign shows)."""
    return np.concatenate([x[:, nh:], x[:, :nh] if wrong_sign else -x[:, :nh]], axis=1)


def gram_sq_ref(aoP, nh=0, wrong_sign=False):
    S = aoP.dot(aoP.T)
    if nh == 0:
        return S * S
    T = rot(aoP, nh, wrong_sign).dot(aoP.T)
    return S * S + T * T


def pair_rows_ref(aoP, ao, nh=0):
    S = aoP.dot(ao)
    if nh == 0:
        return S * S
    T = rot(aoP, nh).dot(ao)
    return S * S + T * T


def gram_prod_ref(aoP, psiP):
    return aoP.dot(aoP.T) * psiP.dot(psiP.T)


def pair_prod_rows_ref(aoP, psiP, ao, psi):
    return aoP.dot(ao) * psiP.dot(psi)


def gram_prod_cplx_ref(aoP, nh, psiP, npsi_h):
    return aoP.dot(aoP.T) * psiP.dot(psiP.T) + rot(aoP, nh).dot(aoP.T) * rot(psiP, npsi_h).dot(psiP.T)


def pair_prod_rows_cplx_ref(aoP, nh, psiP, npsi_h, ao, psi):
    return aoP.dot(ao) * psiP.dot(psi) + rot(aoP, nh).dot(ao) * rot(psiP, npsi_h).dot(psi)


def gram_bound(nao, amax, nocc=None, pmax=None, cplx=False):
    """Upper bound of any partial sum on the way to a Gram entry: |S| <= nao amax^2, squared (or times the second factor's
    bound), twice that in complex mode."""
    s = nao * amax * amax
    t = s if nocc is None else nocc * pmax * pmax
    return s * t * (2 if cplx else 1)


def complex_operands(rng, P, nh, ng, amax=3):
    """(aoP (P, 2 nh), ao (2 nh, ng)) integers stored [Re | Im] / [Re; Im]."""
    return ints(rng, (P, 2 * nh), amax), ints(rng, (2 * nh, ng), amax)


def gram_sq_operand(P, nh, nao=GRAM_NAO):
    """The aoP of a Gram case: (P, 2 nh) stored [Re | Im] (nh = 0: (P, nao) real).  Row 0 starts with Re = 2, Im = 3, so that
    even the single entry of P = 1 tells [Im | -Re] from [Im | Re]."""
    rng = np.random.default_rng([P, nh, 5])
    aoP = ints(rng, (P, 2 * nh if nh else nao), 3)
    if nh:
        aoP[0, 0], aoP[0, nh] = 2, 3
    return aoP


# ---- fit_apply on integers ----------------------------------------------------------------------------------------------------
def apply_case(ng, nh=0, P=APPLY_P, nao=APPLY_NAO, seed=3):
    """Integer aoP, ao in [-2, 2] and a unit bidiagonal factor: B = pair rows, Y = L^-1 B, Theta = L^-T Y, all int64."""
    rng = np.random.default_rng([seed, ng, nh, P])
    aoP, ao = ints(rng, (P, nao), 2), ints(rng, (nao, ng), 2)
    L, Linv = bidiagonal_factor(rng, P)
    B = pair_rows_ref(aoP, ao, nh)
    Y = Linv.dot(B)
    return dict(aoP=aoP, ao=ao, L=L, Linv=Linv, B=B, Y=Y, Theta=Linv.T.dot(Y))


# ---- fit_from_chol on integers ------------------------------------------------------------------------------------------------
def from_chol_case(k, m, seed=9):
    """Integer rows L (k, m) whose pivot columns form a unit upper triangular T: Theta = T^-1 L is an integer matrix with the
    identity at the pivot columns.  T = U^T for a unit lower pair (U, Uinv), so T^-1 = Uinv^T."""
    rng = np.random.default_rng([seed, k, m])
    U, Uinv = bidiagonal_factor(rng, k)
    piv = rng.permutation(m)[:k].astype(np.int64)
    L = ints(rng, (k, m), 3)
    L[:, piv] = U.T
    return dict(L=L, piv=piv, T=U.T, Theta=Uinv.T.dot(L))


# ---- the exactly singular Gram matrix -----------------------------------------------------------------------------------------
def singular_case(seed=SING_SEED, P=SING_P, nao=SING_NAO, ng=SING_NG):
    """Integer aoP in [-2, 2] with rows 0 and 1 both (1, 1, 1, 1, 0, ...): A = (aoP aoP^T)^2 has A00 = A01 = A11 = 16, so the
    second pivot is 16 - 16 = 0 in any arithmetic order.  ao (nao, ng) carries the rows at the (distinct) columns ip."""
    rng = np.random.default_rng(seed)
    aoP = ints(rng, (P, nao), 2)
    aoP[0] = 0
    aoP[0, :4] = 1
    aoP[1] = aoP[0]
    ip = rng.permutation(ng)[:P].astype(np.int64)
    ao = ints(rng, (nao, ng), 2)
    ao[:, ip] = aoP.T
    A = gram_sq_ref(aoP)
    return dict(aoP=aoP, ao=ao, ip=ip, A=A, maxdiag=int(A.diagonal().max()))


def shifted(A, reg, maxdiag):
    """A + reg maxdiag I as the device forms it: one rounded addition per diagonal entry."""
    out = np.array(A, dtype=np.float64)
    if reg > 0:
        out[np.diag_indices(out.shape[0])] += reg * float(maxdiag)
    return out


def healthy_matrix(P, seed=1):
    """(A, L0): A = L0 L0^T for the integer factor L0 of factor_pair, as exact float64 integers."""
    L0, _ = factor_pair(P, seed)
    return exact_dot(L0, L0.T), L0


# ---- rounding measure ---------------------------------------------------------------------------------------------------------
UNIT = 2.0 ** -53


def rel_err(x, ref):
    ref = np.asarray(ref, dtype=np.longdouble)
    return float(abs(np.asarray(x, dtype=np.longdouble) - ref).max() / abs(ref).max())


def rounding_ratio(dev_err, host_err):
    """Device error over numpy's float64 error of the same operation, both against the same reference and relative to its
    largest entry.  Where numpy happens to be exact (integer inputs) the denominator is one unit roundoff, 2^-53: no float64
    evaluation that rounds at all can be expected to do better than that."""
    return dev_err / max(host_err, UNIT)


def solve_lower_longdouble(L, B, trans=False):
    """op(L)^-1 B by substitution in np.longdouble (L lower triangular, read below and on the diagonal only)."""
    L = np.tril(np.asarray(L, dtype=np.longdouble))
    X = np.array(B, dtype=np.longdouble)
    m = L.shape[0]
    if not trans:
        for i in range(m):
            X[i] = (X[i] - L[i, :i].dot(X[:i])) / L[i, i]
    else:
        for i in range(m - 1, -1, -1):
            X[i] = (X[i] - L[i + 1:, i].dot(X[i + 1:])) / L[i, i]
    return X
