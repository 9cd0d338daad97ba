"""Second derivatives of 'b88,' and 'lda,vwn' and the multigrid response surface built on them (CPU half).

The numpy kernels below restate the device's isdf_gga_b88_fxc / isdf_lda_vwn_fxc_add / isdf_xc_fxc_apply; they are checked against
central differences of the oracle's first derivatives (oracle.multigrid.b88_exchange, vwn_correlation), and then drive
pyscf_isdf_amd.multigrid's response functions on the CPU checker backend, where nr_rks_fxc / nr_uks_fxc must be the derivative of
nr_rks / nr_uks's potential matrix along the response density."""
import numpy as np
import pytest
import torch
from pyscf_isdf_amd import gto
from pyscf_isdf_amd import multigrid as pmg
from oracle import multigrid as omg
from oracle_backend import OracleBackend

B88_BETA = 0.0042
SYM4 = np.array([[0, 1, 2, 3], [1, 4, 5, 6], [2, 5, 7, 8], [3, 6, 8, 9]])     # (x, y) -> index of the 10 unique components


def b88_fxc(rho, grad):
    """(4, 4, G) kernel of e(rho, grad rho) = 2 f(rho/2, |grad rho|/2), eval_xc_eff's layout: [0,0] = v2rho2,
    [0,i] = 2 v2rhosigma d_i rho, [i,j] = 4 v2sigma2 d_i rho d_j rho + 2 vsigma delta_ij.  rho <= 1e-14 -> 0."""
    rho = np.asarray(rho, dtype=float)
    grad = np.asarray(grad, dtype=float)
    beta = B88_BETA
    cx = 1.5 * (3.0 / (4.0 * np.pi)) ** (1.0 / 3.0)
    m = rho > 1e-14
    rs = np.where(m, 0.5 * rho, 1.0)
    r13 = np.cbrt(rs)
    r43 = rs * r13
    x = 0.5 * np.sqrt((grad ** 2).sum(axis=0)) / r43
    x2 = x * x
    a = np.arcsinh(x)
    s = np.sqrt(1.0 + x2)
    a_x = np.where(x < 1e-3, 1.0 - x2 / 6.0 + 0.075 * x2 * x2, a / np.where(x < 1e-3, 1.0, x))
    D = 1.0 + 6.0 * beta * x * a
    Dp = 6.0 * beta * (a + x / s)
    Dpp = 6.0 * beta * (2.0 + x2) / s ** 3
    Dp_x = 6.0 * beta * (a_x + 1.0 / s)
    G = -cx - beta * x2 / D
    Gp_x = -beta * (2.0 * D - x * Dp) / D ** 2
    Gpp = -beta * ((2.0 * D - x2 * Dpp) * D - 2.0 * x * Dp * (2.0 * D - x * Dp)) / D ** 3
    H = -beta * (2.0 * Dp * Dp - D * Dpp - 3.0 * D * Dp_x) / D ** 3          # (G'' - G'/x) / x^2
    f00 = (2.0 / 9.0) * (G - x2 * Gp_x + 4.0 * x2 * Gpp) / (r13 * r13)
    c01 = -Gpp / (3.0 * rs * r43)
    vs2 = Gp_x / (2.0 * r43)
    s2 = H / (8.0 * rs ** 4)
    f = np.zeros((4, 4) + rho.shape)
    f[0, 0] = f00
    for i in range(3):
        f[0, 1 + i] = f[1 + i, 0] = c01 * grad[i]
        for j in range(3):
            f[1 + i, 1 + j] = s2 * grad[i] * grad[j] + (vs2 if i == j else 0.0)
    return np.where(m, f, 0.0)


def vwn_fxc(rho):
    """d2(rho eps_c)/d rho2 of the VWN5 correlation: -x (5 eps_c' - x eps_c'') / (36 rho), x = sqrt(rs).  rho <= 1e-24 -> 0."""
    A, b, c, x0 = omg.VWN5
    rho = np.asarray(rho, dtype=float)
    m = rho > 1e-24
    r = np.where(m, rho, 1.0)
    x = np.sqrt(np.cbrt(3.0 / (4.0 * np.pi * r)))
    X = x * x + b * x + c
    X0 = x0 * x0 + b * x0 + c
    Q = np.sqrt(4.0 * c - b * b)
    t = 2.0 * x + b
    den = Q * Q + t * t
    dec = A * (2.0 / x - t / X - 4.0 * b / den - b * x0 / X0 * (2.0 / (x - x0) - t / X - 4.0 * (b + 2.0 * x0) / den))
    dtX = (2.0 * X - t * t) / X ** 2
    d2ec = A * (-2.0 / x ** 2 - dtX + 16.0 * b * t / den ** 2
                - b * x0 / X0 * (-2.0 / (x - x0) ** 2 - dtX + 16.0 * (b + 2.0 * x0) * t / den ** 2))
    return np.where(m, -x * (5.0 * dec - x * d2ec) / (36.0 * r), 0.0)


class ResponseOracleBackend(OracleBackend):
    """The checker backend plus numpy forms of the response entries (isdf_gga_b88_fxc, isdf_xc_fxc_apply, isdf_lda_vwn_fxc_add)."""

    def lda_vwn_fxc_add(self, rho, fxc):
        fxc += torch.from_numpy(vwn_fxc(rho.numpy()))

    def gga_b88_fxc(self, rho0, rho1, wv, fxc=None):
        f = b88_fxc(rho0[0].numpy(), rho0[1:].numpy())
        if rho1 is not None:
            wv.copy_(torch.from_numpy(np.einsum('xng,xyg->yng', rho1.numpy(), f)))
        if fxc is not None:
            iu = np.triu_indices(4)
            fxc.copy_(torch.from_numpy(np.ascontiguousarray(f[iu])))

    def xc_fxc_apply(self, fxc, rho1, wv, accumulate=False):
        w = np.einsum('xng,xyg->yng', rho1.numpy(), fxc.numpy())
        if accumulate:
            wv += torch.from_numpy(w)
        else:
            wv.copy_(torch.from_numpy(w))


def cell_he_split():
    # tests/test_multigrid.py's cell: a sharp and a smooth primitive inside the same two contractions
    return gto.Cell(atom='He 0 0 0; He 2.2 2.4 2.1', basis=[[0, (6., 1, .1), (.4, .1, 1)], [1, (.8, 1)], [2, (1.1, 1)]], unit='B',
                    precision=1e-9, mesh=[30, 32, 30], a=np.eye(3) * 5 + np.array([[0, .3, 0], [0, 0, 0], [.2, 0, 0]]))


def make_dm(cell, seed=2):
    nao = cell.nao_nr()
    dm = np.random.default_rng(seed).random((nao, nao)) * .2 + np.eye(nao)
    return dm + dm.T


def make_kpts_dms(cell, hermitian=True, seed=3):
    rng = np.random.default_rng(seed)
    k0 = rng.random(3) * 0.4
    kpts = np.array([k0, -k0])
    nao = cell.nao_nr()
    dms = rng.random((2, nao, nao)) * .2 + 1j * (rng.random((2, nao, nao)) - .5) * .1
    if hermitian:
        dms = dms + dms.conj().transpose(0, 2, 1) + np.eye(nao)
    return kpts, dms


def _sample_points():
    """rho from 1e-6 to 10, |grad rho| including exactly 0, reduced gradient x up to ~50."""
    rng = np.random.default_rng(4)
    rho = np.repeat(np.array([1e-6, 1e-4, 1e-2, 0.1, 0.7, 3.0, 10.0]), 8)
    xs = np.tile(np.array([0.0, 1e-5, 2e-4, 0.05, 0.8, 4.0, 17.0, 50.0]), 7)
    d = rng.standard_normal((3, rho.size))
    d /= np.linalg.norm(d, axis=0)
    grad = d * (2.0 * xs * (0.5 * rho) ** (4.0 / 3.0))
    return rho, grad


def test_b88_fxc_matches_finite_differences_of_the_potential():
    rho, grad = _sample_points()
    f = b88_fxc(rho, grad)
    assert np.isfinite(f).all()
    v = lambda r, g: np.concatenate([omg.b88_exchange(r, g)[1][None], omg.b88_exchange(r, g)[2]])   # noqa: E731  (4, G)
    for x in range(4):
        h = np.where(rho > 0, 1e-5 * rho, 0.0) if x == 0 else 1e-5 * np.maximum(abs(grad[x - 1]), rho ** (4. / 3))
        rp, gp, rm, gm = rho.copy(), grad.copy(), rho.copy(), grad.copy()
        if x == 0:
            rp, rm = rho + h, rho - h
        else:
            gp[x - 1] += h
            gm[x - 1] -= h
        fd = (v(rp, gp) - v(rm, gm)) / (2 * h)                           # row x: d v_y / d rho_x
        scale = np.maximum(abs(f).max(axis=(0, 1)), 1e-300)
        assert (abs(fd - f[x]) / scale).max() < 1e-7, x
    # the uniform-gas limit is the Slater kernel
    flat = abs(grad).sum(axis=0) == 0
    slater = omg.slater_exchange_fxc(rho[flat])
    assert flat.sum() == 7 and abs(f[0, 0, flat] / slater - 1).max() < 1e-13
    assert abs(b88_fxc(np.array([0.0, 1e-15]), np.zeros((3, 2)))).max() == 0.0


def test_vwn_fxc_matches_finite_differences_of_the_potential():
    rho = np.array([1e-6, 1e-4, 1e-3, 0.05, 0.3, 1.7, 10.0, 20.0])
    h = 1e-5 * rho
    fd = (omg.vwn_correlation(rho + h)[1] - omg.vwn_correlation(rho - h)[1]) / (2 * h)
    assert abs(fd / vwn_fxc(rho) - 1).max() < 1e-7
    assert abs(vwn_fxc(np.array([0.0, 1e-30]))).max() == 0.0


def _checker_df(cell):
    df = pmg.MultiGridFFTDF(cell, backend=ResponseOracleBackend())
    df.split = 'all'
    return df


def check_b88_gamma(df, cell):
    """'b88,' at the Gamma point: the derivative of nr_rks / nr_uks's potential, the Coulomb term, the symmetric part of a
    non-symmetric input, the second-order XC energy, the cache round trips and the spin-scaled forms."""
    nao = cell.nao_nr()
    dm0 = make_dm(cell)
    dm1 = np.random.default_rng(9).standard_normal((2, nao, nao)) * 0.05
    v = pmg.nr_rks_fxc(df, 'b88,', dm0, dm1, with_j=True)
    assert v.shape == dm1.shape
    eps = 1e-4
    sym = 0.5 * (dm1[0] + dm1[0].T)
    fd = (pmg.nr_rks(df, 'b88,', dm0 + eps * sym, with_j=True)[2] - pmg.nr_rks(df, 'b88,', dm0 - eps * sym, with_j=True)[2]) / (2 * eps)
    assert abs(v[0] - fd).max() < 1e-6 * abs(v[0]).max()
    vx = pmg.nr_rks_fxc(df, 'b88,', dm0, dm1)
    vj = df.get_jk(0.5 * (dm1 + dm1.transpose(0, 2, 1)), with_k=False)[0]
    assert abs(v - vx - vj).max() < 1e-10 * abs(v).max()
    assert abs(pmg.nr_rks_fxc(df, 'b88,', dm0, sym[None]) - vx[0]).max() < 1e-12 * abs(vx).max()
    # second-order XC energy: [E(dm0 + h d) + E(dm0 - h d) - 2 E(dm0)] / h^2 = tr(d fxc[d])
    h = 1e-3
    e2 = (pmg.nr_rks(df, 'b88,', dm0 + h * sym)[1] + pmg.nr_rks(df, 'b88,', dm0 - h * sym)[1] - 2 * pmg.nr_rks(df, 'b88,', dm0)[1]) / h ** 2
    assert abs(e2 / np.einsum('ij,ji', sym, vx[0]) - 1) < 1e-5
    # the kernel through the cache, and the singlet / triplet / open-shell forms of exchange by spin scaling
    rho, vxc, fxc = pmg.cache_xc_kernel1(df, 'b88,', dm0)
    G = int(np.prod(cell.mesh))
    assert rho.shape == (4, G) and vxc.shape == (4, G) and fxc.shape == (4, 4, G)
    assert abs(pmg.nr_rks_fxc(df, 'b88,', None, dm1, with_j=True, rho0=rho, fxc=fxc) - v).max() < 1e-12 * abs(v).max()
    v0 = pmg.nr_rks_fxc(df, 'b88,', dm0, dm1)
    vs = pmg.nr_rks_fxc_st(df, 'b88,', dm0, dm1, singlet=True)
    assert abs(vs - 2 * v0).max() < 1e-10 * abs(vs).max()
    assert abs(pmg.nr_rks_fxc_st(df, 'b88,', dm0, dm1, singlet=False) - vs).max() < 1e-12 * abs(vs).max()
    pair0 = np.stack([dm0 * .6, dm0 * .4])
    pair1 = np.stack([dm1[0], dm1[1], dm1[1] * .5, dm1[0] * -.3])
    vu = pmg.nr_uks_fxc(df, 'b88,', pair0, pair1, with_j=True)
    d = np.stack([0.5 * (pair1[0] + pair1[0].T), 0.5 * (pair1[2] + pair1[2].T)])
    fdu = (pmg.nr_uks(df, 'b88,', pair0 + eps * d, with_j=True)[2] - pmg.nr_uks(df, 'b88,', pair0 - eps * d, with_j=True)[2]) / (2 * eps)
    assert abs(vu[[0, 2]] - fdu).max() < 1e-6 * abs(vu).max()
    r2, v2, f2 = pmg.cache_xc_kernel1(df, 'b88,', pair0, spin=1)
    assert r2.shape == (2, 4, G) and v2.shape == (2, 4, G) and f2.shape == (2, 4, 2, 4, G) and abs(f2[0, :, 1]).max() == 0
    assert abs(pmg.nr_uks_fxc(df, 'b88,', None, pair1, with_j=True, rho0=r2, fxc=f2) - vu).max() < 1e-12 * abs(vu).max()
    # 'lda,': the caller-supplied open-shell kernel too
    vl = pmg.nr_uks_fxc(df, 'lda,', pair0, pair1, with_j=True)
    r2, v2, f2 = pmg.cache_xc_kernel1(df, 'lda,', pair0, spin=1)
    assert abs(pmg.nr_uks_fxc(df, 'lda,', None, pair1, with_j=True, rho0=r2, fxc=f2) - vl).max() < 1e-12 * abs(vl).max()


def check_b88_kpts(df, cell):
    """'b88,' at k-points: a Hermitian response is the derivative of the k-point nr_rks; H + iA gives v(H) + i v(A)."""
    kpts, dm0 = make_kpts_dms(cell)
    _, dm1 = make_kpts_dms(cell, seed=11)
    dm1 = dm1 - np.eye(cell.nao_nr())
    v = pmg.nr_rks_fxc(df, 'b88,', dm0, dm1, with_j=True, kpts=kpts)
    assert v.shape == dm1.shape
    eps = 1e-4
    fd = (pmg.nr_rks(df, 'b88,', dm0 + eps * dm1, kpts=kpts, with_j=True)[2]
          - pmg.nr_rks(df, 'b88,', dm0 - eps * dm1, kpts=kpts, with_j=True)[2]) / (2 * eps)
    assert abs(v - fd).max() < 1e-6 * abs(v).max()
    _, A = make_kpts_dms(cell, seed=13)
    vA = pmg.nr_rks_fxc(df, 'b88,', dm0, A, with_j=True, kpts=kpts)
    vHA = pmg.nr_rks_fxc(df, 'b88,', dm0, (dm1 + 1j * A)[None], with_j=True, kpts=kpts)
    assert vHA.shape == (1,) + dm1.shape
    assert abs(vHA[0] - (v + 1j * vA)).max() < 1e-10 * abs(v).max()


def check_vwn(df, cell):
    nao = cell.nao_nr()
    dm0 = make_dm(cell)
    dm1 = np.random.default_rng(9).standard_normal((2, nao, nao)) * 0.05
    v = pmg.nr_rks_fxc(df, 'lda,vwn', dm0, dm1, with_j=True)
    eps = 1e-4
    sym = 0.5 * (dm1[0] + dm1[0].T)
    fd = (pmg.nr_rks(df, 'lda,vwn', dm0 + eps * sym, with_j=True)[2] - pmg.nr_rks(df, 'lda,vwn', dm0 - eps * sym, with_j=True)[2]) / (2 * eps)
    assert abs(v[0] - fd).max() < 1e-6 * abs(v[0]).max()
    assert abs(v - pmg.nr_rks_fxc(df, 'lda,', dm0, dm1, with_j=True)).max() > 1e-4 * abs(v).max()
    vs = pmg.nr_rks_fxc_st(df, 'lda,vwn', dm0, dm1, singlet=True)
    assert abs(vs - 2 * pmg.nr_rks_fxc(df, 'lda,vwn', dm0, dm1)).max() < 1e-10 * abs(vs).max()
    rho, vxc, fxc = pmg.cache_xc_kernel1(df, 'lda,vwn', dm0)
    assert abs(pmg.nr_rks_fxc(df, 'lda,vwn', None, dm1, with_j=True, rho0=rho, fxc=fxc) - v).max() < 1e-12 * abs(v).max()
    pair = np.stack([dm0, dm0]) * .5
    with pytest.raises(NotImplementedError):
        pmg.nr_rks_fxc_st(df, 'lda,vwn', dm0, dm1, singlet=False)
    with pytest.raises(NotImplementedError):
        pmg.nr_uks_fxc(df, 'lda,vwn', pair, np.stack([dm1[0], dm1[0]]))
    with pytest.raises(NotImplementedError):
        pmg.cache_xc_kernel1(df, 'lda,vwn', pair, spin=1)
    for xc in ('pbe,pbe', 'b3lyp', 'lda,pw'):
        with pytest.raises(NotImplementedError):
            pmg.nr_rks_fxc(df, xc, dm0, dm1)
        with pytest.raises(NotImplementedError):
            pmg.cache_xc_kernel1(df, xc, dm0)


def test_b88_response_is_the_derivative_of_the_potential_on_checker_backend():
    cell = cell_he_split()
    check_b88_gamma(_checker_df(cell), cell)


def test_b88_kpts_response_on_checker_backend():
    cell = cell_he_split()
    check_b88_kpts(_checker_df(cell), cell)


def test_lda_vwn_response_and_refusals_on_checker_backend():
    cell = cell_he_split()
    check_vwn(_checker_df(cell), cell)


class _MF:
    def __init__(self, df, xc, kpts):
        self.with_df, self.xc, self.kpts = df, xc, kpts


def check_generators(df, cell):
    """_gen_rhf_response / _gen_uhf_response against the uncached response functions (reference test_gen_rhf_response's shape)."""
    kpts, dm0 = make_kpts_dms(cell)
    _, dm1 = make_kpts_dms(cell, seed=11)
    for xc in ('lda,', 'b88,'):
        vind = pmg._gen_rhf_response(_MF(df, xc, kpts), dm0, hermi=1)
        ref = pmg.nr_rks_fxc(df, xc, dm0, dm1, with_j=True, kpts=kpts)
        assert abs(vind(dm1) - ref).max() < 1e-12 * abs(ref).max()
        assert abs(pmg._gen_rhf_response(_MF(df, xc, kpts), dm0, hermi=2)(dm1)).max() == 0
    # Gamma point: singlet / triplet and the open-shell generator against the uncached calls
    g0 = np.zeros((1, 3))
    dmr = make_dm(cell)
    nao = cell.nao_nr()
    d1 = np.random.default_rng(5).standard_normal((2, nao, nao)) * 0.05
    for xc in ('lda,', 'b88,'):
        mf = _MF(df, xc, g0)
        for singlet in (True, False):
            ref = pmg.nr_rks_fxc_st(df, xc, dmr, d1, singlet=singlet)
            assert abs(pmg._gen_rhf_response(mf, dmr, singlet=singlet)(d1) - ref).max() < 1e-12 * abs(ref).max()
        pair0 = np.stack([dmr * .6, dmr * .4])
        pair1 = np.concatenate([d1, d1[::-1] * .5])
        ref = pmg.nr_uks_fxc(df, xc, pair0, pair1, with_j=True)
        assert abs(pmg._gen_uhf_response(mf, pair0)(pair1) - ref).max() < 1e-12 * abs(ref).max()


def test_response_generators_on_checker_backend():
    cell = cell_he_split()
    check_generators(_checker_df(cell), cell)
