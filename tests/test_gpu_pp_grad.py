"""The pseudopotential / local-potential force kernels on the device: isdf_pp_projector_overlaps_ip, isdf_pp_local_force and
isdf_rowdot3 entry by entry, then pp_nuc_grad / get_pp_ip1 / get_j_nuc_grad / nuc_grad_local end to end.  The references are the
longdouble restatements of tests/pp_grad_reference.py; every bound of a floating-point comparison is pp_cases.device_bound of the
float64 oracle's error against longdouble on the same shape (8 x that error, at least 64 ulp of the largest reference entry,
failing outright above 1e-11 of it).  isdf_rowdot3 runs on integer-valued operands whose sums are exact: equality."""
import numpy as np
import pytest
import torch
import cells
import pp_cases as pc
import pp_reference as ref
import pp_grad_reference as pgr

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not ref.LD_OK, reason=ref.LD_SKIP_REASON)]
EPS = np.finfo(np.float64).eps


@pytest.fixture(scope='module')
def be():
    from pyscf_isdf_amd.backend import HipBackend
    return HipBackend(0)


def _compare(name, got, want, oracle):
    """max|got - want| against the rule's bound; returns the bound (absolute)."""
    scale = abs(want).max()
    oerr = abs(oracle - want).max()
    bound = pc.device_bound(oerr, scale)
    err = abs(got - want).max()
    print('%-40s device %.2e  oracle %.2e  bound %.2e  (of max|ref| = %.3g)' % (name, err / scale, oerr / scale, bound / scale, scale))
    assert np.all(np.isfinite(got))
    assert err <= bound, (name, float(err / scale), float(bound / scale))
    return bound


# ---- isdf_pp_projector_overlaps_ip ------------------------------------------------------------------------------------------
def _overlaps_ip(be, args, nrows, fill=float('nan')):
    out = torch.full((4, nrows, 22), complex(fill, fill), dtype=torch.complex128, device=be.device)
    be.pp_projector_overlaps_ip(*args, out)
    return be.to_host(out)


@pytest.mark.parametrize('mesh,kname', pc.OV_CASES)
def test_projector_overlaps_ip(be, mesh, kname):
    """The tables of tests/test_gpu_pp.py (all nine (l, i) projectors, s / p / d shells, Gamma and k = (0.21, -0.13, 0.34)) on the
    meshes that make the chunk loop of 16384 columns run one ragged chunk (720), exactly one (16384), a second of 436 (16820) and
    three (33792); the output starts as NaN.  Component 0 against the longdouble overlaps and against the existing entry's
    output on the same handle (within the bound of the shape: they differ by the zgemm's row count only); components 1..3,
    sum_G (i G_x) conj(SI_a) p_j(G+k) aoG(G+k) with G the lattice vector at the k-point too, against their longdouble form.
    Oracle against longdouble (CPU) of the largest entry (8.3 / 9.2): 1.4e-15 .. 2.7e-15 on 720 points, 9.2e-15 .. 1.9e-14 on the
    larger meshes, so the bounds are 1.4e-14 .. 2.2e-14 and 7.4e-14 .. 1.5e-13.  Device, observed on the MI355X: component 0
    2.3e-15 .. 2.9e-14 and bit-identical to the existing entry's output in all eight cases; components 1..3 1.9e-15 .. 1.9e-14."""
    args = pc.ov_inputs(mesh, kname)
    nrows = pc.ov_rows()[1]
    want, orc = pc.cached(pgr.ov_ip_ld, mesh, kname), pc.cached(pgr.ov_ip_oracle, mesh, kname)
    got = _overlaps_ip(be, args, nrows)
    b0 = _compare('overlaps_ip[0] %s %s' % (mesh, kname), got[0], want[0], orc[0])
    _compare('overlaps_ip[1:] %s %s' % (mesh, kname), got[1:], want[1:], orc[1:])
    old = torch.full((nrows, 22), complex('nan'), dtype=torch.complex128, device=be.device)
    be.pp_projector_overlaps(*args, old)
    d = abs(got[0] - be.to_host(old)).max()
    print('component 0 - isdf_pp_projector_overlaps: %.2e of max' % (d / abs(want[0]).max()))
    assert d <= b0


def test_projector_overlaps_ip_reuses_workspaces(be):
    """Three chunks with the whole table, then one ragged chunk with the first five projectors only (9 of the 40 rows: the
    component stride of pp_SPG and of the output changes), then the first call again: the small result holds its bound against the
    leading rows of the reference, the third is bit-identical to the first."""
    big, small = pc.ov_inputs((33, 32, 32), 'k'), list(pc.ov_inputs((10, 9, 8), 'k'))
    small[5], small[6] = small[5][:5], small[6][:5]
    nrows = pc.ov_rows()[1]
    first = _overlaps_ip(be, big, nrows)
    mid = _overlaps_ip(be, small, 9, fill=7.0)
    third = _overlaps_ip(be, big, nrows, fill=-3.0)
    assert np.array_equal(first, third)
    want, orc = pc.cached(pgr.ov_ip_ld, (10, 9, 8), 'k'), pc.cached(pgr.ov_ip_oracle, (10, 9, 8), 'k')
    _compare('overlaps_ip (10,9,8) k, 9 rows, between', mid, want[:, :9], orc[:, :9])


# ---- isdf_pp_local_force ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nset', [1, 3])
@pytest.mark.parametrize('lat,par', pc.VLOC_CASES)
def test_local_force(be, lat, par, nset):
    """The meshes and parameter sets of the local-potential test (four off-grid atoms, one of them bare, nexp 0..4) with a random
    real density of 1 and of 3 rows (3: a full pair of rows and a half-filled one in the kernel's tiling; (15, 14, 16) = 3360
    points: two chunks of 2048, the second ragged): (nset, natm, 3) against the longdouble force stated with one inverse
    transform per atom and direction.  Output prefilled with NaN; a second call after one on another mesh is bit-identical.
    Oracle against longdouble (CPU): 7.0e-16 .. 5.1e-15 of the largest entry, so the bounds are 1.4e-14 (the floor) .. 4.1e-14.
    Device, observed on the MI355X: 2.0e-16 .. 7.1e-15 (the largest on fcc nexp024, one row, where the oracle has its 5.1e-15)."""
    coords, pp_par, mesh, a = pc.vloc_inputs(lat, par)
    want, orc = pc.cached(pgr.force_ld, lat, par, nset), pc.cached(pgr.force_oracle, lat, par, nset)

    def run(lat, par, nset):
        coords, pp_par, mesh, a = pc.vloc_inputs(lat, par)
        rho = be.to_device(pgr.force_rho(lat, nset))
        out = torch.full((nset, len(coords), 3), float('nan'), dtype=torch.float64, device=be.device)
        be.pp_local_force(rho, coords, pp_par, mesh, a, out)
        return be.to_host(out)

    got = run(lat, par, nset)
    _compare('local force %s %s nset %d' % (lat, par, nset), got, want, orc)
    other = [c for c in pc.VLOC_CASES if c[0] != lat][0]
    run(*other, 2)
    assert np.array_equal(run(lat, par, nset), got)


# ---- isdf_rowdot3 -----------------------------------------------------------------------------------------------------------------
def test_rowdot3_exact(be):
    """Integer-valued operands (|A| <= 3, |s| <= 2, |B| <= 3, alpha = -2: every partial sum is an integer below 2^53) over rows
    1, 5, 64, 65 x k = 1, 63, 64, 257, 4133 in five layouts: packed when k is even, else padded to an even leading dimension (the
    16-byte path, whose odd last column goes the scalar way), leading dimensions larger than k and even (16-byte path), odd leading
    dimensions, an odd plane stride, and a base off by one double (the scalar path, three ways).  accumulate off on a NaN
    prefill, then accumulate on.  Both kernels must have run (the profile's names)."""
    rng = np.random.default_rng(31)
    be.prof_reset()
    be.prof_enable(True)
    try:
        for M in (1, 5, 64, 65):
            for K in (1, 63, 64, 257, 4133):
                A = rng.integers(-3, 4, (3, M, K)).astype(np.float64)
                s = rng.integers(-2, 3, K).astype(np.float64)
                B = rng.integers(-3, 4, (M, K)).astype(np.float64)
                want = -2.0 * np.einsum('xmk,k,mk->xm', A, s, B)
                # (leading dimension, extra doubles between planes, offset of the base)
                for ld, gap, off in [(K + (K & 1), 0, 0), (K + 6 + (K & 1), 0, 0), (K + 3 + (K & 1), 0, 0), (K + (K & 1), 1, 0),
                                     (K + 2 + (K & 1), 0, 1)]:
                    bufA = torch.full((3 * (M * ld + gap) + 2,), float('nan'), dtype=torch.float64, device=be.device)
                    dA = bufA[off:off + 3 * (M * ld + gap)].view(3, M * ld + gap)[:, :M * ld].view(3, M, ld)[:, :, :K]
                    dA.copy_(be.to_device(A))
                    bufB = torch.full((M * ld + 2,), float('nan'), dtype=torch.float64, device=be.device)
                    dB = bufB[off:off + M * ld].view(M, ld)[:, :K]
                    dB.copy_(be.to_device(B))
                    ds = torch.full((K + 2,), float('nan'), dtype=torch.float64, device=be.device)[off:off + K]
                    ds.copy_(be.to_device(s))
                    out = torch.full((3, M + 1), float('nan'), dtype=torch.float64, device=be.device)
                    be.rowdot3(dA, ds, dB, out[:, :M], alpha=-2.0)
                    got = be.to_host(out)
                    assert np.array_equal(got[:, :M], want), (M, K, ld, gap, off)
                    assert np.all(np.isnan(got[:, M]))
                    be.rowdot3(dA, ds, dB, out[:, :M], alpha=-2.0, accumulate=True)
                    assert np.array_equal(be.to_host(out)[:, :M], 2 * want), (M, K, ld, gap, off, 'accumulate')
        names = be.prof_results()
    finally:
        be.prof_enable(False)
    assert names['rowdot3_kernel<true>[byte]']['launches'] == 2 * 20 * 2 and names['rowdot3_kernel<false>[byte]']['launches'] == 2 * 20 * 3


# ---- end to end -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def e2e():
    su = pgr.CellSetup(pc.e2e_cell())
    x = np.random.default_rng(3).standard_normal((su.cell.nao_nr(),) * 2)
    su.dm = 0.5 * (x + x.T)
    su.ip1_ld, su.grad_ld = pgr.e2e_ld(su, su.dm)
    return su


def test_pp_nuc_grad_and_ip1_end_to_end(e2e):
    """pp_nuc_grad and get_pp_ip1 of pp_cases.e2e_cell() (triclinic, mesh (12, 11, 10), s / p / d shells, the fixture's Ge and Y
    entries) with a random symmetric D against their longdouble restatement, the float64 restatement giving the oracle's error;
    e1_grid_chunk = 512 walks the 1320 points in three chunks, the last of 296.  The AO values and gradients on the grid are
    the oracle's in both references, taken as data, so the device's collocation error is inside the comparison.
    Oracle against longdouble (CPU): 2.9e-14 of the largest gradient entry 0.32 and 7.3e-15 of the largest matrix entry 2.1, so
    the bounds are 2.3e-13 and 5.9e-14.  Device, observed on the MI355X: 1.6e-14 and 8.0e-15."""
    from pyscf_isdf_amd.isdf import ISDF
    su = e2e
    df = ISDF(su.cell)
    df.e1_grid_chunk = 512
    grad, ip1 = df.pp_nuc_grad(su.dm), df.get_pp_ip1()
    assert grad.shape == (su.cell.natm, 3) and ip1.shape == (3,) + su.dm.shape and ip1.dtype == np.float64
    _compare('pp_nuc_grad', grad, su.grad_ld, pgr.pp_nuc_grad(su, su.dm))
    _compare('get_pp_ip1', ip1, su.ip1_ld, sum(pgr.get_pp_ip1(su)))
    stack = df.pp_nuc_grad(np.array([su.dm, 2 * su.dm]))
    assert stack.shape == (2, su.cell.natm, 3)
    assert abs(stack[0] - grad).max() <= 64 * EPS * abs(grad).max() and abs(stack[1] - 2 * grad).max() <= 128 * EPS * abs(grad).max()


def test_pp_nuc_grad_is_the_derivative_of_the_device_get_pp(e2e):
    """One central difference of the device's own get_pp: atom 1, axis 2, h = 2e-2 and 1e-2 Bohr.  Bound on |analytic - FD(h/2)| as
    in tests/test_pp_grad.py: |FD(h) - FD(h/2)| (three times the finer estimate's truncation error) plus 64 ulp of sum|D o V|
    divided by h/2.  Observed on the MI355X: analytic +3.1979470032e-01, FD(h/2) +3.1970516093e-01, |diff| 8.95e-05 against
    |FD(h) - FD(h/2)| 2.69e-04 (one third: the finer estimate's truncation error) and a rounding term of 2.6e-11."""
    from pyscf_isdf_amd.isdf import ISDF
    su, ia, x, h = e2e, 1, 2, 2e-2
    grad = ISDF(su.cell).pp_nuc_grad(su.dm)[ia, x]

    def energy(d):
        return np.einsum('mn,nm', ISDF(pgr.displaced_cell(ia, x, d)).get_pp(), su.dm)

    fd = {s: (energy(s) - energy(-s)) / (2 * s) for s in (h, h / 2)}
    own = abs(fd[h] - fd[h / 2])
    rounding = 64 * EPS * abs(su.dm * ISDF(su.cell).get_pp()).sum() / (h / 2)
    print('analytic %+.10e  fd %+.10e  |diff| %.2e  |FD(h) - FD(h/2)| %.2e  rounding %.2e' %
          (grad, fd[h / 2], abs(grad - fd[h / 2]), own, rounding))
    assert abs(grad - fd[h / 2]) <= own + rounding


def test_j_force_and_the_multigrid_object():
    """get_j_nuc_grad against the contraction 2 sum_(mu in a) sum_nu get_j_e1(D)[x, mu, nu] D_(nu mu) of the device's own get_j_e1 on
    diamond / gth-szv at 12^3 (e1_grid_chunk = 1000: 1728 = 1000 + 728), to 1e-12 of the largest entry.  Then nuc_grad_local on a
    MultiGridFFTDF with the Slater potential of its density (the 'lda,' potential of nr_rks: isdf_lda_exchange): shape, finiteness
    and agreement with the plain object - a smoke of the inheritance.  Observed on the MI355X: 1.1e-15 of the largest entry 0.27."""
    from pyscf_isdf_amd.isdf import ISDF
    from pyscf_isdf_amd import multigrid as pmg
    cell = cells.cell_diamond_prim('gth-szv', (12, 12, 12))
    nao = cell.nao_nr()
    c = np.linalg.qr(np.random.default_rng(11).standard_normal((nao, nao)))[0]
    occ = np.zeros(nao)
    occ[:cell.nelectron // 2] = 2
    dm = (c * occ).dot(c.T)
    df = ISDF(cell)
    df.e1_grid_chunk = 1000
    aosl = np.asarray(cell.aoslice_by_atom())[:, -2:]
    e1 = df.get_j_e1(dm)
    want = np.array([2 * np.einsum('xmn,nm->x', e1[:, p0:p1], dm[:, p0:p1]) for p0, p1 in aosl])
    got = df.get_j_nuc_grad(dm)
    print('get_j_nuc_grad - contraction of get_j_e1: %.2e of max %.3g' % (abs(got - want).max() / abs(want).max(), abs(want).max()))
    assert got.shape == (cell.natm, 3) and abs(got - want).max() <= 1e-12 * abs(want).max()

    mg = pmg.MultiGridFFTDF(cell)
    be = mg.backend
    G = int(np.prod(cell.mesh))
    mg.collocate()
    rho, exc, vxc = be.empty((1, G)), be.empty((G,)), be.empty((G,))
    be.rho_pair(mg.ao, mg.ao, G, be.to_device(dm[None]), rho)
    be.lda_exchange(rho[0], exc, vxc)
    f = mg.nuc_grad_local(vxc, dm)
    assert f.shape == (cell.natm, 3) and np.all(np.isfinite(f)) and abs(f).max() > 0
    assert abs(f - df.nuc_grad_local(be.to_host(vxc), dm)).max() <= 1e-12 * abs(f).max()
