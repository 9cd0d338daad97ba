"""The XC nuclear forces on the device: isdf_gga_aow entry by entry (integer-valued operands whose sums are exact: equality with
numpy), then xc_nuc_grad / get_vxc_e1 / xc_nuc_grad_uks end to end on cell_he_split - against the dense numpy restatement
(tests/xc_grad_reference.py, pinned on the CPU by tests/test_xc_grad.py) at 1e-9 of the largest entry, the device bound of
test_gpu_multigrid_gga_b88 / check_lyp_ladder for the same operations, and against central differences of the device's own nr_rks /
nr_uks energies under a displaced atom."""
import numpy as np
import pytest
import xc_grad_reference as xr
from pyscf_isdf_amd import gto
from pyscf_isdf_amd import multigrid as pmg
from test_multigrid import cell_he_split, make_dm

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
H = 2e-3            # Bohr: the larger of the two central-difference steps; the finer one is H / 2
# the ladder's own density error in the force, measured on the CPU checker backend (tests/test_xc_grad.py): 2.7e-10 of max|F|
LADDER_FORCE = 2.7e-10


@pytest.fixture(scope='module')
def be():
    from pyscf_isdf_amd.backend import HipBackend
    return HipBackend(0)


# ---- isdf_gga_aow ------------------------------------------------------------------------------------------------------------------
def _aow_numpy(a, w):
    Z = w[0] * a[0] + w[1] * a[1] + w[2] * a[2] + w[3] * a[3]
    G = np.stack([w[1] * a[p] + w[2] * a[q] + w[3] * a[r] for p, q, r in ((4, 5, 6), (5, 7, 8), (6, 8, 9))])
    return Z, G


@pytest.mark.parametrize('nset', [1, 3])
@pytest.mark.parametrize('layout', ['padded', 'odd_plane', 'offset'])
@pytest.mark.parametrize('K', [1031, 1024])
def test_gga_aow_is_exact_on_integers(be, K, layout, nset):
    """M = 5 rows; K = 1031 (no multiple of the 256-lane block or of 2: a ragged last block, and on the 16-byte path an odd last
    column) and K = 1024; ld = K + 7 throughout; 'padded': an even plane stride and aligned bases (the 16-byte path for K = 1031, where
    ld is even; K = 1024 makes ld odd: the scalar path), 'odd_plane': an odd plane stride, 'offset': every base one double off 16-byte
    alignment (both the scalar path).  A sentinel behind every row and plane, inputs and outputs.  Integer values |v| <= 8: every sum
    is exact, so the result equals numpy's bit for bit."""
    import torch
    M, ld = 5, K + 7
    plane = M * ld + (4 if layout == 'padded' else 5 if layout == 'odd_plane' else 6)
    off = 1 if layout == 'offset' else 0
    rng = np.random.default_rng(K + nset)
    a = rng.integers(-8, 9, size=(10, M, K)).astype(np.float64)
    w = rng.integers(-8, 9, size=(nset, 4, K)).astype(np.float64)

    def padded(values, lead, ld_, plane_):
        """values (lead..., M, K) in a sentinel-filled flat buffer with row stride ld_ and stride plane_ between (M, K) blocks."""
        nb = int(np.prod(lead))
        host = np.full(off + nb * plane_ + 2, SENTINEL)
        body = host[off:off + nb * plane_].reshape(nb, plane_)[:, :M * ld_].reshape(nb, M, ld_)
        body[:, :, :K] = values.reshape(nb, M, K)
        flat = be.to_device(host)
        view = flat[off:off + nb * plane_].view(nb, plane_)[:, :M * ld_].unflatten(1, (M, ld_))
        return flat, view, host

    ao_flat, ao_view, ao_host = padded(a, (10,), ld, plane)
    w_host = np.full(off + nset * 4 * ld + 2, SENTINEL)
    w_host[off:off + nset * 4 * ld].reshape(nset, 4, ld)[:, :, :K] = w
    w_flat = be.to_device(w_host)
    w_view = w_flat[off:off + nset * 4 * ld].view(nset, 4, ld)[:, :, :K]
    Z_flat, Z_view, _ = padded(np.zeros((nset, M, K)), (nset,), ld, plane)
    G_flat, G_view, _ = padded(np.zeros((nset, 3, M, K)), (nset, 3), ld, plane)
    Z_flat.fill_(SENTINEL)
    G_flat.fill_(SENTINEL)
    G_view = G_view.unflatten(0, (nset, 3))
    vec = layout == 'padded' and ld % 2 == 0
    assert (ao_view.data_ptr() % 16 == 0) == (layout != 'offset')
    be.prof_enable(True)
    be.prof_reset()
    for s in range(nset):
        be.gga_aow(ao_view[:, :, :K], w_view[s], Z_view[s, :, :K], G_view[s, :, :, :K])
    labels = be.prof_results()
    be.prof_enable(False)
    assert ('gga_aow_kernel<true>[byte]' in labels) == vec and ('gga_aow_kernel<false>[byte]' in labels) == (not vec)
    Zh = be.to_host(Z_flat)[off:off + nset * plane].reshape(nset, plane)
    Gh = be.to_host(G_flat)[off:off + nset * 3 * plane].reshape(nset, 3, plane)
    for s in range(nset):
        Zr, Gr = _aow_numpy(a, w[s])
        assert np.array_equal(Zh[s, :M * ld].reshape(M, ld)[:, :K], Zr)
        assert np.array_equal(Gh[s, :, :M * ld].reshape(3, M, ld)[:, :, :K], Gr)
    # nothing but the (M, K) blocks was written, and the inputs are as they were
    assert (Zh[:, :M * ld].reshape(nset, M, ld)[:, :, K:] == SENTINEL).all() and (Zh[:, M * ld:] == SENTINEL).all()
    assert (Gh[:, :, :M * ld].reshape(nset, 3, M, ld)[..., K:] == SENTINEL).all() and (Gh[:, :, M * ld:] == SENTINEL).all()
    for flat in (Z_flat, G_flat):
        h = be.to_host(flat)
        assert (h[:off] == SENTINEL).all() and (h[-2:] == SENTINEL).all()
    assert np.array_equal(be.to_host(ao_flat), ao_host) and np.array_equal(be.to_host(w_flat), w_host)


# ---- the product -------------------------------------------------------------------------------------------------------------------
def _he_split(shift=None):
    """cell_he_split with atom ``shift[0]`` displaced by ``shift[2]`` Bohr along axis ``shift[1]``."""
    base = cell_he_split()
    xyz = np.array([[0., 0., 0.], [2.2, 2.4, 2.1]])
    if shift is not None:
        xyz[shift[0], shift[1]] += shift[2]
    return gto.Cell(atom=[['He', tuple(r)] for r in xyz], basis=[[0, (6., 1, .1), (.4, .1, 1)], [1, (.8, 1)], [2, (1.1, 1)]], unit='B',
                    precision=1e-9, mesh=[30, 32, 30], a=base.lattice_vectors())


def _device_df(cell, levels):
    df = pmg.MultiGridFFTDF(cell)
    if levels == 'one':
        df.max_levels = 1
    else:
        df.split = 'all'
    return df


@pytest.fixture(scope='module')
def dense():
    su = xr.CellSetup(cell_he_split())
    su.dm = make_dm(su.cell)
    su.ao10 = su.ao10()
    return su


def _rel(x, ref):
    return float(abs(x - ref).max() / abs(ref).max())


def test_the_displaced_cell_builder_restates_cell_he_split():
    a, b = cell_he_split(), _he_split()
    assert np.array_equal(a._bas, b._bas) and np.allclose(a._env, b._env, rtol=0, atol=1e-15) and np.array_equal(a.mesh, b.mesh)


@pytest.mark.parametrize('levels', ['one', 'all'])
@pytest.mark.parametrize('code', ['blyp', 'b3lyp5'])
def test_force_and_matrix_match_the_restatement(dense, code, levels):
    """1e-9 of the largest entry; on the several-level ladder the force bound is ten times the ladder's own density error measured on
    the CPU (2.7e-9 of max|F|, the larger of the two), the matrix bound stays 1e-9 (its CPU-measured ladder difference is 3.4e-12)."""
    df = _device_df(dense.cell, levels)
    F, e1 = pmg.xc_nuc_grad(df, code, dense.dm), pmg.get_vxc_e1(df, code, dense.dm)
    assert len(df.tasks) == (1 if levels == 'one' else 3)
    Fr = xr.xc_nuc_grad(dense.ao10, dense.dm, code, dense.weight, dense.aoslices)
    er = xr.get_vxc_e1(dense.ao10, dense.dm, code, dense.weight)
    print('%s %s: force %.3e, matrix %.3e' % (code, levels, _rel(F, Fr), _rel(e1, er)))
    assert F.shape == Fr.shape and e1.shape == er.shape
    assert _rel(F, Fr) < (1e-9 if levels == 'one' else max(1e-9, 10 * LADDER_FORCE))
    assert _rel(e1, er) < 1e-9
    assert _rel(xr.contract_e1(e1, dense.dm, dense.aoslices), F) < 1e-9
    assert 'S8_xc_nuc_grad' in df.timings


def _fd_check(energy, analytic, what):
    fd = {h: (energy(h) - energy(-h)) / (2 * h) for h in (H, H / 2)}
    own, diff = abs(fd[H] - fd[H / 2]), abs(analytic - fd[H / 2])
    print('%s: analytic %+.10e  fd %+.10e  |diff| %.2e  |FD(h) - FD(h/2)| %.2e' % (what, analytic, fd[H / 2], diff, own))
    assert abs(analytic) > 1e-2
    assert diff <= 0.5 * own, (diff, own)


def test_force_is_the_central_difference_of_the_devices_nr_rks(dense):
    """Atom 1 along y, h = 2e-3 and 1e-3 Bohr, 'blyp' on the one-level ladder (the energy is then the dense quadrature the force
    differentiates): |F - FD(h/2)| <= 0.5 |FD(h) - FD(h/2)|."""
    F = pmg.xc_nuc_grad(_device_df(dense.cell, 'one'), 'blyp', dense.dm)
    _fd_check(lambda d: pmg.nr_rks(_device_df(_he_split((1, 1, d)), 'one'), 'blyp', dense.dm)[1], F[1, 1], 'nr_rks blyp atom 1 y')


def test_open_shell_force_is_the_central_difference_of_the_devices_nr_uks(dense):
    """The same for the pair (0.6 D, 0.4 D) and 'blyp': B88 by spin scaling, LYP from the spin-polarised kernel."""
    pair = np.array([0.6 * dense.dm, 0.4 * dense.dm])
    F = pmg.xc_nuc_grad_uks(_device_df(dense.cell, 'one'), 'blyp', pair)
    assert F.shape == (dense.cell.natm, 3)
    _fd_check(lambda d: pmg.nr_uks(_device_df(_he_split((1, 1, d)), 'one'), 'blyp', pair)[1], F[1, 1], 'nr_uks blyp atom 1 y')


def test_ragged_chunks_give_the_default_walks_numbers(dense):
    """e1_grid_chunk = 4099: 28800 = 7 * 4099 + 107, eight chunks with odd lengths and offsets (the scalar path of isdf_gga_aow and of
    isdf_rowdot3) against the one-chunk default, 1e-12 relative; a stack of two matrices on the way."""
    df = _device_df(dense.cell, 'one')
    stack = np.array([dense.dm, make_dm(dense.cell, seed=7)[::-1, ::-1].copy()])
    F, e1 = pmg.xc_nuc_grad(df, 'blyp', stack), pmg.get_vxc_e1(df, 'blyp', stack)
    assert F.shape == (2, dense.cell.natm, 3) and e1.shape == (3, 2) + dense.dm.shape
    df.e1_grid_chunk = 4099
    try:
        Fc, ec = pmg.xc_nuc_grad(df, 'blyp', stack), pmg.get_vxc_e1(df, 'blyp', stack)
    finally:
        df.e1_grid_chunk = 65536
    assert _rel(Fc, F) < 1e-12 and _rel(ec, e1) < 1e-12
