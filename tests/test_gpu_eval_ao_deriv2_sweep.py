"""Sweep of isdf_eval_ao_deriv2 (pyscf_isdf_amd/csrc/eval_ao.hip): the ten planes value, x, y, z, xx, xy, xz, yy, yz, zz on the cell,
the point sets and the sentinel / padded harness of tests/test_gpu_eval_ao_sweep.py (s / p / d / f shells with 4 / 3 / 2 / 2
contractions, 553 images; 'all' = 1320 points in six workgroups with a ragged last one, 'permuted513' whose workgroup boxes span the
cell, 'first100' a single partial workgroup; ld = npts + 3, plane stride nao * ld + 5).

Planes 0 .. 3 come from the same pass of the same shell body as isdf_eval_ao_deriv1's and are compared with them bit for bit.  Planes
4 .. 9 against the numpy restatement tests/ao_deriv2_reference.py (pinned by central differences of the oracle's gradient planes,
tests/test_ao_deriv2_reference.py) at the project's derivative bound TOL_DERIV = 1e-11 * max(1, max|ref|): the float64 restatement's
own error, measured against its np.longdouble evaluation on these points, is
    all: 8.0e-15, permuted513: 8.0e-15, first100: 6.2e-15   (planes of up to 6.3)
- far below 1e-12, so no wider bound is called for."""
import functools
import numpy as np
import pytest
import ao_deriv2_reference as r2
import test_gpu_eval_ao_sweep as sw
from test_gpu_eval_ao_sweep import POINT_SETS, SENTINEL, TOL_DERIV, sweep_cell, points
from pyscf_isdf_amd.lib import IsdfError

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def be():
    from pyscf_isdf_amd.backend import HipBackend
    return HipBackend(0)


@functools.lru_cache(maxsize=None)
def reference(pts):
    """(10, nao, npts) from the restatement, once per point set."""
    cell, Ls, rcut = sweep_cell()
    v = np.ascontiguousarray(r2.eval_ao_deriv2(cell._atm, cell._bas, cell._env, points(pts), Ls, rcut).transpose(0, 2, 1))
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def _got(be, pts):
    """One call into a sentinel-filled buffer with ld = npts + 3 and plane stride nao * ld + 5: (the ten planes (10, nao, npts), whether
    any padding was written)."""
    import torch
    cell, Ls, rcut = sweep_cell()
    coords = points(pts)
    npts, nao = len(coords), cell.nao_nr()
    ld = npts + 3
    plane = nao * ld + 5
    flat = torch.full((10 * plane,), SENTINEL, dtype=torch.float64, device=be.device)
    view = flat.view(10, plane)[:, :nao * ld].unflatten(1, (nao, ld))
    be.eval_ao_deriv2(cell._atm, cell._bas, cell._env, Ls, rcut, be.to_device(np.ascontiguousarray(coords.T)), view)
    host = be.to_host(flat).reshape(10, plane)
    body, tail = host[:, :nao * ld].reshape(10, nao, ld), host[:, nao * ld:]
    clean = bool((body[..., npts:] == SENTINEL).all() and (tail == SENTINEL).all())
    out = np.ascontiguousarray(body[..., :npts])
    out.setflags(write=False)
    return out, clean


@pytest.mark.parametrize('pts', POINT_SETS)
def test_padding_is_untouched(be, pts):
    assert _got(be, pts)[1], 'padding was written'


@pytest.mark.parametrize('pts', POINT_SETS)
def test_planes_0_to_3_are_eval_ao_deriv1_bit_for_bit(be, pts):
    cell, Ls, rcut = sweep_cell()
    body, _ = sw.run(be, cell, Ls, rcut, points(pts), 'eval_ao_deriv1')
    d1 = body[0][..., :len(points(pts))]
    got = _got(be, pts)[0]
    assert got.shape == (10, cell.nao_nr(), len(points(pts)))
    assert np.array_equal(got[:4], d1)


@pytest.mark.parametrize('pts', POINT_SETS)
def test_second_derivative_planes_against_the_restatement(be, pts):
    ref, got = reference(pts), _got(be, pts)[0]
    scale = max(1.0, abs(ref[4:]).max())
    for p in range(4, 10):
        err = abs(got[p] - ref[p]).max()
        print('%s plane %d: error %.3e (max|ref| %.3e)' % (pts, p, err, abs(ref[p]).max()))
        assert abs(ref[p]).max() > 0.1
        assert err < TOL_DERIV * scale
    assert abs(got[:4] - ref[:4]).max() < TOL_DERIV * max(1.0, abs(ref[:4]).max())


def _refused(be, cell, message):
    import torch
    _, Ls, rcut = sweep_cell()
    rc = np.resize(rcut, len(cell._bas))
    nao, G = 200, 8
    d_c = be.to_device(np.ascontiguousarray(points('first100')[:G].T))
    a10 = torch.full((10, nao, G), SENTINEL, dtype=torch.float64, device=be.device)
    with pytest.raises(IsdfError, match=message):
        be.eval_ao_deriv2(cell._atm, cell._bas, cell._env, Ls, rc, d_c, a10)
    assert (be.to_host(a10) == SENTINEL).all()                    # nothing was launched


def test_refuses_l_4(be):
    _refused(be, sw._small_cell([4, [1.2, 1.0]]), 'has l=4; l <= 3 is supported')


def test_refuses_5_contractions(be):
    _refused(be, sw._small_cell([0, [1.2, 0.5, 0.4, 0.3, 0.2, 0.1], [0.6, 0.1, 0.2, 0.3, 0.4, 0.5]]), 'has 5 contractions; at most 4 supported')
