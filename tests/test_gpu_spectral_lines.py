"""The packed spectra from the x-lines their points touch ("line coverage"): isdf_spectral_rows_lines
transforms the listed x-lines only and packs from LDS, isdf_block_invert solves a block's own columns only.  Neither changes
an operation on a value that is kept, so everything here is compared bit for bit (torch.equal on the doubles and on their
int64 views: signed zeros count), the outputs filled with NaN before the call.

The meshes: (10, 12, 16) three different axes, n1 (n2/2+1) = 108 lines = 6.75 tiles of 16: the last tile is ragged;
(12, 12, 15) odd n2, no Nyquist plane; (12, 12, 12) 84 lines = 5.25 tiles; (120, 120, 120) with 2 rows, the pipelined plane
kernel and 16-line tiles of 120 points."""
import types
import numpy as np
import pytest
import torch
import cells

pytestmark = pytest.mark.gpu

MESHES = [(10, 12, 16), (12, 12, 15), (12, 12, 12), (120, 120, 120)]
LISTS = ['sphere_fcc', 'sphere_cubic', 'box', 'point', 'last_line', 'random']
FCC = 3.37 * np.array([[0.0, 1.0, 1.0], [1.0, 0.0, 1.0], [1.0, 1.0, 0.0]])
CUBIC = 6.0 * np.eye(3)


@pytest.fixture(scope='module')
def be():
    from pyscf_isdf_amd.backend import HipBackend
    return HipBackend(0)


def _sphere_list(a, mesh):
    """The shell-sorted list of a build (w_sphere = 100, 256 shells) for the lattice a."""
    from pyscf_isdf_amd.fit_route import FitRouteMixin
    me = types.SimpleNamespace(cell=types.SimpleNamespace(lattice_vectors=lambda: a), w_sphere=100.0, w_sort_bins=256)
    n0, n1, n2 = mesh
    return FitRouteMixin._spectral_point_set(me, np.asarray(mesh), np.ones((n0, n1, n2 // 2 + 1), dtype=bool), None)[0]


def _point_list(kind, mesh):
    """(idx, lines touched as the case wants them, or None where the case is not about their number)"""
    n0, n1, n2 = mesh
    per = n1 * (n2 // 2 + 1)
    rng = np.random.default_rng(n0 + 3 * n1 + 7 * n2)
    if kind == 'sphere_fcc':
        return _sphere_list(FCC, mesh), None
    if kind == 'sphere_cubic':
        return _sphere_list(CUBIC, mesh), None
    if kind == 'box':
        return np.arange(n0 * per), per
    if kind == 'point':
        return np.array([(n0 // 3) * per + per // 2 + 1]), 1
    if kind == 'last_line':
        kx = rng.permutation(n0)[:max(2, n0 // 2)]
        return kx * per + (per - 1), 1
    # two points in five of a random half of the lines, in random order
    half = rng.permutation(per)[:per // 2]
    pts = (np.arange(n0)[:, None] * per + half[None, :]).ravel()
    return rng.permutation(pts)[:2 * len(pts) // 5], None


def _both(be, rows, mesh, idx, ldx, batch):
    """(X of isdf_spectral_rows, X of isdf_spectral_rows_lines, lines touched) on the same rows, list and seeded scales"""
    from pyscf_isdf_amd.fit_route import spectral_line_plan
    idx = np.asarray(idx).astype(np.int32)
    scale = np.random.default_rng(len(idx)).uniform(0.5, 2.0, len(idx))
    lines, slot, slot_scale, nlines = spectral_line_plan(idx, scale, mesh, be.spectral_lines_tile(mesh))
    d_idx, d_scale = be.to_device(idx), be.to_device(scale)
    out = []
    for kw in ({}, dict(lines=be.to_device(lines), slot=be.to_device(slot), slot_scale=be.to_device(slot_scale), nlines=nlines)):
        X = torch.full((rows.shape[0], ldx), float('nan'), dtype=torch.float64, device=rows.device)
        be.spectral_rows(rows, np.asarray(mesh), d_idx, d_scale, X, batch=batch, **kw)
        out.append(X)
    return out[0], out[1], nlines


def _same_bits(a, b):
    return torch.equal(a, b) and torch.equal(a.view(torch.int64), b.view(torch.int64))


@pytest.mark.parametrize('kind', LISTS)
@pytest.mark.parametrize('mesh', MESHES, ids=lambda m: '%dx%dx%d' % m)
def test_lines_entry_is_bitwise_the_plain_one(be, mesh, kind):
    """Every mesh with every list: the sphere lists of an fcc and a cubic cell, the whole box (every line: the fall-through to
    the plain kernels), one point, a few points of the mesh's last line (the one the plain pass holds in its ragged tile; 15 of
    the 16 slots of the listed tile are empty), a fifth of the points in random order.  3 rows in batches of 2 (2 rows at
    120^3), ldx = 2 npts + 6: the padding reads +0.0."""
    n0, n1, n2 = mesh
    per = n1 * (n2 // 2 + 1)
    idx, want_lines = _point_list(kind, mesh)
    touched = len(np.unique(np.asarray(idx) % per))
    # what the case is about, counted on the host before anything runs
    if want_lines is not None:
        assert touched == want_lines
    if kind == 'box':
        assert touched == per                         # no line left out: the plain kernels
    else:
        assert touched * 10 < per * 9                 # lines are left out: the listed pass
    nrows = 2 if n0 == 120 else 3
    rows = be.to_device(np.random.default_rng(5).standard_normal((nrows, n0 * n1 * n2)))
    ldx = 2 * len(idx) + 6
    ref, got, nlines = _both(be, rows, mesh, idx, ldx, 2)
    assert nlines == touched
    assert not torch.isnan(ref).any()
    assert _same_bits(ref[:, 2 * len(idx):], torch.zeros_like(ref[:, 2 * len(idx):]))
    assert _same_bits(got, ref)


@pytest.mark.parametrize('nrows,batch', [(1, 512), (3, 512), (3, 1), (5, 2)])
def test_lines_entry_row_and_batch_edges(be, nrows, batch):
    """One row, three rows in one batch, one row per batch, a last batch that is short; the leading dimension of a build
    (a multiple of 128) on a view of a wider buffer."""
    mesh = (10, 12, 16)
    idx = _sphere_list(FCC, mesh)
    rows = be.to_device(np.random.default_rng(nrows).standard_normal((nrows, 10 * 12 * 16)))
    ldx = -(-2 * len(idx) // 128) * 128 + 128
    ref, got, _ = _both(be, rows, mesh, idx, ldx, batch)
    assert not torch.isnan(ref).any()
    assert _same_bits(got, ref)


def test_a_point_named_twice_has_no_line_plan():
    from pyscf_isdf_amd.fit_route import spectral_line_plan
    assert spectral_line_plan(np.array([5, 9, 5]), np.ones(3), (10, 12, 16), 16) is None


@pytest.mark.parametrize('sizes', [[234, 234, 234], [100, 156], [300], [40], [1, 65, 64]])
def test_block_invert_is_the_forward_solve_of_the_identity(be, sizes):
    """isdf_block_invert (a block's own columns only, the rest zeroed at once) against isdf_block_solve(side 0, trans 0) on an
    explicit identity; D as tests/test_gpu_row_frontier.py builds it."""
    rng = np.random.default_rng(sum(sizes))
    off = np.append(0, np.cumsum(sizes)).astype(np.int32)
    P = int(off[-1])
    D = np.zeros((P, P))
    for b in range(len(sizes)):
        s = slice(off[b], off[b + 1])
        M = rng.standard_normal((sizes[b], sizes[b]))
        D[s, s] = np.linalg.cholesky(M.dot(M.T) + sizes[b] * np.eye(sizes[b]))
    dD = be.to_device(D)
    ref = be.to_device(np.eye(P))
    be.block_solve(dD, off, 0, 0, ref)
    got = torch.full((P, P), float('nan'), dtype=torch.float64, device=ref.device)
    be.block_invert(dD, off, got)
    assert _same_bits(got, ref)


def test_build_is_bitwise_the_one_over_every_line():
    """Diamond primitive cell, gth-dzvp on 24^3, c = 18, the 100 % sphere (w_sphere_tol opened: this coarse mesh does not pass
    the guard), route 'auto' so that the probe runs: ip, X, W and bj_check with and without the plan's lines."""
    from pyscf_isdf_amd.isdf import ISDF
    cell = cells.cell_diamond_prim('gth-dzvp', (24, 24, 24))
    got = []
    for with_lines in (False, True):
        df = ISDF(cell, c_isdf=18, select='refined')
        df.fit_route, df.w_spectral, df.w_sphere, df.w_sphere_tol, df.fft_batch = 'auto', True, 100, np.inf, 256
        df.bj_max_c, df.bj_check_tol, df.w_spectral_check_tol = 18, 1e-5, 1e-5
        df.w_spectral_lines = with_lines
        df.build()
        assert df._fit_state['kind'] == 'blockjacobi-spectral' and df.fit_route_used == 'blockjacobi'
        kw = df._spectral_plan()['lines_kw']
        assert bool(kw) == with_lines
        if with_lines:
            assert kw['nlines'] * 10 < 24 * 13 * 9              # lines are left out: the listed pass ran
        P = len(df.ip)
        X = df._buffer('theta', (P, df._last_spectral_ldx)).clone()
        got.append((df.ip.copy(), X, df.W.clone(), df.bj_check))
    assert np.array_equal(got[0][0], got[1][0])
    assert _same_bits(got[0][1], got[1][1])
    assert _same_bits(got[0][2], got[1][2])
    assert got[0][3] == got[1][3]
