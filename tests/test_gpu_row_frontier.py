"""The spectral build's two frontiers: pair-row products in pieces of full GEMM tiles
(``ISDF.pair_rows_align``), the block apply following on block boundaries.  Element for element the rows are those of the
block-bound pieces - a product's k chain does not depend on its row count, the block apply and the transforms work per block
and per row - so the packed spectrum X and W are compared bit for bit, on a build and on the native entry's edge cases."""
import numpy as np
import pytest
import torch
import cells

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def be():
    from pyscf_isdf_amd.backend import HipBackend
    return HipBackend(0)


@pytest.mark.parametrize('route', ['blockjacobi', 'auto'])
def test_build_is_bitwise_the_block_bound_one(route):
    """Diamond primitive cell, gth-dzvp on 24^3, c = 18: two blocks and more points than one 256-row piece.  The old pieces
    (fft_batch = 256) end on block boundaries; the first new product (256 rows) ends inside the second block, whose head waits
    in the scratch for the second round.  'auto' adds the probe's rows_combine on the applied rows (tolerances opened so that the whole box
    of this coarse mesh keeps the spectral form)."""
    from pyscf_isdf_amd.isdf import ISDF
    cell = cells.cell_diamond_prim('gth-dzvp', (24, 24, 24))
    got = []
    for align in (0, 256):
        df = ISDF(cell, c_isdf=18, select='refined')
        df.fit_route, df.w_spectral, df.w_sphere, df.fft_batch = route, True, 0, 256
        df.bj_max_c, df.bj_check_tol, df.w_spectral_check_tol = 18, 1e-5, 1e-5
        df.pair_rows_align = align
        df.build()
        assert df._fit_state['kind'] == 'blockjacobi-spectral' and df.fit_route_used == 'blockjacobi'
        P = len(df.ip)
        sizes = np.diff(df._fit_state['ip_off'])
        assert df._pair_rows_piece(int(sizes.max())) == align
        assert P > 256 and len(sizes) == 2 and 0 < sizes[0] < 256
        X = df._buffer('theta', (P, df._last_spectral_ldx)).clone()
        got.append((df.ip.copy(), X, df.W.clone(), df.bj_check))
    assert np.array_equal(got[0][0], got[1][0])
    assert torch.equal(got[0][1], got[1][1])
    assert torch.equal(got[0][2], got[1][2])
    if route == 'auto':
        print('bj_check, block-bound pieces %.6e, full tiles %.6e' % (got[0][3], got[1][3]))
        assert got[0][3] <= 1e-5 and got[1][3] <= 1e-5


@pytest.mark.parametrize('sizes', [[234, 234, 234], [100, 156], [300], [40]])
@pytest.mark.parametrize('own', [0, 1])
def test_frontier_entry_edges(be, sizes, own):
    """isdf_pair_rows_frontier in 256-row pieces, blocks applied as they complete, against one whole-block call of
    isdf_pair_rows_block_apply: a boundary inside a piece, one on a piece's end, a block wider than a piece, fewer rows than a
    piece.  Bit for bit on the library (nao 24); with option gemm_nn_own (nao 32) the own NN kernel takes the pieces its tiles
    fit and the square rides the product, decided once for the piece size."""
    rng = np.random.default_rng(sum(sizes))
    nao, n = (32, 3000) if own else (24, 3000)
    off = np.append(0, np.cumsum(sizes)).astype(np.int32)
    P = int(off[-1])
    D = np.zeros((P, P))
    for b in range(len(sizes)):
        s = slice(off[b], off[b + 1])
        M = rng.standard_normal((sizes[b], sizes[b]))
        D[s, s] = np.linalg.cholesky(M.dot(M.T) + sizes[b] * np.eye(sizes[b]))
    dI = be.empty((P, P))
    be.block_invert(be.to_device(D), off, dI)
    aoP, ao = be.to_device(rng.standard_normal((P, nao))), be.to_device(rng.standard_normal((nao, n)))
    be.set_option('gemm_nn_own', own)
    try:
        ref = be.empty((P, n))
        be.pair_rows_block_apply(aoP, ao, n, dI, off, ref)
        piece = 256
        squared = be.pair_rows_squared(aoP, min(piece, P), ao, n)
        assert squared == bool(own and P > 128)
        scratch = torch.full((piece + max(sizes), n), float('nan'), dtype=torch.float64, device=ref.device)
        out = torch.full((P, n), float('nan'), dtype=torch.float64, device=ref.device)
        app = prod = 0
        while app < P:
            new = min(piece, P - prod)
            i = int(np.searchsorted(off, app))
            j = int(np.searchsorted(off, prod + new, side='right')) - 1
            end = int(off[j])
            be.pair_rows_frontier(aoP[prod:prod + new], ao, n, squared, dI[app:, app:], (off[i:j + 1] - app).astype(np.int32),
                                  scratch, prod - app)
            prod += new
            if end > app:
                out[app:end] = scratch[:end - app]
                tail = scratch[end - app:prod - app].clone()
                scratch.fill_(float('nan'))
                scratch[:prod - end] = tail
                app = end
    finally:
        be.set_option('gemm_nn_own', 0)
    if not own:
        assert torch.equal(out, ref)
    else:
        # a ragged last piece falls outside the own kernel's tiles and goes through the library: another k order in a
        # 32-term product, so the bound is the one tests/test_gpu_parity.py holds the fused form itself to
        assert not torch.isnan(out).any() and abs(out - ref).max() <= 1e-12 * abs(ref).max()
