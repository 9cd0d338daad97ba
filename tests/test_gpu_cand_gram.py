"""The per-atom candidate selection with its dot products read from the blocks' Gram triangles (isdf_select_ip_ws with a
workspace, option "cand_gram") against the form that streams the AO slab at every pivot (no workspace) on the same inputs:
rank, pivots and Cholesky rows are compared with np.array_equal - the matrix-core product is the same k-ordered fma chain."""
import numpy as np
import pytest
from pyscf_isdf_amd import gto
from oracle import isdf as oisdf

pytestmark = pytest.mark.gpu

GRAM_LABELS = ('cand_gram_transpose[byte]', 'cand_gram_blocks[flop]', 'select_update_gram_kernel[byte]')
AO_LABEL = 'select_update_kernel[byte]'


@pytest.fixture(scope='module')
def be():
    from pyscf_isdf_amd.backend import HipBackend
    b = HipBackend(0)
    b.prof_enable(True)
    yield b
    b.prof_enable(False)
    b.prof_reset()


def _select(be, aoT, blk_off, nip, work_bytes=None, tie_rtol=1e-10, tol=-1.0):
    """work_bytes None: the AO form.  Returns rank, piv, L (host) and the profile labels the call left."""
    import torch
    kmax = int(max(nip))
    L = be.zeros((kmax, aoT.shape[1]))
    piv = be.empty((len(nip), kmax), dtype=torch.int64)
    work = None if work_bytes is None else be.empty((int(work_bytes) // 8,))
    be.prof_reset()
    rank = be.select_ip(be.to_device(np.ascontiguousarray(aoT)), blk_off, nip, tol, tie_rtol, L, piv, work=work)
    return rank, be.to_host(piv), be.to_host(L), set(be.prof_results())


def _assert_same(got, ref, blk_off, gram_ran):
    rank, piv, L, labels = got
    rank0, piv0, L0, labels0 = ref
    assert np.array_equal(rank, rank0)
    for b in range(len(rank)):
        assert np.array_equal(piv[b, :rank[b]], piv0[b, :rank[b]])
        assert np.array_equal(L[:rank[b], blk_off[b]:blk_off[b + 1]], L0[:rank0[b], blk_off[b]:blk_off[b + 1]])
    assert AO_LABEL in labels0 and not labels0.intersection(GRAM_LABELS)
    if gram_ran:
        assert labels.issuperset(GRAM_LABELS) and AO_LABEL not in labels
    else:
        assert AO_LABEL in labels and not labels.intersection(GRAM_LABELS)


@pytest.fixture(scope='module')
def ragged(be):
    """nao = 37 (K tail: 37 -> 64), blocks that cross 256-row tiles, are no multiple of 16, and one of a single point."""
    rng = np.random.default_rng(5)
    nao = 37
    sizes = [700, 130, 1025, 64, 1]
    nip = [25, 10, 40, 30, 1]
    blk_off = np.append(0, np.cumsum(sizes))
    aoT = rng.standard_normal((nao, blk_off[-1])) * np.exp(-rng.random(blk_off[-1]) * 3)
    need = [be.select_ip_work_bytes(nao, m) for m in sizes]
    return aoT, blk_off, nip, need, _select(be, aoT, blk_off, nip)


def test_ragged_blocks_ample_workspace(be, ragged):
    """All blocks in one group; also the oracle's pivots (and its rows to the 1e-9 of test_select_ip_blocks_match_oracle)."""
    aoT, blk_off, nip, need, ref = ragged
    got = _select(be, aoT, blk_off, nip, sum(need) + 256)
    _assert_same(got, ref, blk_off, True)
    rank, piv, L, _ = got
    for b in range(len(nip)):
        pr, Lr = oisdf.select_ip(aoT[:, blk_off[b]:blk_off[b + 1]], nip[b])
        assert rank[b] == len(pr) and np.array_equal(piv[b, :rank[b]], pr)
        assert abs(L[:rank[b], blk_off[b]:blk_off[b + 1]] - Lr).max() < 1e-9 * abs(Lr).max()


def test_ragged_blocks_workspace_of_the_largest_block(be, ragged):
    """The workspace holds the 1025-point block and nothing beside it.  The greedy grouping of consecutive blocks then
    makes three groups, {700, 130}, {1025}, {64, 1}: a group of one block, and group boundaries on both sides of it (no
    workspace can separate the two small pairs and still hold the largest block)."""
    aoT, blk_off, nip, need, ref = ragged
    assert need[0] + need[1] < max(need) < need[1] + need[2] and need[2] == max(need)
    _assert_same(_select(be, aoT, blk_off, nip, max(need) + 256), ref, blk_off, True)


def test_ragged_blocks_workspace_too_small_falls_back(be, ragged):
    """One block that does not fit sends the whole call down the AO form."""
    aoT, blk_off, nip, need, ref = ragged
    _assert_same(_select(be, aoT, blk_off, nip, max(need) - 4096), ref, blk_off, False)


def test_option_off_takes_the_ao_form(be, ragged):
    aoT, blk_off, nip, need, ref = ragged
    be.set_option('cand_gram', 0)
    try:
        got = _select(be, aoT, blk_off, nip, sum(need) + 256)
    finally:
        be.set_option('cand_gram', 1)
    _assert_same(got, ref, blk_off, False)


def test_ties_lowest_index(be):
    """Three exact copies of 300 columns: every step ties to the last bit in the Gram entries as well."""
    rng = np.random.default_rng(11)
    base = rng.standard_normal((5, 300))
    aoT = np.concatenate([base, base, base], axis=1)
    ref = _select(be, aoT, [0, 900], [12])
    got = _select(be, aoT, [0, 900], [12], be.select_ip_work_bytes(5, 900) + 256)
    _assert_same(got, ref, [0, 900], True)
    assert got[0][0] == 12 and (got[1][0, :12] < 300).all()
    assert np.array_equal(got[1][0, :12], oisdf.select_ip(aoT, 12)[0])


def test_rank_deficient_stops_at_the_same_step(be):
    """3 AOs span 6 pair products: 12 points asked, the tolerance stops both forms (and the oracle) at the same step."""
    rng = np.random.default_rng(3)
    aoT = rng.standard_normal((3, 777))
    ref = _select(be, aoT, [0, 777], [12])
    got = _select(be, aoT, [0, 777], [12], be.select_ip_work_bytes(3, 777) + 256)
    _assert_same(got, ref, [0, 777], True)
    pr = oisdf.select_ip(aoT, 12)[0]
    assert got[0][0] == len(pr) < 12 and np.array_equal(got[1][0, :len(pr)], pr)


def test_zero_rows_padded_or_removed(be):
    """40 rows of which 15 vanish on a block (another 15 on the next block), against the rows packed per block to 25: exact
    zeros inside the K range and in its padding (40 -> 64, 25 -> 32) leave every bit as it was."""
    rng = np.random.default_rng(17)
    sizes = [500, 300]
    blk_off = np.append(0, np.cumsum(sizes))
    nip = [30, 20]
    full = rng.standard_normal((40, 800)) * np.exp(-rng.random(800) * 2)
    packed = np.zeros((25, 800))
    for b in range(2):
        zero = rng.choice(40, 15, replace=False)
        s = slice(blk_off[b], blk_off[b + 1])
        full[zero, s] = 0.0
        packed[:, s] = full[np.setdiff1d(np.arange(40), zero), s]
    ref = _select(be, packed, blk_off, nip)
    for x in (full, packed):
        need = sum(be.select_ip_work_bytes(x.shape[0], m) for m in sizes)
        _assert_same(_select(be, x, blk_off, nip, need + 256), ref, blk_off, True)


def test_end_to_end_same_points_and_exchange(be):
    """The 8-He cell of test_candidate_stage_skips_rows_that_vanish_on_a_block_without_changing_the_points (mesh 30^3, c = 6,
    refined) with df.cand_gram off and on: df.ip and vk equal to the last bit, and the Gram form really ran."""
    from pyscf_isdf_amd.isdf import ISDF
    atoms = '; '.join('He %g %g %g' % (x, y, z) for x in (0.3, 4.2) for y in (0.1, 4.4) for z in (0.2, 4.1))
    cell = gto.Cell(atom=atoms, basis={'He': [[0, [2.2, 1]], [0, [1.1, 1]], [1, [1.6, 1]]]}, a=np.eye(3) * 8.0, mesh=[30] * 3)
    nao = cell.nao_nr()
    rng = np.random.default_rng(5)
    dm = rng.standard_normal((nao, nao)); dm = dm + dm.T
    out = {}
    for flag in (False, True):
        df = ISDF(cell, c_isdf=6, select='refined', backend=be)
        df.cand_gram = flag
        be.prof_reset()
        vk = df.get_jk(dm, with_j=False)[1]
        out[flag] = (df.ip.copy(), vk, set(be.prof_results()))
    assert AO_LABEL in out[False][2] and not out[False][2].intersection(GRAM_LABELS)
    assert out[True][2].issuperset(GRAM_LABELS) and AO_LABEL not in out[True][2]
    assert np.array_equal(out[False][0], out[True][0])
    assert np.array_equal(out[False][1], out[True][1])
