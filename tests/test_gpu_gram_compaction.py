"""The final pick (isdf_select_ip_gram) with the stored order compacted onto the candidates not yet pivoted, against the
same pick on the whole matrix and against the oracle restatement: identical pivots (original candidate indices) and rank."""
import numpy as np
import pytest
from oracle import isdf as oisdf

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def be():
    from pyscf_isdf_amd.backend import HipBackend
    return HipBackend(0)


def _gram_with_duplicates(seed, nao, m, ndup):
    """(ao^T ao)^2 on m columns of which ndup are exact copies of others, scattered: exact ties on the diagonal."""
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((nao, m - ndup)) * np.exp(-2.0 * rng.random(m - ndup))
    ao = np.concatenate([base, base[:, rng.integers(0, m - ndup, ndup)]], axis=1)[:, rng.permutation(m)]
    return ao.T.dot(ao) ** 2


def _pick(be, A, nip, panel, compact, permille=875):
    """(rank, pivots, number of compactions the pick made, from the library's profiler)"""
    import torch
    be.set_option('gram_compact', int(compact))
    be.set_option('gram_compact_permille', permille)
    be.prof_reset()
    be.prof_enable(True)
    try:
        piv = be.empty((nip,), dtype=torch.int64)
        r = be.select_ip_gram(be.to_device(A), nip, -1.0, 1e-10, piv, panel=panel)
        ent = be.prof_results().get('gram_compact[byte]')
    finally:
        be.prof_enable(False)
        be.prof_reset()
        be.set_option('gram_compact', 1)
        be.set_option('gram_compact_permille', 875)
    return r, be.to_host(piv)[:r], (ent['launches'] if ent else 0)


@pytest.mark.parametrize('m,nao,nip,panel,permille,ncompact', [(4500, 60, 1100, 256, 1000, 4), (4500, 60, 1100, 64, 1000, 17),
                                                               (4500, 60, 1100, 256, 875, 1), (9001, 80, 1300, 256, 1000, 5)])
def test_compacted_pick_matches_whole_matrix_and_oracle(be, m, nao, nip, panel, permille, ncompact):
    """permille = 1000 compacts after every panel but the last, 875 is the default threshold (one compaction at m = 4500: after
    panel 3, 3732 columns remain of 4500); m = 9001 is ragged against the 256-column workgroups and the 2048-column strips.  A
    fifth of the columns duplicate others: the lowest original index must win every exact tie, as on the whole matrix."""
    A = _gram_with_duplicates(m + nip, nao, m, m // 5)
    r_off, piv_off, n_off = _pick(be, A, nip, panel, compact=False)
    r_on, piv_on, n_on = _pick(be, A, nip, panel, compact=True, permille=permille)
    assert n_off == 0 and n_on == ncompact
    assert r_on == r_off == nip
    assert np.array_equal(piv_on, piv_off)
    assert len(set(piv_on.tolist())) == r_on and piv_on.min() >= 0 and piv_on.max() < m
    pr, _ = oisdf.pivoted_cholesky_gram(A, nip)
    assert np.array_equal(piv_on, pr)


def test_compacted_pick_stops_at_the_rank(be):
    """A rank-deficient matrix (nao = 6: 21 independent pair products) stops at its rank with compaction after every panel of
    4; the pivots of the last stretch are translated to original indices too."""
    A = _gram_with_duplicates(5, 6, 2100, 300)
    r_off, piv_off, _ = _pick(be, A, 50, 4, compact=False)
    r_on, piv_on, n_on = _pick(be, A, 50, 4, compact=True, permille=1000)
    assert n_on == 5
    pr, _ = oisdf.pivoted_cholesky_gram(A, 50)
    assert r_on == r_off == len(pr) == 21
    assert np.array_equal(piv_on, piv_off) and np.array_equal(piv_on, pr)
