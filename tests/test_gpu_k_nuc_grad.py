"""get_k_nuc_grad / get_jk_nuc_grad on the device.  Cell: diamond primitive, gth-dzvp, 12^3, c_isdf = 4 'local' (26 AOs, P = 104),
robust_k; the exact limit on gth-szv 'global' c_isdf = 5 (tests/test_jk_e1.py).

The contracted route and the host contraction of the device's own get_k_e1 are two float64 orders of one sum, so their mismatch
is measured and the bound is ten times the measured value, relative to max|f| (a bound above 1e-10 would mean a defect, not
rounding).  Measured on an MI355X, relative to max|f|: contracted route against the matrix route 5.6e-15 (low rank), 3.8e-15
(non-symmetric), 7.2e-15 ('occ'); the one launch against the composition 2.9e-16; chunks of 500 and batches of 40 against the
defaults 5.7e-16; exact limit: plain K mismatch 5.9e-15 of max|K|, force against the exact restatement contracted 1.1e-14."""
import numpy as np
import pytest
import e1_reference as e1
from oracle import isdf as oisdf, fftdf
from test_gpu_jk_e1 import _Product
from test_k_nuc_grad import contract, _rel

gpu = pytest.mark.gpu

FUSED = 'gemm_nn_had_kernel[flop]'
ROUTE_BOUND = 7.2e-14            # 10 x the largest measured mismatch of the contracted and the matrix route (module docstring)
ORDER_BOUND = 5.7e-15            # 10 x the largest measured mismatch of two orders of the contracted route itself


def _labels(df, fn):
    be = df.backend
    be.prof_enable(True)
    be.prof_reset()
    try:
        out = fn()
        return out, set(be.prof_results())
    finally:
        be.prof_enable(False)


@pytest.fixture(scope='module')
def prod():
    p = _Product('gth-dzvp', 4)
    assert p.nao == 26 and len(p.df.ip) == 104
    p.fk, p.fk_labels = _labels(p.df, lambda: p.df.get_k_nuc_grad(p.dm))
    return p


@gpu
def test_device_contracted_route_equals_the_matrix_route(prod):
    p, df = prod, prod.df
    assert p.fk.shape == (p.cell.natm, 3) and 'S8_get_k_nuc_grad' in df.timings
    assert FUSED in p.fk_labels, sorted(p.fk_labels)
    worst = 0.0
    for name, dm in (('low rank', p.dm), ('non-symmetric', p.dn)):
        sym = 0.5 * (dm + dm.T)
        f = df.get_k_nuc_grad(dm)
        m = _rel(f, contract(p.cell, df.get_k_e1(sym), sym))
        print('device %-14s |contracted - matrix| / max = %.3e' % (name, m))
        worst = max(worst, m)
    print('device: largest mismatch of the two routes %.3e' % worst)
    assert worst <= ROUTE_BOUND


@gpu
def test_device_fused_against_composition_chunks_and_batches(prod):
    p, df = prod, prod.df
    df.k_grad_fused = False
    try:
        fc, labels = _labels(df, lambda: df.get_k_nuc_grad(p.dm))
    finally:
        df.k_grad_fused = True
    assert FUSED not in labels and 'hadamard_rows_kernel[byte]' in labels, sorted(labels)
    m = _rel(p.fk, fc)
    print('device: |fused - composition| / max = %.3e' % m)
    assert m <= ORDER_BOUND
    df.e1_grid_chunk, df.e1_row_batch = 500, 40                   # 1728 = 3 * 500 + 228, 104 = 2 * 40 + 24
    try:
        fb, labels = _labels(df, lambda: df.get_k_nuc_grad(p.dm))
    finally:
        df.e1_grid_chunk, df.e1_row_batch = 65536, None
    assert FUSED in labels, sorted(labels)                        # batches of 40: a fused prefix of 32 points, a composed tail of 8
    m = _rel(fb, p.fk)
    print('device: |chunks of 500, batches of 40 - defaults| / max = %.3e' % m)
    assert m <= ORDER_BOUND


@gpu
def test_device_stack_and_the_pair_of_calls(prod):
    p, df = prod, prod.df
    stack = np.array([p.dm, p.dn])
    fs = df.get_k_nuc_grad(stack)
    assert fs.shape == (2, p.cell.natm, 3)
    assert _rel(fs[0], p.fk) <= ORDER_BOUND and _rel(fs[1], df.get_k_nuc_grad(p.dn)) <= ORDER_BOUND
    fj, fk = df.get_jk_nuc_grad(p.dm)
    assert np.array_equal(fj, df.get_j_nuc_grad(p.dm)) and _rel(fk, p.fk) <= ORDER_BOUND
    assert _rel(fj, contract(p.cell, p.vj, p.dm)) < 1e-10          # the bound of the J side in tests/test_gpu_jk_e1.py
    assert _rel(df.get_k_nuc_grad(p.dm, exxdiv='ewald'), p.fk) <= ORDER_BOUND


@gpu
def test_device_exact_limit():
    """gth-szv 'global' c_isdf = 5: the force against the exact restatement contracted, within ten times the plain K's mismatch
    against the exact exchange measured in the same run."""
    from test_jk_e1 import EXACT_C
    p = _Product('gth-szv', EXACT_C, select='global')
    df = p.df
    k_isdf = oisdf.get_k(df.backend.to_host(df.aoP), df.backend.to_host(df.W), p.dm)
    mismatch = _rel(k_isdf, fftdf.get_k(p.ao4[0], p.dm, p.a, p.mesh))
    err = _rel(df.get_k_nuc_grad(p.dm), contract(p.cell, e1.get_k_e1(p.ao4, p.dm, p.a, p.mesh), p.dm))
    print('device, c_isdf = %d global: P = %d, plain K mismatch %.3e, force mismatch %.3e' % (EXACT_C, len(df.ip), mismatch, err))
    assert mismatch < 1e-9
    assert err <= 10 * mismatch


@gpu
def test_device_occ_pair_space():
    p = _Product('gth-dzvp', 4, pair_space='occ')
    df = p.df
    f = df.get_k_nuc_grad(p.dm)
    assert df._fit_dm is not None
    m = _rel(f, contract(p.cell, df.get_k_e1(p.dm), p.dm))
    print("device 'occ': |contracted - matrix| / max = %.3e" % m)
    assert m <= ROUTE_BOUND
