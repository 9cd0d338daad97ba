"""Sweep of the layer that turns the kernels into J and K (csrc/jk.hip, csrc/kpts.hip, the symmetrisers of csrc/coulomb.hip,
isdf_rho_pair / isdf_dot of csrc/multigrid.hip) over every chunk edge, window, tile edge and stride.

The older tests reach these entries through drivers on cells of fewer than 32768 grid points, with one Hadamard pass (P = 300) and
contiguous buffers, and compare at chemical accuracy.  This module drives HipBackend directly:

  A  isdf_rho / isdf_rho_pair / isdf_rho_k over ng = 1, 255, 256, 257, 32767, 32768, 32769, 65573 (the 32768-column passes JCHUNK /
     RCHUNK / CH: one pass, exactly one, a ragged second, two full passes and a ragged third), nao = 1, 5, 33, nset = 1, 3, ld = ng + 0 /
     1 / 6, ldrho > ng; isdf_vj_from_vR / isdf_vj_k over ng = 1, 63, 257, 32769 (the four-call composition and its signs)
  B  isdf_get_k over P = 1, 300, 4095, 4096, 4097 (Hadamard passes of 4096 rows), at P = 4097 over windows that start past row 0, end
     at the pass edge, hold one row or none, at P = 4099 over a window that starts past row 0 and still takes two passes; W a
     non-symmetric view with ldw = P + 3
  C  isdf_get_k_pair over P = 1, 37, 256, 300 x nao = 1, 5, 18 on complex integers, and P = 1100 (P^2 past one grid-stride round of the
     Hadamard kernel)
  D  isdf_hadamard_rows / isdf_zhadamard_planes (row and column edges, the refusal of 65536 rows), the mirror and mean kernels and
     isdf_finish_Wq over P = 1, 2, 31, 32, 33, 63, 64, 65, 100 (ragged 32 x 32 tiles, the in-place diagonal tile) x ldw = P, P + 1,
     P + 5, isdf_dot over n = 1 ... 1 000 003 (past 1024 x 256)
  E  the entries that contain a transform - isdf_get_j and its three pieces, isdf_coulG_half, isdf_get_k_exact, isdf_get_k_exact_kpt
     (pass loops x windows), isdf_nyquist_spectra, and the hipFFT forms of isdf_coulomb_rows / isdf_coulomb_rows_q past one
     grid-stride round of their element-wise kernels - against numpy.fft in complex128 plus an exact contraction.

Conventions.  A to D are EXACT: operands are small integers held as doubles (|x| <= 3, complex ones per component), sized so that every
partial sum is an integer below 2^53 (each docstring states its largest magnitude), so the float64 / int64 numpy contraction IS the
answer in any summation order and np.array_equal has no tolerance.  Every output buffer is prefilled with NaN (or, where the entry
accumulates, with a known integer field) and is one element wider than the result: padding columns, rows outside a window and the
guard element must be NaN afterwards; inputs must be bit-unchanged.  Strided forms are views big[:, :n] of wider NaN-filled tensors
with even and odd paddings.  Which transform ran is read from the profiling labels.  Failing cases are collected per test and
reported together.

Bound for E.  The project's convolution bound is TOL = 1e-12 of max|ref| (test_gpu_fft_sweep.py).  Propagated through the exact
contraction that follows the convolution V, an output element sum_g V(g) a_i(g) b_j(g) may be off by
    |got - ref| <= 1e-12 max|V| sum_g |a_i(g)| |b_j(g)|
(for the exchange entries: weight x sum_g sum_j |mo_j(g)| |ao_l(g)|), computed from the reference's own intermediates.  Plain
transforms (potential, spectra, convolved rows) are held to TOL of max|ref| itself, the kernel table to 1e-12 of its largest entry
(the bound of test_coulG_q_kernel_matches_reference_pins_and_oracle).

Measured on an MI355X (256 CUs), largest error / bound per entry (1.0 would be the bound):

  entry                          largest error / bound
  isdf_get_j                     2.49e-04  (32, 32, 33)
  isdf_coulomb_potential         1.34e-03  (32, 32, 33)
  isdf_coulG_half                3.14e-04  (32, 32, 33)
  isdf_get_k_exact               2.31e-04  (12, 10, 9), max_rows 3, window (0, 7)
  isdf_get_k_exact_kpt           6.17e-04  (9, 8, 7), max_rows 3, window (0, 7)
  isdf_nyquist_spectra           3.25e-04  (6, 5, 4), axis 2, 5 rows
  isdf_coulomb_rows (hipFFT)     1.14e-03  row 638 of 1041
  isdf_coulomb_rows_q (hipFFT)   8.17e-04  row 529 of 607

Every case stays three orders under its bound; the covers of isdf_get_k_exact / _kpt give the bits of the full call for every
max_rows, also where the window changes the number of AO rows per pass.

Found and fixed: nothing.  All 17 tests passed on the first run against the unchanged kernels (11 s inside the suite, 18 s for the
module alone with the start of the process); the source change is the header, which now states what the tests pin (overwrite
versus accumulate, which rows are written, the diagonal of Wim, the refusals).

Mutations tried on a scratch copy (not committed), each arithmetic only and inside its buffers:
  - rho_reduce_kernel / rho_k_reduce_kernel given ld for the stride of the workspace T (run at ng <= 257 only, where that stays
    inside the workspace): test_A_rho fails in 36 and test_A_rho_k in 36 of the 54 cases left (all with nao > 1).
  - isdf_get_k always with beta = 0: test_B_get_k_windows fails at P = 4097, window (0, 4097), and in its three covers (and only
    there, as it has to: every other listed window is one pass).
  - mirror_upper_sign_kernel writing r >= cc: test_D_symmetrize_upper_and_hermitian fails in the imaginary plane for every P and ldw
    (the diagonal of Wim changes sign).
  - finish_Wq_kernel with the sign of fi flipped: test_D_finish_Wq fails for every P > 1 and both kinds of phases (P = 1 passes, and
    has to: fi = 0 on the diagonal).
  - pair_reduce_cplx_kernel without the conjugate: test_E_get_k_exact_kpt fails in all its cases, error / bound 2e11.
  - isdf_dot's block cap 512 instead of 1024: test_D_dot passes, as it has to - it pins values, not launch shapes.
  - one more library with a mutation for every test the six above do not reach: the g0 offset of aoA dropped in isdf_rho_pair
    (test_A_rho_pair: 21 of the 24 cases past 32768 columns), the sign of the fourth product of isdf_vj_k (test_A_vj_from_vR_and_vj_k),
    W read with leading dimension P in isdf_get_k (test_B_get_k_windows, every P > 1), the first grid-stride round only in
    zhadamard_kernel (test_C_get_k_pair_past_one_grid_stride_round; test_C_get_k_pair passes, as it has to) and in mul_full_kernel /
    mul_half_kernel (test_E_hipfft_forms_past_one_grid_stride_round: exactly the last row of each), the last column past 256
    skipped in hadamard_rows_kernel (test_D_hadamard_rows_and_zhadamard_planes: cols 257 and 1000), the lower tile of
    mean_symmetric_kernel not transposed (test_D_symmetrize_mean: every P > 32), rows written from the top of vk in
    isdf_get_k_exact (test_E_get_k_exact: every window past row 0), every second pair skipped in nyquist_reduce_kernel
    (test_E_nyquist_spectra: the axes longer than 2).  The eight tests whose kernels it leaves alone pass.
"""
import ctypes
import numpy as np
import pytest
import torch
from oracle import pbc_tools as otools

pytestmark = pytest.mark.gpu

NAN = float('nan')
A_TRI = np.array([[4.1, 0.3, -0.2], [0.5, 3.7, 0.4], [-0.3, 0.6, 4.4]])     # the triclinic lattice of test_gpu_fft_sweep.py
TOL = 1e-12                                                                 # convolutions, relative to max|ref| (same module)
NGS = (1, 255, 256, 257, 32767, 32768, 32769, 65536 + 37)
NGS_VJ = (1, 63, 257, 32769)
PADS = (0, 1, 6)
TILE_PS = (1, 2, 31, 32, 33, 63, 64, 65, 100)
MESHES = ((6, 5, 4), (9, 8, 7), (12, 10, 9), (32, 32, 33))                  # G = 33792 of the last one crosses a 32768 chunk
# the k-point exchange makes a hipFFT plan (0.3 - 0.7 s) per (mesh, rows of a pass): less than one workgroup of grid points, a
# ragged second one, and the large mesh
MESHES_KPT = ((6, 5, 4), (9, 8, 7), (32, 32, 33))
OWN_CONV = {'coulomb_conv_own_3pass[byte]', 'coulomb_conv_own_5pass[byte]'}
HIPFFT_CONV = 'coulomb_conv_d2z_mul_z2d[byte]'
HIPFFT_CONV_Q = 'coulomb_conv_z2z[byte]'
OWN_CONV_Q = 'coulomb_conv_q_own[byte]'
EXACT_KPT = 'exact_k_kpt_pairs[byte]'
FFT_LABELS = OWN_CONV | {HIPFFT_CONV, HIPFFT_CONV_Q, OWN_CONV_Q, EXACT_KPT}


@pytest.fixture(scope='module')
def be():
    from pyscf_isdf_amd.backend import HipBackend
    b = HipBackend(0)
    b.prof_enable(True)
    yield b
    b.prof_enable(False)
    b.prof_reset()
    b.set_option('own_fft', 2)
    b.release_workspace()


# ---- helpers ------------------------------------------------------------------------------------------------------------------
def _ints(rng, shape, lim=3):
    return rng.integers(-lim, lim + 1, shape).astype(np.float64)


def _cints(rng, shape, lim=3):
    return _ints(rng, shape, lim) + 1j * _ints(rng, shape, lim)


def _wide(be, a, pad):
    """(big, view): a NaN-filled device tensor of pad more columns than the 2-D host array a, and its view big[:, :n] holding a."""
    rows, n = a.shape
    big = torch.full((rows, n + pad), NAN, dtype=torch.float64, device=be.device)
    view = big[:, :n]
    view.copy_(be.to_device(a))
    return big, view


def _flat(be, shape, dtype=torch.float64):
    """(buf, view): a NaN-filled flat device buffer of one element more than ``shape`` holds, and its contiguous view of that shape."""
    n = int(np.prod(shape))
    fill = complex(NAN, NAN) if dtype == torch.complex128 else NAN
    buf = torch.full((n + 1,), fill, dtype=dtype, device=be.device)
    return buf, buf[:n].view(*shape)


def _snap(be, *tensors):
    return [be.to_host(t).copy() for t in tensors]


def _unchanged(be, tensors, snaps):
    return all(np.array_equal(be.to_host(t), s, equal_nan=True) for t, s in zip(tensors, snaps))


def _nan_outside(host, ncols):
    """Columns ncols.. of a host array are all NaN."""
    return bool(np.all(np.isnan(host[..., ncols:])))


def _labels(be, fn):
    be.prof_reset()
    out = fn()
    return out, set(be.prof_results())


def _report(fails):
    assert not fails, '%d failing cases:\n%s' % (len(fails), '\n'.join(map(str, fails[:60])))


def _ncu(be):
    return torch.cuda.get_device_properties(be.device).multi_processor_count


# ---- A: density and potential contractions ----------------------------------------------------------------------------------
def test_A_rho(be):
    """isdf_rho = sum_mn dm[i, m, n] ao[m, g] ao[n, g], overwriting rows of leading dimension ldrho.  |ao|, |dm| <= 3, nao <= 33:
    |dm ao| <= 297 and |rho| <= 33 * 297 * 3 < 2^15, all integers."""
    fails = []
    for ng in NGS:
        for nao in (1, 5, 33):
            rng = np.random.default_rng([1, ng, nao])
            ao = _ints(rng, (nao, ng))
            dms = {nset: _ints(rng, (nset, nao, nao)) for nset in (1, 3)}
            want = {nset: np.einsum('img,mg->ig', dms[nset] @ ao, ao) for nset in dms}
            for pad in PADS:
                big, view = _wide(be, ao, pad)
                snap = _snap(be, big)
                for nset in (1, 3):
                    d_dm = be.to_device(dms[nset])
                    out = torch.full((nset, ng + 1 + pad), NAN, dtype=torch.float64, device=be.device)
                    be.rho(view, ng, d_dm, out[:, :ng])
                    got = be.to_host(out)
                    case = ('ng', ng, 'nao', nao, 'nset', nset, 'ld', ng + pad, 'ldrho', ng + 1 + pad)
                    if not np.array_equal(got[:, :ng], want[nset]):
                        bad = np.argwhere(got[:, :ng] != want[nset])
                        fails.append(case + ('%d wrong, first at %s' % (len(bad), bad[0]),))
                    if not _nan_outside(got, ng):
                        fails.append(case + ('padding / guard written',))
                    if not np.array_equal(be.to_host(d_dm), dms[nset]):
                        fails.append(case + ('dm changed',))
                if not _unchanged(be, [big], snap):
                    fails.append(('ng', ng, 'nao', nao, 'ld', ng + pad, 'ao changed'))
    _report(fails)


def test_A_rho_pair(be):
    """isdf_rho_pair = sum_(m < nA, n < nB) aoA[m, g] dm[i, m, n] aoB[n, g] with nA != nB, both row blocks of one AO buffer.
    |rho| <= 7 * 3 * 9 * 3 < 2^10."""
    fails = []
    for ng in NGS:
        for nA, nB in ((3, 7), (7, 3)):
            rng = np.random.default_rng([2, ng, nA])
            ao = _ints(rng, (nA + nB, ng))
            dms = {nset: _ints(rng, (nset, nA, nB)) for nset in (1, 3)}
            want = {nset: np.einsum('img,mg->ig', dms[nset] @ ao[nA:], ao[:nA]) for nset in dms}
            for pad in PADS:
                big, view = _wide(be, ao, pad)
                snap = _snap(be, big)
                for nset in (1, 3):
                    out = torch.full((nset, ng + 1 + pad), NAN, dtype=torch.float64, device=be.device)
                    be.rho_pair(view[:nA], view[nA:], ng, be.to_device(dms[nset]), out[:, :ng])
                    got = be.to_host(out)
                    case = ('ng', ng, 'nA, nB', nA, nB, 'nset', nset, 'ld', ng + pad)
                    if not np.array_equal(got[:, :ng], want[nset]):
                        bad = np.argwhere(got[:, :ng] != want[nset])
                        fails.append(case + ('%d wrong, first at %s' % (len(bad), bad[0]),))
                    if not _nan_outside(got, ng):
                        fails.append(case + ('padding / guard written',))
                if not _unchanged(be, [big], snap):
                    fails.append(('ng', ng, 'nA, nB', nA, nB, 'ld', ng + pad, 'ao changed'))
    _report(fails)


def test_A_rho_k(be):
    """isdf_rho_k ACCUMULATES rho[g] += scale Re sum_ij D_ij u_i(g) conj(u_j(g)) with D^T given as two independent, non-symmetric
    planes; scale = -2 on an integer prefill, and a second call adds the same again.  |D^T u| <= 2 * 297 per component,
    |sum| <= 33 * 2 * 594 * 3 < 2^17."""
    fails = []
    for ng in NGS:
        for nao in (1, 5, 33):
            rng = np.random.default_rng([3, ng, nao])
            u = _cints(rng, (nao, ng))
            DT = _cints(rng, (nao, nao))
            D = DT.T
            rho0 = _ints(rng, ng, 50)
            s = np.einsum('jg,jg->g', D.T @ u, u.conj()).real            # sum_ij D_ij u_i conj(u_j), T_j = sum_i D_ij u_i
            d_DTr, d_DTi = be.to_device(DT.real.copy()), be.to_device(DT.imag.copy())
            for pad in PADS:
                bigr, ur = _wide(be, u.real.copy(), pad)
                bigi, ui = _wide(be, u.imag.copy(), pad)
                snap = _snap(be, bigr, bigi, d_DTr, d_DTi)
                buf = torch.full((ng + 1,), NAN, dtype=torch.float64, device=be.device)
                buf[:ng] = be.to_device(rho0)
                case = ('ng', ng, 'nao', nao, 'ld', ng + pad)
                for call in (1, 2):
                    be.rho_k(ur, ui, ng, d_DTr, d_DTi, -2.0, buf[:ng])
                    got = be.to_host(buf)
                    want = rho0 - 2.0 * call * s
                    if not np.array_equal(got[:ng], want):
                        bad = np.flatnonzero(got[:ng] != want)
                        fails.append(case + ('call %d' % call, '%d wrong, first at %d' % (len(bad), bad[0])))
                    if not np.isnan(got[ng]):
                        fails.append(case + ('guard written',))
                if not _unchanged(be, [bigr, bigi, d_DTr, d_DTi], snap):
                    fails.append(case + ('inputs changed',))
    _report(fails)


def test_A_vj_from_vR_and_vj_k(be):
    """isdf_vj_from_vR: vj[s] = einsum('ig,g,jg->ij', ao, vR[s], ao) with ldv > ng; isdf_vj_k: vj_ij = sum_g conj(u_i) vR u_j in two
    planes (four scaled NT products and their signs).  |terms| <= 3 * 3 * 18 (complex), sums over 32769 points < 2^23."""
    fails = []
    for ng in NGS_VJ:
        for nao in (1, 5, 33):
            rng = np.random.default_rng([4, ng, nao])
            u = _cints(rng, (nao, ng))
            ao = u.real.copy()
            vR = _ints(rng, (3, ng))
            want_k = (u.conj() * vR[0]) @ u.T                            # einsum('ig,g,jg->ij', conj(u), vR, u)
            for pad in PADS:
                bigr, ur = _wide(be, ao, pad)
                bigi, ui = _wide(be, u.imag.copy(), pad)
                for nset in (1, 3):
                    bigv, vv = _wide(be, vR[:nset], pad + 2)
                    snap = _snap(be, bigr, bigv)
                    buf, vj = _flat(be, (nset, nao, nao))
                    be.vj_from_vR(ur, ng, vv, vj)
                    got = be.to_host(buf)
                    want = (ao[None] * vR[:nset, None, :]) @ ao.T            # einsum('ig,sg,jg->sij', ao, vR, ao)
                    case = ('vj_from_vR', 'ng', ng, 'nao', nao, 'nset', nset, 'ld', ng + pad)
                    if not np.array_equal(got[:-1].reshape(want.shape), want):
                        fails.append(case + ('wrong values',))
                    if not np.isnan(got[-1]):
                        fails.append(case + ('guard written',))
                    if not _unchanged(be, [bigr, bigv], snap):
                        fails.append(case + ('inputs changed',))
                d_v = be.to_device(vR[0].copy())
                snap = _snap(be, bigr, bigi, d_v)
                bre, vre = _flat(be, (nao, nao))
                bim, vim = _flat(be, (nao, nao))
                be.vj_k(ur, ui, ng, d_v, vre, vim)
                gre, gim = be.to_host(bre), be.to_host(bim)
                case = ('vj_k', 'ng', ng, 'nao', nao, 'ld', ng + pad)
                got_k = gre[:-1].reshape(nao, nao) + 1j * gim[:-1].reshape(nao, nao)
                if not np.array_equal(got_k, want_k):
                    fails.append(case + ('wrong values',))
                if not (np.isnan(gre[-1]) and np.isnan(gim[-1])):
                    fails.append(case + ('guard written',))
                if not _unchanged(be, [bigr, bigi, d_v], snap):
                    fails.append(case + ('inputs changed',))
    _report(fails)


# ---- B: isdf_get_k --------------------------------------------------------------------------------------------------------------
PMAX = 4099
# (row0, nrows) per P, the full window first; P = 4097: two passes from row 0, one pass that starts past row 0 and ends at the pass
# edge or at P, the single row of the second pass, no row; P = 4099: a window that starts past row 0 AND takes two passes
GET_K_WINDOWS = {1: ((0, 1),), 300: ((0, 300), (0, 100), (100, 200)), 4095: ((0, 4095),), 4096: ((0, 4096),),
                 4097: ((0, 4097), (1, 4096), (0, 4096), (3, 4094), (4096, 1), (2000, 0), (0, 1), (0, 3)),
                 4099: ((0, 4099), (2, 4097), (0, 2))}
GET_K_COVERS = {300: (((0, 100), (100, 200)),), 4097: (((0, 4096), (4096, 1)), ((0, 1), (1, 4096)), ((0, 3), (3, 4094))),
                4099: (((0, 2), (2, 4097)),)}


@pytest.fixture(scope='module')
def bigW(be):
    """One integer field of 4099 x 4102 doubles (134.5 MB) on the host and on the device, and a device buffer of the same size in
    which every P carves its (P, P + 3) matrix: the W of P rows is the first P (P + 3) entries of the field."""
    base = _ints(np.random.default_rng(41), PMAX * (PMAX + 3))
    d_base = be.to_device(base)
    yield base, d_base, torch.empty_like(d_base)
    del d_base
    be.empty_cache()


def test_B_get_k_windows(be, bigW):
    """isdf_get_k = aoP^T [(aoP dm aoP^T) .* W][window] aoP, overwriting all of vk for every set; nrows = 0 gives exact zeros.  nao = 6,
    nset = 2, W non-symmetric with ldw = P + 3 and NaN in the padding, dm non-symmetric.  |aoP dm aoP^T| <= 6 * 54 * 3 = 972, times W
    2916, times aoP summed over 4099 points < 3.6e7, the outer sum over 4099 points < 4.5e11 < 2^53."""
    base, d_base, d_work = bigW
    fails = []
    nao, nset = 6, 2
    for P in sorted(GET_K_WINDOWS):
        rng = np.random.default_rng([5, P])
        aoP = _ints(rng, (P, nao))
        dms = _ints(rng, (nset, nao, nao))
        n = P * (P + 3)
        W = base[:n].reshape(P, P + 3)[:, :P]
        d_work[:n].copy_(d_base[:n])
        d_Wbig = d_work[:n].view(P, P + 3)
        d_Wbig[:, P:] = NAN
        d_W = d_Wbig[:, :P]
        Z = np.stack([(((aoP @ dms[i]) @ aoP.T) * W) @ aoP for i in range(nset)])      # (nset, P, nao): Hadamard rows times aoP
        d_aoP, d_dm = be.to_device(aoP), be.to_device(dms)
        got = {}
        for row0, nrows in GET_K_WINDOWS[P]:
            buf, vk = _flat(be, (nset, nao, nao))
            be.get_k(d_aoP, d_W, row0, nrows, d_dm, vk)
            h = be.to_host(buf)
            got[row0, nrows] = h[:-1].reshape(nset, nao, nao)
            want = np.einsum('pm,spn->smn', aoP[row0:row0 + nrows], Z[:, row0:row0 + nrows])
            if not np.array_equal(got[row0, nrows], want):
                fails.append(('P', P, 'window', (row0, nrows), 'wrong values, max |diff| %s' % np.nanmax(abs(got[row0, nrows] - want))))
            if nrows == 0 and not np.all(got[row0, nrows] == 0.0):
                fails.append(('P', P, 'window', (row0, nrows), 'not zeroed'))
            if not np.isnan(h[-1]):
                fails.append(('P', P, 'window', (row0, nrows), 'guard written'))
        for cover in GET_K_COVERS.get(P, ()):
            if not np.array_equal(sum(got[w] for w in cover), got[0, P]):
                fails.append(('P', P, 'cover', cover, 'does not add up to the full call'))
        hw = be.to_host(d_Wbig)
        if not (np.array_equal(hw[:, :P], W) and _nan_outside(hw, P) and np.array_equal(be.to_host(d_aoP), aoP)
                and np.array_equal(be.to_host(d_dm), dms)):
            fails.append(('P', P, 'inputs changed'))
    _report(fails)


# ---- C: isdf_get_k_pair ---------------------------------------------------------------------------------------------------------
def _get_k_pair_case(be, P, nao, fails):
    rng = np.random.default_rng([6, P, nao])
    A1, A2 = _cints(rng, (P, nao)), _cints(rng, (P, nao))
    D2, Wq = _cints(rng, (nao, nao)), _cints(rng, (P, P))
    vk0 = _cints(rng, (nao, nao), 50)
    want = vk0 - 2.0 * (A1.conj().T @ (((A2 @ D2) @ A2.conj().T) * Wq) @ A1)
    ins = [be.to_device(x) for x in (A1, A2, D2, Wq)]
    snap = _snap(be, *ins)
    buf, vk = _flat(be, (nao, nao), torch.complex128)
    vk.copy_(be.to_device(vk0))
    be.get_k_pair(*ins, -2.0, vk)
    got = be.to_host(buf)
    case = ('P', P, 'nao', nao)
    if not np.array_equal(got[:-1].reshape(nao, nao), want):
        fails.append(case + ('wrong values',))
    if not (np.isnan(got[-1].real) and np.isnan(got[-1].imag)):
        fails.append(case + ('guard written',))
    if not _unchanged(be, ins, snap):
        fails.append(case + ('inputs changed',))


def test_C_get_k_pair(be):
    """isdf_get_k_pair ACCUMULATES vk += scale A1^H [(A2 D2 A2^H) .* Wq] A1 on complex integers (components <= 3), A1 != A2, D2 and
    Wq non-Hermitian, scale = -2, integer prefill.  Per component: |A2 D2| <= 18 * 18, |A2 D2 A2^H| <= 18 * 324 * 6 < 3.5e4, times
    Wq < 2.1e5, times A1 summed over 300 points < 3.8e8, the outer sum < 6.9e11 < 2^53."""
    fails = []
    for P in (1, 37, 256, 300):
        for nao in (1, 5, 18):
            _get_k_pair_case(be, P, nao, fails)
    _report(fails)


def test_C_get_k_pair_past_one_grid_stride_round(be):
    """P = 1100, nao = 3: P^2 exceeds the 16 x 256 x CUs threads of the complex Hadamard launch, so its grid-stride loop repeats.
    Magnitudes: |X| <= 3 * 54 * 6 < 1e3, times Wq < 6e3, sums over 1100 points twice < 4.4e10."""
    P = 1100
    assert P * P > 16 * 256 * _ncu(be), 'P = %d no longer crosses one grid-stride round on %d CUs' % (P, _ncu(be))
    fails = []
    _get_k_pair_case(be, P, 3, fails)
    _report(fails)


# ---- D: element-wise and tile helpers --------------------------------------------------------------------------------------------
def test_D_hadamard_rows_and_zhadamard_planes(be):
    """X .*= Y and (Ar + i Ai) .*= (Br + i Bi) on integer data (products <= 18), leading dimensions of X and Y different from each
    other and from cols; the padding of X stays NaN, Y is unchanged.  65536 rows (past the launch's y dimension) are refused with
    the argument error and leave the buffer untouched."""
    from pyscf_isdf_amd.lib import IsdfError
    fails = []
    shapes = [(r, c) for r in (1, 2) for c in (1, 255, 256, 257, 1000)] + [(65535, 3)]
    for rows, cols in shapes:
        rng = np.random.default_rng([7, rows, cols])
        for padx, pady in ((1, 4), (6, 3)):
            X, Y = _cints(rng, (rows, cols)), _cints(rng, (rows, cols))
            bx, vx = _wide(be, X.real.copy(), padx)
            by, vy = _wide(be, Y.real.copy(), pady)
            snap = _snap(be, by)
            be.hadamard_rows(vx, vy)
            got = be.to_host(bx)
            case = ('hadamard_rows', rows, cols, 'ldx', cols + padx, 'ldy', cols + pady)
            if not np.array_equal(got[:, :cols], X.real * Y.real):
                fails.append(case + ('wrong values',))
            if not (_nan_outside(got, cols) and _unchanged(be, [by], snap)):
                fails.append(case + ('padding written or Y changed',))
            bar, var = _wide(be, X.real.copy(), padx)
            bai, vai = _wide(be, X.imag.copy(), padx)
            bbr, vbr = _wide(be, Y.real.copy(), pady)
            bbi, vbi = _wide(be, Y.imag.copy(), pady)
            snap = _snap(be, bbr, bbi)
            be.zhadamard_planes(var, vai, vbr, vbi)
            gr, gi = be.to_host(bar), be.to_host(bai)
            case = ('zhadamard_planes', rows, cols, 'lda', cols + padx, 'ldb', cols + pady)
            if not (np.array_equal(gr[:, :cols], (X * Y).real) and np.array_equal(gi[:, :cols], (X * Y).imag)):
                fails.append(case + ('wrong values',))
            if not (_nan_outside(gr, cols) and _nan_outside(gi, cols) and _unchanged(be, [bbr, bbi], snap)):
                fails.append(case + ('padding written or B changed',))
    rows, cols = 65536, 3
    X = _ints(np.random.default_rng(8), (rows, cols))
    for name in ('hadamard_rows', 'zhadamard_planes'):
        bx, vx = _wide(be, X, 1)
        bi, vi = _wide(be, X, 1)
        by, vy = _wide(be, X, 2)
        snap = _snap(be, bx, bi)
        try:
            if name == 'hadamard_rows':
                be.hadamard_rows(vx, vy)
            else:
                be.zhadamard_planes(vx, vi, vy, vy)
            fails.append((name, '65536 rows accepted'))
        except IsdfError as e:
            if 'status 1' not in str(e):
                fails.append((name, '65536 rows', 'not the argument error: %s' % e))
        if not _unchanged(be, [bx, bi], snap):
            fails.append((name, '65536 rows', 'buffer touched by the refused call'))
    _report(fails)


def test_D_symmetrize_upper_and_hermitian(be):
    """W[q][p] = W[p][q] (Re) / -W[p][q] (Im) for q > p on integer upper triangles with NaN in the lower one and in the padding:
    afterwards the lower triangle is the mirror, the upper triangle and the diagonal - that of Wim included, which the call leaves
    as it is - are bit-unchanged and the padding is untouched."""
    fails = []
    for P in TILE_PS:
        rng = np.random.default_rng([9, P])
        for pad in (0, 1, 5):
            U = [_ints(rng, (P, P), 9) for _ in range(3)]
            low = np.tril(np.ones((P, P), dtype=bool), -1)
            for M in U:
                M[low] = NAN
            want = []
            for M, sign in zip(U, (1.0, 1.0, -1.0)):
                w = M.copy()
                w[low] = (sign * M.T)[low]
                want.append(w)
            b0, v0 = _wide(be, U[0], pad)
            be.symmetrize_upper(v0)
            b1, v1 = _wide(be, U[1], pad)
            b2, v2 = _wide(be, U[2], pad)
            be.symmetrize_hermitian(v1, v2)
            for name, b, w in (('upper', b0, want[0]), ('hermitian Re', b1, want[1]), ('hermitian Im', b2, want[2])):
                got = be.to_host(b)
                if not np.array_equal(got[:, :P], w):
                    bad = np.argwhere(got[:, :P] != w)
                    fails.append((name, 'P', P, 'ldw', P + pad, '%d wrong, first at %s' % (len(bad), bad[0])))
                if not _nan_outside(got, P):
                    fails.append((name, 'P', P, 'ldw', P + pad, 'padding written'))
    _report(fails)


def test_D_symmetrize_mean(be):
    """W <- (W + W^T) / 2 and (W - W^T) / 2 on integers <= 9 (halves are exact); the antisymmetric form gives an exactly zero
    diagonal; the padding stays NaN."""
    fails = []
    for P in TILE_PS:
        rng = np.random.default_rng([10, P])
        for pad in (0, 1, 5):
            for anti in (False, True):
                M = _ints(rng, (P, P), 9)
                big, view = _wide(be, M, pad)
                be.symmetrize_mean(view, antisymmetric=anti)
                got = be.to_host(big)
                want = (M - M.T) / 2 if anti else (M + M.T) / 2
                if not np.array_equal(got[:, :P], want):
                    bad = np.argwhere(got[:, :P] != want)
                    fails.append(('P', P, 'ldw', P + pad, 'antisymmetric', anti, '%d wrong, first at %s' % (len(bad), bad[0])))
                if not _nan_outside(got, P):
                    fails.append(('P', P, 'ldw', P + pad, 'antisymmetric', anti, 'padding written'))
    _report(fails)


def test_D_finish_Wq(be):
    """Wc = (Wre + i Wim)[p][q] ph[p] conj(ph[q]) with ldw = P + 3 and "phases" from {1, -1, i, -i} and from Gaussian integers
    (|component| <= 2; the kernel needs no unit modulus), so every product is an exact integer (< 9 * 8 * 2 * 2)."""
    fails = []
    units = np.array([1, -1, 1j, -1j])
    for P in TILE_PS:
        rng = np.random.default_rng([11, P])
        for kind in ('units', 'gaussian integers'):
            ph = units[rng.integers(0, 4, P)] if kind == 'units' else _cints(rng, P, 2)
            Wre, Wim = _ints(rng, (P, P), 9), _ints(rng, (P, P), 9)
            br, vr = _wide(be, Wre, 3)
            bi, vi = _wide(be, Wim, 3)
            d_ph = be.to_device(ph.astype(np.complex128))
            snap = _snap(be, br, bi, d_ph)
            buf, Wc = _flat(be, (P, P), torch.complex128)
            be.finish_Wq(vr, vi, d_ph, Wc)
            got = be.to_host(buf)
            want = (Wre + 1j * Wim) * ph[:, None] * ph.conj()[None, :]
            if not np.array_equal(got[:-1].reshape(P, P), want):
                bad = np.argwhere(got[:-1].reshape(P, P) != want)
                fails.append(('P', P, kind, '%d wrong, first at %s' % (len(bad), bad[0])))
            if not (np.isnan(got[-1].real) and np.isnan(got[-1].imag)):
                fails.append(('P', P, kind, 'guard written'))
            if not _unchanged(be, [br, bi, d_ph], snap):
                fails.append(('P', P, kind, 'inputs changed'))
    _report(fails)


def test_D_dot(be):
    """isdf_dot on integers (|x| <= 3: |sum| <= 9 000 027) against Python integer sums, n up to 1 000 003: past 1024 x 256 = 262 144
    elements every workgroup strides more than once."""
    fails = []
    for n in (1, 255, 256, 257, 262143, 262144, 262145, 1000003):
        rng = np.random.default_rng([12, n])
        x, y = rng.integers(-3, 4, n), rng.integers(-3, 4, n)
        x[-1], y[-1] = 3, -2                                          # the last element counts
        bx = torch.full((n + 1,), NAN, dtype=torch.float64, device=be.device)
        by = torch.full((n + 1,), NAN, dtype=torch.float64, device=be.device)
        bx[:n] = be.to_device(x.astype(np.float64))
        by[:n] = be.to_device(y.astype(np.float64))
        sx, sxy = sum(x.tolist()), sum(a * b for a, b in zip(x.tolist(), y.tolist()))          # Python integers
        g1, g2 = be.dot(bx[:n]), be.dot(bx[:n], by[:n])
        if g1 != sx or g2 != sxy:
            fails.append(('n', n, 'sum', g1, 'want', sx, 'dot', g2, 'want', sxy))
        if not np.array_equal(be.to_host(bx[:n]), x) or not np.array_equal(be.to_host(by[:n]), y):
            fails.append(('n', n, 'inputs changed'))
    _report(fails)


# ---- E: entries that contain a transform -----------------------------------------------------------------------------------------
def _conv_ref(rows, mesh, table):
    """ifftn(table * fftn(rows)) in complex128, rows (n, G)."""
    z = np.fft.fftn(rows.reshape(len(rows), *mesh), axes=(1, 2, 3)) * table.reshape(mesh)
    return np.fft.ifftn(z, axes=(1, 2, 3)).reshape(len(rows), -1)


def _weight(mesh):
    return abs(np.linalg.det(A_TRI)) / float(np.prod(mesh))


class _Worst(dict):
    def add(self, entry, ratio, case):
        if ratio > self.get(entry, (-1.0, None))[0]:
            self[entry] = (float(ratio), case)

    def show(self):
        for entry in sorted(self):
            print('  %-28s largest error / bound %.2e at %s' % (entry, self[entry][0], self[entry][1]))


def test_E_get_j_pieces_and_table(be):
    """isdf_get_j against rho -> convolve -> vj restated with numpy (nao = 5, nset = 2, ld = G + 2, Gaussian data, non-symmetric dm):
    |vj - ref| <= 1e-12 max|v| sum_g |ao_i| |ao_j|; isdf_rho + isdf_coulomb_potential + isdf_vj_from_vR give the bits of isdf_get_j;
    the potential itself within TOL of max|v|; isdf_coulG_half against the oracle's symmetrised table to 1e-12 of its largest
    entry.  The own transform must have run (label)."""
    fails, worst = [], _Worst()
    nao, nset = 5, 2
    for mesh in MESHES:
        G = int(np.prod(mesh))
        rng = np.random.default_rng([13, G])
        ao, dm = rng.standard_normal((nao, G)), rng.standard_normal((nset, nao, nao))
        table = otools.get_coulG(A_TRI, list(mesh))
        rho = np.einsum('img,mg->ig', dm @ ao, ao)
        v = _weight(mesh) * _conv_ref(rho, mesh, table).real
        ref = np.einsum('ig,sg,jg->sij', ao, v, ao)
        bound = TOL * abs(v).max(axis=1)[:, None, None] * np.einsum('ig,jg->ij', abs(ao), abs(ao))[None]
        big, view = _wide(be, ao, 2)
        d_dm = be.to_device(dm)
        snap = _snap(be, big, d_dm)
        buf, vj = _flat(be, (nset, nao, nao))
        _, labels = _labels(be, lambda: be.get_j(view, G, np.asarray(mesh), A_TRI, d_dm, vj))
        got = be.to_host(buf)
        if len(labels & OWN_CONV) != 1 or labels & (FFT_LABELS - OWN_CONV):
            fails.append((mesh, 'get_j labels %s' % sorted(labels & FFT_LABELS)))
        ratio = (abs(got[:-1].reshape(ref.shape) - ref) / bound).max()
        worst.add('isdf_get_j', ratio, mesh)
        if not ratio <= 1.0:
            fails.append((mesh, 'get_j error / bound %.3e' % ratio))
        if not np.isnan(got[-1]) or not _unchanged(be, [big, d_dm], snap):
            fails.append((mesh, 'get_j guard written or inputs changed'))
        d_rho = be.empty((nset, G))
        be.rho(view, G, d_dm, d_rho)
        be.coulomb_potential(d_rho, np.asarray(mesh), A_TRI)
        buf2, vj2 = _flat(be, (nset, nao, nao))
        be.vj_from_vR(view, G, d_rho, vj2)
        if not np.array_equal(be.to_host(buf2)[:-1], got[:-1]):
            fails.append((mesh, 'the three pieces differ from get_j'))
        ratio = abs(be.to_host(d_rho) - v).max() / (TOL * abs(v).max())
        worst.add('isdf_coulomb_potential', ratio, mesh)
        if not ratio <= 1.0:
            fails.append((mesh, 'potential error / bound %.3e' % ratio))
        flip = table.reshape(mesh)[np.ix_(*[(-np.arange(n)) % n for n in mesh])]
        tab_ref = (0.5 * (table.reshape(mesh) + flip) / G)[:, :, :mesh[2] // 2 + 1]
        ratio = abs(be.coulG_half(np.asarray(mesh), A_TRI) - tab_ref).max() / (1e-12 * abs(tab_ref).max())
        worst.add('isdf_coulG_half', ratio, mesh)
        if not ratio <= 1.0:
            fails.append((mesh, 'coulG_half error / bound %.3e' % ratio))
    print()
    worst.show()
    _report(fails)


KX_WINDOWS = ((0, 7), (2, 4), (6, 1), (3, 0), (0, 2))
KX_COVER = ((0, 2), (2, 4), (6, 1))
KX_MAX_ROWS = (3, 7, 1000)            # nocc = 3: one AO row per pass; two with a ragged last pass; one pass


def test_E_get_k_exact(be):
    """isdf_get_k_exact (nao = 7, nocc = 3, ld = G + 2) writes rows i0 .. i0 + ni of a full (nao, nao) vk and nothing else: the other
    rows and the guard stay NaN, ni = 0 writes nothing.  Against numpy with |vk - ref| <= 1e-12 max|V| w sum_g sum_j |mo_j| |ao_l|; the
    windows of a cover give the bits of the full call at the same max_rows."""
    fails, worst = [], _Worst()
    nao, nocc = 7, 3
    for mesh in MESHES:
        G = int(np.prod(mesh))
        w = _weight(mesh)
        rng = np.random.default_rng([14, G])
        ao, C = rng.standard_normal((nao, G)), rng.standard_normal((nao, nocc))
        table = otools.get_coulG(A_TRI, list(mesh))
        mo = C.T @ ao
        V = _conv_ref((ao[:, None, :] * mo[None]).reshape(nao * nocc, G), mesh, table).real.reshape(nao, nocc, G)
        ref = w * np.einsum('ijg,jg,lg->il', V, mo, ao)
        bound = TOL * abs(V).max() * w * np.einsum('jg,lg->l', abs(mo), abs(ao))[None, :]
        big, view = _wide(be, ao, 2)
        d_C = be.to_device(C)
        snap = _snap(be, big, d_C)
        for max_rows in KX_MAX_ROWS:
            got = {}
            for i0, ni in KX_WINDOWS:
                buf, vk = _flat(be, (nao, nao))
                _, labels = _labels(be, lambda: be.get_k_exact(view, G, d_C, np.asarray(mesh), A_TRI, i0, ni, max_rows, vk))
                h = be.to_host(buf)
                g = got[i0, ni] = h[:-1].reshape(nao, nao)
                case = (mesh, 'max_rows', max_rows, 'window', (i0, ni))
                if ni and (len(labels & OWN_CONV) != 1 or labels & (FFT_LABELS - OWN_CONV)):
                    fails.append(case + ('labels %s' % sorted(labels & FFT_LABELS),))
                outside = np.ones(nao, dtype=bool)
                outside[i0:i0 + ni] = False
                if not (np.all(np.isnan(g[outside])) and np.isnan(h[-1])):
                    fails.append(case + ('rows outside the window or the guard written',))
                if ni:
                    ratio = (abs(g[i0:i0 + ni] - ref[i0:i0 + ni]) / bound).max()
                    worst.add('isdf_get_k_exact', ratio, case)
                    if not ratio <= 1.0:
                        fails.append(case + ('error / bound %.3e' % ratio,))
            union = np.vstack([got[win][win[0]:win[0] + win[1]] for win in KX_COVER])
            if not np.array_equal(union, got[0, nao]):
                fails.append((mesh, 'max_rows', max_rows, 'the cover differs from the full call by %.3e' % abs(union - got[0, nao]).max()))
        if not _unchanged(be, [big, d_C], snap):
            fails.append((mesh, 'inputs changed'))
    print()
    worst.show()
    _report(fails)


def test_E_get_k_exact_kpt(be):
    """isdf_get_k_exact_kpt ACCUMULATES rows i0 .. i0 + ni into an (ni, nao) block (prefilled with an integer field), kernel table
    random positive without inversion symmetry, u1 (ld = G + 2) and m2 (ld = G + 3) complex with independent planes.  Reference: the
    formula of oracle/kisdf.py's exact path in periodic parts, vk[p, l] = weight sum_g sum_j conv_q[conj(u1_p) m2_j] conj(m2_j) u1_l,
    with |vk - ref| <= 1e-12 max|V| weight sum_g sum_j |m2_j| |u1_l|.  ni = 0 touches nothing.  hipFFT Z2Z always (label)."""
    fails, worst = [], _Worst()
    nao, nocc, weight = 7, 3, 0.37
    for mesh in MESHES_KPT:
        G = int(np.prod(mesh))
        rng = np.random.default_rng([15, G])
        u1 = rng.standard_normal((nao, G)) + 1j * rng.standard_normal((nao, G))
        m2 = rng.standard_normal((nocc, G)) + 1j * rng.standard_normal((nocc, G))
        table = rng.random(G) + 0.1
        F = _cints(rng, (nao, nao), 3)
        V = _conv_ref((u1.conj()[:, None, :] * m2[None]).reshape(nao * nocc, G), mesh, table).reshape(nao, nocc, G)
        ref = weight * np.einsum('pjg,jg,lg->pl', V, m2.conj(), u1)
        bound = TOL * abs(V).max() * weight * np.einsum('jg,lg->l', abs(m2), abs(u1))[None, :]
        b1r, u1r = _wide(be, u1.real.copy(), 2)
        b1i, u1i = _wide(be, u1.imag.copy(), 2)
        b2r, m2r = _wide(be, m2.real.copy(), 3)
        b2i, m2i = _wide(be, m2.imag.copy(), 3)
        d_tab = be.to_device(table)
        ins = [b1r, b1i, b2r, b2i, d_tab]
        snap = _snap(be, *ins)
        for max_rows in KX_MAX_ROWS:
            got = {}
            for i0, ni in KX_WINDOWS:
                case = (mesh, 'max_rows', max_rows, 'window', (i0, ni))
                if ni == 0:           # an (0, nao) tensor has no address: the C entry directly, on a guard buffer that must stay as it is
                    gre, _ = _flat(be, (1,))
                    gim, _ = _flat(be, (1,))
                    m = np.ascontiguousarray(mesh, dtype=np.int32)
                    be._stream()
                    be.handle.call('isdf_get_k_exact_kpt', be._p(u1r), be._p(u1i), nao, u1r.stride(0), be._p(m2r), be._p(m2i), nocc,
                                   m2r.stride(0), m.ctypes.data_as(ctypes.c_void_p), be._p(d_tab), weight, i0, 0, max_rows,
                                   be._p(gre), be._p(gim))
                    if not (np.all(np.isnan(be.to_host(gre))) and np.all(np.isnan(be.to_host(gim)))):
                        fails.append(case + ('ni = 0 wrote something',))
                    continue
                bre, vre = _flat(be, (ni, nao))
                bim, vim = _flat(be, (ni, nao))
                vre.copy_(be.to_device(F.real[i0:i0 + ni].copy()))
                vim.copy_(be.to_device(F.imag[i0:i0 + ni].copy()))
                _, labels = _labels(be, lambda: be.get_k_exact_kpt(u1r, u1i, m2r, m2i, np.asarray(mesh), d_tab, weight, i0, ni,
                                                                   max_rows, vre, vim))
                hre, him = be.to_host(bre), be.to_host(bim)
                g = got[i0, ni] = hre[:-1].reshape(ni, nao) + 1j * him[:-1].reshape(ni, nao)
                if labels & FFT_LABELS != {EXACT_KPT}:
                    fails.append(case + ('labels %s' % sorted(labels & FFT_LABELS),))
                if not (np.isnan(hre[-1]) and np.isnan(him[-1])):
                    fails.append(case + ('guard written',))
                ratio = (abs(g - F[i0:i0 + ni] - ref[i0:i0 + ni]) / bound).max()
                worst.add('isdf_get_k_exact_kpt', ratio, case)
                if not ratio <= 1.0:
                    fails.append(case + ('error / bound %.3e' % ratio,))
            union = np.vstack([got[win] for win in KX_COVER])
            if not np.array_equal(union, got[0, nao]):
                fails.append((mesh, 'max_rows', max_rows, 'the cover differs from the full call by %.3e' % abs(union - got[0, nao]).max()))
        if not _unchanged(be, ins, snap):
            fails.append((mesh, 'inputs changed'))
    print()
    worst.show()
    _report(fails)


def test_E_nyquist_spectra(be):
    """isdf_nyquist_spectra on every even axis of (6, 5, 4), (4, 6, 10), (9, 8, 7), (2, 2, 2), 1 and 5 rows with ld = G + 3, against
    the Nyquist plane of np.fft.fftn within TOL of max|ref|."""
    fails, worst = [], _Worst()
    for mesh in ((6, 5, 4), (4, 6, 10), (9, 8, 7), (2, 2, 2)):
        G = int(np.prod(mesh))
        for axis in range(3):
            if mesh[axis] % 2:
                continue
            for nrow in (1, 5):
                rows = np.random.default_rng([16, G, axis, nrow]).standard_normal((nrow, G))
                spec = np.fft.fftn(rows.reshape(nrow, *mesh), axes=(1, 2, 3))
                ref = np.take(spec, mesh[axis] // 2, axis=axis + 1).reshape(nrow, -1)
                big, view = _wide(be, rows, 3)
                snap = _snap(be, big)
                bre, vre = _flat(be, ref.shape)
                bim, vim = _flat(be, ref.shape)
                be.nyquist_spectra(view, np.asarray(mesh), axis, vre, vim)
                hre, him = be.to_host(bre), be.to_host(bim)
                got = hre[:-1].reshape(ref.shape) + 1j * him[:-1].reshape(ref.shape)
                case = (mesh, 'axis', axis, 'rows', nrow)
                ratio = abs(got - ref).max() / (TOL * abs(ref).max())
                worst.add('isdf_nyquist_spectra', ratio, case)
                if not ratio <= 1.0:
                    fails.append(case + ('error / bound %.3e' % ratio,))
                if not (np.isnan(hre[-1]) and np.isnan(him[-1]) and _unchanged(be, [big], snap)):
                    fails.append(case + ('guard written or input changed',))
    print()
    worst.show()
    _report(fails)


def test_E_hipfft_forms_past_one_grid_stride_round(be):
    """own_fft = 0 on (12, 12, 12): isdf_coulomb_rows_q with rows x G and isdf_coulomb_rows with rows x G_half just past
    16 x 256 x CUs elements, so the grid-stride loops of pack_real_to_complex / mul_full / unpack_complex and of mul_half repeat;
    the hipFFT labels asserted, every row within TOL of its own max|ref|."""
    fails, worst = [], _Worst()
    mesh = (12, 12, 12)
    G, gc = 12 ** 3, 12 * 12 * 7
    threads = 16 * 256 * _ncu(be)
    n_q, n_g = threads // G + 1, threads // gc + 1
    assert n_q * G > threads and n_g * gc > threads
    rng = np.random.default_rng(17)
    be.set_option('own_fft', 0)
    try:
        rows, table = rng.standard_normal((n_q, G)), rng.random(G) + 0.1
        ref = _conv_ref(rows, mesh, table)
        d_rows, d_tab = be.to_device(rows), be.to_device(table)
        bre = torch.full((n_q + 1, G), NAN, dtype=torch.float64, device=be.device)
        bim = torch.full((n_q + 1, G), NAN, dtype=torch.float64, device=be.device)
        _, labels = _labels(be, lambda: be.coulomb_rows_q(d_rows, np.asarray(mesh), d_tab, bre[:n_q], bim[:n_q]))
        hre, him = be.to_host(bre), be.to_host(bim)
        if labels & FFT_LABELS != {HIPFFT_CONV_Q}:
            fails.append(('coulomb_rows_q', 'labels %s' % sorted(labels & FFT_LABELS)))
        err = np.maximum(abs(hre[:n_q] - ref.real).max(axis=1), abs(him[:n_q] - ref.imag).max(axis=1)) / abs(ref).max(axis=1)
        worst.add('isdf_coulomb_rows_q (hipFFT)', err.max() / TOL, 'row %d of %d' % (err.argmax(), n_q))
        if not err.max() <= TOL:
            fails.append(('coulomb_rows_q', '%d rows off, worst row %d by %.3e' % ((err > TOL).sum(), err.argmax(), err.max())))
        if not (np.all(np.isnan(hre[n_q])) and np.all(np.isnan(him[n_q])) and np.array_equal(be.to_host(d_rows), rows)):
            fails.append(('coulomb_rows_q', 'guard row written or input changed'))

        rows = rng.standard_normal((n_g, G))
        ref = _conv_ref(rows, mesh, otools.get_coulG(A_TRI, list(mesh))).real
        d_rows = be.to_device(rows)
        out = torch.full((n_g + 1, G), NAN, dtype=torch.float64, device=be.device)
        _, labels = _labels(be, lambda: be.coulomb_rows(d_rows, np.asarray(mesh), A_TRI, n_g, out=out[:n_g]))
        h = be.to_host(out)
        if labels & FFT_LABELS != {HIPFFT_CONV}:
            fails.append(('coulomb_rows', 'labels %s' % sorted(labels & FFT_LABELS)))
        err = abs(h[:n_g] - ref).max(axis=1) / abs(ref).max(axis=1)
        worst.add('isdf_coulomb_rows (hipFFT)', err.max() / TOL, 'row %d of %d' % (err.argmax(), n_g))
        if not err.max() <= TOL:
            fails.append(('coulomb_rows', '%d rows off, worst row %d by %.3e' % ((err > TOL).sum(), err.argmax(), err.max())))
        if not (np.all(np.isnan(h[n_g])) and np.array_equal(be.to_host(d_rows), rows)):
            fails.append(('coulomb_rows', 'guard row written or input changed'))
    finally:
        be.set_option('own_fft', 2)
    print()
    worst.show()
    _report(fails)
