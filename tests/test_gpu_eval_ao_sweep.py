"""Sweep of the AO collocation (pyscf_isdf_amd/csrc/eval_ao.hip): all four entry points - eval_ao, eval_ao_deriv1, eval_ao_k,
eval_ao_k_deriv1 - against the CPU oracle on one small cell that reaches every edge of the kernels: s / p / d / f shells with
4 / 3 / 2 / 2 contractions (4 is the NCMAX edge), more than 512 lattice images (three rounds of the 256-wide image cull, the
last one ragged), point sets that fill several workgroups with a ragged last one, a workgroup box that spans the cell (nearly
every image survives the cull) and a single partial workgroup; padded leading dimensions and plane strides whose padding must
stay untouched; Bloch sums with and without the periodic-part phase.  The host-side refusals (l > 3, more than 4
contractions, an atom's shells not contiguous) close the file.

Bounds (those of test_gpu_parity.py): values 1e-12 * max(1, max|ref|), derivatives 1e-11 * max(1, max|ref|); component 0 of
a derivative form equals the value form to 1e-14; the k forms at kpt = 0 with the periodic part equal the Gamma forms to the
same 1e-14 (the Bloch factors are then exactly 1 + 0i), with a zero imaginary plane.  tools/ao_bits.py imports POINT_SETS,
FORMS, KPT, the cell, the points and run() from here."""
import functools
import numpy as np
import pytest
from pyscf_isdf_amd import gto
from pyscf_isdf_amd.lib import IsdfError
from oracle import ao as oao

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
KPT = np.array([0.21, -0.13, 0.34])
TOL_VALUE, TOL_DERIV, TOL_COMPONENT0 = 1e-12, 1e-11, 1e-14
# (name, selection of the 1320 grid points)
POINT_SETS = ('all', 'permuted513', 'first100')
# (entry point, kpt or None, periodic_part)
FORMS = (('eval_ao', None, False), ('eval_ao_deriv1', None, False),
         ('eval_ao_k', KPT, False), ('eval_ao_k', KPT, True),
         ('eval_ao_k_deriv1', KPT, False), ('eval_ao_k_deriv1', KPT, True))
CASES = [(pts, entry, kpt, periodic) for pts in POINT_SETS for entry, kpt, periodic in FORMS]


def _basis():
    s = [0, [2.3, 0.4, -0.2, 0.1, 0.3], [1.4, 0.5, 0.3, -0.4, 0.2], [0.8, 0.3, 0.6, 0.5, -0.3], [0.35, 0.1, 0.2, 0.7, 0.6]]
    p = [1, [1.9, 0.6, -0.3, 0.2], [0.9, 0.5, 0.4, -0.5], [0.4, 0.2, 0.7, 0.6]]
    d = [2, [1.6, 0.7, -0.4], [0.6, 0.4, 0.8]]
    f = [3, [1.2, 0.7, 0.5], [0.5, 0.4, -0.6]]
    return {'He': [s, p, d, f]}


@functools.lru_cache(maxsize=None)
def sweep_cell():
    a = 0.6 * np.array([[4.2, 0.3, 0.], [0.1, 4.0, 0.2], [0.4, 0., 4.4]])
    cell = gto.Cell(atom='He 0.3 0.1 0.2; He 1.3 1.5 0.9', basis=_basis(), a=a, mesh=[11, 10, 12], unit='B')
    rcut = gto.estimate_rcut_per_shell(cell)
    Ls = gto.get_lattice_Ls(cell, rcut=rcut.max())
    return cell, Ls, rcut


@functools.lru_cache(maxsize=None)
def points(name):
    coords = sweep_cell()[0].get_uniform_grids()
    if name == 'all':
        return coords
    if name == 'permuted513':
        return coords[np.random.default_rng(513).permutation(len(coords))[:513]]
    return coords[:100]


@functools.lru_cache(maxsize=None)
def reference(pts, deriv, with_kpt, periodic):
    """(ncomp, nao, npts) complex array from the oracle; computed once per combination and shared."""
    cell, Ls, rcut = sweep_cell()
    c = points(pts)
    if periodic:                                          # as tests/oracle_backend.py applies it
        v = reference(pts, deriv, with_kpt, False) * np.exp(-1j * c.dot(KPT))[None, None, :]
        v.setflags(write=False)
        return v
    if deriv:
        v = np.asarray(oao.eval_ao_deriv1(cell._atm, cell._bas, cell._env, c, Ls, rcut, kpt=KPT if with_kpt else None), dtype=complex)
    elif with_kpt:
        v = np.asarray(oao.eval_ao(cell._atm, cell._bas, cell._env, c, Ls, rcut, kpts=KPT.reshape(1, 3), rule='point')[0], dtype=complex)[None]
    else:
        v = np.asarray(oao.eval_ao(cell._atm, cell._bas, cell._env, c, Ls, rcut, rule='point'), dtype=complex)[None]
    v = np.ascontiguousarray(v.transpose(0, 2, 1))
    v.setflags(write=False)
    return v


def run(be, cell, Ls, rcut, coords, entry, kpt=None, periodic=False):
    """One call into a sentinel-filled buffer with ld = npts + 3 (and plane stride nao * ld + 5 for the derivative forms; for
    the k forms the real and imaginary outputs are the two halves of one buffer).  Returns the host copy of the whole buffer
    viewed as (halves, ncomp, nao, ld) and the flat tail that no view covers."""
    import torch
    npts, nao = len(coords), cell.nao_nr()
    ld = npts + 3
    ncomp = 4 if entry.endswith('deriv1') else 1
    halves = 2 if '_k' in entry else 1
    plane = nao * ld + (5 if ncomp == 4 else 0)
    flat = torch.full((halves * ncomp * plane,), SENTINEL, dtype=torch.float64, device=be.device)
    view = flat.view(halves, ncomp, plane)[:, :, :nao * ld].unflatten(2, (nao, ld))        # (halves, ncomp, nao, ld)
    d_c = be.to_device(np.ascontiguousarray(coords.T))
    args = (cell._atm, cell._bas, cell._env, Ls, rcut)
    if entry == 'eval_ao':
        be.eval_ao(*args, d_c, view[0, 0])
    elif entry == 'eval_ao_deriv1':
        be.eval_ao_deriv1(*args, d_c, view[0])
    elif entry == 'eval_ao_k':
        be.eval_ao_k(*args, kpt, periodic, d_c, view[0, 0], view[1, 0])
    else:
        be.eval_ao_k_deriv1(*args, kpt, periodic, d_c, view[0], view[1])
    host = be.to_host(flat).reshape(halves, ncomp, plane)
    return host[:, :, :nao * ld].reshape(halves, ncomp, nao, ld), host[:, :, nao * ld:]


@pytest.fixture(scope='module')
def be():
    from pyscf_isdf_amd.backend import HipBackend
    return HipBackend(0)


@functools.lru_cache(maxsize=None)
def _got(be, pts, entry, with_kpt, periodic, zero_kpt=False):
    cell, Ls, rcut = sweep_cell()
    kpt = (np.zeros(3) if zero_kpt else KPT) if with_kpt else None
    body, tail = run(be, cell, Ls, rcut, points(pts), entry, kpt, periodic)
    npts = len(points(pts))
    assert (body[..., npts:] == SENTINEL).all() and (tail == SENTINEL).all(), 'padding was written'
    out = body[..., :npts]
    out = out[0] + 1j * out[1] if out.shape[0] == 2 else out[0].astype(complex)
    out.setflags(write=False)
    return out                                           # (ncomp, nao, npts)


def test_the_case_is_as_large_as_stated():
    cell, Ls, rcut = sweep_cell()
    assert cell.nao_nr() == 74 and len(cell.get_uniform_grids()) == 1320
    assert len(Ls) > 512, len(Ls)                       # three rounds of the 256-wide cull loop
    assert len(Ls) % 256 != 0
    assert max(cell.bas_nctr(i) for i in range(cell.nbas)) == 4
    assert sorted(set(cell.bas_angular(i) for i in range(cell.nbas))) == [0, 1, 2, 3]


@pytest.mark.parametrize('pts,entry,kpt,periodic', CASES,
                         ids=['%s-%s%s%s' % (p, e, '-k' if k is not None else '', '-periodic' if per else '') for p, e, k, per in CASES])
def test_against_the_oracle(be, pts, entry, kpt, periodic):
    deriv = entry.endswith('deriv1')
    ref = reference(pts, deriv, kpt is not None, periodic)
    got = _got(be, pts, entry, kpt is not None, periodic)
    assert got.shape == ref.shape
    scale = max(1.0, abs(ref).max())
    err_value = abs(got[0] - ref[0]).max()
    print('%s %s: value error %.3e (max|ref| %.3e)' % (pts, entry, err_value, abs(ref).max()))
    if kpt is None:
        assert (got.imag == 0).all()
    if deriv:
        err = abs(got - ref).max()
        print('%s %s: derivative error %.3e' % (pts, entry, err))
        assert err < TOL_DERIV * scale
    else:
        assert err_value < TOL_VALUE * scale


@pytest.mark.parametrize('pts', POINT_SETS)
@pytest.mark.parametrize('with_kpt,periodic', [(False, False), (True, False), (True, True)])
def test_component_0_of_the_derivative_form_is_the_value_form(be, pts, with_kpt, periodic):
    k = '_k' if with_kpt else ''
    val = _got(be, pts, 'eval_ao' + k, with_kpt, periodic)
    d1 = _got(be, pts, 'eval_ao' + k + '_deriv1', with_kpt, periodic)
    assert abs(d1[0] - val[0]).max() < TOL_COMPONENT0


@pytest.mark.parametrize('pts', POINT_SETS)
def test_k_forms_at_zero_kpt_are_the_gamma_forms(be, pts):
    for deriv in ('', '_deriv1'):
        gam = _got(be, pts, 'eval_ao' + deriv, False, False)
        k0 = _got(be, pts, 'eval_ao_k' + deriv, True, True, zero_kpt=True)
        assert (k0.imag == 0).all()
        assert abs(k0.real - gam.real).max() < TOL_COMPONENT0


def _refused(be, cell, message, bas=None):
    """All four entry points refuse with the host check's own message, and write nothing."""
    import torch
    _, Ls, rcut = sweep_cell()
    bas = cell._bas if bas is None else bas
    rc = np.resize(rcut, len(bas))
    nao, G = 200, 8
    d_c = be.to_device(np.ascontiguousarray(points('first100')[:G].T))
    args = (cell._atm, bas, cell._env, Ls, rc)
    a1, a4 = torch.full((2, nao, G), SENTINEL, dtype=torch.float64, device=be.device), torch.full((2, 4, nao, G), SENTINEL, dtype=torch.float64, device=be.device)
    with pytest.raises(IsdfError, match=message):
        be.eval_ao(*args, d_c, a1[0])
    with pytest.raises(IsdfError, match=message):
        be.eval_ao_deriv1(*args, d_c, a4[0])
    with pytest.raises(IsdfError, match=message):
        be.eval_ao_k(*args, KPT, True, d_c, a1[0], a1[1])
    with pytest.raises(IsdfError, match=message):
        be.eval_ao_k_deriv1(*args, KPT, True, d_c, a4[0], a4[1])
    assert (be.to_host(a1) == SENTINEL).all() and (be.to_host(a4) == SENTINEL).all()      # nothing was launched


def _small_cell(shell):
    a = 0.6 * np.array([[4.2, 0.3, 0.], [0.1, 4.0, 0.2], [0.4, 0., 4.4]])
    return gto.Cell(atom='He 0.3 0.1 0.2; He 1.3 1.5 0.9', basis={'He': [[0, [1.1, 1.0]], shell]}, a=a, mesh=[11, 10, 12], unit='B')


def test_refuses_l_4(be):
    _refused(be, _small_cell([4, [1.2, 1.0]]), 'has l=4; l <= 3 is supported')


def test_refuses_5_contractions(be):
    _refused(be, _small_cell([0, [1.2, 0.5, 0.4, 0.3, 0.2, 0.1], [0.6, 0.1, 0.2, 0.3, 0.4, 0.5]]), 'has 5 contractions; at most 4 supported')


def test_refuses_shells_of_an_atom_not_contiguous(be):
    cell = sweep_cell()[0]
    bas = np.array(cell._bas)
    assert len(bas) == 8 and bas[3, 0] != bas[4, 0]
    bas[[3, 4]] = bas[[4, 3]]                            # atom 0, 0, 0, 1, 0, 1, 1, 1
    _refused(be, cell, 'shells of atom 0 are not contiguous in bas', bas)
