"""The GTH pseudopotential kernels of pp.hip (vloc_G_kernel, ft_ao_kernel, proj_kernel) through their two entry points, entry by
entry against the longdouble restatement of tests/pp_reference.py and against oracle/pp.py, on hand-built tables
(tests/pp_cases.py).  No bound is a chosen number: each is pp_cases.device_bound of the float64 oracle's error against the
longdouble restatement on the same shape - 8 x that error, at least 64 ulp of the largest reference entry, failing outright above
1e-11 of it.  tests/test_pp_pins.py measures those errors on the CPU and pins the closed forms of both references to quadrature.
Against the oracle itself the device is allowed the same bound plus the oracle's own error (triangle inequality)."""
import numpy as np
import pytest
import torch
import pp_cases as pc
import pp_reference as ref

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not ref.LD_OK, reason=ref.LD_SKIP_REASON)]


@pytest.fixture(scope='module')
def be():
    from pyscf_isdf_amd.backend import HipBackend
    return HipBackend(0)


def _compare(name, got, want, oracle):
    """max|got - want| against the rule's bound; returns the bound (absolute)."""
    scale = abs(want).max()
    oerr = abs(oracle - want).max()
    bound = pc.device_bound(oerr, scale)
    err, err_o = abs(got - want).max(), abs(got - oracle).max()
    print('%-34s device %.2e  oracle %.2e  bound %.2e  (of max|ref| = %.3g); device - oracle %.2e'
          % (name, err / scale, oerr / scale, bound / scale, scale, err_o / scale))
    assert np.all(np.isfinite(got))
    assert err <= bound, (name, float(err / scale), float(bound / scale))
    assert err_o <= bound + oerr, (name, float(err_o / scale))
    return bound


def _vloc(be, lat, par):
    coords, pp_par, mesh, a = pc.vloc_inputs(lat, par)
    out = be.empty((1, int(np.prod(mesh))))
    out.fill_(float('nan'))
    be.pp_local_potential(coords, pp_par, mesh, a, out)
    return be.to_host(out)[0]


@pytest.mark.parametrize('lat,par', pc.VLOC_CASES)
def test_local_potential(be, lat, par):
    """isdf_pp_local_potential on (10,9,8) triclinic, (12,12,12) fcc and (15,14,16) cubic; four off-grid atoms of which one has no
    pseudopotential entry and the others nexp = 0, 2, 4 (second set: 1, 3, 2, the bare atom in another place); the coefficient
    slots past nexp hold numbers that must be ignored.  Whole array relative to max|vlocR|, and the mean over the mesh - which is
    the G = 0 term alone - relative to itself.  The call is repeated after one on another mesh: bit-identical (FFT plan cache,
    pp_Z / pp_tab workspaces).
    Oracle against longdouble (CPU): 4.1e-16 .. 2.1e-15 for the array, 5.5e-17 .. 3.3e-16 for the mean, so the bound is the floor
    of 64 ulp = 1.4e-14 everywhere but fcc nexp024 (1.6e-14).  Device, observed on the MI355X (array / mean, nexp024 then nexp13):
    triclinic 4.5e-16 / 1.3e-16 and 5.2e-16 / 6.4e-16; fcc 2.1e-15 / 7.8e-17 and 1.5e-15 / 1.6e-16; cubic 1.3e-15 / 8.8e-17 and
    9.7e-16 / 2.9e-16; against the oracle at most 6.6e-16."""
    want, orc = pc.cached(pc.vloc_ld, lat, par), pc.cached(pc.vloc_oracle, lat, par)
    got = _vloc(be, lat, par)
    _compare('vlocR %s %s' % (lat, par), got, want, orc)
    n = want.size
    mean = lambda v: np.array([np.asarray(v, dtype=ref.LD).sum() / n])
    _compare('  mean over the mesh', mean(got), mean(want), mean(orc))
    other = [c for c in pc.VLOC_CASES if c[0] != lat][0]
    _vloc(be, *other)
    assert np.array_equal(_vloc(be, lat, par), got)


def _overlaps(be, args, fill=float('nan')):
    nrows = pc.ov_rows()[1]
    nao = 22
    out = torch.full((nrows, nao), complex(fill, fill), dtype=torch.complex128, device=be.device)
    be.pp_projector_overlaps(*args, out)
    return be.to_host(out)


@pytest.mark.parametrize('mesh,kname', pc.OV_CASES)
def test_projector_overlaps(be, mesh, kname):
    """isdf_pp_projector_overlaps, the (40, 22) matrix of all nine (l, i) projectors (atoms 0 and 2, another r_l per channel; atom
    1 between them has AOs and no projector) with s, p and d shells (one of three primitives and two contractions; d shells at
    AO 1 and AO 17), at Gamma and at k = (0.21, -0.13, 0.34), on meshes that make the chunk loop (16384 columns, blocks of 128) run
    one ragged chunk (720), exactly one (16384), a second of 436 = 3 x 128 + 52 (16820) and three (33792).  The output starts as
    NaN, so the first chunk must overwrite it.
    Oracle against longdouble (CPU), Gamma / k, of the largest entry 8.3: 1.9e-15 / 1.4e-15, 1.2e-14 / 9.2e-15, 1.3e-14 / 1.1e-14,
    1.7e-14 / 1.3e-14, so the bounds are 1.5e-14 / 1.4e-14, 9.5e-14 / 7.3e-14, 1.1e-13 / 9.0e-14, 1.4e-13 / 1.0e-13.  Device,
    observed on the MI355X, Gamma / k: 2.6e-15 / 2.3e-15, 2.6e-14 / 1.6e-14, 2.9e-14 / 1.8e-14, 1.8e-14 / 1.3e-14; against the oracle
    at most 2.5e-14."""
    want, orc = pc.cached(pc.ov_ld, mesh, kname), pc.cached(pc.ov_oracle, mesh, kname)
    got = _overlaps(be, pc.ov_inputs(mesh, kname))
    _compare('overlaps %s %s' % (mesh, kname), got, want, orc)


def test_projector_overlaps_reuse_workspaces(be):
    """Large mesh, small mesh, large mesh on one handle, at the k-point: the first and the third result are bit-identical and the
    small one in between holds its own bound (pp_tables / pp_aoG / pp_SPG are kept across calls; rocBLAS zgemm on the same shape
    is run-to-run deterministic, atomics being off by default)."""
    big, small = pc.ov_inputs((33, 32, 32), 'k'), pc.ov_inputs((10, 9, 8), 'k')
    first = _overlaps(be, big)
    mid = _overlaps(be, small, fill=7.0)
    third = _overlaps(be, big, fill=-3.0)
    assert np.array_equal(first, third)
    _compare('overlaps (10,9,8) k, between', mid, pc.cached(pc.ov_ld, (10, 9, 8), 'k'), pc.cached(pc.ov_oracle, (10, 9, 8), 'k'))
    _compare('overlaps (33,32,32) k, third', third, pc.cached(pc.ov_ld, (33, 32, 32), 'k'), pc.cached(pc.ov_oracle, (33, 32, 32), 'k'))


def test_projector_rows_that_vanish_by_symmetry(be):
    """At k = 0 an l = 1 or l = 2 projector against an s function on the same atom leaves sum_G f(|G|) S_lm(G).  On the orthorhombic
    lattice diag(1.5, 1.4, 1.45) with mesh (10, 9, 8) every summand has died out (below 1e-25) before the unpaired -n/2 frequency of
    the even axes, so the G set is closed under each axis reflection and the p rows and the xy, yz, xz rows are zero - 27 entries;
    z^2 and x^2-y^2 are even under all reflections and stay (pp_cases.symmetry_zero_entries).  This needs no reference: a wrong
    (-i)^l, exp(+iG.R) or harmonic order breaks it.  The longdouble restatement has 4e-21 of the largest entry there; the device is
    held to the bound of the shape (oracle error 9.8e-16, so the floor of 64 ulp = 1.4e-14 of the largest entry, 7.6).
    Device, observed on the MI355X: 1.1e-15 for the whole matrix, 1.4e-18 for the largest of the 27 entries."""
    key = ((10, 9, 8), 'gamma', 'ortho_small')
    want, orc = pc.cached(pc.ov_ld, *key), pc.cached(pc.ov_oracle, *key)
    got = _overlaps(be, pc.ov_inputs(*key))
    bound = _compare('overlaps orthorhombic', got, want, orc)
    worst = max(abs(got[i, j]) for i, j in pc.symmetry_zero_entries())
    print('largest entry that vanishes by symmetry: %.2e of max|ref|' % (worst / abs(want).max()))
    assert worst <= bound


def test_refusals_leave_the_output_untouched(be):
    """An AO shell with l = 3, and proj_tab entries with l = 3, i = 3 or a negative index, are refused with ISDF_ERR_ARG before
    anything is launched: the call raises and the output keeps its fill."""
    from pyscf_isdf_amd.lib import IsdfError
    args = list(pc.ov_inputs((10, 9, 8), 'k'))

    def run(a):
        out = torch.full((pc.ov_rows()[1], 22), 5.0 + 5.0j, dtype=torch.complex128, device=be.device)
        with pytest.raises(IsdfError) as e:
            be.pp_projector_overlaps(*a, out)
        torch.cuda.synchronize()
        assert np.all(be.to_host(out) == 5.0 + 5.0j)
        return str(e.value)

    bas = args[1].copy()
    bas[2, 1] = 3
    assert 'l<=2' in run(args[:1] + [bas] + args[2:])
    for j, col, val in [(5, 1, 3), (2, 2, 3), (0, 1, -1), (0, 2, -1)]:
        tab = args[5].copy()
        tab[j, col] = val
        run(args[:5] + [tab] + args[6:])
    got = _overlaps(be, args)                                   # the handle is still good
    _compare('overlaps (10,9,8) k, after refusals', got, pc.cached(pc.ov_ld, (10, 9, 8), 'k'), pc.cached(pc.ov_oracle, (10, 9, 8), 'k'))


def test_get_pp_with_d_and_three_s_projectors():
    """ISDF.get_pp end to end on a two-atom triclinic cell, mesh (12, 11, 10), s/p/d shells, with the fixture's Ge-q4 (nexp = 0,
    channels 3/2/1) and Y-q3 (nexp = 1, channels 3/2/2) entries written over cell._pseudo: the blocks / hl contraction of hcore.py
    for nl > 1, against oracle.pp.get_pp and its longdouble restatement on the same tables (AO values on the grid: the oracle's).
    At Gamma both sides keep the real part, as the reference does.  The k-point matrix is Hermitian to the same bound.
    Oracle against longdouble (CPU): 7.1e-15 (Gamma) and 4.1e-15 (k) of the largest entry 1.9, so the bounds are 5.7e-14 and
    3.3e-14.  Device, observed on the MI355X: 6.5e-15 and 4.3e-15; against the oracle 5.3e-15 and 5.9e-15."""
    from pyscf_isdf_amd.isdf import ISDF
    cell = pc.e2e_cell()
    want, orc = pc.e2e_ld(cell), pc.e2e_oracle(cell)
    df = ISDF(cell)
    v0, vk = df.get_pp(), df.get_pp(pc.E2E_KPT)
    assert v0.dtype == np.float64 and v0.shape == vk.shape == (cell.nao_nr(),) * 2
    _compare('get_pp Gamma', v0, want[0].real, orc[0])
    bound = _compare('get_pp k', vk, want[1], orc[1])
    assert abs(vk - vk.conj().T).max() <= bound

