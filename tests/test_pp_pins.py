"""CPU pins of the GTH pseudopotential closed forms, term by term.

oracle/pp.py (the checker of pp.hip) and the longdouble restatement in tests/pp_reference.py both write closed forms; here each
closed form is compared with 30-digit quadrature of its integral definition (tests/pp_reference.py, part 1), which shares no
formula with either.  Tolerances: the float64 oracle gets 1e-13 relative to the value - the quadrature is good to better than
1e-20 and a quartic in x^2 costs a few ulp - or 1e-13 of the scale of the terms where the value is below a tenth of that scale,
that is where it passes through a root.  The longdouble restatement gets the same few-ulp allowance in its own format, 64 of its
ulp (6.9e-18).  The last tests measure the float64 oracle against the longdouble restatement on every shape of
tests/test_gpu_pp.py; the device bounds there are computed from these very errors."""
import mpmath as mp
import numpy as np
import pytest
import pp_cases as pc
import pp_reference as ref
from oracle import pp as opp, pbc_tools as otools

TOL64 = 1e-13
TOLLD = 64 * float(np.finfo(np.longdouble).eps)
needs_ld = pytest.mark.skipif(not ref.LD_OK, reason=ref.LD_SKIP_REASON)


def _ld(v):
    return np.longdouble(mp.nstr(v, 28))


def _cld(v):
    return _ld(mp.re(v)) + np.clongdouble(1j) * _ld(mp.im(v))


def _check(got, want, scale, tol, what):
    """|got - want| <= tol * |want|, or tol * scale where want is below a tenth of the scale of its terms (a root)."""
    want_f, scale_f = abs(complex(want)), float(scale)
    den = want_f if want_f >= 0.1 * scale_f else scale_f
    err = abs(got - (_cld(want) if tol == TOLLD else complex(want)))
    print('%-44s rel err %.2e%s' % (what, err / den if den else 0., '' if den == want_f else ' (of scale)'))
    assert err <= tol * den, (what, float(err), den)


# (R, G): G R = 0.81, then 1.001 x the first root of the polynomial (set per (l, i) below), then G R = 3.28
QLI_ROOT_X2 = {(0, 1): 3., (0, 2): 5 - 10 ** .5, (1, 1): 5., (1, 2): 7 - 14 ** .5, (2, 1): 7., (2, 2): 9 - 18 ** .5}


@pytest.mark.parametrize('l,i', [(l, i) for l in range(3) for i in range(3)])
def test_qli_against_radial_quadrature(l, i):
    """oracle.pp.qli and the longdouble q_l,i against int p_i^l(r) 4 pi r^2 j_l(G r) dr divided by its prefactor, for G R below 1,
    within 1e-3 of the polynomial's first root (i = 0 has none: G R = 1.7) and above 3.  Measured: oracle at most 7.3e-16 of the
    value (2.7e-16 of the scale at the roots), longdouble at most 2.4e-19."""
    xr = 1.001 * QLI_ROOT_X2.get((l, i), 1.7 ** 2 / 1.001 ** 2) ** .5
    scale = abs(ref.qli(l, i, 0.45, 0.01 / 0.45))        # the polynomial at x = 0.01: its constant term
    for R, G in [(0.3, 2.7), (0.45, xr / 0.45), (0.8, 4.1)]:
        want = ref.qli(l, i, R, G)
        _check(opp.qli(np.float64(G * R), l, i), want, scale, TOL64, 'oracle qli(%d,%d) x=%.3f' % (l, i, G * R))
        if ref.LD_OK:
            _check(ref.qli_ld(ref.LD(G) * ref.LD(R), l, i), want, scale, TOLLD, 'longdouble qli(%d,%d) x=%.3f' % (l, i, G * R))


PIN_VLOC = [(2., None), (4., (0.54, [])), (3., (0.90, [-0.344])), (5., (0.29, [-12.2, 1.77])), (6., (0.33, [9.1, -4.4, 0.62])),
            (3., (0.40, [-14.0, 9.55, -1.77, 0.084]))]


def test_vlocG_against_radial_quadrature():
    """oracle.pp.get_vlocG and the longdouble v_a(G) against -4 pi int V(r) r^2 j_0(G r) dr (bare -Z/r added analytically), for a
    bare nucleus and nexp = 0..4, at G = 0 and |G| = 1.04, 2.49 and 3.73 on a triclinic mesh.  Measured: oracle at most 2.0e-16 of
    the value (6.8e-17 of the scale at G = 0 for nexp = 2 and 4, whose terms cancel there), longdouble at most 1.4e-19."""
    a, mesh = pc.LATTICES['triclinic'], (5, 5, 5)
    Gv = otools.get_Gv(2 * np.pi * np.linalg.inv(a.T), mesh)
    pick = [0, np.ravel_multi_index((1, 0, 0), mesh), np.ravel_multi_index((2, 4, 0), mesh), np.ravel_multi_index((2, 3, 2), mesh)]
    pseudo = [None if p is None else [None, p[0], len(p[1]), p[1]] for _, p in PIN_VLOC]
    got = opp.get_vlocG([z for z, _ in PIN_VLOC], pseudo, a, mesh, Gv)
    G2 = np.einsum('gx,gx->g', Gv, Gv)
    assert G2[0] == 0 and len(set(np.round(G2[pick], 6))) == 4
    for ia, (Z, p) in enumerate(PIN_VLOC):
        par = [0, Z, 0, 0, 0, 0, 0, 0] if p is None else [1, Z, p[0], len(p[1])] + p[1] + [0.] * (4 - len(p[1]))
        got_ld = ref.vlocG_atom_ld(Z, par, np.asarray(G2[pick], dtype=ref.LD))
        for n, ig in enumerate(pick):
            terms = ref.vloc_G_terms(Z, p, float(G2[ig]))
            head = 2 if (p is not None and ig != 0) else 1     # Z/r and its erfc correction are one term of the closed form
            with mp.workdps(ref.DPS):
                want = mp.fsum(terms)
                scale = abs(mp.fsum(terms[:head])) + mp.fsum(abs(t) for t in terms[head:])
            what = 'vloc Z=%g nexp=%s |G|=%.2f' % (Z, 'none' if p is None else len(p[1]), G2[ig] ** .5)
            _check(got[ia, ig], want, scale, TOL64, 'oracle ' + what)
            if ref.LD_OK:
                _check(got_ld[n], want, scale, TOLLD, 'longdouble ' + what)


PIN_FT_COORDS = np.array([[0., 0., 0.], [0.7, -0.4, 1.1]])
PIN_FT_SHELLS = [s for l in range(3) for s in [(0, l, [2.3], [[1.]]), (1, l, [0.45], [[1.]]),
                                               (1, l, [3.1, 1.1, 0.45], [[0.21, 0.55, 0.38], [-0.17, 0.09, 0.81]])]]
PIN_FT_Q = np.array([[0.9, -0.5, 1.3], [2.1, 1.7, -0.8], [0., 0., 1.7]])


def test_ft_ao_against_radial_quadrature():
    """oracle.pp.ft_ao and the longdouble transform against (-i)^l 4 pi S_lm(q/|q|) int r^(l+2) exp(-a r^2) j_l(q r) dr for l = 0, 1,
    2: exponents 2.3 (at the origin) and 0.45 (displaced centre), a shell of three primitives and two contractions, three q of
    which one lies along z, where the x, y, xy, yz, xz and x^2-y^2 harmonics vanish (held to the scale of the shell's largest
    component there).  Measured: oracle at most 5.6e-16, longdouble at most 3.4e-19."""
    atm, bas, env = pc.make_tables(PIN_FT_COORDS, PIN_FT_SHELLS)
    got = opp.ft_ao(atm, bas, env, PIN_FT_Q)
    got_ld = ref.ft_ao_ld(bas, env, np.asarray(PIN_FT_COORDS, dtype=ref.LD), np.asarray(PIN_FT_Q, dtype=ref.LD))
    for iq, q in enumerate(PIN_FT_Q):
        p0 = 0
        for ia, l, es, cs in PIN_FT_SHELLS:
            want = ref.ft_shell(l, es, cs, PIN_FT_COORDS[ia], q)
            prim = [ref.ft_gaussian(l, e, tuple(float(t) for t in q)) for e in es]
            for k, ck in enumerate(cs):
                scale = max(mp.fsum(abs(c * p[m]) for c, p in zip(ck, prim)) for m in range(2 * l + 1))
                for m in range(2 * l + 1):
                    what = 'ft_ao l=%d nprim=%d k=%d m=%d q%d' % (l, len(es), k, m, iq)
                    _check(got[iq, p0], want[k][m], scale, TOL64, 'oracle ' + what)
                    if ref.LD_OK:
                        _check(got_ld[iq, p0], want[k][m], scale, TOLLD, 'longdouble ' + what)
                    p0 += 1
        assert p0 == got.shape[1]
    assert np.all(got[2, [4, 5]] == 0) and abs(got[2, 6]) > 0.1          # q along z: the p_x, p_y of the first p shell vanish


def _report(name, got, want):
    scale = abs(want).max()
    err = abs(got - want).max()
    print('%-40s oracle error %.2e of max|ref| = %.3g  -> device bound %.2e' % (name, err / scale, scale,
                                                                              pc.device_bound(err, scale) / scale))
    return float(err / scale)


@needs_ld
@pytest.mark.parametrize('lat,par', pc.VLOC_CASES)
def test_oracle_vlocR_error_against_longdouble(lat, par):
    """The float64 oracle's vlocR against the longdouble restatement on the shapes of the device test, relative to max|vlocR|, and
    the same for the mean over the mesh (the G = 0 term), relative to the mean.  Measured (whole array / mean), nexp024 then
    nexp13: triclinic (10,9,8) 5.4e-16 / 6.3e-17 and 4.1e-16 / 3.3e-16; fcc (12,12,12) 2.1e-15 / 9.5e-17 and 1.8e-15 / 2.2e-16;
    cubic (15,14,16) 1.6e-15 / 5.5e-17 and 1.2e-15 / 1.9e-16.  So every device bound is its floor of 64 ulp = 1.4e-14, but for
    fcc nexp024 (1.6e-14).  Asserted here: the rule stays under its 1e-11 cap."""
    want, got = pc.cached(pc.vloc_ld, lat, par), pc.cached(pc.vloc_oracle, lat, par)
    assert _report('vlocR %s %s' % (lat, par), got, want) < pc.CAP / pc.MARGIN
    mw, mg = want.sum() / want.size, got.astype(ref.LD).sum() / got.size
    assert _report('  its mean', np.array([mg]), np.array([mw])) < pc.CAP / pc.MARGIN


@needs_ld
@pytest.mark.parametrize('mesh,kname', pc.OV_CASES)
def test_oracle_overlap_error_against_longdouble(mesh, kname):
    """The float64 oracle's (40, 22) projector/AO overlaps against the longdouble restatement on the shapes of the device test,
    relative to the largest entry (8.3).  Measured, Gamma / k: (10,9,8) 1.9e-15 / 1.4e-15; (32,32,16) 1.2e-14 / 9.2e-15;
    (29,29,20) 1.3e-14 / 1.1e-14; (33,32,32) 1.7e-14 / 1.3e-14 (the oracle's einsum adds the G terms in sequence, so its error
    grows with the mesh).  Device bounds from these: 1.5e-14, 1.4e-14 (floor), 9.5e-14, 7.3e-14, 1.1e-13, 9.0e-14, 1.4e-13,
    1.0e-13.  Asserted here: the rule stays under its 1e-11 cap."""
    want, got = pc.cached(pc.ov_ld, mesh, kname), pc.cached(pc.ov_oracle, mesh, kname)
    assert want.shape == (40, 22)
    assert _report('overlaps %s %s' % (mesh, kname), got, want) < pc.CAP / pc.MARGIN


@needs_ld
def test_oracle_error_on_the_symmetry_and_end_to_end_shapes():
    """The same measurement for the two remaining device shapes.  Overlaps on the small orthorhombic lattice at Gamma: 9.8e-16 of
    the largest entry (7.6), and the entries that vanish by symmetry (pp_cases.symmetry_zero_entries) are 4e-21 of it in the
    longdouble restatement - zero to its rounding - and 1.9e-18 in the oracle.  get_pp of the two-atom cell with the fixture's
    Ge and Y entries: Gamma (real part) 7.1e-15 and k 4.1e-15 of the largest entry (1.9); the longdouble k-point matrix is
    Hermitian to 2.3e-19."""
    want, got = pc.cached(pc.ov_ld, (10, 9, 8), 'gamma', 'ortho_small'), pc.cached(pc.ov_oracle, (10, 9, 8), 'gamma', 'ortho_small')
    assert _report('overlaps orthorhombic', got, want) < pc.CAP / pc.MARGIN
    zero = pc.symmetry_zero_entries()
    assert len(zero) == 27
    assert max(abs(want[i, j]) for i, j in zero) < 64 * np.finfo(np.longdouble).eps * abs(want).max()
    cell = pc.e2e_cell()
    want, got = pc.e2e_ld(cell), pc.e2e_oracle(cell)
    assert _report('get_pp Gamma', got[0], want[0].real) < pc.CAP / pc.MARGIN
    assert _report('get_pp k', got[1], want[1]) < pc.CAP / pc.MARGIN
    assert abs(want[1] - want[1].conj().T).max() < 64 * np.finfo(np.longdouble).eps * abs(want[1]).max()


def test_parser_reads_the_fixture():
    """gto.parse_pseudo on tests/golden/gth_pade_cases.dat: multi-line upper triangles come back as symmetric h, nexp = 0 gives
    an empty coefficient list, a channel with n_l = 0 keeps its position, and load_pseudo still reads the bundled file."""
    from pyscf_isdf_amd import gto
    ge, y, ca, li, n = [pc.fixture_entry(s) for s in ('Ge', 'Y', 'Ca', 'Li', 'N')]
    assert ge[:5] == [[2, 2], 0.54, 0, [], 3]
    assert [c[1] for c in ge[5:]] == [3, 2, 1] and [c[0] for c in ge[5:]] == [0.49374254, 0.60106438, 0.78836851]
    assert ge[5][2] == [[3.82689099, -0.42611775, -0.32795553], [-0.42611775, 1.10023129, 0.84677753],
                        [-0.32795553, 0.84677753, -1.34421765]]
    assert ge[6][2] == [[1.36251781, 0.26511216], [0.26511216, -0.62736987]] and ge[7][2] == [[0.19120485]]
    assert y[:5] == [[2, 0, 1], 0.9, 1, [-0.34389132], 3] and [c[1] for c in y[5:]] == [3, 2, 2]
    assert y[7] == [0.6538506, 2, [[-1.25692979, 0.03323415], [0.03323415, -0.07536797]]]
    for e in (ge, y, ca):
        for rl, nl, h in e[5:]:
            assert np.shape(h) == (nl, nl) and np.array_equal(h, np.transpose(h))
    assert ca[:5] == [[4, 6], 0.39, 2, [-4.92814602, -1.23285409], 3] and [c[1] for c in ca[5:]] == [2, 2, 1]
    assert li == [[3], 0.4, 4, [-14.03486849, 9.55347627, -1.76648817, 0.08436998], 0]
    assert n[4] == 2 and n[5] == [0.25660487, 1, [[13.55224272]]] and n[6] == [0.27013369, 0, []]
    with pytest.raises(KeyError):
        pc.fixture_entry('Mg')
    assert gto.load_pseudo('gth-pade', 'Mg')[1:4] == [0.21094954, 2, [-19.41900751, 2.87133099]]
    assert gto.load_pseudo('GTH_PADE', 'C')[5:] == [[0.30455321, 1, [[9.52284179]]], [0.2326773, 0, []]]
