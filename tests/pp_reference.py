"""Independent definitions of the GTH pseudopotential pieces (helper module, not a test).

Part 1 states each formula from its integral definition and evaluates it by mpmath quadrature at 30 digits; no closed form
is taken from pp.hip or oracle/pp.py.  The real solid harmonics are written from their square-root normalisations, in
libcint's order (p: x, y, z; d: xy, yz, z^2, xz, x^2-y^2).

Part 2 restates the two full device outputs (vlocR and the (rows, nao) projector/AO overlap matrix) in numpy.longdouble from
the closed forms that tests/test_pp_pins.py pins against part 1.  It is the extended-precision reference of the device tests.
"""
import functools
import mpmath as mp
import numpy as np

DPS = 30
SPLITS = [0, 1, 2, 4, 8, 16]           # every integrand here is below 1e-49 of its peak beyond r = 16 (Gaussian widths <= 1.1)

LD_OK = np.finfo(np.longdouble).eps < 2e-19
LD_SKIP_REASON = 'numpy.longdouble is no extended type on this platform (eps = %.3g)' % np.finfo(np.longdouble).eps


# ---- part 1: quadrature ------------------------------------------------------------------------------------------------
def _jl(l, z):
    """Spherical Bessel function from the ordinary one of half-integer order."""
    if z == 0:
        return mp.mpf(1 if l == 0 else 0)
    return mp.sqrt(mp.pi / (2 * z)) * mp.besselj(l + mp.mpf(1) / 2, z)


def _quad(f):
    with mp.workdps(DPS):
        return mp.quad(f, SPLITS)


def proj_G(l, i, R, G):
    """int_0^inf p_i^l(r) 4 pi r^2 j_l(G r) dr with the projector of the reference (i counted from 1)."""
    with mp.workdps(DPS):
        R, G = mp.mpf(R), mp.mpf(G)
        n = l + mp.mpf(4 * i - 1) / 2
        norm = mp.sqrt(2) / (R ** n * mp.sqrt(mp.gamma(n)))
        return _quad(lambda r: norm * r ** (l + 2 * (i - 1)) * mp.exp(-r * r / (2 * R * R)) * 4 * mp.pi * r * r * _jl(l, G * r))


def qli(l, i0, R, G):
    """The projector polynomial q_l,i (i0 counted from 0, as the kernels count) by its definition:
    pG / (pi^(5/4) G^l R^(l+3/2) exp(-(G R)^2/2))."""
    with mp.workdps(DPS):
        R, G = mp.mpf(R), mp.mpf(G)
        return proj_G(l, i0 + 1, R, G) / (mp.pi ** (mp.mpf(5) / 4) * G ** l * R ** (l + mp.mpf(3) / 2) * mp.exp(-(G * R) ** 2 / 2))


def vloc_G_terms(Z, pp, G2):
    """The terms of v(G), G = sqrt(G2), = -4 pi int V(r) r^2 j_0(G r) dr for V = -Z/r erf(r/(sqrt2 rloc)) + exp(-r^2/2rloc^2) sum_i C_i (r/rloc)^(2i-2),
    as a list (their sum is the value; the sum of their moduli is the scale a float64 evaluation can be held to).  The bare -Z/r
    goes in analytically as 4 pi Z / G^2 (dropped at G = 0, like the reference's coulG); the short-range rest is integrated.
    pp = None is the bare nucleus; else pp = (rloc, [C_1, ...])."""
    with mp.workdps(DPS):
        G, Z = mp.sqrt(mp.mpf(G2)), mp.mpf(Z)
        terms = [4 * mp.pi * Z / mp.mpf(G2)] if G2 != 0 else []
        if pp is None:
            return terms or [mp.mpf(0)]
        rloc = mp.mpf(pp[0])
        terms.append(-4 * mp.pi * _quad(lambda r: Z * mp.erfc(r / (mp.sqrt(2) * rloc)) * r * _jl(0, G * r)))
        for i, C in enumerate(pp[1]):
            terms.append(-4 * mp.pi * _quad(lambda r: mp.mpf(C) * (r / rloc) ** (2 * i) * mp.exp(-r * r / (2 * rloc * rloc))
                                            * r * r * _jl(0, G * r)))
        return terms


def solid_harmonics_mp(l, x, y, z):
    if l == 0:
        return [1 / (2 * mp.sqrt(mp.pi))]
    if l == 1:
        c = mp.sqrt(3 / (4 * mp.pi))
        return [c * x, c * y, c * z]
    c15, c5 = mp.sqrt(15 / mp.pi), mp.sqrt(5 / mp.pi)
    return [c15 / 2 * x * y, c15 / 2 * y * z, c5 / 4 * (2 * z * z - x * x - y * y), c15 / 2 * x * z, c15 / 4 * (x * x - y * y)]


@functools.lru_cache(maxsize=None)
def ft_gaussian(l, a, q):
    """FT[S_lm(r) exp(-a r^2)](q) for all m: (-i)^l 4 pi S_lm(q/|q|) int_0^inf r^(l+2) exp(-a r^2) j_l(|q| r) dr; q a tuple."""
    with mp.workdps(DPS):
        a = mp.mpf(a)
        q = [mp.mpf(float(t)) for t in q]
        qn = mp.sqrt(sum(t * t for t in q))
        rad = _quad(lambda r: r ** (l + 2) * mp.exp(-a * r * r) * _jl(l, qn * r))
        S = solid_harmonics_mp(l, *[t / qn for t in q]) if qn != 0 else solid_harmonics_mp(l, 0, 0, 0)
        return [mp.mpc(0, -1) ** l * 4 * mp.pi * s * rad for s in S]


def ft_shell(l, exps, coefs, R, q):
    """(nctr, 2l+1) transform of one contracted shell centred at R: sum_p c_kp FT[...](q) exp(-i q.R)."""
    with mp.workdps(DPS):
        ph = mp.expj(-sum(mp.mpf(float(t)) * mp.mpf(float(r)) for t, r in zip(q, R)))
        prim = [ft_gaussian(l, e, tuple(float(t) for t in q)) for e in exps]
        return [[ph * sum(mp.mpf(float(c)) * p[m] for c, p in zip(ck, prim)) for m in range(2 * l + 1)] for ck in coefs]


# ---- part 2: numpy.longdouble restatement of the device outputs -----------------------------------------------------
LD = np.longdouble
CLD = np.clongdouble


def _ld_pi():
    return LD('3.14159265358979323846264338327950288')


def _ld(x):
    return np.asarray(x, dtype=LD)


def gvec_ld(mesh, a):
    """(G, 3) reciprocal vectors in FFT order and the cell volume; integer frequencies as numpy.fft.fftfreq orders them."""
    a = _ld(a).reshape(3, 3)
    cr = lambda u, v: np.array([u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]], dtype=LD)
    det = a[0].dot(cr(a[1], a[2]))
    b = 2 * _ld_pi() / det * np.array([cr(a[1], a[2]), cr(a[2], a[0]), cr(a[0], a[1])], dtype=LD)
    fr = [_ld(np.fft.fftfreq(n, 1. / n).round()) for n in mesh]
    Gv = fr[0][:, None, None, None] * b[0] + fr[1][None, :, None, None] * b[1] + fr[2][None, None, :, None] * b[2]
    return Gv.reshape(-1, 3), abs(det)


def _expi(x):
    return np.cos(x) + CLD(1j) * np.sin(x)


def qli_ld(x, l, i):
    """Closed forms of q_l,i, each pinned to the quadrature by tests/test_pp_pins.py."""
    x2, s = x * x, np.sqrt
    one = LD(1)
    if l == 0:
        return [4 * s(LD(2)) + 0 * x, 8 * s(LD(2) / 15) * (3 - x2), one * 16 / 3 * s(LD(2) / 105) * (15 - 10 * x2 + x2 * x2)][i]
    if l == 1:
        return [8 * s(one / 3) + 0 * x, 16 * s(one / 105) * (5 - x2), one * 32 / 3 * s(one / 1155) * (35 - 14 * x2 + x2 * x2)][i]
    return [8 * s(LD(2) / 15) + 0 * x, one * 16 / 3 * s(LD(2) / 105) * (7 - x2),
            one * 32 / 3 * s(LD(2) / 15015) * (63 - 18 * x2 + x2 * x2)][i]


def solid_harmonics_ld(l, q):
    pi, s = _ld_pi(), np.sqrt
    x, y, z = q[:, 0], q[:, 1], q[:, 2]
    if l == 0:
        return [np.full(len(q), 1 / (2 * s(pi)))]
    if l == 1:
        c = s(3 / (4 * pi))
        return [c * x, c * y, c * z]
    c15, c5 = s(15 / pi), s(5 / pi)
    return [c15 / 2 * x * y, c15 / 2 * y * z, c5 / 4 * (2 * z * z - x * x - y * y), c15 / 2 * x * z, c15 / 4 * (x * x - y * y)]


def vlocG_atom_ld(Z, par, G2):
    """v_a(G) of one atom; par = (has_pp, Z, rloc, nexp, C1..C4) as the device takes it."""
    pi = _ld_pi()
    zero = G2 == 0
    coul = np.where(zero, LD(0), 4 * pi / np.where(zero, LD(1), G2))
    v = LD(Z) * coul
    if par[0] == 0:
        return v
    rloc, nexp = LD(par[2]), int(par[3])
    x = G2 * rloc * rloc
    ex = np.exp(-x / 2)
    v = np.where(zero, -2 * pi * LD(Z) * rloc * rloc, v * ex)
    polys = [1 + 0 * x, 3 - x, 15 - 10 * x + x * x, 105 - 105 * x + 21 * x * x - x * x * x]
    cf = sum((LD(par[4 + i]) * polys[i] for i in range(nexp)), 0 * x)
    return v - (2 * pi) ** LD(1.5) * rloc ** 3 * ex * cf


def _idft_axis(z, axis):
    n = z.shape[axis]
    jk = np.outer(np.arange(n), np.arange(n)) % n
    W = _expi(2 * _ld_pi() * _ld(jk) / n) / n
    return np.moveaxis(np.tensordot(W, z, axes=([1], [axis])), 0, axis)


def vlocR_ld(coords, pp_par, mesh, a):
    """vlocR = ifft(-sum_a SI_a(G) v_a(G)).real on the whole mesh, the inverse transform by direct summation per axis."""
    Gv, _ = gvec_ld(mesh, a)
    G2 = (Gv * Gv).sum(axis=1)
    coords, pp_par = _ld(coords), np.asarray(pp_par, dtype=float)
    vG = np.zeros(len(Gv), dtype=CLD)
    for ia in range(len(coords)):
        vG -= _expi(-Gv.dot(coords[ia])) * vlocG_atom_ld(pp_par[ia, 1], pp_par[ia], G2)
    z = vG.reshape(tuple(mesh))
    for ax in range(3):
        z = _idft_axis(z, ax)
    return z.real.ravel()


def _matmul_c(A, B):
    """Complex product from four real ones (numpy's real longdouble loop is several times quicker than its complex one)."""
    Ar, Ai, Br, Bi = np.ascontiguousarray(A.real), np.ascontiguousarray(A.imag), np.ascontiguousarray(B.real), np.ascontiguousarray(B.imag)
    return (Ar.dot(Br) - Ai.dot(Bi)) + CLD(1j) * (Ar.dot(Bi) + Ai.dot(Br))


def ft_ao_ld(bas, env, coords, q):
    """(G, nao): closed-form transform of the AOs at wave vectors q, (-i)^l (pi/a)^(3/2) (2a)^(-l) S_lm(q) exp(-q^2/4a) exp(-iq.R)."""
    pi = _ld_pi()
    bas = np.asarray(bas).reshape(-1, 8)
    env = _ld(env)
    nao = int(sum((2 * b[1] + 1) * b[3] for b in bas))
    out = np.zeros((len(q), nao), dtype=CLD)
    q2 = (q * q).sum(axis=1)
    p0 = 0
    for b in bas:
        ia, l, npr, nc, pe, pc = int(b[0]), int(b[1]), int(b[2]), int(b[3]), int(b[5]), int(b[6])
        es, cs = env[pe:pe + npr], env[pc:pc + npr * nc].reshape(nc, npr)
        rad = np.array([(pi / e) ** LD(1.5) * (2 * e) ** (-l) * np.exp(-q2 / (4 * e)) for e in es], dtype=LD)
        rad = cs.dot(rad)
        ph = [1, CLD(-1j), -1][l] * _expi(-q.dot(coords[ia]))
        S = solid_harmonics_ld(l, q)
        for k in range(nc):
            for m in range(2 * l + 1):
                out[:, p0] = rad[k] * S[m] * ph
                p0 += 1
    return out


def overlaps_ld(bas, env, coords, kpt, proj_tab, proj_rl, mesh, a):
    """(rows, nao) = sum_G conj(SI_a(G)) p_lim(G + k) aoG(G + k) / sqrt(vol); rows in the order of proj_tab, 2l+1 rows each."""
    pi = _ld_pi()
    Gv, vol = gvec_ld(mesh, a)
    coords = _ld(coords)
    q = Gv + _ld(kpt)
    qn = np.sqrt((q * q).sum(axis=1))
    aoG = ft_ao_ld(bas, env, coords, q) / np.sqrt(vol)
    rows = []
    for (ia, l, i), rl in zip(np.asarray(proj_tab).reshape(-1, 3), proj_rl):
        rl = LD(rl)
        base = rl ** (l + LD(1.5)) * pi ** LD(1.25) * np.exp(-rl * rl * qn * qn / 2) * qli_ld(qn * rl, int(l), int(i))
        ph = _expi(Gv.dot(coords[int(ia)]))
        rows.extend(base * s * ph for s in solid_harmonics_ld(int(l), q))
    return _matmul_c(np.array(rows, dtype=CLD), aoG)


@functools.lru_cache(maxsize=None)
def cached(fn, *key):
    """Compute fn(*key) once per process; the arguments are hashable case names, the results are not to be modified."""
    out = fn(*key)
    if isinstance(out, np.ndarray):
        out.setflags(write=False)
    return out
