"""CPU restatement of the Lee-Yang-Parr correlation and of the weighted sums the multigrid XC evaluates with it (TEST-ONLY).

LYP (Lee, Yang, Parr, PRB 37, 785; libxc GGA_C_LYP) in the gradient-only form of Miehlich, Savin, Stoll and Preuss (CPL 157, 200),
a = 0.04918, b = 0.132, c = 0.2533, d = 0.349: with rho = rho_a + rho_b, t = rho^(-1/3), omega = exp(-c t) t^11 / (1 + d t),
delta = c t + d t / (1 + d t), K = 2^(11/3) (3/10) (3 pi^2)^(2/3),
    e = -4a rho_a rho_b / (rho (1 + d t)) - a b omega G,
    G = K rho_a rho_b (rho_a^(8/3) + rho_b^(8/3)) + G_aa sigma_aa + G_ab sigma_ab + G_bb sigma_bb,
    G_aa = rho_a rho_b [(1 - 3 delta)/9 - (delta - 11)/9 rho_a / rho] - rho_b^2   (G_bb: a <-> b),
    G_ab = rho_a rho_b (47 - 7 delta)/9 - (4/3) rho^2.
libxc is not part of this tree: the form is pinned by the reference's BLYP constants (tests/test_lyp.py), its closed-form
derivatives by central differences of ``lyp_energy_density``.

The point formulas are written once over a small math namespace, so the same text runs on numpy arrays (the float64
restatement) and on mpmath numbers (the 30-digit evaluation that measures the float64 restatement's own error).
"""
import contextlib
import numpy as np
from oracle import multigrid as omg, pbc_tools as tools

LYP_ABCD = (0.04918, 0.132, 0.2533, 0.349)
RHO_MIN = 1e-14                # total densities at or below this give zero, as in oracle.multigrid.b88_exchange
# (A, b, c, x0), paramagnetic: fit V of the VWN paper (libxc LDA_C_VWN; pinned by the reference's 'lda,vwn' energies) and its fit to the
# RPA energies (libxc LDA_C_VWN_RPA; CITED from the paper, not pinned by any constant of the reference that this tree can reproduce)
_B88, _SLATER, _VWN5 = omg.b88_exchange, omg.slater_exchange, omg.vwn_correlation      # the oracle's own, whatever oracle_gga swaps
VWN_FITS = {'V': omg.VWN5, 'RPA': (0.0310907, 13.0720, 42.7198, -0.409286)}


class _NP:
    exp, cbrt, sqrt, log, atan, asinh, pi = np.exp, np.cbrt, np.sqrt, np.log, np.arctan, np.arcsinh, np.pi


def _mp(digits=30):
    import mpmath

    class MP:
        exp, cbrt, sqrt, log, atan, asinh = mpmath.exp, mpmath.cbrt, mpmath.sqrt, mpmath.log, mpmath.atan, mpmath.asinh
    mpmath.mp.dps = digits
    MP.pi = mpmath.pi
    return MP, mpmath.mpf


# ---- point formulas (no thresholds; every density positive) --------------------------------------------------------------------
def slater_point(m, r):
    e = -0.75 * m.cbrt(3 / m.pi) * m.cbrt(r)
    return e, 4 * e / 3


def vwn_point(m, r, fit):
    A, b, c, x0 = fit
    x = m.sqrt(m.cbrt(3 / (4 * m.pi * r)))
    X, X0 = x * x + b * x + c, x0 * x0 + b * x0 + c
    Q = m.sqrt(4 * c - b * b)
    at = m.atan(Q / (2 * x + b))
    ec = A * (m.log(x * x / X) + 2 * b / Q * at - b * x0 / X0 * (m.log((x - x0) ** 2 / X) + 2 * (b + 2 * x0) / Q * at))
    den = Q * Q + (2 * x + b) ** 2
    dec = A * (2 / x - (2 * x + b) / X - 4 * b / den - b * x0 / X0 * (2 / (x - x0) - (2 * x + b) / X - 4 * (b + 2 * x0) / den))
    return ec, ec - x / 6 * dec


def b88_point(m, r, g2):
    """(exc per particle, vrho, wfac) of Becke-88, w = wfac grad rho (the formulas of oracle.multigrid.b88_exchange)."""
    beta = 0.0042
    cx = 3 * m.cbrt(3 / (4 * m.pi)) / 2
    rs = r / 2
    r13 = m.cbrt(rs)
    r43 = rs * r13
    x = m.sqrt(g2) / 2 / r43
    a = m.asinh(x)
    D = 1 + 6 * beta * x * a
    Dp = 6 * beta * (a + x / m.sqrt(1 + x * x))
    G = -cx - beta * x * x / D
    Gp_x = -beta * (2 * D - x * Dp) / (D * D)
    return 2 * r43 * G / r, 4 * r13 * (G - x * x * Gp_x) / 3, Gp_x / (2 * r43)


def lyp_point(m, ra, rb, saa, sab, sbb, abcd=LYP_ABCD):
    """(e, de/drho_a, de/drho_b, de/dsigma_aa, de/dsigma_ab, de/dsigma_bb) of the energy density per volume; rho_a + rho_b > 0.
    No division by a spin density: rho_b = 0 is a regular point."""
    a, b, c, d = abcd
    K = 8 * m.cbrt(4) * 3 * m.cbrt(9 * m.pi ** 4) / 10
    r = ra + rb
    t = 1 / m.cbrt(r)
    den = 1 + d * t
    om = m.exp(-c * t) * t ** 11 / den
    dl = c * t + d * t / den
    dlp = -t * (c + d / den ** 2) / (3 * r)
    omp = om * (dl - 11) / (3 * r)
    ra83, rb83 = m.cbrt(ra) ** 8, m.cbrt(rb) ** 8
    ab, xa, xb = ra * rb, ra / r, rb / r
    c1, c2, c3 = (1 - 3 * dl) / 9, (dl - 11) / 9, (47 - 7 * dl) / 9
    Gaa = ab * (c1 - c2 * xa) - rb * rb
    Gbb = ab * (c1 - c2 * xb) - ra * ra
    Gab = ab * c3 - 4 * r * r / 3
    G = K * ab * (ra83 + rb83) + Gaa * saa + Gab * sab + Gbb * sbb
    Gaa_a = rb * (c1 - c2 * xa) + ab * (-dlp / 3 - dlp * xa / 9 - c2 * xb / r)
    Gaa_b = ra * (c1 - c2 * xa) + ab * (-dlp / 3 - dlp * xa / 9 + c2 * xa / r) - 2 * rb
    Gbb_b = ra * (c1 - c2 * xb) + ab * (-dlp / 3 - dlp * xb / 9 - c2 * xa / r)
    Gbb_a = rb * (c1 - c2 * xb) + ab * (-dlp / 3 - dlp * xb / 9 + c2 * xb / r) - 2 * ra
    Gab_a = c3 * rb - 7 * dlp * ab / 9 - 8 * r / 3
    Gab_b = c3 * ra - 7 * dlp * ab / 9 - 8 * r / 3
    G_a = K * rb * (11 * ra83 / 3 + rb83) + Gaa_a * saa + Gab_a * sab + Gbb_a * sbb
    G_b = K * ra * (11 * rb83 / 3 + ra83) + Gaa_b * saa + Gab_b * sab + Gbb_b * sbb
    f1, f1t = 1 / (r * den), d * t / (3 * den)
    e = -4 * a * ab * f1 - a * b * om * G
    va = -4 * a * rb * f1 * (1 - xa + xa * f1t) - a * b * (omp * G + om * G_a)
    vb = -4 * a * ra * f1 * (1 - xb + xb * f1t) - a * b * (omp * G + om * G_b)
    return e, va, vb, -a * b * om * Gaa, -a * b * om * Gab, -a * b * om * Gbb


# ---- float64 restatement on arrays ---------------------------------------------------------------------------------------------
def lyp_energy_density(ra, rb, saa, sab, sbb):
    """e(rho_a, rho_b, sigma_aa, sigma_ab, sigma_bb) per volume, for finite differences (positive total density)."""
    with np.errstate(all='ignore'):
        return lyp_point(_NP, *(np.asarray(x, dtype=float) for x in (ra, rb, saa, sab, sbb)))[0]


def _clean_spins(rho_a, rho_b, grad_a, grad_b):
    """A spin density <= 0 counts as zero with a zero gradient (negative ripples of the FFT)."""
    rho_a, rho_b = np.asarray(rho_a, dtype=float), np.asarray(rho_b, dtype=float)
    ka, kb = rho_a > 0, rho_b > 0
    return np.where(ka, rho_a, 0.0), np.where(kb, rho_b, 0.0), np.where(ka, grad_a, 0.0), np.where(kb, grad_b, 0.0)


def lyp_polarised(rho_a, rho_b, grad_a, grad_b):
    """(e per volume, de/drho_a, de/drho_b, w_a, w_b) with w_s = de/d(grad rho_s) = 2 vsigma_ss grad rho_s + vsigma_ab grad rho_s';
    rho_s (G,), grad_s (3, G); rho_a + rho_b <= 1e-14 -> 0."""
    ra, rb, ga, gb = _clean_spins(rho_a, rho_b, np.asarray(grad_a, dtype=float), np.asarray(grad_b, dtype=float))
    ok = ra + rb > RHO_MIN
    one = np.where(ok, ra, 1.0), np.where(ok, rb, 1.0)
    with np.errstate(all='ignore'):
        e, va, vb, vaa, vab, vbb = lyp_point(_NP, one[0], one[1], (ga * ga).sum(axis=0), (ga * gb).sum(axis=0), (gb * gb).sum(axis=0))
    e, va, vb, vaa, vab, vbb = (np.where(ok, x, 0.0) for x in (e, va, vb, vaa, vab, vbb))
    return e, va, vb, 2 * vaa * ga + vab * gb, 2 * vbb * gb + vab * ga


def lyp_closed_shell(rho, grad):
    """(exc per particle, vrho, w = de/d(grad rho)) of a spin-unpolarised density, the conventions of oracle.multigrid.b88_exchange:
    the polarised form at rho_a = rho_b = rho/2."""
    rho, grad = np.asarray(rho, dtype=float), np.asarray(grad, dtype=float)
    ok = rho > RHO_MIN
    h = np.where(ok, 0.5 * rho, 1.0)
    s = 0.25 * (grad * grad).sum(axis=0)
    with np.errstate(all='ignore'):
        e, va, vb, vaa, vab, vbb = lyp_point(_NP, h, h, s, s, s)
    return np.where(ok, e / (2 * h), 0.0), np.where(ok, va, 0.0), np.where(ok, 0.5 * (vaa + vab + vbb), 0.0)[None] * grad


def vwn_correlation(rho, fit='V'):
    """(eps_c, v_c) of the named VWN fit; rho <= 1e-24 -> 0 (oracle.multigrid.vwn_correlation is fit V)."""
    rho = np.asarray(rho, dtype=float)
    ok = rho > 1e-24
    ec, vc = vwn_point(_NP, np.where(ok, rho, 1.0), VWN_FITS[fit])
    return np.where(ok, ec, 0.0), np.where(ok, vc, 0.0)


# code -> (c_slater, c_b88, c_vwn, vwn fit, c_lyp), the restatement's own table
WEIGHTS = {'blyp': (0, 1, 0, 'V', 1), 'b88,lyp': (0, 1, 0, 'V', 1), ',lyp': (0, 0, 0, 'V', 1), 'b88,': (0, 1, 0, 'V', 0),
           'lda,vwn': (1, 0, 1, 'V', 0), 'b3lyp5': (.08, .72, .19, 'V', .81), 'b3lyp': (.08, .72, .19, 'RPA', .81),
           'b3lypg': (.08, .72, .19, 'RPA', .81)}


def xc_weighted(rho, grad, coeffs, fit='V'):
    """(exc, vrho, w) of c_s Slater + c_b B88 + c_v VWN(fit) + c_l LYP, coeffs = (c_s, c_b, c_v, c_l); the first three from the
    oracle's own closed forms."""
    cs, cb, cv, cl = coeffs
    rho, grad = np.asarray(rho, dtype=float), np.asarray(grad, dtype=float)
    exc, vrho, w = np.zeros_like(rho), np.zeros_like(rho), np.zeros_like(grad)
    if cs:
        e, v = _SLATER(rho)
        exc, vrho = exc + cs * e, vrho + cs * v
    if cb:
        e, v, ww = _B88(rho, grad)
        exc, vrho, w = exc + cb * e, vrho + cb * v, w + cb * ww
    if cv:
        e, v = _VWN5(rho) if fit == 'V' else vwn_correlation(rho, fit)
        exc, vrho = exc + cv * e, vrho + cv * v
    if cl:
        e, v, ww = lyp_closed_shell(rho, grad)
        exc, vrho, w = exc + cl * e, vrho + cl * v, w + cl * ww
    return exc, vrho, w


def functional(code):
    """rho, grad -> (exc, vrho, w) of a code of WEIGHTS."""
    cs, cb, cv, fit, cl = WEIGHTS[code]
    return lambda rho, grad: xc_weighted(rho, grad, (cs, cb, cv, cl), fit)


@contextlib.contextmanager
def oracle_gga(fn):
    """The oracle's GGA drivers (nr_rks_b88, nr_rks_b88_dense, nr_rks_b88_kpts, nr_rks_b88_dense_kpts) are functional-agnostic but
    for the one name they call: inside this context they evaluate ``fn`` (rho, grad) -> (exc, vrho, w) in its place.  The oracle
    package itself stays as it is."""
    keep = omg.b88_exchange
    omg.b88_exchange = fn
    try:
        yield omg
    finally:
        omg.b88_exchange = keep


def nr_uks_lyp(tasks, atm, dms, a, fft_mesh, c_b88=1.0, c_lyp=1.0, with_j=False):
    """(nelec, exc, veff (2, nao, nao), ecoul) of an (alpha, beta) pair at the Gamma point through the ladder, c_b88 B88 (each spin
    channel in its own variables, oracle.multigrid.b88_spin_channel) + c_lyp LYP (polarised, both spins together); the structure
    of oracle.multigrid.nr_uks_b88."""
    a = np.asarray(a, dtype=float)
    fft_mesh = np.asarray(fft_mesh)
    ngrids = int(np.prod(fft_mesh))
    vol = abs(np.linalg.det(a))
    weight = vol / ngrids
    nao = np.asarray(dms).shape[-1]
    rhoG = [omg.eval_rhoG_gga(tasks, atm, dms[s], a, fft_mesh) for s in range(2)]
    coulG = tools.get_coulG(a, fft_mesh).reshape(rhoG[0].shape[1:])
    tot = rhoG[0][0] + rhoG[1][0]
    vG = tot * coulG
    ecoul = (.5 * (tot.real * vG.real).sum() + .5 * (tot.imag * vG.imag).sum()) / vol
    rhoR = [tools.ifft(rhoG[s].reshape(4, ngrids), fft_mesh).real / weight for s in range(2)]
    ec, va, vb, wa, wb = lyp_polarised(rhoR[0][0], rhoR[1][0], rhoR[0][1:], rhoR[1][1:])
    nelec, exc, veff = 0.0, c_lyp * ec.sum() * weight, []
    for s, (vl, wl) in enumerate(((va, wa), (vb, wb))):
        f, vrho, w = omg.b88_spin_channel(rhoR[s][0], rhoR[s][1:]) if c_b88 else (np.zeros(ngrids), np.zeros(ngrids), np.zeros((3, ngrids)))
        nelec += rhoR[s][0].sum() * weight
        exc += c_b88 * f.sum() * weight
        wvG = tools.fft(weight * np.vstack([(c_b88 * vrho + c_lyp * vl)[None], c_b88 * w + c_lyp * wl]), fft_mesh).reshape(rhoG[s].shape)
        if with_j:
            wvG[0] += vG
        veff.append(omg.integrate_gga(tasks, atm, wvG, a, fft_mesh, nao))
    return nelec, exc, np.array(veff), ecoul


# ---- 30-digit evaluation of the same formulas (the float64 restatement's own error) -------------------------------------------
def xc_weighted_mp(rho, grad, coeffs, fit='V', digits=30):
    """xc_weighted point by point in ``digits``-digit arithmetic, rounded to float64 at the end; the same thresholds."""
    m, mpf = _mp(digits)
    cs, cb, cv, cl = (mpf(float(x)) for x in coeffs)
    pars, abcd = VWN_FITS[fit], LYP_ABCD                    # the same float64 constants as the restatement
    n = len(rho)
    exc, vrho, w = np.zeros(n), np.zeros(n), np.zeros((3, n))
    for i in range(n):
        r = mpf(float(rho[i]))
        g = [mpf(float(grad[c, i])) for c in range(3)]
        g2 = g[0] * g[0] + g[1] * g[1] + g[2] * g[2]
        e = v = wf = mpf(0)
        if cs and rho[i] > 1e-24:
            x = slater_point(m, r)
            e, v = e + cs * x[0], v + cs * x[1]
        if cb and rho[i] > RHO_MIN:
            x = b88_point(m, r, g2)
            e, v, wf = e + cb * x[0], v + cb * x[1], wf + cb * x[2]
        if cv and rho[i] > 1e-24:
            x = vwn_point(m, r, pars)
            e, v = e + cv * x[0], v + cv * x[1]
        if cl and rho[i] > RHO_MIN:
            x = lyp_point(m, r / 2, r / 2, g2 / 4, g2 / 4, g2 / 4, abcd)
            e, v, wf = e + cl * x[0] / r, v + cl * x[1], wf + cl * (x[3] + x[4] + x[5]) / 2
        exc[i], vrho[i] = float(e), float(v)
        for c in range(3):
            w[c, i] = float(wf * g[c])
    return exc, vrho, w


def lyp_polarised_mp(rho_a, rho_b, grad_a, grad_b, digits=30):
    """lyp_polarised point by point in ``digits``-digit arithmetic."""
    m, mpf = _mp(digits)
    abcd = LYP_ABCD
    ra, rb, ga, gb = _clean_spins(rho_a, rho_b, np.asarray(grad_a, dtype=float), np.asarray(grad_b, dtype=float))
    n = len(ra)
    e, va, vb, wa, wb = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros((3, n)), np.zeros((3, n))
    for i in range(n):
        if not ra[i] + rb[i] > RHO_MIN:
            continue
        A = [mpf(float(x)) for x in ga[:, i]]
        B = [mpf(float(x)) for x in gb[:, i]]
        dot = lambda p, q: p[0] * q[0] + p[1] * q[1] + p[2] * q[2]
        x = lyp_point(m, mpf(float(ra[i])), mpf(float(rb[i])), dot(A, A), dot(A, B), dot(B, B), abcd)
        e[i], va[i], vb[i] = float(x[0]), float(x[1]), float(x[2])
        for c in range(3):
            wa[c, i] = float(2 * x[3] * A[c] + x[4] * B[c])
            wb[c, i] = float(2 * x[5] * B[c] + x[4] * A[c])
    return e, va, vb, wa, wb
