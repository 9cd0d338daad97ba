"""CPU restatement of the short-range Becke-88 exchange of CAM-B3LYP and of the weighted sum the multigrid XC evaluates with it
(TEST-ONLY).

Becke-88 with the attenuation of Iikura, Tsuneda, Yanai and Hirao (JCP 115, 3540; libxc GGA_X_ITYH), closed shell, rho_s = rho/2:
    x = |grad rho| / (2 rho_s^(4/3)),  G(x) = -c_x - beta x^2 / (1 + 6 beta x asinh x)   (lyp_reference.b88_point),
    K = -2 G,  k = sqrt(9 pi / K) rho_s^(1/3)  (the Fermi wave vector in the LDA limit),  a = omega / (2 k),
    e_sr = 2 rho_s^(4/3) G(x) F(a)   per volume,
    F(a) = 1 - (8/3) a [sqrt(pi) erf(1/(2a)) + 2a (b - c)],  b = exp(-1/(4a^2)) - 1,  c = 2 a^2 b + 1/2.
The direct form of F cancels as a grows (at a = 1 it is 0.027 = 1 - 0.973); from A_SWITCH on the float64 restatement sums
    F = sum_(n >= 1) (-1)^(n+1) 2 / ((n+1)! (2n+1) (n+2) 4^n) a^(-2n) = 1/(36 a^2) - 1/(960 a^4) + 1/(26880 a^6) - ...
(the expansion of the direct form in u = 1/(2a), SERIES_TERMS terms).  libxc is not part of this tree: the form is pinned by the
reference's CAM-B3LYP energies (tests/test_rsh.py), the derivatives by central differences of the 30-digit energy density.

Written over the math namespaces of lyp_reference, so the same text runs on numpy arrays and on mpmath numbers.
"""
import math
import numpy as np
import scipy.special
import lyp_reference as lyp

A_SWITCH = 0.5                 # direct form below, series from here on
SERIES_TERMS = 16
# code -> ((c_slater, c_b88, c_vwn, c_lyp), vwn fit, c_b88_sr, omega, alpha, hyb): the restatement's own table
CAM_B3LYP = ((0.0, 0.35, 0.19, 0.81), 'V', 0.46, 0.33, 0.65, 0.19)


class _NP(lyp._NP):
    erf = scipy.special.erf


def _mp(digits=30):
    """lyp_reference's mpmath namespace with erf, as a subclass of its own: lyp_reference's stays as it is."""
    import mpmath
    MP, mpf = lyp._mp(digits)

    class MPR(MP):
        erf = mpmath.erf
    return MPR, mpf


def series_coefficient(n):
    """c_n of F = sum c_n a^(-2n), an exact ratio of integers rounded once."""
    return (-1) ** (n + 1) * 2.0 / (math.factorial(n + 1) * (2 * n + 1) * (n + 2) * 4 ** n)


def attenuation_direct(m, a):
    """(F, dF/da) from the closed form."""
    rpi = m.sqrt(m.pi)
    er = m.erf(1 / (2 * a))
    b = m.exp(-1 / (4 * a * a)) - 1
    c = 2 * a * a * b + 0.5
    F = 1 - 8 * a * (rpi * er + 2 * a * (b - c)) / 3
    dF = -8 * (rpi * er + 2 * a * b - 16 * a * a * a * b - 4 * a) / 3
    return F, dF


def attenuation_series(m, a, nterms=SERIES_TERMS):
    """(F, dF/da) from the expansion in 1/a^2, Horner from the smallest term."""
    t = 1 / (a * a)
    F, dF = 0 * t, 0 * t
    for n in range(nterms, 0, -1):
        c = series_coefficient(n)
        F = (F + c) * t
        dF = (dF - 2 * n * c) * t
    return F, dF / a


def attenuation(m, a):
    """(F, dF/da): float64 arrays switch between the two forms at A_SWITCH; mpmath numbers take the direct form with 40 guard
    digits (at a = 1e4 the direct dF/da loses 18)."""
    if issubclass(m, lyp._NP):                                   # lyp_reference's own numpy namespace too (it has no erf: _NP serves)
        a = np.asarray(a, dtype=float)
        low = a < A_SWITCH
        with np.errstate(all='ignore'):
            Fd, dFd = attenuation_direct(_NP, np.where(low, a, 0.5))
            Fs, dFs = attenuation_series(_NP, np.where(low, 1.0, a))
        return np.where(low, Fd, Fs), np.where(low, dFd, dFs)
    import mpmath
    with mpmath.workdps(mpmath.mp.dps + 40):
        F, dF = attenuation_direct(m, a)
    return +F, +dF


def b88_sr_point(m, r, g2, omega):
    """(exc per particle, vrho, wfac) of the short-range Becke-88, w = wfac grad rho; no threshold, rho > 0.  The derivatives:
    with f = rho_s^(4/3) G F per spin, d ln a / d rho_s = -(1 + 2 x G'/G) / (3 rho_s) and d ln a / d g_s = G' / (2 G rho_s^(4/3)),
    vrho = rho_s^(1/3) [4 (G - x G') F - a F' (G + 2 x G')] / 3,  de/d|grad rho| = G' (F + a F'/2)."""
    beta = 0.0042
    cx = 3 * m.cbrt(3 / (4 * m.pi)) / 2
    rs = r / 2
    r13 = m.cbrt(rs)
    r43 = rs * r13
    x = m.sqrt(g2) / 2 / r43
    ash = m.asinh(x)
    D = 1 + 6 * beta * x * ash
    Dp = 6 * beta * (ash + x / m.sqrt(1 + x * x))
    G = -cx - beta * x * x / D
    Gp_x = -beta * (2 * D - x * Dp) / (D * D)
    k = m.sqrt(9 * m.pi / (-2 * G)) * r13
    a = omega / (2 * k)
    F, dF = attenuation(m, a)
    xGp = x * x * Gp_x
    return 2 * r43 * G * F / r, r13 * (4 * (G - xGp) * F - a * dF * (G + 2 * xGp)) / 3, Gp_x * (F + a * dF / 2) / (2 * r43)


def b88_sr_exchange(rho, grad, omega):
    """(exc per particle, vrho, w = de/d(grad rho)) on arrays, the conventions of oracle.multigrid.b88_exchange: rho <= 1e-14 -> 0."""
    rho, grad = np.asarray(rho, dtype=float), np.asarray(grad, dtype=float)
    ok = rho > lyp.RHO_MIN
    with np.errstate(all='ignore'):
        e, v, wf = b88_sr_point(_NP, np.where(ok, rho, 1.0), (grad * grad).sum(axis=0), float(omega))
    return np.where(ok, e, 0.0), np.where(ok, v, 0.0), np.where(ok, wf, 0.0)[None] * grad


def xc_weighted_rsh(rho, grad, coeffs, fit='V', c_b88_sr=0.0, omega=0.0):
    """(exc, vrho, w) of lyp_reference.xc_weighted(coeffs, fit) + c_b88_sr short-range B88(omega)."""
    exc, vrho, w = lyp.xc_weighted(rho, grad, coeffs, fit)
    if c_b88_sr:
        e, v, ww = b88_sr_exchange(rho, grad, omega)
        exc, vrho, w = exc + c_b88_sr * e, vrho + c_b88_sr * v, w + c_b88_sr * ww
    return exc, vrho, w


def functional(code='camb3lyp', omega=None):
    """rho, grad -> (exc, vrho, w) of CAM-B3LYP, with its own omega or the caller's."""
    assert code == 'camb3lyp'
    coeffs, fit, csr, om = CAM_B3LYP[:4]
    return lambda rho, grad: xc_weighted_rsh(rho, grad, coeffs, fit, csr, om if omega is None else omega)


def xc_weighted_rsh_mp(rho, grad, coeffs, fit='V', c_b88_sr=0.0, omega=0.0, digits=30):
    """xc_weighted_rsh point by point in ``digits``-digit arithmetic, summed there and rounded to float64 at the end; the same
    thresholds (the loop of lyp_reference.xc_weighted_mp with one more term)."""
    m, mpf = _mp(digits)
    cs, cb, cv, cl, csr, om = (mpf(float(x)) for x in tuple(coeffs) + (c_b88_sr, omega))
    pars = lyp.VWN_FITS[fit]
    n = len(rho)
    exc, vrho, w = np.zeros(n), np.zeros(n), np.zeros((3, n))
    for i in range(n):
        r = mpf(float(rho[i]))
        g = [mpf(float(grad[c, i])) for c in range(3)]
        g2 = g[0] * g[0] + g[1] * g[1] + g[2] * g[2]
        e = v = wf = mpf(0)
        if cs and rho[i] > 1e-24:
            x = lyp.slater_point(m, r)
            e, v = e + cs * x[0], v + cs * x[1]
        if cb and rho[i] > lyp.RHO_MIN:
            x = lyp.b88_point(m, r, g2)
            e, v, wf = e + cb * x[0], v + cb * x[1], wf + cb * x[2]
        if cv and rho[i] > 1e-24:
            x = lyp.vwn_point(m, r, pars)
            e, v = e + cv * x[0], v + cv * x[1]
        if cl and rho[i] > lyp.RHO_MIN:
            x = lyp.lyp_point(m, r / 2, r / 2, g2 / 4, g2 / 4, g2 / 4)
            e, v, wf = e + cl * x[0] / r, v + cl * x[1], wf + cl * (x[3] + x[4] + x[5]) / 2
        if csr and rho[i] > lyp.RHO_MIN:
            x = b88_sr_point(m, r, g2, om)
            e, v, wf = e + csr * x[0], v + csr * x[1], wf + csr * x[2]
        exc[i], vrho[i] = float(e), float(v)
        for c in range(3):
            w[c, i] = float(wf * g[c])
    return exc, vrho, w
