"""Opposite-spin MP2 from the ISDF factors.

At the Gamma point the fit is a tensor hypercontraction of the integrals, (pq|rs) = sum_PQ phi_p(P) phi_q(P) W_PQ phi_r(Q) phi_s(Q),
and with the Laplace transform of the energy denominator the opposite-spin energy needs no integral:

    E_OS = - sum_iajb (ia|jb)^2 / (e_a + e_b - e_i - e_j) = - sum_t w_t Tr[(W A(tau_t))^2],
    A(tau) = (Phi_o diag(e^{+e_i tau}) Phi_o^T) o (Phi_v diag(e^{-e_a tau}) Phi_v^T),   Phi_o = aoP C_occ, Phi_v = aoP C_vir.

Per quadrature point: ``thc_pair`` (A in one pass, symmetric to the bit), ``gemm_nt`` (B = W A^T = W A, 2 P^3 flop, the only cubic
step) and ``trace_sq`` (sum_PS B_PS B_SP).  Host orchestration only; the three steps run in libmi355_isdf.so.  The same-spin
(exchange-like) term is quartic in this form and is not built; closed shell, Gamma point, pair_space='ao', one device.
"""
import numpy as np


def laplace_grid(dmin, dmax, rtol=1e-8):
    """(tau, w), w > 0, with max over x in [dmin, dmax] of |x sum_t w_t exp(-x tau_t) - 1| <= rtol.

    Trapezoid rule for 1/x = int exp(s - x e^s) ds (tau = e^s, w = h e^s).  With u = s + ln x the integrand is exp(u - e^u) for every
    x, so the relative error does not depend on x but for the truncation.  Three contributions, each held to rtol / 10:
      * the step: the rule's error on the whole line is 2 sum_k |Gamma(1 + 2 pi i k / h)| ~ 2 sqrt(2 pi om) exp(-pi om / 2),
        om = 2 pi / h; the step solving that for rtol / 10 is taken 10 % shorter;
      * the lower end: int_{-inf}^{u} exp(v - e^v) dv < e^u, largest for x = dmax;
      * the upper end: int_u^inf exp(v - e^v) dv = exp(-e^u), largest for x = dmin.
    About 2.4 points per decade of dmax / dmin plus 12 per decade of 1 / rtol: 124 points for dmax / dmin = 1e4 at rtol = 1e-10."""
    dmin, dmax, rtol = float(dmin), float(dmax), float(rtol)
    if not (0.0 < dmin <= dmax) or not np.isfinite(dmax):
        raise ValueError('laplace_grid needs 0 < dmin <= dmax, got %r, %r' % (dmin, dmax))
    if not (1e-13 <= rtol <= 1e-1):
        raise ValueError('laplace_grid: rtol must lie in [1e-13, 1e-1], got %r' % rtol)
    eps = rtol / 10
    h = 0.5
    for _ in range(60):
        h = np.pi ** 2 / np.log(2 * np.sqrt(4 * np.pi ** 2 / h) / eps)
    h *= 0.9
    s_lo = np.log(eps) - np.log(dmax / dmin) - h
    s_hi = np.log(-np.log(eps)) + h
    n = int(np.ceil((s_hi - s_lo) / h)) + 1
    tau = np.exp(s_lo + h * np.arange(n))
    return tau / dmin, h * tau / dmin


class ThcMP2Result:
    """e_os = - sum_t weights[t] terms[t] (summed in grid order), e_sos = c_os e_os; terms[t] = Tr[(W A(tau_t))^2]."""

    def __init__(self, e_os, c_os, rtol, tau, weights, terms):
        self.e_os = e_os
        self.c_os = c_os
        self.e_sos = c_os * e_os
        self.rtol = rtol
        self.ngrid = len(tau)
        self.tau, self.weights, self.terms = tau, weights, terms
        self.seconds = None                       # wall time of the loop over the grid

    def __repr__(self):
        return 'ThcMP2Result(e_os=%.12g, e_sos=%.12g, ngrid=%d, rtol=%g)' % (self.e_os, self.e_sos, self.ngrid, self.rtol)


def _refuse(df, mo_energy, mo_occ, what='mp2_os'):
    """Everything mp2_os (and thc_rpa.rpa, which passes its own name) does not do, before any work: no build, no buffer, no change
    of the object."""
    if df.kpts_symm is not None:
        raise NotImplementedError('%s with k-point symmetry is not implemented (Gamma point only)' % what)
    if not df._is_gamma(df.kpts) or not df._is_gamma(df.kpts_band):
        raise NotImplementedError('%s at k-points is not implemented (Gamma point only)' % what)
    if df._sharded:
        raise NotImplementedError('%s on the grid-sharded (multi-GPU) path is not implemented (one device)' % what)
    if df.pair_space == 'occ':
        raise NotImplementedError("%s with pair_space='occ' is not implemented: its W is the fit of one density's (AO x occupied) "
                                  "pairs, not of the occupied-virtual products (pair_space='ao')" % what)
    occ = np.asarray(mo_occ)
    if occ.ndim != 1 or not np.all((occ == 0) | (occ == 2)):
        raise NotImplementedError('%s for open shells is not implemented (mo_occ must be a vector of 0 and 2)' % what)
    e = np.asarray(mo_energy, dtype=float)
    if e.shape != occ.shape:
        raise ValueError('%s: mo_energy and mo_occ differ in shape' % what)
    if not (occ == 2).any() or not (occ == 0).any():
        raise ValueError('%s needs at least one occupied and one virtual orbital' % what)
    gap = e[occ == 0].min() - e[occ == 2].max()
    if not gap > 0:
        raise ValueError('%s needs a positive gap between occupied and virtual orbital energies, got %g' % (what, gap))


def mp2_os(df, mo_coeff, mo_energy, mo_occ, rtol=1e-8, c_os=1.3):
    """Opposite-spin MP2 correlation energy of closed-shell Gamma-point orbitals from the factors of ``df`` (an ISDF or
    MultiGridFFTDF object; built and fitted on demand as ao2mo does).  ``rtol`` bounds the relative error of the Laplace quadrature
    in e_os (every term of the sum over i, a, j, b has the same sign).  Returns a ThcMP2Result; e_sos = c_os e_os (SOS-MP2: 1.3)."""
    import time
    _refuse(df, mo_energy, mo_occ)
    occ = np.asarray(mo_occ)
    e = np.asarray(mo_energy, dtype=float)
    c = np.asarray(mo_coeff)
    if np.iscomplexobj(c):
        if abs(c.imag).max() > 1e-12:
            raise NotImplementedError('mp2_os with complex orbitals is not implemented (real Gamma-point orbitals)')
        c = c.real
    if c.ndim != 2 or c.shape[1] != len(occ) or c.shape[0] != df.cell.nao_nr():
        raise ValueError('mp2_os: mo_coeff must be (nao, nmo) with nmo = len(mo_occ)')
    eo, ev = e[occ == 2], e[occ == 0]
    mid = 0.5 * (eo.max() + ev.min())            # both exponentials <= 1; the denominator does not see the shift
    tau, w = laplace_grid(2 * (ev.min() - eo.max()), 2 * (ev.max() - eo.min()), rtol)

    if not df._built:
        if hasattr(df, '_k_requested'):           # MultiGridFFTDF: the fit lives in the parent's build
            df._k_requested = True
        df.build()
    df._ensure_fit()
    be = df.backend
    P, nao = df.aoP.shape
    no, nv = len(eo), len(ev)
    # W is there; A and B are the other two P x P buffers, Phi_o and Phi_v are P x nmo
    new = 8 * (2 * P * P + P * (no + nv + 2))
    if df.max_device_memory:
        held = sum(int(b.numel()) * b.element_size() for k, b in df._bufs.items() if k not in ('thc_A', 'thc_B', 'thc_phi'))
        if held + new > int(df.max_device_memory):
            raise MemoryError('mp2_os needs %d bytes for A, B (P x P, P = %d) and the orbital values next to the %d bytes the '
                              'object holds: more than max_device_memory = %d' % (new, P, held, int(df.max_device_memory)))
    A = df._buffer('thc_A', (P, P))
    B = df._buffer('thc_B', (P, P))
    # Phi_o | Phi_v side by side, each block starting on an even column of an even row length (16-byte aligned rows)
    off = no + (no & 1)
    phi = df._buffer('thc_phi', (P, off + nv + (nv & 1)))
    phio, phiv = phi[:, :no], phi[:, off:off + nv]
    # rows of C^T with the AO index contiguous: Phi = aoP (C^T)^T on the NT kernel
    be.gemm_nt(df.aoP, be.to_device(np.ascontiguousarray(c[:, occ == 2].T, dtype=np.float64)), phio)
    be.gemm_nt(df.aoP, be.to_device(np.ascontiguousarray(c[:, occ == 0].T, dtype=np.float64)), phiv)

    t0 = time.perf_counter()
    terms = []
    for t in range(len(tau)):
        so = be.to_device(np.exp((eo - mid) * tau[t]))
        sv = be.to_device(np.exp(-(ev - mid) * tau[t]))
        be.thc_pair(phio, so, phiv, sv, A)
        be.gemm_nt(df.W, A, B)                    # W A^T: A is symmetric to the bit, so the NT form is W A exactly
        terms.append(be.trace_sq(B))              # synchronises: so and sv may go
    e_os = 0.0
    for wt, tr in zip(w, terms):                  # host sum in grid order
        e_os -= wt * tr
    res = ThcMP2Result(e_os, c_os, rtol, tau, w, np.asarray(terms))
    res.seconds = time.perf_counter() - t0
    return res
