"""Direct RPA correlation energy from the ISDF factors.

With the Gamma-point fit as a tensor hypercontraction, (ia|jb) = sum_PQ Y_P,ia W_PQ Y_Q,jb, Y_P,ia = Phi_o[P,i] Phi_v[P,a], the
non-interacting response on the imaginary axis lives in the point basis and the direct (bubble) RPA energy needs no integral:

    S(w)_PQ = sum_ia Y_P,ia d_ia(w) Y_Q,ia,   d_ia(w) = 4 D_ia / (D_ia^2 + w^2),   D_ia = e_a - e_i > 0       (S = -chi0(iw), PSD)
    E_c^RPA = 1/(2 pi) sum_k w_k [ln det(1 + S(w_k) W) - Tr(S(w_k) W)]
    E^(2)   = -1/(4 pi) sum_k w_k Tr[(W S(w_k))^2]            (the second-order term: the direct MP2 energy, 2 e_os of mp2_os)

Per frequency: ``thc_chi0`` (S in one launch, the pair rows Y never stored, symmetric to the bit), ``gemm_nt`` (B = W S^T = W S),
``dot`` (Tr(W S) = sum_PQ W_PQ S_PQ), ``trace_sq`` (Tr[(W S)^2]) and ``logdet_lu`` (ln det(1 + W S) by LU, in place in B).  Host
orchestration only; the steps run in libmi355_isdf.so.  Closed shell, Gamma point, pair_space='ao', one device.
"""
import numpy as np
from .thc_mp2 import _refuse


def frequency_grid(nw=40, x0=0.5):
    """(freqs, weights) on [0, inf): the nw Gauss-Legendre nodes t in (-1, 1) mapped by w = x0 (1 + t) / (1 - t), with the Jacobian
    2 x0 / (1 - t)^2 in the weights.  Half of the nodes lie below x0."""
    nw, x0 = int(nw), float(x0)
    if nw < 1 or not (x0 > 0 and np.isfinite(x0)):
        raise ValueError('frequency_grid needs nw >= 1 and a finite x0 > 0, got %r, %r' % (nw, x0))
    t, wt = np.polynomial.legendre.leggauss(nw)
    return x0 * (1 + t) / (1 - t), wt * 2 * x0 / (1 - t) ** 2


class RpaResult:
    """e_corr = sum_k weights[k] terms[k] / (2 pi) (summed in grid order), terms[k] = ln det(1 + S W) - Tr(S W) at freqs[k];
    e_mp2_direct = -sum_k weights[k] Tr[(W S)^2] / (4 pi)."""

    def __init__(self, e_corr, e_mp2_direct, freqs, weights, terms):
        self.e_corr = e_corr
        self.e_mp2_direct = e_mp2_direct
        self.freqs, self.weights, self.terms = freqs, weights, terms
        self.nw = len(freqs)
        self.seconds = None                       # wall time of the loop over the frequencies

    def __repr__(self):
        return 'RpaResult(e_corr=%.12g, e_mp2_direct=%.12g, nw=%d)' % (self.e_corr, self.e_mp2_direct, self.nw)


def rpa(df, mo_coeff, mo_energy, mo_occ, nw=40, x0=0.5):
    """Direct RPA correlation energy of closed-shell Gamma-point orbitals from the factors of ``df`` (an ISDF or MultiGridFFTDF
    object; built and fitted on demand as ao2mo does) on the ``nw``-point frequency grid of ``frequency_grid``.  All orbitals passed
    are correlated: to freeze some, drop them from mo_coeff, mo_energy and mo_occ.  A determinant that is not positive means that W
    is too far from positive semidefinite for the RPA energy to be defined (a ValueError naming the frequency).  Returns an
    RpaResult."""
    import time
    _refuse(df, mo_energy, mo_occ, 'rpa')
    occ = np.asarray(mo_occ)
    e = np.asarray(mo_energy, dtype=float)
    c = np.asarray(mo_coeff)
    if np.iscomplexobj(c):
        if abs(c.imag).max() > 1e-12:
            raise NotImplementedError('rpa with complex orbitals is not implemented (real Gamma-point orbitals)')
        c = c.real
    if c.ndim != 2 or c.shape[1] != len(occ) or c.shape[0] != df.cell.nao_nr():
        raise ValueError('rpa: mo_coeff must be (nao, nmo) with nmo = len(mo_occ)')
    freqs, w = frequency_grid(nw, x0)
    eo, ev = e[occ == 2], e[occ == 0]
    delta = ev[None, :] - eo[:, None]

    if not df._built:
        if hasattr(df, '_k_requested'):           # MultiGridFFTDF: the fit lives in the parent's build
            df._k_requested = True
        df.build()
    df._ensure_fit()
    be = df.backend
    P, nao = df.aoP.shape
    no, nv = len(eo), len(ev)
    # W is there; S and B are the other two P x P buffers, Phi_o and Phi_v are P x nmo (mp2_os's buffers and accounting)
    new = 8 * (2 * P * P + P * (no + nv + 2))
    if df.max_device_memory:
        held = sum(int(b.numel()) * b.element_size() for k, b in df._bufs.items() if k not in ('thc_A', 'thc_B', 'thc_phi'))
        if held + new > int(df.max_device_memory):
            raise MemoryError('rpa needs %d bytes for S, B (P x P, P = %d) and the orbital values next to the %d bytes the '
                              'object holds: more than max_device_memory = %d' % (new, P, held, int(df.max_device_memory)))
    S = df._buffer('thc_A', (P, P))
    B = df._buffer('thc_B', (P, P))
    off = no + (no & 1)
    phi = df._buffer('thc_phi', (P, off + nv + (nv & 1)))
    phio, phiv = phi[:, :no], phi[:, off:off + nv]
    be.gemm_nt(df.aoP, be.to_device(np.ascontiguousarray(c[:, occ == 2].T, dtype=np.float64)), phio)
    be.gemm_nt(df.aoP, be.to_device(np.ascontiguousarray(c[:, occ == 0].T, dtype=np.float64)), phiv)

    t0 = time.perf_counter()
    terms, second = [], []
    for k in range(len(freqs)):
        d = be.to_device(4 * delta / (delta ** 2 + freqs[k] ** 2))
        be.thc_chi0(phio, phiv, d, S)
        be.gemm_nt(df.W, S, B)                    # W S^T: S is symmetric to the bit, so the NT form is W S exactly
        trace = be.dot(df.W.view(-1), S.view(-1)) # Tr(W S) = sum_PQ W_PQ S_QP, S_QP = S_PQ; synchronises: d may go
        second.append(be.trace_sq(B))
        logdet, sign = be.logdet_lu(B, 1.0)       # 1 + W S, factorised in place
        if sign <= 0:
            raise ValueError('rpa: det(1 + S W) is not positive at the imaginary frequency %g (point %d of %d): W is too far from '
                             'positive semidefinite for the RPA energy to be defined' % (freqs[k], k, len(freqs)))
        terms.append(logdet - trace)
    e_corr = e2 = 0.0
    for wk, tk, sk in zip(w, terms, second):      # host sums in grid order
        e_corr += wk * tk
        e2 -= wk * sk
    res = RpaResult(e_corr / (2 * np.pi), e2 / (4 * np.pi), freqs, w, np.asarray(terms))
    res.seconds = time.perf_counter() - t0
    return res
