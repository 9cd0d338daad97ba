"""Numpy restatement of the (AO x occupied) pair space of the k-point ISDF exchange, built on
oracle.kisdf.  TEST INFRASTRUCTURE ONLY.

The periodic parts are stacked as real rows like oracle.kisdf.periodic_stack: X = [Re u; Im u] (2 nh rows) and
Psi = [Re psi~; Im psi~] with psi~^k_j = sum_nu u^k_nu C^k_nu,j sqrt(occ_j) for the SCF k-points.  The pair functions
conj(u^{k1}_mu) psi~^{k2}_j are fitted with one real Theta; their Gram matrix is

    A(r, r') = Re[S_u(r, r') conj(S_psi(r, r'))] = Re S_u Re S_psi + Im S_u Im S_psi,

Re S = xP x and Im S = xP_rot x with xP_rot = [Im xP | -Re xP].  W^q and K are those of oracle.kisdf (build_Wq, get_k_kpts):
sum_j psi^{k2}_j(r_P) conj(psi^{k2}_j(r_Q)) = (phi_P D^{k2} phi_Q^H) when D^{k2} = C C^H.
"""
import numpy as np
import scipy.linalg
from oracle import isdf as oisdf, kisdf


def rot_cols(xP):
    """xP (P, 2 n) = [Re | Im] at the points -> [Im | -Re] (the imaginary part's factor)."""
    n = xP.shape[1] // 2
    return np.hstack([xP[:, n:], -xP[:, :n]])


def occupied_stack(X, nao, orbs):
    """Psi (2 npsi_h, G) for per-k orbitals orbs[k] (N, nocc_k) complex; X's first len(orbs) blocks are the SCF k-points."""
    nh = X.shape[0] // 2
    u = X[:nh] + 1j * X[nh:]
    psi = np.vstack([np.asarray(c).T.dot(u[k * nao:(k + 1) * nao]) for k, c in enumerate(orbs)])
    return np.vstack([psi.real, psi.imag])


def gram_occ(aoP, psiP):
    """A_PP (P, P) from the stacked values at the points: aoP (P, 2 nh), psiP (P, 2 npsi_h)."""
    return aoP.dot(aoP.T) * psiP.dot(psiP.T) + rot_cols(aoP).dot(aoP.T) * rot_cols(psiP).dot(psiP.T)


def rows_occ(aoP, psiP, X, Psi):
    """B (P, G) between the points and the grid."""
    return aoP.dot(X) * psiP.dot(Psi) + rot_cols(aoP).dot(X) * rot_cols(psiP).dot(Psi)


def refine_pick_occ(X, Psi, cand, k, tol=-1.0, tie_rtol=kisdf.TIE_RTOL):
    """The final pick among candidates: pivoted Cholesky of gram_occ on the candidates."""
    A = gram_occ(X[:, cand].T, Psi[:, cand].T)
    piv, _ = oisdf.pivoted_cholesky_gram(A, k, tol=tol, tie_rtol=tie_rtol)
    return np.asarray(cand)[piv]


def fit_theta_occ(X, Psi, ip, reg_rel=0.0):
    """Theta = (A_PP + reg_rel max(diag) I)^-1 B by Cholesky; returns (theta, A_PP unshifted)."""
    A = gram_occ(X[:, ip].T, Psi[:, ip].T)
    As = A + reg_rel * np.diag(A).max() * np.eye(len(ip)) if reg_rel > 0 else A
    B = rows_occ(X[:, ip].T, Psi[:, ip].T, X, Psi)
    return scipy.linalg.cho_solve(scipy.linalg.cho_factor(As), B), A


def get_k_occ(theta, ip, ao_kpts, coords, kpts, a, mesh, dms, ao_band=None, kpts_band=None):
    """K at the band k-points (default: the k-points) from the fit theta at the grid points ip; ao_kpts: Bloch AOs (G, N)."""
    qs, qindex = kisdf.unique_q(kpts, kpts_band)
    r_ip = coords[ip]
    Ws = [kisdf.build_Wq(theta, a, mesh, q, r_ip) for q in qs]
    aoP = [np.ascontiguousarray(np.asarray(x)[ip]) for x in ao_kpts]
    aoPb = None if ao_band is None else [np.ascontiguousarray(np.asarray(x)[ip]) for x in ao_band]
    return kisdf.get_k_kpts(aoP, Ws, qindex, dms, aoP_band=aoPb)


def restated_k(df, cell, kpts, orbs, dms, kpts_band=None):
    """The restatement's K for the points an ISDF object picked (df.ip), from its own periodic parts (df.ao, the stack of the
    SCF k-points then the extra band k-points); orbs: per SCF k-point (N, nocc_k).  Returns (K, X, Psi)."""
    X = df.backend.to_host(df.ao)
    nao = cell.nao_nr()
    coords = cell.get_uniform_grids()
    kst = df._kstack
    nh = X.shape[0] // 2
    u = X[:nh] + 1j * X[nh:]
    bloch = [(u[k * nao:(k + 1) * nao] * np.exp(1j * coords.dot(kst[k]))[None, :]).T for k in range(len(kst))]
    Psi = occupied_stack(X, nao, orbs)
    theta, _ = fit_theta_occ(X, Psi, df.ip, reg_rel=df.reg_rel)
    band = None if kpts_band is None else [bloch[i] for i in df._band_index]
    return get_k_occ(theta, df.ip, bloch[:len(kpts)], coords, kpts, cell.lattice_vectors(), cell.mesh, dms,
                     ao_band=band, kpts_band=kpts_band), X, Psi
