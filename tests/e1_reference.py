"""Numpy restatements of the FFTDF derivative matrices (TEST-ONLY): the reference's exact get_j_e1 / get_k_e1 at the Gamma point
(pyscf/pbc/df/fft_jk.py:111-175 and :304-411) on dense (4, G, nao) collocations with the oracle's fft / ifft / get_coulG, the
half-fitted ISDF form of the exchange derivative written directly, and the checker backend with isdf_gemm_nt_had3 in numpy."""
import numpy as np
import torch
from oracle import isdf as oisdf, pbc_tools as tools
from oracle_backend import OracleBackend


def _sets(dm):
    dms = np.asarray(dm, dtype=float)
    return dms.reshape(-1, dms.shape[-2], dms.shape[-1]), dms.shape


def get_j_e1(ao4, dm, a, mesh):
    """vj_e1[a] = - sum_g d_a phi_mu(g) vR(g) phi_nu(g), vR = w ifft(coulG fft(rho)) (fft_jk.py:127-138, :157-171); ao4 (4, G, nao).
    make_rho with hermi = 1 is the quadratic form of D: the density of its symmetric part."""
    dms, shape = _sets(dm)
    G = ao4.shape[1]
    w = abs(np.linalg.det(a)) / G
    coulG = tools.get_coulG(a, mesh)
    vj = np.zeros((3,) + dms.shape)
    for i, d in enumerate(dms):
        rho = np.einsum('gi,ij,gj->g', ao4[0], d, ao4[0], optimize=True)
        vR = tools.ifft(coulG * tools.fft(rho, mesh), mesh).real * w
        aow = ao4[0] * vR[:, None]
        vj[:, i] -= np.einsum('axi,xj->aij', ao4[1:], aow, optimize=True)
    return vj.reshape((3,) + shape)


def get_k_e1(ao4, dm, a, mesh, blksize=4):
    """vk_e1[a, i, k] = - w sum_g { sum_j conv[d_a phi_i phi_j](g) (D phi)_j(g) } phi_k(g) (fft_jk.py:359-403 with one k-point,
    no MO shortcut); ao4 (4, G, nao)."""
    dms, shape = _sets(dm)
    nset, nao = dms.shape[:2]
    G = ao4.shape[1]
    w = abs(np.linalg.det(a)) / G
    coulG = tools.get_coulG(a, mesh)
    ao1T = np.ascontiguousarray(ao4.transpose(0, 2, 1))            # (4, nao, G)
    ao2T = ao1T[0]
    ao_dms = [d.dot(ao2T) for d in dms]
    vR_dm = np.empty((3, nset, nao, G))
    for p0 in range(0, nao, blksize):
        p1 = min(nao, p0 + blksize)
        rho1 = np.einsum('aig,jg->aijg', ao1T[1:, p0:p1], ao2T)
        vG = tools.fft(rho1.reshape(-1, G), mesh)
        vG *= coulG
        vR = tools.ifft(vG, mesh).real.reshape(3, p1 - p0, nao, G)
        for i in range(nset):
            vR_dm[:, i, p0:p1] = np.einsum('aijg,jg->aig', vR, ao_dms[i])
    vk = np.zeros((3,) + dms.shape)
    for i in range(nset):
        vk[:, i] -= w * np.einsum('aig,jg->aij', vR_dm[:, i], ao1T[0])
    return vk.reshape((3,) + shape)


def get_k_e1_isdf(aoT, dao, ip, theta, dm, a, mesh):
    """The half-fitted form: only the pair (sig nu) of (d_a mu lam | sig nu) is interpolated, phi_sig phi_nu ~ sum_P Theta_P
    phi_sig(P) phi_nu(P).  F_P(g) = sum_(lam sig) phi_lam(g) D_(lam sig) phi_sig(P), T_a[P, mu] = w sum_g F_P(g) V_P(g) d_a phi_mu(g),
    vk_e1[a, mu, nu] = - sum_P T_a[P, mu] phi_nu(P); aoT (nao, G), dao (3, nao, G), theta (P, G)."""
    dms, shape = _sets(dm)
    G = aoT.shape[1]
    w = abs(np.linalg.det(a)) / G
    aoP = np.ascontiguousarray(aoT[:, ip].T)
    V = oisdf.coulomb_V(theta, a, mesh)
    vk = np.zeros((3,) + dms.shape)
    for i, d in enumerate(dms):
        F = aoP.dot(d.T).dot(aoT) * V                              # (P, G)
        T = w * np.einsum('pg,amg->apm', F, dao, optimize=True)
        vk[:, i] = -np.einsum('apm,pn->amn', T, aoP, optimize=True)
    return vk.reshape((3,) + shape)


class E1OracleBackend(OracleBackend):
    """The checker backend plus the numpy form of isdf_gemm_nt_had3; ``had3_calls`` counts its use."""
    had3_calls = 0

    def gemm_nt_had3(self, A, H, B3, C3, alpha=1.0, beta=0.0):
        self.had3_calls += 1
        ah = A.numpy() if H is None else A.numpy() * H.numpy()
        for x in range(3):
            C3[x].copy_(torch.from_numpy(alpha * ah.dot(B3[x].numpy().T) + beta * C3[x].numpy()))
