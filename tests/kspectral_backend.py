"""The CPU checker backend with the two entry points of the k-point spectral W^q (TEST-ONLY): tests/oracle_backend.OracleBackend plus
pack_table_pm and herm_kscale_nt in numpy, and the numpy reference M_q_truncated - the DEFINING sum over the kept points of the
FULL spectrum, without any folding - that the folded device form is checked against."""
import numpy as np
import torch
from oracle_backend import OracleBackend


def half_to_full(idx, mesh):
    """(pos, neg, mult): for half-spectrum flat indices idx (in n0 x n1 x (n2/2+1)) the flat indices of G and of its index-wise
    negation (-i) mod n in the full n0 x n1 x n2 table, and the multiplicity (1 on the kz = 0 and z-Nyquist planes, else 2)."""
    n0, n1, n2 = (int(x) for x in mesh)
    n2h = n2 // 2 + 1
    idx = np.asarray(idx, dtype=np.int64)
    kz, r = idx % n2h, idx // n2h
    j, i = r % n1, r // n1
    pos = (i * n1 + j) * n2 + kz
    neg = (((-i) % n0) * n1 + ((-j) % n1)) * n2 + ((-kz) % n2)
    mult = np.where((kz == 0) | (2 * kz == n2), 1, 2)
    return pos, neg, mult


def pack_table_pm(table, mesh, idx, scale, ldx):
    """numpy gather of isdf_pack_table_pm: (s, a) of length ldx."""
    pos, neg, mult = half_to_full(idx, mesh)
    table = np.asarray(table, dtype=float).ravel()
    cp, cm = table[pos], (mult - 1) * table[neg]
    s, a = np.zeros(ldx), np.zeros(ldx)
    n = len(pos)
    s[0:2 * n:2] = s[1:2 * n:2] = scale * (cp + cm)
    a[0:2 * n:2] = a[1:2 * n:2] = scale * (cp - cm)
    return s, a


def herm_kscale_nt(A, B, s, a, alpha=1.0):
    """numpy form of isdf_herm_kscale_nt (beta = 0): (Cre, Cim)."""
    K = A.shape[1]
    Bt = np.empty_like(B)
    Bt[:, 0::2] = -B[:, 1::2]
    Bt[:, 1::2] = B[:, 0::2]
    return alpha * (A * s[:K]).dot(B.T), alpha * (A * a[:K]).dot(Bt.T)


def keep_mask_from_half(idx, mesh):
    """Boolean mask over the full spectrum (G,) of the points a packed half-spectrum list stands for: each G_j and -G_j."""
    pos, neg, _ = half_to_full(idx, mesh)
    keep = np.zeros(int(np.prod(mesh)), dtype=bool)
    keep[pos] = True
    keep[neg] = True
    return keep


def M_q_truncated(Y, table, mesh, keep_mask, w):
    """M^q_PQ = (w / G) sum_{G kept} c_q(G) Y^_P(G) conj(Y^_Q(G)) over the kept points of the full spectrum: Y (P, G) real rows,
    table (G,) the kernel table of q, keep_mask (G,) bool.  With every point kept this is w ifft(c fft(Y)) Y^T."""
    mesh = [int(x) for x in mesh]
    G = int(np.prod(mesh))
    Yh = np.fft.fftn(np.asarray(Y).reshape(-1, *mesh), axes=(1, 2, 3)).reshape(len(Y), G)
    c = np.where(keep_mask, np.asarray(table, dtype=float).ravel(), 0.0)
    return (w / G) * (Yh * c).dot(Yh.conj().T)


class KSpectralOracleBackend(OracleBackend):
    def pack_table_pm(self, table, mesh, idx, scale, s, a):
        sv, av = pack_table_pm(table.numpy(), mesh, idx.numpy(), scale, s.numel())
        s.copy_(torch.from_numpy(sv))
        a.copy_(torch.from_numpy(av))

    def herm_kscale_nt(self, A, B, s, a, Cre, Cim, alpha=1.0, beta=0.0):
        re, im = herm_kscale_nt(A.numpy(), B.numpy(), s.numpy(), a.numpy(), alpha)
        Cre.copy_(torch.from_numpy(re + beta * Cre.numpy()))
        Cim.copy_(torch.from_numpy(im + beta * Cim.numpy()))
