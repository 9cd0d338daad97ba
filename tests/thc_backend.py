"""The CPU checker backend with the two steps that came with the THC opposite-spin MP2 (TEST-ONLY): tests/rsh_backend's most derived
checker plus numpy forms of thc_pair and trace_sq, so that pyscf_isdf_amd.thc_mp2.mp2_os runs on the CPU through the product's own
orchestration."""
import numpy as np
import torch
from rsh_backend import RshGradOracleBackend


def thc_pair_numpy(xo, so, xv, sv):
    """(Xo diag(so) Xo^T) o (Xv diag(sv) Xv^T), symmetrised the way the kernel stores it: the lower triangle, mirrored."""
    a = (xo * so).dot(xo.T) * (xv * sv).dot(xv.T)
    return np.tril(a) + np.tril(a, -1).T


class ThcOracleBackend(RshGradOracleBackend):
    def thc_pair(self, Xo, so, Xv, sv, A):
        A.copy_(torch.from_numpy(thc_pair_numpy(Xo.numpy(), so.numpy(), Xv.numpy(), sv.numpy())))

    def trace_sq(self, B):
        b = B.numpy()
        return float(np.einsum('ij,ji->', b, b))
