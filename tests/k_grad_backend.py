"""The checker backend of tests/test_pp_grad.py (an E1OracleBackend with rowdot3) plus the numpy form of isdf_gemm_nn_had (TEST-ONLY).
``nn_had_calls`` lists the beta of every call, in order: the accumulation over the batches of points is visible there."""
import torch
from pp_grad_backend import PPGradOracleBackend


class KGradOracleBackend(PPGradOracleBackend):
    def __init__(self):
        super().__init__()
        self.nn_had_calls = []

    def gemm_nn_had(self, A, H, B, C, alpha=1.0, beta=0.0):
        self.nn_had_calls.append(float(beta))
        r = alpha * A.numpy().dot(H.numpy() * B.numpy())
        C.copy_(torch.from_numpy(r if beta == 0.0 else r + beta * C.numpy()))


class KGradPlainBackend(PPGradOracleBackend):
    """The same without gemm_nn_had: get_k_nuc_grad must run the composition."""
