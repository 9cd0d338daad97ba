"""The CPU checker backend with the functional method that came with CAM-B3LYP (TEST-ONLY): tests/lyp_backend.LypOracleBackend plus
xc_fused_rsh, evaluated by the restatement of tests/rsh_reference.py."""
import torch
import rsh_reference as rsh
from lyp_backend import LypOracleBackend


class RshOracleBackend(LypOracleBackend):
    def xc_fused_rsh(self, rho, grad, coeffs, vwn_rpa, c_b88_sr, omega, exc, vrho, w):
        e, v, ww = rsh.xc_weighted_rsh(rho.numpy(), grad.numpy(), coeffs, 'RPA' if vwn_rpa else 'V', c_b88_sr, omega)
        exc.copy_(torch.from_numpy(e))
        vrho.copy_(torch.from_numpy(v))
        w.copy_(torch.from_numpy(ww))


from xc_grad_backend import XCGradOracleBackend  # noqa: E402


class RshGradOracleBackend(XCGradOracleBackend, RshOracleBackend):
    """The same on top of the checker backend of the XC nuclear forces."""
