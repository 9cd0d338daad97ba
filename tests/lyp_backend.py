"""The CPU checker backend with the two functional methods that came with LYP (TEST-ONLY): tests/oracle_backend.OracleBackend plus
xc_fused and gga_lyp_polarised, evaluated by the restatement of tests/lyp_reference.py."""
import torch
import lyp_reference as lyp
from oracle_backend import OracleBackend


class LypOracleBackend(OracleBackend):
    def xc_fused(self, rho, grad, coeffs, vwn_rpa, exc, vrho, w):
        e, v, ww = lyp.xc_weighted(rho.numpy(), grad.numpy(), coeffs, 'RPA' if vwn_rpa else 'V')
        exc.copy_(torch.from_numpy(e))
        vrho.copy_(torch.from_numpy(v))
        w.copy_(torch.from_numpy(ww))

    def gga_lyp_polarised(self, rho, weight, ec, vxc, accumulate=False):
        r = rho.numpy()
        e, va, vb, wa, wb = lyp.lyp_polarised(r[0, 0], r[0, 1], r[1:, 0], r[1:, 1])
        ec.copy_(torch.from_numpy(weight * e))
        if not accumulate:
            vxc.zero_()
        vxc[0, 0] += torch.from_numpy(weight * va)
        vxc[0, 1] += torch.from_numpy(weight * vb)
        vxc[1:, 0] += torch.from_numpy(weight * wa)
        vxc[1:, 1] += torch.from_numpy(weight * wb)
