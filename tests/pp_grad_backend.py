"""The checker backend of tests/test_jk_e1.py plus the pseudopotential entries in numpy (TEST-ONLY): pp_local_potential and
pp_projector_overlaps as oracle/pp.py has them, and the three new entries pp_projector_overlaps_ip, pp_local_force (by the
Parseval sum the device evaluates; tests/pp_grad_reference.py states the same force with one inverse transform per atom) and
rowdot3.  ``calls`` counts the new entries' use."""
import collections
import numpy as np
import torch
import pp_cases as pc
import pp_grad_reference as pgr
from e1_reference import E1OracleBackend
from oracle import pp as opp, pbc_tools as otools


class PPGradOracleBackend(E1OracleBackend):
    def __init__(self):
        self.calls = collections.Counter()

    def pp_local_potential(self, coords, pp_par, mesh, a, vlocR):
        a, pp_par = np.asarray(a, dtype=float), np.asarray(pp_par, dtype=float)
        Gv = otools.get_Gv(2 * np.pi * np.linalg.inv(a.T), mesh)
        SI = np.exp(-1j * np.dot(coords, Gv.T))
        vG = -np.einsum('ij,ij->j', SI, opp.get_vlocG(pp_par[:, 1], pc._pseudo_of(pp_par), a, mesh, Gv))
        vlocR.copy_(torch.from_numpy(np.fft.ifftn(vG.reshape(tuple(mesh))).real.reshape(tuple(vlocR.shape))))

    def pp_projector_overlaps(self, atm, bas, env, coords, kpt, proj_tab, proj_rl, mesh, a, out):
        out.copy_(torch.from_numpy(pc.overlaps_oracle(atm, bas, env, coords, kpt, proj_tab, proj_rl, mesh, np.asarray(a, dtype=float))))

    def pp_projector_overlaps_ip(self, atm, bas, env, coords, kpt, proj_tab, proj_rl, mesh, a, out):
        self.calls['pp_projector_overlaps_ip'] += 1
        out.copy_(torch.from_numpy(pgr.overlaps_ip_oracle(atm, bas, env, coords, kpt, proj_tab, proj_rl, mesh, np.asarray(a, dtype=float))))

    def pp_local_force(self, rho, coords, pp_par, mesh, a, out):
        self.calls['pp_local_force'] += 1
        a, pp_par = np.asarray(a, dtype=float), np.asarray(pp_par, dtype=float)
        Gv = otools.get_Gv(2 * np.pi * np.linalg.inv(a.T), mesh)
        vG = opp.get_vlocG(pp_par[:, 1], pc._pseudo_of(pp_par), a, mesh, Gv)
        SI = np.exp(-1j * np.dot(coords, Gv.T))
        rhoG = np.fft.fftn(rho.numpy().reshape((-1,) + tuple(int(n) for n in mesh)), axes=(1, 2, 3)).reshape(rho.shape[0], -1)
        f = np.einsum('gx,ag,sg->sax', 1j * Gv, SI * vG, rhoG.conj()).real / Gv.shape[0]
        out.copy_(torch.from_numpy(f))

    def rowdot3(self, A3, s, B, out, alpha=1.0, accumulate=False):
        self.calls['rowdot3'] += 1
        r = alpha * np.einsum('xmk,k,mk->xm', A3.numpy(), s.numpy(), B.numpy())
        out.copy_(torch.from_numpy(r + out.numpy() if accumulate else r))
