"""The CPU checker backend for the XC nuclear forces (TEST-ONLY): the e1 walk and rowdot3 of tests/pp_grad_backend.py, the functional
entries of tests/lyp_backend.py and numpy forms of the two new entries, eval_ao_deriv2 (tests/ao_deriv2_reference.py) and gga_aow.
``calls`` counts the new entries' use.  Collocations are remembered by their arguments: the tests walk the same few meshes many
times."""
import numpy as np
import torch
import ao_deriv2_reference as r2
from oracle import ao as oao
from pp_grad_backend import PPGradOracleBackend
from lyp_backend import LypOracleBackend

_MEMO = {}


def _remember(fn, *args):
    key = (fn.__name__,) + tuple(np.ascontiguousarray(x).tobytes() for x in args)
    if key not in _MEMO:
        _MEMO[key] = fn(*args)
    return _MEMO[key]


class XCGradOracleBackend(PPGradOracleBackend, LypOracleBackend):
    def eval_ao(self, atm, bas, env, Ls, rcut, coords_soa, ao):
        v = _remember(oao.eval_ao, atm, bas, env, coords_soa.numpy().T, Ls, rcut)
        ao[:, :v.shape[0]] = torch.from_numpy(np.ascontiguousarray(v.T))

    def eval_ao_deriv1(self, atm, bas, env, Ls, rcut, coords_soa, ao4):
        v = _remember(oao.eval_ao_deriv1, atm, bas, env, coords_soa.numpy().T, Ls, rcut)
        ao4[:, :, :v.shape[1]] = torch.from_numpy(np.ascontiguousarray(v.transpose(0, 2, 1)))

    def eval_ao_deriv2(self, atm, bas, env, Ls, rcut, coords_soa, ao10):
        self.calls['eval_ao_deriv2'] += 1
        v = _remember(r2.eval_ao_deriv2, atm, bas, env, coords_soa.numpy().T, Ls, rcut)      # (10, G, nao)
        ao10[:, :, :v.shape[1]] = torch.from_numpy(np.ascontiguousarray(v.transpose(0, 2, 1)))

    def gga_aow(self, ao10, wv, Z, G3):
        self.calls['gga_aow'] += 1
        a, w = ao10.numpy(), wv.numpy()
        Z.copy_(torch.from_numpy(w[0] * a[0] + w[1] * a[1] + w[2] * a[2] + w[3] * a[3]))
        for x, planes in enumerate(((4, 5, 6), (5, 7, 8), (6, 8, 9))):
            G3[x].copy_(torch.from_numpy(sum(w[1 + y] * a[p] for y, p in enumerate(planes))))
