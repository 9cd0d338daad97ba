"""Dense numpy restatement of the XC nuclear force and of its derivative matrix (TEST-ONLY), on the closed-form functionals of
tests/lyp_reference.py and the ten collocation planes of tests/ao_deriv2_reference.py.  For a real symmetric D, wq = vol / G,
(exc, v_rho, w) = functional(rho, grad rho), rho = sum D phi phi, grad rho = 2 sum D grad phi phi:

    E_xc = wq sum_g rho exc
    Z_nu = v_rho phi_nu + w . grad phi_nu,   G_(x mu) = sum_y w_y d_x d_y phi_mu
    vxc_e1[x, mu, nu] = - wq sum_g [d_x phi_mu Z_nu + G_(x mu) phi_nu]
    dE_xc/dR_(A x) = - 2 sum_(mu in A) wq sum_g [d_x phi_mu (D Z)_mu + G_(x mu) (D phi)_mu]

(the AOs move with their atoms, the uniform mesh stays).  The XC codes are those of lyp_reference.WEIGHTS plus 'lda,'."""
import numpy as np
import lyp_reference as lyp
import ao_deriv2_reference as r2
from oracle import ao as oao, multigrid as omg
from pyscf_isdf_amd import gto

HESS_INDEX = np.array([[4, 5, 6], [5, 7, 8], [6, 8, 9]])          # plane of d_x d_y phi


def functional(code):
    if code == 'lda,':
        def slater(rho, grad):
            e, v = omg.slater_exchange(rho)
            return e, v, np.zeros_like(grad)
        return slater
    return lyp.functional(code)


class CellSetup:
    """The dense collocation tables of a cell: coordinates, images, cutoffs, the AO slices of the atoms, wq."""

    def __init__(self, cell):
        self.cell = cell
        self.coords = cell.get_uniform_grids()
        self.rcut = gto.estimate_rcut_per_shell(cell)
        self.Ls = gto.get_lattice_Ls(cell, rcut=self.rcut.max())
        self.weight = cell.vol / len(self.coords)
        self.aoslices = np.asarray(cell.aoslice_by_atom())[:, -2:]
        self.ptr = np.asarray(cell._atm).reshape(-1, 6)[:, 1]         # PTR_COORD of every atom

    def ao4(self, env=None):
        """(4, G, nao) from the oracle, for the cell's own coordinates or those of a displaced ``env``."""
        return oao.eval_ao_deriv1(self.cell._atm, self.cell._bas, self.cell._env if env is None else env, self.coords, self.Ls, self.rcut)

    def ao10(self):
        return r2.eval_ao_deriv2(self.cell._atm, self.cell._bas, self.cell._env, self.coords, self.Ls, self.rcut)


def density(ao4, dm):
    """rho (G,), grad rho (3, G) of the symmetric part of dm."""
    d = 0.5 * (dm + dm.T)
    B = ao4[0].dot(d)                                                 # (G, nao)
    return np.einsum('gi,gi->g', B, ao4[0]), 2.0 * np.einsum('xgi,gi->xg', ao4[1:], B)


def exc_energy(ao4, dm, code, weight):
    rho, grad = density(ao4, dm)
    exc = functional(code)(rho, grad)[0]
    return weight * float(rho.dot(exc))


def potentials(ao4, dm, code):
    """(v_rho (G,), w (3, G)) at the density of dm."""
    rho, grad = density(ao4, dm)
    _, v, w = functional(code)(rho, grad)
    return v, w


def _aow(ao10, v, w):
    Z = ao10[0] * v[:, None] + np.einsum('xg,xgi->gi', w, ao10[1:4])
    G3 = np.einsum('yg,xygi->xgi', w, ao10[HESS_INDEX])
    return Z, G3


def get_vxc_e1(ao10, dm, code, weight):
    v, w = potentials(ao10[:4], dm, code)
    Z, G3 = _aow(ao10, v, w)
    return -weight * (np.einsum('xgm,gn->xmn', ao10[1:4], Z, optimize=True) + np.einsum('xgm,gn->xmn', G3, ao10[0], optimize=True))


def xc_nuc_grad(ao10, dm, code, weight, aoslices):
    d = 0.5 * (dm + dm.T)
    v, w = potentials(ao10[:4], dm, code)
    Z, G3 = _aow(ao10, v, w)
    rows = weight * (np.einsum('xgm,gm->xm', ao10[1:4], Z.dot(d)) + np.einsum('xgm,gm->xm', G3, ao10[0].dot(d)))
    return np.array([-2.0 * rows[:, p0:p1].sum(axis=1) for p0, p1 in aoslices])


def contract_e1(e1, dm, aoslices):
    """2 sum_(mu in A) sum_nu e1[x, mu, nu] D_(nu mu), (natm, 3)."""
    d = 0.5 * (dm + dm.T)
    return np.array([2.0 * np.einsum('xmn,nm->x', e1[:, p0:p1], d[:, p0:p1]) for p0, p1 in aoslices])
