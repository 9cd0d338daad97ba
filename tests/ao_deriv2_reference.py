"""Numpy restatement of the AO collocation with Cartesian second derivatives (TEST-ONLY): the ten planes of numint.eval_ao(deriv=2) -
value, x, y, z, xx, xy, xz, yy, yz, zz - with the loop structure, the image order and the per-point cutoff rule of
oracle.ao.eval_ao_deriv1 (an image contributes to a point iff |r - R - T| < rcut[shell]).  With R_n = sum_p c_p a_p^n exp(-a_p r^2),
d = r - R_atom - T:

    d_a d_b phi = (d_a d_b ang) R_0 - 2 [d_b d_a ang + d_a d_b ang + delta_ab ang] R_1 + 4 d_a d_b ang R_2.

``dtype=np.longdouble`` evaluates the same text in extended precision (the cutoff decisions stay those of float64), which measures
the float64 restatement's own rounding error."""
import numpy as np
from oracle import ao as oao
from oracle.ao import (ATOM_OF, ANG_OF, NPRIM_OF, NCTR_OF, PTR_EXP, PTR_COEFF, BAS_SLOTS, PTR_COORD, ATM_SLOTS, FAC_S, FAC_P,
                       D_XY, D_Z2_ZZ, D_Z2_XXYY, D_X2Y2, F_3, F_2M, F_1, F_0, F_2)

HESS_PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))       # planes 4 .. 9


def _angular_hess(l, dx, dy, dz):
    """Second derivatives of the real-spherical angular polynomials of oracle.ao._angular: per m a dict (a, b) -> array, a <= b."""
    z = np.zeros_like(dx)
    o = np.ones_like(dx)

    def rows(*entries):
        out = []
        for e in entries:
            h = {p: z for p in HESS_PAIRS}
            h.update(e)
            out.append(h)
        return out
    if l == 0:
        return rows({})
    if l == 1:
        return rows({}, {}, {})
    if l == 2:
        return rows({(0, 1): D_XY * o}, {(1, 2): D_XY * o},
                    {(0, 0): -2 * D_Z2_XXYY * o, (1, 1): -2 * D_Z2_XXYY * o, (2, 2): 2 * D_Z2_ZZ * o},
                    {(0, 2): D_XY * o}, {(0, 0): 2 * D_X2Y2 * o, (1, 1): -2 * D_X2Y2 * o})
    if l == 3:
        return rows({(0, 0): 6 * F_3 * dy, (0, 1): 6 * F_3 * dx, (1, 1): -6 * F_3 * dy},
                    {(0, 1): F_2M * dz, (0, 2): F_2M * dy, (1, 2): F_2M * dx},
                    {(0, 0): -2 * F_1 * dy, (0, 1): -2 * F_1 * dx, (1, 1): -6 * F_1 * dy, (1, 2): 8 * F_1 * dz, (2, 2): 8 * F_1 * dy},
                    {(0, 0): -6 * F_0 * dz, (0, 2): -6 * F_0 * dx, (1, 1): -6 * F_0 * dz, (1, 2): -6 * F_0 * dy, (2, 2): 12 * F_0 * dz},
                    {(0, 0): -6 * F_1 * dx, (0, 1): -2 * F_1 * dy, (0, 2): 8 * F_1 * dz, (1, 1): -2 * F_1 * dx, (2, 2): 8 * F_1 * dx},
                    {(0, 0): 2 * F_2 * dz, (0, 2): 2 * F_2 * dx, (1, 1): -2 * F_2 * dz, (1, 2): -2 * F_2 * dy},
                    {(0, 0): 6 * F_3 * dx, (0, 1): -6 * F_3 * dy, (1, 1): -6 * F_3 * dx})
    raise NotImplementedError('l > 3')


def eval_ao_deriv2(atm, bas, env, coords, Ls, rcut, dtype=np.float64):
    """(10, G, nao) at the Gamma point: planes 0 .. 3 as oracle.ao.eval_ao_deriv1, planes 4 .. 9 the second derivatives in the order
    of HESS_PAIRS."""
    atm = np.asarray(atm).reshape(-1, ATM_SLOTS)
    bas = np.asarray(bas).reshape(-1, BAS_SLOTS)
    coords64 = np.asarray(coords, dtype=np.float64)
    coords = coords64.astype(dtype)
    env_t = np.asarray(env, dtype=np.float64).astype(dtype)
    G = coords.shape[0]
    loc = oao.ao_loc(bas)
    out = np.zeros((10, loc[-1], G), dtype=dtype)
    rcut = np.asarray(rcut, dtype=float)
    for ia in range(len(atm)):
        shl = np.where(bas[:, ATOM_OF] == ia)[0]
        if len(shl) == 0:
            continue
        p0 = atm[ia, PTR_COORD]
        rc_max = rcut[shl].max()
        for L in Ls:
            d64 = coords64 - (np.asarray(env[p0:p0 + 3], dtype=np.float64) + L)
            rr64 = np.einsum('gx,gx->g', d64, d64)
            if not (rr64 < rc_max * rc_max).any():
                continue
            d = coords - (env_t[p0:p0 + 3] + np.asarray(L, dtype=np.float64).astype(dtype))
            rr = np.einsum('gx,gx->g', d, d)
            for ib in shl:
                l, npr, nc = bas[ib, ANG_OF], bas[ib, NPRIM_OF], bas[ib, NCTR_OF]
                idx = np.nonzero(rr64 < rcut[ib] * rcut[ib])[0]
                if idx.size == 0:
                    continue
                es = env_t[bas[ib, PTR_EXP]:bas[ib, PTR_EXP] + npr]
                cs = env_t[bas[ib, PTR_COEFF]:bas[ib, PTR_COEFF] + npr * nc].reshape(nc, npr)
                fac = FAC_S if l == 0 else (FAC_P if l == 1 else 1.0)
                e = np.exp(-np.outer(es, rr[idx])) * fac
                rad, rad1, rad2 = cs.dot(e), (cs * es).dot(e), (cs * es * es).dot(e)
                dd = [d[idx, 0], d[idx, 1], d[idx, 2]]
                ang = oao._angular(l, *dd)
                gang = oao._angular_grad(l, *dd)
                hang = _angular_hess(l, *dd)
                deg = 2 * l + 1
                for k in range(nc):
                    for mm in range(deg):
                        row = loc[ib] + k * deg + mm
                        out[0, row, idx] += rad[k] * ang[mm]
                        for x in range(3):
                            out[1 + x, row, idx] += gang[mm][x] * rad[k] - 2.0 * dd[x] * ang[mm] * rad1[k]
                        for h, (a, b) in enumerate(HESS_PAIRS):
                            mid = dd[b] * gang[mm][a] + dd[a] * gang[mm][b] + (ang[mm] if a == b else 0.0)
                            out[4 + h, row, idx] += hang[mm][(a, b)] * rad[k] - 2.0 * mid * rad1[k] + 4.0 * dd[a] * dd[b] * ang[mm] * rad2[k]
    return np.ascontiguousarray(out.transpose(0, 2, 1))
