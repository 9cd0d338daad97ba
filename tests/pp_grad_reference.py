"""Numpy restatements of the pseudopotential force pieces (TEST-ONLY, helper module, not a test): get_pp_ip1 and pp_nuc_grad
written from their formulas on the oracle's pieces (oracle.pp.get_vlocG / ft_ao / qli / solid_harmonics, the oracle's deriv-1
collocation), and numpy.longdouble forms of the two new device outputs - the i G_x weighted projector overlaps and the local
Hellmann-Feynman force - on the pieces of tests/pp_reference.py.

The local force is stated here as it is defined, one inverse transform per atom and direction,
    HF[s, a, x] = sum_g rho_s(g) Re ifft(i G_x SI_a vloc_a)(g),
not by the Parseval sum the device evaluates.  E_pp(R; D) = sum D_(nu mu) get_pp_(mu nu); phi_mu = phi(r - R_mu), so
d phi_mu / d R_mu = - grad phi_mu, and at Gamma S_(j mu) depends on R_a - R_mu only: dS/dR_a = S^x = - dS/dR_mu."""
import numpy as np
import pp_reference as ref
import pp_cases as pc
from oracle import ao as oao, pp as opp, pbc_tools as otools

LD, CLD = ref.LD, ref.CLD


# ---- float64, on the oracle's pieces -------------------------------------------------------------------------------------
def overlaps_ip_oracle(atm, bas, env, coords, kpt, proj_tab, proj_rl, mesh, a):
    """(4, nrows, nao): pp_cases.overlaps_oracle and its three i G_x weighted forms (G the lattice vector, not G + k)."""
    Gv = otools.get_Gv(2 * np.pi * np.linalg.inv(a.T), mesh)
    SI = np.exp(-1j * np.dot(coords, Gv.T))
    Gk = Gv + kpt
    Gr = np.linalg.norm(Gk, axis=1)
    aokG = opp.ft_ao(atm, bas, env, Gk) * (1. / abs(np.linalg.det(a))) ** .5
    wts = [np.ones(len(Gv))] + [1j * Gv[:, x] for x in range(3)]
    rows = [[] for _ in wts]
    for (ia, l, i), rl in zip(proj_tab, proj_rl):
        S = np.array(opp.solid_harmonics(l, Gk))
        pY = rl ** (l + 1.5) * np.pi ** 1.25 * np.exp(-.5 * rl ** 2 * Gr ** 2) * S * opp.qli(Gr * rl, l, i)
        for c, wt in enumerate(wts):                          # the contraction as oracle.pp.get_pp / pp_cases.overlaps_oracle write it
            rows[c].append(np.einsum('g,mg,gp->mp', wt * SI[ia].conj(), pY, aokG))
    return np.array([np.vstack(r) for r in rows])


def local_force_oracle(rho, coords, pp_par, mesh, a):
    """(nset, natm, 3) in float64, numpy's FFT."""
    Gv = otools.get_Gv(2 * np.pi * np.linalg.inv(a.T), mesh)
    vG = opp.get_vlocG(pp_par[:, 1], pc._pseudo_of(pp_par), a, mesh, Gv)
    SI = np.exp(-1j * np.dot(coords, Gv.T))
    out = np.zeros((len(rho), len(coords), 3))
    for ia in range(len(coords)):
        for x in range(3):
            d = np.fft.ifftn((1j * Gv[:, x] * SI[ia] * vG[ia]).reshape(tuple(mesh))).real.ravel()
            out[:, ia, x] = rho.dot(d)
    return out


def cell_tables(cell):
    """ps (one GTH entry or None per atom), pp_par, proj_tab, proj_rl, blocks (row0, l, nl, h, atom), nrows - read off the cell
    independently of hcore.py."""
    ps = [(getattr(cell, '_pseudo', None) or {}).get(cell.atom_symbol(i)) for i in range(cell.natm)]
    pp_par = np.zeros((cell.natm, 8))
    proj_tab, proj_rl, blocks, row = [], [], [], 0
    for ia, pp in enumerate(ps):
        pp_par[ia, 1] = cell.atom_charges()[ia]
        if pp is None:
            continue
        pp_par[ia, 0], pp_par[ia, 2], pp_par[ia, 3] = 1, pp[1], pp[2]
        pp_par[ia, 4:4 + pp[2]] = pp[3]
        for l, (rl, nl, hl) in enumerate(pp[5:]):
            if nl:
                blocks.append((row, l, nl, np.asarray(hl, dtype=float), ia))
                proj_tab += [(ia, l, i) for i in range(nl)]
                proj_rl += [rl] * nl
                row += nl * (2 * l + 1)
    return ps, pp_par, proj_tab, proj_rl, blocks, row


class CellSetup:
    """The grid, images, cutoffs and deriv-1 collocation (4, G, nao) of a cell, and tr(D get_pp) of the oracle at a displaced
    geometry (env with other atom coordinates)."""

    def __init__(self, cell):
        from pyscf_isdf_amd import gto
        self.cell = cell
        self.a, self.mesh = np.asarray(cell.lattice_vectors(), dtype=float), np.asarray(cell.mesh)
        self.coords = cell.get_uniform_grids()
        self.rcut = gto.estimate_rcut_per_shell(cell)
        self.Ls = gto.get_lattice_Ls(cell, rcut=self.rcut.max())
        self.ptr = np.asarray(cell._atm)[:, gto.PTR_COORD]
        self.tables = cell_tables(cell)
        self.ao4 = self.collocate(np.asarray(cell._env))

    def collocate(self, env):
        cell = self.cell
        return oao.eval_ao_deriv1(cell._atm, cell._bas, env, self.coords, self.Ls, self.rcut)

    def atom_coords(self, env):
        return np.array([env[p:p + 3] for p in self.ptr])

    def get_pp(self, env):
        cell = self.cell
        ao = oao.eval_ao(cell._atm, cell._bas, env, self.coords, self.Ls, self.rcut, rule='point')
        return opp.get_pp(cell._atm, cell._bas, env, self.atom_coords(env), cell.atom_charges(), self.tables[0], self.a, self.mesh,
                          self.coords, [np.asarray(ao, dtype=complex)], np.zeros((1, 3)))[0]

    def vlocR(self):
        cell = self.cell
        Gv = otools.get_Gv(2 * np.pi * np.linalg.inv(self.a.T), self.mesh)
        SI = np.exp(-1j * np.dot(cell.atom_coords(), Gv.T))
        vG = -np.einsum('ij,ij->j', SI, opp.get_vlocG(cell.atom_charges(), self.tables[0], self.a, self.mesh, Gv))
        return np.fft.ifftn(vG.reshape(tuple(self.mesh))).real.ravel()

    def overlaps_ip(self):
        cell = self.cell
        _, _, proj_tab, proj_rl, _, _ = self.tables
        return overlaps_ip_oracle(np.asarray(cell._atm), np.asarray(cell._bas), np.asarray(cell._env), cell.atom_coords(), np.zeros(3),
                                  proj_tab, proj_rl, self.mesh, self.a)


def get_pp_ip1(su):
    """(vloc, vnl), each (3, nao, nao): vloc[x, mu, nu] = sum_g d_x phi_mu vlocR phi_nu, vnl[x, mu, nu] = 1/vol Re sum_blocks
    conj(S^x)_(i m mu) h_ij S_(j m nu)."""
    vloc = np.einsum('xgm,g,gn->xmn', su.ao4[1:], su.vlocR(), su.ao4[0], optimize=True)
    nao = su.ao4.shape[2]
    vnl = np.zeros((3, nao, nao))
    S4 = su.overlaps_ip()
    vol = abs(np.linalg.det(su.a))
    for row0, l, nl, hl, _ in su.tables[4]:
        deg = 2 * l + 1
        S = S4[0, row0:row0 + nl * deg].reshape(nl, deg, nao)
        Sx = S4[1:, row0:row0 + nl * deg].reshape(3, nl, deg, nao)
        vnl += np.einsum('ximp,ij,jmq->xpq', Sx.conj(), hl, S, optimize=True).real / vol
    return vloc, vnl


def pp_nuc_grad_terms(su, dm):
    """dict of (natm, 3) arrays for one symmetric dm: hf_loc, pulay_loc, hf_nl, pulay_nl."""
    cell = su.cell
    natm = cell.natm
    _, pp_par, _, _, blocks, _ = su.tables
    rho = np.einsum('gm,mn,gn->g', su.ao4[0], dm, su.ao4[0], optimize=True)
    hf_loc = local_force_oracle(rho[None], cell.atom_coords(), pp_par, su.mesh, su.a)[0]
    vloc, _ = get_pp_ip1(su)
    aosl = np.asarray(cell.aoslice_by_atom())[:, -2:]
    pulay_loc = np.array([-2 * np.einsum('xmn,nm->x', vloc[:, p0:p1], dm[:, p0:p1]) for p0, p1 in aosl])
    hf_nl, pulay_nl = np.zeros((natm, 3)), np.zeros((natm, 3))
    S4 = su.overlaps_ip()
    vol = abs(np.linalg.det(su.a))
    nao = dm.shape[0]
    for row0, l, nl, hl, ia in blocks:
        deg = 2 * l + 1
        S = S4[0, row0:row0 + nl * deg].reshape(nl, deg, nao)
        Sx = S4[1:, row0:row0 + nl * deg].reshape(3, nl, deg, nao)
        v = np.einsum('ximp,ij,jmq->xpq', Sx.conj(), hl, S, optimize=True).real / vol       # this block's vnl
        hf_nl[ia] += 2 * np.einsum('xmn,nm->x', v, dm)
        for ib, (p0, p1) in enumerate(aosl):
            pulay_nl[ib] -= 2 * np.einsum('xmn,nm->x', v[:, p0:p1], dm[:, p0:p1])
    return {'hf_loc': hf_loc, 'pulay_loc': pulay_loc, 'hf_nl': hf_nl, 'pulay_nl': pulay_nl}


def pp_nuc_grad(su, dm):
    return sum(pp_nuc_grad_terms(su, dm).values())


# ---- numpy.longdouble, on the pieces of pp_reference.py -------------------------------------------------------------------
def overlaps_ip_ld(bas, env, coords, kpt, proj_tab, proj_rl, mesh, a):
    """(4, nrows, nao) clongdouble: pp_reference.overlaps_ld and its i G_x weighted forms."""
    pi = ref._ld_pi()
    Gv, vol = ref.gvec_ld(mesh, a)
    coords = ref._ld(coords)
    q = Gv + ref._ld(kpt)
    qn = np.sqrt((q * q).sum(axis=1))
    aoG = ref.ft_ao_ld(bas, env, coords, q) / np.sqrt(vol)
    rows = []
    for (ia, l, i), rl in zip(np.asarray(proj_tab).reshape(-1, 3), proj_rl):
        rl = LD(rl)
        base = rl ** (l + LD(1.5)) * pi ** LD(1.25) * np.exp(-rl * rl * qn * qn / 2) * ref.qli_ld(qn * rl, int(l), int(i))
        ph = ref._expi(Gv.dot(coords[int(ia)]))
        rows.extend(base * s * ph for s in ref.solid_harmonics_ld(int(l), q))
    rows = np.array(rows, dtype=CLD)
    return np.array([ref._matmul_c(rows, aoG)] + [ref._matmul_c(rows * (CLD(1j) * Gv[:, x]), aoG) for x in range(3)])


def local_force_ld(rho, coords, pp_par, mesh, a):
    """(nset, natm, 3) longdouble; the inverse transforms by direct summation per axis."""
    Gv, _ = ref.gvec_ld(mesh, a)
    G2 = (Gv * Gv).sum(axis=1)
    coords, pp_par, rho = ref._ld(coords), np.asarray(pp_par, dtype=float), ref._ld(rho)
    out = np.zeros((len(rho), len(coords), 3), dtype=LD)
    for ia in range(len(coords)):
        f = ref._expi(-Gv.dot(coords[ia])) * ref.vlocG_atom_ld(pp_par[ia, 1], pp_par[ia], G2)
        for x in range(3):
            z = (CLD(1j) * Gv[:, x] * f).reshape(tuple(mesh))
            for ax in range(3):
                z = ref._idft_axis(z, ax)
            out[:, ia, x] = rho.dot(z.real.ravel())
    return out


def e2e_ld(su, dm):
    """(get_pp_ip1 (3, nao, nao), pp_nuc_grad (natm, 3)) in longdouble from the restated vlocR, overlaps and local force; the AO
    values and gradients on the grid are the oracle's, taken as data."""
    cell = su.cell
    _, pp_par, proj_tab, proj_rl, blocks, _ = su.tables
    ao4, dm = ref._ld(su.ao4), ref._ld(dm)
    nao = dm.shape[0]
    vlocR = ref.vlocR_ld(cell.atom_coords(), pp_par, su.mesh, su.a)
    vol = LD(ref.gvec_ld(su.mesh, su.a)[1])
    S4 = overlaps_ip_ld(cell._bas, cell._env, cell.atom_coords(), np.zeros(3), proj_tab, proj_rl, su.mesh, su.a)
    ip1 = np.array([(ao4[1 + x].T * vlocR).dot(ao4[0]) for x in range(3)])
    rho = (ao4[0].dot(dm) * ao4[0]).sum(axis=1)
    grad = local_force_ld(rho[None], cell.atom_coords(), pp_par, su.mesh, su.a)[0]
    for row0, l, nl, hl, ia in blocks:
        deg = 2 * l + 1
        S = S4[0, row0:row0 + nl * deg].reshape(nl, deg, nao)
        Sx = S4[1:, row0:row0 + nl * deg].reshape(3, nl, deg, nao)
        v = np.einsum('ximp,ij,jmq->xpq', Sx.conj(), ref._ld(hl), S).real / vol
        ip1 = ip1 + v
        grad[ia] += 2 * np.einsum('xmn,nm->x', v, dm)
    aosl = np.asarray(cell.aoslice_by_atom())[:, -2:]
    for ib, (p0, p1) in enumerate(aosl):
        grad[ib] -= 2 * np.einsum('xmn,nm->x', ip1[:, p0:p1], dm[:, p0:p1])
    return ip1, grad


def displaced_cell(ia, x, d):
    """pp_cases.e2e_cell() with coordinate x of atom ia moved by d Bohr."""
    cell = pc.e2e_cell()
    pseudo = cell._pseudo
    atoms = [(s, np.array(c, dtype=float)) for s, c in cell._atom]
    atoms[ia][1][x] += d
    cell.atom, cell.unit = [(s, tuple(c)) for s, c in atoms], 'B'
    cell.build()
    cell._pseudo = pseudo
    return cell


# ---- cases of the device tests ------------------------------------------------------------------------------------------------
def ov_ip_ld(mesh, kname):
    _, bas, env, coords, kpt, proj_tab, proj_rl, m, a = pc.ov_inputs(mesh, kname)
    return overlaps_ip_ld(bas, env, coords, kpt, proj_tab, proj_rl, m, a)


def ov_ip_oracle(mesh, kname):
    return overlaps_ip_oracle(*pc.ov_inputs(mesh, kname))


def force_rho(lat, nset):
    """A random real density of nset rows on the mesh of the lattice's local-potential case."""
    G = int(np.prod(pc.VLOC_MESHES[lat]))
    return np.random.default_rng(5 + nset).standard_normal((nset, G))


def force_ld(lat, par, nset):
    return local_force_ld(force_rho(lat, nset), *pc.vloc_inputs(lat, par))


def force_oracle(lat, par, nset):
    return local_force_oracle(force_rho(lat, nset), *pc.vloc_inputs(lat, par))
