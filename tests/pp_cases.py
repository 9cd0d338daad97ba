"""Hand-built inputs of the GTH pseudopotential kernel tests (tests/test_pp_pins.py on the CPU, tests/test_gpu_pp.py on the
device), the float64 oracle's answer per case, and the rule that turns the oracle's measured error into the device bound.
The parameters are test inputs, not chemistry.  Helper module, not a test."""
import os
import numpy as np
import pp_reference as ref
from oracle import pp as opp, pbc_tools as otools

EPS = np.finfo(np.float64).eps
MARGIN, FLOOR_ULP, CAP = 8, 64, 1e-11

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'gth_pade_cases.dat')


def fixture_entry(symb):
    from pyscf_isdf_amd import gto
    with open(FIXTURE) as f:
        return gto.parse_pseudo(f.read(), symb)


def device_bound(oracle_err, scale):
    """The bound of a device comparison, absolute: 8 x the float64 oracle's own error against the longdouble restatement on the
    same shape, never below 64 ulp of the largest reference entry ``scale``.  (8: the device's exp, sincos and pow differ from the
    host's by an ulp or two each and rocBLAS sums up to 33792 terms in another order; neither is systematic.)  A rule that yields
    more than 1e-11 of the largest entry means the reference is the problem: that fails outright."""
    b = max(MARGIN * float(oracle_err), FLOOR_ULP * EPS * float(scale))
    assert b <= CAP * float(scale), 'the oracle is off by %.3g of the largest entry: fix the reference' % (oracle_err / scale)
    return b


# ---- lattices ----------------------------------------------------------------------------------------------------------
LATTICES = {
    'triclinic': np.array([[6.1, 0.4, 0.2], [0.5, 5.8, -0.3], [0.3, 0.6, 6.4]]),
    'fcc': np.array([[0., 3.37, 3.37], [3.37, 0., 3.37], [3.37, 3.37, 0.]]),
    'cubic': np.eye(3) * 5.3,
    'ortho_small': np.diag([1.5, 1.4, 1.45]),
}

# ---- local potential ---------------------------------------------------------------------------------------------------
VLOC_MESHES = {'triclinic': (10, 9, 8), 'fcc': (12, 12, 12), 'cubic': (15, 14, 16)}
VLOC_FRAC = np.array([[0.113, 0.271, 0.059], [0.537, 0.419, 0.683], [0.291, 0.847, 0.377], [0.771, 0.133, 0.909]])
# per atom (has_pp, Z, rloc, nexp, C1..C4); unused coefficients are set, so a count that is ignored shows
VLOC_PARS = {
    'nexp024': np.array([[0, 2., 0., 0, 0., 0., 0., 0.],
                         [1, 4., 0.54, 0, 7.7, -3.3, 1.9, -0.6],
                         [1, 5., 0.29, 2, -12.2, 1.77, 2.9, -0.8],
                         [1, 3., 0.40, 4, -14.0, 9.55, -1.77, 0.084]]),
    'nexp13': np.array([[1, 3., 0.90, 1, -0.344, 5.1, -2.2, 0.7],
                        [1, 6., 0.33, 3, 9.1, -4.4, 0.62, 1.3],
                        [0, 1., 0., 0, 0., 0., 0., 0.],
                        [1, 4., 0.39, 2, -4.93, -1.23, 3.1, 0.9]]),
}
VLOC_CASES = [(lat, par) for lat in VLOC_MESHES for par in VLOC_PARS]


def vloc_inputs(lat, par):
    a = LATTICES[lat]
    return VLOC_FRAC.dot(a), VLOC_PARS[par], np.array(VLOC_MESHES[lat], dtype=np.int32), a


def _pseudo_of(par):
    return [None if p[0] == 0 else [None, p[2], int(p[3]), list(p[4:4 + int(p[3])])] for p in par]


def vloc_oracle(lat, par):
    """vlocR as oracle.pp.get_pp forms it (float64)."""
    coords, pp_par, mesh, a = vloc_inputs(lat, par)
    Gv = otools.get_Gv(2 * np.pi * np.linalg.inv(a.T), mesh)
    SI = np.exp(-1j * np.dot(coords, Gv.T))
    vG = -np.einsum('ij,ij->j', SI, opp.get_vlocG(pp_par[:, 1], _pseudo_of(pp_par), a, mesh, Gv))
    return np.fft.ifftn(vG.reshape(tuple(mesh))).real.ravel()


def vloc_ld(lat, par):
    return ref.vlocR_ld(*vloc_inputs(lat, par))


# ---- projector overlaps ------------------------------------------------------------------------------------------------
OV_MESHES = [(10, 9, 8), (32, 32, 16), (29, 29, 20), (33, 32, 32)]
OV_KPTS = {'gamma': (0., 0., 0.), 'k': (0.21, -0.13, 0.34)}
OV_CASES = [(m, k) for m in OV_MESHES for k in OV_KPTS]
OV_FRAC = np.array([[0.137, 0.211, 0.089], [0.431, 0.523, 0.467], [0.719, 0.853, 0.617]])
# (atom, l, exponents, coefficients (nctr, nprim)).  The d shells start at AO 1 and AO 17; atom 1 has AOs and no projector.
OV_SHELLS = [
    (0, 0, [1.3], [[0.9]]),
    (0, 2, [0.9], [[0.7]]),
    (1, 1, [3.1, 1.1, 0.45], [[0.21, 0.55, 0.38], [-0.17, 0.09, 0.81]]),
    (1, 0, [0.7], [[1.1]]),
    (2, 0, [2.2, 0.6], [[0.4, 0.7]]),
    (2, 1, [0.8], [[1.3]]),
    (2, 2, [1.4, 0.5], [[0.6, 0.5]]),
]
OV_S_OF_ATOM = {0: [0], 2: [13]}           # the s AOs on the atoms that carry projectors
# all nine (l, i) on atoms 0 and 2, another r_l per channel
OV_PROJ = [(0, 0, 0, 0.49), (0, 0, 1, 0.49), (0, 0, 2, 0.49), (0, 1, 0, 0.60), (0, 1, 1, 0.60), (0, 2, 0, 0.79),
           (2, 0, 0, 0.26), (2, 0, 1, 0.26), (2, 1, 0, 0.31), (2, 1, 1, 0.31), (2, 1, 2, 0.31),
           (2, 2, 0, 0.45), (2, 2, 1, 0.45), (2, 2, 2, 0.45)]
PTR_ENV_START = 20


def make_tables(coords, shells):
    """libcint-style atm / bas / env for hand-given shells (coefficients taken as they are)."""
    env, atm, bas = [np.zeros(PTR_ENV_START)], [], []
    ptr = PTR_ENV_START
    for c in coords:
        atm.append([1, ptr, 1, ptr + 3, 0, 0])
        env.append(np.append(c, 0.))
        ptr += 4
    for ia, l, es, cs in shells:
        cs = np.asarray(cs, dtype=float)
        env += [np.asarray(es, dtype=float), cs.reshape(-1)]
        bas.append([ia, l, len(es), len(cs), 0, ptr, ptr + len(es), 0])
        ptr += len(es) * (1 + len(cs))
    return np.array(atm, dtype=np.int32), np.array(bas, dtype=np.int32), np.hstack(env)


def ov_inputs(mesh, kname, lat='triclinic'):
    a = LATTICES[lat]
    coords = OV_FRAC.dot(a)
    atm, bas, env = make_tables(coords, OV_SHELLS)
    proj_tab = np.array([p[:3] for p in OV_PROJ], dtype=np.int32)
    proj_rl = np.array([p[3] for p in OV_PROJ])
    return atm, bas, env, coords, np.array(OV_KPTS[kname]), proj_tab, proj_rl, np.array(mesh, dtype=np.int32), a


def ov_rows():
    """First row of each projector in the output, and the row count."""
    r0, n = [], 0
    for _, l, _, _ in OV_PROJ:
        r0.append(n)
        n += 2 * l + 1
    return r0, n


def overlaps_oracle(atm, bas, env, coords, kpt, proj_tab, proj_rl, mesh, a):
    """The SPG / ft_ao contraction of oracle.pp.get_pp (float64), one block of 2l+1 rows per entry of proj_tab."""
    Gv = otools.get_Gv(2 * np.pi * np.linalg.inv(a.T), mesh)
    SI = np.exp(-1j * np.dot(coords, Gv.T))
    Gk = Gv + kpt
    Gr = np.linalg.norm(Gk, axis=1)
    aokG = opp.ft_ao(atm, bas, env, Gk) * (1. / abs(np.linalg.det(a))) ** .5
    rows = []
    for (ia, l, i), rl in zip(proj_tab, proj_rl):
        S = np.array(opp.solid_harmonics(l, Gk))
        pY = rl ** (l + 1.5) * np.pi ** 1.25 * np.exp(-.5 * rl ** 2 * Gr ** 2) * S * opp.qli(Gr * rl, l, i)
        rows.append(np.einsum('g,mg,gp->mp', SI[ia].conj(), pY, aokG))
    return np.vstack(rows)


def ov_oracle(mesh, kname, lat='triclinic'):
    return overlaps_oracle(*ov_inputs(mesh, kname, lat))


def ov_ld(mesh, kname, lat='triclinic'):
    _, bas, env, coords, kpt, proj_tab, proj_rl, m, a = ov_inputs(mesh, kname, lat)
    return ref.overlaps_ld(bas, env, coords, kpt, proj_tab, proj_rl, m, a)


def symmetry_zero_entries():
    """(row, ao) pairs of the overlap matrix that vanish at k = 0 on an orthorhombic lattice when the summand has died out before
    the unpaired -n/2 frequency of the even axes: an l = 1 or l = 2 projector against an s function on the same atom leaves
    sum_G f(|G|) S_lm(G), and S_lm is odd under a reflection of one axis for the three p rows and for xy, yz, xz (rows 0, 1, 3 of
    a d block).  z^2 and x^2-y^2 are even under all three reflections and vanish only on a cubic lattice with a cubic mesh."""
    r0, _ = ov_rows()
    out = []
    for (ia, l, _, _), row in zip(OV_PROJ, r0):
        for m in ([0, 1, 2] if l == 1 else [0, 1, 3] if l == 2 else []):
            out += [(row + m, p) for p in OV_S_OF_ATOM[ia]]
    return out


# ---- end to end ----------------------------------------------------------------------------------------------------------
def e2e_cell():
    """Two atoms, triclinic, mesh (12, 11, 10), s/p/d shells; the pseudopotentials are the fixture's Ge-q4 and Y-q3 entries
    (three s, two p, one and two d projectors), written over cell._pseudo after build()."""
    from pyscf_isdf_amd import gto
    basis = {'C': [[0, [1.1, 0.6, 0.2], [0.4, 0.5, 0.7]], [1, [0.9, 1.0]], [2, [0.8, 1.0]]],
             'O': [[0, [1.4, 1.0]], [1, [1.2, 0.5], [0.5, 0.6]], [2, [1.0, 1.0]]]}
    cell = gto.Cell(unit='B', atom='C 0.7 1.1 0.4; O 2.9 2.2 3.1', basis=basis, pseudo='gth-pade',
                    a=np.array([[5.2, 0.3, 0.1], [0.4, 4.9, -0.2], [0.2, 0.5, 5.5]]), mesh=[12, 11, 10])
    cell._pseudo = {'C': fixture_entry('Ge'), 'O': fixture_entry('Y')}
    return cell


E2E_KPT = np.array([0.21, -0.13, 0.34])


def e2e_reference_inputs(cell):
    from pyscf_isdf_amd import gto
    coords = cell.get_uniform_grids()
    rcut = gto.estimate_rcut_per_shell(cell)
    Ls = gto.get_lattice_Ls(cell, rcut=rcut.max())
    from oracle import ao as oao
    kpts = np.array([np.zeros(3), E2E_KPT])
    aos = oao.eval_ao(cell._atm, cell._bas, cell._env, coords, Ls, rcut, kpts=kpts, rule='point')
    ps = [cell._pseudo.get(cell.atom_symbol(i)) for i in range(cell.natm)]
    return coords, kpts, [np.asarray(x, dtype=complex) for x in aos], ps


def e2e_oracle(cell):
    coords, kpts, aos, ps = e2e_reference_inputs(cell)
    return opp.get_pp(cell._atm, cell._bas, cell._env, cell.atom_coords(), cell.atom_charges(), ps, cell.lattice_vectors(),
                      cell.mesh, coords, aos, kpts)


def e2e_ld(cell):
    """get_pp in longdouble from the restated vlocR and overlaps; the AO values on the grid are the oracle's, taken as data."""
    LD, CLD = ref.LD, ref.CLD
    coords, kpts, aos, ps = e2e_reference_inputs(cell)
    a, mesh = cell.lattice_vectors(), np.asarray(cell.mesh)
    pp_par = np.zeros((cell.natm, 8))
    proj_tab, proj_rl, blocks, row = [], [], [], 0
    for ia, pp in enumerate(ps):
        pp_par[ia, :4] = 1, cell.atom_charges()[ia], pp[1], pp[2]
        pp_par[ia, 4:4 + pp[2]] = pp[3]
        for l, (rl, nl, hl) in enumerate(pp[5:]):
            if nl:
                blocks.append((row, l, nl, np.asarray(hl, dtype=LD)))
                proj_tab += [(ia, l, i) for i in range(nl)]
                proj_rl += [rl] * nl
                row += nl * (2 * l + 1)
    vlocR = ref.vlocR_ld(cell.atom_coords(), pp_par, mesh, a)
    vol = ref.gvec_ld(mesh, a)[1]
    out = []
    for k, ao in zip(kpts, aos):
        ao = ao.astype(CLD)
        v = ref._matmul_c(ao.conj().T, vlocR[:, None] * ao)
        S = ref.overlaps_ld(cell._bas, cell._env, cell.atom_coords(), k, proj_tab, proj_rl, mesh, a)
        for row0, l, nl, hl in blocks:
            blk = S[row0:row0 + nl * (2 * l + 1)].reshape(nl, 2 * l + 1, -1)
            v = v + np.einsum('imp,ij,jmq->pq', blk.conj(), hl, blk) / LD(vol)
        out.append(v)
    return out


def cached(fn, *key):
    return ref.cached(fn, *key)
