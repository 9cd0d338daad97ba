"""Multigrid J, XC potential and XC linear response on MI355X, paired with the ISDF exchange.

Role of ``pyscf.pbc.dft.multigrid`` (multigrid.py:500-529 get_j_kpts, :531-678 _eval_rhoG, :838-935 _get_j_pass2, :1046-1150
nr_rks, :1556-1570 get_rho, :1853-1902 MultiGridFFTDF): the density of a Gaussian basis does not need the dense FFT mesh
everywhere - only products that involve a sharp primitive do.  Primitives are sorted into levels by the kinetic-energy cutoff
their own density needs; level t owns the products (h, h') and (h, l) of its primitives h with each other and with all
smoother ones l, collocates them on a mesh just fine enough for h, and adds the level's spectrum into the dense mesh's
spectrum at the matching frequencies.  The potential goes the other way: its spectrum is cut back to each level's mesh and
integrated there against the same pairs.  The result is the FFTDF J (to the cell precision) at a fraction of the
collocation / contraction work.

What differs from the reference, by design for the GPU:
  * the level ladder is planned, not grown: the primitives' cutoffs cluster into a handful of values, and the ladder is the
    split of that sequence into levels (meshes with factors 2, 3, 5, 7) that minimises a cost model of the two passes
    (multi_grids_tasks).  The reference grows windows by a fixed ratio 1.3 from a 12^3 mesh: a dozen thin levels, each a
    collocation, a GEMM and a batched FFT - launch-bound on a GPU - while a coarse fixed ratio saves nothing when the sharp
    primitives sit close together;
  * a level is (dense rows | sparse rows) of ONE collocation buffer; the pair density is the rectangular contraction
    rho = sum_h aoH_h (D_ht aoT)_h (rocBLAS dgemm + one reduction pass, isdf_rho_pair) and the potential integral is the FP64
    MFMA NT kernel with the potential as its per-k scale (isdf_gemm_nt) - no primitive-pair loops;
  * contracted functions are split by primitives, as in the reference, and contractions without any primitive in a level's
    window are dropped from that level (general contractions such as GTH-DZVP's second function would otherwise be
    collocated as zero rows on every sharp level);
  * half spectra (D2Z / Z2D) throughout.
Everything numerical runs in libmi355_isdf.so (multigrid.hip, eval_ao.hip, gemm_f64.hip); this file plans the levels and
scatters the small level matrices into J on the host.

Surface: MultiGridFFTDF (get_jk, get_j_kpts, get_rho, tasks), nr_rks, nr_uks, hybrid_coeff, rsh_and_hybrid_coeff, hybrid_k,
nr_rks_fxc, nr_rks_fxc_st, nr_uks_fxc, cache_xc_kernel1, _gen_rhf_response, _gen_uhf_response, multi_grids_tasks,
multigrid_fftdf - the names of pyscf/pbc/dft/multigrid/__init__.py and multigrid.py - and the XC nuclear forces get_vxc_e1,
xc_nuc_grad, xc_nuc_grad_uks (xc_grad.py).

K is the ISDF exchange of the parent class (``MultiGridFFTDF(ISDF)``): hybrid functionals get J/XC from here and K from the
interpolation, which is the pairing SURVEY section 8 f-3 names.  XC: the Slater exchange ('lda,') and Becke's 1988 exchange
('b88,', a GGA; Gamma point and k-points) in closed form - libxc is not part of this tree; both are pinned by the reference's SCF energies.
LYP correlation completes them to BLYP and to the semilocal part of the B3LYP family (_XC_TABLE; one fused launch per density,
isdf_xc_fused; open shell: isdf_gga_lyp_polarised), pinned by the reference's BLYP constants; hybrid_coeff tells the caller how much
of the ISDF K to add.  CAM-B3LYP adds the short-range B88 exchange (the ITYH attenuation; isdf_xc_fused_rsh, closed shell), pinned by
the reference's CAM-B3LYP energies; hybrid_k combines the ISDF K with the long-range K of ISDF.get_jk(omega=...) for it.
k-points: the same two passes on the periodic parts u_k, real and imaginary planes stacked so that the complex
contractions are the Gamma point's real rectangular ones (get_j_kpts, nr_rks with kpts).
"""
import copy
import numpy as np
import torch
from . import gto
from .isdf import ISDF
from ._common import TaggedArray

MIN_LEVEL_MESH = 12     # no level mesh below this per dimension (the reference's smallest task mesh, multigrid.py:57)
ANG_OF, NPRIM_OF, NCTR_OF, PTR_EXP, PTR_COEFF = 1, 2, 3, 5, 6


def _estimate_ke_cutoff(alpha, l, c, precision):
    """Cutoff above which the density of a primitive contributes less than ``precision`` (cell.py:436-448, omega = 0)."""
    norm_ang = (2 * l + 1) / (4 * np.pi)
    fac = 32 * np.pi ** 2 * (2 * np.pi) ** 1.5 * c ** 2 * norm_ang / (2 * alpha) ** (2 * l + .5) / precision
    ecut = 20.
    ecut = np.log(fac * (ecut * 2) ** (l - .5) + 1.) * 4 * alpha
    ecut = np.log(fac * (ecut * 2) ** (l - .5) + 1.) * 4 * alpha
    return ecut


def primitive_ke_cutoff(cell, precision=None):
    """Per shell, the cutoff of every primitive (multigrid.py:1825-1850: the cell precision per unit volume)."""
    if precision is None:
        precision = cell.precision
    precision = precision / max(cell.vol, 1)
    out = []
    for ib in range(cell.nbas):
        cs = abs(cell._libcint_ctr_coeff(ib)).max(axis=1)
        out.append(_estimate_ke_cutoff(cell.bas_exp(ib), cell.bas_angular(ib), cs, precision))
    return out


def _plane_spacing_recip(a):
    # component of b_i orthogonal to the other two reciprocal vectors = 2 pi / |a_i| ... along a_i, whose planes are h_i apart
    return 2 * np.pi / np.linalg.norm(np.asarray(a, dtype=float), axis=1)


def cutoff_to_mesh(a, ke):
    """Smallest odd mesh whose frequencies reach |G|^2 / 2 = ke along every reciprocal axis (pbc.py:703-727)."""
    return (np.ceil(np.sqrt(2 * ke) / _plane_spacing_recip(a)).astype(int) * 2 + 1)


def mesh_to_cutoff(a, mesh):
    """Kinetic energy of the highest frequency a mesh carries along each axis (pbc.py:729-742)."""
    return ((np.asarray(mesh) - 1) // 2 * _plane_spacing_recip(a)) ** 2 / 2


def _fft_friendly(n):
    n = int(n)
    while True:
        m = n
        for p in (2, 3, 5, 7):
            while m % p == 0:
                m //= p
        if m == 1:
            return n
        n += 1


class Level:
    """One mesh of the ladder: shells (dense rows first, then sparse rows) of a collocation cell and their places in J."""

    def __init__(self, mesh, ke_window, bas, env, nbas_h, nH, idx_h, idx_l, Ls, rcut):
        self.mesh = np.asarray(mesh, dtype=np.int32)
        self.ke_window = ke_window
        self.bas, self.env = bas, env
        self.nbas_h = int(nbas_h)        # bas[:nbas_h] are the dense shells, the rest the sparse ones (each part atom by atom)
        self.nH = int(nH)
        self.idx_h = np.asarray(idx_h, dtype=np.int64)
        self.idx_l = np.asarray(idx_l, dtype=np.int64)
        self.Ls, self.rcut = Ls, rcut

    @property
    def nT(self):
        return self.nH + len(self.idx_l)

    @property
    def ngrids(self):
        return int(np.prod(self.mesh))

    def __repr__(self):
        return 'Level(mesh=%s, window=(%.3g, %.3g], dense=%d, sparse=%d)' % (
            tuple(int(x) for x in self.mesh), self.ke_window[0], self.ke_window[1], self.nH, len(self.idx_l))


def _split_shells(cell, ke_prim, select):
    """Rows of a collocation cell holding, per shell, the primitives ``select(ke)`` keeps and the contractions that still have a
    coefficient among them.  Returns (bas rows, env blocks, AO indices of the kept functions in the full cell)."""
    ao_loc = cell.ao_loc_nr()
    rows, blocks, idx = [], [], []
    for ib in range(cell.nbas):
        keep = np.where(select(ke_prim[ib]))[0]
        if len(keep) == 0:
            continue
        l = cell.bas_angular(ib)
        cs = cell._libcint_ctr_coeff(ib)[keep]                      # (kept primitives, contractions)
        ctr = np.where(abs(cs).max(axis=0) > 0)[0]
        if len(ctr) == 0:
            continue
        rows.append((cell.bas_atom(ib), l, len(keep), len(ctr)))
        blocks.append((cell.bas_exp(ib)[keep], cs[:, ctr].T.ravel()))
        for c in ctr:
            idx.extend(range(ao_loc[ib] + c * (2 * l + 1), ao_loc[ib] + (c + 1) * (2 * l + 1)))
    return rows, blocks, idx


def _collocation_cell(cell, parts):
    """A cell object whose shells are the concatenation of ``parts`` (lists from _split_shells), for the collocation kernel and
    the cutoff estimates: same atoms and lattice, new _bas / _env."""
    env = [np.asarray(cell._env, dtype=np.float64)]
    ptr = len(cell._env)
    bas = []
    for rows, blocks in parts:
        for (ia, l, nprim, nctr), (es, cs) in zip(rows, blocks):
            bas.append([ia, l, nprim, nctr, 0, ptr, ptr + nprim, 0])
            env += [es, cs]
            ptr += nprim + nprim * nctr
    sub = copy.copy(cell)
    sub._bas = np.asarray(bas, dtype=np.int32).reshape(-1, 8)
    sub._env = np.hstack(env)
    sub._rcut = gto.estimate_rcut(sub, cell.precision)
    return sub


LEVEL_TOLL = 2e-4       # seconds a level costs before it does any work (launches, FFT plans' fixed part, host scatter)


def _level_cost(ngrids, nH, nT, toll=LEVEL_TOLL):
    """Seconds one level costs, both passes: the two rectangular contractions (4 nH nT flop per point at ~60 TF/s), two
    collocations of nT functions (~1.6e11 function values per second, eval_ao.hip at configs[2]) and a fixed launch / FFT toll."""
    return ngrids * (4.0 * nH * nT / 6e13 + 2.0 * nT / 1.6e11) + toll


def multi_grids_tasks(cell, fft_mesh=None, max_levels=None, level_toll=LEVEL_TOLL, split='cost', verbose=None):
    """The level ladder of ``cell`` under the dense mesh ``fft_mesh`` (role of multigrid.py:1572-1822).

    The primitives' cutoffs fall into a few clusters (one per exponent, near enough).  A level is a run of neighbouring
    clusters on the mesh its sharpest member needs (rounded up to factors 2, 3, 5, 7, floored at MIN_LEVEL_MESH, capped by the
    dense mesh); the ladder is the split of the cluster sequence into runs that minimises the modelled time (_level_cost) -
    a shortest-path problem over at most a few dozen clusters, solved exactly.  The reference grows windows by a fixed
    ratio from a fixed start mesh; a fixed ratio either lumps GTH-DZVP's two sharpest primitives with the rest (ratio 3: no
    saving at configs[2]) or makes a dozen launch-bound levels (ratio 1.3).  Clusters whose mesh reaches the dense mesh in
    every dimension share the top level, as in the reference (a user-chosen dense mesh may be coarser than the sharpest
    primitive asks for - the FFTDF answer on that mesh is what has to be reproduced)."""
    a = np.asarray(cell.lattice_vectors(), dtype=float)
    fft_mesh = np.asarray(cell.mesh if fft_mesh is None else fft_mesh, dtype=int)
    ke_prim = primitive_ke_cutoff(cell)
    ao_loc = cell.ao_loc_nr()
    # clusters of cutoffs (1 % apart or less), ascending
    kes = np.sort(np.concatenate(ke_prim))
    tops = [kes[0]]
    for k in kes[1:]:
        if k > tops[-1] * 1.01:
            tops.append(k)
        else:
            tops[-1] = k
    tops = np.asarray(tops)

    def mesh_of(ke):
        m = np.array([_fft_friendly(max(x, MIN_LEVEL_MESH)) for x in cutoff_to_mesh(a, ke)])
        return np.minimum(m, fft_mesh)
    meshes = [mesh_of(k) for k in tops]
    while len(tops) > 1 and (meshes[-2] >= fft_mesh).all():      # everything that needs the dense mesh anyway: one cluster
        tops, meshes = tops[:-1], meshes[:-1]
    tops[-1] = np.inf
    meshes[-1] = fft_mesh
    m = len(tops)
    # functions (contractions x m_l) with a primitive in cluster c: count per cluster range through prefix tables
    nfun_upto = np.zeros((m + 1,), dtype=int)                     # functions with any primitive in clusters < c
    has = []                                                      # per shell contraction: boolean over clusters
    for ib in range(cell.nbas):
        cs = cell._libcint_ctr_coeff(ib)
        which = np.searchsorted(tops, ke_prim[ib] / 1.0000001)    # cluster of every primitive
        for c in range(cs.shape[1]):
            row = np.zeros(m, dtype=bool)
            row[which[abs(cs[:, c]) > 0]] = True
            has.append((row, 2 * cell.bas_angular(ib) + 1))
    for c in range(m + 1):
        nfun_upto[c] = sum(n for row, n in has if row[:c].any())

    def counts(i, j):                                            # level = clusters i .. j-1
        nH = sum(n for row, n in has if row[i:j].any())
        return nH, nH + nfun_upto[i]
    if split == 'all':
        # one level per distinct mesh, whatever it costs (tests; the planner's answer does not change J beyond the precision)
        runs, j = [], m
        while j > 0:
            i = j - 1
            while i > 0 and (meshes[i - 1] == meshes[j - 1]).all():
                i -= 1
            runs.append((i, j))
            j = i
        return _levels_of_runs(cell, ke_prim, tops, meshes, runs)
    best = [0.0] + [np.inf] * m
    cut = [0] * (m + 1)
    nlev = [0] * (m + 1)
    for j in range(1, m + 1):
        G = float(np.prod(meshes[j - 1]))
        for i in range(j):
            if max_levels is not None and nlev[i] + 1 > max_levels and i > 0:
                continue
            nH, nT = counts(i, j)
            c = best[i] + _level_cost(G, nH, nT, level_toll)
            if c < best[j]:
                best[j], cut[j], nlev[j] = c, i, nlev[i] + 1
    runs, j = [], m
    while j > 0:
        runs.append((cut[j], j))
        j = cut[j]
    return _levels_of_runs(cell, ke_prim, tops, meshes, runs)


def _levels_of_runs(cell, ke_prim, tops, meshes, runs):
    levels = []
    for i, j in runs:                                            # top level first
        ke1 = tops[j - 1]
        ke0 = tops[i - 1] if i > 0 else 0.0
        dense = _split_shells(cell, ke_prim, lambda k: (ke0 * 1.0000001 < k) & (k <= ke1 * 1.0000001))
        sparse = _split_shells(cell, ke_prim, lambda k: k <= ke0 * 1.0000001)
        sub = _collocation_cell(cell, [dense[:2], sparse[:2]])
        rcut = gto.estimate_rcut_per_shell(sub)
        Ls = gto.get_lattice_Ls(sub, rcut=rcut.max())
        levels.append(Level(meshes[j - 1], (ke0, ke1), sub._bas, sub._env, len(dense[0]), len(dense[2]), dense[2], sparse[2], Ls, rcut))
    return levels


def _xc_rows():
    """The functional table: normalised code (upper case, no blanks) -> (c_slater, c_b88, c_vwn, vwn_fit, c_lyp, hyb), the weights of
    Slater exchange, Becke-88 exchange (which contains the Slater term), VWN correlation (fit 'V' = libxc LDA_C_VWN, or 'RPA' =
    LDA_C_VWN_RPA), LYP correlation, and the fraction of exact exchange the caller adds."""
    rows = {}
    for codes, w in (
            (('LDA,', 'SLATER,', 'LDA_X,', 'LDA', 'SLATER', 'LDA_X'), (1.0, 0.0, 0.0, 'V', 0.0, 0.0)),
            (('LDA,VWN', 'LDA,VWN5', 'SLATER,VWN', 'SLATER,VWN5', 'SVWN', 'SVWN5', 'LDA_X,LDA_C_VWN', 'LDA,LDA_C_VWN'),
             (1.0, 0.0, 1.0, 'V', 0.0, 0.0)),
            (('B88,', 'B88', 'GGA_X_B88,', 'GGA_X_B88'), (0.0, 1.0, 0.0, 'V', 0.0, 0.0)),
            (('BLYP', 'B88,LYP', 'GGA_X_B88,GGA_C_LYP'), (0.0, 1.0, 0.0, 'V', 1.0, 0.0)),
            ((',LYP', ',GGA_C_LYP'), (0.0, 0.0, 0.0, 'V', 1.0, 0.0)),
            # libxc.py:737-738 and the 2.3 note there: 'B3LYP' is the VWN-RPA variant (Gaussian's), 'B3LYP5' the fit-V one
            (('B3LYP5', '.2*HF+.08*SLATER+.72*B88,.81*LYP+.19*VWN'), (0.08, 0.72, 0.19, 'V', 0.81, 0.2)),
            (('B3LYP', 'B3LYPG'), (0.08, 0.72, 0.19, 'RPA', 0.81, 0.2))):
        for c in codes:
            rows[c] = w
    # libxc.py:758,1279 (HYB_GGA_XC_CAM_B3LYP): 0.35 B88 + 0.46 short-range B88 + 0.19 VWN fit V + 0.81 LYP; exact exchange
    # 0.19 K + (0.65 - 0.19) K_LR(omega = 0.33).  The fit and the weights are pinned by the reference's energies (tests/test_rsh.py)
    for c in ('CAMB3LYP', 'CAM-B3LYP', 'CAM_B3LYP', 'HYB_GGA_XC_CAM_B3LYP'):
        rows[c] = _RshRow((0.0, 0.35, 0.19, 'V', 0.81, 0.19), c_b88_sr=0.46, omega=0.33, alpha=0.65)
    return rows


class _RshRow(tuple):
    """A row of _XC_TABLE of a range-separated hybrid: the same 6-tuple (hyb: the exact exchange at every range) with the weight of the
    short-range B88 (the ITYH attenuation at ``omega``) and ``alpha``, the exact exchange at long range."""

    def __new__(cls, row, c_b88_sr, omega, alpha):
        self = tuple.__new__(cls, row)
        self.c_b88_sr, self.omega, self.alpha = float(c_b88_sr), float(omega), float(alpha)
        return self

    def with_omega(self, omega):
        if not omega > 0:
            raise ValueError('omega = %r: the range-separation parameter is positive' % (omega,))
        return _RshRow(tuple(self), self.c_b88_sr, omega, self.alpha)


_XC_TABLE = _xc_rows()


def _functional(xc_code):
    """(c_slater, c_b88, c_vwn, vwn_fit, c_lyp, hyb) of ``xc_code``: a code of _XC_TABLE, or such a tuple itself (raw weights: always
    the fused kernel).  Everything else raises NotImplementedError - libxc is not part of this tree."""
    if isinstance(xc_code, (tuple, list)):
        cs, cb, cv, fit, cl, hyb = xc_code
        if fit not in ('V', 'RPA'):
            raise ValueError("vwn_fit is 'V' or 'RPA'")
        return float(cs), float(cb), float(cv), fit, float(cl), float(hyb)
    w = _XC_TABLE.get(str(xc_code).replace(' ', '').upper())
    if w is None:
        raise NotImplementedError("xc=%r: 'lda,' (Slater exchange), 'lda,vwn' (+ VWN5 correlation), 'b88,' (Becke-88 exchange), 'blyp' / "
                                  "'b88,lyp', ',lyp', 'b3lyp5', 'b3lyp' / 'b3lypg' and 'camb3lyp' are implemented (no libxc in this tree)"
                                  % (xc_code,))
    return w


def _functional_at(xc_code, omega):
    """_functional with the caller's ``omega`` in place of the functional's own (the reference's mf.omega); None keeps it.  An omega
    for a functional without range separation is a ValueError."""
    fn = _functional(xc_code)
    if omega is None:
        return fn
    if not isinstance(fn, _RshRow):
        raise ValueError('omega = %r: xc=%r is not range-separated' % (omega, xc_code))
    return fn.with_omega(float(omega))


def hybrid_coeff(xc_code):
    """Fraction of exact exchange of ``xc_code``: 0.2 for the B3LYP family, 0.19 for CAM-B3LYP (at every range; rsh_and_hybrid_coeff
    has the long-range part), 0.0 for the other implemented functionals.  nr_rks returns the semilocal part only, as the reference's
    does; the caller adds -1/2 hybrid_k (closed shell)."""
    return _functional(xc_code)[5]


def rsh_and_hybrid_coeff(xc_code):
    """(omega, alpha, hyb) as numint.rsh_and_hybrid_coeff (numint.py:2708-2727): exact exchange hyb K + (alpha - hyb) K_LR(omega).
    CAM-B3LYP: (0.33, 0.65, 0.19); every other code (0, 0, hybrid_coeff)."""
    fn = _functional(xc_code)
    if isinstance(fn, _RshRow):
        return fn.omega, fn.alpha, fn[5]
    return 0.0, 0.0, fn[5]


def hybrid_k(mydf, xc_code, dm, omega=None, exxdiv='ewald'):
    """The exchange matrix a hybrid Fock build subtracts half of (closed shell): hyb K + (alpha - hyb) K_LR(omega) of
    pbc/dft/rks.py:108-113, K from mydf.get_jk(exxdiv=exxdiv) and K_LR from mydf.get_jk(omega=omega) - the ISDF exchange with the
    plain and the attenuated kernel.  With exxdiv='ewald' the long-range part carries the probe-charge correction of its own
    interaction, madelung(cell, omega=omega) S D S (pbc.py:495-511), S = mydf.overlap().  ``omega`` None: the functional's own.  A
    global hybrid gives hyb K, a functional without exact exchange zeros.  Gamma point, one process."""
    fn = _functional_at(xc_code, omega)
    mydf._ppg_refuse(None, 'hybrid_k')
    hyb = fn[5]
    dm_in = np.asarray(dm)
    vk = np.zeros(dm_in.shape)
    if hyb != 0:
        vk = vk + hyb * mydf.get_jk(dm, with_j=False, exxdiv=exxdiv)[1]
    if isinstance(fn, _RshRow) and fn.alpha != hyb:
        klr = mydf.get_jk(dm, with_j=False, omega=fn.omega, exxdiv='None')[1]
        if exxdiv == 'ewald':
            S = mydf.backend.to_host(mydf.overlap())
            klr = klr + gto.madelung(mydf.cell, omega=fn.omega) * np.einsum('ij,...jk,kl->...il', S, dm_in.real, S)
        vk = vk + (fn.alpha - hyb) * klr
    return vk


class _Planes:
    """Row layout of one level's collocation buffer, and the two maps between matrices and that layout.

    k-points: the buffer holds the periodic parts u_k (the Bloch phases cancel in the density and in the potential matrix) as
    rows (Re dense | Im dense | Re sparse | Im sparse), so that the first 2 nH rows are the dense functions' real and
    imaginary planes and the whole buffer is the level's function set - the complex contractions then ARE real rectangular
    ones on stacked planes.  Gamma point: the same with the imaginary planes absent, rows (dense | sparse)."""

    def __init__(self, lv, cplx):
        nH, nL = lv.nH, lv.nT - lv.nH
        self.nH = nH
        self.n = 2 if cplx else 1                                   # planes per function
        self.rows = self.n * lv.nT
        self.dense = slice(0, self.n * nH)                          # the dense functions' planes lead the buffer
        # (dense rows, sparse rows) of the real planes and of the imaginary ones
        self.re = (slice(0, nH), slice(self.n * nH, self.n * nH + nL))
        self.im = (slice(nH, 2 * nH), slice(2 * nH + nL, 2 * (nH + nL))) if cplx else None

    def stack(self, D):
        """The real matrix M with rho_t = A (M B), A = the dense planes, B = the buffer, for the Hermitian block D (nset, nH, nT):
        rho_t = Re sum_h u_h sum_t D'_ht conj(u_t) with D' = [D_hh | 2 D_hl] ((l, h) pairs ride with (h, l): their products are
        the conjugates), M = [[Re D', Im D'], [-Im D', Re D']] in the buffer's row order; M = D' without imaginary planes."""
        nH = self.nH
        D = D.copy()
        D[:, :, nH:] *= 2.0
        if self.im is None:
            return np.ascontiguousarray(D)
        M = np.empty((D.shape[0], 2 * nH, self.rows))
        for rows, (P, Q) in ((self.re[0], (D.real, D.imag)), (self.im[0], (-D.imag, D.real))):   # rows Re u_h: [p, q]; rows Im u_h: [-q, p]
            M[:, rows, self.re[0]] = P[:, :, :nH]
            M[:, rows, self.im[0]] = Q[:, :, :nH]
            M[:, rows, self.re[1]] = P[:, :, nH:]
            M[:, rows, self.im[1]] = Q[:, :, nH:]
        return M

    def unstack(self, R):
        """V (nH, nT) = conj(u_h) v u_t from the product R of the dense planes with all planes (host array)."""
        if self.im is None:
            return R
        nH = self.nH
        cre, cim = np.r_[self.re], np.r_[self.im]
        # conj(a + ib) v (c + id) = (a v c + b v d) + i (a v d - b v c)
        return (R[:nH][:, cre] + R[nH:][:, cim]) + 1j * (R[:nH][:, cim] - R[nH:][:, cre])


class MultiGridFFTDF(ISDF):
    """FFTDF-shaped object: J (and the XC potential) through the level ladder, K through ISDF.

    ``build()`` plans the levels; the ISDF fit is built the first time K is asked for.  ``tasks`` is the ladder
    (list of Level), as in the reference's attribute of that name."""

    def __init__(self, cell, kpts=np.zeros((1, 3)), **kwargs):
        ISDF.__init__(self, cell, kpts, **kwargs)
        self.tasks = None
        self.max_levels = None            # cap on the number of levels (None: whatever the cost model picks)
        self.level_toll = LEVEL_TOLL      # fixed cost of a level in the planner's model, seconds
        self.split = 'cost'               # 'cost': the cost model decides; 'all': one level per distinct mesh (tests)
        self.ao_cache_fraction = 0.25     # level collocations are kept between the two passes while they fit this share of free HBM
        self._level_cache = {}            # (level, components) -> Gamma-point collocation
        self._k_requested = False

    # ---- planning ----------------------------------------------------------------------------
    def build_tasks(self):
        if self.tasks is None:
            self.tasks = multi_grids_tasks(self.cell, self.mesh, self.max_levels, self.level_toll, self.split)
            self._level_cache = {}
        return self.tasks

    def build(self):
        self.build_tasks()
        if self._k_requested:
            # the ISDF build sizes its fit buffers against the free HBM: hand the level collocations back first (they are
            # re-made on demand and kept again only while they fit next to the fit)
            self._level_cache = {}
            self.backend.empty_cache()
            ISDF.build(self)
        return self

    def reset(self, cell=None):
        self.tasks = None
        self._level_cache = {}
        return ISDF.reset(self, cell)

    # ---- level collocation -------------------------------------------------------------------
    def _level_ao(self, it, kpt, ncomp, keep):
        """(ncomp, rows, G_t padded) collocation of level ``it`` on its own mesh, rows as _Planes lays them out: the functions
        (ncomp = 1) or the functions and their x, y, z derivatives (ncomp = 4; the reference's RHOG_HIGH_ORDER branch), at the
        Gamma point (``kpt`` None, real) or the periodic parts at ``kpt``.  Gamma-point sets are kept for the next pass if ``keep``."""
        if kpt is None:
            hit = self._level_cache.get((it, ncomp))
            if hit is not None:
                return hit
        lv, be, cell = self.tasks[it], self.backend, self.cell
        pl = _Planes(lv, kpt is not None)
        # rows padded with zeros to a multiple of 32 grid points: the potential integral then runs on the aligned MFMA kernel
        # (90^3 and 70^3 are not multiples of 32; the unaligned variant is a third slower)
        buf = be.zeros((ncomp, pl.rows, -(-lv.ngrids // 32) * 32))
        coords_soa = be.uniform_grid(lv.mesh, cell.lattice_vectors())
        atm = np.asarray(cell._atm)
        out = buf[0] if ncomp == 1 else buf            # the plain kernels fill (rows, G) planes, the deriv1 ones (4, rows, G)
        # two launches: the collocation kernel walks one atom's shells per workgroup and wants them contiguous in bas
        nb = lv.nbas_h
        parts = [(0, lv.bas[:nb], lv.rcut[:nb])]
        if lv.nT > lv.nH:
            parts.append((1, lv.bas[nb:], lv.rcut[nb:]))
        for part, bas, rcut in parts:                  # dense shells, sparse shells
            if kpt is None:
                (be.eval_ao if ncomp == 1 else be.eval_ao_deriv1)(atm, bas, lv.env, lv.Ls, rcut, coords_soa, out[..., pl.re[part], :])
            else:
                (be.eval_ao_k if ncomp == 1 else be.eval_ao_k_deriv1)(atm, bas, lv.env, lv.Ls, rcut, kpt, True, coords_soa,
                                                                     out[..., pl.re[part], :], out[..., pl.im[part], :])
        if keep:
            self._level_cache[(it, ncomp)] = buf
        return buf

    def _cache_plan(self, kpts, ncomp):
        """Whether this pass keeps its collocations for the next one: Gamma-point sets only (k-point sets are made per k-point
        and used once), while the ladder's ``ncomp``-component set fits the allowed share of the free memory or sets of that
        kind are resident already."""
        if kpts is not None:
            return False
        need = sum(8 * ncomp * lv.nT * lv.ngrids for lv in self.tasks)
        return need <= self.ao_cache_fraction * self.backend.free_bytes() or any(nc == ncomp for _, nc in self._level_cache)

    # ---- the two passes ----------------------------------------------------------------------
    def _spectrum_size(self):
        m = [int(x) for x in self.mesh]
        return m[0] * m[1] * (m[2] // 2 + 1)

    def _eval_rhoG(self, dms, kpts=None, ncomp=1):
        """Half spectra (ncomp, nset, gc) on the dense mesh, integral-normalised (rho(G) = int rho e^{-iGr}) as the reference's
        _eval_rhoG, of rho = 1/nk sum_k sum_ij D^k_ij u^k_i conj(u^k_j) and, with ncomp = 4, of d rho / dx, dy, dz, for HERMITIAN
        ``dms`` (nset, nk, nao, nao); ``kpts`` None: the Gamma point, nk = 1 and ``dms`` real symmetric.  The gradient of a level's
        density is taken in real space, d_c rho_t = sum_h (d_c phi_h) (D' phi_T)_h + phi_h (D' d_c phi_T)_h - two rectangular
        contractions per component."""
        be, cell = self.backend, self.cell
        self.build_tasks()
        nset, nk = dms.shape[:2]
        mesh = np.asarray(self.mesh, dtype=np.int32)
        spec = be.zeros((ncomp, nset, self._spectrum_size()), dtype=torch.complex128)
        keep = self._cache_plan(kpts, ncomp)
        for it, lv in enumerate(self.tasks):
            pl = _Planes(lv, kpts is not None)
            idx_t = np.append(lv.idx_h, lv.idx_l)
            rho = be.empty((nset, lv.ngrids))
            w = cell.vol / lv.ngrids / nk
            for k, kpt in enumerate([None] if kpts is None else kpts):
                ao = self._level_ao(it, kpt, ncomp, keep)
                d_M = be.to_device(pl.stack(dms[:, k][:, lv.idx_h[:, None], idx_t]))      # from D (nset, nH, nT)
                be.rho_pair(ao[0, pl.dense], ao[0], lv.ngrids, d_M, rho)
                be.mg_embed_density(rho, lv.mesh, w, spec[0], mesh, accumulate=True)
                for c in range(1, ncomp):
                    be.rho_pair(ao[c, pl.dense], ao[0], lv.ngrids, d_M, rho)
                    be.mg_embed_density(rho, lv.mesh, w, spec[c], mesh, accumulate=True)
                    be.rho_pair(ao[0, pl.dense], ao[c], lv.ngrids, d_M, rho)
                    be.mg_embed_density(rho, lv.mesh, w, spec[c], mesh, accumulate=True)
                del ao
        return spec

    def _integrate(self, wspec, kpts_band=None):
        """(nset, nband, nao, nao) matrices sum_r conj(u_i) [v0 u_j + v_c d_c u_j] + conj(d_c u_i) v_c u_j of the real potentials
        given by their half spectra ``wspec`` (ncomp, nset, gc) on the dense mesh (role of _get_j_pass2 and, with ncomp = 4, of
        _get_gga_pass2, multigrid.py:936-1043): one MFMA product per level and k-point, or seven, with the potentials as per-k
        scales, on the stacked planes and combined once.  ``kpts_band`` None: the Gamma point, nband = 1 and a real result."""
        be, cell = self.backend, self.cell
        nao = cell.nao_nr()
        ncomp, nset = wspec.shape[:2]
        mesh = np.asarray(self.mesh, dtype=np.int32)
        band = [None] if kpts_band is None else kpts_band
        out = np.zeros((nset, len(band), nao, nao), dtype=np.float64 if kpts_band is None else np.complex128)
        keep = self._cache_plan(kpts_band, ncomp)
        for it, lv in enumerate(self.tasks):
            pl = _Planes(lv, kpts_band is not None)
            nH = lv.nH
            v = be.empty((ncomp, nset, lv.ngrids))
            for c in range(ncomp):
                be.mg_restrict_potential(wspec[c], mesh, lv.mesh, 1.0 / lv.ngrids, v[c])
            for ib, kb in enumerate(band):
                ao = self._level_ao(it, kb, ncomp, keep)
                R = be.empty((pl.n * nH, pl.rows))
                vpad = be.zeros((ao.shape[2],))
                for i in range(nset):
                    vpad[:lv.ngrids].copy_(v[0, i])
                    be.gemm_nt(ao[0, pl.dense], ao[0], R, kscale=vpad)
                    for c in range(1, ncomp):
                        vpad[:lv.ngrids].copy_(v[c, i])
                        be.gemm_nt(ao[0, pl.dense], ao[c], R, beta=1.0, kscale=vpad)
                        be.gemm_nt(ao[c, pl.dense], ao[0], R, beta=1.0, kscale=vpad)
                    V = pl.unstack(be.to_host(R))
                    out[i, ib][lv.idx_h[:, None], lv.idx_h] += V[:, :nH]
                    if len(lv.idx_l):
                        out[i, ib][lv.idx_h[:, None], lv.idx_l] += V[:, nH:]
                        out[i, ib][lv.idx_l[:, None], lv.idx_h] += V[:, nH:].conj().T
                del ao, R, vpad
            del v
        return out

    # ---- matrices in, matrices out -----------------------------------------------------------
    def _real_dms(self, dm):
        dm_in = np.asarray(dm)
        nao = self.cell.nao_nr()
        if np.iscomplexobj(dm_in) and abs(dm_in.imag).max() > 1e-12:
            raise NotImplementedError('multigrid J at the Gamma point takes real density matrices')
        return dm_in.shape, np.ascontiguousarray(dm_in.real.reshape(-1, nao, nao), dtype=np.float64)

    def _format_dms(self, dm, kpts, kpts_band=None):
        """(dms (nset, nk, nao, nao), kpts, band k-points, shape of the result) for the two passes.  ``kpts`` None: the Gamma
        point - real matrices, kpts and band None, the result shaped like ``dm``; else complex matrices, kpts (nk, 3), and the
        result on kpts or on kpts_band, shaped as df_jk._format_jks shapes it (df_jk.py:1426-1444)."""
        if kpts is None:
            shape, dms = self._real_dms(dm)
            return dms[:, None], None, None, shape
        kpts = np.asarray(kpts, dtype=float).reshape(-1, 3)
        nao = self.cell.nao_nr()
        dm_in = np.asarray(dm)
        dms = np.asarray(dm_in, dtype=np.complex128).reshape(-1, len(kpts), nao, nao)
        band_in = None if kpts_band is None else np.asarray(kpts_band, dtype=float)
        band = kpts if band_in is None else band_in.reshape(-1, 3)
        shape = dm_in.shape if band_in is None else (dm_in.shape[:-3] + ((len(band),) if band_in.ndim > 1 else ()) + (nao, nao))
        return dms, kpts, band, shape

    def _hermitian_parts(self, dms, anti=True):
        """D = H + i A with H, A Hermitian: the density of D is rho(H) + i rho(A), both real (fft_jk.py:63-72 builds a complex
        density for hermi = 0; J is linear, so the two real densities go through the ladder one after the other).  Returns
        [(1, H)] and, if ``anti`` and A is there, (i, A).  Real matrices (the Gamma point, real functions): only the symmetric part
        of D reaches the density."""
        H = 0.5 * (dms + dms.conj().transpose(0, 1, 3, 2))
        parts = [(1.0, H)]
        if anti and np.iscomplexobj(dms):
            A = -0.5j * (dms - dms.conj().transpose(0, 1, 3, 2))
            if abs(A).max() > 1e-10:
                parts.append((1j, A))
        return parts

    def _get_j(self, dm, kpts, kpts_band=None):
        dms, kpts, band, shape = self._format_dms(dm, kpts, kpts_band)
        vj = 0.0
        for fac, part in self._hermitian_parts(dms):
            spec = self._eval_rhoG(part, kpts)
            self.backend.mg_coulomb_kernel(spec[0], np.asarray(self.mesh, dtype=np.int32), self.cell.lattice_vectors())
            vj = vj + fac * self._integrate(spec, band)
        return vj.reshape(shape)

    def get_j_kpts(self, dm_kpts, hermi=1, kpts=None, kpts_band=None):
        """k-point J through the level ladder (multigrid.py:500-529); shapes as df_jk._format_jks."""
        return self._get_j(dm_kpts, self.kpts if kpts is None else kpts, kpts_band)

    def get_j(self, dm):
        """J of the Gamma-point density matrix (or stack of them) through the level ladder."""
        return self._get_j(dm, None)

    def get_rho(self, dm, kpts=None):
        """Density on the dense mesh (multigrid.py:1556-1570)."""
        if kpts is not None and not self._is_gamma(kpts):
            raise NotImplementedError('multigrid get_rho is implemented at the Gamma point')
        dms = self._format_dms(dm, None)[0]
        spec = self._eval_rhoG(self._hermitian_parts(dms)[0][1])
        out = self.backend.to_host(_real_space(self, spec, 1.0 / self.cell.vol)[0])
        return out[0] if np.asarray(dm).ndim == 2 else out

    # ---- FFTDF surface -----------------------------------------------------------------------
    def get_jk(self, dm, hermi=1, kpts=None, kpts_band=None, with_j=True, with_k=True, omega=None, exxdiv=None):
        if kpts is None:
            kpts = self.kpts
        gamma = self._is_gamma(kpts) and self._is_gamma(self.kpts) and self._is_gamma(kpts_band)
        if omega is not None and abs(omega) > 0:
            # range separation: the parent's J with the attenuated kernel (dense mesh) and its own W; not a multigrid case
            self._k_requested = True
            return ISDF.get_jk(self, dm, hermi, kpts, kpts_band, with_j, with_k, omega, exxdiv)
        vj = vk = None
        if with_j:
            vj = self.get_j(dm) if gamma else self.get_j_kpts(dm, hermi, kpts, kpts_band)
        if with_k:
            self._k_requested = True      # the fit (Gamma point or k-points) lives in the parent's build
            vk = ISDF.get_jk(self, dm, hermi, kpts, kpts_band, False, True, omega, exxdiv)[1]
        return vj, vk


def get_j_kpts(mydf, dm_kpts, hermi=1, kpts=np.zeros((1, 3)), kpts_band=None):
    """Module-level form of the reference (multigrid.py:500-529)."""
    kpts = np.asarray(kpts, dtype=float).reshape(-1, 3)
    if mydf._is_gamma(kpts) and mydf._is_gamma(kpts_band):
        return mydf.get_jk(dm_kpts, hermi, kpts, kpts_band, with_j=True, with_k=False)[0]
    return mydf.get_j_kpts(dm_kpts, hermi, kpts, kpts_band)


def _real_space(mydf, spec, scale):
    """scale * the real fields (ncomp, nset, G) on the dense mesh of the half spectra ``spec`` (ncomp, nset, gc)."""
    be = mydf.backend
    mesh = np.asarray(mydf.mesh, dtype=np.int32)
    out = be.empty(tuple(spec.shape[:2]) + (int(np.prod(mesh)),))
    for c in range(spec.shape[0]):
        be.mg_restrict_potential(spec[c], mesh, mesh, scale, out[c])
    return out


def _ncomp(kind):
    """Components the ladder carries for a response kind: the density, or (a GGA) the density and its gradient."""
    return 4 if kind == 'b88' else 1


def _kpts_or_gamma(mydf, kpts, kpts_band):
    """None where the Gamma-point layout (real matrices) serves, else the k-points; ``kpts`` None: those of ``mydf``."""
    if kpts is None:
        kpts = mydf.kpts
    return None if mydf._is_gamma(kpts) and mydf._is_gamma(kpts_band) else kpts


def nr_rks(mydf, xc_code, dm_kpts, hermi=1, kpts=None, kpts_band=None, with_j=False, return_j=False, verbose=None, omega=None):
    """XC energy and potential matrix of a closed-shell density through the level ladder (multigrid.py:1046-1150): the functionals
    of _XC_TABLE - Slater exchange (with or without VWN5 correlation), Becke-88 exchange, BLYP, LYP alone and the semilocal part of
    the B3LYP family and of CAM-B3LYP (hybrid_k gives the exact exchange the caller adds); Gamma point (real matrices) or k-points
    (dm (nk, nao, nao) or (nset, nk, nao, nao), complex result on the k-points or on kpts_band).  Returns (nelec, exc, veff) with
    veff tagged ecoul / exc / vj / vk like the reference's; with_j adds the Coulomb potential to veff before the integration pass
    (one pass for J + XC).  ``omega`` replaces the range-separation parameter of a range-separated functional in the attenuation
    of its short-range exchange (the reference's mf.omega); for any other functional it is a ValueError."""
    fn = _functional_at(xc_code, omega)
    return _nr_ks(mydf, fn, isinstance(xc_code, (tuple, list)), dm_kpts, _kpts_or_gamma(mydf, kpts, kpts_band), kpts_band, with_j,
                  return_j, False)


def nr_uks(mydf, xc_code, dm_kpts, hermi=1, kpts=None, kpts_band=None, with_j=False, return_j=False, verbose=None):
    """Open-shell form (multigrid.py:1152-1257): dm = (alpha, beta), each (nao, nao) at the Gamma point or (nk, nao, nao) at
    k-points.  Returns (nelec [both spins together], exc, veff (2, ...)); exchange functionals by spin scaling,
    E_x[rho_a, rho_b] = (E_x[2 rho_a] + E_x[2 rho_b]) / 2, v_a = v_x[2 rho_a]; LYP ('blyp', ',lyp') from the spin-polarised kernel
    on (rho_a, rho_b) together; the Coulomb potential of with_j is that of the total density.  Functionals with VWN correlation
    ('lda,vwn', the B3LYP family) are refused: the spin-polarised VWN is not implemented."""
    fn = _functional(xc_code)
    if fn[2] != 0:
        raise NotImplementedError("xc=%r: the spin-polarised VWN correlation is not implemented (closed-shell nr_rks only)" % (xc_code,))
    kpts = _kpts_or_gamma(mydf, kpts, kpts_band)
    dm_in = np.asarray(dm_kpts)
    if dm_in.shape[0] != 2 or dm_in.ndim != (3 if kpts is None else 4):
        raise ValueError('nr_uks takes one pair (alpha, beta) of density matrices')
    return _nr_ks(mydf, fn, isinstance(xc_code, (tuple, list)), dm_in, kpts, kpts_band, with_j, return_j, True)


def _xc_dispatch(be, fn, raw, spin):
    """Which kernels evaluate the functional ``fn`` (a row of _XC_TABLE; ``raw``: caller's weights) - shared by _nr_ks and the
    nuclear forces of xc_grad: (ncomp, pair_lyp, per_channel, channel).  ncomp: 1 without gradients, 4 with; channel(rho (ncomp, G),
    exc (G,), vxc (ncomp, G)) launches the one kernel of a density - isdf_lda_exchange [+ isdf_lda_vwn_add], isdf_gga_b88 for Becke's
    exchange alone, isdf_xc_fused for every other weighted sum, isdf_xc_fused_rsh for one with a short-range B88 weight; ``spin``: the
    channel is the exchange part alone (at 2 rho_s), pair_lyp says that LYP of (rho_a, rho_b) together follows
    (isdf_gga_lyp_polarised), per_channel that there is a channel part at all.  (No range-separated functional reaches this with
    ``spin``: the only one carries VWN, which nr_uks and xc_nuc_grad_uks refuse first.)"""
    cs, cb, cv, fit, cl, _ = fn
    csr, omega = (fn.c_b88_sr, fn.omega) if isinstance(fn, _RshRow) else (0.0, 0.0)
    ncomp = 4 if (cb != 0 or cl != 0 or csr != 0 or raw) else 1
    pair_lyp = spin and cl != 0                                              # LYP of (rho_a, rho_b) together
    if spin:
        cv, cl = 0.0, 0.0                                                    # per channel: the exchange part alone
    per_channel = not (pair_lyp and cs == 0 and cb == 0)                     # ',lyp' of a pair: nothing but the coupled term

    def channel(rho, exc, vxc):
        if ncomp == 1:
            be.lda_exchange(rho[0], exc, vxc[0])
            if cv != 0:
                be.lda_vwn_add(rho[0], exc, vxc[0])
        elif csr != 0:
            be.xc_fused_rsh(rho[0], rho[1:], (cs, cb, cv, cl), fit == 'RPA', csr, omega, exc, vxc[0], vxc[1:])
        elif (cs, cb, cv, cl) == (0.0, 1.0, 0.0, 0.0) and not raw:
            be.gga_b88(rho[0], rho[1:], exc, vxc[0], vxc[1:])
        else:
            be.xc_fused(rho[0], rho[1:], (cs, cb, cv, cl), fit == 'RPA', exc, vxc[0], vxc[1:])
    return ncomp, pair_lyp, per_channel, channel


def _nr_ks(mydf, fn, raw, dm, kpts, kpts_band, with_j, return_j, spin):
    """The Kohn-Sham pass pair behind nr_rks and nr_uks: rho (and grad rho for a GGA, real-space gradients per level) from the
    ladder, the functional ``fn`` (a row of _XC_TABLE) on the dense mesh, the potential v_rho phi phi + (de/d grad rho) .
    grad(phi phi) back through the ladder.  The functional is one launch per density: isdf_lda_exchange [+ isdf_lda_vwn_add]
    without gradients, isdf_gga_b88 for Becke's exchange alone, isdf_xc_fused for every other weighted sum (and for ``raw``
    weights).  ``kpts`` None: the Gamma point.  ``spin``: dm is the pair (alpha, beta); each spin channel is the closed-shell
    exchange at (2 rho_s, 2 grad rho_s) - potentials come out as they are, energies halved - LYP couples the channels and comes
    from isdf_gga_lyp_polarised on (rho_a, rho_b), its energy added once; the Hartree potential is that of the total density."""
    be, cell = mydf.backend, mydf.cell
    ncomp, pair_lyp, per_channel, channel = _xc_dispatch(be, fn, raw, spin)
    dms, kpts, band, shape = mydf._format_dms(dm, kpts, kpts_band)
    # the XC functional sees the real density: the Hermitian part of D (the reference takes the real part of rho)
    spec = mydf._eval_rhoG(mydf._hermitian_parts(dms, anti=False)[0][1], kpts, ncomp)

    def integrate(sp):
        return mydf._integrate(sp, band).reshape(shape)
    nset = dms.shape[0]
    mesh = np.asarray(mydf.mesh, dtype=np.int32)
    G = int(np.prod(mesh))
    weight = cell.vol / G
    scale = 2.0 if spin else 1.0                                             # 2 rho_sigma: what the spin-scaled functional sees
    rho = _real_space(mydf, spec, scale / cell.vol)
    rho_s = _real_space(mydf, spec, 1.0 / cell.vol) if pair_lyp else None     # the spin densities themselves, for LYP
    be.mg_coulomb_kernel(spec[0], mesh, cell.lattice_vectors())              # spec[0] now holds the Hartree potentials, set by set
    vH = _real_space(mydf, spec[:1], 1.0 / cell.vol)[0]
    exc = be.empty((nset, G))
    vxc = be.empty((ncomp, nset, G))                                         # v_rho and, for a GGA, de/d grad rho
    nelec, excsum, ecoul = np.zeros(nset), np.zeros(nset), np.zeros(nset)
    for i in range(nset):
        if per_channel:
            channel(rho[:, i], exc[i], vxc[:, i])
        nelec[i] = be.dot(rho[0, i]) / scale * weight
        if per_channel:
            excsum[i] = be.dot(rho[0, i], exc[i]) / scale * weight
        # a spin's density meets the Hartree potential of both spins, a closed-shell density its own
        ecoul[i] = 0.5 / scale * sum(be.dot(rho[0, i], vH[j]) for j in (range(nset) if spin else (i,))) * weight
    e_pair = 0.0
    if pair_lyp:
        be.gga_lyp_polarised(rho_s, fn[4], exc[0], vxc, accumulate=per_channel)     # exc[0] is free again: the energy density
        e_pair = be.dot(exc[0]) * weight
    del exc, rho, rho_s
    vj = integrate(spec[:1]) if return_j else None
    # potential spectra: XC on every component; J stays where it is for a closed shell, and is added in real space for a pair
    spec[1:].zero_()
    if spin or not with_j:
        spec[0].zero_()
    for c in range(ncomp):
        be.mg_embed_density(vxc[c], mesh, weight, spec[c], mesh, accumulate=True)
    if spin:
        nelec, excsum, ecoul = nelec.sum(), excsum.sum() + e_pair, ecoul.sum()
        if return_j:
            vj = vj[0] + vj[1]
        if with_j:                                                           # veff_sigma += the Hartree potential of the total density
            vtot = be.empty((2, G))
            for sp in range(2):
                vtot[sp].copy_(vH[1 - sp])
            be.mg_embed_density(vH, mesh, weight, spec[0], mesh, accumulate=True)
            be.mg_embed_density(vtot, mesh, weight, spec[0], mesh, accumulate=True)
    elif nset == 1:
        nelec, excsum, ecoul = nelec[0], excsum[0], ecoul[0]
    veff = integrate(spec)
    return nelec, excsum, TaggedArray(veff, ecoul=ecoul, exc=excsum, vj=vj, vk=None)


# ---- linear response of the XC potential (TDDFT / stability / Hessians), multigrid.py:1259-1550 ---------------------------
def _density_passes(mydf, dm_in, kpts, ncomp=1):
    """What the response functions share: the spectra (ncomp, nset, gc) of the (real) densities - with their gradients for
    ncomp = 4 - a stack of matrices stands for, each with its factor (Gamma: one pass; k-points: Hermitian and, if present,
    anti-Hermitian part), an integrator and nset."""
    dms, kpts, band, shape = mydf._format_dms(dm_in, None if kpts is None or mydf._is_gamma(kpts) else kpts)
    passes = [(fac, mydf._eval_rhoG(part, kpts, ncomp)) for fac, part in mydf._hermitian_parts(dms)]
    return passes, (lambda sp: mydf._integrate(sp, band).reshape(shape)), dms.shape[0]


def _ground_density(mydf, dm0, kpts, scale=1.0, ncomp=1):
    """scale * rho (ncomp = 4: and grad rho) of the ground-state matrix (or (alpha, beta) pair) on the dense mesh, device
    (ncomp, nset, G)."""
    passes, _, _ = _density_passes(mydf, dm0, kpts, ncomp)
    return _real_space(mydf, passes[0][1], scale / mydf.cell.vol)


def _response(mydf, dms, kpts, contract, with_j, total_j=False, w_scale=1.0, ncomp=1):
    """veff[n] = matrix of  w_scale * wv[n]  with wv = contract(rho1) (ncomp, nset, G), rho1 = the density (ncomp = 4: and its
    gradient) of each response matrix (+ Hartree potential of rho1[n], or of the pair's sum with total_j, on component 0)."""
    be, cell = mydf.backend, mydf.cell
    mesh = np.asarray(mydf.mesh, dtype=np.int32)
    weight = cell.vol / int(np.prod(mesh))
    passes, integrate, nset = _density_passes(mydf, dms, kpts, ncomp)
    veff = 0.0
    for fac, spec in passes:
        wv = contract(_real_space(mydf, spec, 1.0 / cell.vol))
        if with_j:
            be.mg_coulomb_kernel(spec[0], mesh, cell.lattice_vectors())
            if total_j:                                                      # both spins feel the Hartree potential of the sum
                _add_partner_hartree(mydf, spec[:1], nset)
        else:
            spec[0].zero_()
        spec[1:].zero_()
        for c in range(ncomp):
            be.mg_embed_density(wv[c], mesh, weight * w_scale, spec[c], mesh, accumulate=True)
        veff = veff + fac * integrate(spec)
    return np.asarray(veff)


def _add_partner_hartree(mydf, spec, nset):
    """spec (1, nset, gc) holds the Hartree potentials of (alpha responses | beta responses): add to each the one of its partner
    spin."""
    be, cell = mydf.backend, mydf.cell
    mesh = np.asarray(mydf.mesh, dtype=np.int32)
    vH = _real_space(mydf, spec, 1.0 / cell.vol)[0]
    swapped = be.empty(tuple(vH.shape))
    half = nset // 2
    swapped[:half].copy_(vH[half:])
    swapped[half:].copy_(vH[:half])
    be.mg_embed_density(swapped, mesh, cell.vol / int(np.prod(mesh)), spec[0], mesh, accumulate=True)


def _response_kind(xc_code, open_shell=False):
    """'lda' / 'vwn' / 'b88' for the response functions; open_shell: the spin-resolved kernel is needed (nr_uks_fxc, the triplet,
    cache_xc_kernel1(spin=1)) - for 'lda,vwn' that is the spin-polarised VWN, which is not implemented."""
    weights = None if isinstance(xc_code, (tuple, list)) else _XC_TABLE.get(str(xc_code).replace(' ', '').upper())
    kind = {(1.0, 0.0, 0.0, 0.0): 'lda', (1.0, 0.0, 1.0, 0.0): 'vwn', (0.0, 1.0, 0.0, 0.0): 'b88'}.get(
        None if weights is None else (weights[0], weights[1], weights[2], weights[4]))
    if kind is None:                        # every code with LYP among them: its second derivatives are not built
        raise NotImplementedError("xc=%r: the response is implemented for 'lda,', 'lda,vwn' and 'b88,' (no libxc in this tree)"
                                  % (xc_code,))
    if kind == 'vwn':
        if open_shell:
            raise NotImplementedError("xc=%r: the spin-polarised VWN correlation is not implemented (open-shell and triplet "
                                      "response; the closed-shell nr_rks_fxc and the singlet are)" % (xc_code,))
        return 'vwn'
    return kind


def _nset_of(mydf, dms, kpts):
    nao = mydf.cell.nao_nr()
    nk = 1 if kpts is None or mydf._is_gamma(kpts) else len(np.asarray(kpts).reshape(-1, 3))
    return int(np.asarray(dms).size // (nk * nao * nao))


# ---- contract: rho1 (ncomp, nset, G) -> wv (ncomp, nset, G), the kernel applied to every response density ----------------------
def _kernel_rows(mydf, rho0_dev, fxc, nrows, vwn=False):
    """Device rows f[n] = f_x(density row) (+ f_c of VWN5) (or the caller's fxc), one per response density (ground-state rows
    repeated)."""
    be = mydf.backend
    if fxc is not None:
        f = be.to_device(np.ascontiguousarray(np.asarray(fxc, dtype=np.float64).reshape(-1, rho0_dev.shape[1])))
    else:
        f = be.empty(tuple(rho0_dev.shape))
        for i in range(rho0_dev.shape[0]):
            be.lda_exchange_fxc(rho0_dev[i], f[i])
            if vwn:
                be.lda_vwn_fxc_add(rho0_dev[i], f[i])
    reps = nrows // f.shape[0]
    if reps <= 1:
        return f
    out = be.empty((nrows, f.shape[1]))
    for n in range(nrows):
        out[n].copy_(f[n // reps])
    return out


def _rows_contract(mydf, kernel_rows):
    """One component (LDA): wv[0, n] = kernel_rows[n] * rho1[0, n], a row product in place."""
    def contract(rho1):
        for n in range(rho1.shape[1]):
            mydf.backend.hadamard_rows(rho1[0, n:n + 1], kernel_rows[n:n + 1])
        return rho1
    return contract


def _b88_contract(mydf, rho0):
    """rho1 (4, nset, G) -> wv of the B88 kernel at rho0 (4, G) (device; the fused kernel isdf_gga_b88_fxc)."""
    def contract(rho1):
        wv = mydf.backend.empty(tuple(rho1.shape))
        mydf.backend.gga_b88_fxc(rho0, rho1, wv)
        return wv
    return contract


def _b88_contract_spins(mydf, rho0_2):
    """Open shell by spin scaling: rows of spin s (the s-th half of rho1) see the kernel at 2 rho_s, rho0_2 (4, 2, G) = (2 rho_s, ...);
    the factor 2 of f_ss = 2 f(2 rho_s) is the caller's w_scale."""
    def contract(rho1):
        be = mydf.backend
        half = rho1.shape[1] // 2
        wv = be.empty(tuple(rho1.shape))
        for sp in range(2):
            sl = slice(sp * half, (sp + 1) * half)
            be.gga_b88_fxc(rho0_2[:, sp], rho1[:, sl], wv[:, sl])
        return wv
    return contract


def _fxc_contract(mydf, fxc):
    """rho1 (nx, nset, G) -> wv of a caller-supplied closed-shell kernel fxc (nx, nx, G) (isdf_xc_fxc_apply)."""
    be = mydf.backend
    f = np.asarray(fxc, dtype=np.float64)
    nx = 1 if f.ndim <= 2 else f.shape[0]
    f_dev = be.to_device(np.ascontiguousarray(f.reshape(nx, nx, -1)))

    def contract(rho1):
        wv = be.empty(tuple(rho1.shape))
        be.xc_fxc_apply(f_dev, rho1, wv)
        return wv
    return contract


def _fxc_contract_spins(mydf, fxc):
    """Open-shell kernel fxc (2, nx, 2, nx, G): wv of spin b = sum_a rho1 of spin a through block fxc[a, :, b, :]."""
    be = mydf.backend
    f = np.asarray(fxc, dtype=np.float64)
    nx = f.shape[1]
    f_dev = be.to_device(np.ascontiguousarray(f.reshape(2, nx, 2, nx, -1)))

    def contract(rho1):
        half = rho1.shape[1] // 2
        wv = be.empty(tuple(rho1.shape))
        for b in range(2):
            for a in range(2):
                be.xc_fxc_apply(f_dev[a, :, b], rho1[:, a * half:(a + 1) * half], wv[:, b * half:(b + 1) * half], accumulate=a > 0)
        return wv
    return contract


def _closed_shell_contract(mydf, kind, r0, fxc, nset):
    """The contract of a closed-shell kernel: the caller's ``fxc`` (nx, nx, G), else the functional's at the total density ``r0``
    (ncomp, G) on the device.  LDA is the row product either way (``r0`` then only gives the row length under a caller's fxc)."""
    if kind == 'b88':
        return _fxc_contract(mydf, fxc) if fxc is not None else _b88_contract(mydf, r0)
    return _rows_contract(mydf, _kernel_rows(mydf, r0, fxc, nset, vwn=kind == 'vwn'))


def _b88_kernel_host(mydf, rho0):
    """(vxc (4, G), fxc (4, 4, G)) of B88 at rho0 (4, G) device: the potential of isdf_gga_b88 and the kernel's unique components
    written out by isdf_gga_b88_fxc."""
    be = mydf.backend
    G = rho0.shape[1]
    e, v = be.empty((1, G)), be.empty((4, G))
    be.gga_b88(rho0[0], rho0[1:], e[0], v[0], v[1:])
    f10 = be.empty((10, G))
    be.gga_b88_fxc(rho0, None, None, fxc=f10)
    f10 = be.to_host(f10)
    sym = [[0, 1, 2, 3], [1, 4, 5, 6], [2, 5, 7, 8], [3, 6, 8, 9]]
    return be.to_host(v), f10[np.array(sym)]


def nr_rks_fxc(mydf, xc_code, dm0, dms, hermi=0, with_j=False, rho0=None, vxc=None, fxc=None, kpts=None, verbose=None):
    """Closed-shell response matrix f_xc[rho0] rho1 (+ J[rho1]) of the matrices ``dms`` (multigrid.py:1259-1318): 'lda,', 'lda,vwn'
    and 'b88,' (rho1 and grad rho1 from the ladder, the fused kernel on the dense mesh, the GGA integration pass)."""
    kind = _response_kind(xc_code)
    ncomp = _ncomp(kind)
    r0 = None
    if ncomp == 1 or fxc is None:
        r0 = mydf.backend.to_device(np.asarray(rho0, dtype=np.float64).reshape(ncomp, -1)) if rho0 is not None \
            else _ground_density(mydf, dm0, kpts, ncomp=ncomp)[:, 0]
    contract = _closed_shell_contract(mydf, kind, r0, fxc, _nset_of(mydf, dms, kpts))
    return _response(mydf, dms, kpts, contract, with_j, ncomp=ncomp)


def nr_rks_fxc_st(mydf, xc_code, dm0, dms_alpha, singlet=True, rho0=None, vxc=None, fxc=None, kpts=None, verbose=None):
    """Singlet / triplet response of the alpha-spin response matrices (multigrid.py:1321-1386): f_aa +- f_ab at rho_a = rho0/2.
    For exchange alone f_ab = 0 and f_aa(rho0/2) = 2 f(rho0): singlet and triplet coincide.  A caller's fxc is the open-shell
    kernel (2, nx, 2, nx, G) of cache_xc_kernel1(spin=1).  'lda,vwn': the singlet only (f_aa + f_ab = 2 f(rho0))."""
    kind = _response_kind(xc_code, open_shell=not singlet)
    ncomp = _ncomp(kind)
    be = mydf.backend
    if fxc is not None:
        f = np.asarray(fxc, dtype=np.float64)
        fxc = f[0, :, 0] + f[0, :, 1] if singlet else f[0, :, 0] - f[0, :, 1]
        r0 = be.empty((1, fxc.size)) if ncomp == 1 else None
    elif rho0 is not None:
        r0 = be.to_device(2.0 * np.asarray(rho0, dtype=np.float64).reshape(2, ncomp, -1)[0])   # (rho_a, rho_b) in, total density out
    else:
        r0 = _ground_density(mydf, dm0, kpts, ncomp=ncomp)[:, 0]
    contract = _closed_shell_contract(mydf, kind, r0, fxc, _nset_of(mydf, dms_alpha, kpts))
    return _response(mydf, dms_alpha, kpts, contract, False, w_scale=1.0 if fxc is not None else 2.0, ncomp=ncomp)


def nr_uks_fxc(mydf, xc_code, dm0, dms, hermi=0, with_j=False, rho0=None, vxc=None, fxc=None, kpts=None, verbose=None):
    """Open-shell response (multigrid.py:1389-1452): dm0 = (alpha, beta), dms = (alpha responses..., beta responses...);
    w_s = f_ss(rho0_s) rho1_s with f_ss(rho_s) = 2 f(2 rho_s) by spin scaling, the Coulomb term of with_j from rho1_a + rho1_b.
    A caller's fxc is the kernel (2, nx, 2, nx, G) of cache_xc_kernel1(spin=1), applied block by block."""
    kind = _response_kind(xc_code, open_shell=True)
    ncomp = _ncomp(kind)
    if fxc is not None:
        return _response(mydf, dms, kpts, _fxc_contract_spins(mydf, fxc), with_j, total_j=True, ncomp=ncomp)
    if rho0 is not None:
        r0 = mydf.backend.to_device(2.0 * np.asarray(rho0, dtype=np.float64).reshape(2, ncomp, -1).transpose(1, 0, 2))
    else:
        r0 = _ground_density(mydf, dm0, kpts, scale=2.0, ncomp=ncomp)
    # r0 (ncomp, 2, G) = (2 rho_s, ...): what the spin-scaled kernel of each spin sees
    contract = _b88_contract_spins(mydf, r0) if kind == 'b88' else \
        _rows_contract(mydf, _kernel_rows(mydf, r0[0], None, _nset_of(mydf, dms, kpts)))
    return _response(mydf, dms, kpts, contract, with_j, total_j=True, w_scale=2.0, ncomp=ncomp)


def cache_xc_kernel1(mydf, xc_code, dm, spin=0, kpts=None):
    """(rho, vxc, fxc) of the ground state for the response functions (multigrid.py:1457-1500), array shapes of eval_xc_eff:
    LDA ('lda,', 'lda,vwn' at spin 0): spin 0 -> rho (G,), vxc (1, G), fxc (1, 1, G); spin 1 -> rho (2, G), vxc (2, 1, G),
    fxc (2, 1, 2, 1, G).  GGA ('b88,'): spin 0 -> rho (4, G), vxc (4, G), fxc (4, 4, G); spin 1 -> rho (2, 4, G), vxc (2, 4, G),
    fxc (2, 4, 2, 4, G) (spin scaling: the cross-spin blocks are zero)."""
    kind = _response_kind(xc_code, open_shell=spin == 1)
    be = mydf.backend
    rho = _ground_density(mydf, dm, kpts, ncomp=_ncomp(kind))               # (ncomp, n_dm, G)
    if spin == 0 and rho.shape[1] != 1:
        raise ValueError('spin = 0 takes one density matrix')
    if kind == 'b88':
        if spin == 0:
            r0 = rho[:, 0].contiguous()
            v, f = _b88_kernel_host(mydf, r0)
            return be.to_host(r0), v, f
        r = be.to_host(rho).transpose(1, 0, 2)                               # (n_dm, 4, G)
        if r.shape[0] == 1:
            r = np.repeat(r, 2, axis=0) * .5
        G = r.shape[2]
        vx, fx = np.empty((2, 4, G)), np.zeros((2, 4, 2, 4, G))
        for sp in range(2):
            v, f = _b88_kernel_host(mydf, be.to_device(np.ascontiguousarray(2.0 * r[sp])))
            vx[sp], fx[sp, :, sp] = v, 2.0 * f
        return np.ascontiguousarray(r), vx, fx
    rho = rho[0]
    if spin == 0:
        e, v, f = be.empty(tuple(rho.shape)), be.empty(tuple(rho.shape)), be.empty(tuple(rho.shape))
        be.lda_exchange(rho[0], e[0], v[0])
        be.lda_exchange_fxc(rho[0], f[0])
        if kind == 'vwn':
            be.lda_vwn_add(rho[0], e[0], v[0])
            be.lda_vwn_fxc_add(rho[0], f[0])
        return be.to_host(rho)[0], be.to_host(v), be.to_host(f)[None]
    r = be.to_host(rho)
    if r.shape[0] == 1:
        r = np.repeat(r, 2, axis=0) * .5
    r2 = be.to_device(2.0 * r)
    e, v, f = be.empty((2, r.shape[1])), be.empty((2, r.shape[1])), be.empty((2, r.shape[1]))
    fx = np.zeros((2, 1, 2, 1, r.shape[1]))
    for sp in range(2):
        be.lda_exchange(r2[sp], e[sp], v[sp])
        be.lda_exchange_fxc(r2[sp], f[sp])
    fh = be.to_host(f)
    fx[0, 0, 0, 0], fx[1, 0, 1, 0] = 2.0 * fh[0], 2.0 * fh[1]
    return r, be.to_host(v)[:, None], fx


def cache_xc_kernel(mydf, xc_code, mo_coeff, mo_occ, spin=0, kpts=None):
    raise NotImplementedError          # as the reference (multigrid.py:1454-1455)


def _mf_kpts(mf):
    if getattr(mf, 'kpts', None) is not None:
        return np.asarray(mf.kpts, dtype=float).reshape(-1, 3)
    return np.asarray(mf.kpt, dtype=float).reshape(1, 3)


def _gen_rhf_response(mf, dm0, singlet=None, hermi=0):
    """Closed-shell response function dm1 -> v1 for Newton / stability / TDDFT (multigrid.py:1503-1532): the kernel is cached once
    (cache_xc_kernel1); singlet None gives f_xc rho1 + J[rho1] (nr_rks_fxc, the orbital Hessian of a closed shell), True / False the
    singlet / triplet f_xc alone (nr_rks_fxc_st).  No exchange term: a hybrid caller adds ISDF.get_jk(dm1, with_j=False) itself.
    ``mf`` needs .with_df, .xc and .kpts (or .kpt)."""
    kpts = _mf_kpts(mf)
    rho0, vxc, fxc = cache_xc_kernel1(mf.with_df, mf.xc, dm0, 0 if singlet is None else 1, kpts)

    def vind(dm1):
        if hermi == 2:
            return np.zeros_like(dm1)
        if singlet is None:
            return nr_rks_fxc(mf.with_df, mf.xc, None, dm1, hermi, True, rho0, vxc, fxc, kpts)
        return nr_rks_fxc_st(mf.with_df, mf.xc, None, dm1, singlet, rho0, vxc, fxc, kpts)
    return vind


def _gen_uhf_response(mf, dm0, with_j=True, hermi=0):
    """Open-shell response function (multigrid.py:1534-1550): dm1 = (alpha responses..., beta responses...) -> nr_uks_fxc with the
    cached spin-resolved kernel."""
    kpts = _mf_kpts(mf)
    rho0, vxc, fxc = cache_xc_kernel1(mf.with_df, mf.xc, dm0, 1, kpts)

    def vind(dm1):
        if hermi == 2:
            return np.zeros_like(dm1)
        return nr_uks_fxc(mf.with_df, mf.xc, None, dm1, hermi, with_j, rho0, vxc, fxc, kpts)
    return vind


def multigrid_fftdf(mf):
    """Swap a mean-field object's density-fitting object for a MultiGridFFTDF on the same cell (multigrid.py:1904-1910)."""
    old = mf.with_df
    mf.with_df = MultiGridFFTDF(mf.cell, getattr(old, 'kpts', np.zeros((1, 3))))
    return mf


multigrid = multigrid_fftdf


from .xc_grad import get_vxc_e1, xc_nuc_grad, xc_nuc_grad_uks      # noqa: E402,F401  (the XC nuclear forces; xc_grad.py)
