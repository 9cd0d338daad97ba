"""Nuclear forces of the XC energy on the device: ``get_vxc_e1`` / ``xc_nuc_grad`` / ``xc_nuc_grad_uks``, the grid term of an RKS / UKS
gradient (pyscf/pbc/grad/krks.py:68-112 ``get_vxc``; pyscf/grad/rks.py:196-240 for the GGA products) for the functionals of
multigrid._XC_TABLE.  Re-exported from pyscf_isdf_amd.multigrid.

Gamma point, one process, real AOs.  For a real symmetric D, rho = sum D_(mu nu) phi_mu phi_nu, the quadrature
weight wq = vol / G, (v_rho, w) = (de/d rho, de/d grad rho) from the functional kernels nr_rks uses, the AOs moving with their atoms:

  B = D phi
  Z_nu(g)   = v_rho(g) phi_nu(g) + sum_y w_y(g) d_y phi_nu(g)                                          isdf_gga_aow
  G_(x mu)(g) = sum_y w_y(g) d_x d_y phi_mu(g)                                                         isdf_gga_aow
  vxc_e1[x, mu, nu] = - wq sum_g [ d_x phi_mu Z_nu + G_(x mu) phi_nu ]                                  six isdf_gemm_nt per chunk
  dE_xc/dR_(A x) at fixed D = 2 sum_(mu in A) sum_nu vxc_e1[x, mu, nu] D_(nu mu)
                            = - 2 sum_(mu in A) wq sum_g [ d_x phi_mu (D Z)_mu + G_(x mu) B_mu ]        two isdf_gemm_nn, two isdf_rowdot3

Without gradients ('lda,', 'lda,vwn') w = 0: the force is nuc_grad_local(v_rho, D) and the matrix the three scaled products of
get_pp_ip1's local part.  The GGAs of this tree take grad rho from analytic AO gradients, so the exact derivative needs the AO
second derivatives: the dense mesh is walked in chunks as jk_e1 walks it, ten planes per chunk (isdf_eval_ao_deriv2).

Host orchestration only.  rho and grad rho come from the object's own level ladder (multigrid._ground_density's passes), the
potentials from the dispatch nr_rks / nr_uks use (multigrid._xc_dispatch).  A chunk holds 16 nao-row blocks of its columns (ten
planes, Z, G (3), B, D Z); the chunk is e1_grid_chunk, lowered so that those blocks take at most ``XC_GRAD_FRACTION`` of the free
device memory (a resident fit stays where it is).
"""
import time
import numpy as np

XC_GRAD_FRACTION = 0.25       # share of the free device memory the walk's 16 (nao, chunk) blocks may take
_BLOCKS = 16                  # ten collocation planes, Z, three planes of G, B = D phi, C = D Z


def _mg():
    from . import multigrid
    return multigrid


def _refuse(mydf, kpts, what):
    mydf._ppg_refuse(kpts, what)
    if not mydf._is_gamma(mydf.kpts_band):
        raise NotImplementedError('%s with kpts_band is not implemented (Gamma point only)' % what)


def _potentials(mydf, fn, raw, dms, spin):
    """(ncomp, nset, G) on the device: v_rho and, for a GGA, de/d grad rho of each symmetric real matrix of ``dms`` (nset, nao, nao) -
    a closed-shell density each, or (``spin``) the pair (alpha, beta): row s is then the potential spin s feels, exchange by spin
    scaling and LYP of both spins together, as multigrid._nr_ks(spin=True) makes them."""
    mg = _mg()
    be, cell = mydf.backend, mydf.cell
    ncomp, pair_lyp, per_channel, channel = mg._xc_dispatch(be, fn, raw, spin)
    spec = mg._density_passes(mydf, dms, None, ncomp)[0][0][1]
    nset = dms.shape[0]
    G = int(np.prod(mydf.mesh))
    rho = mg._real_space(mydf, spec, (2.0 if spin else 1.0) / cell.vol)      # 2 rho_sigma: what the spin-scaled functional sees
    exc = be.empty((nset, G))
    vxc = be.empty((ncomp, nset, G))
    if per_channel:
        for i in range(nset):
            channel(rho[:, i], exc[i], vxc[:, i])
    if pair_lyp:
        rho_s = mg._real_space(mydf, spec, 1.0 / cell.vol)
        be.gga_lyp_polarised(rho_s, fn[4], exc[0], vxc, accumulate=per_channel)
    return vxc


def _walk_chunk(mydf, nao):
    """Columns per chunk of the ten-plane walk."""
    fit = int(XC_GRAD_FRACTION * mydf.backend.free_bytes() // (8 * _BLOCKS * nao))
    return min(int(mydf.e1_grid_chunk), max(256, fit // 256 * 256))


def _gga_walk(mydf, vxc, dms, force):
    """The walk over the dense mesh for potentials ``vxc`` (4, nset, G) and symmetric matrices ``dms`` (nset, nao, nao), both on
    the device.  force: rows (nset, 3, nao) with rows[s, x, mu] = wq sum_g [d_x phi_mu (D Z)_mu + G_(x mu) B_mu]; else the matrices
    (nset, 3, nao, nao) = - wq sum_g [d_x phi_mu Z_nu + G_(x mu) phi_nu].  On the host."""
    be, cell = mydf.backend, mydf.cell
    nset, nao = dms.shape[:2]
    w = cell.vol / int(np.prod(mydf.mesh))
    chunk = _walk_chunk(mydf, nao)
    out = be.zeros((nset, 3, nao)) if force else be.zeros((nset, 3, nao, nao))
    work = ones = None
    for s0, s1, ao in mydf._e1_chunks(10, chunk):
        n = s1 - s0
        if work is None:                                               # the first chunk is the longest
            work = be.empty(((6 if force else 4) * nao * n,))
            ones = be.to_device(np.ones(n))
        Z = work[:nao * n].view(nao, n)
        G3 = work[nao * n:4 * nao * n].view(3, nao, n)
        for s in range(nset):
            be.gga_aow(ao, vxc[:, s, s0:s1], Z, G3)
            if force:
                B = work[4 * nao * n:5 * nao * n].view(nao, n)
                C = work[5 * nao * n:6 * nao * n].view(nao, n)
                be.gemm_nn(dms[s], ao[0], B)
                be.gemm_nn(dms[s], Z, C)
                be.rowdot3(ao[1:4], ones[:n], C, out[s], alpha=w, accumulate=s0 > 0)
                be.rowdot3(G3, ones[:n], B, out[s], alpha=w, accumulate=True)
            else:
                for x in range(3):
                    be.gemm_nt(ao[1 + x], Z, out[s, x], alpha=-w, beta=1.0)
                    be.gemm_nt(G3[x], ao[0], out[s, x], alpha=-w, beta=1.0)
    return be.to_host(out)


def _lda_matrices(mydf, v, nset):
    """(nset, 3, nao, nao) = - wq sum_g d_x phi_mu v_s(g) phi_nu: the scaled products of get_pp_ip1's local part; v (nset, G)."""
    be, cell = mydf.backend, mydf.cell
    nao = cell.nao_nr()
    w = cell.vol / int(np.prod(mydf.mesh))
    out = be.zeros((nset, 3, nao, nao))
    for s0, s1, dao in mydf._e1_chunks():
        for s in range(nset):
            for x in range(3):
                be.gemm_nt(dao[1 + x], dao[0], out[s, x], alpha=-w, beta=1.0, kscale=v[s, s0:s1])
    return be.to_host(out)


def _forces(mydf, fn, raw, dms, spin):
    """(nset, natm, 3): the force of each matrix of ``dms`` under its own potential."""
    be = mydf.backend
    t0 = time.perf_counter()
    vxc = _potentials(mydf, fn, raw, dms, spin)
    if vxc.shape[0] == 1:
        f = mydf.nuc_grad_local(vxc[0], dms)
    else:
        rows = _gga_walk(mydf, vxc, be.to_device(dms), True)
        f = -2.0 * mydf._ppg_by_atom(rows).transpose(0, 2, 1)
    mydf._tick('S8_xc_nuc_grad', t0)
    return f


def xc_nuc_grad(mydf, xc_code, dm, kpts=None, omega=None):
    """dE_xc/dR_A at fixed D for the closed-shell XC energy of nr_rks(mydf, xc_code, dm), the AOs moving with their atoms: (natm, 3),
    or (nset, natm, 3) for a stack, without the (3, nao, nao) matrix of get_vxc_e1.  Exact for every code of _XC_TABLE on the dense
    mesh (the GGAs through the AO second derivatives); no grid response (the uniform mesh does not move with the atoms).  dm is real
    (max|Im| above 1e-12 raises ValueError); only its symmetric part contributes.  ``omega`` as in nr_rks."""
    mg = _mg()
    fn = mg._functional_at(xc_code, omega)
    _refuse(mydf, kpts, 'xc_nuc_grad')
    dms, single = mydf._ppg_dms(dm)
    f = _forces(mydf, fn, isinstance(xc_code, (tuple, list)), dms, False)
    return f[0] if single else f


def xc_nuc_grad_uks(mydf, xc_code, dm_ab):
    """The same for the open-shell energy of nr_uks(mydf, xc_code, dm_ab), dm_ab = (alpha, beta): (natm, 3), the two spin channels'
    forces summed - each channel's matrix under the potential that spin feels (exchange by spin scaling, LYP from the spin-polarised
    kernel).  Codes with VWN correlation are refused as nr_uks refuses them."""
    mg = _mg()
    fn = mg._functional(xc_code)
    if fn[2] != 0:
        raise NotImplementedError("xc=%r: the spin-polarised VWN correlation is not implemented (closed-shell nr_rks only)" % (xc_code,))
    _refuse(mydf, None, 'xc_nuc_grad_uks')
    if np.ndim(dm_ab) != 3 or np.shape(dm_ab)[0] != 2:
        raise ValueError('xc_nuc_grad_uks takes one pair (alpha, beta) of density matrices')
    dms, _ = mydf._ppg_dms(dm_ab)
    return _forces(mydf, fn, isinstance(xc_code, (tuple, list)), dms, True).sum(axis=0)


def get_vxc_e1(mydf, xc_code, dm, kpts=None, omega=None):
    """vxc_e1[x, mu, nu] = - wq sum_g [d_x phi_mu Z_nu + G_(x mu) phi_nu], the derivative on the bra: the reference's get_vxc
    (pyscf/pbc/grad/krks.py:68-112, -vmat) at the Gamma point for the potential of the closed-shell density of dm.  (3, nao, nao)
    for one matrix, (3, nset, nao, nao) for a stack - the shapes of get_j_e1.  For a symmetric dm,
    xc_nuc_grad(dm)[A] = 2 sum_(mu in A) sum_nu vxc_e1[:, mu, nu] dm_(nu mu).  ``omega`` as in nr_rks."""
    mg = _mg()
    fn = mg._functional_at(xc_code, omega)
    _refuse(mydf, kpts, 'get_vxc_e1')
    dms, single = mydf._ppg_dms(dm)
    t0 = time.perf_counter()
    vxc = _potentials(mydf, fn, isinstance(xc_code, (tuple, list)), dms, False)
    if vxc.shape[0] == 1:
        v = _lda_matrices(mydf, vxc[0], len(dms))
    else:
        v = _gga_walk(mydf, vxc, mydf.backend.to_device(dms), False)
    mydf._tick('S8_xc_nuc_grad', t0)
    v = v.transpose(1, 0, 2, 3)
    return np.ascontiguousarray(v[:, 0]) if single else np.ascontiguousarray(v)
