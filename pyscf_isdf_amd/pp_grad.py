"""Nuclear forces of the pseudopotential energy and of local potentials on the device: ``pp_nuc_grad`` / ``get_pp_ip1`` /
``nuc_grad_local`` / ``get_j_nuc_grad``, the pseudopotential part of pyscf/pbc/grad/krhf.py:86-209 and the contraction of
krhf.py:64 without the N^2 G pair array of the one and the (3, N, N) matrix of the other.

Gamma point, one process, real AOs.  With E_pp(R; D) = sum_(mu nu) D_(nu mu) get_pp()_(mu nu), phi(r - R_mu):

  HF_loc[a, x]    = sum_g rho(g) Re ifft(i G_x SI_a vloc_a)(g)                          isdf_pp_local_force (Parseval, no FFT per atom)
  vloc[x, mu, nu] = sum_g d_x phi_mu(g) vlocR(g) phi_nu(g)
  S^x_(j m, mu)   = sum_G (i G_x) conj(SI_a(G)) p_jm(G) aoG_mu(G)                        isdf_pp_projector_overlaps_ip
                  = dS/dR_a (the projector's atom) = - dS/dR_mu (the AO's atom) = <p_jm | d_x phi_mu>
  vnl[x, mu, nu]  = 1/vol Re sum_blocks conj(S^x)_(i m mu) h_ij S_(j m nu)
  HF_nl[a, x]     = 2 sum_(blocks on a) sum_(mu nu) D_(nu mu) vnl_block[x, mu, nu]
  pp_nuc_grad[a]  = HF_loc[a] + HF_nl[a] - 2 sum_(mu in a) sum_nu (vloc + vnl)[:, mu, nu] D_(nu mu)
  nuc_grad_local(v, D)[a, x] = - 2 sum_(mu in a) sum_nu D_(mu nu) w sum_g d_x phi_mu(g) v(g) phi_nu(g),   w = vol / G.

Host orchestration only.  The grid is walked in chunks of ``e1_grid_chunk`` columns as jk_e1 walks it: per chunk one collocation of
(phi, grad phi), B = D phi (isdf_gemm_nn) and ONE isdf_rowdot3 per density (pp_nuc_grad also takes the chunk's density from that
B); nothing of size N x G x 3 is resident and no (3, N, N) matrix is formed for a force.  The nproj-sized contractions with the h_ij blocks and D run on the host.
"""
import time
import numpy as np
import torch
from ._common import _aoslice_by_atom


class PPGradMixin:
    # ---- refusals and shapes -------------------------------------------------------------------------------------------
    def _ppg_refuse(self, kpts, what):
        if hasattr(kpts, 'kpts_ibz') or self.kpts_symm is not None:
            raise NotImplementedError('%s with k-point symmetry is not implemented (Gamma point only)' % what)
        if not self._is_gamma(kpts) or not self._is_gamma(self.kpts):
            raise NotImplementedError('%s at k-points is not implemented (Gamma point only)' % what)
        if self._sharded:
            raise NotImplementedError('%s on the grid-sharded (multi-GPU) path is not implemented (one process only)' % what)

    def _ppg_dms(self, dm):
        """The symmetric parts (nset, nao, nao) of a real density matrix or stack, and whether it was a single matrix."""
        dm_in = np.asarray(dm)
        if np.iscomplexobj(dm_in):
            if abs(dm_in.imag).max() > 1e-12:
                raise ValueError('a real density matrix is needed: max|Im dm| = %.3g' % abs(dm_in.imag).max())
            dm_in = dm_in.real
        nao = self.cell.nao_nr()
        dms = np.asarray(dm_in, dtype=np.float64).reshape(-1, nao, nao)
        return 0.5 * (dms + dms.transpose(0, 2, 1)), dm_in.ndim == 2

    def _ppg_by_atom(self, rows):
        """(..., nao) -> (..., natm): the sum over the AOs of each atom."""
        aosl = _aoslice_by_atom(self.cell)
        return np.stack([rows[..., int(p0):int(p1)].sum(axis=-1) for p0, p1 in aosl[:, :2]], axis=-1)

    # ---- the walk over the grid (jk_e1's _e1_chunks) ----------------------------------------------------------------------
    def _ppg_local_rows(self, vR, d_sym, scale, rho=None):
        """r[s, x, mu] = scale sum_g d_x phi_mu(g) v_s(g) (D_s phi)_mu(g) on the host, (nset, 3, nao); vR (1 or nset, G) and
        d_sym (nset, nao, nao) on the device.  rho (nset, G), if given, receives the density of d_sym from the same collocation."""
        be = self.backend
        nset, nao = d_sym.shape[:2]
        rows = be.zeros((nset, 3, nao))
        ones = be.to_device(np.ones((1, nao)))
        B_buf = None
        for s0, s1, dao in self._e1_chunks():
            n = s1 - s0
            if B_buf is None:
                B_buf = be.empty((nao * n,))
            B = B_buf[:nao * n].view(nao, n)
            for s in range(nset):
                be.gemm_nn(d_sym[s], dao[0], B)
                be.rowdot3(dao[1:], vR[s if vR.shape[0] > 1 else 0, s0:s1], B, rows[s], alpha=scale, accumulate=s0 > 0)
                if rho is not None:                                # rho = sum_mu phi_mu (D phi)_mu from the B at hand, not a second D phi
                    be.hadamard_rows(B, dao[0])
                    be.gemm_nn(ones, B, rho[s:s + 1, s0:s1])
        return be.to_host(rows)

    def _ppg_rho(self, d_sym, rho):
        """rho (nset, G) of the symmetric d_sym, from the resident collocation when there is one."""
        be = self.backend
        if self.ao is not None:
            be.rho_pair(self.ao, self.ao, rho.shape[1], d_sym, rho)
        else:
            for s0, s1, phi in self._e1_chunks(1):
                be.rho_pair(phi, phi, s1 - s0, d_sym, rho[:, s0:s1])

    # ---- public surface --------------------------------------------------------------------------------------------------
    def nuc_grad_local(self, vR, dm, kpts=None):
        """The Pulay force of a real local potential on the dense mesh, (natm, 3) or (nset, natm, 3) for a stack:
            - 2 sum_(mu in a) sum_nu D^sym_(mu nu) w sum_g d_x phi_mu(g) v(g) phi_nu(g),   w = vol / G.
        vR is (G,) shared by the densities or (nset, G), one per density, on the host or the device: the XC potential of an LDA
        code, for instance (a GGA's force needs the gradient terms too: multigrid.xc_nuc_grad).  Only the symmetric part of dm
        contributes."""
        self._ppg_refuse(kpts, 'nuc_grad_local')
        dms, single = self._ppg_dms(dm)
        be = self.backend
        G = int(np.prod(self.mesh))
        v = vR if isinstance(vR, torch.Tensor) else be.to_device(np.asarray(vR, dtype=np.float64))
        v = v.reshape(-1, G)
        if v.shape[0] not in (1, len(dms)):
            raise ValueError('vR has %d rows for %d density matrices' % (v.shape[0], len(dms)))
        t0 = time.perf_counter()
        rows = self._ppg_local_rows(v, be.to_device(dms), self.cell.vol / G)
        self._tick('S8_nuc_grad_local', t0)
        f = -2.0 * self._ppg_by_atom(rows).transpose(0, 2, 1)
        return f[0] if single else f

    def get_j_nuc_grad(self, dm, kpts=None):
        """nuc_grad_local with v = v_J of the symmetric part of dm (one isdf_rho_pair and one isdf_coulomb_rows, as get_j_e1 makes
        them): the contraction 2 sum_(mu in a) sum_nu get_j_e1(dm)[x, mu, nu] dm_(nu mu) of pyscf/pbc/grad/krhf.py:64 for a
        symmetric dm, without the (3, nao, nao) matrix."""
        self._ppg_refuse(kpts, 'get_j_nuc_grad')
        if getattr(self.cell, 'omega', 0):
            raise NotImplementedError('get_j_nuc_grad with a range-separated Coulomb kernel (omega) is not implemented')
        dms, single = self._ppg_dms(dm)
        be = self.backend
        mesh = np.asarray(self.mesh, dtype=np.int32)
        G = int(np.prod(mesh))
        t0 = time.perf_counter()
        d_sym = be.to_device(dms)
        vJ = be.empty((len(dms), G))
        self._ppg_rho(d_sym, vJ)
        be.coulomb_rows(vJ, mesh, np.asarray(self.cell.lattice_vectors(), dtype=float), len(dms))
        rows = self._ppg_local_rows(vJ, d_sym, self.cell.vol / G)
        self._tick('S8_nuc_grad_local', t0)
        f = -2.0 * self._ppg_by_atom(rows).transpose(0, 2, 1)
        return f[0] if single else f

    def _ppg_overlaps(self, tables):
        """(4, nrows, nao) complex on the host: the projector overlaps and their i G_x weighted forms at Gamma; None without
        projectors."""
        cell, be = self.cell, self.backend
        _, proj_tab, proj_rl, _, nrows = tables
        if not proj_tab:
            return None
        ov = be.empty((4, nrows, cell.nao_nr()), dtype=torch.complex128)
        be.pp_projector_overlaps_ip(np.asarray(cell._atm), np.asarray(cell._bas), np.asarray(cell._env),
                                    np.asarray(cell.atom_coords(), dtype=float), np.zeros(3), np.array(proj_tab), np.array(proj_rl),
                                    np.asarray(self.mesh, dtype=np.int32), np.asarray(cell.lattice_vectors(), dtype=float), ov)
        return be.to_host(ov)

    def pp_nuc_grad_terms(self, dm, kpts=None):
        """The four terms of pp_nuc_grad, each (nset, natm, 3): 'hf_loc', 'pulay_loc', 'hf_nl', 'pulay_nl'."""
        self._ppg_refuse(kpts, 'pp_nuc_grad')
        dms, _ = self._ppg_dms(dm)
        tables = self._pp_tables()
        cell, be = self.cell, self.backend
        nset, natm = len(dms), cell.natm
        mesh = np.asarray(self.mesh, dtype=np.int32)
        G = int(np.prod(mesh))
        a = np.asarray(cell.lattice_vectors(), dtype=float)
        acoords = np.asarray(cell.atom_coords(), dtype=float)
        t0 = time.perf_counter()
        vlocR = be.empty((1, G))
        be.pp_local_potential(acoords, tables[0], mesh, a, vlocR)
        d_sym = be.to_device(dms)
        rho = be.empty((nset, G))
        rows = self._ppg_local_rows(vlocR, d_sym, 1.0, rho=rho)          # no quadrature weight: get_pp's local part has none
        t0 = self._tick('S8_nuc_grad_local', t0)
        hf_loc = be.empty((nset, natm, 3))
        be.pp_local_force(rho, acoords, tables[0], mesh, a, hf_loc)
        hf_loc = be.to_host(hf_loc)
        t0 = self._tick('S8_pp_grad_local_hf', t0)
        hf_nl, pulay_nl = np.zeros((nset, natm, 3)), np.zeros((nset, natm, 3))
        S4 = self._ppg_overlaps(tables)
        if S4 is not None:
            aosl = _aoslice_by_atom(cell)
            ao_atom = np.repeat(np.arange(natm), aosl[:, 1] - aosl[:, 0])
            for s in range(nset):
                SD = S4[0].dot(dms[s])                                    # (nrows, nao): sum_nu S_(j m nu) D_(nu mu)
                for row0, l, nl, hl, ia in tables[3]:
                    deg = 2 * l + 1
                    W = np.einsum('ij,jmp->imp', hl, SD[row0:row0 + nl * deg].reshape(nl, deg, -1))
                    Sx = S4[1:, row0:row0 + nl * deg].reshape(3, nl, deg, -1)
                    c = (2.0 / cell.vol) * np.einsum('ximp,imp->xp', Sx.conj(), W).real     # (3, nao)
                    hf_nl[s, ia] += c.sum(axis=1)
                    np.subtract.at(pulay_nl[s], ao_atom, c.T)
        self._tick('S8_pp_grad_nonlocal', t0)
        return {'hf_loc': hf_loc, 'pulay_loc': -2.0 * self._ppg_by_atom(rows).transpose(0, 2, 1), 'hf_nl': hf_nl,
                'pulay_nl': pulay_nl}

    def pp_nuc_grad(self, dm, kpts=None):
        """dE_pp/dR_a at fixed D for E_pp = sum_(mu nu) D_(nu mu) get_pp()_(mu nu), the AOs moving with their atoms: (natm, 3), or
        (nset, natm, 3) for a stack.  The pseudopotential part of sum tr(hcore_deriv(ia) dm) of pyscf/pbc/grad/krhf.py:144-209
        (vpploc_part1_nuc_grad + vpploc_part2_nuc_grad + vppnl_nuc_grad of the pair code), as the EXACT derivative of this
        object's get_pp: same mesh, normalisation and G = 0 handling, bare charges for atoms without an entry.  One difference
        from krhf.get_hcore: the reference's gradient code transforms the collocated AOs by FFT in the non-local part; get_pp
        here, like pyscf/pbc/df/fft.py:88-140, uses the analytic transform of the AOs, and the derivative follows get_pp.
        dm is real (max|Im| above 1e-12 raises ValueError); only its symmetric part contributes."""
        single = np.ndim(dm) == 2
        t = self.pp_nuc_grad_terms(dm, kpts)
        f = t['hf_loc'] + t['pulay_loc'] + t['hf_nl'] + t['pulay_nl']
        return f[0] if single else f

    def get_pp_ip1(self, kpts=None):
        """(3, nao, nao) real, the derivative on the bra: vloc[x, mu, nu] = sum_g d_x phi_mu(g) vlocR(g) phi_nu(g) plus
        vnl[x, mu, nu] = 1/vol Re sum_blocks conj(S^x)_(i m mu) h_ij S_(j m nu), S^x the projector overlap with grad phi_mu: the
        pseudopotential part of h1 of krhf.get_hcore (h1 without int1e_ipkin), with get_pp's analytic AO transform in the non-local
        part (see pp_nuc_grad).  For a symmetric D, pp_nuc_grad(D)[a] = HF[a] - 2 sum_(mu in a) sum_nu ip1[:, mu, nu] D_(nu mu) with
        HF = hf_loc + hf_nl of pp_nuc_grad_terms."""
        self._ppg_refuse(kpts, 'get_pp_ip1')
        tables = self._pp_tables()
        cell, be = self.cell, self.backend
        nao = cell.nao_nr()
        mesh = np.asarray(self.mesh, dtype=np.int32)
        G = int(np.prod(mesh))
        t0 = time.perf_counter()
        vlocR = be.empty((1, G))
        be.pp_local_potential(np.asarray(cell.atom_coords(), dtype=float), tables[0], mesh,
                              np.asarray(cell.lattice_vectors(), dtype=float), vlocR)
        d_v = be.zeros((3, nao, nao))
        for s0, s1, dao in self._e1_chunks():
            for x in range(3):
                be.gemm_nt(dao[1 + x], dao[0], d_v[x], alpha=1.0, beta=1.0, kscale=vlocR[0, s0:s1])
        v = be.to_host(d_v)
        t0 = self._tick('S8_nuc_grad_local', t0)
        S4 = self._ppg_overlaps(tables)
        if S4 is not None:
            for row0, l, nl, hl, _ in tables[3]:
                deg = 2 * l + 1
                blk = S4[:, row0:row0 + nl * deg].reshape(4, nl, deg, nao)
                v += np.einsum('ximp,ij,jmq->xpq', blk[1:].conj(), hl, blk[0], optimize=True).real / cell.vol
        self._tick('S8_pp_grad_nonlocal', t0)
        return v
