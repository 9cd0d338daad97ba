"""``get_j_e1`` / ``get_k_e1`` / ``get_jk_e1``: the derivative matrices of FFTDF (pyscf/pbc/df/fft.py:277-291,
pyscf/pbc/df/fft_jk.py:111-175 and :304-411), the only ``with_df`` methods pyscf/pbc/grad/krhf.py:313-337 calls.

Gamma point, one process, real AOs, w = vol / G:

  vj_e1[a, mu, nu] = - sum_g w d_a phi_mu(g) v_J(g) phi_nu(g),   v_J = conv(rho), rho of the symmetric part of D (exact);
  vk_e1[a, mu, nu] = - sum_(lam sig) D_(lam sig) (d_a mu lam | sig nu)  with only the pair (sig nu) fitted:
      F_P(g) = sum_(lam sig) phi_lam(g) D_(lam sig) phi_sig(P),   T_a[P, mu] = w sum_g F_P(g) V_P(g) d_a phi_mu(g),
      vk_e1[a] = - T_a^T phi_P,   V_P = conv(Theta_P) = what a robust_k build keeps.

Host orchestration only.  The grid is walked in column chunks (``e1_grid_chunk``): per chunk one collocation of (phi, grad phi),
for J three scaled NT products per density, for K per batch of points F = left . right[:, chunk] and ONE launch of
isdf_gemm_nt_had3 (``e1_fused``, up to ``e1_fused_max_nao`` AOs; else hadamard_rows + three gemm_nt) that accumulates into the
resident T (3, P, nao).

``get_k_nuc_grad`` / ``get_jk_nuc_grad``: the same half-fitted exchange derivative contracted with D before the grid sum.  With the
symmetric D = U e U^T (r kept eigenvectors), left = phi_P U e (P, r), right = U^T phi (r, G), F = left . right, V = conv(Theta):

  2 sum_(mu in A) sum_nu vk_e1[x, mu, nu] D_(nu mu) = - 2 w sum_(mu in A) sum_g d_x phi_mu(g) Y[mu, g],   Y = U Z,   Z = left^T (F o V).

Per chunk and batch of points F (isdf_gemm_nn) and ONE launch of isdf_gemm_nn_had (``k_grad_fused``, up to ``k_grad_fused_max_rank``
kept eigenvectors; else hadamard_rows + gemm_nn) that accumulates Z (r, chunk) over the batches; per chunk Y = U Z and one
isdf_rowdot3.  Per density 4 P r G + 2 N r G flop instead of 2 P r G + 6 P N G, and nothing of size P x N x 3 or N x N x 3 exists.
"""
import time
import numpy as np
import torch
from . import gto


class JKE1Mixin:
    e1_grid_chunk = 65536         # grid columns per chunk: (4, nao, chunk) of collocation is all that is resident of size N x G
    e1_fused = True               # K: A o H B_a^T for the three components in one launch (isdf_gemm_nt_had3); False, or a backend
                                  # without gemm_nt_had3: the composition hadamard_rows + three gemm_nt
    e1_fused_max_nao = 512        # the one launch runs up to this many AOs: on an MI355X it is 9 - 18 % ahead of the composition at 208
                                  # AOs and 16 - 19 % behind at 1024 and 2048 (its 32-column tile re-reads A and H four times as often
                                  # as the NT kernels' 128 columns; profiles/r13_e1_had3_fused_vs_composition.log); the crossover
                                  # between 208 and 1024 has not been located more finely
    e1_row_batch = None           # K: points per batch of F rows (None: F at most 2 GiB)
    k_grad_fused = True           # get_k_nuc_grad: Z += left^T (V o F) in one launch (isdf_gemm_nn_had); False, or a backend without
                                  # gemm_nn_had: the composition hadamard_rows + gemm_nn
    k_grad_fused_max_rank = 256   # the one launch runs up to this many kept eigenvectors of D (one 256-row tile): on an MI355X, on
                                  # batches of 4096 points x 65 536 columns, it is 49 % ahead of the composition at r = 32 and 30 % at
                                  # 256, and 7 % and 16 % behind at 702 and 1664, where rocBLAS runs the plain product faster than the
                                  # own NN kernel (profiles/r17_k_nuc_grad_diamond222_diamond444.log); the crossover between 256 and
                                  # 702 has not been located more finely

    def _e1_refuse(self, kpts, kpts_band):
        if hasattr(kpts, 'kpts_ibz') or self.kpts_symm is not None:
            raise NotImplementedError('get_jk_e1 with k-point symmetry is not implemented (Gamma point only)')
        if not self._is_gamma(kpts) or not self._is_gamma(self.kpts):
            raise NotImplementedError('get_jk_e1 at k-points is not implemented (Gamma point only)')
        if not self._is_gamma(kpts_band) or not self._is_gamma(self.kpts_band):
            raise NotImplementedError('get_jk_e1 with kpts_band is not implemented (Gamma point only)')
        if self._sharded:
            raise NotImplementedError('get_jk_e1 on the grid-sharded (multi-GPU) path is not implemented (one process only)')
        if getattr(self.cell, 'omega', 0):
            raise NotImplementedError('get_jk_e1 with a range-separated Coulomb kernel (omega) is not implemented')

    def _e1_refuse_omega(self, *args, **kwargs):
        raise NotImplementedError('get_jk_e1 with a range-separated Coulomb kernel (omega) is not implemented')

    # ---- public surface ----------------------------------------------------------------------------------------------------
    def get_j_e1(self, dm, kpts=None, kpts_band=None):
        self._e1_refuse(kpts, kpts_band)
        return self._e1_linear(dm, True, False)[0]

    def get_k_e1(self, dm, kpts=None, kpts_band=None, exxdiv=None):
        self._e1_refuse(kpts, kpts_band)
        self._e1_check_exxdiv(exxdiv)
        return self._e1_linear(dm, False, True)[1]

    def get_jk_e1(self, dm, kpts=None, kpts_band=None, exxdiv=None):
        self._e1_refuse(kpts, kpts_band)
        self._e1_check_exxdiv(exxdiv)
        return self._e1_linear(dm, True, True)

    def get_k_nuc_grad(self, dm, kpts=None, exxdiv=None):
        """The exchange force contracted on the device, (natm, 3) or (nset, natm, 3) for a stack (each density its own exchange
        force: a UHF pair is a stack of two):
            2 sum_(mu in A) sum_nu get_k_e1(dm_sym)[x, mu, nu] dm_sym[nu, mu],   dm_sym the symmetric part of dm,
        without T (3, P, nao) and without the (3, nao, nao) matrix (module docstring; shapes and signs as get_j_nuc_grad).  The
        RHF two-electron force of pyscf/pbc/grad/krhf.py:64 is get_j_nuc_grad(dm) - 1/2 get_k_nuc_grad(dm).  Needs what get_k_e1
        needs: a robust_k build; None and 'ewald' give the same numbers."""
        self._kg_refuse(kpts, exxdiv, 'get_k_nuc_grad')
        return self._kg_forces(dm, False)[1]

    def get_jk_nuc_grad(self, dm, kpts=None, exxdiv=None):
        """(get_j_nuc_grad(dm), get_k_nuc_grad(dm)) from ONE walk over the grid chunks: (phi, grad phi) of a chunk is collocated
        once for both."""
        self._kg_refuse(kpts, exxdiv, 'get_jk_nuc_grad')
        return self._kg_forces(dm, True)

    def _kg_refuse(self, kpts, exxdiv, what):
        if hasattr(kpts, 'kpts_ibz') or self.kpts_symm is not None:
            raise NotImplementedError('%s with k-point symmetry is not implemented (Gamma point only)' % what)
        if not self._is_gamma(kpts) or not self._is_gamma(self.kpts):
            raise NotImplementedError('%s at k-points is not implemented (Gamma point only)' % what)
        if not self._is_gamma(self.kpts_band):
            raise NotImplementedError('%s with kpts_band is not implemented (Gamma point only)' % what)
        if self._sharded:
            raise NotImplementedError('%s on the grid-sharded (multi-GPU) path is not implemented (one process only)' % what)
        if getattr(self.cell, 'omega', 0):
            self._kg_refuse_omega(what)
        if exxdiv is None:
            exxdiv = self.exxdiv
        if exxdiv not in (None, 'ewald'):
            raise NotImplementedError("%s with exxdiv=%r is not implemented (None and 'ewald')" % (what, exxdiv))

    def _kg_refuse_omega(self, what='get_k_nuc_grad'):
        raise NotImplementedError('%s with a range-separated Coulomb kernel (omega) is not implemented' % what)

    def _e1_check_exxdiv(self, exxdiv):
        # the G = 0 term has no gradient (fft_jk.py:406-409): None and 'ewald' give the same matrix
        if exxdiv is None:
            exxdiv = self.exxdiv
        if exxdiv not in (None, 'ewald'):
            raise NotImplementedError("get_k_e1 with exxdiv=%r is not implemented (None and 'ewald')" % (exxdiv,))

    def _e1_linear(self, dm, with_j, with_k):
        """Shapes as _format_jks gives each component: dm (nao, nao) -> (3, nao, nao), (nset, nao, nao) -> (3, nset, nao, nao); a
        complex dm by linearity, as get_jk has it."""
        if with_k and not self.robust_k and self._V is None:
            raise RuntimeError('robust_k needs a build with robust_k=True (Theta explicit, V = conv(Theta) kept)')
        dm_in = np.asarray(dm)
        if np.iscomplexobj(dm_in):
            if abs(dm_in.imag).max() > 1e-12:
                re = self._e1_linear(dm_in.real, with_j, with_k)
                im = self._e1_linear(dm_in.imag, with_j, with_k)
                return tuple(None if r is None else r + 1j * i for r, i in zip(re, im))
            dm_in = dm_in.real
        nao = self.cell.nao_nr()
        dms = np.ascontiguousarray(dm_in.reshape(-1, nao, nao), dtype=np.float64)
        if with_k:
            if not self._built:
                if hasattr(self, '_k_requested'):            # MultiGridFFTDF: the fit lives in the parent's build
                    self._k_requested = True
                self.build()
            if self.pair_space == 'occ':
                self._ensure_fit(dm)
            if self._V is None:
                raise RuntimeError('robust_k needs a build with robust_k=True (Theta explicit, V = conv(Theta) kept)')
        vj, vk = self._e1_walk(dms, with_j, with_k)
        shape = (3,) + dm_in.shape
        return (None if vj is None else vj.transpose(1, 0, 2, 3).reshape(shape),
                None if vk is None else vk.transpose(1, 0, 2, 3).reshape(shape))

    # ---- the walk over the grid ----------------------------------------------------------------------------------------------
    def _e1_left_right(self, D):
        """left (P, r), right (r, G) with F = left . right = [sum_(lam sig) phi_lam(g) D_(lam sig) phi_sig(P)], formed as
        _robust_k_correction forms them: through the eigenvectors of a symmetric D of low rank, else left = phi_P D^T, right = phi."""
        be = self.backend
        nao = self.cell.nao_nr()
        P = self.aoP.shape[0]
        if bool(torch.allclose(D, D.T, rtol=0, atol=1e-13 * float(D.abs().max()) + 1e-300)):
            ev, U = torch.linalg.eigh(D)
            keep = ev.abs() > 1e-12 * float(ev.abs().max())
            r = int(keep.sum())
            if 0 < r <= nao // 2:
                Ur = U[:, keep].contiguous()
                left = be.empty((P, r))
                be.gemm_nn(self.aoP, (Ur * ev[keep]).contiguous(), left)
                right = be.empty((r, self.ao.shape[1]))
                be.gemm_nn(Ur.T.contiguous(), self.ao, right)
                return left, right
        left = be.empty((P, nao))
        be.gemm_nn(self.aoP, D.T.contiguous(), left)
        return left, self.ao

    def _e1_chunks(self, ncomp=4, chunk=None):
        """(s0, s1, collocation (4, nao, n) of (phi, grad phi), phi (nao, n) for ncomp = 1, or (10, nao, n) with the second
        derivatives for ncomp = 10) over the grid in chunks of e1_grid_chunk columns (or ``chunk``); the same shells, images and
        cutoffs as collocate().  One buffer: a chunk is valid until the next."""
        cell, be = self.cell, self.backend
        nao = cell.nao_nr()
        G = int(np.prod(self.mesh))
        chunk = max(1, min(int(self.e1_grid_chunk if chunk is None else chunk), G))
        rcut = gto.estimate_rcut_per_shell(cell)
        Ls = gto.get_lattice_Ls(cell, rcut=rcut.max())
        ao_args = (np.asarray(cell._atm), np.asarray(cell._bas), np.asarray(cell._env), Ls, rcut)
        coords = self.grids.coords
        buf = be.empty((ncomp * nao * chunk,))
        for s0 in range(0, G, chunk):
            s1 = min(G, s0 + chunk)
            xyz = be.to_device(np.ascontiguousarray(coords[s0:s1].T))
            if ncomp == 1:
                out = buf[:nao * (s1 - s0)].view(nao, s1 - s0)
                be.eval_ao(*ao_args, xyz, out)
            elif ncomp == 10:
                out = buf[:10 * nao * (s1 - s0)].view(10, nao, s1 - s0)
                be.eval_ao_deriv2(*ao_args, xyz, out)
            else:
                out = buf[:4 * nao * (s1 - s0)].view(4, nao, s1 - s0)
                be.eval_ao_deriv1(*ao_args, xyz, out)
            yield s0, s1, out

    def _e1_walk(self, dms, with_j, with_k):
        """(vj, vk), each (nset, 3, nao, nao) on the host or None, of real density matrices dms (nset, nao, nao)."""
        cell, be = self.cell, self.backend
        nset, nao = dms.shape[:2]
        mesh = np.asarray(self.mesh, dtype=np.int32)
        G = int(np.prod(mesh))
        a = np.asarray(cell.lattice_vectors(), dtype=float)
        w = cell.vol / G
        chunk = max(1, min(int(self.e1_grid_chunk), G))
        t0 = time.perf_counter()
        d_vj = vJ = None
        if with_j:
            # rho of the symmetric part of D (hermi = 1, fft_jk.py:119) on the whole grid, then ONE convolution per density
            d_sym = be.to_device(0.5 * (dms + dms.transpose(0, 2, 1)))
            vJ = be.empty((nset, G))
            if self.ao is not None:
                be.rho_pair(self.ao, self.ao, G, d_sym, vJ)
            else:
                for s0, s1, phi in self._e1_chunks(1):
                    be.rho_pair(phi, phi, s1 - s0, d_sym, vJ[:, s0:s1])
            be.coulomb_rows(vJ, mesh, a, nset)
            d_vj = be.zeros((nset, 3, nao, nao))
            t0 = self._tick('S8_get_j_e1', t0)
        T = lr = None
        fused = bool(self.e1_fused) and hasattr(be, 'gemm_nt_had3') and nao <= int(self.e1_fused_max_nao)
        if with_k:
            V = self._V
            P = V.shape[0]
            d_dm = be.to_device(dms)
            lr = [self._e1_left_right(d_dm[s]) for s in range(nset)]
            T = be.zeros((nset, 3, P, nao))
            nb = int(self.e1_row_batch) if self.e1_row_batch else max(128, int((2 << 30) // (8 * chunk)))
            nb = max(1, min(P, nb))
            F_buf = be.empty((nb * chunk,))
            t0 = self._tick('S8_get_k_e1', t0)
        for s0, s1, dao in self._e1_chunks():
            n = s1 - s0
            if with_j:
                for s in range(nset):
                    ks = vJ[s, s0:s1]
                    for x in range(3):
                        be.gemm_nt(dao[1 + x], dao[0], d_vj[s, x], alpha=-w, beta=1.0, kscale=ks)
                t0 = self._tick('S8_get_j_e1', t0)
            if with_k:
                for s in range(nset):
                    left, right = lr[s]
                    for r0 in range(0, P, nb):
                        r1 = min(P, r0 + nb)
                        F = F_buf[:(r1 - r0) * n].view(r1 - r0, n)
                        be.gemm_nn(left[r0:r1], right[:, s0:s1], F)
                        if fused:
                            be.gemm_nt_had3(F, V[r0:r1, s0:s1], dao[1:], T[s, :, r0:r1], alpha=w, beta=1.0)
                        else:
                            be.hadamard_rows(F, V[r0:r1, s0:s1])
                            for x in range(3):
                                be.gemm_nt(F, dao[1 + x], T[s, x, r0:r1], alpha=w, beta=1.0)
                t0 = self._tick('S8_get_k_e1', t0)
        vj = vk = None
        if with_j:
            vj = be.to_host(d_vj)
        if with_k:
            d_vk = be.empty((nset, 3, nao, nao))
            for s in range(nset):
                for x in range(3):
                    be.gemm_nn(T[s, x].T.contiguous(), self.aoP, d_vk[s, x], alpha=-1.0)
            self._tick('S8_get_k_e1', t0)
            vk = be.to_host(d_vk)
        return vj, vk

    # ---- the contracted exchange force ------------------------------------------------------------------------------------------
    def _kg_forces(self, dm, with_j):
        """(fj or None, fk), each (natm, 3) or (nset, natm, 3), of the symmetric part of dm."""
        if not self.robust_k and self._V is None:
            raise RuntimeError('robust_k needs a build with robust_k=True (Theta explicit, V = conv(Theta) kept)')
        dms, single = self._ppg_dms(dm)
        if not self._built:
            if hasattr(self, '_k_requested'):                # MultiGridFFTDF: the fit lives in the parent's build
                self._k_requested = True
            self.build()
        if self.pair_space == 'occ':
            self._ensure_fit(dms[0] if single else dms)
        if self._V is None:
            raise RuntimeError('robust_k needs a build with robust_k=True (Theta explicit, V = conv(Theta) kept)')
        rows = self._kg_walk(dms, with_j)
        out = []
        for r in rows:
            f = None if r is None else -2.0 * self._ppg_by_atom(r).transpose(0, 2, 1)
            out.append(f if f is None or not single else f[0])
        return tuple(out)

    def _kg_factors(self, D):
        """U (nao, r), A = left^T (r, P) and right (r, G) of a symmetric D = U e U^T, left = phi_P U e and right = U^T phi: every
        eigenvector with |e| > 1e-12 max|e| is kept (a full-rank D gives r = nao).  A's rows start on 16-byte boundaries."""
        be = self.backend
        P = self.aoP.shape[0]
        ev, U = torch.linalg.eigh(D)
        keep = ev.abs() > 1e-12 * float(ev.abs().max())
        r = int(keep.sum())
        if r == 0:
            return None
        Ur = U[:, keep].contiguous()
        left = be.empty((P, r))
        be.gemm_nn(self.aoP, (Ur * ev[keep]).contiguous(), left)
        A = be.empty((r, P + (P & 1)))[:, :P]
        A.copy_(left.T)
        right = be.empty((r, self.ao.shape[1]))
        be.gemm_nn(Ur.T.contiguous(), self.ao, right)
        return Ur, A, left, right

    def _kg_walk(self, dms, with_j):
        """(rows_j or None, rows_k) on the host, (nset, 3, nao) each, of symmetric density matrices dms (nset, nao, nao):
            rows_j[s, x, mu] = w sum_g d_x phi_mu(g) v_J(g) (D phi)_mu(g)           as _ppg_local_rows has it, operation by operation
            rows_k[s, x, mu] = w sum_g d_x phi_mu(g) Y[mu, g],   Y = U Z,   Z = left^T (F o V),   F = left . right."""
        cell, be = self.cell, self.backend
        nset, nao = dms.shape[:2]
        mesh = np.asarray(self.mesh, dtype=np.int32)
        G = int(np.prod(mesh))
        w = cell.vol / G
        chunk = max(1, min(int(self.e1_grid_chunk), G))
        t0 = time.perf_counter()
        d_sym = be.to_device(dms)
        rows_j = vJ = None
        if with_j:
            vJ = be.empty((nset, G))
            self._ppg_rho(d_sym, vJ)
            be.coulomb_rows(vJ, mesh, np.asarray(cell.lattice_vectors(), dtype=float), nset)
            rows_j = be.zeros((nset, 3, nao))
            t0 = self._tick('S8_nuc_grad_local', t0)
        V = self._V
        P = V.shape[0]
        fac = [self._kg_factors(d_sym[s]) for s in range(nset)]
        rmax = max([f[0].shape[1] for f in fac if f is not None] + [1])
        rows_k = be.zeros((nset, 3, nao))
        nb = int(self.e1_row_batch) if self.e1_row_batch else max(128, int((2 << 30) // (8 * chunk)))
        nb = max(1, min(P, nb))
        F_buf = be.empty((nb * chunk,))
        Z_buf = be.empty((rmax * chunk,))
        Y_buf = be.empty((nao * chunk,))
        ones = be.to_device(np.ones(chunk))
        fused = bool(self.k_grad_fused) and hasattr(be, 'gemm_nn_had')
        t0 = self._tick('S8_get_k_nuc_grad', t0)
        for s0, s1, dao in self._e1_chunks():
            n = s1 - s0
            Y = Y_buf[:nao * n].view(nao, n)
            if with_j:
                for s in range(nset):
                    be.gemm_nn(d_sym[s], dao[0], Y)
                    be.rowdot3(dao[1:], vJ[s, s0:s1], Y, rows_j[s], alpha=w, accumulate=s0 > 0)
                t0 = self._tick('S8_nuc_grad_local', t0)
            for s in range(nset):
                if fac[s] is None:
                    continue
                U, A, left, right = fac[s]
                Z = Z_buf[:U.shape[1] * n].view(U.shape[1], n)
                for r0 in range(0, P, nb):
                    r1 = min(P, r0 + nb)
                    F = F_buf[:(r1 - r0) * n].view(r1 - r0, n)
                    be.gemm_nn(left[r0:r1], right[:, s0:s1], F)
                    beta = 0.0 if r0 == 0 else 1.0
                    if fused and U.shape[1] <= int(self.k_grad_fused_max_rank):
                        be.gemm_nn_had(A[:, r0:r1], V[r0:r1, s0:s1], F, Z, alpha=1.0, beta=beta)
                    else:
                        be.hadamard_rows(F, V[r0:r1, s0:s1])
                        be.gemm_nn(A[:, r0:r1], F, Z, alpha=1.0, beta=beta)
                be.gemm_nn(U, Z, Y)
                be.rowdot3(dao[1:], ones[:n], Y, rows_k[s], alpha=w, accumulate=s0 > 0)
            t0 = self._tick('S8_get_k_nuc_grad', t0)
        return (None if rows_j is None else be.to_host(rows_j)), be.to_host(rows_k)
