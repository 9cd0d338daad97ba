"""k-point build and J/K of ``isdf.ISDF``, including band k-points.  Host orchestration only."""
import time
import warnings
import numpy as np
import torch
from . import gto
from ._common import partition_grid_by_atom, _monkhorst_pack_size


class KPointMixin:
    # ---- k-points (BASELINE configs[3]); DESIGN.md "k-points" -----------------------------------------
    def _get_k_exact_kpts(self, dm=None, mo_coeff=None, mo_occ=None, kpts_band=None, rows=None, max_rows=None):
        """The reference's exact k-point exchange on the device (pyscf/pbc/df/fft_jk.py:250-292; isdf_get_k_exact_kpt): one
        complex FFT pair per (AO at k1, occupied orbital at k2) for every (k1, k2) - the yardstick the k-point ISDF exchange is
        measured against.  Occupied orbitals from mo_coeff / mo_occ (per k-point, fft_jk.py:206-210) or from the eigenvectors of
        Hermitian positive semidefinite density matrices.  rows = (i0, ni): only the AO rows i0..i0+ni of K (a sample, for
        sizes where all rows take too long).  Returns vk (nband, nao or ni, nao) complex128."""
        cell, be = self.cell, self.backend
        kpts = np.asarray(self.kpts, dtype=float).reshape(-1, 3)
        band = kpts if kpts_band is None else np.asarray(kpts_band, dtype=float).reshape(-1, 3)
        nk, nao = len(kpts), cell.nao_nr()
        mesh = np.asarray(self.mesh, dtype=np.int32)
        G = int(np.prod(mesh))
        a = np.asarray(cell.lattice_vectors(), dtype=float)
        if mo_coeff is None:
            mo_coeff, mo_occ = getattr(dm, 'mo_coeff', None), getattr(dm, 'mo_occ', None)
        orbs = []
        for k in range(nk):
            if mo_coeff is not None:
                orbs.append(self._orbitals_from_tag(mo_coeff[k], mo_occ[k]))
            else:
                orbs.append(self._orbitals_from_psd(np.asarray(dm).reshape(-1, nao, nao)[k]))
                if orbs[-1] is None:
                    raise ValueError('get_k_exact needs occupied orbitals or positive semidefinite density matrices')
        i0, ni = (0, nao) if rows is None else (int(rows[0]), int(rows[1]))
        rcut = gto.estimate_rcut_per_shell(cell)
        Ls = gto.get_lattice_Ls(cell, rcut=rcut.max())
        ao_args = (np.asarray(cell._atm), np.asarray(cell._bas), np.asarray(cell._env), Ls, rcut)
        coords_soa = be.to_device(np.ascontiguousarray(self.grids.coords.T))
        u = be.empty((2, nao, G))
        m2 = []
        for k in range(nk):                                     # occupied orbitals at k2 as periodic parts: m2 = C^T u
            be.eval_ao_k(*ao_args, kpts[k], True, coords_soa, u[0], u[1])
            m = be.empty((2, orbs[k].shape[1], G))
            self._orbitals_on_grid(u[0], u[1], orbs[k], m[0], m[1])
            m2.append(m)
        nocc_max = max(m.shape[1] for m in m2)
        if max_rows is None:
            max_rows = max(nocc_max, min(int((6 << 30) // (16 * G)), 65535) // nocc_max * nocc_max)
        weight = cell.vol / G / nk
        out = np.zeros((len(band), ni, nao), dtype=np.complex128)
        coulG = be.empty((G,))
        for b, kb in enumerate(band):
            be.eval_ao_k(*ao_args, kb, True, coords_soa, u[0], u[1])
            vr, vi = be.zeros((ni, nao)), be.zeros((ni, nao))
            for k2 in range(nk):
                be.coulG_q(mesh, a, kpts[k2] - kb, out=coulG)
                be.get_k_exact_kpt(u[0], u[1], m2[k2][0], m2[k2][1], mesh, coulG, weight, i0, ni, max_rows, vr, vi)
            out[b] = be.to_host(vr) + 1j * be.to_host(vi)
        return out

    def _kocc_eligible(self):
        """pair_space='occ' at k-points: the (AO x occupied) pair space is fitted for select 'local' / 'refined' on one process
        with the Cholesky fit route, without robust_k and without a kpts_symm.KPoints input; everything else keeps the Bloch
        AO pairs."""
        return (self.pair_space == 'occ' and self.select in ('local', 'refined') and self.comm.size == 1
                and not getattr(self.comm, 'always', False) and not self.robust_k and not self.bj_auto_kpts
                and self.kpts_symm is None and self.fit_route in ('auto', 'cholesky'))

    def _build_kpts(self):
        """Periodic parts u^k of all Bloch AOs -> real points/Theta (complex-mode S2/S3) -> one complex
        W^q per difference vector q = k2 - k1.  The q list is split over the ranks (each rank holds the
        fit, builds its share of the W^q and later the K terms that use them).  pair_space='occ' (_kocc_eligible): the build
        stops after the density-independent per-atom candidates; get_jk makes the final pick, the fit and the W^q for the
        occupied orbitals of its density (_ensure_fit_kpts)."""
        from . import pbc_tools
        cell, be, comm = self.cell, self.backend, self.comm
        self.timings = {}
        occ_pairs = self._kocc_eligible()
        if self.pair_space == 'occ' and not occ_pairs:
            warnings.warn("ISDF: pair_space='occ' at k-points needs select 'local' or 'refined', one process, the Cholesky fit "
                          "route and no robust_k or kpts_symm; the k-point build interpolates the Bloch AO pairs")
        t0 = time.perf_counter()
        kpts_scf = np.asarray(self.kpts, dtype=float).reshape(-1, 3)
        # band k-points (kpts_band of get_jk) join the stack: the fit must also represent conj(u^{kb}) u^{k}
        band = kpts_scf if self.kpts_band is None else np.asarray(self.kpts_band, dtype=float).reshape(-1, 3)
        kall = [k for k in kpts_scf]
        self._band_index = []
        for kb in band:
            hit = [i for i, k in enumerate(kall) if abs(k - kb).max() < 1e-9]
            if hit:
                self._band_index.append(hit[0])
            else:
                kall.append(kb)
                self._band_index.append(len(kall) - 1)
        kpts = np.array(kall)
        self._kstack = kpts.copy()           # k-vectors of the stacked periodic parts (SCF k-points, then extra band k-points)
        nk = len(kpts)                       # size of the stack; the first len(kpts_scf) entries carry density
        mesh = np.asarray(self.mesh, dtype=np.int32)
        G = int(np.prod(mesh))
        nao = cell.nao_nr()
        nh = nk * nao
        coords = self.grids.coords
        rcut = gto.estimate_rcut_per_shell(cell)
        Ls = gto.get_lattice_Ls(cell, rcut=rcut.max())
        ao_args = (np.asarray(cell._atm), np.asarray(cell._bas), np.asarray(cell._env), Ls, rcut)
        t0 = self._tick('host_setup', t0)

        coords_soa = be.to_device(np.ascontiguousarray(coords.T))
        X = self._buffer('aok', (2 * nh, G))
        for k in range(nk):
            be.eval_ao_k(*ao_args, kpts[k], True, coords_soa, X[k * nao:(k + 1) * nao], X[nh + k * nao:nh + (k + 1) * nao])
        del coords_soa
        self.ao = X
        t0 = self._tick('S1_eval_ao', t0)

        # S2 selection (complex mode); the number of points scales with the number of distinct pair
        # families: c_isdf * nao * kfac by default (capped by the grid)
        kfac = self.k_ip_factor or min(nk, 2)
        P_target = int(min(self.c_isdf * nao * kfac, G))
        sel = dict(P_target=P_target, kpts_scf=kpts_scf, band=band, kpts=kpts, nao=nao, nh=nh)
        if self.select == 'global':
            theta = self._buffer('theta', (P_target, G))
            piv = be.empty((1, P_target), dtype=torch.int64)
            rank = be.select_ip_cplx(X, nh, [0, G], [P_target], self.select_tol, self.tie_rtol, theta, piv)
            sel['ip'] = be.to_host(piv[0, :int(rank[0])].contiguous()).astype(np.int64)
            sel['rank'] = rank
        else:
            owner, perm, counts, blk_off, nip_final, nip = self._voronoi_budget(kfac)
            kmax = int(nip.max())
            Xs = be.empty((2 * nh, G))
            be.gather_cols(X, be.to_device(perm), Xs)
            L = be.empty((kmax, G))
            piv = be.empty((cell.natm, kmax), dtype=torch.int64)
            rank = be.select_ip_cplx(Xs, nh, blk_off, nip, self.select_tol, self.tie_rtol, L, piv)
            del Xs, L
            piv_h = be.to_host(piv)
            sel.update(owner=owner, nip_final=nip_final, rank=rank,
                       per_atom=[perm[blk_off[b] + piv_h[b, :rank[b]]] for b in range(cell.natm)])
        self._ksel = sel
        self._built = True
        self._k_built = kpts_scf.copy()
        self._band_built = None if self.kpts_band is None else band.copy()
        self._nk_stack = nk
        if occ_pairs:
            # the final pick ('refined'), the fit and the W^q need the occupied orbitals: made by get_jk (_ensure_fit_kpts)
            self._tick('S2_select_candidates' if self.select == 'refined' else 'S2_select_ip', t0)
            self._fit_pending = True
            return self
        self._kpts_pick_and_fit(None, t0)
        return self

    def _kpts_pick_and_fit(self, orbs, t0=None):
        """S2 second stage + S3 + S4 + S5 of the k-point build from the selection in self._ksel.  orbs None: the Bloch AO pairs;
        else, per SCF k-point, the (N, nocc_k) complex coefficients C sqrt(occ) of the density's occupied orbitals: the
        (AO x occupied) pair space conj(u^{k1}_mu) psi~^{k2}_j, psi~^k = sum_nu u^k_nu C^k_nu,j."""
        from . import pbc_tools
        cell, be, comm = self.cell, self.backend, self.comm
        if t0 is None:
            t0 = time.perf_counter()
        sel = self._ksel
        X = self.ao
        P_target, kpts_scf, band, kpts, nao, nh = (sel[k] for k in ('P_target', 'kpts_scf', 'band', 'kpts', 'nao', 'nh'))
        nk = len(kpts)
        coords = self.grids.coords
        G = X.shape[1]
        self._W_omega = {}
        Psi = psiP = None
        if orbs is not None:
            # psi~ on the grid, stacked like the periodic parts: rows [Re psi~ (all k, all j); Im psi~]
            nocc_k = [c.shape[1] for c in orbs]
            npsi_h = int(sum(nocc_k))
            Psi = self._buffer('psik', (2 * npsi_h, G))
            o = 0
            for k, c in enumerate(orbs):
                if c.shape[1]:
                    self._orbitals_on_grid(X[k * nao:(k + 1) * nao], X[nh + k * nao:nh + (k + 1) * nao], c,
                                           Psi[o:o + c.shape[1]], Psi[npsi_h + o:npsi_h + o + c.shape[1]])
                o += c.shape[1]
            t0 = self._tick('S2_occupied_on_grid', t0)
        if self.select == 'global':
            self.ip = sel['ip']
            ip_dev = be.to_device(self.ip)
        else:
            rank = sel['rank']
            clusters = self._bj_clusters()
            per_atom = sel['per_atom']
            if self.select == 'refined':
                owner = sel['owner']
                cand = np.concatenate(per_atom).astype(np.int64)
                aoC = be.empty((len(cand), 2 * nh))
                d_cand = be.to_device(cand)
                be.gather_aoP(X, d_cand, aoC)
                psiC = None
                if Psi is not None:
                    psiC = be.empty((len(cand), Psi.shape[0]))
                    be.gather_aoP(Psi, d_cand, psiC)
                chosen = self._refine_pick(aoC, cand, int(sel['nip_final'].sum()), nh=nh, psiC=psiC)
                del aoC, psiC
                own = owner[chosen]
                per_atom = [chosen[own == b] for b in range(cell.natm)]
                rank = np.array([len(x) for x in per_atom], dtype=np.int32)
            self.ip = np.concatenate([per_atom[b] for cl in clusters for b in cl]).astype(np.int64)
            ip_dev = be.to_device(self.ip)
        P = len(self.ip)
        t0 = self._tick('S2_select_ip', t0)

        # S3 global fit, forward solve only (Y); the factor is applied to the (P, P) matrices
        Y = self._buffer('theta', (max(P, P_target), G))[:P]
        aoP_X = self._buffer('aoP', (P, 2 * nh))
        # q list: W^{-q} = conj(W^q) (Theta is real, coulG_{-q}[-G] = coulG_q[G]): build one of each +-q pair,
        # the primaries dealt round-robin over the ranks
        self._qs, self._qindex = pbc_tools.unique_q(kpts_scf, band)      # index[k1 in band][k2 in kpts]
        nq = len(self._qs)
        mesh = np.asarray(self.mesh, dtype=np.int32)
        batch = self.fft_batch or max(1, min(P, int((4 << 30) // (8 * G)) // 256 * 256 or int((4 << 30) // (8 * G)) // 128 * 128 or 64))   # 256-row multiples: the 256x128 GEMM tile
        partner = -np.ones(nq, dtype=int)
        for iq in range(nq):
            for jq in range(nq):
                if abs(self._qs[iq] + self._qs[jq]).max() < 1e-9:
                    partner[iq] = jq
        pair_q = self.kpt_pair_q
        if pair_q not in ('auto', 'uncorrected', True, False):
            raise ValueError("kpt_pair_q must be 'auto', 'uncorrected', True or False")
        if not pair_q:
            # every W^q from its OWN kernel table (twice the products)
            partner[:] = -1
        # the pairing W^{-q} = conj(W^q) assumes coulG_{-q}(G) = coulG_q(-G) index by index, which the Nyquist index of an even mesh
        # breaks (index n/2 is labelled -n/2 for both signs of q, and the wrap-around rule of pbc.py:272-302 zeroes it for one sign
        # only): 'auto' / True add the missing Nyquist-plane terms (_nyquist_pair_correction), 'uncorrected' is round 2's behaviour
        self._pair_correct = pair_q in ('auto', True) and any(int(n) % 2 == 0 for n in mesh)
        primary = [iq for iq in range(nq) if partner[iq] < 0 or partner[iq] >= iq]
        self._q_owner = np.zeros(nq, dtype=int)
        for n, iq in enumerate(primary):
            self._q_owner[iq] = n % comm.size
            if partner[iq] >= 0:
                self._q_owner[partner[iq]] = n % comm.size
        r_ip = coords[self.ip]

        # S3 + S4 + S5, route by route.  'auto' means the Cholesky route here unless bj_auto_kpts is set; then: block-
        # Jacobi, verified on W^{q=0}, Cholesky when the check fails (the fit is replicated, so every rank takes the
        # agreed decision after its share of the q list)
        routes = self._fit_routes() if self.select != 'global' else ['cholesky']
        if (self.fit_route == 'auto' and not self.bj_auto_kpts) or self._want_theta or Psi is not None:
            routes = ['cholesky']
        for route in routes:
            if route == 'blockjacobi':
                ip_off = self._bj_blocks(rank, clusters)
                Afac, Dblk = self._bj_prepare(X, nh, ip_dev, ip_off, aoP_X)
                self._bj_rows(aoP_X, X, G, Dblk, ip_off, Y, nh=nh)
            elif Psi is not None:
                # (AO x occupied) pairs: A_PP = Re[S_u conj(S_psi)] at the points, the rows B likewise, Y = L^-1 B
                chol = self._buffer('factor', (P, P))
                be.gather_aoP(X, ip_dev, aoP_X)
                psiP = be.empty((P, Psi.shape[0]))
                be.gather_aoP(Psi, ip_dev, psiP)
                be.gram_prod_cplx(aoP_X, nh, psiP, Psi.shape[0] // 2, chol)
                be.shift_diag(chol, self.reg_rel)
                self.reg_used = self.reg_rel + be.chol_inplace(chol, 0.0, scratch=self._buffer('Wre', (P, P)))
                be.pair_prod_rows_cplx(aoP_X, nh, psiP, Psi.shape[0] // 2, X, Psi, G, Y)
                be.factor_solve_half(chol, False, Y)
                if self._want_theta:
                    be.factor_solve_half(chol, True, Y)
                del psiP
            else:
                chol = self._buffer('factor', (P, P))
                self.reg_used = be.fit_prepare_cplx(X, nh, ip_dev, self.reg_rel, aoP_X, chol)
                be.fit_apply_cplx(chol, aoP_X, nh, X, G, Y, forward_only=not self._want_theta)
            t0 = self._tick('S3_fit', t0)
            self._kfit_state = dict(route=route, Y=Y, primary=primary, partner=partner, r_ip=r_ip, batch=batch, nao=nao, nh=nh, aoP_X=aoP_X,
                                    chol=None if route == 'blockjacobi' else chol,
                                    bj=(Afac, Dblk, ip_off) if route == 'blockjacobi' else None)
            self._kfit_state['spec'] = self._kspectral_prepare(Y)
            if self._kfit_state['spec'] is not None:
                t0 = self._tick('S4_spectral_rows', t0)
            self._Wq, check, t0 = self._build_Wq(None, t0, probe=(route == 'blockjacobi' and self.fit_route == 'auto'))
            self.fit_route_used = route
            if route == 'blockjacobi' and self.fit_route == 'auto':
                self.bj_check = comm.agree_max(check)
                if self.bj_check <= self.bj_check_tol:
                    break
                warnings.warn('ISDF: block-Jacobi fit route failed its probe check (mismatch %.2e > %.2e); '
                              'rebuilding the W^q with the Cholesky route' % (self.bj_check, self.bj_check_tol))
                t0 = self._tick('S4S5_coulomb_W', t0)

        # Bloch AOs at the points: phi^k(r_P) = exp(i k.r_P) u^k(r_P), (P, nao) complex per k
        uP = be.to_host(aoP_X)                                   # (P, 2 nh)
        self._aoP_k = []
        for k in range(nk):
            u = uP[:, k * nao:(k + 1) * nao] + 1j * uP[:, nh + k * nao:nh + (k + 1) * nao]
            self._aoP_k.append(be.to_device(np.ascontiguousarray(u * np.exp(1j * r_ip.dot(kpts[k]))[:, None])))
        self._q_partner = partner
        t0 = self._tick('S4S5_coulomb_W', t0)
        return self

    # ---- pair_space='occ' at k-points: the fit follows the density ------------------------------------------------
    @staticmethod
    def _orbitals_from_tag(mo_coeff, mo_occ):
        """(N, nocc) coefficients C sqrt(occ) of the occupied orbitals of one k-point (pyscf/pbc/df/fft_jk.py:206-210)."""
        occ = np.asarray(mo_occ, dtype=float)
        return np.asarray(mo_coeff)[:, occ > 0] * np.sqrt(occ[occ > 0])

    @staticmethod
    def _orbitals_from_psd(d):
        """(N, r) orbitals u sqrt(ev) of a Hermitian positive semidefinite matrix from its eigenvectors; None when it is not
        positive semidefinite."""
        ev, u = np.linalg.eigh(0.5 * (d + d.conj().T))
        if ev.min() < -1e-10 * abs(ev).max():
            return None
        keep = ev > 1e-12 * ev.max()
        return u[:, keep] * np.sqrt(ev[keep])

    def _orbitals_on_grid(self, ur, ui, orb, out_re, out_im):
        """psi~ = C^T u^k on the grid (periodic parts of the orbitals orb (N, nocc) complex): the real and imaginary planes
        (nocc, G) from those of u^k, four real products."""
        be = self.backend
        c = np.ascontiguousarray(orb.T)                 # (nocc, nao)
        cr, ci = be.to_device(np.ascontiguousarray(c.real)), be.to_device(np.ascontiguousarray(c.imag))
        be.gemm_nn(cr, ur, out_re)
        be.gemm_nn(ci, ui, out_re, alpha=-1.0, beta=1.0)
        be.gemm_nn(cr, ui, out_im)
        be.gemm_nn(ci, ur, out_im, alpha=1.0, beta=1.0)

    def _kpoint_occupied(self, dm, nk):
        """Per SCF k-point, the (N, nocc_k) complex coefficients C sqrt(occ) of the density get_jk was called with: from its
        per-k-point mo_coeff / mo_occ tag (shaped (nk, N, nmo) / (nk, nmo), or with a leading nset axis), else from the
        eigenvectors of Hermitian positive semidefinite density matrices (nk, N, N) or (nset, nk, N, N).  Several sets (the
        spins of a KUHF density): their orbitals side by side, as at the Gamma point.  None when the density has no such form
        (a response or difference density, or rank > N/2 at some k-point): the Bloch AO pairs are fitted then."""
        nao = self.cell.nao_nr()
        mo_coeff, mo_occ = getattr(dm, 'mo_coeff', None), getattr(dm, 'mo_occ', None)
        cols = [[] for _ in range(nk)]
        if mo_coeff is not None and mo_occ is not None:
            sets = [(mo_coeff, mo_occ)] if np.ndim(mo_occ[0]) == 1 else list(zip(mo_coeff, mo_occ))
            for cs, os_ in sets:
                if len(cs) != nk or len(os_) != nk:
                    return None
                for k in range(nk):
                    cols[k].append(self._orbitals_from_tag(cs[k], os_[k]))
        else:
            dms = np.asarray(dm).reshape(-1, nk, nao, nao)
            for s in range(dms.shape[0]):
                for k in range(nk):
                    d = dms[s, k]
                    if abs(d - d.conj().T).max() > 1e-10 * max(abs(d).max(), 1e-300):
                        return None
                    c = self._orbitals_from_psd(d)
                    if c is None:
                        return None
                    cols[k].append(c)
        out = [np.ascontiguousarray(np.hstack(c), dtype=np.complex128) for c in cols]
        if sum(c.shape[1] for c in out) == 0 or any(c.shape[1] > nao // 2 for c in out):
            return None
        return out

    def _ensure_fit_kpts(self, dm=None):
        """pair_space='occ' at k-points (_kocc_eligible): make sure the fit suits what is about to be contracted with the W^q,
        as isdf.ISDF._ensure_fit does at the Gamma point.  dm with an occupied-orbital form: the (AO x occupied) pair space of
        THAT density - refit when its occupied space differs from the fitted one (occ_refit='always') or keep the first such
        fit ('once').  dm None (get_ao_eri / ao2mo) or a density without such a form: the Bloch AO pairs."""
        if getattr(self, '_ksel', None) is None or not self._kocc_eligible():
            return
        nk = len(self._ksel['kpts_scf'])
        orbs = None if dm is None else self._kpoint_occupied(dm, nk)
        want = None if orbs is None else np.array([c.dot(c.conj().T) for c in orbs])
        if not self._fit_pending:
            have = self._fit_dm
            if want is None:
                if have is None:
                    return                                            # the AO-pair fit is in place
            elif have is None:
                if self.occ_refit == 'once':
                    return                                            # an AO-pair fit came first and is kept
            elif self.occ_refit == 'once' or abs(want - have).max() <= 1e-12 * abs(want).max():
                return
        self._fit_dm = want
        self._kpts_pick_and_fit(orbs)
        self._fit_pending = False

    def _keep_Wq(self, Wc):
        """A finished W^q stays on the device while there is room for the rest of the build and for get_jk's work areas (about
        ten P x P matrices); beyond that it moves to pinned host memory and is uploaded when the K loop reaches its q (3.4 GB
        per matrix at configs[3], where the 27 matrices of the 2x2x2 mesh, Theta and the stacked periodic parts exceed 288 GB)."""
        be = self.backend
        P = Wc.shape[0]
        if not Wc.is_cuda or be.free_bytes() > 10 * 16 * P * P + (8 << 30):
            return Wc
        host = torch.empty(Wc.shape, dtype=Wc.dtype, pin_memory=True)
        host.copy_(Wc)
        return host

    def _build_Wq(self, omega, t0, probe=False):
        """S4 + S5 for this rank's share of the q list from the fit held in self._kfit_state: {iq: W^q (P, P) complex}.
        omega: range separation of the kernel (pyscf/pbc/tools/pbc.py:408-418) - the fit does not depend on it."""
        cell, be, comm = self.cell, self.backend, self.comm
        st = self._kfit_state
        Y, r_ip = st['Y'], st['r_ip']
        P, G = Y.shape
        mesh = np.asarray(self.mesh, dtype=np.int32)
        w = cell.vol / G
        spec = st.get('spec')
        Wre = self._buffer('Wre', (P, P))
        Wim = self._buffer('Wim', (P, P))
        out, check = {}, 0.0
        for iq in st['primary']:
            if self._q_owner[iq] != comm.rank:
                continue
            q = self._qs[iq]
            coulG = be.coulG_q(mesh, cell.lattice_vectors(), q, omega=omega)
            if spec is not None:
                self._kspectral_Mq(spec, coulG, Wre, Wim)
            else:
                be.coulomb_Wq(Y, mesh, coulG, w, 0, P, st['batch'], Wre, Wim, upper_only=True)
                be.symmetrize_hermitian(Wre, Wim)
            jq = int(st['partner'][iq])
            twin = None
            if spec is not None:
                # no packed point on a Nyquist plane (any sphere): coulG_{-q}(G) = coulG_q(-G) on every point, the twin is the plain
                # conjugate (taken where it is used, _jk_from_Wq).  The whole box of an even mesh: the twin from its OWN tables
                if self._pair_correct and jq >= 0 and jq != iq and not spec['pair_exact']:
                    twin = (be.empty((P, P)), be.empty((P, P)))
                    self._kspectral_Mq(spec, be.coulG_q(mesh, cell.lattice_vectors(), -np.asarray(q), omega=omega), twin[0], twin[1])
            elif self._pair_correct and jq >= 0 and jq != iq:
                # M^{-q} = conj(M^q) + the Nyquist-plane terms the pairing misses on an even mesh; finished like M^q below
                twin = (be.empty((P, P)), be.empty((P, P)))
                twin[0].copy_(Wre)
                twin[1].copy_(Wim)
                twin[1].neg_()
                self._nyquist_pair_correction(q, omega, coulG, twin[0], twin[1])
            if st['route'] == 'blockjacobi':
                Afac, Dblk, ip_off = st['bj']
                self._bj_finish(Afac, Dblk, ip_off, Wre)
                self._bj_finish(Afac, Dblk, ip_off, Wim, antisymmetric=True)
                if probe and abs(q).max() < 1e-9:
                    # W^0 is real: the Gamma-point probe check with the densities sum_k u^k* R u^k
                    t1 = self._tick('S4S5_coulomb_W', t0)
                    nao, nh, aoP_X = st['nao'], st['nh'], st['aoP_X']
                    planes = [aoP_X[:, o:o + nao].T.contiguous() for o in range(0, 2 * nh, nao)]
                    check = self._bj_probe_mismatch(planes, Afac, Dblk, ip_off, Y, G, None, W=Wre)
                    del planes
                    t0 = self._tick('S5_route_check', t1)
            elif not self._want_theta:
                be.W_from_factor(st['chol'], 0, Wre)
                be.W_from_factor(st['chol'], 0, Wim)
            Wc = be.empty((P, P), dtype=torch.complex128)
            be.finish_Wq(Wre, Wim, be.to_device(np.exp(-1j * r_ip.dot(q))), Wc)
            out[iq] = self._keep_Wq(Wc)
            del Wc
            if twin is not None:
                if st['route'] == 'blockjacobi':
                    self._bj_finish(Afac, Dblk, ip_off, twin[0])
                    self._bj_finish(Afac, Dblk, ip_off, twin[1], antisymmetric=True)
                elif not self._want_theta:
                    be.W_from_factor(st['chol'], 0, twin[0])
                    be.W_from_factor(st['chol'], 0, twin[1])
                Wt = be.empty((P, P), dtype=torch.complex128)
                be.finish_Wq(twin[0], twin[1], be.to_device(np.exp(1j * r_ip.dot(q))), Wt)      # phases of -q
                out[jq] = self._keep_Wq(Wt)
                del twin, Wt
        return out, check, t0

    # ---- kpt_w_spectral: every M^q from one packed half spectrum of the fit rows --------------------------------------------------
    def _kspectral_prepare(self, Y):
        """X (P, ldx) = the half spectra of the real fit rows Y on the packed points (fit_route._spectral_point_set: sphere,
        multiplicities, shell order; unit scale, consecutive (Re, Im) pairs, zero padded), made ONCE per fit: the rows do not depend
        on q, so every M^q - of this build and of later kernels on the kept fit - is two table-scaled products over X
        (_kspectral_Mq), without any transform.  None (the classic build) when kpt_w_spectral is off, the plane FFT does not cover
        the mesh, or w_sphere='auto' refuses the sphere.  Records the form in w_spectral_fraction."""
        self.w_spectral_fraction = None
        if self.kpt_w_spectral is False:
            return None
        if self.kpt_w_spectral is not True:
            raise ValueError('kpt_w_spectral must be True or False')
        be = self.backend
        mesh = np.asarray(self.mesh, dtype=np.int32)
        nbat = int(self.fft_batch or 512)
        if not be.spectral_supported(mesh, nbat):
            return None
        n0, n1, n2 = (int(x) for x in mesh)
        pts = self._spectral_point_set(mesh, np.ones((n0, n1, n2 // 2 + 1), dtype=bool), self._ksphere_share)
        if pts is None:
            return None
        idx = pts[0]
        P, G = Y.shape
        npts = len(idx)
        ldx = -(-2 * npts // 128) * 128
        # the +-q pairing is exact when no packed point lies on the Nyquist plane of an even axis
        i2 = idx % (n2 // 2 + 1)
        i1 = (idx // (n2 // 2 + 1)) % n1
        i0 = idx // ((n2 // 2 + 1) * n1)
        on_nyq = np.zeros(npts, dtype=bool)
        for i, n in ((i0, n0), (i1, n1), (i2, n2)):
            if n % 2 == 0:
                on_nyq |= (i == n // 2)
        d_idx = be.to_device(idx)
        X = self._buffer('kspecX', (P, ldx))
        be.spectral_rows(Y, mesh, d_idx, be.to_device(np.ones(npts)), X, batch=nbat, **self._spectral_lines_kw(idx, np.ones(npts), mesh))
        self.w_spectral_fraction = 2.0 * npts / G
        return dict(X=X, idx=d_idx, npts=npts, ldx=ldx, pair_exact=not on_nyq.any(), strip=nbat,
                    s=self._buffer('kspec_s', (ldx,)), a=self._buffer('kspec_a', (ldx,)))

    def _ksphere_share(self, pct, mult, box, keep):
        """The guard of w_sphere='auto' at k-points: fit_route._sphere_energy_share on the rows of self.ao, here the stacked
        periodic-part planes (Re and Im of every u^k), with the plain q = 0 kernel table.  Measured once per mesh.  A table with
        negative entries (a truncated or attenuated kernel left active in the backend) gives no energy share: the guard refuses."""
        mesh = np.asarray(self.mesh, dtype=np.int32)
        key = ('kpts', tuple(int(x) for x in mesh), round(float(pct), 6))
        if getattr(self, '_sphere_share', (None,))[0] != key:
            cg = self.backend.coulG_half(mesh, np.asarray(self.cell.lattice_vectors(), dtype=float))
            share = np.inf if (cg < 0).any() else \
                self._sphere_energy_share(mesh, cg, mult, box, keep, self.cell.vol / int(np.prod(mesh)))
            self._sphere_share = (key, share)
        return self._sphere_share[1]

    def _kspectral_Mq(self, spec, coulG, Mre, Mim):
        """Mre + i Mim <- M^q = (w / G) sum_G c_q(G) Y^_P(G) conj(Y^_Q(G)) over the packed points, folded onto the half spectrum:
            Re M = sum_j ts_j (Re Re + Im Im)_j,  Im M = sum_j ta_j (Im Re - Re Im)_j,  ts/ta_j = (w / G) [c_q(G_j) +- (m_j - 1) c_q(-G_j)],
        one pass per strip of rows over X for both planes (isdf_herm_kscale_nt), block-upper part, mirrored at the end."""
        be = self.backend
        X = spec['X']
        P = X.shape[0]
        mesh = np.asarray(self.mesh, dtype=np.int32)
        G = int(np.prod(mesh))
        be.pack_table_pm(coulG, mesh, spec['idx'], self.cell.vol / G / G, spec['s'], spec['a'])
        nb = spec['strip']
        for b0 in range(0, P, nb):
            b1 = min(P, b0 + nb)
            be.herm_kscale_nt(X[b0:b1], X[b0:], spec['s'], spec['a'], Mre[b0:b1, b0:], Mim[b0:b1, b0:])
        be.symmetrize_hermitian(Mre, Mim)

    def _nyquist_planes(self):
        """For every even mesh axis: the DFT of the fit rows on that axis' Nyquist plane (P x plane entries, real and imaginary
        planes), the flat grid index of each plane entry and of its index-negated image, and the mask of the entries an earlier
        axis' plane has not counted already.  Made once per build (the rows do not depend on q)."""
        st = self._kfit_state
        if st.get('nyq') is not None:
            return st['nyq']
        be = self.backend
        Y = st['Y']
        P, G = Y.shape
        n = [int(x) for x in self.mesh]
        ii = [np.arange(m) for m in n]
        out = []
        for ax in range(3):
            if n[ax] % 2:
                continue
            oth = [i for i in range(3) if i != ax]
            A, B = np.meshgrid(ii[oth[0]], ii[oth[1]], indexing='ij')
            idx3 = [None, None, None]
            idx3[ax] = np.full(A.shape, n[ax] // 2)
            idx3[oth[0]], idx3[oth[1]] = A, B
            flat = ((idx3[0] * n[1] + idx3[1]) * n[2] + idx3[2]).ravel()
            neg = ((((-idx3[0]) % n[0]) * n[1] + ((-idx3[1]) % n[1])) * n[2] + ((-idx3[2]) % n[2])).ravel()
            fresh = np.ones(flat.shape, dtype=bool)
            for prev in range(ax):
                if n[prev] % 2 == 0:
                    fresh &= (idx3[prev].ravel() != n[prev] // 2)
            npl = len(flat)
            Tr, Ti = be.empty((P, npl)), be.empty((P, npl))
            nb = max(1, min(P, 65535, int((1 << 30) // (16 * npl))))
            for r0 in range(0, P, nb):
                r1 = min(P, r0 + nb)
                be.nyquist_spectra(Y[r0:r1], np.asarray(n, dtype=np.int32), ax, Tr[r0:r1], Ti[r0:r1])
            out.append(dict(Tr=Tr, Ti=Ti, flat=be.to_device(flat.astype(np.int64)), neg=be.to_device(neg.astype(np.int64)),
                            fresh=be.to_device(fresh.astype(np.float64))))
        st['nyq'] = out
        return out

    def _nyquist_pair_correction(self, q, omega, tab_q, Mre, Mim):
        """(Mre + i Mim) += M^{-q} - conj(M^q) = w/G sum_{G on the Nyquist planes} [coulG_{-q}(G) - coulG_q(-G)] Y^_P(G) conj(Y^_Q(G)):
        what W^{-q} = conj(W^q) leaves out on an even mesh.  3/n of the grid: a few per cent of a full product."""
        cell, be = self.cell, self.backend
        mesh = np.asarray(self.mesh, dtype=np.int32)
        G = int(np.prod(mesh))
        w = cell.vol / G
        tab_m = be.coulG_q(mesh, cell.lattice_vectors(), -np.asarray(q), omega=omega)
        for pl in self._nyquist_planes():
            d = ((tab_m[pl['flat']] - tab_q[pl['neg']]) * pl['fresh']).contiguous()
            Tr, Ti = pl['Tr'], pl['Ti']
            # sum_G d T_P conj(T_Q): Re = Tr d Tr^T + Ti d Ti^T, Im = Ti d Tr^T - Tr d Ti^T     (the 1/G of the Parseval sum: alpha)
            # the correction is Hermitian like M itself: block-upper part only (512-row blocks), mirrored once at the end
            P = Tr.shape[0]
            for r0 in range(0, P, 512):
                r1 = min(P, r0 + 512)
                be.gemm_nt(Tr[r0:r1], Tr[r0:], Mre[r0:r1, r0:], alpha=w / G, beta=1.0, kscale=d)
                be.gemm_nt(Ti[r0:r1], Ti[r0:], Mre[r0:r1, r0:], alpha=w / G, beta=1.0, kscale=d)
                be.gemm_nt(Ti[r0:r1], Tr[r0:], Mim[r0:r1, r0:], alpha=w / G, beta=1.0, kscale=d)
                be.gemm_nt(Tr[r0:r1], Ti[r0:], Mim[r0:r1, r0:], alpha=-w / G, beta=1.0, kscale=d)
        be.symmetrize_hermitian(Mre, Mim)
        del tab_m

    def _get_jk_kpts(self, dm, hermi, kpts, kpts_band, with_j, with_k, exxdiv, omega=None):
        """k-point J and K (pyscf/pbc/df/fft_jk.py:33-109,177-302 semantics).  dm (nk, N, N) or (nset, nk, N, N); with
        kpts_band the result lives on the band k-points, (nband, N, N) [(N, N) for a single (3,) band vector], as
        df_jk._format_jks shapes it (pyscf/pbc/df/df_jk.py:1426-1444)."""
        ex = exxdiv if exxdiv is not None else self.exxdiv
        if ex not in (None, 'None', 'ewald', 'vcut_sph', 'vcut_ws'):
            raise NotImplementedError("k-point ISDF: exxdiv None, 'ewald', 'vcut_sph' and 'vcut_ws' are implemented")
        if omega and ex in ('ewald', 'vcut_sph', 'vcut_ws'):
            raise NotImplementedError('range-separated J/K: only exxdiv=None is implemented')
        cell, be, comm = self.cell, self.backend, self.comm
        kpts = np.asarray(kpts, dtype=float).reshape(-1, 3)
        band_in = None if kpts_band is None else np.asarray(kpts_band, dtype=float)
        band = None if band_in is None else band_in.reshape(-1, 3)

        def same(x, y):
            if x is None or y is None:
                return x is None and y is None
            return x.shape == y.shape and abs(x - y).max() < 1e-9
        if not self._built or getattr(self, '_k_built', None) is None or not same(kpts, self._k_built) \
                or not same(band, getattr(self, '_band_built', None)):
            self.kpts = kpts
            self.kpts_band = band
            self.build()
        if with_k:
            self._ensure_fit_kpts(dm)                            # pair_space='occ': the fit for this density's occupied orbitals
        nk = len(kpts)
        nks = self._nk_stack                                     # k-points in the stacked periodic parts
        bidx = list(range(nk)) if band is None else list(self._band_index)
        nband = len(bidx)
        nao = cell.nao_nr()
        nh = nks * nao
        dm_in = np.asarray(dm)
        dms = np.asarray(dm_in, dtype=np.complex128).reshape(-1, nk, nao, nao)
        nset = dms.shape[0]
        # a non-Hermitian density matrix gives a complex density: J is then built from its real and imaginary parts
        herm_dm = abs(dms - dms.conj().transpose(0, 1, 3, 2)).max() <= 1e-10
        mesh = np.asarray(self.mesh, dtype=np.int32)
        G = int(np.prod(mesh))
        a = np.asarray(cell.lattice_vectors(), dtype=float)
        X = self.ao

        def planes(k):
            return X[k * nao:(k + 1) * nao], X[nh + k * nao:nh + (k + 1) * nao]
        out_shape = dm_in.shape if band is None else \
            (dm_in.shape[:-3] + ((nband,) if band_in.ndim > 1 else ()) + (nao, nao))
        vj = vk = None
        t0 = time.perf_counter()
        Wq_set = self._Wq
        if omega:
            # range separation: same fit, the W^q rebuilt with the attenuated kernel once per omega (until the next build)
            key = round(float(omega), 10)
            if key not in self._W_omega and self._kfit_state is not None:       # (no fit yet: pair_space='occ', J alone)
                self._W_omega[key], _, t0 = self._build_Wq(omega, t0)
                t0 = self._tick('S4S5_coulomb_W_omega', t0)
            Wq_set = self._W_omega.get(key)
            be.set_coulomb_omega(omega)                          # the J kernel table lives on the device
        elif ex == 'vcut_sph' and with_k:
            # exchange with the spherically truncated kernel (pbc.py:312-317, Rc from the nk-fold cell): its own W^q set
            if 'vcut_sph' not in self._W_omega:
                be.set_coulomb_cutoff(self._vcut_sph_radius(nk))
                try:
                    self._W_omega['vcut_sph'], _, t0 = self._build_Wq(None, t0)
                finally:
                    be.set_coulomb_cutoff(0.0)
                t0 = self._tick('S4S5_coulomb_W_variant', t0)
            Wq_set = self._W_omega['vcut_sph']
        elif ex == 'vcut_ws' and with_k:
            # exchange with the Wigner-Seitz truncated kernel (pbc.py:318-346) of the k-mesh's supercell: its own W^q set
            if 'vcut_ws' not in self._W_omega:
                be.set_coulomb_ws(self._ws_kernel(_monkhorst_pack_size(cell, kpts)))
                try:
                    self._W_omega['vcut_ws'], _, t0 = self._build_Wq(None, t0)
                finally:
                    be.set_coulomb_ws(None)
                t0 = self._tick('S4S5_coulomb_W_variant', t0)
            Wq_set = self._W_omega['vcut_ws']
        try:
            vj, vk = self._jk_from_Wq(Wq_set, dms, nk, bidx, planes, out_shape, with_j, with_k, ex, herm_dm, kpts, t0)
        finally:
            if omega:
                be.set_coulomb_omega(0.0)
        return vj, vk

    def _jk_from_Wq(self, Wq_set, dms, nk, bidx, planes, out_shape, with_j, with_k, ex, herm_dm, kpts, t0):
        cell, be, comm = self.cell, self.backend, self.comm
        nset, nband, nao = dms.shape[0], len(bidx), cell.nao_nr()
        mesh = np.asarray(self.mesh, dtype=np.int32)
        G = int(np.prod(mesh))
        a = np.asarray(cell.lattice_vectors(), dtype=float)
        vj = vk = None
        if with_j:
            vj = np.zeros((nset, nband, nao, nao), dtype=np.complex128)
            for s in range(nset):
                # rho = 1/nk sum_k sum_ij D_ij u_i conj(u_j); isdf_rho_k gives Re(rho); Im(rho) = Re of the same with -i D
                for part, fac in ((0, 1.0), (1, -1j)):
                    if part == 1 and herm_dm:
                        break
                    rho = be.zeros((1, G))
                    for k in range(nk):
                        dT = (fac * dms[s, k]).T
                        be.rho_k(*planes(k), G, be.to_device(np.ascontiguousarray(dT.real)),
                                 be.to_device(np.ascontiguousarray(dT.imag)), 1.0 / nk, rho)
                    be.coulomb_potential(rho, mesh, a)
                    for ib, kb in enumerate(bidx):
                        vre = be.empty((nao, nao))
                        vim = be.empty((nao, nao))
                        be.vj_k(*planes(kb), G, rho, vre, vim)
                        vj[s, ib] += (1.0 if part == 0 else 1j) * (be.to_host(vre) + 1j * be.to_host(vim))
            t0 = self._tick('S6_get_j', t0)
            vj = vj.reshape(out_shape)
        if with_k:
            d_vk = be.zeros((nset, nband, nao, nao), dtype=torch.complex128)
            # the (k1, k2) pairs grouped by their difference vector: a W^q that lives in host memory is uploaded once per group
            groups = {}
            for i1, k1 in enumerate(bidx):
                for k2 in range(nk):
                    iq = int(self._qindex[i1, k2])
                    if self._q_owner[iq] == comm.rank:
                        groups.setdefault(iq, []).append((i1, k1, k2))
            for s in range(nset):
                d_dm = [be.to_device(np.ascontiguousarray(dms[s, k])) for k in range(nk)]
                for iq, pairs in groups.items():
                    if iq in Wq_set:
                        Wq = Wq_set[iq]
                        if not Wq.is_cuda:
                            Wq = Wq.to(be.device, non_blocking=True)
                    else:                          # stored as its time-reversal partner: W^{-q} = conj(W^q) ('uncorrected' / odd meshes)
                        Wp = Wq_set[self._q_partner[iq]]
                        Wq = torch.conj_physical(Wp if Wp.is_cuda else Wp.to(be.device, non_blocking=True))
                    for i1, k1, k2 in pairs:
                        be.get_k_pair(self._aoP_k[k1], self._aoP_k[k2], d_dm[k2], Wq, 1.0 / nk, d_vk[s, i1])
                    del Wq
            if comm.size > 1 or getattr(comm, 'always', False):
                flat = torch.view_as_real(d_vk)
                comm.all_reduce_sum(flat)
            vk = be.to_host(d_vk)
            if self.robust_k:
                if Wq_set is not self._Wq or ex in ('vcut_sph', 'vcut_ws'):
                    raise NotImplementedError('robust_k at k-points: plain kernel only (exxdiv None or ewald, no omega)')
                if not herm_dm:
                    raise NotImplementedError('robust_k at k-points needs Hermitian density matrices')
                vk = self._robust_k_kpts(dms, vk, bidx, kpts, self._nk_stack)
            if ex == 'ewald':
                # vk[k] += madelung * S^k D^k S^k (pyscf/pbc/df/df_jk.py:1446-1465) for the band k-points that are
                # k-points of the density; S^k by quadrature on the grid from the periodic parts (the phases cancel)
                mad = gto.madelung(cell, _monkhorst_pack_size(cell, kpts))
                w_const = be.to_device(np.full((1, G), cell.vol / G))
                for ib, kb in enumerate(bidx):
                    if kb >= nk:
                        continue
                    sre, sim = be.empty((nao, nao)), be.empty((nao, nao))
                    be.vj_k(*planes(kb), G, w_const, sre, sim)
                    Sk = be.to_host(sre) + 1j * be.to_host(sim)
                    for s in range(nset):
                        vk[s, ib] += mad * Sk.dot(dms[s, kb]).dot(Sk)
            t0 = self._tick('S7_get_k', t0)
            vk = vk.reshape(out_shape)
        return vj, vk

    def _robust_k_kpts(self, dms, vk_isdf, bidx, kpts, nks):
        """K <- K1 + K1^H - K_isdf at k-points (Dunlap's robust form; Hermitian density matrices):
            K1^{k1}_{pq} = w/nk sum_{k2} sum_P conj(u1_p(r_P)) sum_g V^q_P(g) [u2_P D^{k2} conj(u2(g))] u1_q(g),   q = k2 - k1,
        V^q_P = conv_q(Theta_P) recomputed per call, batch of points by batch (keeping it for all q would take nq x 16 P G bytes:
        2.9 TB at configs[3]); per (k1, k2) and batch two complex (batch, N, G) products on the real / imaginary planes
        (isdf_gemm_nn, isdf_zhadamard_planes, isdf_gemm_nt).  Cost 16 nk^2 P N G flop per K: a small-cell, high-accuracy path.
        Single process."""
        cell, be, comm = self.cell, self.backend, self.comm
        if comm.size > 1:
            raise NotImplementedError('robust_k at k-points is a single-process path')
        st = self._kfit_state
        theta, aoP_X, nao, nh = st['Y'], st['aoP_X'], st['nao'], st['nh']     # Theta itself (build with robust_k: both solves)
        P, G = theta.shape
        nk = len(kpts)
        nset, nband = vk_isdf.shape[0], len(bidx)
        mesh = np.asarray(self.mesh, dtype=np.int32)
        a = np.asarray(cell.lattice_vectors(), dtype=float)
        w = cell.vol / G
        X = self.ao

        def planes(k):
            return X[k * nao:(k + 1) * nao], X[nh + k * nao:nh + (k + 1) * nao]
        uP = be.to_host(aoP_X)                                                 # periodic parts at the points, (P, 2 nh)
        uPk = [uP[:, k * nao:(k + 1) * nao] + 1j * uP[:, nh + k * nao:nh + (k + 1) * nao] for k in range(nks)]
        band_vec = [self._kstack[b] for b in bidx]
        nb = max(1, min(P, int((3 << 30) // (16 * G))))
        Vr, Vi = be.empty((nb, G)), be.empty((nb, G))
        Fr, Fi = be.empty((nb, G)), be.empty((nb, G))
        Kr, Ki = be.empty((nb, nao)), be.empty((nb, nao))
        coulG = be.empty((G,))
        out = vk_isdf.reshape(nset, nband, nao, nao).copy()
        k1acc = np.zeros((nset, nband, nao, nao), dtype=np.complex128)
        for i1, b1 in enumerate(bidx):
            u1r, u1i = planes(b1)
            for k2 in range(nk):
                be.coulG_q(mesh, a, kpts[k2] - band_vec[i1], out=coulG)
                u2r, u2i = planes(k2)
                for r0 in range(0, P, nb):
                    r1 = min(P, r0 + nb)
                    n = r1 - r0
                    be.coulomb_rows_q(theta[r0:r1], mesh, coulG, Vr[:n], Vi[:n])
                    for s in range(nset):
                        T = uPk[k2][r0:r1].dot(dms[s, k2])                    # (n, N) complex: u2_P D
                        Tr, Ti = be.to_device(np.ascontiguousarray(T.real)), be.to_device(np.ascontiguousarray(T.imag))
                        # F = T conj(u2) = (Tr u2r + Ti u2i) + i (Ti u2r - Tr u2i)
                        be.gemm_nn(Tr, u2r, Fr[:n])
                        be.gemm_nn(Ti, u2i, Fr[:n], beta=1.0)
                        be.gemm_nn(Ti, u2r, Fi[:n])
                        be.gemm_nn(Tr, u2i, Fi[:n], alpha=-1.0, beta=1.0)
                        be.zhadamard_planes(Fr[:n], Fi[:n], Vr[:n], Vi[:n])   # F <- V o F
                        # (V o F) u1^T = (Fr u1r^T - Fi u1i^T) + i (Fr u1i^T + Fi u1r^T)
                        be.gemm_nt(Fr[:n], u1r, Kr[:n])
                        be.gemm_nt(Fi[:n], u1i, Kr[:n], alpha=-1.0, beta=1.0)
                        be.gemm_nt(Fr[:n], u1i, Ki[:n])
                        be.gemm_nt(Fi[:n], u1r, Ki[:n], beta=1.0)
                        Kt = be.to_host(Kr[:n]) + 1j * be.to_host(Ki[:n])
                        k1acc[s, i1] += uPk[b1][r0:r1].conj().T.dot(Kt)
        k1acc *= w / nk
        out = k1acc + k1acc.conj().transpose(0, 1, 3, 2) - out
        return out.reshape(vk_isdf.shape)

    def _get_ao_eri_kpts(self, kpts, mo_coeffs=None):
        """(i^{k1} j^{k2} | k^{k3} l^{k4}) = sum_PQ conj(phi^{k1}_i) phi^{k2}_j (P)  W^{q}_PQ  conj(phi^{k3}_k) phi^{k4}_l (Q),
        q = k2 - k1 = k3 - k4, as FFTDF.get_ao_eri (pyscf/pbc/df/fft_ao2mo.py:45-99) returns it: complex (nao^2, nao^2), s1.
        kpts: one k-point (all four equal) or four with k1 - k2 + k3 - k4 = 0.  Small systems (host contraction).
        mo_coeffs (four (nao, n_i) arrays): the same in the MO basis, phi^{k}_i -> sum_mu phi^{k}_mu C_mu,i
        (FFTDF.ao2mo / get_mo_eri, fft_ao2mo.py:101-152)."""
        be = self.backend
        kk = np.asarray(kpts, dtype=float).reshape(-1, 3)
        if len(kk) == 1:
            kk = np.tile(kk, (4, 1))
        if len(kk) != 4:
            raise ValueError('get_ao_eri needs one or four k-points')
        if abs(kk[0] - kk[1] + kk[2] - kk[3]).max() > 1e-7:
            raise ValueError('k-points do not conserve momentum (k1 - k2 + k3 - k4 != 0)')
        if self.comm.size > 1:
            raise NotImplementedError('k-point ERIs are a single-process path')
        uniq, idx = [], []
        for k in kk:
            hit = [i for i, u in enumerate(uniq) if abs(u - k).max() < 1e-7]
            if hit:
                idx.append(hit[0])
            else:
                uniq.append(k)
                idx.append(len(uniq) - 1)
        uniq = np.array(uniq)
        built = getattr(self, '_k_built', None)
        if not self._built or built is None or built.shape != uniq.shape or abs(built - uniq).max() > 1e-9 \
                or getattr(self, '_band_built', None) is not None:
            self.kpts = uniq
            self.kpts_band = None
            self.build()                     # through build(): drops the state (range-separated W^q included) of the old k-point set
        self._ensure_fit_kpts()              # pair_space='occ': integrals come from the Bloch AO pairs
        iq = self._qindex[idx[0], idx[1]]
        Wq = self._Wq[iq] if iq in self._Wq else torch.conj_physical(self._Wq[self._q_partner[iq]])
        Wq = be.to_host(Wq)
        a = [be.to_host(self._aoP_k[i]) for i in idx]
        if mo_coeffs is not None:
            a = [x.dot(np.asarray(c)) for x, c in zip(a, mo_coeffs)]
        P = len(self.ip)
        left = (a[0].conj()[:, :, None] * a[1][:, None, :]).reshape(P, -1)
        right = (a[2].conj()[:, :, None] * a[3][:, None, :]).reshape(P, -1)
        return left.T.dot(Wq).dot(right)

