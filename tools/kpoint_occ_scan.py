"""Scan c_isdf for the k-point ISDF exchange with Bloch AO pairs (pair_space='ao') against (AO x occupied) pairs
(pair_space='occ'), for SCF orbitals: KRKS 'lda,' on the diamond primitive cell (gth-szv, 19^3) converged with the multigrid
J/XC ladder, the density tagged per k-point with the orbitals of the final Fock matrix.  Reports, per c and pair space, the
number of points, max|dK| and |dE_K| against get_k_exact, and the build + get_jk seconds (build and fit included: for
pair_space='occ' the fit is made by get_jk).

    python tools/kpoint_occ_scan.py [--kmesh 2,1,1] [--c 2,3,4,5,6] [--combine P,nh,npsi_h,ng]

--combine also times isdf_pair_prod_rows_cplx at one shape (random operands) and prints the bytes its combine pass moves,
for the kernel's share of HBM peak under rocprofv3 --kernel-trace --stats."""
import argparse
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import scipy.linalg

ap = argparse.ArgumentParser()
ap.add_argument('--kmesh', default='2,1,1')
ap.add_argument('--c', default='2,3,4,5,6')
ap.add_argument('--combine', default=None)
args = ap.parse_args()

from pyscf_isdf_amd import gto, multigrid as pmg
from pyscf_isdf_amd.isdf import ISDF
from pyscf_isdf_amd._common import tag_array
import scf_helpers

if args.combine:
    import torch
    from pyscf_isdf_amd.backend import HipBackend
    P, nh, npsi_h, ng = (int(x) for x in args.combine.split(','))
    be = HipBackend(0)
    g = torch.Generator(device=be.device).manual_seed(1)
    X = torch.randn((2 * nh, ng), dtype=torch.float64, device=be.device, generator=g)
    Psi = torch.randn((2 * npsi_h, ng), dtype=torch.float64, device=be.device, generator=g)
    aoP = torch.randn((P, 2 * nh), dtype=torch.float64, device=be.device, generator=g)
    psiP = torch.randn((P, 2 * npsi_h), dtype=torch.float64, device=be.device, generator=g)
    B = be.empty((P, ng))
    for rep in range(4):
        be.synchronize()
        t0 = time.perf_counter()
        be.pair_prod_rows_cplx(aoP, nh, psiP, npsi_h, X, Psi, ng, B)
        be.synchronize()
        dt = time.perf_counter() - t0
    gemm = 2.0 * 2 * P * ng * (2 * nh + 2 * npsi_h)
    print('pair_prod_rows_cplx P=%d nh=%d npsi_h=%d ng=%d: %.3f s (GEMMs %.2f TFLOP; combine pass moves %.2f GB = 5 x 8 B x P x ng)'
          % (P, nh, npsi_h, ng, dt, gemm / 1e12, 40.0 * P * ng / 1e9), flush=True)
    del X, Psi, aoP, psiP, B
    be.empty_cache()

cell = gto.Cell(unit='B', atom='C 0. 0. 0.; C 1.68506879 1.68506879 1.68506879',
                a=[[0., 3.37013758, 3.37013758], [3.37013758, 0., 3.37013758], [3.37013758, 3.37013758, 0.]],
                basis='gth-szv', pseudo='gth-pade', mesh=[19] * 3)
kpts = cell.make_kpts([int(x) for x in args.kmesh.split(',')])
nk, nao, nocc = len(kpts), cell.nao_nr(), cell.nelectron // 2
t0 = time.perf_counter()
S, T = scf_helpers.overlap_kinetic_from_ft_kpts(cell, kpts)
mg = pmg.MultiGridFFTDF(cell, kpts=kpts)
mg.split = 'all'
hcore = T + np.asarray(mg.get_pp(kpts))


def veff(dms):
    n, exc, v = pmg.nr_rks(mg, 'lda,', dms, kpts=kpts, with_j=True)
    return np.asarray(v), float(v.ecoul), float(exc)


e_tot, dms = scf_helpers.krks(hcore, S, veff, nocc, scf_helpers.ewald_energy(cell))
f = hcore + veff(dms)[0]
mo = np.array([scipy.linalg.eigh(f[k], S[k])[1] for k in range(nk)])
occ = np.zeros((nk, nao))
occ[:, :nocc] = 2.0
dms = np.einsum('kpi,ki,kqi->kpq', mo, occ, mo.conj())
tagged = tag_array(dms, mo_coeff=mo, mo_occ=occ)
print('diamond primitive, gth-szv, 19^3, k-mesh %s: KRKS lda, e_tot = %.10f (%.1f s)' % (args.kmesh, e_tot, time.perf_counter() - t0),
      flush=True)

k_ex = None
print('%4s %4s %6s %11s %11s %9s' % ('c', 'pair', 'P', 'max|dK|', '|dE_K|', 'seconds'), flush=True)
for c in [int(x) for x in args.c.split(',')]:
    for space in ('ao', 'occ'):
        df = ISDF(cell, kpts=kpts, c_isdf=c, select='refined')
        df.pair_space = space
        df.backend.synchronize()
        t0 = time.perf_counter()
        df.build()
        vk = df.get_jk(tagged, kpts=kpts, with_j=False)[1]
        df.backend.synchronize()
        dt = time.perf_counter() - t0
        if k_ex is None:
            k_ex = df.get_k_exact(tagged)
        dk = vk - k_ex
        de = abs(np.einsum('kij,kji', dms, dk).real) / (4 * nk)
        print('%4d %4s %6d %11.3e %11.3e %9.3f' % (c, space, len(df.ip), abs(dk).max(), de, dt), flush=True)
        del df
