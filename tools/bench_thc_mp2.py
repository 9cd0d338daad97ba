"""Times of the THC opposite-spin MP2 (ISDF.mp2_os).  Per workload: the build, then mp2_os twice (the first run allocates A, B and
the library's workspaces) with the host clock around a device synchronise, then once more under the library's kernel profile: seconds
per quadrature point, TF/s of the pair kernel and of the W A product from the profiler's flop labels, ngrid.  Orbitals: 'scf' = a
Gamma-point RHF on the object itself (tools/scf_demo.py's path: T and S by plane-wave quadrature of the collocation, get_pp, get_jk),
'random' = the benchmark's random orthogonal orbitals with synthetic orbital energies (occupied in [-0.8, -0.2], virtual in
[0.2, 3.2] Eh: only ngrid depends on them).  Needs an MI355X.
    python tools/bench_thc_mp2.py [workload:c_isdf:scf|random ...] > profiles/NAME.log
    (default: diamond-222-dzvp-80:10:scf diamond-444-dzvp-120:12:random)"""
import os
import sys
import time
import numpy as np
import scipy.linalg
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyscf_isdf_amd import workloads
from pyscf_isdf_amd.isdf import ISDF



def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def scf_orbitals(df):
    cell = df.cell
    nao, nocc = cell.nao_nr(), cell.nelectron // 2
    mesh = np.asarray(cell.mesh)
    G = int(np.prod(mesh))
    F = np.fft.fftn(df.backend.to_host(df.ao).reshape(nao, *mesh), axes=(1, 2, 3)).reshape(nao, G)
    b = 2 * np.pi * np.linalg.inv(cell.lattice_vectors().T)
    fr = [np.fft.fftfreq(n, 1. / n) for n in mesh]
    Gv = (fr[0][:, None, None, None] * b[0] + fr[1][None, :, None, None] * b[1] + fr[2][None, None, :, None] * b[2]).reshape(-1, 3)
    T = 0.5 * cell.vol / G ** 2 * (F.conj() * np.einsum('gi,gi->g', Gv, Gv)).dot(F.T).real
    S = cell.vol / G ** 2 * F.conj().dot(F.T).real
    del F
    hcore = T + df.get_pp()
    e, c = scipy.linalg.eigh(hcore, S)
    focks, errs, e_last = [], [], 0.0
    for it in range(40):
        dm = 2 * c[:, :nocc].dot(c[:, :nocc].T)
        vj, vk = df.get_jk(dm)
        f = hcore + vj - 0.5 * vk
        e_el = 0.5 * np.einsum('ij,ji', hcore + f, dm)
        err = f.dot(dm).dot(S) - S.dot(dm).dot(f)
        if abs(e_el - e_last) < 1e-9 and abs(err).max() < 1e-6:
            break
        e_last = e_el
        focks, errs = (focks + [f])[-8:], (errs + [err])[-8:]
        n = len(focks)
        if n > 1:
            B = -np.ones((n + 1, n + 1))
            B[n, n] = 0
            for i in range(n):
                for j in range(n):
                    B[i, j] = np.vdot(errs[i], errs[j])
            rhs = np.zeros(n + 1)
            rhs[n] = -1
            f = sum(ci * fi for ci, fi in zip(np.linalg.lstsq(B, rhs, rcond=None)[0][:n], focks))
        e, c = scipy.linalg.eigh(f, S)
    e, c = scipy.linalg.eigh(hcore + vj - 0.5 * vk, S)
    occ = np.zeros(nao)
    occ[:nocc] = 2
    print('  RHF: %d iterations, E_el %.10f Eh, gap %.4f Eh, orbital energies %.3f .. %.3f' % (it + 1, e_el, e[nocc] - e[nocc - 1], e[0], e[-1]),
          flush=True)
    return c, e, occ


def random_orbitals(cell):
    _, c, occ = workloads.make_dm(cell)
    nocc = int((occ > 0).sum())
    e = np.concatenate([np.linspace(-0.8, -0.2, nocc), np.linspace(0.2, 3.2, len(occ) - nocc)])
    return c, e, occ


def run(name, c_isdf, orbitals):
    cell = workloads.make_cell(name)
    df = ISDF(cell, c_isdf=c_isdf)
    t_build, _ = wall(df.build)
    P, nao = len(df.ip), cell.nao_nr()
    print('\n%s: natm %d, nao %d, G %d, c_isdf %d, P %d, route %s, build %.2f s' %
          (name, cell.natm, nao, int(np.prod(cell.mesh)), c_isdf, P, df.fit_route_used, t_build), flush=True)
    c, e, occ = scf_orbitals(df) if orbitals == 'scf' else random_orbitals(cell)
    print('  orbitals: %s; no %d, nv %d' % (orbitals, int((occ > 0).sum()), int((occ == 0).sum())), flush=True)
    be = df.backend
    for rep in range(2):
        t, res = wall(lambda: df.mp2_os(c, e, occ))
        print('  mp2_os run %d: %.3f s in all, %.4f s per quadrature point (loop %.3f s), ngrid %d, rtol %g, e_os %.10f Eh, e_sos %.10f Eh' %
              (rep, t, res.seconds / res.ngrid, res.seconds, res.ngrid, res.rtol, res.e_os, res.e_sos), flush=True)
    be.prof_reset()
    be.prof_enable(True)
    res = df.mp2_os(c, e, occ)
    be.synchronize()
    prof = be.prof_results()
    be.prof_enable(False)
    for k in sorted(prof, key=lambda k: -prof[k]['ms'])[:6]:
        p = prof[k]
        rate = p['work'] / max(p['ms'], 1e-9) * 1e-6
        print('    kernel %-36s %6d launches %10.2f ms  %8.2f %s' % (k, p['launches'], p['ms'], rate * (1e-3 if k.endswith('[flop]') else 1.0),
                                                                    'TF/s' if k.endswith('[flop]') else 'GB/s'), flush=True)
    df.reset()
    del df
    torch.cuda.empty_cache()


if __name__ == '__main__':          # tools/bench_thc_rpa.py imports the orbitals from here
    print('device', torch.cuda.get_device_name(0), 'CUs', torch.cuda.get_device_properties(0).multi_processor_count, flush=True)
    print('a new capability: there is no parent-commit time to compare with', flush=True)
    for arg in sys.argv[1:] or ['diamond-222-dzvp-80:10:scf', 'diamond-444-dzvp-120:12:random']:
        parts = arg.split(':')
        run(parts[0], int(parts[1]) if len(parts) > 1 else 10, parts[2] if len(parts) > 2 else 'scf')
