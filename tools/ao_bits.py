"""SHA-256 of the AO collocation's outputs, one per output plane: every case of tests/test_gpu_eval_ao_sweep.py (cases, cell and
calls are imported from it, padding included in the hashed planes) and one user-sized case, the first 262 144 grid points of
diamond 4x4x4 / gth-dzvp on the 120^3 mesh through all four entry points.  Run once per tree (--lib PATH loads another build of
the library), each in a process of its own, and compare the two listings line for line: eval_ao.hip is built with
-ffp-contract=off, so the outputs are a function of the source expression trees and a refactor leaves every line as it was.

--time N: instead of the hashes, the user-sized case timed - 3 warm-up calls and N timed calls per entry point, the kernel's
milliseconds from the library's own profiler; prints the median and the extremes per profiling label."""
import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
ap = argparse.ArgumentParser()
ap.add_argument('--lib', default=None, help='libmi355_isdf.so to load instead of the tree\'s own')
ap.add_argument('--time', type=int, default=0, metavar='N', help='time the user-sized case (N calls per entry point) instead of hashing')
args = ap.parse_args()
import pyscf_isdf_amd.lib as isdf_lib
if args.lib:
    isdf_lib.LIB_PATH = os.path.abspath(args.lib)
import numpy as np
import torch
import test_gpu_eval_ao_sweep as sw
from pyscf_isdf_amd import gto
from pyscf_isdf_amd.backend import HipBackend

be = HipBackend(0)
USER_POINTS = 262144


def sha(t):
    return hashlib.sha256(np.ascontiguousarray(be.to_host(t)).tobytes()).hexdigest()


def name_of(entry, kpt, periodic):
    return '%s%s' % (entry, '' if kpt is None else ' kpt=(%g,%g,%g) periodic_part=%d' % (*kpt, periodic))


def sweep_cases():
    cell, Ls, rcut = sw.sweep_cell()
    forms = list(sw.FORMS) + [('eval_ao_k', np.zeros(3), True), ('eval_ao_k_deriv1', np.zeros(3), True)]
    for pts in sw.POINT_SETS:
        for entry, kpt, periodic in forms:
            body, tail = sw.run(be, cell, Ls, rcut, sw.points(pts), entry, kpt, periodic)
            for h in range(body.shape[0]):
                for x in range(body.shape[1]):
                    print('sweep %-12s %-52s %s x=%d  %s' % (pts, name_of(entry, kpt, periodic), 'im' if h else 're', x,
                                                             hashlib.sha256(body[h, x].tobytes() + tail[h, x].tobytes()).hexdigest()), flush=True)


def user_case():
    """(cell, Ls, rcut, device coordinates (3, USER_POINTS), the four calls as (entry, profiling label, shape, call(buf)))."""
    cell = gto.diamond_supercell(4, 'gth-dzvp', (120, 120, 120))
    rcut = gto.estimate_rcut_per_shell(cell)
    Ls = gto.get_lattice_Ls(cell, rcut=rcut.max())
    d_c = be.to_device(np.ascontiguousarray(cell.get_uniform_grids()[:USER_POINTS].T))
    a = (cell._atm, cell._bas, cell._env, Ls, rcut)
    nao, G = cell.nao_nr(), USER_POINTS
    calls = [('eval_ao', 'eval_ao_kernel[byte]', (1, 1, nao, G), lambda b: be.eval_ao(*a, d_c, b[0, 0])),
             ('eval_ao_deriv1', 'eval_ao_deriv1_kernel[byte]', (1, 4, nao, G), lambda b: be.eval_ao_deriv1(*a, d_c, b[0])),
             ('eval_ao_k', 'eval_ao_k_kernel[byte]', (2, 1, nao, G), lambda b: be.eval_ao_k(*a, sw.KPT, True, d_c, b[0, 0], b[1, 0])),
             ('eval_ao_k_deriv1', 'eval_ao_k_deriv1_kernel[byte]', (2, 4, nao, G), lambda b: be.eval_ao_k_deriv1(*a, sw.KPT, True, d_c, b[0], b[1]))]
    return cell, Ls, calls


def user_hashes():
    cell, Ls, calls = user_case()
    print('user case: diamond 4x4x4 gth-dzvp 120^3, first %d points, nao %d, %d images' % (USER_POINTS, cell.nao_nr(), len(Ls)), flush=True)
    for entry, label, shape, call in calls:
        buf = torch.full(shape, sw.SENTINEL, dtype=torch.float64, device=be.device)
        call(buf)
        for h in range(shape[0]):
            for x in range(shape[1]):
                print('user  %-65s %s x=%d  %s' % (name_of(entry, sw.KPT if shape[0] == 2 else None, True), 'im' if h else 're', x, sha(buf[h, x])),
                      flush=True)
        del buf


def user_times(n):
    cell, Ls, calls = user_case()
    be.prof_enable(True)
    for entry, label, shape, call in calls:
        buf = be.empty(shape)
        ms = []
        for it in range(3 + n):
            be.prof_reset()
            call(buf)
            be.synchronize()
            ms.append(be.prof_results()[label]['ms'])
        ms = np.sort(ms[3:])
        print('time  %-32s median %9.4f ms  min %9.4f  max %9.4f  (%d calls after 3 warm-up)' % (label, np.median(ms), ms[0], ms[-1], n), flush=True)
        del buf


if args.time:
    user_times(args.time)
else:
    sweep_cases()
    user_hashes()
