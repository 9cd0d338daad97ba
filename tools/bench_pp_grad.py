"""Times of the pseudopotential and Hartree forces per term: pp_nuc_grad through its stage ticks (host clock around a device
synchronise) and the library's kernel profile, then get_j_nuc_grad against get_j_e1 plus the host contraction of
pyscf/pbc/grad/krhf.py:64 on the same object, alternating.  Needs an MI355X.
    python tools/bench_pp_grad.py [workload ...] > profiles/NAME.log      (default: diamond-222-dzvp-80 diamond-444-dzvp-120)"""
import os
import sys
import time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyscf_isdf_amd import workloads
from pyscf_isdf_amd.isdf import ISDF

print('device', torch.cuda.get_device_name(0), 'CUs', torch.cuda.get_device_properties(0).multi_processor_count, flush=True)


def stat(x):
    x = np.sort(np.array(x))
    return 'median %9.2f ms (min %9.2f max %9.2f, n=%d)' % (np.median(x), x[0], x[-1], len(x))


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), out


for name in sys.argv[1:] or ['diamond-222-dzvp-80', 'diamond-444-dzvp-120']:
    cell = workloads.make_cell(name)
    dm = workloads.make_dm(cell)[0]
    nao, G = cell.nao_nr(), int(np.prod(cell.mesh))
    df = ISDF(cell)
    be = df.backend
    print('\n%s: natm %d, nao %d, G %d, e1_grid_chunk %d' % (name, cell.natm, nao, G, df.e1_grid_chunk), flush=True)
    df.pp_nuc_grad(dm)                                            # warm: workspaces, FFT plan, rocBLAS
    reps = 3
    ticks, total = {}, []
    for r in range(reps):
        df.timings = {}
        t, g = wall(lambda: df.pp_nuc_grad(dm))
        total.append(t)
        for k, v in df.timings.items():
            ticks.setdefault(k, []).append(1e3 * v)
    print('  pp_nuc_grad               %s   max|grad| %.3e, sum over atoms %.1e' % (stat(total), abs(g).max(), abs(g.sum(axis=0)).max()))
    for k in ('S8_nuc_grad_local', 'S8_pp_grad_local_hf', 'S8_pp_grad_nonlocal'):
        print('    %-23s %s' % (k, stat(ticks[k])))
    be.prof_reset()
    be.prof_enable(True)
    df.pp_nuc_grad(dm)
    be.synchronize()
    prof = be.prof_results()
    be.prof_enable(False)
    for k in sorted(prof, key=lambda k: -prof[k]['ms']):
        p = prof[k]
        rate = p['work'] / max(p['ms'], 1e-9) * 1e-6
        print('    kernel %-34s %6d launches %9.2f ms  %8.1f %s' % (k, p['launches'], p['ms'], rate * (1e-3 if k.endswith('[flop]') else 1.0),
                                                                  'TF/s' if k.endswith('[flop]') else 'GB/s'))
    df.get_pp_ip1()
    print('  get_pp_ip1 (3, nao, nao)  %9.2f ms (one call, warm)' % wall(lambda: df.get_pp_ip1())[0], flush=True)

    # the Hartree force: contracted route against the matrix route, alternating
    aosl = np.asarray(cell.aoslice_by_atom())[:, -2:]

    def matrix_route():
        e1 = df.get_j_e1(dm)
        return np.array([2 * np.einsum('xmn,nm->x', e1[:, p0:p1], dm[:, p0:p1]) for p0, p1 in aosl])

    fa, fb = df.get_j_nuc_grad(dm), matrix_route()
    print('  get_j_nuc_grad vs contraction of get_j_e1: max rel diff %.2e' % (abs(fa - fb).max() / abs(fb).max()))
    ta, tb = [], []
    for r in range(reps):
        ta.append(wall(lambda: df.get_j_nuc_grad(dm))[0])
        tb.append(wall(matrix_route)[0])
    print('  get_j_nuc_grad                        %s' % stat(ta))
    print('  get_j_e1 + host contraction           %s' % stat(tb), flush=True)
    df.reset()
    del df
    torch.cuda.empty_cache()
