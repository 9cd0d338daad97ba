"""Times of the XC nuclear force ('blyp'): xc_nuc_grad through its stage tick (host clock around a device synchronise) and the
library's kernel profile, then xc_nuc_grad against get_vxc_e1 plus the host contraction 2 sum_(mu in A) sum_nu vxc_e1 D on the same
object, alternating.  Needs an MI355X.
    python tools/bench_xc_grad.py [workload ...] > profiles/NAME.log      (default: diamond-222-dzvp-80 diamond-444-dzvp-120)"""
import os
import sys
import time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyscf_isdf_amd import workloads, xc_grad
from pyscf_isdf_amd import multigrid as pmg

print('device', torch.cuda.get_device_name(0), 'CUs', torch.cuda.get_device_properties(0).multi_processor_count, flush=True)
XC = 'blyp'


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
    dm = 0.5 * (dm + dm.T)
    nao, G = cell.nao_nr(), int(np.prod(cell.mesh))
    df = pmg.MultiGridFFTDF(cell)
    be = df.backend
    df.build_tasks()
    print('\n%s: natm %d, nao %d, G %d, %d levels, chunk of the ten-plane walk %d columns' %
          (name, cell.natm, nao, G, len(df.tasks), xc_grad._walk_chunk(df, nao)), flush=True)
    pmg.xc_nuc_grad(df, XC, dm)                                    # warm: workspaces, FFT plans, rocBLAS
    reps = 3
    total, tick = [], []
    for r in range(reps):
        df.timings = {}
        t, g = wall(lambda: pmg.xc_nuc_grad(df, XC, dm))
        total.append(t)
        tick.append(1e3 * df.timings['S8_xc_nuc_grad'])
    print('  xc_nuc_grad(%r)         %s   max|F| %.3e' % (XC, stat(total), abs(g).max()))
    print('    %-23s %s' % ('S8_xc_nuc_grad', stat(tick)))
    t_pot = [wall(lambda: xc_grad._potentials(df, pmg._functional(XC), False, dm[None], False))[0] for r in range(reps)]
    print('    of which rho, grad rho through the ladder and the functional: %s' % stat(t_pot))
    be.prof_reset()
    be.prof_enable(True)
    pmg.xc_nuc_grad(df, XC, dm)
    be.synchronize()
    prof = be.prof_results()
    be.prof_enable(False)
    for k in sorted(prof, key=lambda k: -prof[k]['ms'])[:12]:
        p = prof[k]
        rate = p['work'] / max(p['ms'], 1e-9) * 1e-6
        print('    kernel %-34s %6d launches %9.2f ms  %8.1f %s' % (k, p['launches'], p['ms'], rate * (1e-3 if k.endswith('[flop]') else 1.0),
                                                                  'TF/s' if k.endswith('[flop]') else 'GB/s'))

    # contracted route against the matrix route, alternating
    aosl = np.asarray(cell.aoslice_by_atom())[:, -2:]

    def matrix_route():
        e1 = pmg.get_vxc_e1(df, XC, dm)
        return np.array([2 * np.einsum('xmn,nm->x', e1[:, p0:p1], dm[:, p0:p1]) for p0, p1 in aosl])

    fa, fb = pmg.xc_nuc_grad(df, XC, dm), matrix_route()
    print('  xc_nuc_grad vs contraction of get_vxc_e1: max rel diff %.2e' % (abs(fa - fb).max() / abs(fb).max()))
    ta, tb = [], []
    for r in range(reps):
        ta.append(wall(lambda: pmg.xc_nuc_grad(df, XC, dm))[0])
        tb.append(wall(matrix_route)[0])
    print('  xc_nuc_grad                           %s' % stat(ta))
    print('  get_vxc_e1 + host contraction         %s' % stat(tb), flush=True)
    df.reset()
    del df
    torch.cuda.empty_cache()
