"""Times of the direct RPA energy from the ISDF factors (ISDF.rpa).  Per workload: the build, then rpa twice (the first run allocates
S, B and the libraries' workspaces) with the host clock around a device synchronise, then once more under the library's kernel
profile: seconds per frequency, the four steps per frequency (S, W S, the traces, the LU) and the TF/s of thc_chi0_kernel from the
profiler's flop labels.  Then the form the kernel replaces, timed in the same process: the pair rows Y[:, (i, a)] = Phi_o[:, i]
Phi_v[:, a] materialised in column chunks (element-wise torch ops) and the library dgemm S += (Y d) Y^T per chunk, with the largest
deviation of its S from the kernel's.  Orbitals as in tools/bench_thc_mp2.py ('scf' or 'random').  Needs an MI355X.
    python tools/bench_thc_rpa.py [workload:c_isdf:scf|random:nw ...] > profiles/NAME.log
    (default: diamond-222-dzvp-80:10:scf:40 diamond-444-dzvp-120:12:random:3)"""
import os
import sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pyscf_isdf_amd import workloads
from pyscf_isdf_amd.isdf import ISDF
from bench_thc_mp2 import scf_orbitals, random_orbitals, wall

print('device', torch.cuda.get_device_name(0), 'CUs', torch.cuda.get_device_properties(0).multi_processor_count, flush=True)
print('a new capability: there is no parent-commit time to compare with; the kernel is compared with the materialised form', flush=True)
args = sys.argv[1:] or ['diamond-222-dzvp-80:10:scf:40', 'diamond-444-dzvp-120:12:random:3']
CHUNK_BYTES = 2 << 30          # of one materialised chunk of pair rows (there are two: Y and Y d)


def materialised(phio, phiv, d, S):
    """S <- sum_ia Y_ia d_ia Y_ia^T with Y stored chunk by chunk (whole occupied orbitals per chunk) and torch's dgemm."""
    P, no = phio.shape
    nv = phiv.shape[1]
    step = max(1, min(no, CHUNK_BYTES // (8 * P * nv)))
    S.zero_()
    for i0 in range(0, no, step):
        i1 = min(no, i0 + step)
        y = (phio[:, i0:i1, None] * phiv[:, None, :]).reshape(P, -1)
        yd = y * d[i0:i1].reshape(1, -1)
        S.addmm_(yd, y.t())
        del y, yd
    return step


def run(name, c_isdf, orbitals, nw):
    cell = workloads.make_cell(name)
    df = ISDF(cell, c_isdf=c_isdf)
    t_build, _ = wall(df.build)
    P, nao = len(df.ip), cell.nao_nr()
    print('\n%s: natm %d, nao %d, G %d, c_isdf %d, P %d, route %s, build %.2f s' %
          (name, cell.natm, nao, int(np.prod(cell.mesh)), c_isdf, P, df.fit_route_used, t_build), flush=True)
    c, e, occ = scf_orbitals(df) if orbitals == 'scf' else random_orbitals(cell)
    no, nv = int((occ > 0).sum()), int((occ == 0).sum())
    print('  orbitals: %s; no %d, nv %d, nw %d' % (orbitals, no, nv, nw), flush=True)
    be = df.backend
    for rep in range(2):
        t, res = wall(lambda: df.rpa(c, e, occ, nw=nw))
        print('  rpa run %d: %.3f s in all, %.4f s per frequency (loop %.3f s), nw %d, e_corr %.10f Eh, e_mp2_direct %.10f Eh' %
              (rep, t, res.seconds / res.nw, res.seconds, res.nw, res.e_corr, res.e_mp2_direct), flush=True)
    be.prof_reset()
    be.prof_enable(True)
    res = df.rpa(c, e, occ, nw=nw)
    be.synchronize()
    prof = be.prof_results()
    be.prof_enable(False)
    for k in sorted(prof, key=lambda k: -prof[k]['ms'])[:7]:
        p = prof[k]
        rate = p['work'] / max(p['ms'], 1e-9) * 1e-6
        print('    kernel %-36s %6d launches %10.2f ms  %9.3f ms per frequency %8.2f %s' %
              (k, p['launches'], p['ms'], p['ms'] / nw, rate * (1e-3 if k.endswith('[flop]') else 1.0),
               'TF/s' if k.endswith('[flop]') else 'GB/s'), flush=True)
    # the kernel against the materialised form, same operands, one frequency (the middle of the grid)
    off = no + (no & 1)
    phi = df._bufs['thc_phi'][:P * (off + nv + (nv & 1))].view(P, -1)
    phio, phiv = phi[:, :no], phi[:, off:off + nv]
    delta = e[occ == 0][None, :] - e[occ > 0][:, None]
    d = be.to_device(4 * delta / (delta ** 2 + res.freqs[nw // 2] ** 2))
    S = df._bufs['thc_A'][:P * P].view(P, P)
    S2 = df._bufs['thc_B'][:P * P].view(P, P)
    flop = P * (P + 1.0) * no * nv
    for rep in range(2):
        tk, _ = wall(lambda: be.thc_chi0(phio, phiv, d, S))
        tm, step = wall(lambda: materialised(phio, phiv, d, S2))
        print('  S(w) run %d: thc_chi0_kernel %.4f s (%.2f TF/s of the triangle)   materialised + dgemm %.4f s (%d occupied per chunk, '
              '%.2f TF/s of the same flop)   ratio %.2f' % (rep, tk, flop / tk * 1e-12, tm, step, flop / tm * 1e-12, tm / tk), flush=True)
    print('  max |S_kernel - S_materialised| / max |S| = %.2e' % (float((S - S2).abs().max()) / float(S.abs().max())), flush=True)
    df.reset()
    del df, S, S2, phi, phio, phiv
    torch.cuda.empty_cache()


for arg in args:
    parts = arg.split(':')
    run(parts[0], int(parts[1]) if len(parts) > 1 else 10, parts[2] if len(parts) > 2 else 'scf', int(parts[3]) if len(parts) > 3 else 40)
