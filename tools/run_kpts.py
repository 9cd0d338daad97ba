"""Developer helper: k-point ISDF build + get_jk on one workload, per-stage wall times.

    python tools/run_kpts.py [workload] [reps] [--spectral]     (--spectral: kpt_w_spectral=True with w_sphere='auto';
                                                                 --kernels: the library's per-kernel table of the last iteration)
"""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from pyscf_isdf_amd import workloads
from pyscf_isdf_amd.isdf import ISDF

spectral = '--spectral' in sys.argv
kernels = '--kernels' in sys.argv
argv = [x for x in sys.argv if x not in ('--spectral', '--kernels')]
name = argv[1] if len(argv) > 1 else 'mgo-222-dzvp-k222'
reps = int(argv[2]) if len(argv) > 2 else 1
cell = workloads.make_cell(name)
kpts = workloads.make_kpts(name, cell)
nk, nao = len(kpts), cell.nao_nr()
rng = np.random.default_rng(20240203)
dms = []
for k in range(nk):
    c = np.linalg.qr(rng.standard_normal((nao, nao)) + 1j * rng.standard_normal((nao, nao)))[0]
    occ = np.zeros(nao); occ[:cell.nelectron // 2] = 2
    dms.append((c * occ).dot(c.conj().T))
dms = np.array(dms)
print(name, 'natm', cell.natm, 'nao', nao, 'mesh', cell.mesh, 'nk', nk, flush=True)
df = ISDF(cell, kpts=kpts, c_isdf=10, select='local')
df.kpt_w_spectral = spectral
for it in range(reps):
    if kernels and it == reps - 1:
        df.backend.prof_enable(True)
        df.backend.prof_reset()
    t0 = time.perf_counter()
    df.build()
    vj, vk = df.get_jk(dms, kpts=kpts)
    df.backend.synchronize()
    print('iter %d total %.3f s  P=%d  nq=%d (built %d)  W^q form: %s' % (it, time.perf_counter() - t0, len(df.ip), len(df._qs), len(df._Wq),
          'classic' if df.w_spectral_fraction is None else 'spectral, 2 npts / G = %.3f' % df.w_spectral_fraction))
    for k, v in df.timings.items():
        print('   %-18s %8.3f s' % (k, v))
    print('   EJ %.10f  EK %.10f  herm(K) %.2e' % (np.einsum('kij,kji', vj, dms).real / 2 / nk, np.einsum('kij,kji', vk, dms).real / 4 / nk,
                                                  abs(vk - vk.conj().transpose(0, 2, 1)).max()), flush=True)
if kernels:
    for k, v in sorted(df.backend.prof_results().items(), key=lambda kv: -kv[1]['ms']):
        unit = 'TF/s' if k.endswith('[flop]') else 'GB/s'
        rate = v['work'] / max(v['ms'], 1e-9) / (1e9 if unit == 'TF/s' else 1e6)
        print('   %-44s %6d launches %10.1f ms  %8.1f %s' % (k, v['launches'], v['ms'], rate, unit))
