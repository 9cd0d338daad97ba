"""isdf_gemm_nt_had3 (one launch) against the composition (hadamard_rows + three gemm_nt) on the shapes of get_k_e1, and
get_k_e1 against the robust K of get_jk on one build, alternating the variants in one process; device events around each
kernel-level call, the S7 / S8 ticks (host clock around a device synchronise) for the product.  Needs an MI355X.
    python tools/bench_e1_had3.py > profiles/NAME.log"""
import os
import sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyscf_isdf_amd.backend import HipBackend
from pyscf_isdf_amd import gto
from pyscf_isdf_amd.isdf import ISDF

be = HipBackend(0)
print('device', torch.cuda.get_device_name(0), 'CUs', torch.cuda.get_device_properties(0).multi_processor_count, flush=True)


def ev_time(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def stat(x):
    x = np.sort(np.array(x))
    return 'median %8.3f ms (min %8.3f max %8.3f, n=%d)' % (np.median(x), x[0], x[-1], len(x))


w = 0.37
for M, N, K in ((2048, 208, 65536), (2048, 1024, 65536), (4096, 2048, 32768), (1664, 208, 64000)):
    g = torch.Generator(device='cuda').manual_seed(M + N + K)
    A = torch.randn((M, K), device='cuda', dtype=torch.float64, generator=g)
    H = 1.0 + 0.01 * torch.randn((M, K), device='cuda', dtype=torch.float64, generator=g)
    B3 = torch.randn((3, N, K), device='cuda', dtype=torch.float64, generator=g)
    Tf, Tc, Ty = be.zeros((3, M, N)), be.zeros((3, M, N)), be.zeros((M, N))
    F = A.clone()

    def fused():
        be.gemm_nt_had3(A, H, B3, Tf, alpha=w, beta=1.0)

    def comp():
        be.hadamard_rows(F, H)
        for x in range(3):
            be.gemm_nt(F, B3[x], Tc[x], alpha=w, beta=1.0)

    def yard():                       # the inner product of one batch of _robust_k_correction: F .*= V, F ao^T
        be.hadamard_rows(F, H)
        be.gemm_nt(F, B3[0], Ty, alpha=w)

    # same numbers first (beta = 0 from the same inputs)
    be.gemm_nt_had3(A, H, B3, Tf, alpha=w, beta=0.0)
    be.hadamard_rows(F, H)
    for x in range(3):
        be.gemm_nt(F, B3[x], Tc[x], alpha=w, beta=0.0)
    diff = float((Tf - Tc).abs().max() / Tc.abs().max())
    F.copy_(A)
    for fn in (fused, comp, yard, fused, comp, yard):
        fn()
    torch.cuda.synchronize()
    reps = 12
    tf, tc, ty = [], [], []
    for r in range(reps):
        tf.append(ev_time(fused))
        tc.append(ev_time(comp))
        ty.append(ev_time(yard))
    flop = 6.0 * M * N * K
    print('M=%d N=%d K=%d: fused vs composition max rel diff %.2e' % (M, N, K, diff))
    print('  fused        %s  %.1f TF/s' % (stat(tf), flop / np.median(tf) * 1e-9))
    print('  composition  %s  %.1f TF/s' % (stat(tc), flop / np.median(tc) * 1e-9))
    print('  yardstick (hadamard + ONE gemm_nt) %s' % stat(ty), flush=True)
    del A, H, B3, Tf, Tc, Ty, F
    torch.cuda.empty_cache()

# ---- the product: robust K of get_jk (S7_get_k) against get_k_e1 (S8_get_k_e1), fused and composed
cell = gto.diamond_supercell(2, 'gth-dzvp', (40, 40, 40))
nao = cell.nao_nr()
rng = np.random.default_rng(5)
c = np.linalg.qr(rng.standard_normal((nao, nao)))[0]
occ = np.zeros(nao)
occ[:cell.nelectron // 2] = 2
dm = (c * occ).dot(c.T)
df = ISDF(cell, c_isdf=8, select='local')
df.robust_k = True
df.build()
print('product: diamond 2x2x2 gth-dzvp, nao %d, G %d, P %d, route %s' % (nao, int(np.prod(cell.mesh)), len(df.ip), df.fit_route_used), flush=True)
df.get_jk(dm, with_j=False)
k1 = df.get_k_e1(dm)
df.e1_fused = False
k0 = df.get_k_e1(dm)
df.e1_fused = True
print('  get_k_e1 fused vs composition max rel diff %.2e' % (abs(k1 - k0).max() / abs(k0).max()))
res = {'S7_get_k': [], 'fused': [], 'composition': []}
for r in range(5):
    df.timings = {}
    df.get_jk(dm, with_j=False)
    res['S7_get_k'].append(1e3 * df.timings['S7_get_k'])
    for name, flag in (('fused', True), ('composition', False)):
        df.timings = {}
        df.e1_fused = flag
        df.get_k_e1(dm)
        res[name].append(1e3 * df.timings['S8_get_k_e1'])
df.e1_fused = True
print('  robust K of get_jk (S7_get_k, the unchanged _robust_k_correction + get_k) %s' % stat(res['S7_get_k']))
print('  get_k_e1 fused       (S8_get_k_e1) %s' % stat(res['fused']))
print('  get_k_e1 composition (S8_get_k_e1) %s' % stat(res['composition']))
nd = dm + 0.1 * rng.standard_normal((nao, nao))
for name, flag in (('fused', True), ('composition', False)):
    df.e1_fused = flag
    df.get_k_e1(nd)
    t = []
    for r in range(3):
        df.timings = {}
        df.get_k_e1(nd)
        t.append(1e3 * df.timings['S8_get_k_e1'])
    print('  non-symmetric D (left = phi_P D^T, full rank) get_k_e1 %-11s %s' % (name, stat(t)))
