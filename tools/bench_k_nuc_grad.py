"""Times of the contracted exchange force.  Kernel level: isdf_gemm_nn_had (one launch) against isdf_hadamard_rows + isdf_gemm_nn on
the walk's own shapes (M = r, N = 65 536 grid columns, K = a batch of points), device events, alternating.  Product level, per
workload with its benchmark density (symmetric, rank nelec / 2): get_k_nuc_grad fused and composed, get_k_e1 plus the host
contraction on the same object, get_jk_nuc_grad against the two calls; host clock around a device synchronise, warm-up first,
alternating; then the library's kernel profile of one get_k_nuc_grad.  Needs an MI355X.
    python tools/bench_k_nuc_grad.py [workload[:c_isdf] ...] > profiles/NAME.log   (default: diamond-222-dzvp-80:10 diamond-444-dzvp-120:10;
                                                                                  'kernel' alone: the kernel level only)"""
import os
import sys
import time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyscf_isdf_amd import workloads
from pyscf_isdf_amd.backend import HipBackend
from pyscf_isdf_amd.isdf import ISDF

print('device', torch.cuda.get_device_name(0), 'CUs', torch.cuda.get_device_properties(0).multi_processor_count, flush=True)
args = sys.argv[1:] or ['kernel', 'diamond-222-dzvp-80:10', 'diamond-444-dzvp-120:10']


def stat(x):
    x = np.sort(np.array(x))
    return 'median %9.3f ms (min %9.3f max %9.3f, n=%d)' % (np.median(x), x[0], x[-1], len(x))


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), out


def ev_time(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def kernel_level():
    be = HipBackend(0)
    N = 65536
    for M, K in ((32, 2080), (32, 4096), (256, 4096), (702, 4096), (1664, 4096)):
        g = torch.Generator(device='cuda').manual_seed(M + K)
        A = torch.randn((M, K), device='cuda', dtype=torch.float64, generator=g)
        H = 1.0 + 0.01 * torch.randn((K, N), device='cuda', dtype=torch.float64, generator=g)
        B = torch.randn((K, N), device='cuda', dtype=torch.float64, generator=g)
        F = B.clone()
        Zf, Zc = be.zeros((M, N)), be.zeros((M, N))

        def fused():
            be.gemm_nn_had(A, H, B, Zf, alpha=1.0, beta=1.0)

        def comp():                       # as the walk runs it: F is overwritten (refilled by the F product in the walk)
            be.hadamard_rows(F, H)
            be.gemm_nn(A, F, Zc, alpha=1.0, beta=1.0)

        be.gemm_nn_had(A, H, B, Zf, alpha=1.0, beta=0.0)
        be.hadamard_rows(F, H)
        be.gemm_nn(A, F, Zc, alpha=1.0, beta=0.0)
        diff = float((Zf - Zc).abs().max() / Zc.abs().max())
        F.copy_(B)
        for fn in (fused, comp, fused, comp):
            fn()
        torch.cuda.synchronize()
        tf, tc = [], []
        for r in range(12):
            tf.append(ev_time(fused))
            tc.append(ev_time(comp))
        flop = 2.0 * M * N * K
        byt = 8.0 * (2.0 * K * N + 2.0 * M * N)
        print('M=%d N=%d K=%d: fused vs composition max rel diff %.2e' % (M, N, K, diff))
        print('  isdf_gemm_nn_had                     %s  %5.1f TF/s  %6.0f GB/s of H, B, C' % (stat(tf), flop / np.median(tf) * 1e-9, byt / np.median(tf) * 1e-6))
        print('  isdf_hadamard_rows + isdf_gemm_nn    %s  %5.1f TF/s' % (stat(tc), flop / np.median(tc) * 1e-9), flush=True)
        del A, H, B, F, Zf, Zc
        torch.cuda.empty_cache()


def product_level(name, c):
    cell = workloads.make_cell(name)
    dm = workloads.make_dm(cell)[0]
    dm = 0.5 * (dm + dm.T)
    nao, G = cell.nao_nr(), int(np.prod(cell.mesh))
    df = ISDF(cell, c_isdf=c, select='local')
    df.robust_k = True
    t_build, _ = wall(df.build)
    be = df.backend
    aosl = np.asarray(cell.aoslice_by_atom())[:, -2:]
    print('\n%s: natm %d, nao %d, G %d, c_isdf %d, P %d, rank of D %d, robust build %.1f s' %
          (name, cell.natm, nao, G, c, len(df.ip), cell.nelectron // 2, 1e-3 * t_build), flush=True)

    def matrix_route():
        vk = df.get_k_e1(dm)
        return np.array([2 * np.einsum('xmn,nm->x', vk[:, p0:p1], dm[:, p0:p1]) for p0, p1 in aosl])

    def contracted(fused):
        df.k_grad_fused = fused
        try:
            return df.get_k_nuc_grad(dm)
        finally:
            df.k_grad_fused = True

    fa, fc, fb = contracted(True), contracted(False), matrix_route()          # warm: workspaces, rocBLAS
    print('  get_k_nuc_grad vs contraction of get_k_e1: max rel diff %.2e; fused vs composed %.2e; max|f| %.3e' %
          (abs(fa - fb).max() / abs(fb).max(), abs(fa - fc).max() / abs(fa).max(), abs(fa).max()))
    reps = 3
    ta, tc, tb, tick_a, tick_c, tick_b = [], [], [], [], [], []
    for r in range(reps):
        df.timings = {}
        ta.append(wall(lambda: contracted(True))[0])
        tick_a.append(1e3 * df.timings['S8_get_k_nuc_grad'])
        df.timings = {}
        tc.append(wall(lambda: contracted(False))[0])
        tick_c.append(1e3 * df.timings['S8_get_k_nuc_grad'])
        df.timings = {}
        tb.append(wall(matrix_route)[0])
        tick_b.append(1e3 * df.timings['S8_get_k_e1'])
    print('  get_k_nuc_grad fused                  %s   S8_get_k_nuc_grad %s' % (stat(ta), stat(tick_a)))
    print('  get_k_nuc_grad composed               %s   S8_get_k_nuc_grad %s' % (stat(tc), stat(tick_c)))
    print('  get_k_e1 + host contraction           %s   S8_get_k_e1       %s' % (stat(tb), stat(tick_b)))
    df.get_jk_nuc_grad(dm)
    tj, tp = [], []
    for r in range(reps):
        tj.append(wall(lambda: df.get_jk_nuc_grad(dm))[0])
        tp.append(wall(lambda: (df.get_j_nuc_grad(dm), df.get_k_nuc_grad(dm)))[0])
    print('  get_jk_nuc_grad                       %s' % stat(tj))
    print('  get_j_nuc_grad then get_k_nuc_grad    %s' % stat(tp))
    be.prof_reset()
    be.prof_enable(True)
    df.get_k_nuc_grad(dm)
    be.synchronize()
    prof = be.prof_results()
    be.prof_enable(False)
    for k in sorted(prof, key=lambda k: -prof[k]['ms'])[:8]:
        p = prof[k]
        rate = p['work'] / max(p['ms'], 1e-9) * 1e-6
        print('    kernel %-34s %6d launches %9.2f ms  %8.1f %s' % (k, p['launches'], p['ms'], rate * (1e-3 if k.endswith('[flop]') else 1.0),
                                                                  'TF/s' if k.endswith('[flop]') else 'GB/s'), flush=True)
    df.reset()
    del df
    torch.cuda.empty_cache()


for arg in args:
    if arg == 'kernel':
        kernel_level()
    else:
        name, _, c = arg.partition(':')
        product_level(name, int(c or 10))
