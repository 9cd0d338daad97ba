"""Micro-benchmark: the Hermitian twice-scaled NT product (isdf_herm_kscale_nt, one pass for Re and Im of M^q) against the same three
sums made with isdf_gemm_nt and a stored i X, on a strip of the k-point spectral W^q build.  Default shape: the BASELINE configs[3]
strip (512 rows of P = 14580 against all rows, 2 npts = 0.356 G of the 96^3 mesh, padded to 128).  Alternating timed windows;
flop counted as 4 M N K for either route (two real products of K terms per entry)."""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from pyscf_isdf_amd.backend import HipBackend

ap = argparse.ArgumentParser()
ap.add_argument('--M', type=int, default=512)
ap.add_argument('--N', type=int, default=14580)
ap.add_argument('--K', type=int, default=-(-int(0.356 * 96 ** 3) // 128) * 128)
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--rounds', type=int, default=3)
args = ap.parse_args()
be = HipBackend(0)
M, N, K = args.M, args.N, args.K
gen = torch.Generator(device=be.device).manual_seed(1)
X = torch.randn(N, K, dtype=torch.float64, device=be.device, generator=gen)
iX = torch.empty_like(X)
iX[:, 0::2] = -X[:, 1::2]
iX[:, 1::2] = X[:, 0::2]
s = torch.randn(K // 2, dtype=torch.float64, device=be.device, generator=gen).repeat_interleave(2).contiguous()
a = torch.randn(K // 2, dtype=torch.float64, device=be.device, generator=gen).repeat_interleave(2).contiguous()
A = X[:M]
Cre, Cim = be.empty((M, N)), be.empty((M, N))
Gre, Gim = be.empty((M, N)), be.empty((M, N))


def fused():
    be.herm_kscale_nt(A, X, s, a, Cre, Cim)


def composed():
    be.gemm_nt(A, X, Gre, kscale=s)
    be.gemm_nt(A, iX, Gim, kscale=a)


flop = 4.0 * M * N * K
print('strip M=%d N=%d K=%d: %.2f Tflop per strip' % (M, N, K, flop / 1e12), flush=True)
for fn in (fused, composed):
    fn()
torch.cuda.synchronize()
scale = max(Gre.abs().max().item(), Gim.abs().max().item())
print('max|fused - composed| / max|M| = %.2e' % (max((Cre - Gre).abs().max().item(), (Cim - Gim).abs().max().item()) / scale), flush=True)
for r in range(args.rounds):
    for name, fn in (('herm_kscale_nt', fused), ('2 x gemm_nt + stored iX', composed)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / args.reps
        print('round %d  %-24s %8.2f ms  %.1f TF/s' % (r, name, ms, flop / ms / 1e9), flush=True)
