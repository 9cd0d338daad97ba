"""isdf_gemm_nn_had on the device, C = alpha A (H o B) + beta C, in the manner of tests/test_gpu_gemm_sweep.py: integer operands in
[-4, 4] (every product and partial sum an integer far below 2^53), so the result must EQUAL numpy's, bit for bit.

Aligned cases, the one-launch kernel (label gemm_nn_had_kernel): M in {1, 16, 17, 255, 256, 257, 513} (row clamping, two and three
tile rows: a 2 x 16 super-tile with a ragged second half) x N in {2, 126, 128, 130, 1026} (the clamped last column pair, a one-pair
second tile, nine column tiles) x K in {32, 64, 96} (prologue and epilogue of the double buffer only, one pair of chunks, one more).
lda = K + 2, ldh = N + 4, ldb = N + 6, ldc = N + 8; NaN in every padding of A, H and B (a read of padding shows in C), the
sentinel around C and in its padding; (alpha, beta) cycle through (1, 0) onto NaN, (0.5, -2), (-1, 1), (2, 0); A, H and B must be
bit-unchanged afterwards, and a beta = 0 case run twice must give the same bits.

The composition inside the entry point (labels hadamard_rows_kernel + rocblas_dgemm): alone for K = 31, an odd N, an odd ldh, an
odd lda, an A base and a B base off by 8 bytes; for the K tail, next to one fused launch of the multiple-of-32 prefix, for K = 33
and 104 (lda = K + 3 where K is odd: an even leading dimension)."""
import numpy as np
import pytest
from test_gpu_gemm_sweep import ROCBLAS, _ints, _embed, _view, _aligned, _Out, _c0, _profiled, _report

gpu = pytest.mark.gpu

FUSED = 'gemm_nn_had_kernel[flop]'
HADAMARD = 'hadamard_rows_kernel[byte]'
HAD_M = (1, 16, 17, 255, 256, 257, 513)
HAD_N = (2, 126, 128, 130, 1026)
HAD_K = (32, 64, 96)
SCALARS = ((1.0, 0.0), (0.5, -2.0), (-1.0, 1.0), (2.0, 0.0))
# (M, N, K, lda - K, ldh - N, doubles the A base is off by, doubles the B base is off by): one condition of the fused kernel broken each
COMPOSED = ((17, 128, 31, 3, 4, 0, 0), (17, 128, 33, 3, 4, 0, 0), (26, 500, 104, 2, 4, 0, 0), (257, 129, 64, 2, 4, 0, 0),
            (16, 128, 64, 2, 5, 0, 0), (16, 128, 64, 3, 4, 0, 0), (17, 130, 32, 2, 4, 1, 0), (256, 126, 96, 2, 4, 0, 1))


@pytest.fixture(scope='module')
def be():
    from pyscf_isdf_amd.backend import HipBackend
    b = HipBackend(0)
    b.prof_enable(True)
    yield b
    b.prof_enable(False)
    b.prof_reset()
    b.release_workspace()


class _HadRun:
    def __init__(self, be, M, N, K, alpha, beta, da=2, dh=4, off_a=0, off_b=0):
        rng = np.random.default_rng([M, N, K, da, dh, off_a, off_b])
        self.be, self.M, self.N, self.K, self.alpha, self.beta = be, M, N, K, alpha, beta
        self.lda, self.ldh, self.ldb, self.ldc = K + da, N + dh, N + 6, N + 8
        self.A, self.H, self.B = _ints(rng, (M, K), 4), _ints(rng, (K, N), 4), _ints(rng, (K, N), 4)
        self.c0 = _c0(rng, M, N, beta)
        self.hA, self.hH, self.hB = _embed(self.A, self.lda, off=off_a), _embed(self.H, self.ldh), _embed(self.B, self.ldb, off=off_b)
        self.bA, self.bH, self.bB = (be.to_device(x) for x in (self.hA, self.hH, self.hB))
        self.dA = _view(self.bA, M, K, self.lda, off=off_a)
        self.dH = _view(self.bH, K, N, self.ldh)
        self.dB = _view(self.bB, K, N, self.ldb, off=off_b)
        aligned = self.lda % 2 == 0 and self.ldh % 2 == 0 and off_a % 2 == 0 and off_b % 2 == 0
        assert _aligned(self.dH) and _aligned(self.dA) == (off_a % 2 == 0) and _aligned(self.dB) == (off_b % 2 == 0)
        kf = K - K % 32 if aligned and N % 2 == 0 else 0          # what the one-launch kernel takes; the rest is composed
        self.want = ({FUSED} if kf else set()) | ({HADAMARD, ROCBLAS} if kf < K else set())
        self.fused = kf == K
        self.out = None

    def launch(self):
        self.out = _Out(self.be, self.c0, self.ldc)
        self.be.gemm_nn_had(self.dA, self.dH, self.dB, self.out.view, alpha=self.alpha, beta=self.beta)

    def ref(self):
        r = self.alpha * self.A.dot(self.H * self.B)
        return r if self.beta == 0.0 else r + self.beta * self.c0

    def name(self):
        return 'M=%d N=%d K=%d alpha=%g beta=%g lda=%d ldh=%d ldb=%d' % (self.M, self.N, self.K, self.alpha, self.beta, self.lda, self.ldh,
                                                                        self.ldb)

    def check(self):
        bad = []
        prof = _profiled(self.be, self.launch)
        if set(prof) != self.want or any(prof[k]['launches'] != 1 for k in prof):
            bad.append('ran %s, expected one launch each of %s' % (sorted(prof), sorted(self.want)))
        win, clean = self.out.fetch()
        if not clean:
            bad.append('sentinel around C overwritten')
        r = self.ref()
        if not np.array_equal(win, r):
            i, j = np.argwhere(win != r)[0]
            bad.append('%d of %d entries differ, first at (%d, %d): got %r, exact %r' % ((win != r).sum(), r.size, i, j, win[i, j], r[i, j]))
        for nm, dev, host in (('A', self.bA, self.hA), ('H', self.bH, self.hH), ('B', self.bB, self.hB)):
            if not np.array_equal(self.be.to_host(dev).view(np.int64), host.view(np.int64)):
                bad.append('%s was modified' % nm)
        if self.beta == 0.0:
            self.launch()
            again = self.out.fetch()[0]
            if not np.array_equal(win.view(np.int64), again.view(np.int64)):
                bad.append('two runs on the same inputs differ')
        return bad


@gpu
@pytest.mark.parametrize('K', HAD_K)
def test_fused_exact_sweep(be, K):
    fails, n = [], 0
    for M in HAD_M:
        for N in HAD_N:
            alpha, beta = SCALARS[n % 4]
            n += 1
            run = _HadRun(be, M, N, K, alpha, beta)
            assert run.fused
            bad = run.check()
            if bad:
                fails.append((run.name(), bad))
    _report('NN Hadamard sweep, K = %d: %d cases' % (K, n), fails)
    assert not fails, fails


@gpu
def test_other_alignments_take_the_composition(be):
    fails = []
    for n, (M, N, K, da, dh, off_a, off_b) in enumerate(COMPOSED):
        alpha, beta = SCALARS[n % 4]
        run = _HadRun(be, M, N, K, alpha, beta, da=da, dh=dh, off_a=off_a, off_b=off_b)
        assert not run.fused
        bad = run.check()
        if bad:
            fails.append((run.name(), bad))
    _report('NN Hadamard neighbours: %d cases' % len(COMPOSED), fails)
    assert not fails, fails
