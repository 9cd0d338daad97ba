"""Sweep of the hand-written FP64 matrix-core products (csrc/gemm_f64.hip) over every kernel, edge and stride.

The older GEMM tests (test_gpu_parity.py: test_gemm_nt_mfma, test_gemm_nn_mfma, test_pair_gram_rows_squared_epilogue;
test_gpu_kpts_spectral.py: test_herm_kscale_nt_matches_numpy_and_the_gemm_composition) use a few contiguous, aligned shapes with
one alpha / beta and an absolute bound on Gaussian data.  This module chooses its cases from a restatement of the host dispatch
(plan_nt, plan_herm, plan_nn below: variant, tiles, slab count with its cap and wave-quantisation pick, slab length, super-tiles)
as a function of the CU count, and reads what really ran from the profiling labels: the instantiation, whether the slab reduction
ran, and the slab count from that label's work (8 M N (nslab + 1) bytes for NT, 16 M N (nslab + 1) for the Hermitian form).  A case
whose label or slab count differs from the restatement fails and names both, so a dispatch change has to update the sweep.

  NT     gemm_nt_mfma_kernel<false> (generic), <true> (aligned, K % 32 == 16), kernel_d<false / true>, kernel_b<false / true>, each
         with and without kscale: one chunk / two chunks / K < 16, direct, two slabs, three and more slabs with a shorter last one,
         fewer than 8 units, a unit count padded to 8, M and N one below, at and one above the tile edges, odd lda, an A base and
         a kscale base off by one double
  herm   herm_kscale_nt_kernel: M, N in {1, 127, 128, 129, 300} x K in {16, 128, 6160 (3 slabs, the last one shorter)}
  NN     gemm_nn_mfma_kernel<false> (isdf_gemm_nn) and <true> (isdf_pair_gram_rows) with option gemm_nn_own: M in {225, 256, 448,
         1000, 1280} (super-tiles 1 x 32, 2 x 16, 4 x 8 and a ragged 4 x 8) x N in {2, 126, 128, 130, 4226} x K in {32, 64, 416}, and
         the just-unsupported neighbours, which must take rocBLAS and give the same numbers

Layouts and scalars, each seen by every kernel: lda = K + 2, ldb = K + 4, ldc = N + 3; A a row window of B's matrix; A and B the same
pointer; C a row window of a larger matrix; NaN in the column padding of A, B and the tables and in the rows around them (a read
past K or a stored clamped row poisons the result); a sentinel in the ldc padding and in the rows around C that must be
bit-unchanged; (alpha, beta) = (1, 0) onto a C full of NaN, (0.5, -2), (-1, 1), (2, 0); every multi-slab case twice, bit-identical;
multi-slab NT and Hermitian calls alternating on the shared gemm_partials workspace with growing and shrinking partials.

Two references.
  Exact.  Operands are small integers stored as doubles (entries in [-4, 4], kscale and tables in [-2, 2], alpha and beta powers of
  two): every product and partial sum is an integer far below 2^53, so the result does not depend on summation order, slab count
  or FMA contraction and numpy's float64 product IS the answer.  np.array_equal, no tolerance, for every case above.
  Rounding.  Exact small integers survive a lower-precision path, so Gaussian data, one direct and one multi-slab case per
  kernel, against an np.longdouble product (eps 1.08e-19).  The measure is the error of numpy's float64 product of the same
  inputs against the same reference, relative to max|ref|; the device may exceed it by ROUNDING_FACTOR, the smallest power of
  two at or above 4 x the largest device / numpy ratio measured on an MI355X, capped at 64 (six lost mantissa bits are what the
  test exists to catch).  The scalars here are (w, 0) with a non-dyadic w and (-1, 1).

Measured on an MI355X (256 CUs), device error / numpy error, both against the longdouble product (numpy's own error is 6.5e-16 to
1.05e-15 of max|ref| on these cases, the device's 1.6e-15 to 4.3e-15):

  kernel                        direct                     multi-slab
  gemm_nt_mfma_kernel<false>    4.52 (96 x 100 x 2047)     3.06 (96 x 100 x 6149, 3 slabs)
  gemm_nt_mfma_kernel<true>     4.02 (96 x 100 x 2032)     3.39 (96 x 100 x 6160, 3 slabs)
  gemm_nt_mfma_kernel_d         3.13 (129 x 65 x 2048)     3.04 (129 x 65 x 4096, 2 slabs), 2.52 (129 x 65 x 6176, 3 slabs)
  gemm_nt_mfma_kernel_b         3.56 (256 x 128 x 2048)    3.75 (225 x 64 x 4096, 2 slabs), 2.88 (225 x 64 x 6176, 3 slabs)
  herm_kscale_nt_kernel         4.69 / 2.95 (Re / Im)      4.66 / 3.21 (129 x 65 x 6160, 3 slabs)
  gemm_nn_mfma_kernel           1.91, squared 2.07 (256 x 130 x 416)

The largest is 4.69: a slab is one sequential chain of up to 2080 fused multiply-adds per entry where BLAS sums in blocks, so the
device sits a few times above numpy, the short K = 416 chain of the NN kernel least.  4 x 4.69 = 18.8, so ROUNDING_FACTOR = 32.

Found and fixed: nothing.  All 25 GPU tests passed on the first run against the unchanged kernels (6 s for the module).

Mutations tried on a scratch copy (not committed):
  - kscale indexed without k0 in kernel_d: all 8 scaled multi-slab cases of that kernel fail the exact test (nearly every entry);
  - clamping rows with M instead of M - 1 in kernel_d, and dropping min(..., last) on kernel_d's tail load: the sweep passes, and it
    has to - neither changes a stored value.  A clamped row feeds only accumulator rows the epilogue never stores (an MFMA
    output row depends on its own A row alone), and the chunk a tail load fetches goes to an LDS buffer and a fragment set that
    nothing reads after the loop.  Both only move reads (to the row behind the matrix, to the 16 - 32 doubles behind a slab, here
    NaN padding inside the same allocation): no value test can see them, only an access past the end of an allocation would.
"""
import numpy as np
import pytest

gpu = pytest.mark.gpu

# ---- restatement of the host-side dispatch of gemm_f64.hip (to choose and label cases; what ran is read from the profiling
# ---- labels, what it computed is compared with numpy) ---------------------------------------------------------------------
BM, BN, BK, BM2 = 128, 128, 16, 256
REDUCE = 'gemm_reduce_slabs_kernel[byte]'
HERM = 'herm_kscale_nt_kernel[flop]'
ROCBLAS = 'rocblas_dgemm[flop]'
NT_LABEL = {'g': 'gemm_nt_mfma_kernel<false>[flop]', 'a': 'gemm_nt_mfma_kernel<true>[flop]',
            ('d', False): 'gemm_nt_mfma_kernel_d<false>[flop]', ('d', True): 'gemm_nt_mfma_kernel_d<true>[flop]',
            ('b', False): 'gemm_nt_mfma_kernel_b<false>[flop]', ('b', True): 'gemm_nt_mfma_kernel_b<true>[flop]'}
NN_LABEL = {False: 'gemm_nn_mfma_kernel<false>[flop]', True: 'gemm_nn_mfma_kernel<true>[flop]'}
CPU_TEST_CUS = 256


def cdiv(a, b):
    return -(-a // b)


def _slab_count(ntiles, slots, M, N, K, entry_bytes):
    """Target slab count: units to fill the slots about 8 times over, slabs at least 2048 deep, partials at most 2 GiB, then the
    count between the target and twice the target whose last round of units is fullest."""
    nslab = cdiv(8 * slots, ntiles)
    cap = max(1, min(max(1, K // 2048), max(1, (2 << 30) // (M * N * entry_bytes))))
    nslab = max(1, min(nslab, cap))
    if ntiles * nslab > slots:
        best, pick = 1e30, nslab
        for c in range(nslab, min(2 * nslab, cap) + 1):
            units = ntiles * c
            waste = float(cdiv(units, slots) * slots) / float(units)
            if waste < best - 1e-9:
                best, pick = waste, c
        nslab = pick
    return nslab


class Plan(dict):
    __getattr__ = dict.__getitem__


def plan_nt(M, N, K, scaled, ncu, lda=None, ldb=None, mis_a=0, mis_b=0, mis_s=0):
    """gemm_nt_f64_scaled with ISDF_GEMM_VARIANT unset: kern 'g' | 'a' | 'd' | 'b', label, tiles, slabs, units.  mis_*: the
    operand's base is not 16-byte aligned."""
    lda = K if lda is None else lda
    ldb = K if ldb is None else ldb
    aligned = lda % 2 == 0 and ldb % 2 == 0 and not mis_a and not mis_b and not (scaled and mis_s)
    aligned_b = aligned and K % 32 == 0
    fits_b = float(cdiv(M, BM2) * BM2) <= 1.15 * float(M)
    use_b = aligned_b and M > BM and fits_b
    use_d = aligned_b and not use_b
    fast = aligned and K % BK == 0
    kern = 'd' if use_d else 'b' if use_b else 'a' if fast else 'g'
    ntm, ntn = cdiv(M, BM2 if use_b else BM), cdiv(N, BN)
    ntiles = ntm * ntn
    slots = ncu * (1 if use_b else 2)
    nslab = _slab_count(ntiles, slots, M, N, K, 8)
    kslab = cdiv(cdiv(K, nslab), 2 * BK) * (2 * BK)
    nslab = cdiv(K, kslab)
    units = ntiles * nslab
    return Plan(kern=kern, label=NT_LABEL[kern] if kern in 'ga' else NT_LABEL[kern, bool(scaled)], ntm=ntm, ntn=ntn, nslab=nslab,
                kslab=kslab, last=K - (nslab - 1) * kslab, units=units, units_pad=cdiv(units, 8) * 8)


def plan_herm(M, N, K, ncu):
    """isdf_herm_kscale_nt: one workgroup per CU, two planes of partials, slabs a multiple of 16 long."""
    ntm, ntn = cdiv(M, BM), cdiv(N, BN)
    ntiles = ntm * ntn
    nslab = _slab_count(ntiles, ncu, M, N, K, 16)
    kslab = cdiv(cdiv(K, nslab), BK) * BK
    nslab = cdiv(K, kslab)
    units = ntiles * nslab
    return Plan(kern='h', label=HERM, ntm=ntm, ntn=ntn, nslab=nslab, kslab=kslab, last=K - (nslab - 1) * kslab, units=units,
                units_pad=cdiv(units, 8) * 8)


def plan_nn(M, N, K, sq, own=True, lda=None, ldb=None, mis_a=0, mis_b=0, alpha=1.0, beta=0.0):
    """isdf_gemm_nn / product_rows: gemm_nn_f64_supported and the super-tile shape, or rocBLAS."""
    lda = K if lda is None else lda
    ldb = N if ldb is None else ldb
    ok = own and M > BM and float(cdiv(M, BM2) * BM2) <= 1.15 * float(M) and N >= 2 and N % 2 == 0 and K >= 32 and K % 32 == 0 \
        and lda % 2 == 0 and ldb % 2 == 0 and not mis_a and not mis_b and (sq or (alpha == 1.0 and beta == 0.0))
    if not ok:
        return Plan(kern='rocblas', label=ROCBLAS)
    ntm, ntn = cdiv(M, BM2), cdiv(N, BN)
    stm = 4 if ntm >= 4 else 2 if ntm >= 2 else 1
    stn = 32 // stm
    ngm = cdiv(ntm, stm)
    return Plan(kern='nn', label=NN_LABEL[bool(sq)], ntm=ntm, ntn=ntn, stm=stm, stn=stn, ngm=ngm, ragged=ntm % stm != 0,
                units=ngm * cdiv(ntn, stn) * 32)


# ---- the case lists ---------------------------------------------------------------------------------------------------------
LAYOUTS = ('plain', 'strided', 'window')         # 'same' (A and B one pointer) needs M == N: the LAYOUT_SHAPE cases
SCALARS = ((1.0, 0.0), (0.5, -2.0), (-1.0, 1.0), (2.0, 0.0))
NT_TABLE = {
    'g': [(1, 1, 1), (64, 64, 17), (130, 131, 6149), (7, 300, 9261)],
    'a': [(5, 7, 16), (64, 300, 48), (200, 140, 6160), (130, 257, 4112)],
    'd': [(1, 1, 32), (33, 17, 32), (127, 129, 64), (129, 257, 4096), (300, 130, 6176), (128, 128, 8224), (16, 16, 16384)],
    'b': [(225, 130, 32), (256, 128, 4096), (448, 257, 6176), (1000, 130, 8224), (512, 384, 14368)],
}
NT_MISALIGNED = (96, 200, 4096)                   # an aligned shape of kernel_d that odd lda / an offset base sends to the generic kernel
NT_EDGE_K = {'g': 33, 'a': 48, 'd': 64, 'b': 64}
NT_EDGE_M = {'g': (127, 128, 129), 'a': (127, 128, 129), 'd': (127, 128, 129), 'b': (225, 448)}
NT_EDGE_N = (127, 128, 129)
NT_LAYOUT_SHAPE = {'g': (130, 130, 4099), 'a': (130, 130, 4112), 'd': (129, 129, 4096), 'b': (448, 448, 4096)}
# (M, N, K) -> (nslab, last slab) at 256 CUs, as worked out by hand next to the dispatch code
NT_PINNED_256 = {(130, 131, 6149): (3, 1989), (7, 300, 9261): (4, 2253), (200, 140, 6160): (3, 2000), (130, 257, 4112): (2, 2032),
                 (129, 257, 4096): (2, 2048), (300, 130, 6176): (3, 2016), (128, 128, 8224): (4, 1984), (16, 16, 16384): (8, 2048),
                 (256, 128, 4096): (2, 2048), (448, 257, 6176): (3, 2016), (1000, 130, 8224): (4, 1984),
                 (512, 384, 14368): (7, 1888), (64, 64, 17): (1, 17), (225, 130, 32): (1, 32)}
HERM_MN = (1, 127, 128, 129, 300)
HERM_K = (16, 128, 6160)
NN_M = (225, 256, 448, 1000, 1280)
NN_N = (2, 126, 128, 130, 4226)
NN_K = (32, 64, 416)
# (M, N, K, alpha): one condition of gemm_nn_f64_supported / isdf_gemm_nn broken each
NN_NEIGHBOURS = ((256, 127, 64, 1.0), (256, 128, 40, 1.0), (300, 128, 64, 1.0), (256, 128, 64, 2.0))


class Case(dict):
    __getattr__ = dict.__getitem__

    def name(self):
        return '%s %dx%dx%d%s %s%s alpha=%g beta=%g' % (self.kern, self.M, self.N, self.K, ' kscale' if self.get('scaled') else '',
                                                         self.lay, ' mis=' + self.mis if self.get('mis') else '', self.alpha,
                                                         self.beta)


def nt_cases(kern):
    """The NT cases written for one kernel: the table, the tile edges, the four layouts; layouts and scalars rotate."""
    out = []

    def add(shape, scaled, lay=None, mis=None):
        i = len(out)
        alpha, beta = SCALARS[(i // 2 + i) % 4]
        out.append(Case(kern=kern, M=shape[0], N=shape[1], K=shape[2], scaled=scaled, lay=lay or LAYOUTS[(i // 2) % 3], mis=mis,
                        alpha=alpha, beta=beta))
    for shape in NT_TABLE[kern]:
        for scaled in (False, True):
            add(shape, scaled)
    if kern == 'g':
        for scaled in (False, True):
            add(NT_MISALIGNED, scaled, 'plain', 'lda')
            add(NT_MISALIGNED, scaled, 'plain', 'abase')
        add(NT_MISALIGNED, True, 'plain', 'sbase')
    for i, M in enumerate(NT_EDGE_M[kern]):
        for j, N in enumerate(NT_EDGE_N):
            add((M, N, NT_EDGE_K[kern]), (i + j) % 2 == 1)
    for lay in LAYOUTS + ('same',):
        for scaled in (False, True):
            add(NT_LAYOUT_SHAPE[kern], scaled, lay)
    return out


def nt_geometry(c):
    """Leading dimensions and first-element offsets (in doubles, inside 16-byte aligned allocations) of a case's operands.
    Every matrix sits behind two rows of padding, so its first element is at off + 2 ld (+ r0 ld for a row window)."""
    K, N = c.K, c.N
    lda, ldb, ldc = {'plain': (K, K, N), 'strided': (K + 2, K + 4, N + 3), 'window': (K + 2, K + 2, N + 3),
                     'same': (K + 4, K + 4, N)}[c.lay]
    off_a = off_s = 0
    r0 = 3 if c.lay == 'window' else 0
    mis = c.get('mis')
    if mis == 'lda':
        lda = K + 1 if K % 2 == 0 else K
    elif mis == 'abase':
        off_a = 1
    elif mis == 'sbase':
        off_s = 1
    return Plan(lda=lda, ldb=ldb, ldc=ldc, r0=r0, off_a=off_a, off_s=off_s, a0=off_a + (2 + r0) * lda, b0=2 * ldb)


def nt_plan(c, ncu):
    g = nt_geometry(c)
    return plan_nt(c.M, c.N, c.K, c.scaled, ncu, lda=g.lda, ldb=g.ldb, mis_a=g.a0 % 2, mis_b=g.b0 % 2, mis_s=g.off_s % 2)


def herm_cases():
    out = []
    for K in HERM_K:
        for M in HERM_MN:
            for N in HERM_MN:
                i = len(out)
                alpha, beta = SCALARS[(i // 3) % 4]
                lay = 'same' if M == N and M in (127, 128, 300) else LAYOUTS[i % 3]
                out.append(Case(kern='h', M=M, N=N, K=K, lay=lay, alpha=alpha, beta=beta))
    return out


def nn_cases(sq):
    out = []
    for M in NN_M:
        for N in NN_N:
            for K in NN_K:
                out.append(Case(kern='nn', M=M, N=N, K=K, sq=sq, lay=('plain', 'strided')[len(out) % 2], alpha=1.0, beta=0.0))
    return out


def nt_tags(label, scaled, M, N, K, nslab, kslab):
    """(class, coverage tags) of one NT launch, from the label and slab count (predicted or observed)."""
    tile_m = BM2 if '_b<' in label else BM
    units = cdiv(M, tile_m) * cdiv(N, BN) * nslab
    tags = set()
    if nslab == 1:
        tags.add('direct')
    if nslab >= 3 and K - (nslab - 1) * kslab < kslab:
        tags.add('3+ slabs, ragged last')
    if units < 8:
        tags.add('units < 8')
    if units > 8 and units % 8:
        tags.add('units padded')
    if nslab == 1 and (K == 32 if ('_b<' in label or '_d<' in label) else K == 16 if 'kernel<true>' in label else K < 16):
        tags.add('minimal chunks')
    return (label, bool(scaled)), tags


NT_TAGS = {'direct', '3+ slabs, ragged last', 'units < 8', 'units padded', 'minimal chunks'}


def nt_classes(kern):
    if kern in 'ga':
        return [(NT_LABEL[kern], False), (NT_LABEL[kern], True)]
    return [(NT_LABEL[kern, False], False), (NT_LABEL[kern, True], True)]


def _missing(cover, classes, want):
    return ['%s%s: %s' % (cl[0], ' + kscale' if cl[1] else '', t) for cl in classes for t in sorted(want - cover.get(cl, set()))]


def test_plan_covers_every_kernel_and_edge():
    """The restatement at 256 CUs over the case lists: every case lands on the kernel it was written for, the slab counts worked
    out by hand hold, and for every NT instantiation, with and without kscale, the plan has a direct case, one with three or more
    slabs and a shorter last one, one with fewer than 8 units, one with a padded unit count and the minimal chunk count; the
    Hermitian cases are direct and multi-slab; the NN cases reach the three super-tile shapes and a ragged super-tile, and each
    neighbour falls to rocBLAS."""
    ncu = CPU_TEST_CUS
    for (M, N, K), (nslab, last) in NT_PINNED_256.items():
        p = plan_nt(M, N, K, False, ncu)
        assert (p.nslab, p.last) == (nslab, last), ((M, N, K), p)
    for kern in 'gadb':
        cover = {}
        for c in nt_cases(kern):
            p = nt_plan(c, ncu)
            assert p.kern == kern, (c.name(), p)
            if c.mis:
                assert plan_nt(c.M, c.N, c.K, c.scaled, ncu).kern == 'd', c.name()   # aligned, it is kernel_d's
            assert p.last <= p.kslab and (p.nslab - 1) * p.kslab < c.K and p.kslab % 32 == 0
            cl, tags = nt_tags(p.label, c.scaled, c.M, c.N, c.K, p.nslab, p.kslab)
            cover.setdefault(cl, set()).update(tags)
            cover[cl].add('layout ' + c.lay)
            cover[cl].add('scalars %g %g' % (c.alpha, c.beta))
        want = NT_TAGS | {'layout ' + s for s in LAYOUTS + ('same',)} | {'scalars %g %g' % s for s in SCALARS}
        assert not _missing(cover, nt_classes(kern), want), _missing(cover, nt_classes(kern), want)
        edges = {(c.M, c.N) for c in nt_cases(kern) if c.K == NT_EDGE_K[kern]}
        assert edges >= {(M, N) for M in NT_EDGE_M[kern] for N in NT_EDGE_N}
    hp = [plan_herm(c.M, c.N, c.K, ncu) for c in herm_cases()]
    assert {p.nslab for p in hp} == {1, 3} and all(p.last < p.kslab for p in hp if p.nslab > 1)
    for K in HERM_K:                                         # direct and multi-slab see every layout and every scalar pair
        assert {c.lay for c in herm_cases() if c.K == K} == set(LAYOUTS + ('same',))
        assert {(c.alpha, c.beta) for c in herm_cases() if c.K == K} == set(SCALARS)
    for sq in (False, True):
        ps = [nn_plan(c) for c in nn_cases(sq)]
        assert all(p.kern == 'nn' for p in ps)
        assert {(p.stm, p.stn) for p in ps} == {(1, 32), (2, 16), (4, 8)} and any(p.ragged for p in ps)
        assert {p.ntm for p in ps} == {1, 2, 4, 5}
    assert all(nn_plan(c).kern == 'rocblas' for c in nn_neighbour_cases())
    assert nn_plan(Case(kern='nn', M=256, N=128, K=64, sq=False, lay='strided', alpha=1.0, beta=0.0)).kern == 'nn'


def nn_neighbour_cases():
    out = [Case(kern='nn', M=M, N=N, K=K, sq=False, lay='strided', alpha=alpha, beta=0.0) for M, N, K, alpha in NN_NEIGHBOURS]
    return out + [Case(kern='nn', M=300, N=128, K=64, sq=True, lay='strided', alpha=1.0, beta=0.0)]


def nn_geometry(c):
    """A (M, lda), B a column window (first column 2) of a (K, ldb) matrix, C (M, ldc); pair_gram_rows takes a contiguous A."""
    strided = c.lay == 'strided'
    return Plan(lda=c.K + 2 if strided and not c.sq else c.K, ldb=c.N + 6 if strided or c.N % 2 else c.N,
                ldc=c.N + 3 if strided else c.N, col0=2 if strided or c.N % 2 else 0)


def nn_plan(c):
    g = nn_geometry(c)
    return plan_nn(c.M, c.N, c.K, c.sq, lda=g.lda, ldb=g.ldb, mis_a=0, mis_b=(2 * g.ldb + g.col0) % 2, alpha=c.alpha, beta=c.beta)


# ---- device side ------------------------------------------------------------------------------------------------------------
SENTINEL = -777.25
PAD_ROWS = 2


@pytest.fixture(scope='module')
def be():
    from pyscf_isdf_amd.backend import HipBackend
    b = HipBackend(0)
    b.prof_enable(True)
    yield b
    b.prof_enable(False)
    b.prof_reset()
    b.set_option('gemm_nn_own', 0)
    b.release_workspace()


@pytest.fixture(scope='module')
def ncu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _ints(rng, shape, m):
    return rng.integers(-m, m + 1, size=shape).astype(np.float64)


def _embed(mat, ld, off=0, fill=np.nan, col0=0):
    """Flat host buffer: ``off`` doubles, PAD_ROWS rows, the matrix in rows of ld (from column col0), PAD_ROWS rows; ``fill``
    everywhere else."""
    rows = mat.shape[0] + 2 * PAD_ROWS
    buf = np.full(off + rows * ld, fill)
    buf[off:].reshape(rows, ld)[PAD_ROWS:PAD_ROWS + mat.shape[0], col0:col0 + mat.shape[1]] = mat
    return buf


def _view(dbuf, nrow, ncol, ld, off=0, row0=0, col0=0):
    """The (nrow, ncol) window of a device buffer laid out by _embed, starting at matrix row row0."""
    first = off + (PAD_ROWS + row0) * ld
    return dbuf[first:first + nrow * ld].view(nrow, ld)[:, col0:col0 + ncol]


def _aligned(t):
    return t.data_ptr() % 16 == 0


class _Out:
    """A C operand: the (M, N) window of a sentinel-filled buffer with ldc >= N, prefilled with c0 (NaN where beta == 0)."""

    def __init__(self, be, c0, ldc):
        self.be, self.M, self.N, self.ldc = be, c0.shape[0], c0.shape[1], ldc
        self.host = _embed(c0, ldc, fill=SENTINEL)
        self.dev = be.to_device(self.host)
        self.view = _view(self.dev, self.M, self.N, ldc)

    def fetch(self):
        """(the window, whether everything around it is bit-unchanged)."""
        after = self.be.to_host(self.dev)
        win = after.reshape(-1, self.ldc)[PAD_ROWS:PAD_ROWS + self.M, :self.N].copy()
        before = self.host.copy()
        for buf in (after, before):
            buf.reshape(-1, self.ldc)[PAD_ROWS:PAD_ROWS + self.M, :self.N] = 0.0
        return win, np.array_equal(after.view(np.int64), before.view(np.int64))


def _c0(rng, M, N, beta, integer=True):
    if beta == 0.0:
        return np.full((M, N), np.nan)
    return _ints(rng, (M, N), 4) if integer else rng.standard_normal((M, N))


def _iB(B):
    Bt = np.empty_like(B)
    Bt[:, 0::2] = -B[:, 1::2]
    Bt[:, 1::2] = B[:, 0::2]
    return Bt


class _NTRun:
    """One isdf_gemm_nt (herm = False) or isdf_herm_kscale_nt (herm = True) case on the device: operands laid out as the case
    asks, launch(), and check() against a reference computed by ``product`` (numpy float64 for the exact test)."""

    def __init__(self, be, c, rng, herm=False, gaussian=False):
        self.be, self.c, self.herm = be, c, herm
        M, N, K = c.M, c.N, c.K
        g = nt_geometry(c)
        draw = (lambda shape, m: rng.standard_normal(shape)) if gaussian else (lambda shape, m: _ints(rng, shape, m))
        if c.lay in ('window', 'same'):
            assert c.lay == 'window' or M == N
            mat = draw((max(N, g.r0 + M), K), 4)
            self.A, self.B = mat[g.r0:g.r0 + M], mat[:N]
            dbuf = be.to_device(_embed(mat, g.ldb))
            self.dB = _view(dbuf, N, K, g.ldb)
            self.dA = self.dB if c.lay == 'same' else _view(dbuf, M, K, g.ldb, row0=g.r0)
            assert (c.lay == 'same') == (self.dA.data_ptr() == self.dB.data_ptr())
        else:
            self.A, self.B = draw((M, K), 4), draw((N, K), 4)
            self.dA = _view(be.to_device(_embed(self.A, g.lda, off=g.off_a)), M, K, g.lda, off=g.off_a)
            self.dB = _view(be.to_device(_embed(self.B, g.ldb)), N, K, g.ldb)
        assert self.dA.stride(0) == (g.ldb if c.lay in ('window', 'same') else g.lda) and self.dB.stride(0) == g.ldb
        assert _aligned(self.dA) == (g.a0 % 2 == 0) and _aligned(self.dB) == (g.b0 % 2 == 0)
        self.tables, self.dT = [], []
        for _ in range(2 if herm else 1 if c.get('scaled') else 0):
            t = draw(K // 2, 2).repeat(2) if herm else draw(K, 2)          # herm: pair-repeated, as the ABI requires
            self.tables.append(t)
            d = be.to_device(np.concatenate([np.full(g.off_s, np.nan), t, np.full(32, np.nan)]))[g.off_s:g.off_s + K]
            assert _aligned(d) == (g.off_s % 2 == 0)
            self.dT.append(d)
        self.c0 = [_c0(rng, M, N, c.beta, not gaussian) for _ in range(2 if herm else 1)]
        self.ldc = g.ldc
        self.outs = None

    def launch(self):
        be, c = self.be, self.c
        self.outs = [_Out(be, c0, self.ldc) for c0 in self.c0]
        if self.herm:
            be.herm_kscale_nt(self.dA, self.dB, self.dT[0], self.dT[1], self.outs[0].view, self.outs[1].view, alpha=c.alpha,
                              beta=c.beta)
        else:
            be.gemm_nt(self.dA, self.dB, self.outs[0].view, alpha=c.alpha, beta=c.beta, kscale=self.dT[0] if self.dT else None)

    def refs(self, cast=lambda x: x):
        """alpha A (B .* s)^T + beta C0 per output plane, in the precision ``cast`` converts the operands to."""
        c = self.c
        A, B = cast(self.A), cast(self.B)
        if self.herm:
            prods = [(A * cast(self.tables[0])).dot(B.T), (A * cast(self.tables[1])).dot(_iB(B).T)]
        else:
            prods = [A.dot((B * cast(self.tables[0])).T if self.tables else B.T)]
        return [cast(c.alpha) * p + (cast(c.beta) * cast(c0) if c.beta != 0.0 else 0) for p, c0 in zip(prods, self.c0)]

    def fetch(self, bad):
        got = []
        for o in self.outs:
            win, clean = o.fetch()
            got.append(win)
            if not clean:
                bad.append('sentinel around C overwritten')
        return got

    def check_exact(self, bad):
        got = self.fetch(bad)
        for plane, (w, r) in enumerate(zip(got, self.refs())):
            if not np.array_equal(w, r):
                nbad = int((w != r).sum())
                i, j = np.argwhere(w != r)[0]
                bad.append('plane %d: %d of %d entries differ, first at (%d, %d): got %r, exact %r' %
                           (plane, nbad, w.size, i, j, w[i, j], r[i, j]))
        return got


def _profiled(be, fn):
    be.prof_reset()
    fn()
    return be.prof_results()


def _observed_nslab(prof, M, N, entry_bytes):
    if REDUCE not in prof:
        return 1
    return int(round(prof[REDUCE]['work'] / (float(entry_bytes) * M * N))) - 1


def _check_dispatch(prof, plan, M, N, entry_bytes, bad):
    """The labels and the slab count that ran against the restatement; returns the observed (label, nslab)."""
    kernels = sorted(k for k in prof if k != REDUCE)
    nslab = _observed_nslab(prof, M, N, entry_bytes)
    if kernels != [plan.label]:
        bad.append('ran %s, the restatement says %s' % (kernels, plan.label))
    if nslab != plan.nslab or (REDUCE in prof) != (plan.nslab > 1):
        bad.append('ran %d slab(s)%s, the restatement says %d' % (nslab, ' with a reduction' if REDUCE in prof else '', plan.nslab))
    return (kernels[0] if kernels else None), nslab


def _run_exact(be, run, plan, entry_bytes):
    """Launch under the profiler, compare dispatch and values; a multi-slab case runs twice and must repeat bit for bit."""
    bad = []
    prof = _profiled(be, run.launch)
    label, nslab = _check_dispatch(prof, plan, run.c.M, run.c.N, entry_bytes, bad)
    got = run.check_exact(bad)
    if nslab > 1 or plan.nslab > 1:
        run.launch()
        again = run.fetch(bad)
        if not all(np.array_equal(x.view(np.int64), y.view(np.int64)) for x, y in zip(got, again)):
            bad.append('two runs on the same inputs differ')
    return label, nslab, bad


def _report(title, fails, cover=None):
    print('\n' + title)
    for cl in sorted(cover or {}, key=str):
        print('  %-55s %s' % (cl if isinstance(cl, str) else cl[0] + (' + kscale' if cl[1] else ''), ', '.join(sorted(cover[cl]))))
    for name, bad in fails:
        print('  FAILED %s: %s' % (name, '; '.join(bad)))


@gpu
@pytest.mark.parametrize('kern', ['g', 'a', 'd', 'b'])
def test_nt_exact_sweep(be, ncu, kern):
    """Every NT case written for one kernel (generic, aligned, D, B): the instantiation and slab count that ran against the
    restatement, the exact integer product, the sentinel around C, NaN in every padding, two bit-identical runs of the multi-slab
    cases; and the coverage seen from the observed labels must be complete with and without kscale."""
    fails, cover = [], {}
    for c in nt_cases(kern):
        plan = nt_plan(c, ncu)
        run = _NTRun(be, c, np.random.default_rng([c.M, c.N, c.K, int(c.scaled)]))
        label, nslab, bad = _run_exact(be, run, plan, 8)
        if label is not None:
            kslab = plan.kslab if nslab == plan.nslab else cdiv(cdiv(c.K, nslab), 32) * 32
            cl, tags = nt_tags(label, c.scaled, c.M, c.N, c.K, nslab, kslab)
            cover.setdefault(cl, set()).update(tags)
        if bad:
            fails.append((c.name(), bad))
    _report('NT sweep, kernel %s on %d CUs: %d cases' % (kern, ncu, len(nt_cases(kern))), fails, cover)
    assert not fails, fails
    missing = _missing(cover, nt_classes(kern), NT_TAGS)
    assert not missing, missing


@gpu
@pytest.mark.parametrize('K', HERM_K)
def test_herm_exact_sweep(be, ncu, K):
    """isdf_herm_kscale_nt over M, N in {1, 127, 128, 129, 300} at one K of {16, 128, 6160}: label and slab count (16 M N (nslab + 1)
    bytes per call) against the restatement, both planes exact, sentinels, NaN padding behind the operands and the pair-repeated
    tables, every layout and scalar pair, two bit-identical runs of the multi-slab cases (K = 6160: three slabs, the last one
    shorter); what the labels show must be the coverage the plan promised."""
    fails, cover, planned = [], {HERM: set()}, set()

    def tag(nslab):
        return 'direct' if nslab == 1 else 'multi-slab' + (', ragged last' if K % nslab or (K // nslab) % BK else '')
    for c in (c for c in herm_cases() if c.K == K):
        plan = plan_herm(c.M, c.N, c.K, ncu)
        planned.add(tag(plan.nslab))
        run = _NTRun(be, c, np.random.default_rng([c.M, c.N, c.K]), herm=True)
        label, nslab, bad = _run_exact(be, run, plan, 16)
        if label == HERM:
            cover[HERM].add(tag(nslab))
        if bad:
            fails.append((c.name(), bad))
    _report('Hermitian sweep, K = %d on %d CUs: %d cases' % (K, ncu, len(HERM_MN) ** 2), fails, cover)
    assert not fails, fails
    assert cover[HERM] == planned == ({'direct'} if K < 4096 else {'multi-slab, ragged last'}), (cover, planned)


class _NNRun:
    """One own-NN case: isdf_gemm_nn (sq False) or isdf_pair_gram_rows (sq True) with option gemm_nn_own."""

    def __init__(self, be, c, rng, gaussian=False):
        self.be, self.c = be, c
        M, N, K = c.M, c.N, c.K
        g = self.g = nn_geometry(c)
        draw = (lambda shape: rng.standard_normal(shape)) if gaussian else (lambda shape: _ints(rng, shape, 4))
        self.A, self.B = draw((M, K)), draw((K, N))
        self.dA = _view(be.to_device(_embed(self.A, g.lda)), M, K, g.lda)
        self.dB = _view(be.to_device(_embed(self.B, g.ldb, col0=g.col0)), K, N, g.ldb, col0=g.col0)
        assert _aligned(self.dA) and _aligned(self.dB) == ((2 * g.ldb + g.col0) % 2 == 0) and self.dB.stride(0) == g.ldb
        self.out = None

    def launch(self):
        be, c = self.be, self.c
        self.out = _Out(be, np.full((c.M, c.N), np.nan), self.g.ldc)
        be.set_option('gemm_nn_own', 1)
        try:
            if c.sq:
                be.pair_gram_rows(self.dA, self.dB, c.N, self.out.view)
            else:
                be.gemm_nn(self.dA, self.dB, self.out.view, alpha=c.alpha, beta=c.beta)
        finally:
            be.set_option('gemm_nn_own', 0)

    def ref(self, cast=lambda x: x):
        p = cast(self.A).dot(cast(self.B))
        return p * p if self.c.sq else cast(self.c.alpha) * p


def _run_nn_exact(be, c):
    run = _NNRun(be, c, np.random.default_rng([c.M, c.N, c.K, int(c.sq)]))
    plan = nn_plan(c)
    bad = []
    prof = _profiled(be, run.launch)
    if sorted(prof) != [plan.label]:
        bad.append('ran %s, the restatement says %s' % (sorted(prof), plan.label))
    win, clean = run.out.fetch()
    if not clean:
        bad.append('sentinel around C overwritten')
    r = run.ref()
    if not np.array_equal(win, r):
        i, j = np.argwhere(win != r)[0]
        bad.append('%d of %d entries differ, first at (%d, %d): got %r, exact %r' % ((win != r).sum(), r.size, i, j, win[i, j], r[i, j]))
    return plan, sorted(prof), bad


@gpu
@pytest.mark.parametrize('sq', [False, True])
def test_nn_exact_sweep(be, sq):
    """The own NN kernel over M in {225, 256, 448, 1000, 1280} x N in {2, 126, 128, 130, 4226} x K in {32, 64, 416}, plain through
    isdf_gemm_nn and squared through isdf_pair_gram_rows: label, exact product onto a C full of NaN, sentinel in the ldc padding
    and around C, NaN in the padding of A and around B's column window; all three super-tile shapes and a ragged one."""
    fails, cover = [], {NN_LABEL[sq]: set()}
    for c in nn_cases(sq):
        plan, labels, bad = _run_nn_exact(be, c)
        if labels == [NN_LABEL[sq]]:
            cover[NN_LABEL[sq]].add('super-tile %d x %d%s' % (plan.stm, plan.stn, ' ragged' if plan.ragged else ''))
        if bad:
            fails.append((c.name(), bad))
    _report('NN sweep, squared = %s: %d cases' % (sq, len(nn_cases(sq))), fails, cover)
    assert not fails, fails
    assert cover[NN_LABEL[sq]] == {'super-tile 1 x 32', 'super-tile 2 x 16', 'super-tile 4 x 8', 'super-tile 4 x 8 ragged'}, cover


@gpu
def test_nn_unsupported_neighbours_take_rocblas(be):
    """Odd N, K = 40, M = 300 (row padding above 15 %) and alpha = 2 through isdf_gemm_nn, M = 300 through isdf_pair_gram_rows,
    and a supported shape with the option off: the label says rocBLAS, the numbers are the same exact product."""
    fails = []
    cases = nn_neighbour_cases()
    for c in cases:
        plan, labels, bad = _run_nn_exact(be, c)
        if plan.label != ROCBLAS:
            bad.append('the restatement does not send this case to rocBLAS')
        if bad:
            fails.append((c.name(), bad))
    c = Case(kern='nn', M=256, N=128, K=64, sq=False, lay='plain', alpha=1.0, beta=0.0)
    run = _NNRun(be, c, np.random.default_rng(5))
    run.out = _Out(be, np.full((c.M, c.N), np.nan), run.g.ldc)
    prof = _profiled(be, lambda: be.gemm_nn(run.dA, run.dB, run.out.view))
    if sorted(prof) != [ROCBLAS] or not np.array_equal(run.out.fetch()[0], run.ref()):
        fails.append((c.name() + ' option off', sorted(prof)))
    _report('NN neighbours: %d cases' % (len(cases) + 1), fails)
    assert not fails, fails


@gpu
def test_shared_partials_workspace_alternating(be, ncu):
    """NT and Hermitian multi-slab calls share the gemm_partials workspace: alternate the two entry points with partials that grow
    and then shrink, queue all of them before reading any result back, and every product must still be exact."""
    seq = [('nt', 16, 16, 4096), ('herm', 129, 65, 6160), ('nt', 300, 130, 6176), ('herm', 300, 300, 6160),
           ('nt', 512, 384, 14368), ('herm', 129, 65, 6160), ('nt', 16, 16, 4096)]
    be.release_workspace()
    runs, sizes = [], []
    for i, (kind, M, N, K) in enumerate(seq):
        herm = kind == 'herm'
        c = Case(kern='h' if herm else 'nt', M=M, N=N, K=K, scaled=i % 4 == 2, lay='plain', mis=None, alpha=1.0, beta=0.0)
        plan = plan_herm(M, N, K, ncu) if herm else nt_plan(c, ncu)
        assert plan.nslab > 1, (seq[i], plan)
        sizes.append(plan.nslab * M * N * (2 if herm else 1))
        runs.append(_NTRun(be, c, np.random.default_rng([i, M, N, K]), herm=herm))
    assert sizes.index(max(sizes)) not in (0, len(sizes) - 1) and sizes[0] < sizes[1] < sizes[2] and sizes[-1] < sizes[-2] < sizes[-3]
    for run in runs:
        run.launch()
    fails = []
    for run in runs:
        bad = []
        run.check_exact(bad)
        if bad:
            fails.append((run.c.name(), bad))
    _report('shared workspace: partial sizes (doubles) %s' % sizes, fails)
    assert not fails, fails


# ---- rounding ---------------------------------------------------------------------------------------------------------------
# The smallest power of two at or above 4 x the largest device / numpy error ratio measured on an MI355X (4.69, module docstring);
# it may not exceed 64 whatever a later measurement says.
ROUNDING_FACTOR = 32.0
W = 0.7                                            # a non-dyadic alpha
ROUNDING_CASES = [
    # kind, M, N, K, scaled / squared, alpha, beta   (M N K <= 1e8; the second case of each NT kernel is multi-slab)
    ('g', 96, 100, 2047, True, W, 0.0), ('g', 96, 100, 6149, False, -1.0, 1.0),
    ('a', 96, 100, 2032, False, -1.0, 1.0), ('a', 96, 100, 6160, True, W, 0.0),
    ('d', 129, 65, 2048, True, W, 0.0), ('d', 129, 65, 4096, False, -1.0, 1.0), ('d', 129, 65, 6176, True, -1.0, 1.0),
    ('b', 256, 128, 2048, False, W, 0.0), ('b', 225, 64, 6176, True, -1.0, 1.0), ('b', 225, 64, 4096, False, W, 0.0),
    ('h', 129, 65, 2048, None, W, 0.0), ('h', 129, 65, 6160, None, -1.0, 1.0),
    ('nn', 256, 130, 416, False, 1.0, 0.0), ('nn', 256, 130, 416, True, 1.0, 0.0),
]


def _rel_err(x, ref):
    return float(abs(x.astype(np.longdouble) - ref).max() / abs(ref).max())


@gpu
@pytest.mark.parametrize('kind,M,N,K,flag,alpha,beta', ROUNDING_CASES)
def test_rounding_against_longdouble(be, ncu, kind, M, N, K, flag, alpha, beta):
    """Gaussian operands: the device's error against an np.longdouble product may exceed the error of numpy's float64 product of
    the same inputs against the same reference by ROUNDING_FACTOR at most."""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63 and M * N * K <= 1.02e8
    rng = np.random.default_rng([M, N, K, int(bool(flag))])
    ld = lambda x: np.asarray(x, dtype=np.longdouble)
    if kind == 'nn':
        c = Case(kern='nn', M=M, N=N, K=K, sq=flag, lay='strided', alpha=alpha, beta=beta)
        run = _NNRun(be, c, rng, gaussian=True)
        plan = nn_plan(c)
        prof = _profiled(be, run.launch)
        got, refs, f64 = [run.out.fetch()[0]], [run.ref(ld)], [run.ref()]
        multi = False
    else:
        herm = kind == 'h'
        c = Case(kern=kind, M=M, N=N, K=K, scaled=bool(flag), lay='strided', mis=None, alpha=alpha, beta=beta)
        plan = plan_herm(M, N, K, ncu) if herm else nt_plan(c, ncu)
        run = _NTRun(be, c, rng, herm=herm, gaussian=True)
        prof = _profiled(be, run.launch)
        bad = []
        _check_dispatch(prof, plan, M, N, 16 if herm else 8, bad)
        assert not bad, bad
        got, refs, f64 = run.fetch(bad), run.refs(ld), run.refs()
        assert not bad, bad
        multi = plan.nslab > 1
    assert plan.label in prof and (kind in ('h', 'nn') or plan.kern == kind), (sorted(prof), plan)
    for plane, (w, r, n) in enumerate(zip(got, refs, f64)):
        dev, host = _rel_err(w, r), _rel_err(n, r)
        print('rounding %-36s %dx%dx%d %s plane %d: device %.2e, numpy %.2e, ratio %.2f' %
              (plan.label, M, N, K, 'multi-slab' if multi else 'direct', plane, dev, host, dev / host))
        assert np.isfinite(w).all() and host > 0.0
        assert dev <= ROUNDING_FACTOR * host, (plan.label, (M, N, K), dev, host, dev / host)
