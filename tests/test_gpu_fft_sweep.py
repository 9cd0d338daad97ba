"""Sweep of the hand-written FFT (csrc/fft_conv.hip) over every length, axis, path and plane kernel.

The three older FFT tests (test_gpu_parity.py: test_own_fft_convolution_matches_oracle_and_hipfft,
test_spectral_W_matches_the_classic_product; test_gpu_kpts.py: test_coulomb_Wq_own_fft_matches_hipfft_and_numpy) use a few
hand-picked meshes.  This module chooses its meshes from a restatement of factorise() (the radix sequence per length) and of
the path dispatch, asserts from the profiling labels which transform really ran, and compares with numpy's double-precision
FFT / the oracle's coulomb_V - never with the library's own hipFFT path alone:

  A  every accepted length 2..1024 (86 smooth + 159 with a factor 7 / 11 / 13) on every axis through the convolution: PLANE and
     FAST paths for the smooth ones, GENERIC for the others; in place in two batches and out of place
  B  the forward spectrum itself (isdf_spectral_rows with ALL half-spectrum points, G = 0 included) and the k-point convolution
     with a kernel table without inversion symmetry (isdf_coulomb_rows_q), every smooth length on every axis
  C  every compile-time-specialised pipelined plane kernel with more than two rounds of planes per workgroup and a ragged
     last round, conv_pipe = 1 and 0, next to square planes of the non-specialised sizes
  D  conv_sub_rows (bit-identical), meshes at and just past the LDS limit of the PLANE path

Every row (hence every plane) holds its own seeded random data.  Failing cases are collected and reported together.

Bounds.  max|got - ref| < 1e-12 max|ref| for the convolutions and 1e-10 max|v| for packed spectral values, the bounds of the older
tests.  For lengths above 128 the own transform has to stay within max(1e-12, 4 x the error of the hipFFT path of the same
library (own_fft = 0) on the same input against the same reference): two transforms of different factorisation differ by a
small constant in the rounding prefactor, not by orders.  That second opinion is measured whenever a long case misses 1e-12, and
always on the largest length of each stage count (a hipFFT plan per mesh is what costs time here, see HIPFFT_ALL).

Measured on an MI355X (errors relative to max|ref|; hipFFT measured for EVERY length above 128, ISDF_FFT_SWEEP_HIPFFT=all):

  path                     largest error           largest own / hipFFT ratio   largest hipFFT error
  PLANE   (convolution)    1.27e-15 (z = 400)      1.60 (y = 270)               1.16e-15
  FAST    (convolution)    1.12e-15 (z = 200)      1.83 (z = 200)               1.16e-15
  GENERIC (convolution)    1.56e-15 (z = 231)      2.29 (z = 231)               1.39e-15
  k-point convolution      8.35e-16 (y = 800)      1.59 (z = 480)               7.55e-16
  spectral rows            7.82e-16 of max|v| (y = 864)
  plane kernels (C)        1.27e-15 convolution, 9.13e-16 spectral rows, 7.15e-16 k-point, 516 planes on 256 CUs

No length needed the 4x clause: every case stays three orders under 1e-12.  Coverage printed: 171 of 171 (axis, radix, stage
position, stage count) on the PLANE and on the FAST path, 9 of 9 (axis, radix) for 7 / 11 / 13.
"""
import os
import time
import numpy as np
import pytest
from oracle import isdf as oisdf

pytestmark = pytest.mark.gpu

A_TRI = np.array([[4.1, 0.3, -0.2], [0.5, 3.7, 0.4], [-0.3, 0.6, 4.4]])
TOL = 1e-12                     # convolutions, relative to max|ref|
TOL_SPEC = 1e-10                # packed spectral values, relative to max|v|
LONG = 128                      # above this length the hipFFT path may serve as a second opinion (the 4x clause)
# A hipFFT plan per mesh costs 0.3 - 0.7 s to make (measured: 314 of the 316 s of sweep A with one for each of its 435 long
# meshes), so by default the second opinion is measured where the clause could matter - whenever the own transform misses 1e-12 -
# and on the largest length of each stage count; ISDF_FFT_SWEEP_HIPFFT=all measures it for every length above LONG (the run
# recorded in the module docstring).
HIPFFT_ALL = os.environ.get('ISDF_FFT_SWEEP_HIPFFT', '') == 'all'
PARTNERS = (2, 3, 4, 5, 6)      # lengths of the other two axes: odd and even line counts, unpaired last line, Nyquist bins


# ---- restatement of the host-side dispatch of fft_conv.hip (to choose meshes and to predict paths; never asserted against
# ---- itself: what ran is read from the profiling labels, what it computed is compared with numpy) --------------------------
BIG = (16, 15, 12, 10, 9, 8, 6, 5, 4, 3, 2)
MAXSTAGE = 12
PLANE_ENTRIES = 10240
LDS_LIMIT = 160 * 1024
PIPED = {64: (8, 8), 72: (9, 8), 80: (10, 8), 96: (12, 8), 100: (10, 10), 108: (12, 9), 120: (12, 10)}
PIPED_Q = (64, 72, 80, 96)


def factorise(n):
    """Radix sequence factorise() picks for n, or None when it rejects n.  2-3-5 smooth: the shortest non-increasing sequence
    of radices <= 16 (depth first, larger radices first), among the shortest the one with the smallest first radix; otherwise
    4, 2, 3, 5 in that order and then 7, 11, 13."""
    m = n
    for p in (2, 3, 5):
        while m % p == 0:
            m //= p
    if m == 1 and n > 1:
        best = [None, MAXSTAGE + 1, 1 << 30]

        def go(rest, maxr, cur):
            if rest == 1:
                mx = cur[0] if cur else 1
                if len(cur) < best[1] or (len(cur) == best[1] and mx < best[2]):
                    best[:] = [tuple(cur), len(cur), mx]
                return
            if len(cur) + 1 > best[1] or len(cur) >= MAXSTAGE:
                return
            for r in BIG:
                if r <= maxr and rest % r == 0:
                    go(rest // r, r, cur + [r])
        go(n, 16, [])
        if best[1] <= MAXSTAGE:
            return best[0]
    seq = []
    for r in (4, 2, 3, 5):
        while n % r == 0 and n > 1:
            seq.append(r)
            n //= r
    for p in (7, 11, 13):
        while n % p == 0:
            seq.append(p)
            n //= p
    return tuple(seq) if n == 1 and len(seq) <= MAXSTAGE else None


def smooth(seq):
    return not any(r in (7, 11, 13) for r in seq)


def plane_lds_bytes(n1, n2):
    """LDS bytes of the real (y, z) plane pass, 0 when the plane does not fit (plane_geometry, real form)."""
    n2h, npair = n2 // 2 + 1, (n1 + 1) // 2
    Lz = npair
    while Lz % 16 != 1:
        Lz += 1
    bufsz = max(n2 * Lz, n1 * n2h)
    if max(n2 * npair, n1 * n2h) > PLANE_ENTRIES or n1 * n2 > 2 * PLANE_ENTRIES:
        return 0
    nbytes = 16 * (bufsz + n1 + n2)
    return nbytes if nbytes <= LDS_LIMIT else 0


def plane_c2c_lds_bytes(n1, n2):
    """LDS bytes of the complex plane pass of the k-point form, 0 when it does not fit (plane_geometry, complex form)."""
    if n1 * n2 > PLANE_ENTRIES:
        return 0
    Lz = n1
    while Lz % 16 != 1:
        Lz += 1
    nbytes = 16 * (max(n2 * Lz, n1 * n2) + n1 + n2)
    return nbytes if nbytes <= LDS_LIMIT else 0


def predict_path(mesh, own_fft=2):
    """'plane' | 'fast' | 'generic' | 'hipfft': the transform isdf_coulomb_rows takes (conv_rows_own_supported + conv_rows_own)."""
    seqs = [factorise(int(n)) if 1 <= n <= 1024 else None for n in mesh]
    if own_fft == 0 or any(s is None for s in seqs):
        return 'hipfft'
    if all(smooth(s) for s in seqs):
        return 'plane' if own_fft == 2 and plane_lds_bytes(mesh[1], mesh[2]) else 'fast'
    return 'generic'


def predict_q_own(mesh):
    """Whether the k-point convolution takes the own transform (conv_rows_q_own_supported with own_fft != 0)."""
    seqs = [factorise(int(n)) if 2 <= n <= 1024 else None for n in mesh]
    return all(s is not None and smooth(s) for s in seqs) and bool(plane_lds_bytes(mesh[1], mesh[2])) \
        and bool(plane_c2c_lds_bytes(mesh[1], mesh[2]))


def stage_keys(mesh):
    """{(axis, radix, stage position, stage count)} of the transforms a mesh runs."""
    return {(d, r, i, len(factorise(n))) for d, n in enumerate(mesh) for i, r in enumerate(factorise(n))}


ACCEPTED = [n for n in range(2, 1025) if factorise(n) is not None]
SMOOTH = [n for n in ACCEPTED if smooth(factorise(n))]
GENERIC = [n for n in ACCEPTED if not smooth(factorise(n))]
# the largest length of each stage count, smooth and generic: where the second opinion is always measured
SECOND_OPINION = {max(n for n in lst if len(factorise(n)) == k) for lst in (SMOOTH, GENERIC) for k in {len(factorise(n)) for n in lst}}
LABEL = {'plane': 'coulomb_conv_own_3pass[byte]', 'fast': 'coulomb_conv_own_5pass[byte]', 'generic': 'coulomb_conv_own_5pass[byte]',
         'hipfft': 'coulomb_conv_d2z_mul_z2d[byte]'}
LABEL_Q = {True: 'coulomb_conv_q_own[byte]', False: 'coulomb_conv_z2z[byte]'}
LABEL_SPEC = 'spectral_rows_own[byte]'


def sweep_mesh(d, n, i, fits=None):
    """Mesh with n on axis d; the partners rotate through PARTNERS with the position i of n in its list and with the axis.  With
    ``fits`` the first rotation whose mesh satisfies it (a long z axis leaves the PLANE path only a y axis of 2: the pitch of
    the z stage is rounded up to 1 mod 16), None when no partner pair does."""
    for k in range(25):
        mesh = [PARTNERS[(i + d + k) % 5], PARTNERS[(2 * i + d + 1 + k // 5) % 5], PARTNERS[(3 * i + 2 * d + 3 + k) % 5]]
        mesh[d] = n
        if fits is None or fits(tuple(mesh)):
            return tuple(mesh)
    return None


def _is_plane(mesh):
    return predict_path(mesh, 2) == 'plane'


def test_restated_dispatch_counts():
    """The restatement agrees with the counts of the product code: 86 smooth and 159 generic lengths up to 1024, the radix pairs
    of the specialised planes, every PLANE / k-point sweep mesh predicted for its path."""
    assert len(SMOOTH) == 86 and len(GENERIC) == 159
    assert all(factorise(n) == PIPED[n] for n in PIPED)
    assert factorise(17) is None and factorise(7 * 11 * 13) == (7, 11, 13) and factorise(128) == (16, 8) and factorise(28) == (4, 7)
    for d in range(3):
        for i, n in enumerate(SMOOTH):
            mesh = sweep_mesh(d, n, i, _is_plane)
            assert mesh is not None and predict_path(mesh, 1) == 'fast', (d, n)
        for i, n in enumerate(GENERIC):
            assert predict_path(sweep_mesh(d, n, i), 2) == 'generic'


@pytest.fixture(scope='module')
def be():
    from pyscf_isdf_amd.backend import HipBackend
    b = HipBackend(0)
    b.prof_enable(True)
    yield b
    b.prof_enable(False)
    b.prof_reset()
    for key, val in (('own_fft', 2), ('conv_pipe', 1), ('conv_sub_rows', 0)):
        b.set_option(key, val)
    b.release_workspace()


def _labels(be, fn):
    """Run fn and return its result and the profiling labels of the launches it made."""
    be.prof_reset()
    out = fn()
    return out, set(be.prof_results())


def _conv(be, rows, mesh, batch, own_fft=2, out_of_place=False):
    """isdf_coulomb_rows on a fresh device copy: (result, input afterwards, labels)."""
    be.set_option('own_fft', own_fft)
    try:
        d = be.to_device(rows)
        o = be.empty(rows.shape) if out_of_place else None
        _, labels = _labels(be, lambda: be.coulomb_rows(d, np.asarray(mesh), A_TRI, batch, out=o))
        return be.to_host(d if o is None else o), be.to_host(d), labels
    finally:
        be.set_option('own_fft', 2)


def _conv_q(be, rows, mesh, tab, own_fft=2):
    be.set_option('own_fft', own_fft)
    try:
        re, im = be.empty(rows.shape), be.empty(rows.shape)
        _, labels = _labels(be, lambda: be.coulomb_rows_q(be.to_device(rows), np.asarray(mesh), be.to_device(tab), re, im))
        return be.to_host(re) + 1j * be.to_host(im), labels
    finally:
        be.set_option('own_fft', 2)


def _conv_q_ref(rows, mesh, tab):
    z = np.fft.fftn(rows.reshape(len(rows), *mesh), axes=(1, 2, 3)) * tab.reshape(mesh)
    return np.fft.ifftn(z, axes=(1, 2, 3)).reshape(rows.shape)


def _spectral(be, rows, mesh, batch, seed):
    """isdf_spectral_rows over a seeded permutation of ALL half-spectrum points (G = 0 included) with seeded positive scales, a
    leading dimension beyond 2 npts and a sentinel row behind the rows.  Returns (list of complaints, error relative to max|v|)."""
    import torch
    mesh = tuple(int(n) for n in mesh)
    nrow = len(rows)
    gc = mesh[0] * mesh[1] * (mesh[2] // 2 + 1)
    rng = np.random.default_rng(seed)
    idx = rng.permutation(gc).astype(np.int32)
    scale = rng.random(gc) + 0.5
    ldx = 2 * gc + 6
    sentinel = -777.25
    X = torch.full((nrow + 1, ldx), sentinel, dtype=torch.float64, device=be.device)
    d_rows, d_idx, d_scale = be.to_device(rows), be.to_device(idx), be.to_device(scale)
    _, labels = _labels(be, lambda: be.spectral_rows(d_rows, np.asarray(mesh), d_idx, d_scale, X[:nrow], batch=batch))
    x = be.to_host(X)
    v = np.fft.rfftn(rows.reshape(nrow, *mesh), axes=(1, 2, 3)).reshape(nrow, gc)[:, idx] * scale
    bad = []
    if labels != {LABEL_SPEC}:
        bad.append('labels %s' % sorted(labels))
    err = max(abs(x[:nrow, 0:2 * gc:2] - v.real).max(), abs(x[:nrow, 1:2 * gc:2] - v.imag).max()) / abs(v).max()
    if not err < TOL_SPEC:
        bad.append('spectrum off by %.2e of max|v|' % err)
    if abs(x[:nrow, 2 * gc:]).max() != 0.0:
        bad.append('padding columns not zero')
    if not np.all(x[nrow] == sentinel):
        bad.append('sentinel row overwritten')
    if not np.array_equal(be.to_host(d_rows), rows):
        bad.append('input rows changed')
    return bad, err


class _Stats:
    """Largest error per path and the comparison with the hipFFT path for the long lengths."""

    def __init__(self):
        self.err, self.ratio, self.hip, self.needed_4x = {}, {}, {}, []

    def add(self, path, case, err, hip_err=None):
        if err > self.err.get(path, (0.0, None))[0]:
            self.err[path] = (err, case)
        if hip_err is not None:
            self.hip[path] = max(self.hip.get(path, 0.0), hip_err)
            r = err / max(hip_err, 1e-300)
            if r > self.ratio.get(path, (0.0, None))[0]:
                self.ratio[path] = (r, case)
            if err >= TOL:
                self.needed_4x.append((path, case, err, hip_err))

    def report(self, title):
        print('\n' + title)
        for path in sorted(self.err):
            line = '  %-8s largest error %.2e of max|ref| at %s' % (path, self.err[path][0], self.err[path][1])
            if path in self.ratio:
                line += '; largest own / hipFFT ratio %.2f at %s (largest hipFFT error %.2e)' % (self.ratio[path] + (self.hip[path],))
            print(line)
        print('  lengths that needed the 4x clause: %s' % (self.needed_4x or 'none'))


def _within(err, hip_err):
    """The bound: 1e-12 of max|ref|; for the long lengths 4 x the hipFFT path's error on the same input if that is larger."""
    return err < TOL or (hip_err is not None and err <= 4.0 * hip_err)


def test_A_length_sweep_convolution(be):
    """Every accepted length on every axis through isdf_coulomb_rows against oisdf.coulomb_V on a triclinic lattice: PLANE
    (own_fft = 2) and FAST (own_fft = 1) for the 86 smooth lengths, GENERIC for the 159 with a factor 7 / 11 / 13; 5 rows in place in
    batches of 3 + 2 and out of place in one batch; the path asserted from the profiling label.  At the end the sweep must have
    reached every (axis, radix, stage position, stage count) factorise() produces for smooth lengths on both smooth paths and
    the radices 7, 11, 13 on every axis of the generic one."""
    fails, stats = [], _Stats()
    cover = {'plane': set(), 'fast': set(), 'generic': set()}
    nrow, t0, t_hip, ncase, nhip = 5, time.time(), 0.0, 0, 0
    for d in range(3):
        for lengths in (SMOOTH, GENERIC):
            for i, n in enumerate(lengths):
                mesh = sweep_mesh(d, n, i, _is_plane if lengths is SMOOTH else None)
                G = int(np.prod(mesh))
                rows = np.random.default_rng([d, n]).standard_normal((nrow, G))
                ref = oisdf.coulomb_V(rows, A_TRI, np.asarray(mesh))
                scale = abs(ref).max()
                hip = {}

                def hip_err():              # the hipFFT path on the same input against the same reference, measured once
                    if 'err' not in hip:
                        t1 = time.time()
                        got0, _, labels0 = _conv(be, rows, mesh, nrow, own_fft=0)
                        hip['t'] = time.time() - t1
                        hip['err'] = abs(got0 - ref).max() / scale
                        if labels0 != {LABEL['hipfft']}:
                            fails.append(('hipfft', mesh, 'labels %s' % sorted(labels0)))
                    return hip['err']
                if n > LONG and (HIPFFT_ALL or n in SECOND_OPINION):
                    hip_err()
                for path in (('plane', 'fast') if lengths is SMOOTH else ('generic',)):
                    own = 1 if path == 'fast' else 2
                    assert predict_path(mesh, own) == path, (mesh, path)
                    ncase += 1
                    got, _, labels = _conv(be, rows, mesh, 3, own_fft=own)
                    got2, kept, labels2 = _conv(be, rows, mesh, nrow, own_fft=own, out_of_place=True)
                    if labels != {LABEL[path]} or labels2 != {LABEL[path]}:
                        fails.append((path, mesh, 'axis %d' % d, 'labels %s %s' % (sorted(labels), sorted(labels2))))
                        continue
                    cover[path] |= stage_keys(mesh)
                    err = max(abs(got - ref).max(), abs(got2 - ref).max()) / scale
                    if not err < TOL and n > LONG:
                        hip_err()
                    stats.add(path, 'n=%d axis %d' % (n, d), err, hip.get('err'))
                    if not _within(err, hip.get('err')):
                        fails.append((path, mesh, 'axis %d' % d, 'error %.2e of max|ref|' % err, 'hipFFT %s' % hip.get('err')))
                    if not np.array_equal(kept, rows):
                        fails.append((path, mesh, 'axis %d' % d, 'out of place changed its input'))
                t_hip += hip.get('t', 0.0)
                nhip += 'err' in hip
    stats.report('A: convolution sweep, %d cases in %.1f s (%.1f s of it the hipFFT second opinion on %d meshes)'
                 % (ncase, time.time() - t0, t_hip, nhip))
    exact = {(d, r, j, len(factorise(n))) for d in range(3) for n in SMOOTH for j, r in enumerate(factorise(n))}
    for path in ('plane', 'fast'):
        print('  %-8s (axis, radix, stage position, stage count) reached: %d of %d' % (path, len(cover[path] & exact), len(exact)))
        missing = exact - cover[path]
        if missing:
            fails.append((path, 'coverage', sorted(missing)))
        if {(k[0], k[1]) for k in cover[path]} < {(dd, r) for dd in range(3) for r in BIG}:
            fails.append((path, 'not all 11 radices on all 3 axes'))
    got_generic = {(k[0], k[1]) for k in cover['generic'] if k[1] in (7, 11, 13)}
    print('  generic  (axis, radix) reached for 7 / 11 / 13: %d of 9' % len(got_generic))
    if len(got_generic) != 9:
        fails.append(('generic', 'coverage', sorted(got_generic)))
    assert not fails, '%d failing cases:\n%s' % (len(fails), '\n'.join(map(str, fails[:60])))


def test_B_forward_spectrum(be):
    """The raw forward spectrum (isdf_spectral_rows, PLANE path) of every smooth length on every axis against np.fft.rfftn, all
    half-spectrum points in a seeded order with seeded scales: sees a mirrored index, a conjugated spectrum, the DC bin and both
    Nyquist bins, which a convolution with a symmetric real table that is zero at G = 0 cannot.  5 rows in batches of 3 + 2."""
    fails, worst, t0 = [], (0.0, ''), time.time()
    for d in range(3):
        for i, n in enumerate(SMOOTH):
            mesh = sweep_mesh(d, n, i, _is_plane)
            if not be.spectral_supported(np.asarray(mesh), 3):
                fails.append((mesh, 'axis %d' % d, 'spectral_supported says no'))
                continue
            rows = np.random.default_rng([7, d, n]).standard_normal((5, int(np.prod(mesh))))
            bad, err = _spectral(be, rows, mesh, 3, [11, d, n])
            worst = max(worst, (err, 'n=%d axis %d' % (n, d)))
            if bad:
                fails.append((mesh, 'axis %d' % d, bad))
    print('\nB: forward spectrum, %d cases in %.1f s; largest error %.2e of max|v| at %s' % (3 * len(SMOOTH), time.time() - t0, *worst))
    assert not fails, '%d failing cases:\n%s' % (len(fails), '\n'.join(map(str, fails[:60])))


def test_B_kpoint_convolution_sweep(be):
    """isdf_coulomb_rows_q (real rows, full kernel table WITHOUT inversion symmetry, complex result) of every smooth length on
    every axis against ifftn(tab * fftn(rows)), real and imaginary parts; the own transform must have run wherever the restated
    predicate says so (every mesh of this sweep: all lengths on x and y, up to 540 on z, where the complex plane's pitch of
    1 mod 16 lines no longer fits LDS beside even a y axis of 2); hipFFT Z2Z (own_fft = 0) is the second opinion for the long lengths."""
    fails, stats, t0, ncase, left_out = [], _Stats(), time.time(), 0, []
    for d in range(3):
        for i, n in enumerate(SMOOTH):
            mesh = sweep_mesh(d, n, i, predict_q_own)
            if mesh is None:            # no partner >= 2 lets the complex plane fit LDS (z above 540): hipFFT's by design
                left_out.append((d, n))
                continue
            ncase += 1
            rng = np.random.default_rng([5, d, n])
            G = int(np.prod(mesh))
            rows, tab = rng.standard_normal((5, G)), rng.random(G) + 0.1
            ref = _conv_q_ref(rows, mesh, tab)
            scale = abs(ref).max()
            hip = {}

            def hip_err():
                if 'err' not in hip:
                    got0, labels0 = _conv_q(be, rows, mesh, tab, own_fft=0)
                    hip['err'] = abs(got0 - ref).max() / scale
                    if labels0 != {LABEL_Q[False]}:
                        fails.append(('hipfft', mesh, 'labels %s' % sorted(labels0)))
                return hip['err']
            if n > LONG and (HIPFFT_ALL or n in SECOND_OPINION):
                hip_err()
            got, labels = _conv_q(be, rows, mesh, tab)
            if labels != {LABEL_Q[True]}:
                fails.append((mesh, 'axis %d' % d, 'labels %s' % sorted(labels)))
                continue
            err = max(abs(got.real - ref.real).max(), abs(got.imag - ref.imag).max()) / scale
            if not err < TOL and n > LONG:
                hip_err()
            stats.add('kpoint', 'n=%d axis %d' % (n, d), err, hip.get('err'))
            if not _within(err, hip.get('err')):
                fails.append((mesh, 'axis %d' % d, 'error %.2e of max|ref|' % err, 'hipFFT %s' % hip.get('err')))
    stats.report('B: k-point convolution sweep, %d cases in %.1f s' % (ncase, time.time() - t0))
    print('  (axis, length) outside the own k-point transform for every partner: %s' % left_out)
    assert all(d == 2 and n > 540 for d, n in left_out) and ncase == 3 * len(SMOOTH) - len(left_out) >= 240
    assert not fails, '%d failing cases:\n%s' % (len(fails), '\n'.join(map(str, fails[:60])))


def _looping_rows(n0):
    """Rows such that rows * n0 planes exceed twice the CU count without being a multiple of it: every persistent workgroup
    walks at least two planes (prefetch hand-over) and the last round is ragged."""
    import torch
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    rows = 2 * ncu // n0 + 2
    while rows * n0 % ncu == 0 or rows * n0 <= 2 * ncu:
        rows += 1
    return rows, ncu


# square planes: the seven specialised sizes, and 90 / 128 for the default: branch of the switches at a comparable size
PLANE_SIZES = (64, 72, 80, 96, 100, 108, 120, 90, 128)
# k-point form: the four specialised sizes and 90 for the default: branch.  100^2 is named in conv_rows_q_own as the size that is
# not piped; in fact plane_c2c_lds_bytes() declines it (100 lines pitch 113: 11 300 + 200 entries of 10 240), so it takes hipFFT
# under either conv_pipe - kept here so that a change of that predicate meets a reference.
PLANE_SIZES_Q = (64, 72, 80, 96, 100, 90)


def test_C_plane_kernels_loop_over_planes(be):
    """Gamma convolution and spectral rows on (3, N, N) in ONE batch whose plane count exceeds twice the CU count and is not a
    multiple of it, conv_pipe = 1 (persistent workgroups, next plane prefetched) and 0 (one workgroup per plane), both against
    oisdf.coulomb_V / np.fft.rfftn; and a small case with fewer planes than CUs."""
    fails, stats, t0 = [], _Stats(), time.time()
    n0 = 3
    big, ncu = _looping_rows(n0)
    try:
        for N in PLANE_SIZES:
            mesh = (n0, N, N)
            assert predict_path(mesh, 2) == 'plane' and (factorise(N) == PIPED[N] if N in PIPED else len(factorise(N)) == 2)
            for nrow in (big, 2):
                assert (nrow * n0 > 2 * ncu and nrow * n0 % ncu) if nrow == big else nrow * n0 < ncu
                rows = np.random.default_rng([3, N, nrow]).standard_normal((nrow, n0 * N * N))
                ref = oisdf.coulomb_V(rows, A_TRI, np.asarray(mesh))
                scale = abs(ref).max()
                for pipe in (1, 0):
                    be.set_option('conv_pipe', pipe)
                    case = 'N=%d rows=%d (%d planes, %d CUs) conv_pipe=%d' % (N, nrow, nrow * n0, ncu, pipe)
                    got, _, labels = _conv(be, rows, mesh, nrow)
                    err = abs(got - ref).max() / scale
                    stats.add('conv pipe=%d' % pipe, case, err)
                    if labels != {LABEL['plane']} or not err < TOL:
                        fails.append((case, 'convolution', sorted(labels), 'error %.2e of max|ref|' % err))
                    bad, err = _spectral(be, rows, mesh, nrow, [13, N, nrow])
                    stats.add('spec pipe=%d' % pipe, case, err)
                    if bad:
                        fails.append((case, 'spectral rows', bad))
    finally:
        be.set_option('conv_pipe', 1)
    stats.report('C: plane kernels, Gamma form, %d planes on %d CUs, %.1f s' % (big * n0, ncu, time.time() - t0))
    assert not fails, '%d failing cases:\n%s' % (len(fails), '\n'.join(map(str, fails[:60])))


def test_C_plane_kernels_loop_over_planes_kpoint(be):
    """The same for the k-point form (real forward plane pass, complex inverse plane pass) through isdf_coulomb_rows_q with a
    kernel table without inversion symmetry, against numpy; the transform that ran (own, or hipFFT for 100^2) asserted from the
    label."""
    fails, stats, t0 = [], _Stats(), time.time()
    n0 = 3
    big, ncu = _looping_rows(n0)
    try:
        for N in PLANE_SIZES_Q:
            mesh = (n0, N, N)
            own = predict_q_own(mesh)
            assert own == (N != 100)
            for nrow in (big, 2):
                rng = np.random.default_rng([4, N, nrow])
                rows, tab = rng.standard_normal((nrow, n0 * N * N)), rng.random(n0 * N * N) + 0.1
                ref = _conv_q_ref(rows, mesh, tab)
                scale = abs(ref).max()
                for pipe in (1, 0):
                    be.set_option('conv_pipe', pipe)
                    case = 'N=%d rows=%d (%d planes, %d CUs) conv_pipe=%d' % (N, nrow, nrow * n0, ncu, pipe)
                    got, labels = _conv_q(be, rows, mesh, tab)
                    err = max(abs(got.real - ref.real).max(), abs(got.imag - ref.imag).max()) / scale
                    stats.add('kpoint pipe=%d' % pipe, case, err)
                    if labels != {LABEL_Q[own]} or not err < TOL:
                        fails.append((case, sorted(labels), 'error %.2e of max|ref|' % err))
    finally:
        be.set_option('conv_pipe', 1)
    stats.report('C: plane kernels, k-point form, %d planes on %d CUs, %.1f s' % (big * n0, ncu, time.time() - t0))
    assert not fails, '%d failing cases:\n%s' % (len(fails), '\n'.join(map(str, fails[:60])))


def test_D_sub_batches_are_bit_identical(be):
    """conv_sub_rows = 7 on a batch of 20 rows (sub-batches 7 + 7 + 6) against conv_sub_rows = 0 on the PLANE path, piped and
    not: rows are independent in every pass, so the results are bit-identical; both match the oracle."""
    try:
        for mesh in ((3, 64, 64), (5, 12, 10), (4, 27, 25)):
            assert predict_path(mesh, 2) == 'plane'
            rows = np.random.default_rng(list(mesh)).standard_normal((20, int(np.prod(mesh))))
            ref = oisdf.coulomb_V(rows, A_TRI, np.asarray(mesh))
            out = {}
            for sub in (0, 7):
                be.set_option('conv_sub_rows', sub)
                out[sub], _, labels = _conv(be, rows, mesh, 20)
                assert labels == {LABEL['plane']}, (mesh, sub, labels)
                assert abs(out[sub] - ref).max() < TOL * abs(ref).max(), (mesh, sub)
            assert np.array_equal(out[0], out[7]), (mesh, abs(out[0] - out[7]).max())
    finally:
        be.set_option('conv_sub_rows', 0)


def _plane_limit_meshes():
    """Meshes (2, n1, n2) at the LDS limit of the PLANE path and just past it.  plane_lds_bytes() asks for
    max(n2 * ceil(n1 / 2), n1 * (n2 / 2 + 1)) <= PLANE_ENTRIES = 10240 complex entries, n1 * n2 <= 20480 reals and
    16 * (bufsz + n1 + n2) <= 160 KB with bufsz = max(n2 * Lz, n1 * (n2 / 2 + 1)), Lz = ceil(n1 / 2) rounded up to 1 mod 16.  The
    last condition is the binding one (bufsz + n1 + n2 <= 10240 covers the other two), so the edge is searched in that sum: the
    three largest fitting smooth planes in each orientation (n1 > n2, n1 < n2: there the index split (int)((c + 0.5f) / n) runs at
    its largest c) and the three smallest that do not fit, which must take the 5-pass form under own_fft = 2."""
    fit, nofit = [], []
    for n1 in SMOOTH:
        for n2 in SMOOTH:
            if n1 == n2 or min(n1, n2) < 16 or n1 * n2 > 4 * PLANE_ENTRIES:
                continue
            npair, n2h = (n1 + 1) // 2, n2 // 2 + 1
            Lz = npair
            while Lz % 16 != 1:
                Lz += 1
            total = max(n2 * Lz, n1 * n2h) + n1 + n2
            (fit if plane_lds_bytes(n1, n2) else nofit).append((total, n1, n2))
    fit.sort(reverse=True)
    nofit.sort()
    pick = lambda lst, cond: [(2, n1, n2) for _, n1, n2 in lst if cond(n1, n2)][:3]
    inside = pick(fit, lambda a, b: a > b) + pick(fit, lambda a, b: a < b)
    outside = pick(nofit, lambda a, b: a > b) + pick(nofit, lambda a, b: a < b) + [(2, 144, 144), (2, 100, 200), (2, 200, 100)]
    return inside, outside


def test_D_plane_limit(be):
    """Meshes at the PLANE path's LDS limit run the 3-pass form, those just past it silently take the FAST 5-pass form under
    own_fft = 2 - both asserted from the label, both against the oracle (and the spectral rows against numpy where supported)."""
    inside, outside = _plane_limit_meshes()
    assert len(inside) == 6 and all(predict_path(m, 2) == 'plane' for m in inside)
    assert all(predict_path(m, 2) == 'fast' for m in outside)
    fails = []
    for mesh in inside + outside:
        path = predict_path(mesh, 2)
        rows = np.random.default_rng(list(mesh)).standard_normal((5, int(np.prod(mesh))))
        ref = oisdf.coulomb_V(rows, A_TRI, np.asarray(mesh))
        got, _, labels = _conv(be, rows, mesh, 3)
        err = abs(got - ref).max() / abs(ref).max()
        print('D: plane limit %s -> %s, error %.2e of max|ref|' % (mesh, path, err))
        if labels != {LABEL[path]} or not err < TOL:
            fails.append((mesh, path, sorted(labels), 'error %.2e' % err))
        if be.spectral_supported(np.asarray(mesh), 3) != (path == 'plane'):
            fails.append((mesh, 'spectral_supported disagrees with the PLANE path'))
        elif path == 'plane':
            bad, _ = _spectral(be, rows, mesh, 3, list(mesh))
            if bad:
                fails.append((mesh, 'spectral rows', bad))
    assert not fails, '%d failing cases:\n%s' % (len(fails), '\n'.join(map(str, fails)))
