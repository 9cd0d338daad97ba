"""SHA-256 of the own FFT's outputs on a fixed list of seeded cases, one line per case with the path read from the profiling
label: run once per tree (--lib PATH loads another build of the library), each in a process of its own, and compare the two
listings line for line.  stderr carries the GENERIC cases' errors against the sweep's reference.
The cases are the smallest shapes that reach every kernel of fft_conv.hip and every edge (odd line counts, no Nyquist bin,
ragged rounds of the persistent workgroups, narrow tiles, sub-batches).  Data and calls are those of
tests/test_gpu_fft_sweep.py (_conv, _conv_q, _labels, _looping_rows); spectral() below builds its own arguments in the way of
the sweep's _spectral, which checks the output but does not return it, and cuts the point list to an odd npts."""
import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
ap = argparse.ArgumentParser()
ap.add_argument('--lib', default=None, help='libmi355_isdf.so to load instead of the tree\'s own')
args = ap.parse_args()
import pyscf_isdf_amd.lib as isdf_lib
if args.lib:
    isdf_lib.LIB_PATH = os.path.abspath(args.lib)
import numpy as np
import torch
import test_gpu_fft_sweep as sw
from pyscf_isdf_amd.backend import HipBackend

be = HipBackend(0)
be.prof_enable(True)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def show(case, labels, *arrays):
    print('%-64s %-32s %s' % (case, '+'.join(sorted(labels)), ' '.join(sha(a) for a in arrays)), flush=True)


def rows_of(mesh, nrow, seed):
    return np.random.default_rng(seed).standard_normal((nrow, int(np.prod(mesh))))


def conv(name, mesh, nrow, own_fft=2, out_of_place=False, **options):
    for k, v in options.items():
        be.set_option(k, v)
    rows = rows_of(mesh, nrow, [1] + list(mesh))
    try:
        got, _, labels = sw._conv(be, rows, mesh, nrow, own_fft=own_fft, out_of_place=out_of_place)
    finally:
        for k in options:
            be.set_option(k, {'conv_pipe': 1, 'conv_sub_rows': 0}[k])
    show('%s %s rows=%d own_fft=%d%s %s' % (name, mesh, nrow, own_fft, ' out-of-place' if out_of_place else '',
                                            ' '.join('%s=%d' % kv for kv in sorted(options.items()))), labels, got)
    if name == 'generic':         # on stderr, so that the listings stay comparable: the error against the sweep's reference
        ref = sw.oisdf.coulomb_V(rows, sw.A_TRI, np.asarray(mesh))
        print('generic %s error %.4e of max|ref|' % (mesh, abs(got - ref).max() / abs(ref).max()), file=sys.stderr, flush=True)


def spectral(mesh, nrow):
    """All half-spectrum points, an odd npts, a leading dimension with padding (the arguments of the sweep's _spectral)."""
    gc = mesh[0] * mesh[1] * (mesh[2] // 2 + 1)
    rng = np.random.default_rng([2] + list(mesh))
    npts = gc if gc % 2 else gc - 1
    idx = rng.permutation(gc).astype(np.int32)[:npts]
    scale = (rng.random(gc) + 0.5)[:npts]
    ldx = 2 * npts + 6
    X = torch.full((nrow + 1, ldx), -777.25, dtype=torch.float64, device=be.device)
    d_rows, d_idx, d_scale = be.to_device(rows_of(mesh, nrow, [3] + list(mesh))), be.to_device(idx), be.to_device(scale)
    _, labels = sw._labels(be, lambda: be.spectral_rows(d_rows, np.asarray(mesh), d_idx, d_scale, X[:nrow], batch=nrow))
    show('spectral %s rows=%d npts=%d ldx=%d' % (mesh, nrow, npts, ldx), labels, be.to_host(X))


def conv_q(mesh, nrow, **options):
    for k, v in options.items():
        be.set_option(k, v)
    try:
        rng = np.random.default_rng([4] + list(mesh))
        rows, tab = rng.standard_normal((nrow, int(np.prod(mesh)))), rng.random(int(np.prod(mesh))) + 0.1
        got, labels = sw._conv_q(be, rows, mesh, tab)
    finally:
        for k in options:
            be.set_option(k, 1)
    show('kpoint %s rows=%d %s' % (mesh, nrow, ' '.join('%s=%d' % kv for kv in sorted(options.items()))), labels, got.real, got.imag)


# PLANE, one workgroup per plane: odd n1 (unpaired last line), odd n2 (no Nyquist bin), a composite radix on each plane axis
for mesh in ((3, 5, 8), (4, 6, 9), (2, 9, 15)):
    for oop in (False, True):
        conv('plane', mesh, 3, out_of_place=oop)
# PLANE, persistent workgroups: more than two rounds per workgroup and a ragged last round, piped and not
for N in (64, 72, 80, 96, 100, 108, 120):
    big, ncu = sw._looping_rows(2)
    for pipe in (1, 0):
        conv('plane-loop', (2, N, N), big, conv_pipe=pipe)
# FAST: line count 8 on z, line count 2, a narrow x tile; then the fall from own_fft = 2 when the plane does not fit (130 = 2 x 5 x 13:
# the five passes it falls to are the GENERIC ones)
for mesh in ((4, 6, 10), (5, 3, 200), (2, 2, 1024), (384, 2, 3)):
    conv('fast', mesh, 3, own_fft=1)
conv('generic', (6, 5, 130), 3, own_fft=2)
conv('fast', (2, 150, 150), 3, own_fft=2)      # smooth, but the 150 x 150 plane does not fit: own_fft = 2 falls to FAST
# GENERIC (the last mesh: radices 4, 3 and 5 each followed by further stages, so with output twiddles; 2 is in the second)
for mesh in ((7, 11, 13), (14, 22, 26), (3, 4, 231), (2, 2, 1001), (49, 3, 5), (28, 35, 420)):
    conv('generic', mesh, 3)
# spectral rows
spectral((3, 5, 8), 3)
spectral((2, 64, 64), 3)
# k-point form, table without inversion symmetry
conv_q((3, 5, 8), 3)
conv_q((2, 64, 64), sw._looping_rows(2)[0])
conv_q((2, 100, 100), 3)
conv_q((2, 100, 100), 3, conv_pipe=0)
conv_q((2, 96, 96), sw._looping_rows(2)[0])
# sub-batches
conv('sub-batches', (4, 6, 10), 5, conv_sub_rows=2)
