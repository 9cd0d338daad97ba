"""The host driver's backend calls, in order, and a digest of what it computes: the checker backend (tests/oracle_backend.py) runs
the whole build and get_jk on the CPU behind a recording wrapper, case by case.  Per case the listing holds every backend and
communicator call with its arguments (tensors as dtype[shape]/strides@storage offset, numpy arrays as dtype[shape] and the head
of their SHA-256, scalars as they are; what a call returns when that is a number), every warning raised, a SHA-256 over the call
lines, and the SHA-256 of ip, W, vj and vk (vk with a get_jk(omega=0.4) appended, except with robust_k) next to bj_check
(hexadecimal), reg_used, fit_route_used, n_panels, w_spectral_fraction, the fit state's kind and the timing keys.

Run once per tree, each in a process of its own, and compare the two listings line for line: a refactor of the host
orchestration leaves every line as it was.  Uses the public API only, so it runs unchanged in a checkout of an earlier commit.
Allocation and transfer calls (empty, zeros, to_device, to_host, free_bytes, empty_cache) are left OUT of the listing and of its
digest unless --all is given: they carry no arithmetic, and a buffer's lifetime is the driver's business.  The setters of the
Coulomb kernel (set_coulomb_omega / _cutoff / _ws) are not listed as calls either: every call made while another kernel than the
plain one is set carries that state instead ({omega=...}; not the stream, event and synchronise calls, which launch nothing).  The communicator's tensors are
listed without their storage offsets (which slot of an exchange buffer a piece travels in is plumbing).

Cases: the primitive diamond cell of tests/test_multirank_cpu.py (gth-szv, mesh (10, 9, 8), c_isdf 3, bj_check_tol 1e-6) on one
process through the single-GPU driver and, with force_sharded, through the grid-sharded one; two 2x1x1 k-point cases."""
import argparse
import hashlib
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
ap = argparse.ArgumentParser()
ap.add_argument('--out', default=None, help='write the listing to this file instead of the standard output')
ap.add_argument('--all', action='store_true', help='list the allocation and transfer calls too')
ap.add_argument('--digests', action='store_true', help='per case only the two digest lines')
ap.add_argument('--case', action='append', default=None, help='run only this case (may be given several times)')
args = ap.parse_args()
import numpy as np
import torch
import cells
from oracle_backend import OracleBackend
from pyscf_isdf_amd.isdf import ISDF
from pyscf_isdf_amd.parallel import Comm

KERNEL_SETTERS = ('set_coulomb_omega', 'set_coulomb_cutoff', 'set_coulomb_ws')
KERNEL_STATE = {}
NO_KERNEL = ('synchronize', 'new_stream', 'on_stream', 'record_event', 'wait_event')
QUIET = ('empty', 'zeros', 'to_device', 'to_host', 'free_bytes', 'empty_cache')


def describe(x, offsets=True):
    if isinstance(x, torch.Tensor):
        return '%s[%s]/%s%s' % (str(x.dtype).replace('torch.', ''), ','.join(str(n) for n in x.shape),
                                ','.join(str(n) for n in x.stride()), '@%d' % x.storage_offset() if offsets else '')
    if isinstance(x, np.ndarray):
        return 'np.%s[%s]#%s' % (x.dtype, ','.join(str(n) for n in x.shape), hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()[:12])
    if isinstance(x, (list, tuple)):
        return '[' + ', '.join(describe(v, offsets) for v in x) + ']'
    if isinstance(x, dict):
        return '{' + ', '.join('%s: %s' % (k, describe(v)) for k, v in sorted(x.items())) + '}'
    if isinstance(x, (np.floating, float)):
        return float(x).hex()
    if x is None or isinstance(x, (bool, int, np.integer, str)):
        return repr(x if not isinstance(x, np.integer) else int(x))
    return '<%s>' % type(x).__name__


class Recorder:
    """Forwards every attribute of `target`; calls of its methods are appended to `lines` as 'who.method(arguments) -> value'.  An
    attribute the target does not have is missing here too (the driver asks hasattr for optional kernels)."""

    def __init__(self, target, who, lines):
        self.__dict__.update(_target=target, _who=who, _lines=lines)

    def __getattr__(self, name):
        attr = getattr(self._target, name)
        if not callable(attr) or name.startswith('_'):
            return attr

        def call(*a, **kw):
            out = attr(*a, **kw)
            if name in KERNEL_SETTERS:
                KERNEL_STATE[name[len('set_coulomb_'):]] = describe(a[0]) if a[0] else None
            elif args.all or name not in QUIET:
                off = self._who != 'comm'
                text = ', '.join([describe(v, off) for v in a] + ['%s=%s' % (k, describe(v, off)) for k, v in sorted(kw.items())])
                ret = ' -> ' + describe(out) if isinstance(out, (bool, int, float, np.integer, np.floating)) else ''
                state = ', '.join('%s=%s' % kv for kv in sorted(KERNEL_STATE.items()) if kv[1] is not None and name not in NO_KERNEL)
                self._lines.append('%s.%s(%s)%s%s' % (self._who, name, text, ret, ' {%s}' % state if state else ''))
            return out
        return call

    def __setattr__(self, name, value):
        setattr(self._target, name, value)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def tagged_density(nao, rng):
    c = np.linalg.qr(rng.standard_normal((nao, nao)))[0]
    occ = np.zeros(nao)
    occ[:3] = 2

    class Tagged(np.ndarray):
        pass
    dm = (c * occ).dot(c.T).view(Tagged)
    dm.mo_coeff, dm.mo_occ = c, occ
    return dm


# name: (attributes set on the object, select).  'occ': pair_space='occ' with an MO-tagged density
GAMMA = {
    'cholesky': (dict(fit_route='cholesky'), 'local'),
    'blockjacobi': (dict(fit_route='blockjacobi'), 'local'),
    'auto': (dict(fit_route='auto'), 'local'),
    'refined': (dict(fit_route='auto'), 'refined'),
    'paneled': (dict(fit_route='auto', max_resident_rows=14, fft_batch=5), 'local'),
    'spectral': (dict(fit_route='auto', w_sphere=0, w_spectral_check_tol=1e-6, fft_batch=5), 'local'),
    'spectral-blockjacobi': (dict(fit_route='blockjacobi', w_sphere=0, w_spectral_check_tol=1e-6, fft_batch=5), 'local'),
    'spectral-probe-fails': (dict(fit_route='auto', w_sphere=0, w_spectral_check_tol=0.0, fft_batch=5), 'local'),
    'paneled-substitution': (dict(fit_route='auto', max_resident_rows=14, fft_batch=5, block_apply_mfma=False), 'local'),
    'robust_k': (dict(fit_route='cholesky', robust_k=True), 'local'),
    'occ-cholesky': (dict(fit_route='cholesky', pair_space='occ'), 'refined'),
    'occ-blockjacobi': (dict(fit_route='blockjacobi', pair_space='occ'), 'refined'),
    'occ-spectral': (dict(fit_route='blockjacobi', pair_space='occ', w_sphere=0, fft_batch=5), 'refined'),
}
ONE_GPU = ['cholesky', 'blockjacobi', 'auto', 'refined', 'paneled', 'paneled-substitution', 'spectral', 'spectral-blockjacobi',
           'spectral-probe-fails', 'robust_k', 'occ-cholesky', 'occ-blockjacobi', 'occ-spectral']
SHARDED = ['cholesky', 'auto', 'refined', 'spectral', 'spectral-probe-fails', 'robust_k', 'occ-cholesky', 'occ-blockjacobi', 'occ-spectral']
KPOINT = {
    'kpts-local': (dict(fit_route='blockjacobi'), 'local'),
    'kpts-refined': (dict(fit_route='auto', bj_auto_kpts=True), 'refined'),
}


def run_gamma(name, sharded, lines):
    attrs, select = GAMMA[name]
    cell = cells.cell_diamond_prim('gth-szv', (10, 9, 8))
    nao = cell.nao_nr()
    rng = np.random.default_rng(5)
    dm = rng.standard_normal((2, nao, nao))
    dm = dm + dm.transpose(0, 2, 1)
    if attrs.get('pair_space') == 'occ':
        dm = tagged_density(nao, rng)
    df = ISDF(cell, c_isdf=3, select=select, backend=Recorder(OracleBackend(), 'be', lines), comm=Recorder(Comm(), 'comm', lines))
    df.force_sharded = sharded
    df.bj_check_tol = 1e-6
    for k, v in attrs.items():
        setattr(df, k, v)
    df.build()
    vj, vk = df.get_jk(dm)
    vks = [vk]
    if not attrs.get('robust_k'):
        vks.append(df.get_jk(dm, omega=0.4)[1])
    return df, df.W.numpy(), vj, np.concatenate([np.asarray(v).ravel() for v in vks])


def run_kpoints(name, lines):
    attrs, select = KPOINT[name]
    cell = cells.cell_he2_triclinic()
    cell.mesh = np.array([9, 9, 9])
    kpts = cell.make_kpts([2, 1, 1])
    nao = cell.nao_nr()
    rng = np.random.default_rng(2)
    c = rng.standard_normal((2, nao, nao)) + 1j * rng.standard_normal((2, nao, nao))
    dms = np.einsum('kpi,kqi->kpq', c[:, :, :2], c[:, :, :2].conj())
    df = ISDF(cell, kpts=kpts, c_isdf=4, select=select, backend=Recorder(OracleBackend(), 'be', lines), comm=Recorder(Comm(), 'comm', lines))
    df.bj_check_tol = 1e-6
    for k, v in attrs.items():
        setattr(df, k, v)
    vj, vk = df.get_jk(dms, kpts=kpts)
    Wq = getattr(df, '_Wq', None) or {}                     # (the k-point build keeps one W per q and no df.W)
    W = np.concatenate([np.asarray(Wq[iq]).ravel() for iq in sorted(Wq)]) if Wq else np.zeros(0)
    return df, W, vj, vk


def main():
    out = open(args.out, 'w') if args.out else sys.stdout
    print('# fit_call_trace: %s' % ('every backend call' if args.all else 'backend calls without ' + ', '.join(QUIET)), file=out)
    todo = [('one-gpu/' + n, n, False) for n in ONE_GPU] + [('sharded/' + n, n, True) for n in SHARDED] + [(n, n, None) for n in KPOINT]
    for title, name, sharded in todo:
        if args.case and title not in args.case:
            continue
        lines = []
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter('always')
            df, W, vj, vk = run_kpoints(name, lines) if sharded is None else run_gamma(name, sharded, lines)
        lines += ['warning: %s' % w.message for w in caught if 'ISDF' in str(w.message)]
        print('case %s: %d calls' % (title, len(lines)), file=out)
        if not args.digests:
            for ln in lines:
                print('  ' + ln, file=out)
        st = getattr(df, '_fit_state', None) or {}
        print('  calls sha256 %s' % hashlib.sha256('\n'.join(lines).encode()).hexdigest(), file=out)
        print('  result ip %s W %s vj %s vk %s bj_check %s reg_used %s route %s n_panels %s w_spectral_fraction %s kind %s timings %s'
              % (sha(df.ip), sha(W), sha(vj), sha(vk), describe(df.bj_check), describe(df.reg_used), df.fit_route_used, df.n_panels,
                 describe(df.w_spectral_fraction), st.get('kind'), ','.join(sorted(df.timings))), file=out, flush=True)
    if args.out:
        out.close()


main()
