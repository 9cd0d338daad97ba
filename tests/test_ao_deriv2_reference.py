"""The numpy restatement of the ten collocation planes (tests/ao_deriv2_reference.py) on the sweep cell of
tests/test_gpu_eval_ao_sweep.py (s / p / d / f shells, 4 / 3 / 2 / 2 contractions, 553 images) at points('first100'): planes 0 .. 3
against the oracle's eval_ao_deriv1, planes 4 .. 9 against central differences of the oracle's gradient planes in the point
coordinates."""
import numpy as np
import pytest
import ao_deriv2_reference as r2
from oracle import ao as oao
from test_gpu_eval_ao_sweep import sweep_cell, points

EPS = 2.2e-16
H = 2e-3            # Bohr: the larger of the two central-difference steps; the finer one is H / 2


@pytest.fixture(scope='module')
def planes():
    cell, Ls, rcut = sweep_cell()
    c = points('first100')
    args = (cell._atm, cell._bas, cell._env)
    return args, c, Ls, rcut, r2.eval_ao_deriv2(*args, c, Ls, rcut), oao.eval_ao_deriv1(*args, c, Ls, rcut)


def test_planes_0_to_3_are_the_oracles(planes):
    _, _, _, _, got, ref = planes
    assert got.shape == (10,) + ref.shape[1:] and got.dtype == np.float64
    assert abs(got[:4] - ref).max() <= 1e-14 * abs(ref).max()


def test_second_derivative_planes_against_central_differences_of_the_gradient_planes(planes):
    """d_b (d_a phi) by central differences of the oracle's plane 1 + a in coordinate b at h = 2e-3 and h / 2 = 1e-3 Bohr.  Per plane:
    |analytic - FD(h/2)| <= 0.5 |FD(h) - FD(h/2)| + 10 * 2.2e-16 max|grad phi| / (h/2), maxima over the plane.  The exact ratio of a
    second-order difference is 1/3; the floor is the rounding of the difference quotient.  Measured: ratio 0.333 on all six planes,
    |analytic - FD(h/2)| 4.7e-6 .. 1.6e-5 on planes of up to 5.8, floor 4.6e-12."""
    args, c, Ls, rcut, got, ref = planes
    floor = 10 * EPS * abs(ref[1:]).max() / (H / 2)
    fd = {}
    for h in (H, H / 2):
        for b in range(3):
            e = np.zeros(3)
            e[b] = h
            fd[h, b] = (oao.eval_ao_deriv1(*args, c + e, Ls, rcut)[1:] - oao.eval_ao_deriv1(*args, c - e, Ls, rcut)[1:]) / (2 * h)
    for p, (a, b) in enumerate(r2.HESS_PAIRS):
        own = abs(fd[H, b][a] - fd[H / 2, b][a]).max()
        diff = abs(got[4 + p] - fd[H / 2, b][a]).max()
        print('plane %d (%d, %d): |analytic - FD(h/2)| %.3e  |FD(h) - FD(h/2)| %.3e  ratio %.3f  floor %.2e  max|plane| %.3f' %
              (4 + p, a, b, diff, own, diff / own, floor, abs(got[4 + p]).max()))
        assert abs(got[4 + p]).max() > 0.1
        assert diff <= 0.5 * own + floor, (p, diff, own)
        # the mixed derivative from the other side: d_a (d_b phi)
        assert abs(got[4 + p] - fd[H / 2, a][b]).max() <= 0.5 * abs(fd[H, a][b] - fd[H / 2, a][b]).max() + floor


def test_extended_precision_evaluation_bounds_the_float64_rounding(planes):
    """The same text in np.longdouble (cutoff decisions as in float64): the float64 restatement's own error.  Measured 6.2e-15 on
    planes of up to 5.8 - below 1e-12, so the device test holds the kernel to the project's derivative bound."""
    args, c, Ls, rcut, got, _ = planes
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip('no extended precision on this platform')
    ext = r2.eval_ao_deriv2(*args, c, Ls, rcut, dtype=np.longdouble)
    err = abs(got - ext.astype(np.float64)).max()
    print('float64 restatement against longdouble: %.3e' % err)
    assert err < 1e-12
