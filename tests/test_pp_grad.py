"""pp_nuc_grad / get_pp_ip1 / nuc_grad_local / get_j_nuc_grad (pyscf_isdf_amd/pp_grad.py) on the CPU: the numpy restatement
(tests/pp_grad_reference.py) against central differences of tr(D get_pp) of the oracle, the two exact identities of the terms,
then the host orchestration on the checker backend (tests/pp_grad_backend.py) against the restatement."""
import numpy as np
import pytest
import cells
import pp_cases as pc
import pp_grad_reference as pgr
from pp_grad_backend import PPGradOracleBackend
from pyscf_isdf_amd.isdf import ISDF

EPS = np.finfo(np.float64).eps
H = 2e-2            # Bohr: the larger of the two central-difference steps; the finer one is H / 2


def _sym(nao, seed):
    x = np.random.default_rng(seed).standard_normal((nao, nao))
    return 0.5 * (x + x.T)


@pytest.fixture(scope='module')
def su():
    s = pgr.CellSetup(pc.e2e_cell())
    s.nao = s.cell.nao_nr()
    s.dm = _sym(s.nao, 3)
    s.terms = pgr.pp_nuc_grad_terms(s, s.dm)
    s.grad = sum(s.terms.values())
    s.ip1 = sum(pgr.get_pp_ip1(s))
    return s


def _df(su, **kw):
    return ISDF(su.cell, backend=PPGradOracleBackend(), **kw)


def _rel(x, ref):
    return float(abs(x - ref).max() / abs(ref).max())


# ---- the restatement --------------------------------------------------------------------------------------------------------------
def test_restatement_matches_finite_differences_of_the_oracle(su):
    """Every atom and direction of pp_cases.e2e_cell() (triclinic, mesh (12, 11, 10): even and odd axes; s / p / d shells; the
    fixture's Ge and Y entries: three s, two p and d projectors) with a random symmetric D: the restated pp_nuc_grad against
    central differences of tr(D oracle get_pp) at h = 2e-2 and h / 2 = 1e-2 Bohr.
    Bound on |analytic - FD(h/2)|: |FD(h) - FD(h/2)|, which is three times the h/2 estimate's truncation error (the error of a
    central difference is c h^2), plus 64 ulp of sum|D o V| divided by h/2 for the rounding of the differenced energy.  h is
    chosen for the first term to dominate: measured, it is 4e-5 .. 3e-4 absolute (gradient entries 0.08 .. 0.32) and the second
    2.6e-11; |analytic - FD(h/2)| comes out at one third of the first, which is the finer estimate's own truncation error."""
    cell, dm = su.cell, su.dm
    env0 = np.array(cell._env, dtype=float)
    round_term = 64 * EPS * abs(dm * su.get_pp(env0)).sum() / (H / 2)

    def energy(ia, x, d):
        env = env0.copy()
        env[su.ptr[ia] + x] += d
        return np.einsum('mn,nm', su.get_pp(env), dm)

    for ia in range(cell.natm):
        for x in range(3):
            fd = {h: (energy(ia, x, h) - energy(ia, x, -h)) / (2 * h) for h in (H, H / 2)}
            own = abs(fd[H] - fd[H / 2])
            diff = abs(su.grad[ia, x] - fd[H / 2])
            print('atom %d axis %d: analytic %+.10e  fd %+.10e  |diff| %.2e  |FD(h) - FD(h/2)| %.2e  rounding %.2e' %
                  (ia, x, su.grad[ia, x], fd[H / 2], diff, own, round_term))
            assert own > 10 * round_term, 'h does not make the truncation term dominate'
            assert diff <= own + round_term, (ia, x, diff, own)


def test_nonlocal_terms_cancel_over_the_atoms(su):
    """S depends on R_a - R_mu only, so a translation of all atoms leaves the non-local energy: the Hellmann-Feynman and the
    Pulay part summed over all atoms cancel, exactly - to 64 ulp of the largest part."""
    hf, pulay = su.terms['hf_nl'], su.terms['pulay_nl']
    scale = max(abs(hf).max(), abs(pulay).max())
    tot = hf.sum(axis=0) + pulay.sum(axis=0)
    print('sum over atoms %s of parts up to %.3g' % (tot, scale))
    assert scale > 1e-3 and abs(tot).max() <= 64 * EPS * scale


def test_gradient_is_hf_minus_twice_ip1_contracted(su):
    """pp_nuc_grad(D)[a] = HF[a] - 2 sum_(mu in a) sum_nu ip1[:, mu, nu] D_(nu mu) from the two public results of the product on the
    checker backend, to 1e-12 of the largest entry; and both agree with the restatement."""
    df = _df(su)
    grad, ip1, terms = df.pp_nuc_grad(su.dm), df.get_pp_ip1(), df.pp_nuc_grad_terms(su.dm)
    assert grad.shape == (su.cell.natm, 3) and ip1.shape == (3, su.nao, su.nao) and ip1.dtype == np.float64
    hf = (terms['hf_loc'] + terms['hf_nl'])[0]
    aosl = np.asarray(su.cell.aoslice_by_atom())[:, -2:]
    want = hf - 2 * np.array([np.einsum('xmn,nm->x', ip1[:, p0:p1], su.dm[:, p0:p1]) for p0, p1 in aosl])
    assert _rel(grad, want) < 1e-12
    assert _rel(grad, su.grad) < 1e-12 and _rel(ip1, su.ip1) < 1e-12
    for k in su.terms:
        assert _rel(terms[k][0], su.terms[k]) < 1e-12, k
    assert not df._built
    for k in ('S8_nuc_grad_local', 'S8_pp_grad_local_hf', 'S8_pp_grad_nonlocal'):
        assert k in df.timings


# ---- the orchestration on the checker backend ---------------------------------------------------------------------------------
def test_chunks_stacks_and_the_symmetric_part(su):
    df = _df(su)
    G = int(np.prod(su.mesh))
    dn = su.dm + 0.3 * np.random.default_rng(8).standard_normal((su.nao, su.nao))       # not symmetric
    d2 = _sym(su.nao, 9)
    want2 = pgr.pp_nuc_grad(su, d2)
    df.e1_grid_chunk = 500                                          # 1320 = 2 * 500 + 320: a ragged tail
    try:
        assert df.backend.calls['rowdot3'] == 0
        g = df.pp_nuc_grad(su.dm)
        assert df.backend.calls['rowdot3'] == 3 and df.backend.calls['pp_local_force'] == 1
        stack = df.pp_nuc_grad(np.array([su.dm, d2, dn]))
        ip1 = df.get_pp_ip1()
    finally:
        df.e1_grid_chunk = 65536
    assert _rel(g, su.grad) < 1e-12 and _rel(ip1, su.ip1) < 1e-12
    assert stack.shape == (3, su.cell.natm, 3)
    assert _rel(stack[0], su.grad) < 1e-12 and _rel(stack[1], want2) < 1e-12
    assert _rel(stack[2], pgr.pp_nuc_grad(su, 0.5 * (dn + dn.T))) < 1e-12       # a non-symmetric D: its symmetric part's answer
    assert _rel(df.pp_nuc_grad(su.dm + 0j), su.grad) < 1e-12
    with pytest.raises(ValueError, match='real density'):
        df.pp_nuc_grad(su.dm + 1e-6j * d2)

    # nuc_grad_local: vR shared and per set, on the host or the device, against the formula on the dense collocation
    rng = np.random.default_rng(12)
    v = rng.standard_normal((2, G))
    w = su.cell.vol / G
    aosl = np.asarray(su.cell.aoslice_by_atom())[:, -2:]

    def local(vr, d):
        m = w * np.einsum('xgm,g,gn->xmn', su.ao4[1:], vr, su.ao4[0], optimize=True)
        return np.array([-2 * np.einsum('xmn,nm->x', m[:, p0:p1], d[:, p0:p1]) for p0, p1 in aosl])

    df.e1_grid_chunk = 333
    try:
        one = df.nuc_grad_local(v[0], su.dm)
        shared = df.nuc_grad_local(v[1], np.array([su.dm, dn]))
        per_set = df.nuc_grad_local(df.backend.to_device(v), np.array([su.dm, dn]))
    finally:
        df.e1_grid_chunk = 65536
    assert one.shape == (su.cell.natm, 3) and shared.shape == per_set.shape == (2, su.cell.natm, 3)
    assert _rel(one, local(v[0], su.dm)) < 1e-12
    assert _rel(shared[0], local(v[1], su.dm)) < 1e-12 and _rel(shared[1], local(v[1], 0.5 * (dn + dn.T))) < 1e-12
    assert _rel(per_set[0], one) < 1e-12 and _rel(per_set[1], shared[1]) < 1e-12
    with pytest.raises(ValueError, match='rows'):
        df.nuc_grad_local(np.zeros((3, G)), np.array([su.dm, dn]))


def test_j_force_is_the_contraction_of_get_j_e1():
    """get_j_nuc_grad(D)[a] = 2 sum_(mu in a) sum_nu get_j_e1(D)[x, mu, nu] D_(nu mu) (pyscf/pbc/grad/krhf.py:64) for a symmetric D, on
    diamond / gth-szv at 12^3, with and without a resident collocation and through MultiGridFFTDF."""
    from pyscf_isdf_amd import multigrid as pmg
    cell = cells.cell_diamond_prim('gth-szv', (12, 12, 12))
    nao = cell.nao_nr()
    dms = np.array([_sym(nao, 21), _sym(nao, 22)])
    df = ISDF(cell, backend=PPGradOracleBackend())
    aosl = np.asarray(cell.aoslice_by_atom())[:, -2:]
    e1 = df.get_j_e1(dms)                                                   # (3, nset, nao, nao)
    want = np.array([[2 * np.einsum('xmn,nm->x', e1[:, s, p0:p1], dms[s][:, p0:p1]) for p0, p1 in aosl] for s in range(2)])
    df.e1_grid_chunk = 700                                                  # 1728 = 2 * 700 + 328
    got = df.get_j_nuc_grad(dms)
    assert got.shape == (2, cell.natm, 3) and not df._built
    assert _rel(got, want) < 1e-12
    assert _rel(df.get_j_nuc_grad(dms[1]), want[1]) < 1e-12
    df.collocate()                                                          # rho from the resident phi
    assert _rel(df.get_j_nuc_grad(dms), want) < 1e-12
    mg = pmg.MultiGridFFTDF(cell, backend=PPGradOracleBackend())
    assert _rel(mg.get_j_nuc_grad(dms[0]), want[0]) < 1e-12


def test_refusals_fire_before_any_work(su):
    from pyscf_isdf_amd import kpts_symm
    dm = su.dm
    kpt = np.array([[0.1, 0.2, 0.3]])
    G = int(np.prod(su.mesh))

    def calls(df):
        return [lambda **kw: df.pp_nuc_grad(dm, **kw), lambda **kw: df.get_pp_ip1(**kw),
                lambda **kw: df.nuc_grad_local(np.zeros(G), dm, **kw), lambda **kw: df.get_j_nuc_grad(dm, **kw)]

    def untouched(df):
        return not df._built and not df.timings and not sum(df.backend.calls.values())

    df = _df(su)
    for call in calls(df):
        with pytest.raises(NotImplementedError, match='k-points'):
            call(kpts=kpt)
    dk = _df(su, kpts=kpt)
    for call in calls(dk):
        with pytest.raises(NotImplementedError, match='k-points'):
            call()
    sh = _df(su)
    sh.force_sharded = True
    for call in calls(sh):
        with pytest.raises(NotImplementedError, match='sharded'):
            call()
    ks = kpts_symm.make_kpts(su.cell, np.zeros((1, 3)))             # a k-point object, even of the Gamma point alone
    for call in calls(df):
        with pytest.raises(NotImplementedError, match='k-point symmetry'):
            call(kpts=ks)
    dsym = _df(su, kpts=ks)
    for call in calls(dsym):
        with pytest.raises(NotImplementedError, match='k-point symmetry'):
            call()
    assert untouched(df) and untouched(dk) and untouched(sh) and untouched(dsym)
