"""Test-side second-order SCF (TEST INFRASTRUCTURE): Newton steps in the occupied-virtual rotation space with the exact orbital
Hessian, built column by column from a response function (the role of pyscf/soscf/newton_ah.py gen_g_hop_rhf / gen_g_hop_uhf,
without the augmented-Hessian solver: the spaces here are tiny, so the Hessian is formed and solved directly).

Orbitals live in channels c (one per k-point of a closed shell, or one per spin of an open shell), each with occupation o_c, and
the energy is E = (1/nk) sum_c tr(h_c D_c) + E_Hxc, D_c = o_c C_oc C_oc^H.  A rotation C_c -> C_c exp(K_c), K_c = [[0, -x_c^H],
[x_c, 0]], gives to second order (w = 2 o / nk)
    gradient   g_c = w F_vo,
    Hessian    (H x)_c = w (F_vv x_c - x_c F_oo + C_v^H V_c[D1(x)] C_o),   D1_c(x) = o_c (C_v x_c C_o^H + h.c.),
with V = the response (J + f_xc) to the first-order densities.  Complex channels carry (Re x, Im x) as real parameters."""
import numpy as np
import scipy.linalg


def _split(x, shapes, cplx):
    out, p = [], 0
    for (nv, no) in shapes:
        n = nv * no
        if cplx:
            out.append((x[p:p + n] + 1j * x[p + n:p + 2 * n]).reshape(nv, no))
            p += 2 * n
        else:
            out.append(x[p:p + n].reshape(nv, no))
            p += n
    return out


def _flat(blocks, cplx):
    if cplx:
        return np.concatenate([np.concatenate([b.real.ravel(), b.imag.ravel()]) for b in blocks])
    return np.concatenate([b.real.ravel() for b in blocks])


def newton(Cs, nocc, occ, nk, fock_energy, make_response, max_iter=10, gtol=1e-8):
    """Newton iterations from orbitals Cs (nchan, nao, nmo; occupied columns first).

    fock_energy(D (nchan, nao, nao)) -> (E, F (nchan, nao, nao)); make_response(D) -> vind, vind(D1 (ncol, nchan, nao, nao)) ->
    V (ncol, nchan, nao, nao).  Returns (E, Cs, history) with history = [(E, |g|), ...] at every visited point."""
    Cs = np.array(Cs)
    cplx = np.iscomplexobj(Cs)
    nchan, nao, nmo = Cs.shape
    shapes = [(nmo - nocc, nocc)] * nchan
    w = 2.0 * occ / nk
    history = []
    for it in range(max_iter + 1):
        Co, Cv = Cs[:, :, :nocc], Cs[:, :, nocc:]
        D = occ * np.einsum('cpi,cqi->cpq', Co, Co.conj())
        E, F = fock_energy(D)
        Fmo = np.einsum('cpi,cpq,cqj->cij', Cs.conj(), F, Cs)
        g = _flat([w * Fmo[c, nocc:, :nocc] for c in range(nchan)], cplx)
        history.append((E, np.linalg.norm(g)))
        if history[-1][1] < gtol or it == max_iter:
            break
        vind = make_response(D)
        npar = g.size
        cols = np.eye(npar)
        D1 = np.zeros((npar, nchan, nao, nao), dtype=Cs.dtype)
        X = [_split(cols[q], shapes, cplx) for q in range(npar)]
        for q in range(npar):
            for c in range(nchan):
                d = Cv[c].dot(X[q][c]).dot(Co[c].conj().T)
                D1[q, c] = occ * (d + d.conj().T)
        V = np.asarray(vind(D1)).reshape(npar, nchan, nao, nao)
        H = np.empty((npar, npar))
        for q in range(npar):
            hx = []
            for c in range(nchan):
                x = X[q][c]
                hx.append(w * (Fmo[c, nocc:, nocc:].dot(x) - x.dot(Fmo[c, :nocc, :nocc]) + Cv[c].conj().T.dot(V[q, c]).dot(Co[c])))
            H[:, q] = _flat(hx, cplx)
        step = _split(np.linalg.solve(0.5 * (H + H.T), -g), shapes, cplx)
        for c in range(nchan):
            K = np.zeros((nmo, nmo), dtype=Cs.dtype)
            K[nocc:, :nocc] = step[c]
            K[:nocc, nocc:] = -step[c].conj().T
            Cs[c] = Cs[c].dot(scipy.linalg.expm(K))
    return history[-1][0], Cs, history


def rotated(Cs, nocc, scale, seed=0):
    """Cs with a fixed random occupied-virtual rotation of size ``scale`` per element applied to every channel (a start away from
    the minimum, so that several Newton steps are seen)."""
    rng = np.random.default_rng(seed)
    out = np.array(Cs)
    nmo = out.shape[2]
    for c in range(len(out)):
        x = scale * rng.standard_normal((nmo - nocc, nocc))
        K = np.zeros((nmo, nmo))
        K[nocc:, :nocc] = x
        K[:nocc, nocc:] = -x.T
        out[c] = out[c].dot(scipy.linalg.expm(K))
    return out


def assert_quadratic(history, c_max, g_start=1e-2, g_end=1e-8):
    """From the first point with |g| <= g_start every step satisfies |g_(k+1)| <= c_max |g_k|^2 until |g| < g_end."""
    gs = [h[1] for h in history]
    assert gs[-1] < g_end, gs
    k0 = next(i for i, g in enumerate(gs) if g <= g_start)
    for a, b in zip(gs[k0:-1], gs[k0 + 1:]):
        assert b <= c_max * a * a, (a, b, gs)
    return gs
