"""Elastic moduli of a minimum (include/mdhip.h md_elas_*) restated in numpy, on top of
tests/hess_reference.py (pair_list, pair_tk, dense).  Takes nothing from the code under test.

Definitions.  del = x_j(+translation) - x_i, r = |del|, t = U'/r, k = U'', c = (k - t)/r^2, V = |det(cell)|; Green-Lagrange
strain eta (r'^2 = r^2 + 2 del^T eta del), eta_ab and eta_ba one tensor component, no Voigt or engineering factors:
    sigma_ab = (1/V) sum_pairs t del_a del_b                    CB_abcd = (1/V) sum_pairs c del_a del_b del_c del_d
    Xi_{i,c;ab} = sum_j [ -c del_a del_b del_c - t (delta_ac del_b + delta_bc del_a) ]
    u_ab = -H^+ Xi_ab          N_st = (1/V) Xi_s . u_t          C = CB + N
Components: 3-D xx, yy, zz, xy, xz, yz; 2-D xx, yy, xy.

Every assembly takes a dtype: float64 is the reference, numpy.longdouble the same arithmetic with more bits.  The float64
sums are SEQUENTIAL (numpy.add.at / cumsum), the plainest order there is: rounding_floor, the float64 results against the
longdouble ones, is then the error of a sum no more careful than any the device may use."""
import numpy as np

from tests import hess_reference as hr

COMPONENTS = {2: ((0, 0), (1, 1), (0, 1)), 3: ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))}


def pair_u(kind, params, r, si, sj, dtype=np.float64):
    """The pair ENERGY whose derivatives hess_reference.pair_tk returns (0 outside the potential's own cutoff)."""
    T = dtype
    r, si, sj = (np.asarray(a, dtype=T) for a in (r, si, sj))
    p = [T(v) for v in params]
    if kind == hr.POT_LJ:
        eps, rc = p[0], p[2]
        s6 = (((si + sj) / T(2)) / r) ** 6
        u, inside = T(4) * eps * (s6 * s6 - s6), r < rc
    elif kind == hr.POT_POLYDISPERSE:
        rc, eta = p[0], p[1]
        se = T(0.5) * (si + sj) * (T(1) - eta * np.abs(si - sj))
        c0, c2, c4 = T(-28) / rc ** 12, T(48) / rc ** 14, T(-21) / rc ** 16
        q = r / se
        u, inside = q ** -12 + c0 + c2 * q ** 2 + c4 * q ** 4, r < rc * se
    elif kind == hr.POT_LJ_MODIFIED and int(params[3]) == 2:
        eps, rc, ron = p[0], p[2], p[4]
        s6 = (((si + sj) / T(2)) / r) ** 6
        rc2, r2, ron2 = rc * rc, r * r, ron * ron
        S = np.where(r >= ron, (rc2 - r2) ** 2 * (rc2 + T(2) * r2 - T(3) * ron2) / (rc2 - ron2) ** 3, T(1))
        u, inside = S * T(4) * eps * (s6 * s6 - s6), r < rc
    else:
        raise KeyError((kind, params))
    return np.where(inside, u, np.zeros_like(r))


def volume(U):
    return float(abs(np.linalg.det(np.asarray(U, dtype=np.float64))))


def _seq_sum(v, dtype):
    """Sum over axis 0, one term after the other in float64; numpy's own (pairwise) sum in longdouble."""
    v = np.asarray(v, dtype=dtype)
    if len(v) == 0:
        return np.zeros(v.shape[1:], dtype=dtype)
    return np.cumsum(v, axis=0)[-1] if dtype == np.float64 else v.sum(axis=0)


def pair_terms(x, U, cutoff, kind, params, diam, dtype=np.float64, pairs=None):
    """(i, j, del, t, k) of the pairs inside the potential's own cutoff."""
    i, j, dl = hr.pair_list(x, U, cutoff, dtype) if pairs is None else pairs
    dl = np.asarray(dl, dtype=dtype)
    d = np.asarray(diam, dtype=np.float64).astype(dtype)
    r = np.sqrt((dl * dl).sum(axis=1))
    t, k, inside = hr.pair_tk(kind, params, r, d[i], d[j], dtype)
    return i[inside], j[inside], dl[inside], t[inside], k[inside]


def energy_forces(x, U, cutoff, kind, params, diam, dtype=np.float64):
    """(U_total, F[n, d]) of the reference's own pair energy: F_i = sum_j t del (del = x_j - x_i), F_j the negative."""
    n, d = np.asarray(x).shape
    i, j, dl, t, _ = pair_terms(x, U, cutoff, kind, params, diam, dtype)
    dm = np.asarray(diam, dtype=np.float64).astype(dtype)
    r = np.sqrt((dl * dl).sum(axis=1))
    u = pair_u(kind, params, r, dm[i], dm[j], dtype)
    F = np.zeros((n, d), dtype=dtype)
    np.add.at(F, i, t[:, None] * dl)
    np.add.at(F, j, -t[:, None] * dl)
    return u.sum(), F


def affine(x, U, cutoff, kind, params, diam, dtype=np.float64, pairs=None, sabotage=None):
    """dict(stress[nc], born[nc, nc], xi[nc, n, d], stress_abs, born_abs, xi_abs (the sums of |terms|), volume, npairs).

    sabotage: one deliberate mistake, for the tests that show the tolerances would catch it -- ("drop", index) leaves a pair
    out, "no_t" drops the t-term of Xi, "engineering" doubles the shear components of Xi, "one_sided" gives the second member
    of every pair a Xi term that is not the negative of the first's (its t-term is left out), "born_k" builds CB with k in
    place of k - t."""
    T = dtype
    n, d = np.asarray(x).shape
    comps = COMPONENTS[d]
    nc = len(comps)
    i, j, dl, t, k = pair_terms(x, U, cutoff, kind, params, diam, T, pairs)
    if isinstance(sabotage, tuple) and sabotage[0] == "drop":
        keep = np.ones(len(i), dtype=bool)
        keep[sabotage[1]] = False
        i, j, dl, t, k = i[keep], j[keep], dl[keep], t[keep], k[keep]
    V = T(volume(U))
    r2 = (dl * dl).sum(axis=1)
    c = (k - t) / r2
    cb = k / r2 if sabotage == "born_k" else c
    P = np.stack([dl[:, a] * dl[:, b] for a, b in comps], axis=1)                   # [pair, s]
    st = t[:, None] * P
    bt = cb[:, None, None] * P[:, :, None] * P[:, None, :]
    xi = np.zeros((nc, n, d), dtype=T)
    xi_abs = np.zeros((nc, n, d), dtype=T)
    for s, (a, b) in enumerate(comps):
        term = -c[:, None] * P[:, s, None] * dl                                     # [pair, c]
        tt = np.zeros_like(term)
        tt[:, a] -= t * dl[:, b]
        tt[:, b] -= t * dl[:, a]
        if sabotage == "no_t":
            tt[:] = 0
        f = T(2) if (sabotage == "engineering" and a != b) else T(1)
        np.add.at(xi[s], i, f * (term + tt))
        np.add.at(xi[s], j, -f * (term + (0 if sabotage == "one_sided" else tt)))
        np.add.at(xi_abs[s], i, np.abs(term) + np.abs(tt))
        np.add.at(xi_abs[s], j, np.abs(term) + np.abs(tt))
    return dict(stress=_seq_sum(st, T) / V, born=_seq_sum(bt, T) / V, xi=xi, stress_abs=np.abs(st).sum(axis=0) / V,
                born_abs=np.abs(bt).sum(axis=0) / V, xi_abs=xi_abs, volume=float(V), npairs=len(i),
                pair_effect=np.abs(bt).max(axis=(1, 2)))


def affine_floor(x, U, cutoff, kind, params, diam):
    """(a64, a80, floor) of the affine quantities alone (no solve): floor = dict(stress, born (absolute), xi (relative to
    max |Xi|)), float64 against longdouble."""
    a64 = affine(x, U, cutoff, kind, params, diam)
    a80 = affine(x, U, cutoff, kind, params, diam, np.longdouble)
    return a64, a80, dict(stress=float(np.abs(a64["stress"] - a80["stress"]).max()), born=float(np.abs(a64["born"] - a80["born"]).max()),
                          xi=float(np.abs(a64["xi"] - a80["xi"]).max() / np.abs(a80["xi"]).max()))


def stress_matrix(stress, d):
    S = np.zeros((d, d), dtype=np.asarray(stress).dtype)
    for s, (a, b) in enumerate(COMPONENTS[d]):
        S[a, b] = S[b, a] = stress[s]
    return S


def contract(C, E1, E2, d):
    """sum_abcd E1_ab C_abcd E2_cd over ALL tensor indices of a component matrix C[nc, nc] (E1, E2 symmetric d x d)."""
    comps = COMPONENTS[d]
    w = lambda E: np.array([(1.0 if a == b else 2.0) * E[a, b] for a, b in comps])
    return float(w(E1) @ np.asarray(C, dtype=np.float64) @ w(E2))


def null_basis(H, n, d):
    """Orthonormal rows spanning the null space a minimum's H has by construction: the unit vectors of the particles whose
    rows of H are zero (no neighbour), and the d uniform translations of all the others."""
    Hn = np.asarray(H, dtype=np.float64).reshape(n, d, n * d)
    lone = ~np.any(Hn != 0.0, axis=(1, 2))
    rows = []
    for p in np.flatnonzero(lone):
        for a in range(d):
            e = np.zeros((n, d))
            e[p, a] = 1.0
            rows.append(e.reshape(-1))
    nb = int((~lone).sum())
    for a in range(d):
        e = np.zeros((n, d))
        e[~lone, a] = 1.0 / np.sqrt(max(nb, 1))
        rows.append(e.reshape(-1))
    return np.array(rows), lone


def lambda_min(H, n, d):
    """The smallest eigenvalue of H on the complement of null_basis."""
    Nb, _ = null_basis(H, n, d)
    big = 10.0 * np.abs(np.linalg.eigvalsh(H)).max()
    return float(np.linalg.eigvalsh(H + big * (Nb.T @ Nb)).min())


def solve(H64, H80, rhs80, n, d, refine=True):
    """x = H^+ rhs on the complement of null_basis: a float64 solve of the deflated matrix, then iterative refinement with
    the residual formed in longdouble until it stops improving.  Returns (x as longdouble [m, n d], history of |residual|)."""
    Nb, _ = null_basis(H64, n, d)
    big = np.abs(np.diag(H64)).max()
    A = H64 + big * (Nb.T @ Nb)
    Nl = Nb.astype(np.longdouble)
    proj = lambda v: v - (v @ Nl.T) @ Nl
    b = proj(np.asarray(rhs80, dtype=np.longdouble))
    x = proj(np.linalg.solve(A, b.astype(np.float64).T).T.astype(np.longdouble))
    hist = [float(np.abs(b - x @ H80).max())]
    while refine and len(hist) < 12:
        res = proj(b - x @ H80)
        xn = x + proj(np.linalg.solve(A, res.astype(np.float64).T).T.astype(np.longdouble))
        e = float(np.abs(b - xn @ H80).max())
        if not e < 0.5 * hist[-1]:
            break
        x = xn
        hist.append(e)
    return x, hist


def moduli(x, U, cutoff, kind, params, diam):
    """The whole reference of one frame: the float64 assembly, the longdouble assembly with the refined solve, and their
    differences (rounding_floor).  dict(a64, a80 (affine()), u (float64 [nc, n, d]), N (float64 [nc, nc], from longdouble),
    C, lambda_min, floor=dict(stress, born, xi, N, u), refine=history)."""
    n, d = np.asarray(x).shape
    pairs64 = hr.pair_list(x, U, cutoff)
    pairs80 = hr.pair_list(x, U, cutoff, np.longdouble)
    a64 = affine(x, U, cutoff, kind, params, diam, pairs=pairs64)
    a80 = affine(x, U, cutoff, kind, params, diam, np.longdouble, pairs=pairs80)
    H64 = hr.dense(x, U, cutoff, kind, params, diam, pairs=pairs64)
    H80 = hr.dense(x, U, cutoff, kind, params, diam, dtype=np.longdouble, pairs=pairs80)
    nc = len(COMPONENTS[d])
    V = a64["volume"]
    u80, hist = solve(H64, H80, -a80["xi"].reshape(nc, -1), n, d)
    u64, _ = solve(H64, H64.astype(np.longdouble), -a64["xi"].reshape(nc, -1).astype(np.longdouble), n, d, refine=False)
    N80 = (a80["xi"].reshape(nc, -1) @ u80.T) / np.longdouble(V)
    N64 = (a64["xi"].reshape(nc, -1) @ u64.astype(np.float64).T) / V
    floor = dict(stress=float(np.abs(a64["stress"] - a80["stress"]).max()), born=float(np.abs(a64["born"] - a80["born"]).max()),
                 xi=float(np.abs(a64["xi"] - a80["xi"]).max() / np.abs(a80["xi"]).max()) if np.abs(a80["xi"]).max() > 0 else 0.0,
                 N=float(np.abs(N64 - N80).max()), u=float(np.abs(u64 - u80).max()))
    N = N80.astype(np.float64)
    return dict(a64=a64, a80=a80, u=u80.astype(np.float64).reshape(nc, n, d), N=N, C=a80["born"].astype(np.float64) + 0.5 * (N + N.T),
                lambda_min=lambda_min(H64, n, d), floor=floor, refine=hist, H=H64)


def rounding_floor(x, U, cutoff, kind, params, diam):
    """dict(stress, born (absolute), xi (relative to max |Xi|), N, u (absolute)): float64 against longdouble on this frame."""
    return moduli(x, U, cutoff, kind, params, diam)["floor"]


def relax(x, U, cutoff, kind, params, diam, gtol=1e-12, max_steps=400):
    """Newton steps x += H^+ F until max |F| <= gtol: the plain step with the pseudo-inverse wherever H is positive on the
    complement of its null space.  Farther out, where H is indefinite, a step uses |lambda| in place of lambda (none below
    1e-3 of the largest).  No step moves a coordinate by more than 0.05.  Returns (x, max |F|, steps)."""
    x = np.array(x, dtype=np.float64)
    n, d = x.shape
    for step in range(max_steps + 1):
        _, F = energy_forces(x, U, cutoff, kind, params, diam, np.longdouble)
        g = float(np.abs(F).max())
        if g <= gtol or step == max_steps:
            return x, g, step
        H = hr.dense(x, U, cutoff, kind, params, diam)
        Nb, _ = null_basis(H, n, d)
        w, Q = np.linalg.eigh(H + np.abs(np.diag(H)).max() * (Nb.T @ Nb))
        wa = w if w.min() > 0.0 else np.maximum(np.abs(w), 1e-3 * np.abs(w).max())
        f = F.astype(np.float64).reshape(-1)
        f = f - Nb.T @ (Nb @ f)
        dx = Q @ ((Q.T @ f) / wa)
        dx = (dx - Nb.T @ (Nb @ dx)).reshape(n, d)
        x = x + min(1.0, 0.05 / max(np.abs(dx).max(), 1e-300)) * dx
    raise AssertionError("unreachable")


def descend(x, U, cutoff, kind, params, diam, gtol=1e-2, max_steps=20000):
    """Steepest descent with a backtracking step (the energy never rises) from anywhere into the basin of the inherent
    structure: the start near a minimum that relax needs."""
    x = np.array(x, dtype=np.float64)
    e, F = energy_forces(x, U, cutoff, kind, params, diam)
    dt = 1e-3
    for _ in range(max_steps):
        if np.abs(F).max() <= gtol:
            break
        xn = x + dt * F
        en, Fn = energy_forces(xn, U, cutoff, kind, params, diam)
        if en < e:
            x, e, F, dt = xn, en, Fn, dt * 1.1
        else:
            dt *= 0.5
    return x


XPLOR_SMOOTH = dict(r_on=1.83, r_cut=2.125, rho=0.897, dlo=0.97, dhi=1.03, jitter=0.02)


def fcc_xplor_system(m, seed=11):
    """A frame on which finite differences of an XPLOR energy converge as h^2.  The XPLOR switching function is C1 only: U''
    jumps at r_on and r_cut, and a pair that crosses either radius between -h and +h adds O(1) of a pair term to the second
    difference -- in a glass some pair always does (108 particles have 2000 pairs per unit of r there).  Here the particles
    sit on a jittered fcc lattice (m^3 cells, N = 4 m^3) with diameters U[0.97, 1.03]: the neighbour shells stay narrow
    (a / sqrt 2 = 1.16, a = 1.65, a sqrt 1.5 = 2.02, a sqrt 2 = 2.33 at rho = 0.897), r_on = 1.83 and r_cut = 2.125 lie in the
    gaps between them, the third shell inside the switching range, and the disorder still gives an affine force field and a
    non-affine term of a few per cent.  Returns (system dict as tests.util.lj_system's, kind, params, cutoff); the tests
    assert the premise on the relaxed frame with kink_margin."""
    P = XPLOR_SMOOTH
    a = (4.0 / P["rho"]) ** (1.0 / 3.0)
    base = np.array([[0, 0, 0], [0.5, 0.5, 0], [0.5, 0, 0.5], [0, 0.5, 0.5]])
    cells = np.stack(np.meshgrid(*[np.arange(m)] * 3, indexing="ij"), -1).reshape(-1, 1, 3)
    rng = np.random.default_rng(seed)
    x = ((cells + base[None] + 0.25) * a).reshape(-1, 3)          # (a quarter cell in from the faces: the jitter stays inside)
    n = len(x)
    x = x + rng.uniform(-P["jitter"], P["jitter"], x.shape) * a
    diam = rng.uniform(P["dlo"], P["dhi"], n)
    s = dict(n=n, dim=3, box=np.full(3, m * a), x=np.ascontiguousarray(x), v=np.zeros((n, 3)), f=np.zeros((n, 3)),
             img=np.zeros((n, 3), dtype=np.int32), diam=diam, spacing=a)
    return s, hr.POT_LJ_MODIFIED, [1.0, 1.0, P["r_cut"], 2.0, P["r_on"]], P["r_cut"]


def kink_margin(x, U, radii, reach):
    """The smallest | |del| - R | over all pairs within `reach` and the radii R: how far the frame is from a kink of U''."""
    _, _, dl = hr.pair_list(x, U, reach)
    r = np.sqrt((np.asarray(dl, dtype=np.float64) ** 2).sum(axis=1))
    return float(min(np.abs(r - R).min() for R in radii))


def strained(x, U, F):
    """Positions and cell under the deformation gradient F (scaled coordinates fixed): x F^T, F U."""
    return np.asarray(x) @ np.asarray(F).T, np.asarray(F) @ np.asarray(U)


def second_difference_prediction(C, stress, E, V, d):
    """d2U/dh2 at h = 0 for F(h) = I + h E: V (eta1 : C : eta1 + sigma : E^T E), eta1 = (E + E^T) / 2."""
    eta1 = 0.5 * (E + E.T)
    return V * (contract(C, eta1, eta1, d) + float((stress_matrix(stress, d) * (E.T @ E)).sum()))
