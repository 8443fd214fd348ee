"""The Hessian of the pair energy (include/mdhip.h md_hess_*) restated in numpy.  Takes nothing from
the code under test: the pair list is brute force over all particle pairs and all 3^d lattice translations (the search the
oracle's general-cell pair loop makes), U' and U'' of the four built-in potentials are written out here in plain floating
point -- for the FORCE the oracle evaluates, t = -f/r and k = -df/dr -- and tests/test_hessian.py checks them against
central differences of oracle.evaluate and oracle.forces_brute.

Every function takes a dtype: float64 is the reference, numpy.longdouble the same arithmetic with more bits; their
difference on a frame is the fp64 rounding floor of that frame (rounding_floor)."""
import itertools

import numpy as np

POT_LJ, POT_PSEUDOHS, POT_POLYDISPERSE, POT_LJ_MODIFIED = 0, 1, 2, 3
PHS_A, PHS_B = 134.5526623421209, 1.0204081632653061


def pair_full(kind, params, r, si, sj, dtype=np.float64):
    """Everything tests/pair_table.py and pair_tk need of a pair at distances r for diameters si, sj, in one place:
    dict(u, f, k, Su, Sf, Sk, inside) -- the energy, f = -dU/dr, U'' of the smooth branch (NOT masked by `inside`, the
    potential's own cutoff branch), and for each of u, f, k the scale S = the sum of the absolute values of the terms of the
    formula as written here (differences that cancel, rc^2 - r^2 of the XPLOR switch included, enter with both terms)."""
    T = dtype
    r, si, sj = (np.asarray(a, dtype=T) for a in (r, si, sj))
    p = [T(v) for v in params]
    if kind == POT_LJ:
        eps, rc = p[0], p[2]
        sg = (si + sj) / T(2)
        s6 = (sg / r) ** 6
        s12 = s6 * s6
        u = T(4) * eps * (s12 - s6)
        f = T(24) * eps * (T(2) * s12 - s6) / r
        k = T(24) * eps * (T(26) * s12 - T(7) * s6) / (r * r)
        ae = abs(eps)
        Su = T(4) * ae * (s12 + s6)
        Sf = T(24) * ae * (T(2) * s12 + s6) / r
        Sk = T(24) * ae * (T(26) * s12 + T(7) * s6) / (r * r)
        inside = r < rc
    elif kind == POT_PSEUDOHS:
        lam = p[0]
        sr = ((si + sj) / T(2)) / r
        u = T(PHS_A) * (sr ** lam - sr ** (lam - T(1))) + T(1)
        f = T(PHS_A) * (lam * sr ** (lam + T(1)) - (lam - T(1)) * sr ** lam)
        k = T(PHS_A) * lam * ((lam + T(1)) * sr ** (lam + T(1)) - (lam - T(1)) * sr ** lam) / r
        Su = T(PHS_A) * (sr ** lam + sr ** (lam - T(1))) + T(1)
        Sf = T(PHS_A) * (lam * sr ** (lam + T(1)) + abs(lam - T(1)) * sr ** lam)
        Sk = T(PHS_A) * lam * ((lam + T(1)) * sr ** (lam + T(1)) + abs(lam - T(1)) * sr ** lam) / r
        inside = r < T(PHS_B)
    elif kind == POT_POLYDISPERSE:
        rc, eta = p[0], p[1]
        se = T(0.5) * (si + sj) * (T(1) - eta * np.abs(si - sj))
        c0, c2, c4 = T(-28) / rc ** 12, T(48) / rc ** 14, T(-21) / rc ** 16
        q = r / se
        u = (se / r) ** 12 + c0 + c2 * (q * q) + c4 * q ** 4
        f = T(12) * se ** 12 / r ** 13 - T(2) * c2 * r / se ** 2 - T(4) * c4 * r ** 3 / se ** 4
        k = T(156) * se ** 12 / r ** 14 + T(2) * c2 / se ** 2 + T(12) * c4 * r ** 2 / se ** 4
        Su = (se / r) ** 12 + abs(c0) + abs(c2) * (q * q) + abs(c4) * q ** 4
        Sf = T(12) * se ** 12 / r ** 13 + T(2) * abs(c2) * r / se ** 2 + T(4) * abs(c4) * r ** 3 / se ** 4
        Sk = T(156) * se ** 12 / r ** 14 + T(2) * abs(c2) / se ** 2 + T(12) * abs(c4) * r ** 2 / se ** 4
        inside = r < rc * se
    elif kind == POT_LJ_MODIFIED:
        eps, sc, rc, mode, ron = p[0], p[1], p[2], int(params[3]), p[4]
        sg = (si + sj) / T(2)
        s6 = (sg / r) ** 6
        s12 = s6 * s6
        V = T(4) * eps * (s12 - s6)
        F = T(24) * eps * (T(2) * s12 - s6) / r
        V2 = T(24) * eps * (T(26) * s12 - T(7) * s6) / (r * r)
        ae = abs(eps)
        SV = T(4) * ae * (s12 + s6)
        SF = T(24) * ae * (T(2) * s12 + s6) / r
        SV2 = T(24) * ae * (T(26) * s12 + T(7) * s6) / (r * r)
        sc6 = (sc / rc) ** 6
        Vc = T(4) * eps * (sc6 * sc6 - sc6)
        Fc = T(24) * eps * (T(2) * sc6 * sc6 - sc6) / rc
        if mode == 0:
            u, f, k = V - Vc, F, V2
            Su, Sf, Sk = SV + abs(Vc), SF, SV2
        elif mode == 1:
            u = V - Vc + (r - rc) * Fc
            f, k = F - T(24) * eps * (T(2) * sc6 * sc6 - sc6) / rc, V2
            Su, Sf, Sk = SV + abs(Vc) + (r + rc) * abs(Fc), SF + abs(Fc), SV2
        else:
            rc2, r2, ron2 = rc * rc, r * r, ron * ron
            den = (rc2 - ron2) ** 3
            a, b, g = rc2 - r2, rc2 + T(2) * r2 - T(3) * ron2, r2 - ron2
            sw = r >= ron
            S = np.where(sw, a * a * b / den, T(1))
            dS = np.where(sw, T(-12) * r * a * g / den, T(0))
            ddS = np.where(sw, T(-12) * (a * g - T(2) * r2 * g + T(2) * r2 * a) / den, T(0))
            u = V * S
            f = S * F - V * dS
            k = S * V2 - T(2) * F * dS + V * ddS
            A_, B_, G_, ad = rc2 + r2, rc2 + T(2) * r2 + T(3) * ron2, r2 + ron2, abs(den)
            SS = np.where(sw, A_ * A_ * B_ / ad, T(1))
            SdS = np.where(sw, T(12) * r * A_ * G_ / ad, T(0))
            SddS = np.where(sw, T(12) * (A_ * G_ + T(2) * r2 * G_ + T(2) * r2 * A_) / ad, T(0))
            Su = SV * SS
            Sf = SS * SF + SV * SdS
            Sk = SS * SV2 + T(2) * SF * SdS + SV * SddS
        inside = r < rc
    else:
        raise KeyError(kind)
    return dict(u=u, f=f, k=k, Su=Su, Sf=Sf, Sk=Sk, inside=inside)


def pair_tk(kind, params, r, si, sj, dtype=np.float64):
    """(t, k, inside) = (U'/r, U'', the potential's own cutoff branch) at distances r for diameters si, sj."""
    q = pair_full(kind, params, r, si, sj, dtype)
    r = np.asarray(r, dtype=dtype)
    zero = np.zeros_like(r)
    return np.where(q["inside"], -q["f"] / r, zero), np.where(q["inside"], q["k"], zero), q["inside"]


def lattice(box_or_cell, dim):
    U = np.asarray(box_or_cell, dtype=np.float64)
    return np.diag(U[:dim]) if U.ndim == 1 else U[:dim, :dim]


def pair_list(x, U, cutoff, dtype=np.float64):
    """(i, j, del) with i < j and del = (x_j + translation) - x_i, |del| <= cutoff: every particle pair against all 3^d
    lattice translations t = U s, s in {-1, 0, 1}^d (unique image: the cutoff is below half of every face distance)."""
    x = np.asarray(x, dtype=np.float64)
    n, d = x.shape
    xl = x.astype(dtype)
    Ul = np.asarray(U, dtype=np.float64).astype(dtype)
    c2 = dtype(cutoff) * dtype(cutoff)
    iu, ju = np.triu_indices(n, 1)
    I, J, DEL = [], [], []
    for s in itertools.product((-1, 0, 1), repeat=d):
        t = Ul @ np.asarray(s, dtype=dtype)
        dl = (xl[ju] + t) - xl[iu]
        d2 = (dl * dl).sum(axis=1)
        m = d2 <= c2
        I.append(iu[m])
        J.append(ju[m])
        DEL.append(dl[m])
    i, j, dl = np.concatenate(I), np.concatenate(J), np.concatenate(DEL)
    assert len(set(zip(i.tolist(), j.tolist()))) == len(i), "a pair interacts through two images"
    o = np.lexsort((j, i))
    return i[o], j[o], dl[o]


def pair_blocks(kind, params, diam, i, j, dl, dtype=np.float64):
    """The D x D blocks (k - t) n n^T + t I of the listed pairs, and which of them lie inside the potential's own cutoff."""
    T = dtype
    dl = np.asarray(dl, dtype=T)
    diam = np.asarray(diam, dtype=np.float64).astype(T)
    r = np.sqrt((dl * dl).sum(axis=1))
    t, k, inside = pair_tk(kind, params, r, diam[i], diam[j], T)
    nn = dl / r[:, None]
    d = dl.shape[1]
    B = (k - t)[:, None, None] * nn[:, :, None] * nn[:, None, :] + t[:, None, None] * np.eye(d, dtype=T)[None]
    return B, inside


def dense(x, U, cutoff, kind, params, diam, dtype=np.float64, drop=None, pairs=None):
    """The N d x N d Hessian of the smooth pair energy.  drop: index into the pair list of one pair to leave out."""
    n, d = np.asarray(x).shape
    i, j, dl = pair_list(x, U, cutoff, dtype) if pairs is None else pairs
    B, _ = pair_blocks(kind, params, diam, i, j, dl, dtype)
    if drop is not None:
        keep = np.ones(len(i), dtype=bool)
        keep[drop] = False
        i, j, B = i[keep], j[keep], B[keep]
    H = np.zeros((n, d, n, d), dtype=dtype)
    for a in range(d):
        for b in range(d):
            np.add.at(H[:, a, :, b], (i, i), B[:, a, b])
            np.add.at(H[:, a, :, b], (j, j), B[:, a, b])
            np.add.at(H[:, a, :, b], (i, j), -B[:, a, b])
            np.add.at(H[:, a, :, b], (j, i), -B[:, a, b])
    return H.reshape(n * d, n * d)


def rounding_floor(x, U, cutoff, kind, params, diam):
    """(max |H64 - H80| / max |H|, H64): the reference against itself in numpy.longdouble on this frame."""
    H64 = dense(x, U, cutoff, kind, params, diam)
    H80 = dense(x, U, cutoff, kind, params, diam, dtype=np.longdouble)
    return float(np.abs(H64.astype(np.longdouble) - H80).max() / np.abs(H80).max()), H64


def diagonal_blocks(H, n, d):
    return H.reshape(n, d, n, d)[np.arange(n), :, np.arange(n), :]


def translations(n, d):
    """The d uniform translations as orthonormal vectors (d, n, d)."""
    T = np.zeros((d, n, d))
    for c in range(d):
        T[c, :, c] = 1.0 / np.sqrt(n)
    return T
