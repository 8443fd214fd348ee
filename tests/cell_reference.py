"""numpy restatement of md_set_cell (both modes), of md_nonaffine_* and of the AQS loop, for tests/test_deformation.py
and tests/test_gpu_deformation.py.  Nothing here touches the device.

Arithmetic.  The inverse of a general cell is the oracle's (oracle.set_cell.inverse(): cofactors over the determinant, the
formulas mdhip.hip cell_geometry uses); a diagonal cell's is 1 / L per component.  frac = U^-1 x and x = U f are the wrap's
products (oracle/md_oracle.c wrap1 / wrap_tric): L * f per component, or row times vector, left to right, every product
and every sum rounded on its own -- numpy's elementwise operations do exactly that, so positions and images can be
compared with the device bit for bit.

A cell is a d x d array with the lattice vectors in its COLUMNS.  `variant` arguments are deliberate mistakes, for the
tests that show the checks would catch them."""
import numpy as np

from oracle import oracle
from tests import elas_reference as er
from tests import hess_reference as hr

EPS = float(np.finfo(np.float64).eps)


def is_general(U):
    U = np.asarray(U, dtype=np.float64)
    return bool(np.any(U != np.diag(np.diag(U))))


def inverse(U):
    """U^-1 as the library forms it."""
    U = np.ascontiguousarray(U, dtype=np.float64)
    d = U.shape[0]
    if not is_general(U):
        return np.diag(1.0 / np.diag(U))
    with oracle.set_cell(U):
        return np.array(oracle.set_cell.inverse()[:d, :d])


def _matvec(A, v, general):
    """A v per particle (v: [n, d]) in the wrap's operation order."""
    d = A.shape[0]
    if not general:
        return v * np.diag(A)[None, :]
    out = np.empty_like(v)
    for r in range(d):
        t = A[r, 0] * v[:, 0] + A[r, 1] * v[:, 1]
        if d == 3:
            t = t + A[r, 2] * v[:, 2]
        out[:, r] = t
    return out


def frac(x, U, Uinv=None):
    U = np.asarray(U, dtype=np.float64)
    return _matvec(inverse(U) if Uinv is None else Uinv, np.asarray(x, dtype=np.float64), is_general(U))


def cart(f, U):
    U = np.asarray(U, dtype=np.float64)
    return _matvec(U, np.asarray(f, dtype=np.float64), is_general(U))


def export_wrap(x, img, U):
    """What md_download returns for the stored (x, img): the lazy wrap of k_export -- in a general cell a particle with
    any fractional coordinate outside [0, 1) becomes U (frac - floor(frac)); in a diagonal cell each coordinate on its own."""
    U = np.asarray(U, dtype=np.float64)
    x = np.array(x, dtype=np.float64)
    img = np.array(img, dtype=np.int64)
    if is_general(U):
        fr = frac(x, U)
        out = np.any((fr < 0.0) | (fr >= 1.0), axis=1)
        nn = np.floor(fr)
        xw = cart(fr - nn, U)
        x[out] = xw[out]
        img[out] += nn[out].astype(np.int64)
    else:
        L, iL = np.diag(U), 1.0 / np.diag(U)
        for c in range(U.shape[0]):
            out = (x[:, c] < 0.0) | (x[:, c] >= L[c])
            fr = iL[c] * x[:, c]
            nn = np.floor(fr)
            x[out, c] = (L[c] * (fr - nn))[out]
            img[out, c] += nn[out].astype(np.int64)
    return x, img


def affine(x, img, U_old, U_new, variant=None):
    """MD_CELL_AFFINE on the stored (x, img): frac = U_old^-1 x, n = floor(frac), img + n, U_new (frac - n).
    variant "new_inverse": frac taken with the NEW cell's inverse."""
    fr = frac(x, U_new if variant == "new_inverse" else U_old)
    nn = np.floor(fr)
    return cart(fr - nn, U_new), np.asarray(img, dtype=np.int64) + nn.astype(np.int64)


def lattice_matrix(U_old, U_new):
    """The integer M = U_old^-1 U_new of a lattice-preserving change, by the host's rules (ValueError otherwise)."""
    U_old, U_new = np.asarray(U_old, dtype=np.float64), np.asarray(U_new, dtype=np.float64)
    Mf = inverse(U_old) @ U_new
    M = np.rint(Mf)
    if np.any(np.abs(Mf - M) > 1e-9) or np.any(np.abs(M) > 2.0 ** 10):
        raise ValueError("U_old^-1 U_new is not integer")
    M = M.astype(np.int64)
    if round(float(np.linalg.det(M.astype(np.float64)))) not in (1, -1):
        raise ValueError("|det M| != 1")
    scale = (np.abs(U_old)[:, :, None] * np.abs(M.astype(np.float64))[None, :, :]).max(axis=1)
    if np.any(np.abs(U_old @ M.astype(np.float64) - U_new) > 8.0 * EPS * scale):
        raise ValueError("U_old M != U_new")
    return M


def integer_inverse(M):
    """M^-1 of a unimodular integer matrix, exactly (adjugate times the determinant)."""
    M = np.asarray(M, dtype=np.int64)
    d = M.shape[0]
    if d == 2:
        det = int(M[0, 0] * M[1, 1] - M[0, 1] * M[1, 0])
        adj = np.array([[M[1, 1], -M[0, 1]], [-M[1, 0], M[0, 0]]], dtype=np.int64)
    else:
        c = lambda a, b, e, f: int(M[a, b] * M[e, f])
        adj = np.array([[c(1, 1, 2, 2) - c(1, 2, 2, 1), c(0, 2, 2, 1) - c(0, 1, 2, 2), c(0, 1, 1, 2) - c(0, 2, 1, 1)],
                        [c(1, 2, 2, 0) - c(1, 0, 2, 2), c(0, 0, 2, 2) - c(0, 2, 2, 0), c(0, 2, 1, 0) - c(0, 0, 1, 2)],
                        [c(1, 0, 2, 1) - c(1, 1, 2, 0), c(0, 1, 2, 0) - c(0, 0, 2, 1), c(0, 0, 1, 1) - c(0, 1, 1, 0)]],
                       dtype=np.int64)
        det = int(M[0, 0] * adj[0, 0] + M[0, 1] * adj[1, 0] + M[0, 2] * adj[2, 0])
    assert det in (1, -1)
    return det * adj


def lattice(x, img, U_old, U_new, mark=None, variant=None):
    """MD_CELL_LATTICE on the stored (x, img): img' = M^-1 img in integers, then the lazy wrap of the new cell and its shift.
    mark = (frac0, img0) is carried along: M^-1 frac0 (row times vector in doubles), M^-1 img0.  Returns (x, img, mark).
    variants: "wrong_sign" (img' = -M^-1 img), "m_not_inverse" (M used for M^-1), "mark_untouched"."""
    M = lattice_matrix(U_old, U_new)
    Mi = M if variant == "m_not_inverse" else integer_inverse(M)
    if variant == "wrong_sign":
        Mi = -Mi
    img2 = np.asarray(img, dtype=np.int64) @ Mi.T
    xw, img2 = export_wrap(x, img2, U_new)
    if np.any(np.abs(img2) > 2 ** 31 - 1):
        raise OverflowError("image count out of int32")
    if mark is not None and variant != "mark_untouched":
        f0, i0 = mark
        mark = (_matvec(Mi.astype(np.float64), np.asarray(f0, dtype=np.float64), True), np.asarray(i0, dtype=np.int64) @ Mi.T)
    return xw, img2, mark


def mark_of(x, img, U):
    """md_nonaffine_mark on the stored (x, img)."""
    return frac(x, U), np.array(img, dtype=np.int64)


def nonaffine(x, img, U, mark):
    """md_nonaffine on the stored (x, img): (u [n, d], sums[8]); the sums in longdouble (the device's differ by the rounding
    of its own summation order)."""
    f0, i0 = mark
    d = (frac(x, U) - f0) + (np.asarray(img, dtype=np.int64) - i0).astype(np.float64)
    u = cart(d, U)
    u2 = u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]
    if u.shape[1] == 3:
        u2 = u2 + u[:, 2] * u[:, 2]
    sums = np.zeros(8)
    sums[:u.shape[1]] = u.astype(np.longdouble).sum(axis=0)
    sums[3] = u2.astype(np.longdouble).sum()
    sums[4] = (u2 * u2).astype(np.longdouble).sum()
    sums[5] = u2.max()
    sums[6] = int(np.flatnonzero(u2 == u2.max())[0])
    sums[7] = len(u)
    return u, sums


def unwrapped(x, img, U):
    """x + U img in longdouble."""
    return np.asarray(x, dtype=np.longdouble) + np.asarray(img, dtype=np.longdouble) @ np.asarray(U, dtype=np.longdouble).T


def unwrapped_bound(U_list, img_list, ulps=8.0):
    """The rounding bound on a change of x + U img through remaps (per coordinate).

    One remap forms frac = U^-1 x (d products and d - 1 sums of terms up to |U^-1| |x| <= about 1 each, plus the cofactor
    inverse's own relative error of a few ulp), frac - n (exact or one rounding) and U (frac - n) (d products, d - 1 sums of
    terms up to |U|): each step is off by at most a few ulp of max |U|, because an error e in frac becomes |U| e in x.  The
    image term U img is exact in the reference (longdouble) but the CELL differs between the two representations of one
    lattice by the rounding of U_old M, up to 1 ulp of |U| per entry, times |img|.  Together:
    ulps * eps * max |U| * (1 + max |img|) per remap, with ulps = 8 covering d <= 3 (3 products + 2 sums, twice, plus the
    inverse)."""
    return sum(ulps * EPS * float(np.abs(U).max()) * (1.0 + float(np.abs(np.asarray(i, dtype=np.float64)).max()))
               for U, i in zip(U_list, img_list))


def face_distances(U):
    inv = np.linalg.inv(np.asarray(U, dtype=np.float64))
    return 1.0 / np.sqrt((inv * inv).sum(axis=1))


# ---------------------------------------------------------------------------------------------------------------------
# the AQS loop on the CPU: strain in numpy, minimise with the oracle's FIRE under oracle.set_cell
# ---------------------------------------------------------------------------------------------------------------------
AQS_FIRE = dict(max_steps=30000, dt_initial=0.002, dt_max=0.02)     # tests/test_gpu_hessian.py _relax's steps
AQS_STEP, AQS_NSTEPS, AQS_TOL = 1e-3, 3, 1e-9                       # sized in tests/test_deformation.py: no plastic event


def stress_of(x, U, cutoff, kind, params, diam):
    """The configurational stress (1/V) sum_pairs t del_a del_b in elas_reference.COMPONENTS order (tension positive)."""
    d = np.asarray(x).shape[1]
    _, _, dl, t, _ = er.pair_terms(x, U, cutoff, kind, params, diam)
    return np.array([float((t * dl[:, a] * dl[:, b]).sum()) for a, b in er.COMPONENTS[d]]) / er.volume(U)


def aqs_reference(x, diam, U, cutoff, kind, params, strain_step, nsteps, tol, plane=(0, 1)):
    """nsteps increments of simple shear from the frame (x in the cell U, images 0): per increment the affine remap above,
    the mark, oracle.fire_minimize(use_cells=False) under oracle.set_cell, then energy, stress and the non-affine sums.
    Returns dict(energy, stress [nsteps, nc], d2, converged, steps, x (the last minimum), cell)."""
    pot = oracle.make_pot(kind, params)
    x = np.array(x, dtype=np.float64)
    n, d = x.shape
    img = np.zeros((n, d), dtype=np.int64)
    U = np.array(U, dtype=np.float64)
    F = np.eye(d)
    F[plane[0], plane[1]] = strain_step
    out = dict(energy=[], stress=[], d2=[], converged=[], steps=[])
    for _ in range(nsteps):
        U_new = F @ U
        x, img = affine(x, img, U, U_new)
        U = U_new
        mark = mark_of(x, img, U)
        with oracle.set_cell(U):
            r = oracle.fire_minimize(x, img.astype(np.int32), diam, np.diag(U).copy(), cutoff, pot, tol=tol, use_cells=False,
                                     **AQS_FIRE)
        x, img = r["x"], r["img"].astype(np.int64)
        _, sums = nonaffine(x, img, U, mark)
        out["energy"].append(r["energy"] / n)
        out["stress"].append(stress_of(x, U, cutoff, kind, params, diam))
        out["d2"].append(sums[3] / n)
        out["converged"].append(r["converged"])
        out["steps"].append(r["steps"])
    out = {k: np.array(v) for k, v in out.items()}
    out.update(x=x, img=img, cell=U)
    return out
