"""The contract of md_chi4_* (include/mdhip.h) restated in numpy: the displacement and d2 of section
11 with every operation rounded on its own, the strict test d2 < a*a for the mask, and W in extended precision over the
slow set of the ORIGIN frame (tests/test_gpu_sq.py's _rho_true; its _bound is the bound W is held to)."""
import numpy as np

from tests.test_gpu_sq import _bound, _rho_true  # noqa: F401  (re-exported: the tests take both from here)


def displacement(x0, n0, x1, n1, U):
    """del_c = (x1 - x0) + ((U_c0 dn0 + U_c1 dn1) + U_c2 dn2), d2 = (del0^2 + del1^2) + del2^2, each operation rounded."""
    d = x0.shape[1]
    dn = n1.astype(np.float64) - n0.astype(np.float64)
    de = np.empty_like(x0)
    for c in range(d):
        t = U[c, 0] * dn[:, 0] + U[c, 1] * dn[:, 1]
        if d == 3:
            t = t + U[c, 2] * dn[:, 2]
        de[:, c] = (x1[:, c] - x0[:, c]) + t
    d2 = de[:, 0] * de[:, 0] + de[:, 1] * de[:, 1]
    if d == 3:
        d2 = d2 + de[:, 2] * de[:, 2]
    return de, d2


def overlap(x0, n0, x1, n1, U, a):
    """(slow uint8[N], Q): w_i = 1 iff d2 < a2, a2 = a*a in fp64; strict."""
    U = np.asarray(U, dtype=np.float64)
    U = U if U.ndim == 2 else np.diag(U)
    _, d2 = displacement(x0, n0, x1, n1, U)
    slow = (d2 < float(a) * float(a)).astype(np.uint8)
    return slow, int(slow.sum())


def w_true(x0, U, n, slow):
    """W(q_v) = sum over the slow particles of exp(+2 pi i n_v.f(x0)), extended precision; complex128[nvec]."""
    U = np.asarray(U, dtype=np.float64)
    U = U if U.ndim == 2 else np.diag(U)
    re, im = _rho_true(x0[np.asarray(slow, dtype=bool)], U, n)
    return re + 1j * im
