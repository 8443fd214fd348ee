"""The density modes rho(q) = sum_j exp(+2 pi i n.f_j) in extended precision and the bound the device's rho is held to
(DESIGN.md section 12 derives it).  Nothing here comes from the code under test.  (Moved here from tests/test_gpu_sq.py so
that the sampler audit can share them.)"""
import numpy as np

LD = np.longdouble
PI_LD = LD(3.141592653589793) + LD(1.2246467991473532e-16)


def inv_ld(U):
    """U^-1 in extended precision (adjugate / determinant)."""
    d = U.shape[0]
    A = U.astype(LD)
    if d == 2:
        det = A[0, 0] * A[1, 1] - A[0, 1] * A[1, 0]
        return np.array([[A[1, 1], -A[0, 1]], [-A[1, 0], A[0, 0]]], dtype=LD) / det
    C = np.empty((3, 3), dtype=LD)
    for r in range(3):
        for c in range(3):
            r1, r2 = (r + 1) % 3, (r + 2) % 3
            c1, c2 = (c + 1) % 3, (c + 2) % 3
            C[r, c] = A[r1, c1] * A[r2, c2] - A[r1, c2] * A[r2, c1]
    det = A[0, 0] * C[0, 0] + A[0, 1] * C[0, 1] + A[0, 2] * C[0, 2]
    return C.T / det


def rho_true(x, U, n):
    """sum_j exp(+2 pi i n.f_j), f = U^-1 x, in extended precision; returns (re, im) as float64 arrays."""
    assert np.finfo(LD).eps < 2e-19, "np.longdouble is not an extended type here"
    f = x.astype(LD) @ inv_ld(U).T
    re, im = np.empty(n.shape[0]), np.empty(n.shape[0])
    for v0 in range(0, n.shape[0], 256):
        t = f @ n[v0:v0 + 256].astype(LD).T
        r = t - np.rint(t)
        ph = (2 * PI_LD) * r
        re[v0:v0 + 256] = np.sum(np.cos(ph), axis=0).astype(np.float64)
        im[v0:v0 + 256] = np.sum(np.sin(ph), axis=0).astype(np.float64)
    return re, im


def bound(N, U, n):
    kappa = float(np.max(np.sum(np.abs(np.linalg.inv(U)) @ np.abs(U), axis=1)))
    if np.count_nonzero(U - np.diag(np.diagonal(U))) == 0:
        kappa = 1.0
    return N * (32.0 * kappa * np.sum(np.abs(n), axis=1) + 128.0) * 2.0 ** -53
