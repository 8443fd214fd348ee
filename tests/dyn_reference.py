"""The contract of md_dyn_* (include/mdhip.h) restated in numpy: the unwrapped displacement between
two downloaded frames with every operation rounded on its own, and the van Hove bin rule.  Nothing here comes from the
code under test.  (Moved here from tests/test_gpu_dynamics.py so that the sampler audit can share them.)"""
import numpy as np

TOL = 1e-12         # tests/test_gpu_dynamics.py: relative on sum d2 and sum d4, absolute on sum s(q) / (d N)


def restate(x0, n0, x1, n1, U):
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


def bin_counts(d2, r_max, nbins):
    delta = r_max / nbins
    rk = np.arange(nbins + 1, dtype=np.float64) * delta
    e2 = rk * rk
    d2 = d2[d2 < e2[-1]]
    k = np.searchsorted(e2, d2, "right") - 1
    return np.bincount(k, minlength=nbins).astype(np.int64)
