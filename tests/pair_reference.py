"""Pair displacements in the oracle's canonical forms, restated in numpy, and a brute-force pair search on one frame:
what the references of the row-walking samplers start from.  Nothing here comes from the code under test.  (Moved here
from tests/test_gpu_stress.py so that the sampler audit can share them.)"""
import numpy as np


def canon_delta(x, box, pairs):
    """oracle/md_oracle.c canon_d2's displacement for the (a < b) pairs: b translated, every operation rounded on its own
    (the form _canon_d2 of tests/test_gpu_rdf.py squares)."""
    a, b = x[pairs[:, 0]], x[pairs[:, 1]]
    L = np.asarray(box, dtype=np.float64)
    d0 = b - a
    half = 0.5 * L
    s = np.where(d0 > half, -1.0, np.where(d0 < -half, 1.0, 0.0))
    return (b + s * L) - a


def tric_delta(x, U, pairs):
    """oracle/md_oracle.c tric_d2's displacement: the 3^d translations t_r = (s0 U_r0 + s1 U_r1) + s2 U_r2 in its loop
    order, the first strict minimum of d2 kept."""
    d = x.shape[1]
    a, b = x[pairs[:, 0]], x[pairs[:, 1]]
    best = np.full(len(pairs), 1e300)
    out = np.zeros_like(a)
    for s2 in ((-1, 0, 1) if d == 3 else (0,)):
        for s1 in (-1, 0, 1):
            for s0 in (-1, 0, 1):
                de = np.empty_like(a)
                for r in range(d):
                    t = float(s0) * U[r, 0] + float(s1) * U[r, 1]
                    if d == 3:
                        t = t + float(s2) * U[r, 2]
                    de[:, r] = (b[:, r] + t) - a[:, r]
                d2 = de[:, 0] * de[:, 0] + de[:, 1] * de[:, 1]
                if d == 3:
                    d2 = d2 + de[:, 2] * de[:, 2]
                better = d2 < best
                best = np.where(better, d2, best)
                out[better] = de[better]
    return out


def d2_of(de):
    d2 = de[:, 0] * de[:, 0] + de[:, 1] * de[:, 1]
    if de.shape[1] == 3:
        d2 = d2 + de[:, 2] * de[:, 2]
    return d2


def is_orthorhombic(U):
    U = np.asarray(U, dtype=np.float64)
    return U.ndim == 1 or np.count_nonzero(U - np.diag(np.diagonal(U))) == 0


def brute_pairs(x, U, r):
    """(pairs a < b, del, d2) of every pair of the frame x with d2 < (r (1 + 1e-6))^2 in the periodic cell U (d x d, columns
    = lattice vectors), O(N^2): every pair a < b is looked at.  r must stay below half the smallest face distance; then a
    vector shorter than r has fractional coordinates below 1/2, so rounding the fractional difference finds it.  That
    search only selects candidates; del and d2 of the candidates are the canonical forms above."""
    x = np.asarray(x, dtype=np.float64)
    U = np.asarray(U, dtype=np.float64)
    U = np.diag(U) if U.ndim == 1 else U
    n = len(x)
    perp = 1.0 / np.linalg.norm(np.linalg.inv(U), axis=1)
    wide = r * (1.0 + 1e-6)
    assert wide < 0.5 * perp.min(), "brute_pairs: r must be below half the smallest face distance"
    uinv = np.linalg.inv(U)
    found = []
    ids = np.arange(n)
    for a0 in range(0, n, 128):                               # 128 rows of the N x N table at a time
        a = ids[a0:a0 + 128]
        fr = (x[None, :, :] - x[a, None, :]) @ uinv.T
        de = (fr - np.rint(fr)) @ U.T
        ia, ib = np.nonzero(((de * de).sum(axis=2) < wide * wide * (1.0 + 1e-9)) & (ids[None, :] > a[:, None]))
        found.append(np.stack([a[ia], ib], axis=1).astype(np.int64))
    pairs = np.concatenate(found) if found else np.zeros((0, 2), dtype=np.int64)
    de = canon_delta(x, np.diagonal(U), pairs) if is_orthorhombic(U) else tric_delta(x, U, pairs)
    d2 = d2_of(de) if len(pairs) else np.zeros(0)
    keep = d2 < wide * wide
    return pairs[keep], de[keep], d2[keep]
