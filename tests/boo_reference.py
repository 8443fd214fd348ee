"""The numpy / scipy reference of the bond-orientational order sampler (md_boo_*), shared by tests/test_bond_order.py
(lattice values) and tests/test_gpu_bond_order.py (the device against it).  Nothing here comes from the code under test:
Y_lm is scipy.special.lpmv (which carries the Condon-Shortley phase) times exp(i m atan2(y, x)), psi_k is
exp(i k atan2(y, x)), and every sum is a plain numpy sum over the bonds of a particle."""
import math

import numpy as np
from scipy.special import lpmv


def ylm(l, de):
    """Y_lm(de / |de|) for m = 0..l: complex (P, l + 1)."""
    de = np.asarray(de, dtype=np.float64)
    r = np.sqrt((de * de).sum(axis=1))
    ct = de[:, 2] / r
    phi = np.arctan2(de[:, 1], de[:, 0])
    out = np.empty((len(de), l + 1), dtype=np.complex128)
    for m in range(l + 1):
        norm = math.sqrt((2 * l + 1) / (4.0 * math.pi) * math.factorial(l - m) / math.factorial(l + m))
        out[:, m] = norm * lpmv(m, l, ct) * np.exp(1j * m * phi)
    return out


def psik(k, de):
    """((de_x + i de_y) / |de|)^k: complex (P, 1)."""
    de = np.asarray(de, dtype=np.float64)
    return np.exp(1j * k * np.arctan2(de[:, 1], de[:, 0]))[:, None]


def _weights(nm):
    w = np.full(nm, 2.0)
    w[0] = 1.0
    return w


def bond_order(n, pairs, de, order, threshold, min_conn):
    """The contract of include/mdhip.h for the unordered pairs (a, b) with displacement de = x_b(+translation) - x_a.
    Returns a dict: nnb, qlm (N, NM), q, qbar, conn, solid, sij (one per directed bond, with bond_i, bond_j), fr[8]."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    de = np.asarray(de, dtype=np.float64)
    dim = de.shape[1]
    bi = np.concatenate([pairs[:, 0], pairs[:, 1]])
    bj = np.concatenate([pairs[:, 1], pairs[:, 0]])
    dd = np.concatenate([de, -de])
    if dim == 3:
        y, pref = ylm(order, dd), 4.0 * math.pi / (2 * order + 1)
    else:
        y, pref = psik(order, dd), 1.0
    nm = y.shape[1]
    w = _weights(nm)
    nnb = np.bincount(bi, minlength=n).astype(np.int64)
    s = np.zeros((n, nm), dtype=np.complex128)
    np.add.at(s, bi, y)
    qlm = np.where(nnb[:, None] > 0, s / np.maximum(nnb, 1)[:, None], 0.0)
    norm2 = (w * np.abs(qlm) ** 2).sum(axis=1)
    q = np.sqrt(pref * norm2)
    acc = np.zeros((n, nm), dtype=np.complex128)
    np.add.at(acc, bi, qlm[bj])
    Q = (qlm + acc) / (nnb + 1.0)[:, None]
    qbar = np.sqrt(pref * (w * np.abs(Q) ** 2).sum(axis=1))
    nrm = np.sqrt(norm2)
    dot = (w * (qlm[bi] * np.conj(qlm[bj])).real).sum(axis=1)
    den = nrm[bi] * nrm[bj]
    sij = np.where(den > 0.0, dot / np.where(den > 0.0, den, 1.0), 0.0)
    conn = np.bincount(bi, weights=(sij > threshold).astype(np.float64), minlength=n).astype(np.int64)
    solid = conn >= min_conn
    tot_n = float(nnb.sum())
    G = (nnb[:, None] * qlm).sum(axis=0) / tot_n if tot_n > 0 else np.zeros(nm)
    fr = np.array([math.fsum(q), math.fsum(q * q), math.fsum(qbar), math.fsum(qbar * qbar), tot_n, float(conn.sum()),
                   float(solid.sum()), math.sqrt(pref * float((w * np.abs(G) ** 2).sum()))])
    return dict(nnb=nnb, qlm=qlm, q=q, qbar=qbar, conn=conn, solid=solid, sij=sij, bond_i=bi, bond_j=bj, fr=fr)


def bins(values, nbins):
    """The stated bin rule: bin = min((int)(value * nbins), nbins - 1), counted."""
    b = np.minimum((np.asarray(values) * nbins).astype(np.int64), nbins - 1)
    return np.bincount(b, minlength=nbins).astype(np.int64)


def clamped_counts(values):
    """Counts of integer values clamped to 32 (33 bins)."""
    return np.bincount(np.minimum(np.asarray(values, dtype=np.int64), 32), minlength=33).astype(np.int64)


def brute_pairs(x, box, r):
    """(pairs a < b, de) within r of an orthorhombic periodic box by the minimum image, O(N^2): small lattices only."""
    x = np.asarray(x, dtype=np.float64)
    L = np.asarray(box, dtype=np.float64)
    d = x[None, :, :] - x[:, None, :]
    d -= L * np.rint(d / L)
    r2 = (d * d).sum(axis=2)
    a, b = np.nonzero(np.triu(r2 < r * r, k=1))
    return np.stack([a, b], axis=1), d[a, b]


def fcc(nc, a):
    basis = np.array([[0, 0, 0], [0.5, 0.5, 0], [0.5, 0, 0.5], [0, 0.5, 0.5]])
    cells = np.array([[i, j, k] for i in range(nc) for j in range(nc) for k in range(nc)], dtype=np.float64)
    return ((cells[:, None, :] + basis[None, :, :]).reshape(-1, 3) * a), np.full(3, nc * a)


def bcc(nc, a):
    basis = np.array([[0, 0, 0], [0.5, 0.5, 0.5]])
    cells = np.array([[i, j, k] for i in range(nc) for j in range(nc) for k in range(nc)], dtype=np.float64)
    return ((cells[:, None, :] + basis[None, :, :]).reshape(-1, 3) * a), np.full(3, nc * a)


def hcp(nc, a):
    """Ideal hcp (c / a = sqrt(8/3)) in its orthorhombic cell a x sqrt(3) a x c of 4 atoms."""
    cell = np.array([a, math.sqrt(3.0) * a, math.sqrt(8.0 / 3.0) * a])
    basis = np.array([[0, 0, 0], [0.5, 0.5, 0], [0.5, 5.0 / 6.0, 0.5], [0, 1.0 / 3.0, 0.5]])
    cells = np.array([[i, j, k] for i in range(nc) for j in range(nc) for k in range(nc)], dtype=np.float64)
    return ((cells[:, None, :] + basis[None, :, :]).reshape(-1, 3) * cell), nc * cell


def hexagonal(nx, ny, a):
    """2-D triangular lattice commensurate with its box: nx x ny rectangular cells a x sqrt(3) a of 2 atoms."""
    cell = np.array([a, math.sqrt(3.0) * a])
    basis = np.array([[0.0, 0.0], [0.5, 0.5]])
    cells = np.array([[i, j] for i in range(nx) for j in range(ny)], dtype=np.float64)
    return ((cells[:, None, :] + basis[None, :, :]).reshape(-1, 2) * cell), np.array([nx, ny]) * cell
