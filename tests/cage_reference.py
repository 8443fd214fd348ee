"""Numpy reference for the cage-relative dynamics and bond-breaking sampler (md_cage_*): nothing from the code under test.

Inputs are two frames as md_download returns them (wrapped x, image counts, particle-id order), the cell, the origin's
bonds as unordered pairs (a, b) with del = x_b(+translation) - x_a, and the diameters.  Every bond is an entry of both
ends: (j = b, +del) in a's list and (j = a, -del) in b's."""
import numpy as np

NHIST = 33


def cell_matrix(cell):
    c = np.asarray(cell, dtype=np.float64)
    return c if c.ndim == 2 else np.diag(c)


def d2_of(v):
    d2 = v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]
    if v.shape[-1] == 3:
        d2 = d2 + v[..., 2] * v[..., 2]
    return d2


def displacements(x0, im0, x1, im1, cell):
    """Del_c = (x1_c - x0_c) + ((U_c0 dn_0 + U_c1 dn_1) + U_c2 dn_2): the wrapped difference, then the lattice translation of
    the exact image difference."""
    U = cell_matrix(cell)
    d = x0.shape[1]
    dn = np.asarray(im1, dtype=np.float64) - np.asarray(im0, dtype=np.float64)
    de = np.empty_like(x0, dtype=np.float64)
    for c in range(d):
        t = U[c, 0] * dn[:, 0] + U[c, 1] * dn[:, 1]
        if d == 3:
            t = t + U[c, 2] * dn[:, 2]
        de[:, c] = (x1[:, c] - x0[:, c]) + t
    return de


def threshold2(r, diam, i, j, scaled):
    """(r s)(r s), s = (sigma_i + sigma_j) / 2.0 if scaled else 1.0."""
    s = (diam[i] + diam[j]) / 2.0 if scaled else np.ones(len(i))
    t = r * s
    return t * t


def directed(pairs, de):
    """The entries (i, j, del_ij) of both ends of every bond, grouped by i (the order within a group carries no meaning)."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    de = np.asarray(de, dtype=np.float64).reshape(len(pairs), -1)
    i = np.concatenate([pairs[:, 0], pairs[:, 1]])
    j = np.concatenate([pairs[:, 1], pairs[:, 0]])
    v = np.concatenate([de, -de])
    o = np.argsort(i, kind="stable")
    return i[o], j[o], v[o]


def cage(x0, im0, x1, im1, cell, pairs, de, diam, r_break, scaled=False, q=()):
    """Per particle: nnb, dcr (Del^CR), d2, broken; per row: sums = [sum d2, sum d4, sum s(q)...], counts = [particles with
    neighbours, sum n_i, surviving bonds], hist = particles by broken count; also delta (the plain displacements) and the
    directed entries with each bond's squared length at the sample and its squared break radius (for the guards)."""
    n, d = x0.shape
    diam = np.asarray(diam, dtype=np.float64)
    delta = displacements(x0, im0, x1, im1, cell)
    i, j, v = directed(pairs, de)
    nnb = np.bincount(i, minlength=n).astype(np.int64)
    mean = np.zeros((n, d))
    np.add.at(mean, i, delta[j])
    has = nnb > 0
    mean[has] /= nnb[has, None]
    dcr = np.where(has[:, None], delta - mean, 0.0)
    d2 = d2_of(dcr)
    b = v + (delta[j] - delta[i])
    b2 = d2_of(b) if len(i) else np.zeros(0)
    thr2 = threshold2(r_break, diam, i, j, scaled)
    gone = b2 >= thr2
    broken = np.bincount(i[gone], minlength=n).astype(np.int64)
    sums = [d2[has].sum(), (d2[has] * d2[has]).sum()]
    for qq in q:
        s = np.cos(qq * dcr[:, 0])
        for c in range(1, d):
            s = s + np.cos(qq * dcr[:, c])
        sums.append(s[has].sum())
    counts = np.array([np.count_nonzero(has), nnb.sum(), nnb.sum() - broken.sum()], dtype=np.int64)
    hist = np.bincount(broken[has], minlength=NHIST).astype(np.int64)
    return dict(nnb=nnb, dcr=dcr, d2=d2, broken=broken, sums=np.array(sums), counts=counts, hist=hist, delta=delta,
                i=i, j=j, b2=b2, thr2=thr2)


def hexagonal_patch(a=1.0):
    """A 3 x 3 patch of the hexagonal lattice (rows offset by a / 2, row spacing a sqrt(3) / 2), far from every face of
    an open 40 x 40 cell, and its nearest-neighbour bonds, found by hand: ids run along the rows,
        6 7 8
         3 4 5
        0 1 2
    with row 1 shifted right by a / 2.  Returns (x, cell, pairs, del)."""
    h = a * np.sqrt(3.0) / 2.0
    x = np.array([[ix * a + (iy % 2) * 0.5 * a, iy * h] for iy in range(3) for ix in range(3)]) + 10.0
    pairs = np.array([[0, 1], [1, 2], [3, 4], [4, 5], [6, 7], [7, 8],           # along the rows
                      [0, 3], [1, 3], [1, 4], [2, 4], [2, 5],                   # row 0 - row 1
                      [3, 6], [3, 7], [4, 7], [4, 8], [5, 8]])                  # row 1 - row 2
    return x, np.array([40.0, 40.0]), pairs, x[pairs[:, 1]] - x[pairs[:, 0]]
