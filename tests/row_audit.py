"""A direct audit of the Verlet rows: pure numpy, no device.

DESIGN.md section 3 ("How the list is kept valid") derives "the rows the force kernel walks hold every pair within the
cutoff" from three facts -- what the outer rows hold at the build positions x0, what the inner rows hold at the prune
positions x1, and the displacement checks that retire either before its guarantee runs out.  check_rows() tests those facts,
and the conclusion, on a snapshot of the rows themselves: what MDDevice.list_rows() returns (snapshot_of() below), or what
the numpy model of tests/test_row_audit.py builds.

The reference is brute force in fp64 over all ordered (i, j, n), n in {-1, 0, 1}^d: the squared distance of x_j + n . A from
x_i in the reference form the oracle uses (d2_ref: the translation t_r = (n_0 A_r0 + n_1 A_r1) + n_2 A_r2 added with one
rounding, differences, products and sums rounded left to right, no fma).  (A pre-filter on fractional coordinates skips
blocks of (i, j) that cannot be within the radius: |f_j + n - f_i|_c <= r / w_c is necessary, w_c the distance between the
faces of direction c.)  The box rules give at least three cells of width >= rl per axis, so a pair has at most one image
within rl: asserted on every input.

Invariants (rl = rc + skin, rin = rc + inner skin; B = 1e-12):

  O1 completeness  every (i, j, n) with d2(x0) <= rl^2 (1 - B) is an entry of row i
  O2 symmetry      (i, j, n) in row i  <=>  (j, i, -n) in row j
  O3 hygiene       no entry with i == j, no (j, n) twice in a row, every id in [0, n), every image component in {-1, 0, 1}
                   (0 beyond the dimension)
  O4 tightness     every entry has d2(x0) <= the build path's own test radius plus its rounding slack (below)
  I1               inner is a subset of outer, as sets of (j, n) per row
  I2               the inner row is a subsequence of the outer row (the same relative order)
  I3 completeness  every outer entry with d2(x1) <= rin^2 (1 - B) is in the inner row
  I4               no inner entry has d2(x1) > rin^2 (1 + B)
  V1               list_valid  =>  max_i |pos_i - x0_i| <= skin / 2 (+ 4 spacings of the largest coordinate)
  V2               inner_valid =>  max_i |pos_i - x1_i| <= min(inner_skin / 2, skin / 2 - d1) (+ 4 spacings), and the
                   reported d1 >= max_i |x1_i - x0_i|
  V3               the rows the next force evaluation walks (inner if inner_valid, else outer) hold every (i, j, n) with
                   d2(pos) <= rc^2 (1 - B)

The norm of V1 and V2 is the Euclidean one, per particle: k_step_tile, k_kickdrift (and k_force_tile's prune epilogue for
d1) sum the squared components of x - x_ref with an fma chain and compare with the squared limit; d1 is the square root
of the largest such sum.  The 4 spacings cover the roundings of that chain against numpy's.

The bands of relative B in d2 are knife-edge exclusions: a pair inside one is neither required nor forbidden.  They are
counted (band_rl: pairs at x0 about rl^2; band_rin: outer entries at x1 about rin^2; band_rc: pairs at pos about rc^2);
the callers cap the counts.

O4, the bound per build path.
  * two-kernel fallback and the build without tiles (k_build_list): the test is d2 <= rl * rl in fp64 on the same
    coordinates the rows stand for (ghosts are x_owner + n . A, one rounding), d2 by an fma chain where the reference form
    has none: both carry at most d + 1 roundings of relative 2^-53 each, so an accepted entry has
    d2_ref <= rl^2 (1 + 16 * 2^-52).
  * fused build (k_build_tile): the test is d2~ <= rl2f in fp32, rl2f = fl32(rl^2 (1 + 1e-4)), on coordinates
    c~ = fl32(x - org) relative to the tile's first particle.  With u = 2^-24 and X a bound on |x - org| per component
    (every staged particle lies in the cell or its one-cell ghost layer: X = (5/3) max_r sum_k |A_rk|):
    |c~ - c| <= u X, a difference carries 2 u X + u |d~_c|, and the three products and sums of d2~ at most (d + 1) u
    relative.  An accepted entry therefore has
        d <= r_acc + sqrt(d) u (2 X + r_acc),   r_acc^2 = rl^2 (1 + 1e-4) (1 + u) (1 + (d + 2) u),
    and O4 asserts d2_ref(x0) <= that squared.  (The same arithmetic read the other way is why the margin is safe: a pair
    within rl is computed at most sqrt(d) u (2 X + rl) too far, a relative 3e-6 in d2 at X = 40 -- against 1e-4.)
  Largest measured d2(x0) / rl^2 among entries (MI355X, tests/test_gpu_row_audit.py; records, not tolerances): fused build
  1.000099893 against a bound of 1.000103371 (two_words_3d_full); two-kernel fallback and the build without tiles
  0.999999998, with rl put a relative 1e-9 beyond a pair -- never above 1.
"""
import itertools

import numpy as np

BAND = 1e-12
FUSED_MARGIN = 1.0e-4
U32 = 2.0 ** -24
EPS = float(np.finfo(np.float64).eps)
INVARIANTS = ("O1", "O2", "O3", "O4", "I1", "I2", "I3", "I4", "V1", "V2", "V3")


class RowViolation(AssertionError):
    """check: the invariant's name (INVARIANTS) or 'precondition'."""

    def __init__(self, check, msg):
        super().__init__("(%s) %s" % (check, msg))
        self.check = check


def lattice(cell, dim):
    """(dim, dim) matrix, columns = lattice vectors, from box lengths or a cell matrix."""
    c = np.asarray(cell, dtype=np.float64)
    return np.diag(c[:dim]) if c.ndim == 1 else np.ascontiguousarray(c[:dim, :dim])


def image_shift(nv, U):
    """(m, dim) translations n . A in shift_xyz's form: t_r = (n_0 U_r0 + n_1 U_r1) + n_2 U_r2."""
    s = np.asarray(nv, dtype=np.float64)
    dim = U.shape[0]
    t = s[:, [0]] * U[:, 0] + s[:, [1]] * U[:, 1]
    if dim == 3:
        t = t + s[:, [2]] * U[:, 2]
    return t


def _d2_of(d):
    d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]
    if d.shape[-1] == 3:
        d2 = d2 + d[..., 2] * d[..., 2]
    return d2


def entry_d2(x, ent, U):
    """Reference-form squared distance of every entry (id_i, id_j, n...) at positions x."""
    dim = U.shape[0]
    xj = x[ent[:, 1]] + image_shift(ent[:, 2:2 + dim], U)
    return _d2_of(xj - x[ent[:, 0]])


def entry_keys(ent, n):
    """One int64 per entry: ((i n + j) 27 + image code); equal keys <=> equal (i, j, n)."""
    e = ent.astype(np.int64)
    code = (e[:, 2] + 1) + 3 * (e[:, 3] + 1) + 9 * (e[:, 4] + 1)
    return (e[:, 0] * n + e[:, 1]) * 27 + code


def keys_to_entries(keys, n):
    keys = np.asarray(keys, dtype=np.int64)
    code, pair = keys % 27, keys // 27
    out = np.empty((len(keys), 5), dtype=np.int32)
    out[:, 0], out[:, 1] = pair // n, pair % n
    out[:, 2], out[:, 3], out[:, 4] = code % 3 - 1, (code // 3) % 3 - 1, code // 9 - 1
    return out


def reverse_keys(ent, n):
    r = ent.copy()
    r[:, 0], r[:, 1] = ent[:, 1], ent[:, 0]
    r[:, 2:] = -ent[:, 2:]
    return entry_keys(r, n)


def pairs_within(x, U, r2max):
    """Brute force: (keys, d2) of all ordered (i, j, n), n in {-1, 0, 1}^dim, (i, n) != (j, 0), with reference-form
    d2 <= r2max; keys ascending."""
    n, dim = x.shape
    Uinv = np.linalg.inv(U)
    perp = 1.0 / np.linalg.norm(Uinv, axis=1)
    f = x @ Uinv.T
    pad = np.sqrt(r2max) / perp + 1e-9
    flo, fhi = f.min(axis=0), f.max(axis=0)
    ids = np.arange(n)
    keys, d2s = [], []
    for nv in itertools.product((-1, 0, 1), repeat=dim):
        nv3 = np.array(list(nv) + [0] * (3 - dim))
        fj = f + np.array(nv, dtype=np.float64)
        J = ids[np.all((fj <= fhi + pad) & (fj >= flo - pad), axis=1)]
        if J.size == 0:
            continue
        I = ids[np.all((f <= fj[J].max(axis=0) + pad) & (f >= fj[J].min(axis=0) - pad), axis=1)]
        if I.size == 0:
            continue
        xj = x[J] + image_shift(np.array([nv]), U)
        code = int((nv3[0] + 1) + 3 * (nv3[1] + 1) + 9 * (nv3[2] + 1))
        for a in range(0, I.size, 1024):                                 # (blocks of rows: bounded memory)
            Ib = I[a:a + 1024]
            d2 = None
            for c in range(dim):
                dc = xj[None, :, c] - x[Ib, None, c]
                d2 = dc * dc if d2 is None else d2 + dc * dc
            hit = d2 <= r2max
            if not any(nv):
                hit &= Ib[:, None] != J[None, :]
            ii, jj = np.nonzero(hit)
            keys.append((Ib[ii].astype(np.int64) * n + J[jj]) * 27 + code)
            d2s.append(d2[ii, jj])
    keys = np.concatenate(keys) if keys else np.zeros(0, dtype=np.int64)
    d2s = np.concatenate(d2s) if d2s else np.zeros(0)
    order = np.argsort(keys, kind="stable")
    return keys[order], d2s[order]


def required_pairs(x, U, r, what, viol, cache=None):
    """(keys required within r, number of band pairs about r^2); asserts that no pair has two images within r."""
    tag = (what, float(r), x.tobytes()) if cache is not None else None
    if cache is not None and cache.get("tag") == tag:
        return cache["req"], cache["band"]
    r2 = r * r
    keys, d2 = pairs_within(x, U, r2 * (1.0 + BAND))
    pair = keys // 27
    if len(np.unique(pair)) != len(pair):
        viol.append(RowViolation("precondition", "%s: a pair has two periodic images within %.6g" % (what, r)))
    inside = d2 <= r2 * (1.0 - BAND)
    band = int((np.count_nonzero(~inside) + 1) // 2)
    if cache is not None:
        cache.update(tag=tag, req=keys[inside], band=band)
    return keys[inside], band


def fused_bound(rl, U):
    """O4's bound on d2(x0) for rows of the fused build (module docstring)."""
    dim = U.shape[0]
    X = (5.0 / 3.0) * float(np.abs(U).sum(axis=1).max())
    r_acc = np.sqrt(rl * rl * (1.0 + FUSED_MARGIN) * (1.0 + U32) * (1.0 + (dim + 2) * U32))
    return float((r_acc + np.sqrt(dim) * U32 * (2.0 * X + r_acc)) ** 2)


def tightness_bound(info, U):
    rl = info["rl"]
    return fused_bound(rl, U) if info["fused_build"] else rl * rl * (1.0 + 16.0 * EPS)


def _describe(keys, n, limit=4):
    return ", ".join("(%d, %d, %s)" % (e[0], e[1], e[2:].tolist()) for e in keys_to_entries(keys[:limit], n))


def _hygiene(ent, n, dim, name, viol):
    """O3 on one row set; returns the entries that can be looked up (ids and images in range)."""
    ok_id = (ent[:, 0] >= 0) & (ent[:, 0] < n) & (ent[:, 1] >= 0) & (ent[:, 1] < n)
    ok_im = np.all(np.abs(ent[:, 2:]) <= 1, axis=1) & np.all(ent[:, 2 + dim:] == 0, axis=1)
    if not ok_id.all():
        viol.append(RowViolation("O3", "%s rows: %d entries with an id outside [0, %d), first %s"
                                 % (name, np.count_nonzero(~ok_id), n, ent[~ok_id][0].tolist())))
    if not (ok_im | ~ok_id).all():
        viol.append(RowViolation("O3", "%s rows: %d entries with an image outside {-1, 0, 1}^%d, first %s"
                                 % (name, np.count_nonzero(~ok_im & ok_id), dim, ent[~ok_im & ok_id][0].tolist())))
    good = ent[ok_id & ok_im]
    selfs = good[good[:, 0] == good[:, 1]]
    if len(selfs):
        viol.append(RowViolation("O3", "%s rows: %d self entries, first %s" % (name, len(selfs), selfs[0].tolist())))
    k = entry_keys(good, n)
    uk, cnt = np.unique(k, return_counts=True)
    if (cnt > 1).any():
        viol.append(RowViolation("O3", "%s rows: %d entries more than once in a row, first %s"
                                 % (name, np.count_nonzero(cnt > 1), _describe(uk[cnt > 1], n, 1))))
    return good


def check_rows(snapshot, cell, dim, cache=None):
    """Audits one snapshot: dict(info, x0, x1, pos, outer, inner) with info the named fields of MDDevice.list_rows, outer /
    inner int32[m, 5] row entries (id_i, id_j, n_0, n_1, n_2) in row order, rows contiguous (inner: None without valid
    inner rows).  `cell`: box lengths or the cell matrix (columns = lattice vectors).  `cache`: an optional dict that
    carries the brute force at x0 from one snapshot to the next (it changes only with a list build).

    Returns dict(violations, counts): violations a list of RowViolation (empty: every invariant that applies holds), counts
    the coverage figures -- entries and required pairs per row set, the three band counts, the largest d2 / rl^2 and
    d2(x1) / rin^2 among entries, the displacements and their limits."""
    info = snapshot["info"]
    n = int(info["n"])
    U = lattice(cell, dim)
    x0, x1, pos = (np.asarray(snapshot[k], dtype=np.float64) for k in ("x0", "x1", "pos"))
    outer, inner = snapshot.get("outer"), snapshot.get("inner")
    viol = []
    counts = dict(list_valid=int(info["list_valid"]), inner_valid=int(info["inner_valid"]), outer_entries=0,
                  inner_entries=0, required_rl=0, required_rc=0, band_rl=0, band_rin=0, band_rc=0, max_d2_over_rl2=0.0,
                  max_d2x1_over_rin2=0.0, disp0=0.0, disp1=0.0, d1_true=0.0)
    if not info["list_valid"]:
        if outer is not None and len(outer):
            viol.append(RowViolation("precondition", "rows reported for a handle whose list is not valid"))
        return dict(violations=viol, counts=counts)
    if outer is None:
        raise ValueError("check_rows: a valid list needs its outer rows")
    if info["inner_valid"] and inner is None:
        raise ValueError("check_rows: inner_valid is set but the inner rows are missing")
    rc, skin, rl = float(info["rc"]), float(info["skin"]), float(info["rl"])
    spacing = float(np.spacing(max(np.abs(x0).max(), np.abs(x1).max(), np.abs(pos).max(), 1.0)))

    # ---- outer rows against x0
    outer = np.asarray(outer, dtype=np.int32).reshape(-1, 5)
    counts["outer_entries"] = len(outer)
    good = _hygiene(outer, n, dim, "outer", viol)
    ko = entry_keys(good, n)
    ko_sorted = np.unique(ko)
    req, counts["band_rl"] = required_pairs(x0, U, rl, "x0", viol, cache)
    counts["required_rl"] = len(req)
    missing = req[~np.isin(req, ko_sorted)]
    if len(missing):
        viol.append(RowViolation("O1", "%d pairs within rl of x0 are in no outer row, first %s"
                                 % (len(missing), _describe(missing, n))))
    lone = ko[~np.isin(reverse_keys(good, n), ko_sorted)]
    if len(lone):
        viol.append(RowViolation("O2", "%d outer entries without their mirror entry, first %s" % (len(lone), _describe(lone, n))))
    if len(good):
        d2 = entry_d2(x0, good, U)
        bound = tightness_bound(info, U)
        counts["max_d2_over_rl2"] = float(d2.max() / (rl * rl))
        wide = d2 > bound
        if wide.any():
            viol.append(RowViolation("O4", "%d outer entries beyond the build's radius: d2 / rl^2 up to %.9f > %.9f, first %s"
                                     % (np.count_nonzero(wide), d2.max() / (rl * rl), bound / (rl * rl),
                                        good[wide][0].tolist())))

    # ---- inner rows against the outer rows and x1
    walk = ko_sorted
    if info["inner_valid"]:
        rin = rc + float(info["inner_skin"])
        inner = np.asarray(inner, dtype=np.int32).reshape(-1, 5)
        counts["inner_entries"] = len(inner)
        ok = (inner[:, :2] >= 0).all(axis=1) & (inner[:, :2] < n).all(axis=1) & (np.abs(inner[:, 2:]) <= 1).all(axis=1)
        gin = inner[ok]
        ki = entry_keys(gin, n)
        member = np.isin(ki, ko_sorted)
        if not ok.all() or not member.all():
            bad = inner[~ok][0].tolist() if not ok.all() else gin[~member][0].tolist()
            viol.append(RowViolation("I1", "%d inner entries that are not in the outer row, first %s"
                                     % (np.count_nonzero(~ok) + np.count_nonzero(~member), bad)))
        # I2: position of every inner entry in the outer sequence (first occurrence) must increase along a row
        first = np.argsort(ko, kind="stable")
        where = first[np.searchsorted(ko[first], ki[member])]
        row = gin[member][:, 0]
        back = (row[1:] == row[:-1]) & (where[1:] <= where[:-1])
        if back.any():
            viol.append(RowViolation("I2", "%d inner entries out of the outer row's order, first %s"
                                     % (np.count_nonzero(back), gin[member][1:][back][0].tolist())))
        if len(good):
            d2o = entry_d2(x1, good, U)
            need = d2o <= rin * rin * (1.0 - BAND)
            counts["band_rin"] = int((np.count_nonzero((d2o > rin * rin * (1.0 - BAND)) & (d2o <= rin * rin * (1.0 + BAND))) + 1) // 2)
            lost = ko[need][~np.isin(ko[need], np.unique(ki))]
            if len(lost):
                viol.append(RowViolation("I3", "%d outer entries within rin of x1 are not in the inner row, first %s"
                                         % (len(lost), _describe(lost, n))))
        if len(gin):
            d2i = entry_d2(x1, gin, U)
            counts["max_d2x1_over_rin2"] = float(d2i.max() / (rin * rin))
            far = d2i > rin * rin * (1.0 + BAND)
            if far.any():
                viol.append(RowViolation("I4", "%d inner entries beyond rin at x1: d2 / rin^2 up to %.12f, first %s"
                                         % (np.count_nonzero(far), d2i.max() / (rin * rin), gin[far][0].tolist())))
        walk = np.unique(ki)

    # ---- displacement limits
    disp0 = float(np.sqrt(((pos - x0) ** 2).sum(axis=1)).max())
    counts["disp0"], counts["limit0"] = disp0, 0.5 * skin
    if disp0 > 0.5 * skin + 4.0 * spacing:
        viol.append(RowViolation("V1", "a particle is %.6g from its build position, the limit is skin / 2 = %.6g"
                                 % (disp0, 0.5 * skin)))
    if info["inner_valid"]:
        d1 = float(info["d1"])
        d1_true = float(np.sqrt(((x1 - x0) ** 2).sum(axis=1)).max())
        disp1 = float(np.sqrt(((pos - x1) ** 2).sum(axis=1)).max())
        limit1 = min(0.5 * float(info["inner_skin"]), 0.5 * skin - d1)
        counts.update(disp1=disp1, limit1=limit1, d1_true=d1_true, d1=d1)
        if d1 * (1.0 + 4.0 * EPS) + 4.0 * spacing < d1_true:
            viol.append(RowViolation("V2", "reported d1 = %.9g, but max |x1 - x0| = %.9g" % (d1, d1_true)))
        if disp1 > limit1 + 4.0 * spacing:
            viol.append(RowViolation("V2", "a particle is %.6g from its prune position, the limit is %.6g" % (disp1, limit1)))

    # ---- the point of it all
    reqc, counts["band_rc"] = required_pairs(pos, U, rc, "pos", viol)
    counts["required_rc"] = len(reqc)
    gone = reqc[~np.isin(reqc, walk)]
    if len(gone):
        viol.append(RowViolation("V3", "%d pairs within the cutoff are not in the %s rows the next force evaluation walks, first %s"
                                 % (len(gone), "inner" if info["inner_valid"] else "outer", _describe(gone, n))))
    return dict(violations=viol, counts=counts)


def snapshot_of(dev):
    """The snapshot check_rows takes, read from an MDDevice: the outer rows and, when valid, the inner rows."""
    o = dev.list_rows(0)
    snap = dict(info=o["info"], x0=o["x0"], x1=o["x1"], pos=o["pos"], outer=o["entries"], inner=None)
    if o["info"]["inner_valid"]:
        snap["inner"] = dev.list_rows(1)["entries"]
    return snap


def counts_line(name, counts):
    """One line per snapshot or case for the records."""
    c = counts
    return ("%-34s outer %7d  inner %7d | d2/rl^2 <= %.9f  d2(x1)/rin^2 <= %.12f | bands rl %d rin %d rc %d | "
            "V1 %.3f  V2 %.3f" % (name, c["outer_entries"], c["inner_entries"], c["max_d2_over_rl2"], c["max_d2x1_over_rin2"],
                                  c["band_rl"], c["band_rin"], c["band_rc"],
                                  c["disp0"] / c["limit0"] if c.get("limit0") else 0.0,
                                  c["disp1"] / c["limit1"] if c.get("limit1") else 0.0))
