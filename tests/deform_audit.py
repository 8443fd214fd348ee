"""The row audit for rows that md_deform_cell has mapped: tests/row_audit.check_rows on the figures the handle reports, with
the two tightness invariants checked in the metric the rows were made in.

After maps with product M0 since the build, the rows are complete about the mapped x0 to s0 rl (s0 <= sigma_min(M0)), which
is what md_list_rows reports as rl: O1, O2, O3, I1-I3 and V1-V3 hold with the reported figures as they are.  Tightness does
not: an entry made at distance r <= rl lies at up to sigma_max(M0) r in the mapped frame, beyond the reported s0 rl.  (For
M0 = mu 1 the two coincide, which is why md_scale_cell's rows pass check_rows unchanged.)  So O4 and I4 violations, and only
those, are set aside and checked again where they were promised: entry vectors at x0 pulled back by M0^-1 against
row_audit.tightness_bound with the CONFIGURED rl, entry vectors at x1 pulled back by M1^-1 against rin^2 (1 + BAND) with the
configured inner skin.

Rounding of the pull-back.  The stored x0 is k rounded maps of the build's x0, each row-times-vector with d products and
d - 1 sums; the reported M0 is a rounded product of the k maps; the inverse and the pull-back product round again.  Each
contributes at most (d + 1) eps kappa X per coordinate, kappa = ||M^-1||_inf ||M||_inf and X the largest coordinate
involved (positions plus one lattice translation); a difference of two pulled-back coordinates twice that.  With k <= 8:
    delta = 2 (8 + 2) (d + 1) eps kappa X per component,   sqrt(d) delta on a distance,
and the bounds are widened to (sqrt(bound) + sqrt(d) delta)^2 -- by nothing else."""
import numpy as np

from tests import row_audit as ra

MAX_MAPS = 8


def pullback_slack(M, x, U):
    """sqrt(d) delta of the module docstring."""
    M = np.asarray(M, dtype=np.float64)
    d = M.shape[0]
    kappa = float(np.abs(np.linalg.inv(M)).sum(axis=1).max() * np.abs(M).sum(axis=1).max())
    X = float(np.abs(x).max() + np.abs(U).sum(axis=1).max())
    return float(np.sqrt(d) * 2.0 * (MAX_MAPS + 2) * (d + 1) * ra.EPS * kappa * X)


def _pulled_d2(x, ent, U, M):
    Mi = np.linalg.inv(np.asarray(M, dtype=np.float64))
    return ra.entry_d2(np.asarray(x, dtype=np.float64) @ Mi.T, ent, Mi @ U), Mi @ U


def _usable(ent, n):
    ent = np.asarray(ent, dtype=np.int32).reshape(-1, 5)
    ok = (ent[:, :2] >= 0).all(axis=1) & (ent[:, :2] < n).all(axis=1) & (np.abs(ent[:, 2:]) <= 1).all(axis=1)
    return ent[ok]


def check_deformed_rows(snapshot, cell, dim, M0, M1, rl, inner_skin, cache=None):
    """check_rows for a snapshot whose rows were mapped by M0 since the build and M1 since the last prune (d x d; identity
    when nothing was mapped).  rl, inner_skin: the CONFIGURED list radius and inner skin the rows were made with.
    Returns dict(violations, counts, set_aside): set_aside the number of O4 / I4 reports that were checked again."""
    res = ra.check_rows(snapshot, cell, dim, cache=cache)
    keep = [v for v in res["violations"] if v.check not in ("O4", "I4")]
    aside = [v for v in res["violations"] if v.check in ("O4", "I4")]
    info = snapshot["info"]
    n = int(info["n"])
    U = ra.lattice(cell, dim)
    if any(v.check == "O4" for v in aside):
        ent = _usable(snapshot["outer"], n)
        d2, Ub = _pulled_d2(snapshot["x0"], ent, U, M0)
        bound = ra.tightness_bound(dict(info, rl=float(rl)), Ub)
        bound = (np.sqrt(bound) + pullback_slack(M0, snapshot["x0"], U)) ** 2
        wide = d2 > bound
        res["counts"]["max_d2_over_rl2_pulled"] = float(d2.max() / (rl * rl))
        if wide.any():
            keep.append(ra.RowViolation("O4", "%d outer entries beyond the build's radius in the build's own metric: d2 / rl^2 "
                                              "up to %.9f > %.9f, first %s"
                                        % (np.count_nonzero(wide), d2.max() / (rl * rl), bound / (rl * rl), ent[wide][0].tolist())))
    if any(v.check == "I4" for v in aside):
        ent = _usable(snapshot["inner"], n)
        d2, _ = _pulled_d2(snapshot["x1"], ent, U, M1)
        rin = float(info["rc"]) + float(inner_skin)
        bound = (np.sqrt(rin * rin * (1.0 + ra.BAND)) + pullback_slack(M1, snapshot["x1"], U)) ** 2
        far = d2 > bound
        res["counts"]["max_d2x1_over_rin2_pulled"] = float(d2.max() / (rin * rin))
        if far.any():
            keep.append(ra.RowViolation("I4", "%d inner entries beyond rin at x1 in the prune's own metric: d2 / rin^2 up to "
                                              "%.12f, first %s" % (np.count_nonzero(far), d2.max() / (rin * rin), ent[far][0].tolist())))
    return dict(violations=keep, counts=res["counts"], set_aside=len(aside))
