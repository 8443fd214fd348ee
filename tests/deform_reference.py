"""numpy restatement of md_deform_cell and of the shear-flow update, for tests/test_shear_flow.py and
tests/test_gpu_shear_flow.py.  Nothing here touches the device.

Arithmetic.  md_deform_cell forms every mapped vector row times vector, left to right, every product and every sum rounded
on its own, no fma: t = (M_r0 a_0 + M_r1 a_1) + M_r2 a_2.  numpy's elementwise products and sums round the same way, so the
stored frame, x0, x1 and the velocities can be compared bit for bit.  The cell F U is formed the same way, column by column.
What md_download returns is the stored frame through the lazy wrap of the NEW cell (cell_reference.export_wrap).

A cell is a d x d array with the lattice vectors in its COLUMNS; F and G act from the left.  `variant` arguments are
deliberate mistakes, for the tests that show the checks would catch them."""
import numpy as np

from tests import cell_reference as cr

EPS = cr.EPS
WIDEN = 2.0 ** -40


def apply(M, a):
    """M a per row of a ([n, d]) in the device's operation order."""
    return cr._matvec(np.asarray(M, dtype=np.float64), np.asarray(a, dtype=np.float64), True)


def cell_after(F, U):
    """F U in the device's arithmetic: the columns of U are vectors like any other."""
    return np.ascontiguousarray(apply(F, np.asarray(U, dtype=np.float64).T).T)


def deform_frame(x, v, U, F, G=None):
    """(x, v, U) after md_deform_cell on the STORED frame: images are untouched and nothing is wrapped."""
    return apply(F, x), (np.array(v, dtype=np.float64) if G is None else apply(G, v)), cell_after(F, U)


def singular_values(M):
    """(sigma_min, sigma_max) from the symmetric eigenproblem of M^T M."""
    M = np.asarray(M, dtype=np.float64)
    w = np.linalg.eigvalsh(M.T @ M)
    return float(np.sqrt(max(w[0], 0.0))), float(np.sqrt(w[-1]))


def singular_bounds(M):
    """(lo, hi): lo <= sigma_min(M), hi >= sigma_max(M), the exact values widened by a relative 2^-40."""
    lo, hi = singular_values(M)
    return lo * (1.0 - WIDEN), hi * (1.0 + WIDEN)


def effective(rc, skin, inner_skin, s0, s1):
    """(rl_eff, skin_eff, inner_eff) of rows built at rc + skin (pruned at rc + inner_skin) after maps whose smallest
    singular values are at least s0 (s1): a pair within rc now is within rc + 2 disp of the mapped reference positions,
    hence within (rc + 2 disp) / s of the reference positions the rows were made at -- so the rows cover the mapped frame
    to s (rc + skin), and the cutoff does not scale."""
    rl = s0 * (rc + skin)
    return rl, rl - rc, s1 * (rc + inner_skin) - rc


def deformed_bound(U_old, U_new, F, x_old, img):
    """Per coordinate: how far x + U img after md_deform_cell(F) may lie from x + U img after
    md_set_cell(F U, MD_CELL_AFFINE) on the same frame, both in the same array U_new = fl(F U).

    The map stores fl(F x): d products and d - 1 sums, each within eps / 2 of a partial sum bounded by sum_c |F_rc| |x_c|,
    so d eps / 2 ||F||_inf max |x| in all.  The affine remap stands for U_new U_old^-1 x + U_new img, and
    U_new U_old^-1 = F + E with |E| <= (d eps / 2) |F| |U_old| |U_old^-1| entrywise (the rounding of F U carried through the
    inverse): another (d eps / 2) ||F||_inf kappa max |x| with kappa = || |U_old| |U_old^-1| ||_inf >= 1.  The remap's own
    roundings through fractional coordinates and the image term are cell_reference.unwrapped_bound for one remap in the new
    cell, as in baro_reference.scaled_bound."""
    d = np.asarray(F).shape[0]
    normF = float(np.abs(F).sum(axis=1).max())
    Uo = np.asarray(U_old, dtype=np.float64)
    kappa = float((np.abs(Uo) @ np.abs(np.linalg.inv(Uo))).sum(axis=1).max())
    xmax = float(np.abs(x_old).max())
    return cr.unwrapped_bound([U_new], [img]) + 0.5 * d * EPS * normF * (1.0 + kappa) * xmax


def ulp_up(a, k=1):
    a = np.float64(a)
    for _ in range(k):
        a = np.nextafter(a, np.inf)
    return float(a)


# ---------------------------------------------------------------------------------------------------------------------
# the rows under a map: what md_deform_cell does to a snapshot of tests/row_audit.py
# ---------------------------------------------------------------------------------------------------------------------
def deform_snapshot(snap, U, F, state=None, variant=None):
    """(snapshot, cell, state) after md_deform_cell(F) on a snapshot.  state = dict(M0, M1, rl, inner_skin): the maps
    since the build / the prune and the CONFIGURED radius and inner skin (None: rows never mapped, taken from the
    snapshot).  info reports the effective radius and skins and d1 times sigma_max(F), rounded up.
    variants: "x0_unmapped", "x1_unmapped", "sigma_max_for_min" (the skins formed with the largest singular value),
    "d1_unscaled", "inner_limit_kept" (the inner skin reported as before), "m1_not_reset" (used by prune_snapshot)."""
    F = np.asarray(F, dtype=np.float64)
    d = F.shape[0]
    info = dict(snap["info"])
    if state is None:
        state = dict(M0=np.eye(d), M1=np.eye(d), rl=float(info["rl"]), inner_skin=float(info["inner_skin"]))
    rc = float(info["rc"])
    M0, M1 = F @ state["M0"], F @ state["M1"]
    pick = (lambda M: singular_bounds(M)[1]) if variant == "sigma_max_for_min" else (lambda M: singular_bounds(M)[0])
    rl, skin, inner = effective(rc, state["rl"] - rc, state["inner_skin"], pick(M0), pick(M1))
    out = dict(snap, info=info, pos=apply(F, snap["pos"]),
               x0=snap["x0"] if variant == "x0_unmapped" else apply(F, snap["x0"]),
               x1=snap["x1"] if variant == "x1_unmapped" else apply(F, snap["x1"]))
    info.update(rl=rl, skin=skin)
    if info["inner_valid"]:
        if variant != "inner_limit_kept":
            info["inner_skin"] = inner
        if variant != "d1_unscaled":
            info["d1"] = float(singular_bounds(F)[1] * np.float64(info["d1"])) * (1.0 + 2.0 ** -50)
    return out, cell_after(F, U), dict(state, M0=M0, M1=M1)


def prune_snapshot(snap, U, state, variant=None):
    """A prune on the model: x1 <- pos, the inner rows are the outer entries within rc + the configured inner skin of the
    new x1, d1 = max |x1 - x0|, and M1 starts again at the identity (variant "m1_not_reset": it does not, so the next
    map's inner skin is formed from a product that includes maps the new inner rows never saw)."""
    from tests import row_audit as ra
    info = dict(snap["info"])
    rin = float(info["rc"]) + state["inner_skin"]
    x1 = snap["pos"].copy()
    outer = np.asarray(snap["outer"]).reshape(-1, 5)
    inner = outer[ra.entry_d2(x1, outer, U) <= rin * rin]
    info.update(inner_valid=1, inner_skin=state["inner_skin"],
                d1=float(np.sqrt(((x1 - snap["x0"]) ** 2).sum(axis=1)).max()) * (1.0 + 4.0 * EPS))
    d = U.shape[0]
    new_state = dict(state) if variant == "m1_not_reset" else dict(state, M1=np.eye(d))
    return dict(snap, info=info, x1=x1, inner=inner), new_state
