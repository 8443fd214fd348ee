"""numpy restatement of md_scale_cell and of the stochastic cell rescaling step, for tests/test_barostat.py and
tests/test_gpu_barostat.py.  Nothing here touches the device.

Arithmetic.  md_scale_cell multiplies every entry of the cell, every stored coordinate, x0 and x1 by mu and every velocity
component by vscale: one product, one rounding -- numpy's `mu * a` does exactly that, so the stored frame can be compared
bit for bit.  What md_download returns is that frame through the lazy wrap of the NEW cell (cell_reference.export_wrap).

A cell is a d x d array with the lattice vectors in its COLUMNS.  `variant` arguments are deliberate mistakes, for the
tests that show the checks would catch them."""
import numpy as np

from tests import cell_reference as cr

EPS = cr.EPS


def scale_frame(x, v, U, mu, vscale):
    """(x, v, U) after md_scale_cell on the STORED frame: images are untouched and nothing is wrapped."""
    mu, vscale = np.float64(mu), np.float64(vscale)
    return mu * np.asarray(x, dtype=np.float64), vscale * np.asarray(v, dtype=np.float64), mu * np.asarray(U, dtype=np.float64)


def scaled_bound(U_new, x_new, img):
    """Per coordinate: how far x + U img after md_scale_cell(mu) may lie from x + U img after
    md_set_cell(mu U, MD_CELL_AFFINE) on the same frame.

    Both stand for mu (x + U img) of the old frame in the same new cell mu U (formed by the same products).  The scale
    rounds mu x once: eps / 2 of |x_new|.  The affine remap goes through fractional coordinates and back:
    cell_reference.unwrapped_bound for one remap, 8 eps max |U| (1 + max |img|), which also covers the image term (the
    cell is the same array on both sides, so U img differs only by where the wrap put whole lattice vectors -- exact in
    the comparison's longdouble up to the products' roundings counted there)."""
    return cr.unwrapped_bound([U_new], [img]) + 0.5 * EPS * float(np.abs(x_new).max())


def crescale_factor_ld(p_int, volume, ktemp, pressure, compressibility, tau_p, dt_p, xi, dim):
    """barostat.crescale_factor in numpy.longdouble."""
    ld = np.longdouble
    p_int, volume, ktemp, pressure, beta, tau_p, dt_p, xi = (ld(a) for a in (p_int, volume, ktemp, pressure, compressibility,
                                                                             tau_p, dt_p, xi))
    deps = -(beta / tau_p) * (pressure - p_int) * dt_p + np.sqrt(ld(2) * ktemp * beta * dt_p / (volume * tau_p)) * xi
    return np.exp(deps / ld(dim))


def ulps(a, ref):
    """|a - ref| in units of the spacing of the double nearest to ref."""
    return float(abs(np.longdouble(a) - np.longdouble(ref)) / np.longdouble(np.spacing(np.float64(ref))))


def scalar_model(n, ktemp, pressure, k, nsteps, rng, v_form=0.0):
    """The barostat on P_int = n kT / V: nsteps updates of eps = ln V with k = beta_T dt_p / tau_p, V starting at the
    target's mean.  Returns V after every update.  The stationary density of the eps-form is Gamma(n + 1, kT / P0) in V:
    mean (n + 1) kT / P0.  v_form = +-1 adds the V-form's kT / V term with that sign to the drift of eps, where it does
    not belong: the mean moves to (n + 1 + v_form) kT / P0."""
    xi = rng.standard_normal(nsteps)
    out = np.empty(nsteps)
    v = (n + 1.0) * ktemp / pressure
    for t in range(nsteps):
        p_int = n * ktemp / v
        deps = -k * (pressure - p_int - v_form * ktemp / v) + np.sqrt(2.0 * ktemp * k / v) * xi[t]
        v *= np.exp(deps)
        out[t] = v
    return out


def block_mean_and_error(a, nblocks):
    m = len(a) // nblocks
    b = a[:m * nblocks].reshape(nblocks, m).mean(axis=1)
    return float(b.mean()), float(b.std(ddof=1) / np.sqrt(nblocks))


# ---------------------------------------------------------------------------------------------------------------------
# the rows under a scale: what md_scale_cell does to a snapshot of tests/row_audit.py
# ---------------------------------------------------------------------------------------------------------------------
def effective(rc, skin, inner_skin, m0, m1):
    """(rl_eff, skin_eff, inner_eff): rows complete to rc + skin (rc + inner_skin) before scales of m0 (m1) in total are
    complete to m0 (rc + skin) (m1 (rc + inner_skin)) after; the cutoff does not scale."""
    rl = m0 * (rc + skin)
    return rl, rl - rc, m1 * (rc + inner_skin) - rc


def scale_snapshot(snap, U, mu, variant=None):
    """(snapshot, cell) after md_scale_cell(mu) on a snapshot whose rows were never scaled before: positions, x0 and x1 times
    mu, the entries as they are, info reporting the effective radius and skins and d1 times mu, rounded up.
    variants: "x0_unscaled", "x1_unscaled", "old_radius" (rl and skin reported as before), "d1_unscaled",
    "inner_limit_kept" (the inner skin reported as before)."""
    mu = np.float64(mu)
    info = dict(snap["info"])
    rc = float(info["rc"])
    rl, skin, inner = effective(rc, float(info["skin"]), float(info["inner_skin"]), mu, mu)
    out = dict(snap, info=info, pos=mu * snap["pos"], x0=snap["x0"] if variant == "x0_unscaled" else mu * snap["x0"],
               x1=snap["x1"] if variant == "x1_unscaled" else mu * snap["x1"])
    if variant != "old_radius":
        info.update(rl=rl, skin=skin)
    if info["inner_valid"]:
        if variant != "inner_limit_kept":
            info["inner_skin"] = inner
        if variant != "d1_unscaled":
            info["d1"] = float(mu * np.float64(info["d1"])) * (1.0 + 2.0 ** -50)
    return out, mu * np.asarray(U, dtype=np.float64)
