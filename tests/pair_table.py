"""The pair-table audit: the pair potentials checked pair by pair, over their parameters and at their
branch edges.  Takes nothing from the code under test.  A table is a set of ISOLATED DIMERS -- every particle has exactly
one neighbour -- so a particle's force, its Hessian block and its share of U, W and the virial tensor are one pair's
u, f = -dU/dr, t = -f/r, k = U'' and nothing else, and each can be compared with the same formula evaluated in
numpy.longdouble from the uploaded coordinates.

The scale.  u, f and k pass through zero, so an error relative to |q| means nothing near the crossings; an error relative
to max |F| of a frame hides the tail behind the core.  Every quantity is measured against S_q = the sum of the absolute
values of the terms of its written-out formula (hess_reference.pair_full: LJ u -> 4|eps|(s12 + s6), ...): the size of
what fp64 arithmetic actually adds up.  floor(table) is the reference against itself, fp64 through an fp64 d2 as the
oracle goes, against long double; the bounds are B_q = M * floor_q with M = 10, plus, for the r^-2 Lennard-Jones forms, the
documented error of the one-step reciprocal times the power it is raised to (7 for f, 6 for u).

Everything here works on plain arrays (forces, sums, blocks, swap records), so the same checkers take an MDDevice's output
(tests/test_gpu_pair_table.py) and a numpy model's (tests/test_pair_table.py, with its sabotages)."""
import numpy as np

from tests import hess_reference as hr
from tests.util import cutoff_dimers, sqrt_ge_threshold

POT_LJ, POT_PSEUDOHS, POT_POLYDISPERSE, POT_LJ_MODIFIED = hr.POT_LJ, hr.POT_PSEUDOHS, hr.POT_POLYDISPERSE, hr.POT_LJ_MODIFIED
LD = np.longdouble
EPS = 2.0 ** -53
M = 10.0                 # margin over the floor: the Hessian and elasticity tests' (test_gpu_hessian, test_gpu_elasticity)
RCP1 = 2e-15             # md_rcp1's documented relative error (md_kernels.hpp)
MAX_FLOOR = 64 * EPS

# --------------------------------------------------------------------------------------------------------------------
# the cases: name -> (kind, params, list cutoff)
# --------------------------------------------------------------------------------------------------------------------
CASES = {
    "lj": (POT_LJ, [1.0, 1.0, 2.5], 2.5),
    "lj_eps": (POT_LJ, [0.37, 1.0, 2.2], 2.5),
    "lj_wca": (POT_LJ, [2.75, 1.0, 2.0 ** (1.0 / 6.0)], 1.5),
    "lj_sigma": (POT_LJ, [1.0, 1.3, 2.5], 2.5),              # the struct's sigma is ignored, as the oracle ignores it
    "lj_list": (POT_LJ, [1.0, 1.0, 3.0], 2.5),               # the list cutoff ends the range, not r_cut
    "phs50": (POT_PSEUDOHS, [50.0], 1.5),
    "phs49_5": (POT_PSEUDOHS, [49.5], 1.5),
    "phs24": (POT_PSEUDOHS, [24.0], 1.5),
    "phs12": (POT_PSEUDOHS, [12.0], 1.5),
    "poly": (POT_POLYDISPERSE, [1.25, 0.2], 2.1),            # list cutoff >= rcut * the largest sigma_eff (1.62)
    "poly_eta0": (POT_POLYDISPERSE, [1.25, 0.0], 2.1),
    "poly_14": (POT_POLYDISPERSE, [1.4, 0.1], 2.3),
    "poly_20": (POT_POLYDISPERSE, [2.0, 0.35], 3.3),
    "ljmod0": (POT_LJ_MODIFIED, [0.6, 1.1, 2.3, 0.0, 1.7], 2.5),
    "ljmod1": (POT_LJ_MODIFIED, [0.6, 1.1, 2.3, 1.0, 1.7], 2.5),
    "ljmod2": (POT_LJ_MODIFIED, [0.6, 1.1, 2.3, 2.0, 1.7], 2.5),
    "ljmod0_def": (POT_LJ_MODIFIED, [1.0, 1.0, 2.5, 0.0, 2.0], 2.5),
    "ljmod1_def": (POT_LJ_MODIFIED, [1.0, 1.0, 2.5, 1.0, 2.0], 2.5),
    "ljmod2_def": (POT_LJ_MODIFIED, [1.0, 1.0, 2.5, 2.0, 2.0], 2.5),
}
PLUGIN_PARAMS = [0.37, 2.2]                                  # USER_LJ_SRC (eps, r_cut): against the table of "lj_eps"
VARIANTS = ("ones", "uniform", "ulp", "mixed")
BANDS = (("core", 0.55, 0.95), ("zero", 0.95, 1.08), ("well", 1.08, 1.4), ("mid", 1.4, None), ("tail", None, None))
PHS_BANDS = (("core", 0.7, 0.98), ("edge", 0.98, None))
EDGE_IN = 1.0 - 1e-6     # a band's last separation, as a fraction of the branch edge (the edge itself: threshold_table)


def mixed_range(kind):
    return {POT_POLYDISPERSE: (0.73, 1.62), POT_PSEUDOHS: (0.9, 1.0)}.get(kind, (0.7, 1.4))


def sigma_pair(kind, params, si, sj):
    """The length a pair's separation scales with: (si + sj)/2, Polydisperse: sigma_eff."""
    s = 0.5 * (si + sj)
    return s * (1.0 - params[1] * np.abs(si - sj)) if kind == POT_POLYDISPERSE else s


def branch_edge(kind, params, cutoff, sig):
    """Where the pair stops contributing: the potential's own branch, or the list cutoff if that comes first."""
    if kind == POT_POLYDISPERSE:
        own = params[0] * sig
    else:
        own = hr.PHS_B if kind == POT_PSEUDOHS else params[2]
    return np.minimum(own, cutoff)


def pull_distance(cutoff):
    """The separation of a dimer that has been pulled apart: beyond the list cutoff (its pair is exactly zero)."""
    return 1.05 * cutoff + 0.2


def make_table(case, variant, dim=3, seed=5, per_band=48):
    """The dimer table of a case: dict(case, kind, params, cutoff, n, dim, box, x, diam, pairs int[nd, 2] (ids i < j is NOT
    implied), band int[nd], band_names, v, f, img).  Dimer k's separation is r = sigma_ij * rho with rho uniform in band
    k % nbands, clipped per dimer to its branch edge (a band whose range lies beyond the potential's for the nominal
    diameter is dropped); random orientation; ids permuted; no dimer crosses a face, pulled apart or not."""
    kind, params, cutoff = CASES[case]
    rng = np.random.default_rng([seed, dim, VARIANTS.index(variant), sorted(CASES).index(case)])
    lo, hi = mixed_range(kind)
    nominal = {"ones": 1.0, "uniform": 1.17, "ulp": 1.17}.get(variant, 0.5 * (lo + hi))
    sig_nom = float(sigma_pair(kind, params, nominal, nominal))
    edge_nom = float(branch_edge(kind, params, cutoff, sig_nom)) / sig_nom * EDGE_IN
    bands = []
    for name, a, b in (PHS_BANDS if kind == POT_PSEUDOHS else BANDS):
        a = 0.8 * edge_nom if a is None else a
        b = (0.8 * edge_nom if name == "mid" else edge_nom) if b is None else min(b, edge_nom)
        if a < b * (1.0 - 1e-3):
            bands.append((name, a, b))
    nb = len(bands)
    per = max(per_band, -(-141 // nb))                 # more than one 256-particle tile
    nd = per * nb
    while (2 * nd) % 64 == 0 or (2 * nd) % 256 < 8:    # not whole waves, a ragged last tile
        nd += 1
    n = 2 * nd
    assert 256 < n <= 800
    band = np.arange(nd) % nb
    if variant == "mixed":
        diam = rng.uniform(lo, hi, n)
    else:
        diam = np.full(n, nominal)
    perm = rng.permutation(n)
    pairs = np.stack([perm[0::2], perm[1::2]], axis=1)
    if variant == "ulp":
        diam[pairs[nd // 2, 1]] = np.nextafter(1.17, 2.0)
    si, sj = diam[pairs[:, 0]], diam[pairs[:, 1]]
    sig = sigma_pair(kind, params, si, sj)
    edge = branch_edge(kind, params, cutoff, sig) / sig * EDGE_IN
    b_hi = np.minimum(np.array([bands[b][2] for b in band]), edge)
    b_lo = np.minimum(np.array([bands[b][1] for b in band]), 0.9 * b_hi)
    r = sig * (b_lo + (b_hi - b_lo) * rng.uniform(0.0, 1.0, nd))
    pull = pull_distance(cutoff)
    spacing = 3.0 * pull + 1.0                         # no two dimers within the list cutoff, pulled apart or not
    side = int(np.ceil(nd ** (1.0 / dim)))
    sites = np.stack(np.meshgrid(*[np.arange(side)] * dim, indexing="ij"), -1).reshape(-1, dim)[rng.permutation(side ** dim)[:nd]]
    a = (sites + 0.5) * spacing + rng.uniform(-0.25, 0.25, (nd, dim))
    nrm = rng.normal(size=(nd, dim))
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    x = np.zeros((n, dim))
    x[pairs[:, 0]] = a
    x[pairs[:, 1]] = a + r[:, None] * nrm
    return dict(case=case, variant=variant, kind=kind, params=list(params), cutoff=cutoff, n=n, dim=dim,
                box=np.full(dim, side * spacing), x=np.ascontiguousarray(x), diam=diam, pairs=pairs, band=band,
                band_names=[b[0] for b in bands], v=np.zeros((n, dim)), f=np.zeros((n, dim)),
                img=np.zeros((n, dim), dtype=np.int32))


def pulled(table, band):
    """The table's positions with every dimer NOT in `band` pulled apart beyond the list cutoff (along its own axis)."""
    x = table["x"].copy()
    i, j = table["pairs"][table["band"] != band].T
    d = x[j] - x[i]
    x[j] = x[i] + d / np.linalg.norm(d, axis=1)[:, None] * pull_distance(table["cutoff"])
    return np.ascontiguousarray(x)


def table_conditions(table):
    n, nd = table["n"], len(table["pairs"])
    cnt = np.bincount(table["band"], minlength=len(table["band_names"]))
    assert n % 64 != 0 and 256 < n <= 800 and n % 256 != 0, n
    assert cnt.min() >= 48, cnt
    assert sorted(table["pairs"].ravel().tolist()) == list(range(n)) and 2 * nd == n
    assert not np.array_equal(table["pairs"].ravel(), np.arange(n))         # ids are permuted


# --------------------------------------------------------------------------------------------------------------------
# the reference
# --------------------------------------------------------------------------------------------------------------------
def d2_oracle(dl):
    """The oracle's squared distance: every product and sum rounded, left to right."""
    d2 = dl[:, 0] * dl[:, 0] + dl[:, 1] * dl[:, 1]
    return d2 + dl[:, 2] * dl[:, 2] if dl.shape[1] == 3 else d2


def pair_terms(kind, params, r, si, sj, dtype=LD):
    """dict(u, f, t, k, inside, Su, Sf, Sk) of hess_reference.pair_full (the formulas live there), unmasked."""
    q = hr.pair_full(kind, params, r, si, sj, dtype)
    q["t"] = -q["f"] / np.asarray(r, dtype=dtype)
    return q


def reference(table, x=None, diam=None, dtype=LD):
    """The table's pairs in `dtype`: long double takes r from the uploaded coordinates (del = x_j - x_i, r = sqrt(sum del^2),
    all in long double); float64 goes through the oracle's fp64 d2.  The DECISIONS are the oracle's in both: the pair is
    listed iff d2 <= cutoff^2 and contributes iff the potential's own branch accepts sqrt(d2), both in fp64.  Returns
    dict(i, j, del, r, nhat, live, u, f, t, k, Su, Sf, Sk), masked quantities zero where not live."""
    kind, params = table["kind"], table["params"]
    x = table["x"] if x is None else x
    diam = table["diam"] if diam is None else diam
    i, j = table["pairs"].T
    dl64 = x[j] - x[i]
    d2 = d2_oracle(dl64)
    if dtype is np.float64:
        dl, r = dl64, np.sqrt(d2)
    else:
        dl = x[j].astype(LD) - x[i].astype(LD)
        r = np.sqrt((dl * dl).sum(axis=1))
    q = pair_terms(kind, params, r, diam[i].astype(dtype), diam[j].astype(dtype), dtype)
    live = (d2 <= table["cutoff"] * table["cutoff"]) & hr.pair_full(kind, params, np.sqrt(d2), diam[i], diam[j])["inside"]
    out = dict(i=i, j=j, r=r, nhat=dl / r[:, None], live=live)
    out["del"] = dl
    for key in ("u", "f", "t", "k", "Su", "Sf", "Sk"):
        out[key] = np.where(live, q[key], dtype(0))
    return out


def floor(table, x=None, quantities=("u", "f", "k", "blk")):
    """dict(u, f, k, blk): max over the live pairs of |q64 - q80| / S_q -- the reference against itself; blk: the Hessian
    block (k - t) n n^T + t I, element by element, against S_k + S_f / r.  A threshold table holds one separation only, too
    narrow a sample of the rounding: its floor is taken together with that of the full table of table["floor_case"]."""
    a, b = reference(table, x, dtype=np.float64), reference(table, x)
    m = b["live"]
    out = {}
    for q in ("u", "f", "k"):
        if q in quantities:
            out[q] = float((np.abs(a[q].astype(LD) - b[q])[m] / b["S" + q][m]).max())
    if "blk" in quantities:
        B64, B80 = _blocks(a), _blocks(b)
        out["blk"] = float((np.abs(B64.astype(LD) - B80).max(axis=(1, 2))[m] / (b["Sk"] + b["Sf"] / b["r"])[m]).max())
    if "floor_case" in table:
        other = floor(make_table(*table["floor_case"]), quantities=quantities)
        out = {q: max(v, other[q]) for q, v in out.items()}
    return out


def bounds(table, r2_form, x=None, quantities=("u", "f", "k", "blk")):
    """B_u, B_f, B_k, B_blk = M * floor; the r^-2 Lennard-Jones forms (pair_eval<POT_LJ>, the ljA / ljB kernel) add the
    one-step reciprocal's documented error times the power of the reciprocal in the leading term."""
    fl = floor(table, x, quantities)
    for q, v in fl.items():
        assert v <= MAX_FLOOR, (table["case"], q, v / EPS)
    B = {q: M * v for q, v in fl.items()}
    if r2_form:
        assert table["kind"] == POT_LJ
        B["f"] += 7 * RCP1
        B["u"] += 6 * RCP1
    return B


def _blocks(ref):
    d = ref["nhat"].shape[1]
    T = ref["nhat"].dtype.type
    nn = ref["nhat"][:, :, None] * ref["nhat"][:, None, :]
    return (ref["k"] - ref["t"])[:, None, None] * nn + ref["t"][:, None, None] * np.eye(d, dtype=T)[None]


# --------------------------------------------------------------------------------------------------------------------
# the checkers.  Each returns the largest measured error / S in units of 2^-53 (a record) and raises AssertionError with
# the worst pair when a bound is missed.
# --------------------------------------------------------------------------------------------------------------------
def _worst(err, scale, bound, ref, what):
    ratio = np.where(scale > 0, err / np.where(scale > 0, scale, 1), np.where(err > 0, np.inf, 0.0)).astype(np.float64)
    w = int(np.argmax(ratio))
    assert ratio[w] <= bound, "%s: pair %d (ids %d, %d, r = %.6f): error / S = %.3g x 2^-53, bound %.3g x 2^-53" % (
        what, w, ref["i"][w], ref["j"][w], float(ref["r"][w]), ratio[w] / EPS, bound / EPS)
    return float(ratio[w] / EPS)


def check_pair_forces(table, f, B, x=None, symmetric=True, what="forces"):
    """Per particle the force vector against f80 * nhat (particle i: -f nhat, particle j: +f nhat), every component within
    B_f * S_f; exact zero where the oracle's decision gives none; F_i == -F_j bit for bit."""
    ref = reference(table, x)
    i, j = ref["i"], ref["j"]
    want = ref["f"][:, None] * ref["nhat"]
    err = np.maximum(np.abs(f[j].astype(LD) - want).max(axis=1), np.abs(f[i].astype(LD) + want).max(axis=1))
    dead = ~ref["live"]
    assert np.all(f[i][dead] == 0.0) and np.all(f[j][dead] == 0.0), what + ": a force on a pair the oracle leaves out"
    if symmetric:
        assert np.array_equal(f[i], -f[j]), what + ": F_i != -F_j"
    return _worst(err[~dead], ref["Sf"][~dead], B["f"], {k: ref[k][~dead] for k in ("i", "j", "r")}, what)


def band_sums(table, band, x=None):
    """(U, W, virial tensor, S_U, S_W, count) of one band in long double; tensor in the order xx, yy, zz, xy, xz, yz (3-D) or
    xx, yy, xy (2-D): W_ab = sum (f / r) del_a del_b."""
    ref = reference(table, x)
    m = ref["live"] & (table["band"] == band)
    comp = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)) if table["dim"] == 3 else ((0, 0), (1, 1), (0, 1))
    fr = (ref["f"] * ref["r"])[m]
    vir = np.array([(fr * ref["nhat"][m, a] * ref["nhat"][m, b]).sum() for a, b in comp])
    return ref["u"][m].sum(), fr.sum(), vir, ref["Su"][m].sum(), (ref["Sf"] * ref["r"])[m].sum(), int(m.sum())


def check_band_sums(table, band, B, U=None, W=None, vir=None, x=None, what="band sums"):
    """U, W and the virial tensor of one band (x = pulled(table, band)): |sum - sum80| <= (B_q + n 2^-53) * sum S_q."""
    u80, w80, v80, SU, SW, cnt = band_sums(table, band, x)
    out = {}
    for name, got, want, S, Bq in (("U", U, u80, SU, B["u"]), ("W", W, w80, SW, B["f"]), ("vir", vir, v80, SW, B["f"])):
        if got is None:
            continue
        err = float(np.abs(np.asarray(got, dtype=LD) - want).max())
        bound = (Bq + cnt * EPS) * float(S)
        assert err <= bound, "%s: %s of band %s: error %.3g, bound %.3g (%.3g x 2^-53 of sum S)" % (
            what, name, table["band_names"][band], err, bound, err / float(S) / EPS)
        out[name] = err / float(S) / EPS
    return out


def check_blocks(table, H, B, x=None, what="blocks"):
    """md_hess_blocks of a dimer's two particles is exactly (k - t) n n^T + t I: every element within B_blk * (S_k + S_f / r),
    and k = n^T H n, t = e^T H e (e normal to n) recovered from the block within the same."""
    ref = reference(table, x)
    want = _blocks(ref)
    i, j, m = ref["i"], ref["j"], ref["live"]
    assert np.all(H[i][~m] == 0.0) and np.all(H[j][~m] == 0.0), what + ": a block on a pair the oracle leaves out"
    S = ref["Sk"] + ref["Sf"] / ref["r"]
    err = np.maximum(np.abs(H[i].astype(LD) - want).max(axis=(1, 2)), np.abs(H[j].astype(LD) - want).max(axis=(1, 2)))
    n = ref["nhat"]
    e = np.zeros_like(n)                               # a unit vector normal to n
    e[:, 0], e[:, 1] = -n[:, 1], n[:, 0]
    e /= np.sqrt((e * e).sum(axis=1))[:, None]
    for Hp in (H[i].astype(LD), H[j].astype(LD)):
        kd = np.einsum("pa,pab,pb->p", n, Hp, n)
        td = np.einsum("pa,pab,pb->p", e, Hp, e)
        err = np.maximum(err, np.maximum(np.abs(kd - ref["k"]), np.abs(td - ref["t"])))
    sub = {k: ref[k][m] for k in ("i", "j", "r")}
    return _worst(err[m], S[m], B["blk"], sub, what)


def swap_reference_du(table, a, b, diam):
    """(dU, S) of exchanging the diameters of particles a and b (one neighbour each, the dimer mate): the four pair energies
    in long double, S = the sum of their S_u."""
    mate = np.empty(table["n"], dtype=np.int64)
    mate[table["pairs"][:, 0]], mate[table["pairs"][:, 1]] = table["pairs"][:, 1], table["pairs"][:, 0]
    x = table["x"]
    du, S = LD(0), LD(0)
    for p, q in ((a, b), (b, a)):
        k = int(mate[p])
        if k == q:
            continue
        dl64 = (x[k] - x[p])[None]
        d2 = d2_oracle(dl64)
        dl = x[k].astype(LD) - x[p].astype(LD)
        r = np.sqrt((dl * dl).sum())
        for dp, sign in ((diam[q], 1), (diam[p], -1)):
            t = pair_terms(table["kind"], table["params"], r, LD(dp), LD(diam[k]))
            live = (d2[0] <= table["cutoff"] ** 2) and bool(hr.pair_full(table["kind"], table["params"], np.sqrt(d2), dp, diam[k])["inside"][0])
            if live:
                du += sign * t["u"]
                S += t["Su"]
    return du, S


def check_swap(table, partner, status, du, diam, w3, ktemp, Bu, what="swap"):
    """Every decided swap of a round (status 5 rejected, 6 accepted; `diam` = the diameters BEFORE the round; w3[i] = the
    fourth Philox word of particle i): dU within B_u * S of the four long-double pair energies; the decision equal to
    (w3 + 0.5) / 2^32 < exp(-dU / kT) wherever the reference dU is farther from the decision point than its bound.
    Returns dict(decided, close, worst)."""
    decided = np.flatnonzero(status >= 5)
    close, worst = 0, 0.0
    for i in decided:
        j = int(partner[i])
        d80, S = swap_reference_du(table, int(i), j, diam)
        err = abs(LD(du[i]) - d80)
        bound = Bu * S
        assert err <= bound, "%s: dU of (%d, %d): %.17g against %.17g, error / S = %.3g x 2^-53, bound %.3g" % (
            what, i, j, du[i], float(d80), float(err / S) / EPS, Bu / EPS)
        if S > 0:
            worst = max(worst, float(err / S) / EPS)
        u3 = (LD(int(w3[i])) + LD(0.5)) / LD(2.0 ** 32)
        point = -LD(ktemp) * np.log(u3)                  # accept iff dU < point
        if abs(d80 - point) <= bound:
            close += 1
            continue
        assert (status[i] == 6) == bool(d80 < point), "%s: decision of (%d, %d): dU %.17g, decision point %.17g, status %d" % (
            what, i, j, float(d80), float(point), status[i])
    return dict(decided=len(decided), close=close, worst=worst)


def swap_conditions(res):
    assert res["decided"] >= 20 and res["close"] <= 0.05 * res["decided"], res


# --------------------------------------------------------------------------------------------------------------------
# threshold dimers: squared separations ON a branch's d2 threshold, one ulp either side, and between the reference-form
# and the fma-chain value (tests/util.py cutoff_dimers)
# --------------------------------------------------------------------------------------------------------------------
THRESHOLDS = {
    # name -> (kind, params, list cutoff, branch radius, diameter pair, the full table whose floor joins this one's)
    "lj_2.2": (POT_LJ, [0.37, 1.0, 2.2], 2.5, 2.2, (1.0, 1.0), ("lj_eps", "ones")),
    "lj_wca": (POT_LJ, [2.75, 1.0, 2.0 ** (1.0 / 6.0)], 1.5, 2.0 ** (1.0 / 6.0), (1.0, 1.0), ("lj_wca", "ones")),
    "lj_0.9": (POT_LJ, [1.0, 1.0, 0.9], 1.5, 0.9, (1.0, 1.0), ("lj", "ones")),
    "phs": (POT_PSEUDOHS, [50.0], 1.5, hr.PHS_B, (1.0, 1.0), ("phs50", "ones")),
    "poly": (POT_POLYDISPERSE, [1.25, 0.2], 1.5, None, (0.9, 1.3), ("poly", "mixed")),   # radius fl(rcut * sigma_eff) = 1.265
    "ljmod_rcut": (POT_LJ_MODIFIED, [0.6, 1.1, 2.3, 2.0, 1.7], 2.5, 2.3, (1.0, 1.0), ("ljmod2", "ones")),
    "ljmod_ron": (POT_LJ_MODIFIED, [0.6, 1.1, 2.3, 2.0, 1.7], 2.5, 1.7, (1.0, 1.0), ("ljmod2", "ones")),
}


def threshold_table(name):
    """cutoff_dimers (125 dimers) steered about the predecessor of the smallest double whose sqrt reaches the branch radius,
    as a table (one band).  The conditions: every category holds >= 15 dimers and at most 4 are unreached."""
    kind, params, cutoff, radius, (da, db), floor_case = THRESHOLDS[name]
    if radius is None:
        se = 0.5 * (da + db)
        se *= (1.0 - params[1] * abs(da - db))
        radius = params[0] * se
    target = float(np.nextafter(sqrt_ge_threshold(radius), 0.0))
    s = cutoff_dimers(target, n_side=5)
    n = s["n"]
    cat = s["cat"]
    assert (cat == -1).sum() <= 4 and np.bincount(cat[cat >= 0], minlength=6).min() >= 15, np.bincount(cat + 1)
    diam = np.ones(n)
    diam[0::2], diam[1::2] = da, db
    t = dict(s)
    t.update(case=name, variant="threshold", kind=kind, params=list(params), cutoff=cutoff, diam=diam,
             pairs=np.stack([np.arange(0, n, 2), np.arange(1, n, 2)], axis=1), band=np.zeros(n // 2, dtype=np.int64),
             band_names=["threshold"], target=target, radius=radius, floor_case=floor_case)
    return t


def check_decisions(table, oracle, f, pairs=None, what="decisions"):
    """The zero / non-zero force pattern, and the exported pair set when given, equal the oracle's bit for bit."""
    pot = oracle.make_pot(table["kind"], table["params"])
    f_ref, _, _, pairs_ref = oracle.forces_brute(table["x"], table["box"], table["cutoff"], pot, table["diam"], want_pairs=True)
    nz, nz_ref = np.abs(f).max(axis=1) > 0.0, np.abs(f_ref).max(axis=1) > 0.0
    if table["kind"] == POT_POLYDISPERSE and table.get("variant") == "threshold":
        # u, f and U'' all vanish AT this potential's edge: what a dimer on the threshold contributes is the rounding residue
        # of a sum that cancels (|f| ~ 1e-15), exactly zero for some dimers in the oracle's own arithmetic and for others in
        # another's.  The decision shows one way only: beyond the threshold the force is exactly zero.
        live = np.repeat(reference(table)["live"], 2)
        assert np.array_equal(live[table["pairs"].ravel()], live) and not np.any(nz_ref & ~live)
        assert 15 <= live.sum() // 2 <= len(live) // 2 - 15
        bad = np.flatnonzero(nz & ~live)
        assert nz[live].sum() >= 0.8 * live.sum(), what + ": no force where the oracle has one"
        nz_ref = nz
    else:
        bad = np.flatnonzero(nz != nz_ref)
    assert len(bad) == 0, "%s: %d particles decide differently from the oracle, first id %d (category %d)" % (
        what, len(bad), bad[0], table["cat"][bad[0] // 2] if "cat" in table else -2)
    if table.get("variant") == "threshold" and table["case"] != "ljmod_ron":
        assert 15 <= nz_ref.sum() // 2 <= len(nz_ref) // 2 - 15, "the threshold does not split the dimers"
    if pairs is not None:
        assert np.array_equal(pairs, pairs_ref[np.lexsort((pairs_ref[:, 1], pairs_ref[:, 0]))]), what + ": pair set differs"
