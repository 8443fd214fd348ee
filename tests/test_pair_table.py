"""The pair-table audit (tests/pair_table.py) proved on the CPU: its reference against the oracle, its tables against their
conditions, a numpy MODEL of the device's forms through every checker, and the sabotages -- each a plausible mistake in a
host constant or a branch of pair_eval / pair_eval2 that the suite could not see before -- each caught by the checker
named for it.  tests/test_gpu_pair_table.py runs the same checkers on an MDDevice."""
import numpy as np
import pytest

from tests import hess_reference as hr
from tests import pair_table as pt
from tests import swap_reference as sr
from tests.util import lj_system, sqrt_ge_threshold

LD, EPS = pt.LD, pt.EPS
SWAP_SEED, SWAP_KT = 7, 2.0          # chosen here so that the reference alone meets swap_conditions (test_model_swap)
SWAP_CASES = ["lj", "poly", "phs50", "ljmod1"]


# --------------------------------------------------------------------------------------------------------------------
# the model: the device's forms in numpy fp64 (md_kernels.hpp pair_eval, the ljA / ljB kernel, configure_potential), with
# an exact division standing in for the reciprocal.  `sab` switches one deliberate mistake on.
# --------------------------------------------------------------------------------------------------------------------
def _ipow(x, n):
    r = np.ones_like(x)
    while n:
        if n & 1:
            r = r * x
        x = x * x
        n >>= 1
    return r


def model_c2(kind, params, cutoff, sab=None):
    c2 = np.nextafter(cutoff * cutoff, np.inf)
    if kind in (pt.POT_LJ, pt.POT_LJ_MODIFIED):
        c2 = min(c2, params[2] * params[2] if sab == "rc2" else sqrt_ge_threshold(params[2]))
    return c2


def model_eval(kind, params, cutoff, d2, si, sj, uniform, form="r2", sab=None):
    """(u, fpr = f / r, hit) per pair."""
    p = list(params) + [0.0] * 8
    c2 = model_c2(kind, params, cutoff, sab)
    hit = (d2 <= c2) if sab == "le" else (d2 < c2)
    d2m = np.where(hit, d2, 2.0 ** 1000)
    sig_u = float(si[0]) if uniform else None
    if kind == pt.POT_LJ:
        eps = p[0]
        c48, c24, c4 = 48.0 * eps, 24.0 * eps, (4.0 if sab == "c4" else 4.0 * eps)
        inv = 1.0 / d2m
        if sab == "rcp":
            inv = inv * (1.0 + 3e-8)
        if form == "AB":
            assert uniform
            s2 = 1.0 if sab == "ljA_sigma1" else ((sig_u + sig_u) * 0.5) * ((sig_u + sig_u) * 0.5)
            s6 = s2 * s2 * s2
            A, B = c48 * s6 * s6, c24 * s6
            z2 = inv * inv
            fpr = (z2 * z2) * (A * (z2 * inv) - B)
            w3 = s6 * (z2 * inv)
        else:
            sg = (si + sj) * 0.5
            w = (((sig_u + sig_u) * 0.5) * ((sig_u + sig_u) * 0.5) if uniform else sg * sg) * inv
            w3 = (w * w) * w
            fpr = (w3 * inv) * (c48 * w3 - c24)
        u = c4 * (w3 * (w3 - 1.0))
    else:
        r = np.sqrt(d2m)
        sg = np.full_like(r, sig_u) if uniform else (si + sj) / 2.0
        u, fij = np.zeros_like(r), np.zeros_like(r)
        with np.errstate(over="ignore", invalid="ignore", under="ignore"):
            if kind == pt.POT_PSEUDOHS:
                lam = p[0]
                ins = r < (hr.PHS_B * sg if sab == "phs_b_sigma" else hr.PHS_B)
                srr = sg / r
                pl, plm = srr ** lam, srr ** (lam - 1.0)
                u = np.where(ins, hr.PHS_A * (pl - plm) + 1.0, 0.0)
                fij = np.where(ins, (lam * (pl * srr) - (lam - 1.0) * pl) * hr.PHS_A, 0.0)
            elif kind == pt.POT_LJ_MODIFIED:
                eps, sc, rc, mode, ron = p[0], p[1], p[2], int(p[3]), p[4]
                s = (sg if sab == "vcut_pair_sigma" else sc) / rc
                s2 = s * s
                s6 = s2 * s2 * s2
                s12 = s6 * s6
                p5, p6 = 4.0 * eps * (s12 - s6), 24.0 * eps * (2.0 * s12 - s6) / rc
                ins = r < rc
                srr = sg / r
                sr2 = srr * srr
                sr6 = (sr2 * sr2) * sr2
                sr12 = sr6 * sr6
                V = (4.0 * eps) * (sr12 - sr6)
                F = ((24.0 * eps) * (2.0 * sr12 - sr6)) / r
                if mode == 0:
                    uu, ff = V - p5, F
                elif mode == 1:
                    uu = V - p5 - (r - rc) * p6 if sab == "mode1_sign" else V - p5 + (r - rc) * p6
                    ff = F - p6
                else:
                    rc2, r2, ron2 = rc * rc, r * r, ron * ron
                    den = ((rc2 - ron2) * (rc2 - ron2)) * (rc2 - ron2)
                    a, b = rc2 - r2, rc2 + 2.0 * r2 - 3.0 * ron2
                    sw = r >= ron
                    S = np.where(sw, ((a * a) * b) / den, 1.0)
                    dS = np.where(sw, (-12.0 * r * a * (r2 - ron2)) / den, 0.0)
                    if sab == "xplor_ds":
                        dS = -dS
                    uu, ff = V * S, S * F - V * dS
                u, fij = np.where(ins, uu, 0.0), np.where(ins, ff, 0.0)
            else:
                rc, eta = p[0], p[1]
                se = 0.5 * (si + sj)
                se = se * (1.0 - eta * ((si - sj) if sab == "poly_nofabs" else np.abs(si - sj)))
                ins = r < rc * se
                c0, c2_, c4_ = -28.0 / _ipow(rc, 12), 48.0 / _ipow(rc, 14), -21.0 / _ipow(rc, 14 if sab == "poly_c4" else 16)
                q = r / se
                u = np.where(ins, _ipow(se / r, 12) + c0 + c2_ * (q * q) + c4_ * _ipow(q, 4), 0.0)
                fij = np.where(ins, 12.0 * _ipow(se, 12) / _ipow(r, 13) - 2.0 * c2_ * r / (se * se)
                               - 4.0 * c4_ * (r * r * r) / _ipow(se, 4), 0.0)
        fpr = fij / r
    if sab == "tail_1e-9":
        fpr = np.where(np.sqrt(d2) > 2.0 * 0.5 * (si + sj), fpr * (1.0 + 1e-9), fpr)
    return np.where(hit, u, 0.0), np.where(hit, fpr, 0.0), hit


class Model:
    """What the checkers need of a handle, computed from the model: forces(), sums(), blocks(), swap du."""

    def __init__(self, table, form="r2", sab=None):
        self.t, self.form, self.sab = table, form, sab

    def _pairs(self, x, diam=None):
        t = self.t
        x = t["x"] if x is None else x
        diam = t["diam"] if diam is None else diam
        i, j = t["pairs"].T
        dl = x[j] - x[i]
        uniform = bool(np.all(diam == diam[0])) and t["kind"] in (pt.POT_LJ, pt.POT_PSEUDOHS)
        form = self.form if (uniform and t["kind"] == pt.POT_LJ) else "r2"
        u, fpr, hit = model_eval(t["kind"], t["params"], t["cutoff"], pt.d2_oracle(dl), diam[i], diam[j], uniform, form, self.sab)
        return i, j, dl, u, fpr, hit

    def forces(self, x=None):
        i, j, dl, u, fpr, hit = self._pairs(x)
        f = np.zeros_like(self.t["x"])
        f[i] = -fpr[:, None] * dl
        f[j] = fpr[:, None] * dl
        return f

    def sums(self, x=None):
        i, j, dl, u, fpr, hit = self._pairs(x)
        comp = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)) if self.t["dim"] == 3 else ((0, 0), (1, 1), (0, 1))
        return u.sum(), (fpr * pt.d2_oracle(dl)).sum(), np.array([(fpr * dl[:, a] * dl[:, b]).sum() for a, b in comp])

    def blocks(self, x=None):
        t = self.t
        i, j, dl, u, fpr, hit = self._pairs(x)
        d2 = pt.d2_oracle(dl)
        r = np.sqrt(d2)
        tt, kk, ins = hr.pair_tk(t["kind"], t["params"], r, t["diam"][i], t["diam"][j])
        if self.sab == "phs_k_lambda":
            lam = t["params"][0]
            srr = (0.5 * (t["diam"][i] + t["diam"][j])) / r
            kk = np.where(ins, hr.PHS_A * lam * (lam * srr ** (lam + 1.0) - (lam - 1.0) * srr ** lam) / r, 0.0)
        tt, kk = np.where(hit, tt, 0.0), np.where(hit, kk, 0.0)
        B = ((kk - tt) / d2)[:, None, None] * dl[:, :, None] * dl[:, None, :] + tt[:, None, None] * np.eye(t["dim"])[None]
        H = np.zeros((t["n"], t["dim"], t["dim"]))
        H[i], H[j] = B, B
        return H

    def pair_u(self, a, k, da, dk):
        x = self.t["x"]
        dl = (x[k] - x[a])[None]
        return model_eval(self.t["kind"], self.t["params"], self.t["cutoff"], pt.d2_oracle(dl), np.array([da]), np.array([dk]),
                          False, "r2", self.sab)[0][0]


def _all_tables():
    for case in pt.CASES:
        for variant in pt.VARIANTS:
            yield pt.make_table(case, variant)
    for case in ("lj", "poly"):
        yield pt.make_table(case, "uniform" if case == "lj" else "mixed", dim=2)


@pytest.fixture(scope="module")
def tables():
    return {(t["case"], t["variant"], t["dim"]): t for t in _all_tables()}


@pytest.fixture(scope="module")
def thresholds():
    return {name: pt.threshold_table(name) for name in pt.THRESHOLDS}


def _r2(table):
    return table["kind"] == pt.POT_LJ


# --------------------------------------------------------------------------------------------------------------------
def test_tables_meet_their_conditions(tables):
    assert len(tables) == 4 * len(pt.CASES) + 2
    for t in tables.values():
        pt.table_conditions(t)
        ref = pt.reference(t)
        assert ref["live"].all(), (t["case"], t["variant"])            # every dimer of a table interacts ...
        for b in range(len(t["band_names"])):                          # ... and none of another band once pulled apart
            refb = pt.reference(t, pt.pulled(t, b))
            assert np.array_equal(refb["live"], t["band"] == b)
        x = np.concatenate([t["x"]] + [pt.pulled(t, b) for b in range(len(t["band_names"]))])
        assert x.min() > 0.0 and x.max() < t["box"][0]                 # no dimer crosses a face
    u = tables[("lj", "ulp", 3)]["diam"]
    assert (u != 1.17).sum() == 1 and np.abs(u - 1.17).max() == np.spacing(1.17)


def test_reference_against_the_oracle_and_floors(oracle, tables):
    """pair_terms in fp64 against oracle.evaluate over every case within the floor scale; the floors themselves are at most
    64 x 2^-53 (pair_table.bounds asserts it)."""
    worst = 0.0
    for t in tables.values():
        B = pt.bounds(t, False)
        a = pt.reference(t, dtype=np.float64)
        pot = oracle.make_pot(t["kind"], t["params"])
        uf = np.array([oracle.evaluate(pot, float(r), float(t["diam"][i]), float(t["diam"][j])) for r, i, j in zip(a["r"], a["i"], a["j"])])
        eu, ef = np.abs(uf[:, 0] - a["u"]) / a["Su"], np.abs(uf[:, 1] - a["f"]) / a["Sf"]
        assert eu.max() <= B["u"] and ef.max() <= B["f"], (t["case"], t["variant"], eu.max() / EPS, ef.max() / EPS)
        worst = max(worst, max(pt.floor(t).values()) / EPS)
    print("largest floor: %.1f x 2^-53" % worst)


def test_threshold_tables(oracle, thresholds):
    """The conditions (asserted in threshold_table) and the oracle's decisions against hand arithmetic: a dimer contributes
    iff its reference-form d2 is at most the target."""
    for name, t in thresholds.items():
        assert t["cutoff"] > t["radius"]
        d2 = pt.d2_oracle(t["x"][1::2] - t["x"][0::2])
        pot = oracle.make_pot(t["kind"], t["params"])
        f_ref = oracle.forces_brute(t["x"], t["box"], t["cutoff"], pot, t["diam"])[0]
        nz = np.abs(f_ref[0::2]).max(axis=1) > 0.0
        if name == "poly":          # (the force vanishes AT this edge: some dimers inside it cancel to exactly zero)
            assert not np.any(nz & (d2 > t["target"])) and nz.sum() >= 0.8 * (d2 <= t["target"]).sum()
            assert np.abs(f_ref).max() < 1e-14
            nz = d2 <= t["target"]
        elif name != "ljmod_ron":
            assert np.array_equal(nz, d2 <= t["target"]), name
        assert np.array_equal(pt.reference(t)["live"], nz), name
    assert abs(thresholds["poly"]["radius"] - 1.265) < 1e-12


@pytest.mark.parametrize("form", ["r2", "AB"])
def test_model_passes_every_checker(oracle, tables, thresholds, form):
    """The device's forms in numpy: r^-2 LJ with c48 / c24 / c4, ljA z^7 - ljB z^4 on uniform LJ tables, the sqrt forms, the
    searched d2 threshold."""
    worst = {}
    for key, t in tables.items():
        if form == "AB" and not (t["kind"] == pt.POT_LJ and t["variant"] in ("ones", "uniform")):
            continue
        m = Model(t, form)
        B = pt.bounds(t, _r2(t))
        w = dict(f=pt.check_pair_forces(t, m.forces(), B), blk=pt.check_blocks(t, m.blocks(), pt.bounds(t, False)))
        for b in range(len(t["band_names"])):
            xb = pt.pulled(t, b)
            U, W, vir = m.sums(xb)
            r = pt.check_band_sums(t, b, B, U, W, vir, x=xb)
            for q, v in r.items():
                w[q] = max(w.get(q, 0.0), v)
        for q, v in w.items():
            worst[(t["kind"], q)] = max(worst.get((t["kind"], q), 0.0), v)
    print({k: round(v, 1) for k, v in worst.items()})
    if form == "r2":
        for name, t in thresholds.items():
            m = Model(t)
            q = ("u", "f") if name == "ljmod_ron" else ("u", "f", "k", "blk")
            f = m.forces()
            pt.check_decisions(t, oracle, f)
            pt.check_pair_forces(t, f, pt.bounds(t, _r2(t), quantities=q))


def _model_swap(table, sab=None, seed=SWAP_SEED, ktemp=SWAP_KT):
    """One round at fraction 1.0: the selection is swap_reference's, dU and the decision the model's."""
    pot = sr.orc.make_pot(table["kind"], table["params"])
    frame = sr.Frame(dict(x=table["x"], box=table["box"]), table["cutoff"], pot)
    partner, status, w3 = sr.selection(frame, seed, 0, 1.0)
    m = Model(table, sab=sab)
    diam = table["diam"]
    mate = np.empty(table["n"], dtype=np.int64)
    mate[table["pairs"][:, 0]], mate[table["pairs"][:, 1]] = table["pairs"][:, 1], table["pairs"][:, 0]
    du = np.zeros(table["n"])
    for i in np.flatnonzero(status == -1):
        j = int(partner[i])
        for p, q in ((int(i), j), (j, int(i))):
            k = int(mate[p])
            if k != q:
                du[i] += m.pair_u(p, k, diam[q], diam[k]) - m.pair_u(p, k, diam[p], diam[k])
        u3 = (float(w3[i]) + 0.5) / 2.0 ** 32
        with np.errstate(over="ignore"):
            status[i] = 6 if u3 < np.exp(-du[i] / ktemp) else 5
    return partner, status, du, w3


@pytest.mark.parametrize("case", SWAP_CASES)
def test_model_swap(oracle, tables, case):
    t = tables[(case, "mixed", 3)]
    partner, status, du, w3 = _model_swap(t)
    res = pt.check_swap(t, partner, status, du, t["diam"], w3, SWAP_KT, pt.bounds(t, _r2(t))["u"])
    print(case, res, np.bincount(status[status >= 0], minlength=7))
    pt.swap_conditions(res)
    assert (status == 5).sum() >= 3 and (status == 6).sum() >= 3


# --------------------------------------------------------------------------------------------------------------------
# the sabotages: (name, case, variant, form, checker)
# --------------------------------------------------------------------------------------------------------------------
SABOTAGES = [
    ("c4", "lj_eps", "mixed", "r2", "band_sums"),                   # c4 = 4 instead of 4 eps
    ("ljA_sigma1", "lj", "uniform", "AB", "forces"),                # ljA / ljB forget the uniform sigma
    ("vcut_pair_sigma", "ljmod1", "mixed", "r2", "forces"),         # V_cut, F_cut from the pair's sigma
    ("mode1_sign", "ljmod1", "mixed", "r2", "band_sums"),           # the reference text's sign of the linear term
    ("rc2", "lj_2.2", "threshold", "r2", "decisions"),              # threshold rc^2 instead of the searched one
    ("le", "lj_wca", "threshold", "r2", "decisions"),               # <= for <
    ("phs_b_sigma", "phs50", "mixed", "r2", "forces"),              # the range 50/49 scaled by sigma
    ("poly_nofabs", "poly", "mixed", "r2", "forces"),
    ("poly_c4", "poly", "mixed", "r2", "forces"),                   # c4 over rc^14
    ("xplor_ds", "ljmod2", "mixed", "r2", "forces"),
    ("rcp", "lj", "mixed", "r2", "forces"),                         # a dropped Newton step: 3e-8 relative
    ("phs_k_lambda", "phs50", "mixed", "r2", "blocks"),             # U'' with lambda for lambda + 1
    ("tail_1e-9", "lj", "ones", "r2", "forces"),
]


def _run_checker(oracle, t, form, sab, checker):
    m = Model(t, form, sab)
    B = pt.bounds(t, _r2(t))
    if checker == "forces":
        pt.check_pair_forces(t, m.forces(), B)
    elif checker == "blocks":
        pt.check_blocks(t, m.blocks(), pt.bounds(t, False))
    elif checker == "decisions":
        pt.check_decisions(t, oracle, m.forces())
    else:
        for b in range(len(t["band_names"])):
            xb = pt.pulled(t, b)
            U, W, vir = m.sums(xb)
            pt.check_band_sums(t, b, B, U, W, vir, x=xb)


@pytest.mark.parametrize("sab,case,variant,form,checker", SABOTAGES, ids=[s[0] for s in SABOTAGES])
def test_sabotage_is_caught(oracle, tables, thresholds, sab, case, variant, form, checker):
    t = thresholds[case] if variant == "threshold" else tables[(case, variant, 3)]
    _run_checker(oracle, t, form, None, checker)                    # the honest model passes ...
    with pytest.raises(AssertionError) as e:
        _run_checker(oracle, t, form, sab, checker)                 # ... the sabotaged one is reported
    print(sab, "->", str(e.value)[:160])


def test_threshold_sabotages_flip_only_the_steered_dimers(oracle, thresholds):
    """rc^2 for the searched threshold moves the decision by an ulp or two of d2: only the categories at the edge flip."""
    t = thresholds["lj_2.2"]
    good, bad = Model(t).forces(), Model(t, sab="rc2").forces()
    flipped = np.flatnonzero((np.abs(good).max(axis=1) > 0) != (np.abs(bad).max(axis=1) > 0)) // 2
    assert 0 < len(flipped) and set(t["cat"][flipped]) <= {0, 1, 2, 3, 4, 5}


def test_the_sabotage_that_proves_the_gap(oracle, tables):
    """Forces x (1 + 1e-9) for every pair beyond 2 sigma: invisible to |dF|inf <= 1e-11 max(1, |F|inf) on the liquid the parity
    tests use, reported by the table."""
    s = lj_system(1000)
    kind, params, cutoff = pt.CASES["lj"]
    i, j, dl = hr.pair_list(s["x"], np.diag(s["box"]), cutoff)
    d2 = pt.d2_oracle(dl)
    f_ref = oracle.forces_brute(s["x"], s["box"], cutoff, oracle.make_pot(kind, params), s["diam"])[0]
    for sab, passes in ((None, True), ("tail_1e-9", True)):
        u, fpr, hit = model_eval(kind, params, cutoff, d2, s["diam"][i], s["diam"][j], True, "r2", sab)
        f = np.zeros_like(s["x"])
        np.add.at(f, i, -fpr[:, None] * dl)
        np.add.at(f, j, fpr[:, None] * dl)
        err, tol = np.abs(f - f_ref).max(), 1e-11 * max(1.0, np.abs(f_ref).max())
        print("liquid, sabotage %s: |dF|inf = %.3g, tolerance %.3g" % (sab, err, tol))
        assert err <= tol
    assert (np.sqrt(d2[hit]) > 2.0).sum() > 10000                   # ... although it touched most of the pairs
    t = tables[("lj", "ones", 3)]
    B = pt.bounds(t, True)
    pt.check_pair_forces(t, Model(t).forces(), B)
    with pytest.raises(AssertionError, match="error / S"):
        pt.check_pair_forces(t, Model(t, sab="tail_1e-9").forces(), B)
