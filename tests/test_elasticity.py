"""CPU: proves tests/elas_reference.py (the yardstick of tests/test_gpu_elasticity.py) against finite differences of its own
energy and forces, pins two known answers, shows that the comparison tolerances would catch a wrong kernel, and drives
vibrations.elastic_moduli through a stub device.

Frames: poly64 (poly_system(n=64), 2-D Polydisperse, cutoff 1.5) and xplor108 (elas_reference.fcc_xplor_system(3): 108
particles, 3-D LennardJonesXPLOR with per-particle diameters, its switching radii between the neighbour shells), both taken into their inherent structure by the reference's own steepest descent and
then Newton steps with the pseudo-inverse to max |F| <= 1e-12."""
import os
import re
import types

import numpy as np
import pytest

import moleculardynamics.jl_amd as md
from moleculardynamics.jl_amd import _lib, vibrations
from tests import elas_reference as er
from tests import hess_reference as hr
from tests.util import poly_system

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_FRAMES, _MODULI = {}, {}


def _frame(name):
    if name not in _FRAMES:
        if name == "poly64":
            s, cutoff, kind, params = poly_system(n=64), 1.5, hr.POT_POLYDISPERSE, [1.25, 0.2]
        else:
            s, kind, params, cutoff = er.fcc_xplor_system(3)
        d = s["dim"]
        U = np.diag(np.asarray(s["box"], dtype=np.float64)[:d])
        x = er.descend(s["x"], U, cutoff, kind, params, s["diam"])
        x, g, steps = er.relax(x, U, cutoff, kind, params, s["diam"])
        print("%s: relaxed to max |F| = %.3e in %d Newton steps" % (name, g, steps))
        assert g <= 1e-12
        _FRAMES[name] = dict(x=x, U=U, cutoff=cutoff, kind=kind, params=params, diam=np.array(s["diam"]), n=s["n"], d=d)
    return _FRAMES[name]


def _args(fr, x=None, U=None):
    return (fr["x"] if x is None else x, fr["U"] if U is None else U, fr["cutoff"], fr["kind"], fr["params"], fr["diam"])


def _moduli(name):
    if name not in _MODULI:
        _MODULI[name] = er.moduli(*_args(_frame(name)))
        m = _MODULI[name]
        print("%s: lambda_min = %.4g, refinement %s, floors %s" % (name, m["lambda_min"], m["refine"], m["floor"]))
    return _MODULI[name]


def _deformations(d):
    shear, uni = np.zeros((d, d)), np.zeros((d, d))
    shear[0, 1] = 1.0
    uni[0, 0] = 1.0
    return {"shear": shear, "uniaxial": uni, "isotropic": np.eye(d), "general": np.random.default_rng(1).uniform(-1.0, 1.0, (d, d))}


# ---------------------------------------------------------------------------------------------------------------------
# 1. the formulas against finite differences of the reference's own energy and forces
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("defo", ["shear", "uniaxial", "isotropic", "general"])
@pytest.mark.parametrize("name", ["poly64", "xplor108"])
def test_formulas_against_finite_differences(name, defo):
    """F(h) = I + h E.  Scaled coordinates fixed: d2U/dh2 = V (eta1 : CB : eta1 + sigma : E^T E) and dF_i/dh = -Xi : eta1;
    re-relaxed at +-h: the same with C in place of CB.  Central differences: the error falls as h^2, (10/3)^2 = 11 between
    h = 1e-3 and 3e-4 (asserted: >= 5), and is <= 1e-3 of the prediction at 3e-4.

    The h^2 law needs an energy that is smooth along the path.  XPLOR's U'' jumps at r_on and r_cut, so on the xplor108 frame
    no pair may come near either radius: asserted below, with a margin of twice what the largest h can move a separation,
    h (|E|_2 r_cut + 2 max |u|).  (On a glassy XPLOR
    frame some pair always crosses, and the error falls as h: 15, 6, 3, 0 pairs within reach at h = 1e-3, 3e-4, 1e-4, 3e-5
    of a 108-particle glass gave Born errors of 2e-4, 7e-5, 7e-6, 2e-8.)"""
    fr, m = _frame(name), _moduli(name)
    d, E = fr["d"], _deformations(fr["d"])[defo]
    a, V = m["a64"], m["a64"]["volume"]
    if name == "xplor108":
        margin = er.kink_margin(fr["x"], fr["U"], (er.XPLOR_SMOOTH["r_on"], er.XPLOR_SMOOTH["r_cut"]), 2.4)
        assert margin >= 2.0 * 1e-3 * (np.linalg.norm(E, 2) * er.XPLOR_SMOOTH["r_cut"] + 2.0 * np.abs(m["u"]).max()), margin
    eta1 = 0.5 * (E + E.T)
    w = np.array([(1.0 if p == q else 2.0) * eta1[p, q] for p, q in er.COMPONENTS[d]])
    e0 = er.energy_forces(*_args(fr), dtype=np.longdouble)[0]
    pred_b = er.second_difference_prediction(a["born"], a["stress"], E, V, d)
    pred_c = er.second_difference_prediction(m["C"], a["stress"], E, V, d)
    pred_f = -np.tensordot(w, a["xi"], axes=(0, 0))
    err = {"born": [], "relaxed": [], "force": []}
    for h in (1e-3, 3e-4):
        eb, ec, ff = [], [], []
        for sign in (1.0, -1.0):
            xs, Us = er.strained(fr["x"], fr["U"], np.eye(d) + sign * h * E)
            e, F = er.energy_forces(*_args(fr, xs, Us), dtype=np.longdouble)
            eb.append(e)
            ff.append(F)
            xr, g, _ = er.relax(*_args(fr, xs, Us))
            assert g <= 1e-12
            ec.append(er.energy_forces(*_args(fr, xr, Us), dtype=np.longdouble)[0])
        hh = np.longdouble(h)
        err["born"].append(abs(float((eb[0] - 2 * e0 + eb[1]) / hh ** 2) - pred_b) / abs(pred_b))
        err["relaxed"].append(abs(float((ec[0] - 2 * e0 + ec[1]) / hh ** 2) - pred_c) / abs(pred_c))
        err["force"].append(float(np.abs((ff[0] - ff[1]) / (2 * hh) - pred_f).max()) / np.abs(pred_f).max())
    print("%s/%s: d2U/dh2 Born %.6g, relaxed %.6g" % (name, defo, pred_b, pred_c))
    for key, (e1, e2) in err.items():
        print("   %-8s relative error %.3e at h = 1e-3, %.3e at h = 3e-4, ratio %.2f" % (key, e1, e2, e1 / e2))
    for key, (e1, e2) in err.items():
        assert e2 <= 1e-3, (key, e1, e2)
    for key, (e1, e2) in err.items():
        assert e1 >= 5.0 * e2, (key, e1, e2)
    assert abs(pred_b - pred_c) > 1e-3 * abs(pred_b) or defo == "isotropic"      # (the non-affine term is not a detail)


def test_pair_energy_matches_its_derivatives():
    """pair_u is new here; hess_reference.pair_tk is proven elsewhere: U' = t r by a central difference."""
    for kind, params, (si, sj) in ((hr.POT_POLYDISPERSE, [1.25, 0.2], (0.8, 1.1)), (hr.POT_LJ_MODIFIED, [1.0, 1.0, 2.0, 2.0, 1.5], (1.0, 1.1)),
                                   (hr.POT_LJ, [1.0, 1.0, 2.5], (1.0, 1.0))):
        for r in (0.95, 1.05, 1.12, 1.6, 1.9):
            t, _, inside = hr.pair_tk(kind, params, r, si, sj)
            h = 1e-6                      # (truncation h^2 |U'''| / 6 <= 1e-8: |U'''| stays below 6e4 for r >= 0.95)
            fd = (er.pair_u(kind, params, r + h, si, sj, np.longdouble) - er.pair_u(kind, params, r - h, si, sj, np.longdouble)) / (2 * h)
            if inside and hr.pair_tk(kind, params, r + h, si, sj)[2]:
                assert abs(float(fd) - float(t) * r) <= 1e-8 * abs(float(t) * r) + 1e-8, (kind, r)
    # continuous at the cutoff where the potential is smooth
    assert abs(float(er.pair_u(hr.POT_POLYDISPERSE, [1.25, 0.2], 1.25 * (1 - 1e-9), 1.0, 1.0))) <= 1e-12
    assert abs(float(er.pair_u(hr.POT_LJ_MODIFIED, [1.0, 1.0, 2.0, 2.0, 1.5], 2.0 * (1 - 1e-9), 1.0, 1.0))) <= 1e-12


# ---------------------------------------------------------------------------------------------------------------------
# 2. exact cases
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_relaxed_isolated_dimer(dim):
    """Two Lennard-Jones particles at r = 2^(1/6) along x: t = 0, so CB_xxxx = k r^2 / V; the bond simply keeps its length
    under strain, so the non-affine term cancels CB_xxxx; Xi has no transverse component."""
    r = 2.0 ** (1.0 / 6.0)
    x = np.full((2, dim), 3.0)
    x[1, 0] += r
    U = np.eye(dim) * 20.0
    m = er.moduli(x, U, 3.0, hr.POT_LJ, [1.0, 1.0, 2.5], np.ones(2))
    t, k, _ = (float(v) for v in hr.pair_tk(hr.POT_LJ, [1.0, 1.0, 2.5], x[1, 0] - x[0, 0], 1.0, 1.0))
    V = 20.0 ** dim
    cb = m["a64"]["born"][0, 0]
    assert abs(t) <= 1e-13 * k
    assert abs(cb - k * (x[1, 0] - x[0, 0]) ** 2 / V) <= 1e-12 * cb
    assert abs(m["N"][0, 0] + cb) <= 1e-12 * cb and abs(m["C"][0, 0]) <= 1e-12 * cb
    xi = m["a64"]["xi"]
    assert np.abs(xi[0, :, 0]).max() > 0.1 * k and np.abs(xi[:, :, 1:]).max() <= 1e-12 * np.abs(xi).max()
    assert np.abs(xi[1:]).max() <= 1e-12 * np.abs(xi).max()                       # only the xx strain stretches the bond


def test_fcc_crystal_is_affine_with_cubic_symmetry():
    """A perfect fcc Lennard-Jones crystal (test_fcc_crystal_site_blocks_are_equal_and_isotropic's): every site is a centre
    of inversion, so Xi = 0 and C = CB; cubic symmetry; a pair potential's Born tensor obeys the Cauchy relation."""
    mm, rho = 4, 1.0
    a = (4.0 / rho) ** (1.0 / 3.0)
    base = np.array([[0, 0, 0], [0.5, 0.5, 0], [0.5, 0, 0.5], [0, 0.5, 0.5]])
    cells = np.stack(np.meshgrid(*[np.arange(mm)] * 3, indexing="ij"), -1).reshape(-1, 1, 3)
    x = ((cells + base[None]) * a).reshape(-1, 3)
    n = len(x)
    A = er.affine(x, np.eye(3) * (mm * a), 2.5, hr.POT_LJ, [1.0, 1.0, 2.5], np.ones(n))
    assert np.all(np.abs(A["xi"]) <= 1e-11 * A["xi_abs"]) and A["xi_abs"].max() > 1.0
    B = A["born"]
    scale = np.abs(B).max()
    c11, c12, c44 = B[0, 0], B[0, 1], B[3, 3]
    want = np.zeros((6, 6))
    want[:3, :3] = c12
    want[np.arange(3), np.arange(3)] = c11
    want[np.arange(3, 6), np.arange(3, 6)] = c44
    print("fcc: C11 = %.6f, C12 = %.6f, C44 = %.6f, max |Xi| / sum |terms| = %.2e"
          % (c11, c12, c44, (np.abs(A["xi"]) / A["xi_abs"]).max()))
    assert np.abs(B - want).max() <= 1e-12 * scale and c11 > c12 > 0.0
    assert abs(c12 - c44) <= 1e-13 * scale                                         # Cauchy
    # with Xi = 0 to rounding the non-affine term Xi H^+ Xi / V is rounding squared (|H^+| <= 1 / lambda_min): C = CB
    H = hr.dense(x, np.eye(3) * (mm * a), 2.5, hr.POT_LJ, [1.0, 1.0, 2.5], np.ones(n))
    lmin = er.lambda_min(H, n, 3)
    assert lmin > 0.0 and (np.abs(A["xi"]) ** 2).sum(axis=(1, 2)).max() / (lmin * A["volume"]) <= 1e-20 * scale


# ---------------------------------------------------------------------------------------------------------------------
# 3. sabotage: the tolerances of the GPU tests would catch a wrong kernel
# ---------------------------------------------------------------------------------------------------------------------
def _rel_change(a, b):
    """max over sigma, CB and Xi of the largest entry's change, each relative to its own largest entry."""
    return max(float(np.abs(np.asarray(a[k], dtype=np.float64) - np.asarray(b[k], dtype=np.float64)).max()
                     / np.abs(np.asarray(b[k], dtype=np.float64)).max()) for k in ("stress", "born", "xi"))


def _raw_frame(name):
    """The same systems before any relaxation: the forces do not vanish, so the t-term of Xi does not sum to zero (at a
    minimum it does -- sum_j t del is the force -- and a kernel that drops it would go unseen on a relaxed frame)."""
    fr = dict(_frame(name))
    s = poly_system(n=64) if name == "poly64" else er.fcc_xplor_system(3)[0]
    fr["x"] = np.array(s["x"])
    return fr


@pytest.mark.parametrize("name", ["poly64", "xplor108"])
def test_a_wrong_kernel_is_far_above_the_tolerance(name):
    """Each mistake moves some entry of sigma, CB or Xi by more than 1e-5 of that array's largest entry, against a
    comparison tolerance of 10 x the rounding floor (printed).  Frames: the systems as generated, not relaxed."""
    fr = _raw_frame(name)
    pairs = hr.pair_list(fr["x"], fr["U"], fr["cutoff"])
    a = er.affine(*_args(fr), pairs=pairs)
    a80 = er.affine(*_args(fr), dtype=np.longdouble)
    rel = lambda key: float(np.abs(a[key] - a80[key]).max() / np.abs(a80[key]).max())
    tol = 10.0 * max(rel("stress"), rel("born"), rel("xi"))
    i, j, dl, t, k = er.pair_terms(*_args(fr), pairs=pairs)
    # the weakest pair: the one whose largest Xi term is smallest
    strength = (np.abs((k - t) / (dl * dl).sum(axis=1))[:, None] * np.abs(dl) ** 3 + np.abs(t)[:, None] * np.abs(dl)).max(axis=1)
    weakest = int(np.argmin(strength))
    cases = {"weakest pair left out": ("drop", weakest), "no t-term in Xi": "no_t", "engineering factor 2 on shear": "engineering",
             "pair members not antisymmetric": "one_sided", "CB with k for k - t": "born_k"}
    print("%s (not relaxed): %d pairs; comparison tolerance (10 x floor, relative) %.3e" % (name, len(i), tol))
    for label, sab in cases.items():
        b = er.affine(*_args(fr), pairs=pairs, sabotage=sab)
        seen = _rel_change(b, a)
        print("   %-32s moves an entry by %.3e" % (label, seen))
        assert seen > 1e-5 and seen > 10.0 * tol, label
    # on the relaxed frame the engineering factor changes the moduli by O(1) of the non-affine term
    fr, m = _frame(name), _moduli(name)
    nc = len(er.COMPONENTS[fr["d"]])
    b = er.affine(*_args(fr), sabotage="engineering")
    u, _ = er.solve(m["H"], m["H"].astype(np.longdouble), -b["xi"].reshape(nc, -1), fr["n"], fr["d"], refine=False)
    N = (b["xi"].reshape(nc, -1) @ u.astype(np.float64).T) / b["volume"]
    assert np.abs(N - m["N"]).max() > 1e-2 * np.abs(m["N"]).max()


# ---------------------------------------------------------------------------------------------------------------------
# 4. vibrations.elastic_moduli on a stub device
# ---------------------------------------------------------------------------------------------------------------------
class _StubDevice:
    """hess_setup / elas_* backed by the reference: what MDDevice promises, nothing of how it computes it."""
    ELAS_CONVERGED, ELAS_MAX_ITER, ELAS_INDEFINITE = 1, 2, 4

    def __init__(self, m, n, dim, status=1):
        self.m, self.n, self.dim, self.status = m, n, dim, status
        self.frozen = self.affine_done = False
        self.calls = []

    @property
    def elas_components(self):
        return er.COMPONENTS[self.dim]

    def set_potential(self, kind, params):
        self.calls.append(("set_potential", kind))

    def upload(self, **kw):
        self.calls.append(("upload",))
        self.frozen = self.affine_done = False

    def hess_setup(self):
        self.calls.append(("hess_setup",))
        self.frozen, self.affine_done = True, False

    def elas_affine(self, fields=False):
        if not self.frozen:
            raise md.MdhipError("md_elas_affine: no operator for the frame the handle holds now: call md_hess_setup")
        self.calls.append(("elas_affine", fields))
        self.affine_done = True
        a = self.m["a64"]
        out = dict(stress=np.array(a["stress"]), born=0.5 * (a["born"] + a["born"].T))   # (the device's is symmetric)
        if fields:
            out["xi"] = np.array(a["xi"])
        return out

    def elas_solve(self, tol, max_iter, fields=True):
        if not (self.frozen and self.affine_done):
            raise md.MdhipError("md_elas_solve: no affine pass: call md_hess_setup")
        self.calls.append(("elas_solve", tol, max_iter, fields))
        nc = len(self.elas_components)
        N = np.array(self.m["N"])
        N[0, 1] += 1e-9                                                       # (an asymmetry to find again)
        return dict(nonaffine=N, iterations=np.full(nc, 17), residuals=np.full(nc, 1e-11), xi_norm=np.ones(nc),
                    status=self.status, converged=bool(self.status & 1), indefinite=bool(self.status & 4), u=np.array(self.m["u"]))


def _stub_state(name="poly64", status=1):
    fr, m = _frame(name), _moduli(name)
    n, d = fr["n"], fr["d"]
    dev = _StubDevice(m, n, d, status)
    system = types.SimpleNamespace(device=dev, positions=np.array(fr["x"]), xpositions=None,
                                   energy_and_forces=types.SimpleNamespace(forces=np.zeros((n, d)), energy=0.0, virial=0.0))
    state = md.SimulationState(system, np.array(fr["diam"]), np.random.default_rng(1), fr["U"], np.zeros((n, d)),
                               np.zeros((n, d), dtype=np.int32), d, d * (n - 1.0))
    pot = md.Polydisperse(1.25, 0.2) if name == "poly64" else md.LennardJonesXPLOR(epsilon=1.0, sigma=1.0, r_cut=2.0, r_on=1.5)
    return state, md.Parameters(1.0, n, 0.002, pot), dev, m


KEYS = {"components", "volume", "stress", "born", "nonaffine", "moduli", "asymmetry", "shear_modulus", "bulk_modulus",
        "born_shear_modulus", "born_bulk_modulus", "displacements", "affine_forces", "residuals", "iterations", "converged",
        "indefinite", "stable", "operator"}


@pytest.mark.parametrize("name", ["poly64", "xplor108"])
def test_elastic_moduli_on_a_stub_device(name):
    state, params, dev, m = _stub_state(name)
    n, d = dev.n, dev.dim
    res = md.elastic_moduli(state, params)
    assert set(res) == KEYS
    assert [c[0] for c in dev.calls] == ["set_potential", "upload", "hess_setup", "elas_affine", "elas_solve"]
    assert dev.calls[-1][1:] == (1e-10, n * d, True) and dev.calls[-2][1] is True      # defaults: tol, max_iter = N d
    comps = res["components"]
    assert comps == (((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)) if d == 3 else ((0, 0), (1, 1), (0, 1)))
    nc = len(comps)
    a = m["a64"]
    assert res["volume"] == pytest.approx(a["volume"], rel=1e-14)
    assert np.array_equal(res["stress"], er.stress_matrix(a["stress"], d)) and np.array_equal(res["stress"], res["stress"].T)
    assert np.array_equal(res["born"], 0.5 * (a["born"] + a["born"].T)) and res["nonaffine"].shape == (nc, nc)
    N = res["nonaffine"]
    assert np.array_equal(res["moduli"], res["born"] + 0.5 * (N + N.T)) and np.array_equal(res["moduli"], res["moduli"].T)
    assert res["asymmetry"] == np.abs(N - N.T).max() and 0.5e-9 < res["asymmetry"] < 2e-9
    C, B = res["moduli"], res["born"]
    ix = {c: i for i, c in enumerate(comps)}
    shear = np.mean([C[ix[(p, q)], ix[(p, q)]] for p in range(d) for q in range(p + 1, d)])
    bulk = sum(C[p, q] for p in range(d) for q in range(d)) / d ** 2
    assert res["shear_modulus"] == pytest.approx(shear, rel=1e-14) and res["bulk_modulus"] == pytest.approx(bulk, rel=1e-14)
    assert res["born_bulk_modulus"] == pytest.approx(B[:d, :d].sum() / d ** 2, rel=1e-14)
    assert res["born_shear_modulus"] == pytest.approx(np.mean([B[i, i] for i in range(d, nc)]), rel=1e-14)
    assert 0.0 < res["shear_modulus"] < res["born_shear_modulus"]                      # relaxation only softens
    # the assembled tensor predicts the reference's relaxed energy difference (test 1 ties that to finite differences)
    E = _deformations(d)["general"]
    assert er.second_difference_prediction(C, a["stress"], E, a["volume"], d) == pytest.approx(
        er.second_difference_prediction(m["C"], a["stress"], E, a["volume"], d), rel=1e-8)
    assert res["displacements"].shape == (nc, n, d) and res["affine_forces"].shape == (nc, n, d)
    assert np.array_equal(res["iterations"], np.full(nc, 17)) and np.array_equal(res["residuals"], np.full(nc, 1e-11))
    assert res["converged"] is True and res["indefinite"] is False and res["stable"] is True
    assert isinstance(res["operator"], md.HessianOperator) and res["operator"].device is dev
    # operator= is reused: no second upload, no second hess_setup
    dev.calls.clear()
    res2 = md.elastic_moduli(state, params, tol=1e-8, max_iter=50, operator=res["operator"])
    assert [c[0] for c in dev.calls] == ["elas_affine", "elas_solve"] and dev.calls[-1][1:] == (1e-8, 50, True)
    assert res2["operator"] is res["operator"] and np.array_equal(res2["moduli"], res["moduli"])
    for kw in (dict(tol=0.0), dict(max_iter=0), dict(operator=dev)):
        with pytest.raises(ValueError):
            md.elastic_moduli(state, params, **kw)
    dev.upload()                                                               # the frame changes: the operator is stale
    with pytest.raises(md.MdhipError, match="md_hess_setup"):
        md.elastic_moduli(state, params, operator=res["operator"])


@pytest.mark.parametrize("status,flags", [(1, (True, False, True)), (2, (False, False, False)), (4, (False, True, False)),
                                          (1 | 4, (True, True, False)), (2 | 4, (False, True, False))])
def test_flags_follow_the_status_bits(status, flags):
    state, params, dev, _ = _stub_state("poly64", status)
    res = md.elastic_moduli(state, params)                                     # nothing is raised for any of them
    assert (res["converged"], res["indefinite"], res["stable"]) == flags


def test_user_potentials_are_refused_by_the_python_layer():
    state, params, dev, _ = _stub_state()

    class UserPotential(md.Potential):
        def device_spec(self):
            return ("source", "src", "entry", ())

    with pytest.raises(ValueError, match="built-in"):
        md.elastic_moduli(state, md.Parameters(1.0, dev.n, 0.002, UserPotential()))
    assert dev.calls == []


# ---------------------------------------------------------------------------------------------------------------------
# 5. the interface
# ---------------------------------------------------------------------------------------------------------------------
def test_symbols_bindings_header_and_makefile():
    import ctypes as C
    assert "md_elas_affine" in _lib.EXPORTS and "md_elas_solve" in _lib.EXPORTS
    assert "elastic_moduli" in md.__all__ and md.elastic_moduli is vibrations.elastic_moduli
    header = open(os.path.join(ROOT, "include", "mdhip.h")).read()
    defs = dict(re.findall(r"^#define (MD_ELAS_[A-Z_]+) (\d+)", header, flags=re.M))
    assert {k: int(v) for k, v in defs.items()} == {"MD_ELAS_CONVERGED": _lib.MD_ELAS_CONVERGED, "MD_ELAS_MAX_ITER": _lib.MD_ELAS_MAX_ITER,
                                                    "MD_ELAS_INDEFINITE": _lib.MD_ELAS_INDEFINITE} == \
        {"MD_ELAS_CONVERGED": 1, "MD_ELAS_MAX_ITER": 2, "MD_ELAS_INDEFINITE": 4}
    assert (md.MDDevice.ELAS_CONVERGED, md.MDDevice.ELAS_MAX_ITER, md.MDDevice.ELAS_INDEFINITE) == (1, 2, 4)
    assert re.search(r"int md_elas_affine\(md_ctx \*ctx, double \*stress, double \*born, double \*xi\);", header)
    assert re.search(r"int md_elas_solve\(md_ctx \*ctx, double tol, int64_t max_iter, int64_t \*iters, double \*resid, double \*xi_norm, "
                     r"int \*status,\s+double \*nonaffine, double \*u\);", header)
    make = open(os.path.join(ROOT, "moleculardynamics", "jl_amd", "csrc", "Makefile")).read()
    rule = [l for l in make.splitlines() if l.startswith("libmdhip.so:")][0]
    assert "md_elas.hpp" in rule.split() and "md_hess.hpp" in rule.split()
    lib = _lib.load()
    dp = C.POINTER(C.c_double)
    assert lib.md_elas_affine.argtypes == [C.c_void_p, dp, dp, dp] and lib.md_elas_affine.restype is C.c_int
    assert lib.md_elas_solve.argtypes == [C.c_void_p, C.c_double, C.c_int64, C.POINTER(C.c_int64), dp, dp, C.POINTER(C.c_int), dp, dp]
    for text in (vibrations.__doc__, vibrations.lowest_modes.__doc__, open(os.path.join(ROOT, "DESIGN.md")).read()):
        assert "elastic moduli are not provided" not in " ".join(text.split())


def test_a_null_handle_is_refused():
    lib = _lib.load()
    assert lib.md_elas_affine(None, None, None, None) != 0
    assert b"null handle" in lib.md_last_error(None)
    assert lib.md_elas_solve(None, 1e-10, 10, None, None, None, None, None, None) != 0
    assert b"null handle" in lib.md_last_error(None)
