"""-m gpu: elastic moduli of a minimum on the device (md_elas_*, vibrations.elastic_moduli) against tests/elas_reference.py,
on every list layout the handle can take.

Frames (tests/test_gpu_hessian.py's): lj500, poly1200, tric512, xplor500 for the affine pass; poly256 and lj500 (relaxed by
the device's FIRE) and xplor_tric (elas_reference.fcc_xplor_system(4): LennardJonesXPLOR, per-particle diameters, N = 256,
its switching radii between the neighbour shells, in a sheared cell, relaxed by the device's FIRE to 1e-9) for the solve; poly256_raw for a frame that is no minimum.

Tolerances.  Affine quantities: 10 x the frame's fp64 rounding floor (the reference's sequential float64 sums against its
numpy.longdouble ones).  The solve: the bound of a symmetric system, |N_dev - N_ref|_st <= (|Xi_s| resid_t + |Xi_t| resid_s)
/ (lambda_min V) and |u_dev - u_ref| <= resid / lambda_min, plus 10 x the floor.  All computed here, never from the device."""
import ctypes as C

import numpy as np
import pytest

from tests import elas_reference as er
from tests import hess_reference as hr
from tests.test_gpu_hessian import LAYOUTS, _check_layout, _set_layout, frame, state_of
from tests.util import lj_system, sheared

pytestmark = pytest.mark.gpu

_XT, _AFF, _MOD = {}, {}, {}


FIRE_DT = {"xplor_tric": (0.0005, 0.005)}     # (unequal diameters on a lattice: steps of 0.002 .. 0.02 let FIRE diverge from a
#                                               start like that; these do not)


def _fire(dev, name):
    dt0, dt1 = FIRE_DT.get(name, (0.002, 0.02))
    return dev.fire_minimize(max_steps=30000, tol=1e-9, dt_initial=dt0, dt_max=dt1)


def eframe(name):
    if name != "xplor_tric":
        return frame(name)
    if not _XT:
        from moleculardynamics.jl_amd import MDDevice
        import moleculardynamics.jl_amd as md
        s, kind, params, cutoff = er.fcc_xplor_system(4)
        pot = md.LennardJonesXPLOR(epsilon=1.0, sigma=1.0, r_cut=er.XPLOR_SMOOTH["r_cut"], r_on=er.XPLOR_SMOOTH["r_on"])
        spec = pot.device_spec()
        assert spec[1] == kind and list(spec[2]) == params
        s = sheared(s, s["spacing"])              # (a lattice vector of the fcc lattice: the crystal stays periodic)
        with MDDevice(3, s["n"], s["cell"], cutoff) as dev:
            dev.set_potential(spec[1], spec[2])
            dev.upload(s["x"], np.zeros_like(s["x"]), np.zeros_like(s["x"]), s["img"], s["diam"])
            r = _fire(dev, name)
            assert r["converged"], r
            s = dict(s, x=np.ascontiguousarray(dev.download()[0]), fire=r)
        _XT.update(name=name, system=s, cutoff=cutoff, pot=pot, kind=spec[1], params=list(spec[2]))
        print("xplor_tric: FIRE %s" % (s["fire"],))
    return _XT


def _ref_args(fr, x=None, U=None):
    s = fr["system"]
    U0 = hr.lattice(s.get("cell", s["box"]), s["dim"])
    return (s["x"] if x is None else x, U0 if U is None else U, fr["cutoff"], fr["kind"], fr["params"], s["diam"])


def affine_ref(name):
    if name not in _AFF:
        _AFF[name] = er.affine_floor(*_ref_args(eframe(name)))
        print("%s: floors of the affine quantities %s" % (name, _AFF[name][2]))
    return _AFF[name]


def moduli_ref(name):
    if name not in _MOD:
        _MOD[name] = er.moduli(*_ref_args(eframe(name)))
        m = _MOD[name]
        print("%s: lambda_min %.4g, refinement %s, floors %s" % (name, m["lambda_min"], m["refine"], m["floor"]))
    return _MOD[name]


def _vec(stress_matrix, d):
    return np.array([stress_matrix[a, b] for a, b in er.COMPONENTS[d]])


# ---------------------------------------------------------------------------------------------------------------------
# a. the affine pass
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("name", ["lj500", "poly1200", "tric512", "xplor500"])
def test_affine_pass_against_the_reference(monkeypatch, name, layout):
    import moleculardynamics.jl_amd as md
    _set_layout(monkeypatch, layout)
    fr = eframe(name)
    a64, a80, floor = affine_ref(name)
    s = fr["system"]
    d = s["dim"]
    state, params = state_of(fr)
    with state.system.device as dev:
        md.HessianOperator(state, params)
        info = _check_layout(dev, layout)
        A = dev.elas_affine(fields=True)
        B = dev.elas_affine(fields=True)
        dev.stress_setup(0)
        dev.stress_sample()
        _, vir = dev.stress_tensor()
        A2 = dev.elas_affine(fields=False)
    e_s = np.abs(A["stress"] - a80["stress"]).max()
    e_b = np.abs(A["born"] - a80["born"]).max()
    e_x = np.abs(A["xi"] - a80["xi"]).max() / np.abs(a80["xi"]).max()
    e_v = np.abs(A["stress"] + vir / a64["volume"]).max()
    print("%s/%s (fused_build %d): |sigma - ref| %.3e (allowed %.3e), |CB - ref| %.3e (allowed %.3e), |Xi - ref| / max|Xi| %.3e "
          "(allowed %.3e); |sigma + vir / V| %.3e (allowed %.3e)"
          % (name, layout, info["fused_build"], e_s, 10 * floor["stress"], e_b, 10 * floor["born"], e_x, 10 * floor["xi"], e_v,
             1e-13 * a64["stress_abs"].max()))
    assert e_s <= 10 * floor["stress"] and e_b <= 10 * floor["born"] and e_x <= 10 * floor["xi"]
    assert e_v <= 1e-13 * a64["stress_abs"].max()
    assert np.array_equal(A["born"], A["born"].T)
    for k in ("stress", "born", "xi"):
        assert np.array_equal(A[k], B[k]), k
    assert np.array_equal(A2["stress"], A["stress"]) and np.array_equal(A2["born"], A["born"]) and "xi" not in A2
    assert A["xi"].shape == (len(er.COMPONENTS[d]), s["n"], d)


# ---------------------------------------------------------------------------------------------------------------------
# b. the solve
# ---------------------------------------------------------------------------------------------------------------------
_SOLVED = {}


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("name", ["poly256", "lj500", "xplor_tric"])
def test_solve_against_the_reference(monkeypatch, name, layout):
    import moleculardynamics.jl_amd as md
    _set_layout(monkeypatch, layout)
    fr = eframe(name)
    m = moduli_ref(name)
    s = fr["system"]
    n, d = s["n"], s["dim"]
    nc = len(er.COMPONENTS[d])
    tol = 1e-10
    state, params = state_of(fr)
    with state.system.device as dev:
        res = md.elastic_moduli(state, params, tol=tol)
        _check_layout(dev, layout)
        sol = dev.elas_solve(tol, n * d)
    V, lmin, floor = m["a64"]["volume"], m["lambda_min"], m["floor"]
    resid, u, N = res["residuals"], res["displacements"], res["nonaffine"]
    xin = np.sqrt((res["affine_forces"].reshape(nc, -1) ** 2).sum(axis=1))
    bound_N = (xin[:, None] * resid[None, :] + xin[None, :] * resid[:, None]) / (lmin * V) + 10 * floor["N"]
    err_N = np.abs(N - m["N"])
    err_u = np.abs(u - m["u"]).reshape(nc, -1).max(axis=1)
    # (|u_dev - u_ref|_2 <= resid / lambda_min bounds every element)
    bound_u = resid / lmin + 10 * floor["u"]
    mean_u = np.abs(u.mean(axis=1)).max()
    print("%s/%s: iterations %s, converged %s\n  resid / (tol |Xi|)      %s\n  |N - Nref|  max %.3e  (allowed, at that entry, %.3e; floor %.3e)"
          "\n  |u - uref|  %s\n  allowed     %s\n  asymmetry %.3e (allowed %.3e), |mean u| %.3e (allowed %.3e)"
          % (name, layout, res["iterations"], res["converged"], resid / (tol * xin), err_N.max(), bound_N.flat[np.argmax(err_N)],
             floor["N"], err_u, bound_u, res["asymmetry"], 2 * bound_N.max(), mean_u, 1e-12 * np.abs(u).max()))
    print("  shear modulus %.6g (Born %.6g), bulk modulus %.6g (Born %.6g); reference C: shear %.6g"
          % (res["shear_modulus"], res["born_shear_modulus"], res["bulk_modulus"], res["born_bulk_modulus"],
             np.mean([m["C"][i, i] for i in range(d, nc)])))
    assert res["converged"] and res["stable"] and not res["indefinite"]
    assert np.all(resid <= tol * sol["xi_norm"]) and np.all(np.abs(sol["xi_norm"] - xin) <= 1e-12 * xin)
    assert np.all(res["iterations"] >= 1) and np.all(res["iterations"] <= n * d)
    assert np.all(err_N <= bound_N) and np.all(err_u <= bound_u)
    assert mean_u <= 1e-12 * np.abs(u).max()
    assert np.all(np.abs(N - N.T) <= bound_N + bound_N.T)
    assert np.array_equal(sol["nonaffine"], N) and np.array_equal(sol["u"], u)          # a second solve: the same bits
    # the moduli of the three layouts agree within the bound
    _SOLVED.setdefault(name, {})[layout] = (res["moduli"], bound_N)
    for other, (C0, b0) in _SOLVED[name].items():
        assert np.all(np.abs(res["moduli"] - C0) <= bound_N + b0 + 20 * floor["born"]), (layout, other)


# ---------------------------------------------------------------------------------------------------------------------
# c. the energy's second difference through the device's own FIRE
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["poly256", "xplor_tric"])
def test_second_difference_through_fire(name):
    """U(F(+h)) - 2 U(0) + U(F(-h)) over h^2, every energy a minimum the device's FIRE found, against V (eta1 : C : eta1 +
    sigma : E^T E) from elastic_moduli.  Allowed: 10 x the error of the same difference taken with the reference's relaxer
    and the reference's C; the reference itself must stay below 1e-3 at h = 3e-4 (no rearrangement under strain).

    Both potentials must be smooth along the path.  Polydisperse is C2 at its cutoff.  XPLOR's U'' jumps at r_on and r_cut, so
    on xplor_tric no pair may come near either radius: asserted, with a margin of twice what the largest h can move a
    separation, h (|E| r_cut + 2 max |u|) with |E| = 1 for both deformations here.  (The cell's face distance keeps r_cut
    below 2.129, just above the last pair of the third shell.)  tests/test_elasticity.py shows what a crossing pair does."""
    import moleculardynamics.jl_amd as md
    fr = eframe(name)
    m = moduli_ref(name)
    s = fr["system"]
    n, d = s["n"], s["dim"]
    U0 = hr.lattice(s.get("cell", s["box"]), d)
    V, a = m["a64"]["volume"], m["a64"]
    spec = fr["pot"].device_spec()
    z = np.zeros((n, d))

    def fire_energy(x, cell):
        with md.MDDevice(d, n, cell, fr["cutoff"]) as dev:
            dev.set_potential(spec[1], spec[2])
            dev.upload(x, z, z, np.zeros((n, d), dtype=np.int32), s["diam"])
            r = _fire(dev, name)
            assert r["converged"], r
            return r["energy"]

    if name == "xplor_tric":
        margin = er.kink_margin(s["x"], U0, (er.XPLOR_SMOOTH["r_on"], er.XPLOR_SMOOTH["r_cut"]), 2.4)
        print("xplor_tric: nearest pair to r_on or r_cut %.4f, max |u| %.3f" % (margin, np.abs(m["u"]).max()))
        assert margin >= 2.0 * 1e-3 * (er.XPLOR_SMOOTH["r_cut"] + 2.0 * np.abs(m["u"]).max())
    state, params = state_of(fr)
    with state.system.device:
        res = md.elastic_moduli(state, params)
    assert res["stable"]
    e0_dev = fire_energy(s["x"], s.get("cell", s["box"]))
    e0_ref = er.energy_forces(*_ref_args(fr), dtype=np.longdouble)[0]
    assert abs(e0_dev - float(e0_ref)) <= 1e-10 * abs(e0_dev)
    shear = np.zeros((d, d))
    shear[0, 1] = 1.0
    rows = []
    for label, E in (("shear", shear), ("isotropic", np.eye(d))):
        pred_dev = er.second_difference_prediction(res["moduli"], _vec(res["stress"], d), E, res["volume"], d)
        pred_ref = er.second_difference_prediction(m["C"], a["stress"], E, V, d)
        for h in (1e-3, 3e-4):
            ed, erf = [], []
            for sign in (1.0, -1.0):
                xs, Us = er.strained(s["x"], U0, np.eye(d) + sign * h * E)
                xr, g, _ = er.relax(*_ref_args(fr, xs, Us))
                assert g <= 1e-12
                erf.append(er.energy_forces(*_ref_args(fr, xr, Us), dtype=np.longdouble)[0])
                ed.append(fire_energy(xs, Us))
            hh = np.longdouble(h)
            err_ref = abs(float((erf[0] - 2 * e0_ref + erf[1]) / hh ** 2) - pred_ref) / abs(pred_ref)
            err_dev = abs((ed[0] - 2.0 * e0_dev + ed[1]) / h ** 2 - pred_dev) / abs(pred_dev)
            print("%s/%s h = %g: prediction %.8g (reference %.8g); relative error device %.3e, reference %.3e (allowed %.3e)"
                  % (name, label, h, pred_dev, pred_ref, err_dev, err_ref, 10 * err_ref))
            rows.append((label, h, err_dev, err_ref))
    for label, h, err_dev, err_ref in rows:
        assert err_dev <= 10 * err_ref, (label, h)
    for label, h, err_dev, err_ref in rows:
        if h == 3e-4:
            assert err_ref <= 1e-3, "the reference itself is off by %.3e under %s strain at h = %g: not smooth enough a frame" % (err_ref, label, h)


# ---------------------------------------------------------------------------------------------------------------------
# d. a frame that was not minimised
# ---------------------------------------------------------------------------------------------------------------------
def test_a_frame_that_was_not_minimised():
    import moleculardynamics.jl_amd as md
    fr = eframe("poly256_raw")
    state, params = state_of(fr)
    with state.system.device:
        res = md.elastic_moduli(state, params, max_iter=200)
        res2 = md.elastic_moduli(state, params, max_iter=200, operator=res["operator"])
    print("poly256_raw: converged %s, indefinite %s, iterations %s, residuals %s"
          % (res["converged"], res["indefinite"], res["iterations"], res["residuals"]))
    assert res["stable"] is False and (res["indefinite"] or not res["converged"])
    for k in ("nonaffine", "displacements", "residuals", "iterations", "born", "affine_forces"):
        assert np.array_equal(res[k], res2[k], equal_nan=True), k


# ---------------------------------------------------------------------------------------------------------------------
# e. invalidation and refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_invalidation_and_refusals():
    import moleculardynamics.jl_amd as md
    fr = eframe("lj500")
    s = fr["system"]
    n, d = s["n"], s["dim"]
    state, params = state_of(fr)
    with state.system.device as dev:
        md.HessianOperator(state, params)
        with pytest.raises(md.MdhipError, match="md_elas_affine"):
            dev.elas_solve(1e-10, 10)                                          # (no affine pass on this operator yet)
        A = dev.elas_affine()
        S = dev.elas_solve(1e-8, n * d, fields=False)
        dev.compute_forces()                                                   # (a valid list: nothing moves)
        assert np.array_equal(dev.elas_affine()["born"], A["born"])
        assert np.array_equal(dev.elas_solve(1e-8, n * d, fields=False)["nonaffine"], S["nonaffine"])
        dev.hess_setup()                                                       # a new operator: the affine pass is not its
        with pytest.raises(md.MdhipError, match="md_elas_affine"):
            dev.elas_solve(1e-10, 10)
        dev.elas_affine()
        for change in (lambda: dev.upload(v=s["v"]), lambda: dev.run(1, 0.002), lambda: dev.fire_minimize(max_steps=2, tol=1e-300)):
            change()
            for call in (dev.elas_affine, lambda: dev.elas_solve(1e-10, 10)):
                with pytest.raises(md.MdhipError, match="md_hess_setup"):
                    call()
            dev.hess_setup()
            dev.elas_affine()
            dev.elas_solve(1e-6, 5, fields=False)
        for bad in (dict(tol=0.0, max_iter=10), dict(tol=-1.0, max_iter=10), dict(tol=float("nan"), max_iter=10), dict(tol=1e-8, max_iter=0)):
            with pytest.raises(ValueError):
                dev.elas_solve(**bad)
        # the same through the C entry itself
        nc = 6
        it = (C.c_int64 * nc)()
        r, x, N, st = (C.c_double * nc)(), (C.c_double * nc)(), (C.c_double * (nc * nc))(), C.c_int()
        L, h = dev._L, dev._h
        assert L.md_elas_solve(h, 0.0, 10, it, r, x, C.byref(st), N, None) != 0 and b"tol" in L.md_last_error(h)
        assert L.md_elas_solve(h, 1e-8, 0, it, r, x, C.byref(st), N, None) != 0 and b"max_iter" in L.md_last_error(h)
        assert L.md_elas_solve(h, 1e-8, 10, None, r, x, C.byref(st), N, None) != 0 and b"null" in L.md_last_error(h)
        assert L.md_elas_affine(h, None, N, None) != 0 and b"null" in L.md_last_error(h)


def test_user_potentials_and_slab_handles_are_refused():
    from moleculardynamics.jl_amd import MDDevice, MdhipError
    from moleculardynamics.jl_amd.domain import DomainDevice
    from tests.test_gpu_parity import USER_LJ_SRC
    s = lj_system(500)
    with MDDevice(3, 500, s["box"], 2.5) as dev:
        dev.set_potential(0, [1.0, 1.0, 2.5])
        dev.upload(s["x"], s["v"], s["f"], s["img"], s["diam"])
        dev.hess_setup()
        dev.elas_affine()
        dev.set_potential_source(USER_LJ_SRC, "user_lj", [1.0, 2.5])
        with pytest.raises(MdhipError, match="md_elas_affine: not available with a user potential"):
            dev.elas_affine()
        with pytest.raises(MdhipError, match="md_elas_solve: not available with a user potential"):
            dev.elas_solve(1e-8, 10)

    class TwoRanks:
        rank, world = 0, 2

    s = lj_system(4096)
    with DomainDevice(3, s["n"], s["box"], 2.5, TwoRanks()) as dom:
        buf = (C.c_double * 36)()
        assert dom._L.md_elas_affine(dom._h, buf, buf, None) != 0
        assert "md_elas_affine: not available on a slab-decomposition handle" in dom._L.md_last_error(dom._h).decode()
        it, st = (C.c_int64 * 6)(), C.c_int()
        assert dom._L.md_elas_solve(dom._h, 1e-8, 10, it, buf, buf, C.byref(st), buf, None) != 0
        assert "md_elas_solve: not available on a slab-decomposition handle" in dom._L.md_last_error(dom._h).decode()


# ---------------------------------------------------------------------------------------------------------------------
# f. a particle without a neighbour
# ---------------------------------------------------------------------------------------------------------------------
def test_a_particle_without_neighbours_stays_at_zero():
    """The relaxed lj500 frame with one particle taken out of its cage and put where nothing is within the cutoff... there is
    no such place at this density, so the particle is the far-apart pair of test_pair_straddling_the_cutoff instead: a bonded
    pair at r = 1.2 and a third particle 4 away from both, cutoff 2.5.  Row and right-hand side of the third are zero."""
    from moleculardynamics.jl_amd import MDDevice
    r = 2.0 ** (1.0 / 6.0)
    x = np.array([[1.0, 1.0, 1.0], [1.0 + r, 1.0, 1.0], [5.0, 5.5, 5.0]])
    z = np.zeros_like(x)
    with MDDevice(3, 3, np.full(3, 9.0), 2.5) as dev:
        dev.set_potential(0, [1.0, 1.0, 2.5])
        dev.upload(x, z, z, np.zeros((3, 3), dtype=np.int32), np.ones(3))
        dev.hess_setup()
        A = dev.elas_affine(fields=True)
        S = dev.elas_solve(1e-10, 9)
    t, k, _ = hr.pair_tk(hr.POT_LJ, [1.0, 1.0, 2.5], x[1, 0] - x[0, 0], 1.0, 1.0)
    print("lone particle: Xi %s, u %s; iterations %s, status %d; CB_xxxx %.6g, N_xxxx %.6g"
          % (A["xi"][:, 2].ravel()[:3], S["u"][:, 2].ravel()[:3], S["iterations"], S["status"], A["born"][0, 0], S["nonaffine"][0, 0]))
    assert np.array_equal(A["xi"][:, 2], np.zeros((6, 3))) and np.array_equal(S["u"][:, 2], np.zeros((6, 3)))
    assert S["converged"] and not S["indefinite"]
    assert np.array_equal(A["xi"][:, 0], -A["xi"][:, 1])                      # the two members: exact negatives
    V = 9.0 ** 3
    cb = float(k) * (x[1, 0] - x[0, 0]) ** 2 / V
    assert abs(A["born"][0, 0] - cb) <= 1e-12 * cb
    assert abs(S["nonaffine"][0, 0] + A["born"][0, 0]) <= 1e-9 * cb          # (tol 1e-10 on a 1 x 1 problem)
