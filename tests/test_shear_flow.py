"""CPU: md_deform_cell and ShearFlow without a device -- the numpy restatement of the map against longdouble and against the
md_set_cell route, the singular-value bounds, the Verlet rows under a general map on the numpy row model of
tests/test_row_audit.py (the honest model passes tests/deform_audit.py, every mistake is reported), ShearFlow's pure update,
the order of run_simulation's device calls on a fake handle, the energy balance of the split scheme on the oracle, and the
plumbing of md_deform_cell / md_deform_state.

The energy balance.  The flow operator maps x -> F x, v -> F^-1 v with F = 1 + dg e_a e_b^T.  To first order in dg,
dU = dg sum_pairs (phi'/r) del_a del_b and dK = -dg sum v_a v_b, so dK + dU = dg V sigma_ab with the stress of the moment in
ShearFlow's convention, sigma = -(sum v v + sum (f/r) del del) / V (tension positive; with the pressure tensor P = -sigma
this is -dg V P_ab).  The residual is second order in dg: halving dg must divide it by 4.  The potential is the XPLOR-switched
LJ (continuous second derivative): with the plain truncated LJ every pair that crosses the cutoff during the map adds a jump
of phi(r_cut), a FIRST-order term that belongs to the delta function in its force, not to the scheme."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import moleculardynamics.jl_amd as md
from moleculardynamics.jl_amd import _lib, deformation
from oracle import oracle
from tests import cell_reference as cr
from tests import deform_audit as da
from tests import deform_reference as dr
from tests import row_audit as ra
from tests.test_row_audit import MODEL_SYSTEMS, _model
from tests.test_sampler_protocol import N, DIM, _FakeDevice, _fake_state
from tests.util import lj_system

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _maps(d):
    """A simple shear, a pure shear and a general F with every entry non-zero."""
    g = np.array([[1.002, 0.0013, -0.0007], [0.0011, 0.9985, 0.0009], [-0.0006, 0.0012, 1.0008]])[:d, :d]
    return dict(simple=md.simple_shear(d, 2e-3), pure=md.pure_shear(d, 2e-3), general=np.ascontiguousarray(g))


# ---------------------------------------------------------------------------------------------------------------------
# 1. the restatement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [2, 3])
def test_the_map_is_row_times_vector_left_to_right(d):
    rng = np.random.default_rng(3)
    a = rng.uniform(-40.0, 40.0, (500, d))
    for name, F in _maps(d).items():
        got = dr.apply(F, a)
        for r in range(d):
            t = np.float64(F[r, 0]) * a[:, 0] + np.float64(F[r, 1]) * a[:, 1]
            if d == 3:
                t = t + np.float64(F[r, 2]) * a[:, 2]
            assert np.array_equal(got[:, r], t), name
        exact = a.astype(np.longdouble) @ F.astype(np.longdouble).T
        bound = 0.5 * d * dr.EPS * np.abs(F).sum(axis=1).max() * np.abs(a).max()
        assert np.abs(got - exact).max() <= bound, name
    U = np.array([[11.0, 2.5, 0.3], [0.0, 10.0, -1.2], [0.0, 0.0, 12.0]])[:d, :d]
    F = _maps(d)["general"]
    assert np.array_equal(dr.cell_after(F, U)[:, 1], dr.apply(F, U[:, 1][None, :])[0])
    assert np.array_equal(dr.cell_after(np.eye(d), U), U)
    # G = F^-1 of a simple shear is exact, and ShearFlow's pure update forms the cell in the same arithmetic
    Fs, Gs, Un = md.shear_flow_update(U, 0.5, 0.02, (0, 1))
    assert np.array_equal(Fs, md.simple_shear(d, 0.5 * 0.02)) and np.array_equal(Gs, md.simple_shear(d, -(0.5 * 0.02)))
    assert np.array_equal(Fs @ Gs, np.eye(d)) and np.array_equal(Un, dr.cell_after(Fs, U))


@pytest.mark.parametrize("d", [2, 3])
def test_singular_bounds_bracket_the_svd(d):
    rng = np.random.default_rng(5)
    for k in range(50):
        M = np.eye(d) + rng.uniform(-0.05, 0.05, (d, d))
        sv = np.linalg.svd(M, compute_uv=False)
        lo, hi = dr.singular_bounds(M)
        assert lo <= sv[-1] <= lo * (1.0 + 1e-9) and hi >= sv[0] >= hi * (1.0 - 1e-9)
    lo, hi = dr.singular_bounds(1.0021 * np.eye(d))
    assert lo <= 1.0021 <= hi and hi - lo <= 4e-12
    # a simple shear: sigma = sqrt(1 + g^2 / 4) -+ g / 2
    g = 2e-3
    lo, hi = dr.singular_bounds(md.simple_shear(d, g))
    assert abs(lo - (np.sqrt(1 + g * g / 4) - g / 2)) <= 2e-12 and abs(hi - (np.sqrt(1 + g * g / 4) + g / 2)) <= 2e-12


@pytest.mark.parametrize("d", [2, 3])
def test_the_map_against_the_affine_remap_within_the_derived_bound(d):
    rng = np.random.default_rng(11)
    U = np.array([[11.0, 2.5, 0.3], [0.0, 10.0, -1.2], [0.0, 0.0, 12.0]])[:d, :d]
    x = cr.cart(rng.uniform(-0.3, 1.3, (2000, d)), U)         # (stored frames are not wrapped)
    img = rng.integers(-3, 4, (2000, d))
    for name, F in _maps(d).items():
        xm, _, Un = dr.deform_frame(x, np.zeros_like(x), U, F)
        xa, ia = cr.affine(x, img, U, Un)
        err = np.abs(cr.unwrapped(xm, img, Un) - cr.unwrapped(xa, ia, Un)).max()
        bound = dr.deformed_bound(U, Un, F, x, ia)
        print("d = %d %s: map against affine remap %.3e (allowed %.3e)" % (d, name, err, bound))
        assert err <= bound
        # the bound is not slack by orders of magnitude: a cell rounded differently by one ulp per entry is outside it
        assert bound <= 200 * dr.EPS * np.abs(U).max() * (1 + np.abs(ia).max())


# ---------------------------------------------------------------------------------------------------------------------
# 2. the rows under a map
# ---------------------------------------------------------------------------------------------------------------------
def _checks(res):
    return {v.check for v in res["violations"]}


def _named_map(dim, kind, size):
    return md.simple_shear(dim, size) if kind == "simple" else md.pure_shear(dim, size)


@pytest.mark.parametrize("kind,size", [("simple", 6e-3), ("simple", -6e-3), ("pure", 3e-3)])
@pytest.mark.parametrize("with_inner", [True, False])
@pytest.mark.parametrize("name", MODEL_SYSTEMS)
def test_mapped_rows_pass_the_audit(name, with_inner, kind, size):
    snap, U, dim, cell, _ = _model(name, with_inner)
    F = _named_map(dim, kind, size)
    mapped, U2, st = dr.deform_snapshot(snap, U, F)
    res = da.check_deformed_rows(mapped, U2, dim, st["M0"], st["M1"], st["rl"], st["inner_skin"])
    print(ra.counts_line("%s/%s %g" % (name, kind, size), res["counts"]), "set aside", res["set_aside"])
    assert res["violations"] == [], [str(v) for v in res["violations"]]
    # the plain audit alone would object, and only about tightness: entries made at up to rl lie at up to sigma_max rl
    plain = _checks(ra.check_rows(mapped, U2, dim))
    assert plain <= {"O4", "I4"} and "O4" in plain and res["set_aside"] >= 1
    info = mapped["info"]
    assert info["skin"] < snap["info"]["skin"] and (not with_inner or info["inner_skin"] < snap["info"]["inner_skin"])
    # for F = mu 1 the deformed audit is the scaled one: nothing is set aside
    from tests import baro_reference as br
    scaled, U3 = br.scale_snapshot(snap, U, 0.998)
    res = da.check_deformed_rows(scaled, U3, dim, 0.998 * np.eye(dim), 0.998 * np.eye(dim), snap["info"]["rl"],
                                 snap["info"]["inner_skin"])
    assert res["violations"] == [] and res["set_aside"] == 0


@pytest.mark.parametrize("name", MODEL_SYSTEMS)
def test_two_maps_a_prune_and_a_map_back(name):
    """M0 accumulates over the calls, M1 starts again at the prune."""
    snap, U, dim, cell, _ = _model(name, True)
    F1, F2 = md.simple_shear(dim, 3e-3), md.pure_shear(dim, 2e-3)
    s1, U1, st = dr.deform_snapshot(snap, U, F1)
    s2, U2, st = dr.deform_snapshot(s1, U1, F2, state=st)
    assert np.array_equal(st["M0"], F2 @ F1) and np.array_equal(st["M1"], F2 @ F1)
    res = da.check_deformed_rows(s2, U2, dim, st["M0"], st["M1"], st["rl"], st["inner_skin"])
    assert res["violations"] == [], [str(v) for v in res["violations"]]
    s3, st = dr.prune_snapshot(s2, U2, st)
    assert np.array_equal(st["M1"], np.eye(dim))
    res = da.check_deformed_rows(s3, U2, dim, st["M0"], st["M1"], st["rl"], st["inner_skin"])
    assert res["violations"] == [], [str(v) for v in res["violations"]]
    s4, U4, st = dr.deform_snapshot(s3, U2, md.simple_shear(dim, -3e-3), state=st)
    res = da.check_deformed_rows(s4, U4, dim, st["M0"], st["M1"], st["rl"], st["inner_skin"])
    assert res["violations"] == [], [str(v) for v in res["violations"]]


# what each mistake must be reported as (among whatever else it breaks).  x0 not mapped: pulled back by M0^-1 the entries
# are those of a frame sheared the other way, wider than the build's radius.  x1 not mapped: it is farther from the mapped
# positions than the inner limit.  sigma_max for sigma_min: the reported radius claims pairs, in the compressed direction,
# that the rows never held.  d1 not scaled: the distance between the two mapped reference frames is under-reported (the map
# is large here so that some displacement near the largest one points along the stretch).  The inner limit not tightened:
# the old inner skin claims inner entries the prune never kept.
SABOTAGES = [("x0_unmapped", 6e-3, "O4"), ("x1_unmapped", 6e-3, "V2"), ("sigma_max_for_min", 6e-3, "O1"),
             ("d1_unscaled", 4e-2, "V2"), ("inner_limit_kept", 6e-3, "I3")]


@pytest.mark.parametrize("variant,size,expected", SABOTAGES)
@pytest.mark.parametrize("kind", ["simple", "pure"])
@pytest.mark.parametrize("name", MODEL_SYSTEMS)
def test_every_mapping_mistake_is_reported(name, kind, variant, size, expected):
    snap, U, dim, cell, _ = _model(name, True)
    F = _named_map(dim, kind, size)
    mapped, U2, st = dr.deform_snapshot(snap, U, F, variant=variant)
    res = da.check_deformed_rows(mapped, U2, dim, st["M0"], st["M1"], st["rl"], st["inner_skin"])
    got = _checks(res)
    print("%s %s %s: %s" % (name, kind, variant, sorted(got)))
    assert expected in got
    if variant == "d1_unscaled":
        assert any(v.check == "V2" and "reported d1" in str(v) for v in res["violations"])


@pytest.mark.parametrize("kind", ["simple", "pure"])
@pytest.mark.parametrize("name", MODEL_SYSTEMS)
def test_m1_not_reset_at_a_prune_is_reported(name, kind):
    """A map, a prune, the map back.  With M1 carried across the prune the product is the identity and the full inner skin
    is reported for inner rows that were made in the mapped frame and have now been compressed along one direction: the
    audit finds outer entries within the claimed inner radius that the inner rows do not hold."""
    snap, U, dim, cell, _ = _model(name, True)
    F = _named_map(dim, kind, 6e-3)
    outcomes = {}
    for variant in (None, "m1_not_reset"):
        s1, U1, st = dr.deform_snapshot(snap, U, F)
        s2, st = dr.prune_snapshot(s1, U1, st, variant=variant)
        s3, U3, st = dr.deform_snapshot(s2, U1, np.linalg.inv(F), state=st)
        outcomes[variant] = _checks(da.check_deformed_rows(s3, U3, dim, st["M0"], st["M1"], st["rl"], st["inner_skin"]))
    print(name, kind, {k: sorted(v) for k, v in outcomes.items()})
    assert outcomes[None] == set() and "I3" in outcomes["m1_not_reset"]


# ---------------------------------------------------------------------------------------------------------------------
# 3. ShearFlow on a fake handle
# ---------------------------------------------------------------------------------------------------------------------
class _FakeShearDevice(_FakeDevice):
    elas_components = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))

    def __init__(self):
        super().__init__()
        self.unitcell = np.diag([2.0, 2.0, 2.0])

    def deform_cell(self, F, G=None):
        self._log("deform_cell", np.array(F), None if G is None else np.array(G))
        self.unitcell = dr.cell_after(F, self.unitcell)
        return 1

    def set_cell(self, unitcell, mode=0):
        self._log("set_cell", np.array(unitcell), int(mode))
        self.unitcell = np.array(unitcell)

    def compute_forces(self):
        self._log("compute_forces")
        return 0.25, 0.5

    def kinetic(self):
        self._log("kinetic")
        return 2.0

    def stress_tensor(self):
        self._log("stress_tensor")
        return np.array([1.0, 1.0, 1.0, 0.125, 0.0, 0.0]), np.array([3.0, 3.0, 3.0, -0.625, 0.0, 0.0])


def _fake_shear_state():
    state, _ = _fake_state()
    dev = _FakeShearDevice()
    state.system.device = dev
    return state, dev


def test_constructor_refusals_and_columns():
    for bad in (dict(rate=float("nan")), dict(every=0), dict(stress_every=0), dict(plane=(1, 1)), dict(plane=(-1, 0))):
        kw = dict(rate=0.5)
        kw.update(bad)
        with pytest.raises(ValueError):
            md.ShearFlow(**kw)
    assert md.shear_columns() == ["step", "strain", "tilt", "sigma_ab", "pressure", "K_ab", "rows_kept", "flips"]
    doc = md.ShearFlow.__doc__
    assert "FIRST ORDER" in doc and "every=1 is the plain one-step splitting" in doc


def test_call_order_with_shear(tmp_path):
    total, f = 40, 7
    state, dev = _fake_shear_state()
    U0 = np.array(state.unitcell)
    params = md.Parameters(1.0, N, 0.002, md.LennardJones())
    shear = md.ShearFlow(7.0, every=5, stress_every=2)             # (a rate at which the fake's cell flips within 40 steps)
    swap = md.SwapMonteCarlo(10, 2, ktemp=0.7, seed=1)
    boo = md.BondOrder(0.9, order=6, every=1, nbins=5)
    out = str(tmp_path / "out")
    with np.errstate(all="ignore"):
        md.run_simulation(state, params, md.NVE(), total, f, out, bond_order=boo, swap=swap, shear=shear)
    stops = list(range(4, total, 5))
    assert [st for st, m, _ in dev.trace if m == "deform_cell"] == stops and dev.setups.count("stress_setup") == 1
    by_step = {}
    for st, m, _ in dev.trace:
        by_step.setdefault(st, []).append(m)
    flips = 0
    for k, st in enumerate(stops):
        ms = by_step[st]
        i = ms.index("deform_cell")
        tail = [m for m in ms[i + 1:] if m != "snapshot_begin"]
        assert tail in (["compute_forces", "kinetic"], ["set_cell", "compute_forces", "kinetic"])   # map, flip, forces, K
        flips += tail[0] == "set_cell"
        assert "swap_rounds" not in ms[i:] and "boo_sample" not in ms[i:]        # after every sampler and after swap
        assert ((st + 1) % 10 == 0) == ("swap_rounds" in ms[:i])
        assert "snapshot_begin" not in ms[:i]                                    # before the frame export of that step
        # the stress of the moment is read before the flow, at every second coupling
        assert (ms[:i][-2:] == ["stress_sample", "stress_tensor"]) == (k % 2 == 0)
    assert by_step[14] == ["boo_sample", "stress_sample", "stress_tensor", "deform_cell", "compute_forces", "kinetic", "snapshot_begin"]
    # every F and G: the simple shear of rate * every * dt and its exact inverse; the host's cell follows
    dg = 7.0 * (5 * 0.002)
    U = U0
    for (_, m, a), rec in zip([t for t in dev.trace if t[1] == "deform_cell"], shear.records):
        assert np.array_equal(a[0], md.simple_shear(3, dg)) and np.array_equal(a[1], md.simple_shear(3, -dg))
        U = dr.cell_after(a[0], U)
        if rec["flips"]:
            U, M = md.gauss_reduce(U)
        assert rec["tilt"] == U[0, 1] and rec["rows_kept"] == 1
    assert flips == 1 and sum(r["flips"] for r in shear.records) == 1      # the tilt passes half the edge once: 8 * 0.07 * 2 > 1
    assert np.array_equal(state.unitcell, U) and state.system.unitcell is state.unitcell
    assert np.array_equal(dev.unitcell, U) and abs(U[0, 1]) <= 1.0
    strains = [r["strain"] for r in shear.records]
    assert np.all(np.diff(strains) > 0) and abs(strains[-1] - 8 * dg) < 1e-14
    # sigma = -(kin + vir) / V, the pressure -trace / d, K_ab the kinetic part; nan without a reading
    V = 8.0
    for k, r in enumerate(shear.records):
        if k % 2 == 0:
            # (the loop's volume is numpy's determinant of the cell: 8 to rounding)
            assert abs(r["sigma_ab"] + (0.125 - 0.625) / V) < 1e-15 and abs(r["K_ab"] + 0.125 / V) < 1e-15
            assert abs(r["pressure"] - (1.0 + 3.0) / V) < 1e-15
        else:
            assert np.isnan(r["sigma_ab"]) and np.isnan(r["pressure"]) and np.isnan(r["K_ab"])
    assert shear.n_stress == 4 and abs(shear.mean_stress() - 0.5 / V) < 1e-15 and shear.viscosity() == shear.mean_stress() / 7.0
    lines = open(os.path.join(out, "shear.txt")).read().splitlines()
    assert lines[0] == "# " + " ".join(md.shear_columns()) and len(lines) == 1 + len(stops)
    assert [int(l.split()[0]) for l in lines[1:]] == stops and lines[2].split()[3] == "nan"
    assert float(lines[-1].split()[2]) == shear.records[-1]["tilt"]
    # U, W, K of the new cell go on to the loop: the thermo line after a coupling shows the fake's K = 2
    thermo = [l.split() for l in open(os.path.join(out, "thermo.txt")).read().splitlines()[1:]]
    by = {int(t[0]): float(t[2]) for t in thermo}
    assert abs(by[14] - 2.0 * 2.0 / state.nf) < 1e-6 and abs(by[7] - 2.0 * 1.0 / state.nf) < 1e-6
    # every frame carries the cell of its own moment
    tl = open(os.path.join(out, "trajectory.xyz")).read().splitlines()
    at = [int(tl[i + 1]) for i, l in enumerate(tl) if l == "ITEM: TIMESTEP"]
    assert at == list(range(0, total, f))
    heads = [tl[i + 1] for i, l in enumerate(tl) if l.startswith("ITEM: BOX BOUNDS")]
    assert len(set(heads)) >= 5


def test_refusals_before_anything_is_opened(tmp_path):
    params = md.Parameters(1.0, N, 0.002, md.LennardJones())
    kw = dict(lags=[1], origin_every=1)
    combos = dict(dynamics=md.SelfDynamics(**kw), sq=md.StructureFactor(4.5), currents=md.CurrentCorrelations(4.5, **kw),
                  four_point=md.FourPoint(0.3, **kw), cage=md.CageDynamics(0.9, **kw), stress=md.StressTensor(2),
                  barostat=md.StochasticCellRescaling(0.5, 1.0, 0.1))
    for name, smp in combos.items():
        state, dev = _fake_shear_state()
        out = tmp_path / name
        with pytest.raises(ValueError, match="shear= cannot be combined with %s=" % name) as e:
            md.run_simulation(state, params, md.NVT(1.0, 0.1), 5, 2, str(out), shear=md.ShearFlow(0.5), **{name: smp})
        assert not out.exists() and dev.trace == [] and dev.setups == []
        if name == "stress":
            assert "left for later" in str(e.value)
    state, dev = _fake_shear_state()
    out = tmp_path / "brownian"
    with pytest.raises(ValueError, match="Brownian"):
        md.run_simulation(state, params, md.Brownian(1.0), 5, 2, str(out), shear=md.ShearFlow(0.5))
    assert not out.exists() and dev.trace == []
    # the samplers that do not depend on the cell go with it
    state, dev = _fake_shear_state()
    with np.errstate(all="ignore"):
        md.run_simulation(state, params, md.NVE(), 10, 5, str(tmp_path / "ok"), shear=md.ShearFlow(0.5, every=5),
                          rdf=md.RadialDistribution(1.0, 4), bond_order=md.BondOrder(0.9, order=6, every=1, nbins=5),
                          clusters=md.ClusterAnalysis(0.9))
    assert os.path.isfile(tmp_path / "ok" / "shear.txt")


def test_without_shear_the_run_is_the_keywordless_one(tmp_path):
    outs = []
    for kw in ({}, dict(shear=None)):
        state, dev = _fake_shear_state()
        params = md.Parameters(1.0, N, 0.002, md.LennardJones())
        out = str(tmp_path / ("a" if not kw else "b"))
        with np.errstate(all="ignore"):
            md.run_simulation(state, params, md.NVE(), 20, 3, out, stress=md.StressTensor(4), **kw)
        outs.append((dev.trace, dev.segments, {f: open(os.path.join(out, f), "rb").read() for f in sorted(os.listdir(out))}))
    assert outs[0] == outs[1] and "shear.txt" not in outs[0][2]


# ---------------------------------------------------------------------------------------------------------------------
# 4. the energy balance of the split scheme
# ---------------------------------------------------------------------------------------------------------------------
def test_energy_balance_of_the_flow_operator_is_second_order():
    s = lj_system(256)
    kind, params, cutoff = oracle.POT_LJ_MODIFIED, [1.0, 1.0, 2.5, 2.0, 2.0], 2.5
    pot = oracle.make_pot(kind, params)
    U = np.diag(s["box"]).copy()
    U[0, 1] = 0.3                                             # (a general cell: oracle.set_cell's route)
    x, v, diam = s["x"], s["v"], s["diam"]
    V = abs(float(np.linalg.det(U)))

    def energy(xx, vv, cell):
        with oracle.set_cell(cell):
            u = oracle.forces_brute(xx, np.ones(3), cutoff, pot, diam)[1]
        return float(0.5 * (vv.astype(np.longdouble) ** 2).sum()) + u

    sig_conf = cr.stress_of(x, U, cutoff, kind, params, diam)[3]          # xy, tension positive, per volume
    sigma = sig_conf - float((v[:, 0] * v[:, 1]).sum()) / V
    e0 = energy(x, v, U)
    res = []
    for dg in (2e-3, 1e-3):
        F, G, Un = md.shear_flow_update(U, dg, 1.0, (0, 1))
        xm, vm, Um = dr.deform_frame(x, v, U, F, G)
        assert np.array_equal(Um, Un)
        de = energy(xm, vm, Um) - e0
        res.append(de - dg * V * sigma)
        print("dg = %g: dK + dU = %.9e, dg V sigma_ab = %.9e, residual %.3e" % (dg, de, dg * V * sigma, res[-1]))
    ratio = res[0] / res[1]
    print("residual ratio %.4f (second order: 4)" % ratio)
    # the first-order term is matched: the residual is small against it, and it scales as dg^2 (the cubic term moves the
    # ratio by its relative size at dg = 2e-3, a few parts in a thousand; rounding of U ~ 1e3 is 1e-13 against 1e-3)
    assert abs(res[0]) < 0.05 * abs(2e-3 * V * sigma) and abs(ratio - 4.0) < 0.1


# ---------------------------------------------------------------------------------------------------------------------
# 5. plumbing
# ---------------------------------------------------------------------------------------------------------------------
def test_symbols_bindings_header_makefile_and_julia():
    assert "md_deform_cell" in _lib.EXPORTS and "md_deform_state" in _lib.EXPORTS
    for name in ("ShearFlow", "shear_flow_update", "shear_columns"):
        assert name in md.__all__ and getattr(md, name) is getattr(deformation, name)
    assert callable(md.MDDevice.deform_cell) and callable(md.MDDevice.deform_state)
    header = open(os.path.join(ROOT, "include", "mdhip.h")).read()
    assert re.search(r"int md_deform_cell\(md_ctx \*ctx, const double \*F, const double \*G, int \*rows_kept\);", header)
    assert re.search(r"int md_deform_state\(md_ctx \*ctx, double \*m0, double \*m1, double \*sig\);", header)
    assert "fixes its cell at initialisation" in header
    make = open(os.path.join(ROOT, "moleculardynamics", "jl_amd", "csrc", "Makefile")).read()
    rule = [l for l in make.splitlines() if l.startswith("libmdhip.so:")][0]
    assert "md_deform.hpp" in rule.split()
    kernel = open(os.path.join(ROOT, "moleculardynamics", "jl_amd", "csrc", "md_deform.hpp")).read()
    assert "k_deform_cell" in kernel and "contract(off)" in kernel and "__shared__" not in kernel
    assert "atomicAdd" not in kernel
    lib = _lib.load()
    dp = C.POINTER(C.c_double)
    assert lib.md_deform_cell.argtypes == [C.c_void_p, dp, dp, C.POINTER(C.c_int)] and lib.md_deform_cell.restype is C.c_int
    assert lib.md_deform_state.argtypes == [C.c_void_p, dp, dp, dp]
    julia = open(os.path.join(ROOT, "julia", "MDHip.jl")).read()
    assert "(:md_deform_cell, LIB)" in julia and "(:md_deform_state, LIB)" in julia
    assert re.search(r"^function deform_cell!\(", julia, flags=re.M) and re.search(r"^function deform_state\(", julia, flags=re.M)
    assert "deform_cell!" in julia.split("const LIB")[0] and "deform_state" in julia.split("const LIB")[0]
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert re.search(r"^## 27\.", design, flags=re.M) and "md_deform_cell" in design and "first order" in design
    assert os.path.isfile(os.path.join(ROOT, "profiles", "deform_resource_usage.txt"))
    # the slab refusal is one line ahead of every state change (a slab handle needs several ranks)
    src = open(os.path.join(ROOT, "moleculardynamics", "jl_amd", "csrc", "mdhip.hip")).read()
    body = src[src.index("int md_deform_cell(md_ctx *ctx, const double *F, const double *G, int *rows_kept)"):]
    assert body.index("md_deform_cell: not available on a slab-decomposition handle") < body.index("require_state(ctx")


def test_a_null_handle_is_refused():
    lib = _lib.load()
    kept = C.c_int(7)
    F = (C.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    assert lib.md_deform_cell(None, F, None, C.byref(kept)) != 0
    assert b"null handle" in lib.md_last_error(None)
    assert lib.md_deform_state(None, F, None, None) != 0
