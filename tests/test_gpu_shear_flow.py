"""-m gpu: md_deform_cell, md_deform_state and the ShearFlow loop on the device, against tests/deform_reference.py, the row
audit of tests/deform_audit.py, md_set_cell on a twin handle, the oracle's pair loop and the oracle's step loop.

Shapes, as tests/test_gpu_barostat.py: LJ at N = 4000 (15 full tiles + 160), rho = 0.897, cutoff 2.5; the 2-D polydisperse
golden system (N = 1200, per-particle diameters); LJ at N = 1000 in a sheared cell (3 full tiles + 232, a general cell).
A handle in a diagonal cell is first made general by one small shear (which retires its rows: the transition test) wherever a
test needs rows that survive a shear.

Tolerances.  The stored frame, x0, x1 and v after a map: bit for bit against deform_reference.  Against
md_set_cell(F U, AFFINE) on a twin: deform_reference.deformed_bound.  Forces, U, W against the oracle or a fresh handle:
tests/test_gpu_parity.py's (|dF| <= 1e-11 max(1, |F|), U and W relative 1e-12).  Segments of the loop: tests/step_audit.py's.
Row audits: deform_audit.check_deformed_rows with the figures md_list_rows reports, the maps md_deform_state reports (which
must be the product of the test's own F's) and the configured radius and inner skin; knife-edge bands capped as in
tests/test_gpu_row_audit.py.  Singular-value bounds: within a relative 1e-9 of numpy's svd, on the safe side.

The sign test (MI355X, LJ N = 4000, rho = 0.897, T = 0.7, rate 0.5, every 10, dt 0.002; second half of one unit of strain,
50 readings in 5 blocks): the figures are printed by the test and recorded in DESIGN.md section 27."""
import os
import types

import numpy as np
import pytest

from oracle import oracle
from tests import cell_reference as cr
from tests import deform_audit as da
from tests import deform_reference as dr
from tests import row_audit as ra
from tests import step_audit as sa
from tests.test_gpu_barostat import CASES, DT, _brute, _device, _parity, _read, _started, _state, _untouched_checker, case

pytestmark = pytest.mark.gpu


def _maps(d):
    g = np.array([[1.002, 0.0013, -0.0007], [0.0011, 0.9985, 0.0009], [-0.0006, 0.0012, 1.0008]])[:d, :d]
    import moleculardynamics.jl_amd as md
    return dict(simple=md.simple_shear(d, 2e-3), pure=md.pure_shear(d, 2e-3), general=np.ascontiguousarray(g))


def _product(A, B):
    """A B with every product and sum rounded, k ascending: md_deform_state's own order."""
    d = A.shape[0]
    out = np.zeros((d, d))
    for r in range(d):
        for c in range(d):
            v = np.float64(0.0)
            for k in range(d):
                v = v + np.float64(A[r, k]) * np.float64(B[k, c])
            out[r, c] = v
    return out


def _make_general(dev, c):
    """One small shear of a diagonal cell: the rows retire (diagonal -> general), the next evaluation builds; then 30 steps."""
    import moleculardynamics.jl_amd as md
    if cr.is_general(dev.unitcell):
        return 0
    d = c["system"]["dim"]
    builds = dev.stats()["rebuilds"]
    assert dev.deform_cell(md.simple_shear(d, 1e-3), md.simple_shear(d, -1e-3)) == 0
    assert not dev.list_rows(0)["info"]["list_valid"]
    dev.compute_forces()
    assert dev.stats()["rebuilds"] == builds + 1
    dev.run(30, DT)
    return 1


def _audit(name, dev, c, conf, M0=None, M1=None):
    """check_deformed_rows on the handle's rows; M0, M1 default to what the handle reports."""
    snap = ra.snapshot_of(dev)
    dim = c["system"]["dim"]
    m0, m1, sig = dev.deform_state()
    if snap["info"]["inner_valid"] and sig[2] == 1.0 and sig[3] == 1.0:
        conf["inner_skin"] = snap["info"]["inner_skin"]        # (fresh inner rows report the configured inner skin)
    res = da.check_deformed_rows(snap, dev.unitcell, dim, m0 if M0 is None else M0, m1 if M1 is None else M1,
                                 conf["rl"], conf["inner_skin"] or 0.0)
    print(ra.counts_line(name, res["counts"]), "set aside %d" % res["set_aside"])
    assert res["violations"] == [], (name, [str(v) for v in res["violations"]])
    k = res["counts"]
    assert k["band_rl"] + k["band_rin"] + k["band_rc"] <= sa.MAX_EXCLUDED, name
    return snap


def _conf(dev):
    """The configured list radius and inner skin, read while nothing has been mapped since the build."""
    info = dev.list_rows(0)["info"]
    m0, m1, sig = dev.deform_state()
    assert np.array_equal(m0, np.eye(dev.dim)) and tuple(sig) == (1.0, 1.0, 1.0, 1.0)
    return dict(rl=info["rl"], skin=info["skin"], inner_skin=info["inner_skin"] if info["inner_valid"] else None, rc=info["rc"])


def _check_sig(M, lo, hi):
    sv = np.linalg.svd(M, compute_uv=False)
    assert lo <= sv[-1] and sv[-1] - lo <= 1e-9 * sv[-1], (lo, sv)
    assert hi >= sv[0] and hi - sv[0] <= 1e-9 * sv[0], (hi, sv)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the frame
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["simple", "pure", "general"])
@pytest.mark.parametrize("name", CASES)
def test_frame_bit_for_bit_and_against_set_cell(name, which):
    c = case(name)
    s = c["system"]
    d = s["dim"]
    F = _maps(d)[which]
    G = np.linalg.inv(F)
    with _started(c) as dev, _device(c) as twin:
        _make_general(dev, c)
        U0 = np.array(dev.unitcell)
        # (a) live rows, G = F^-1: the stored frame, both reference frames and the velocities, bit for bit; images untouched
        before = dev.list_rows(0)
        x_b, v_b, _, img_b = dev.download()
        kept = dev.deform_cell(F, G)
        after = dev.list_rows(0)
        x_a, v_a, _, img_a = dev.download()
        U1 = dr.cell_after(F, U0)
        assert kept == 1 and np.array_equal(dev.unitcell, U1)
        keys = ("pos", "x0") + (("x1",) if after["info"]["inner_valid"] else ())
        for key in keys:
            assert np.array_equal(after[key], dr.apply(F, before[key])), (name, key)
        assert np.array_equal(v_a, dr.apply(G, v_b))
        un_b, un_a = cr.unwrapped(x_b, img_b, U0), cr.unwrapped(x_a, img_a, U1)
        bound = dr.deformed_bound(U0, U1, F, before["pos"], img_a) + cr.unwrapped_bound([U0, U1], [img_b, img_a])
        assert np.abs(un_a - un_b @ F.astype(np.longdouble).T).max() <= bound
        # (b) G = NULL on a frame the handle stores exactly as a download shows it: x, v, images and cell against the
        # restatement, and against md_set_cell(F U, AFFINE) on the twin within the derived bound
        z = np.zeros_like(x_b)
        for h in (dev, twin):
            h.set_cell(U0)
            h.upload(x_b, v_b, z, img_b, s["diam"])
        dev.deform_cell(F)
        twin.set_cell(U1, twin.CELL_AFFINE)
        xs, vs, _, ims = dev.download()
        xr, vr, Ur = dr.deform_frame(x_b, v_b, U0, F, None)
        xw, iw = cr.export_wrap(xr, img_b, Ur)
        assert np.array_equal(Ur, U1) and np.array_equal(dev.unitcell, U1) and np.array_equal(twin.unitcell, U1)
        assert np.array_equal(xs, xw) and np.array_equal(ims, iw.astype(np.int32)) and np.array_equal(vs, v_b)
        xt, _, _, imt = twin.download()
        err = np.abs(cr.unwrapped(xs, ims, U1) - cr.unwrapped(xt, imt, U1)).max()
        bound = dr.deformed_bound(U0, U1, F, x_b, ims)
        print("%s %s: map against set_cell(AFFINE): |d(x + U img)| %.3e (allowed %.3e)" % (name, which, err, bound))
        assert err <= bound
        # forces, U, W of the mapped frame against a fresh handle in the new cell
        u, w = dev.compute_forces()
        x, v, f, img = dev.download()
        with _device(c, cell=U1) as fresh:
            fresh.upload(x, v, z, img, s["diam"])
            uf, wf = fresh.compute_forces()
            ff = fresh.download()[2]
        _parity("%s %s against a fresh handle" % (name, which), (f, u, w), (ff, uf, wf))


# ---------------------------------------------------------------------------------------------------------------------
# 2. the rows are kept and stay right; md_deform_state
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["default", "no_fused_build"])
@pytest.mark.parametrize("name", CASES)
def test_rows_kept_through_two_shears(monkeypatch, name, path):
    import moleculardynamics.jl_amd as md
    if path == "no_fused_build":
        monkeypatch.setenv("MDHIP_NO_FUSED_BUILD", "1")
    c = case(name)
    s = c["system"]
    d = s["dim"]
    with _started(c) as dev:
        transitions = _make_general(dev, c)                    # diagonal -> general retires once ...
        if not dev.list_rows(0)["info"]["inner_valid"]:
            dev.run(2, DT)
        conf = _conf(dev)
        snap = _audit("%s/%s before" % (name, path), dev, c, conf)
        assert snap["info"]["list_valid"] and snap["info"]["tiled"]
        had_inner = bool(snap["info"]["inner_valid"])
        stats = dev.stats()
        M0, M1 = np.eye(d), np.eye(d)
        for g in (2e-3, -2e-3, 2e-3):
            F = md.simple_shear(d, g)
            assert dev.deform_cell(F, md.simple_shear(d, -g)) == 1          # ... and keeps afterwards
            M0, M1 = _product(F, M0), _product(F, M1)
            m0, m1, sig = dev.deform_state()
            sn = _audit("%s/%s after %g" % (name, path, g), dev, c, conf, M0, M1)
            assert np.array_equal(m0, M0)
            _check_sig(M0, sig[0], sig[1])
            assert (sn["info"]["rl"], sn["info"]["skin"]) == (sig[0] * conf["rl"], sig[0] * conf["rl"] - conf["rc"])
            if sn["info"]["inner_valid"]:
                assert np.array_equal(m1, M1)
                _check_sig(M1, sig[2], sig[3])
                assert sn["info"]["inner_skin"] == sig[2] * (conf["rc"] + conf["inner_skin"]) - conf["rc"]
            else:
                assert np.array_equal(m1, np.eye(d)) and sig[2] == sig[3] == 1.0
        u, w = dev.compute_forces()
        assert dev.stats()["rebuilds"] == stats["rebuilds"]    # the evaluation walked the kept rows
        _audit("%s/%s after compute_forces" % (name, path), dev, c, conf, M0)
        x, v, f, img = dev.download()
        with _device(c, cell=dev.unitcell) as fresh:
            fresh.upload(x, v, np.zeros_like(x), img, s["diam"])
            uf, wf = fresh.compute_forces()
            ff = fresh.download()[2]
        _parity("%s/%s kept rows against a fresh handle" % (name, path), (f, u, w), (ff, uf, wf))
        dev.run(20, DT)
        after = dev.stats()
        m0, m1, sig = dev.deform_state()
        if after["rebuilds"] == stats["rebuilds"]:
            assert np.array_equal(m0, M0)
            if after["prunes"] > stats["prunes"]:
                assert np.array_equal(m1, np.eye(d)) and sig[2] == sig[3] == 1.0   # the prune started M1 again
        else:
            assert np.array_equal(m0, np.eye(d)) and tuple(sig) == (1.0, 1.0, 1.0, 1.0)
        _audit("%s/%s after 20 further steps" % (name, path), dev, c, conf)
        x, _, f, _ = dev.download()
        fr = _brute(c, x, dev.unitcell)[0]
        assert np.abs(f - fr).max() <= 1e-11 * max(1.0, np.abs(fr).max())
        print("%s/%s: transitions %d, inner rows at the first shear: %s, builds %d -> %d, prunes %d -> %d"
              % (name, path, transitions, had_inner, stats["rebuilds"], after["rebuilds"], stats["prunes"], after["prunes"]))


# ---------------------------------------------------------------------------------------------------------------------
# 3. the budget's edge, and retirement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", ["below", "above"])
def test_budget_edge(side):
    """The shear is chosen from the snapshot so that skin_eff / 2 lands a relative 1e-6 below (above) the largest
    displacement from the mapped x0 as it will be after the map: rows retired and the next evaluation builds (kept, none)."""
    import moleculardynamics.jl_amd as md
    c = case("sheared1000")
    with _started(c) as dev:
        snap = ra.snapshot_of(dev)
        for _ in range(10):
            if float(np.sqrt(((snap["pos"] - snap["x0"]) ** 2).sum(axis=1)).max()) >= 0.23:
                break
            dev.run(3, DT)
            snap = ra.snapshot_of(dev)
        info = snap["info"]
        rc, rl = info["rc"], info["rl"]
        disp = snap["pos"] - snap["x0"]
        factor = 1.0 - 1e-6 if side == "below" else 1.0 + 1e-6

        def gap(g):
            F = md.simple_shear(3, g)
            D = float(np.sqrt((dr.apply(F, disp) ** 2).sum(axis=1)).max())
            return 0.5 * (dr.singular_bounds(F)[0] * rl - rc) - D * factor

        lo, hi = 0.0, 0.2
        assert gap(lo) > 0.0 > gap(hi)
        for _ in range(80):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if gap(mid) > 0.0 else (lo, mid)
        g = lo
        F = md.simple_shear(3, g)
        se = dr.singular_bounds(F)[0] * rl - rc
        D = float(np.sqrt((dr.apply(F, disp) ** 2).sum(axis=1)).max())
        assert se >= (2.0 / 3.0) * info["skin"] and abs(0.5 * se / D - factor) < 1e-9, (g, se, D)   # (above the floor)
        builds = dev.stats()["rebuilds"]
        kept = dev.deform_cell(F, md.simple_shear(3, -g))
        after = dev.list_rows(0)["info"]
        print("budget edge (%s): shear %.9f, skin_eff / 2 = %.9f, largest displacement %.9f, kept %d" % (side, g, 0.5 * se, D, kept))
        assert kept == (0 if side == "below" else 1) and after["list_valid"] == kept
        dev.compute_forces()
        assert dev.stats()["rebuilds"] == builds + (1 if side == "below" else 0)
        x, _, f, _ = dev.download()
        fr = _brute(c, x, dev.unitcell)[0]
        assert np.abs(f - fr).max() <= 1e-11 * max(1.0, np.abs(fr).max())


@pytest.mark.parametrize("name", CASES)
def test_retirement(name):
    import moleculardynamics.jl_amd as md
    c = case(name)
    d = c["system"]["dim"]
    with _started(c) as dev:
        _make_general(dev, c)
        assert dev.deform_cell(md.simple_shear(d, 0.2), md.simple_shear(d, -0.2)) == 0
        info = dev.list_rows(0)["info"]
        assert not info["list_valid"] and not info["inner_valid"]
        m0, m1, sig = dev.deform_state()
        assert np.array_equal(m0, np.eye(d)) and tuple(sig) == (1.0, 1.0, 1.0, 1.0)
        u, w = dev.compute_forces()
        x, _, f, _ = dev.download()
        fr, ur, wr, pairs = _brute(c, x, dev.unitcell)
        assert np.array_equal(dev.neighbor_pairs(), pairs)
        _parity("%s retired at a shear of 0.2" % name, (f, u, w), (fr, ur, wr))
        full = dev.list_rows(0)["info"]
        assert full["list_valid"] and full["rl"] == full["rc"] + full["skin"]


@pytest.mark.parametrize("kind", ["skin_0", "user_potential", "no_tiles"])
def test_handles_without_two_level_rows_are_mapped_and_build_again(monkeypatch, kind):
    from moleculardynamics.jl_amd import MDDevice
    from tests.test_gpu_parity import USER_LJ_SRC
    if kind == "no_tiles":
        monkeypatch.setenv("MDHIP_NO_TILES", "1")
    c = case("lj4000")
    s = c["system"]
    with MDDevice(s["dim"], s["n"], c["cell"], c["cutoff"]) as dev:
        if kind == "user_potential":
            dev.set_potential_source(USER_LJ_SRC, "user_lj", [1.0, 2.5])
        else:
            dev.set_potential(c["kind"], c["params"])
        if kind == "skin_0":
            dev.set_skin(0.0)
        dev.upload(s["x"], s["v"], np.zeros_like(s["x"]), s["img"], s["diam"])
        dev.compute_forces()
        dev.run(10, DT)
        stored = dev.list_rows(0)["pos"]
        v_b = dev.download()[1]
        for which in ("general", "simple"):
            F = _maps(3)[which]
            G = np.linalg.inv(F)
            assert dev.deform_cell(F, G) == 0
            info = dev.list_rows(0)
            assert not info["info"]["list_valid"]
            stored, v_b = dr.apply(F, stored), dr.apply(G, v_b)
            assert np.array_equal(info["pos"], stored) and np.array_equal(dev.download()[1], v_b)
            u, w = dev.compute_forces()
            x, _, f, _ = dev.download()
            fr, ur, wr, pairs = _brute(c, x, dev.unitcell)
            assert np.array_equal(dev.neighbor_pairs(), pairs)
            _parity("%s mapped by %s" % (kind, which), (f, u, w), (fr, ur, wr))
            stored = dev.list_rows(0)["pos"]
        dev.run(10, DT)
        x, _, f, _ = dev.download()
        fr = _brute(c, x, dev.unitcell)[0]
        assert np.abs(f - fr).max() <= 1e-11 * max(1.0, np.abs(fr).max())


# ---------------------------------------------------------------------------------------------------------------------
# 4. refusals leave the handle untouched
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_untouched():
    """Every refusal of md_deform_cell but two: the slab one needs several ranks (tests/test_shear_flow.py reads the host
    code), and state_invalid is set only by a device failure, which no test provokes."""
    from moleculardynamics.jl_amd import MdhipError
    c = case("sheared1000")
    U0 = c["cell"]
    perp = cr.face_distances(U0).min()
    I = np.eye(3)
    with _started(c) as dev:
        untouched = _untouched_checker(dev, U0)
        bad = I.copy()
        for val, G, why in ((float("nan"), None, "F must be finite"), (float("inf"), None, "F must be finite")):
            bad[0, 1] = val
            with pytest.raises(MdhipError, match=why):
                dev.deform_cell(bad, G)
            untouched(why)
        for val in (float("nan"), float("inf")):
            Gb = I.copy()
            Gb[1, 2] = val
            with pytest.raises(MdhipError, match="G must be finite"):
                dev.deform_cell(I, Gb)
            untouched("G")
        for Fb in (np.diag([-1.0, 1.0, 1.0]), np.zeros((3, 3)), np.array([[1.0, 2.0, 0.0], [0.5, 1.0, 0.0], [0.0, 0.0, 1.0]])):
            with pytest.raises(MdhipError, match="det F"):
                dev.deform_cell(Fb)
            untouched("det F")
        too_small = 3.0 * c["cutoff"] / perp * 0.999
        with pytest.raises(MdhipError, match="face distance"):
            dev.deform_cell(too_small * I)
        untouched("face distance")
        dev.snapshot_begin()
        with pytest.raises(MdhipError, match="in flight"):
            dev.deform_cell(_maps(3)["simple"])
        dev.snapshot_end()
        untouched("frame in flight")
    small = 3.0 * 3.2 / perp * 0.999
    assert small * perp > 3.0 * c["cutoff"]
    for setup, who in ((lambda h: h.rdf_setup(3.2, 16), "md_rdf_"), (lambda h: h.mpc_setup(3.2, 16, weights=[1.0], tmax=1.0), "md_mpc_")):
        with _started(c) as dev:
            setup(dev)
            untouched = _untouched_checker(dev, U0)
            with pytest.raises(MdhipError, match="r_max"):
                dev.deform_cell(small * I)
            untouched(who + " r_max")
            assert dev.deform_cell(_maps(3)["simple"]) == 1        # (with room for r_max the sampler is no obstacle)
    e1 = np.array([[1.0, 0.0, 0.0]])
    n1 = np.array([[1, 0, 0]], dtype=np.int32)
    for setup, who in ((lambda h: h.dyn_setup(1, 1), "md_dyn_"), (lambda h: h.sq_setup(n1), "md_sq_"),
                       (lambda h: h.cur_setup(n1, e1), "md_cur_"), (lambda h: h.chi4_setup(0.3), "md_chi4_"),
                       (lambda h: h.cage_setup(1, 1, 1.5), "md_cage_")):
        with _started(c) as dev:
            setup(dev)
            untouched = _untouched_checker(dev, U0)
            with pytest.raises(MdhipError, match="the %s sampler" % who):
                dev.deform_cell(_maps(3)["simple"])
            untouched(who)


# ---------------------------------------------------------------------------------------------------------------------
# 5. the loop
# ---------------------------------------------------------------------------------------------------------------------
class _AuditingDevice:
    """An MDDevice seen through run_simulation's eyes: every segment is restated by oracle.run(use_cells=False) under
    oracle.set_cell of the moment from the handle's own downloaded state, every F and G is recomputed on the host and the
    mapped frame compared bit for bit."""

    def __init__(self, dev, c, shear):
        self._d, self._c, self._shear = dev, c, shear
        self.worst = dict(x=0.0, v=0.0, F=0.0)
        self.segments = self.maps = 0
        self._step = 0

    def __getattr__(self, name):
        return getattr(self._d, name)

    def run(self, nsteps, dt, ensemble=0, tau=0.0, nf=None, ktemp=None, r1=None, r2=None, thermo=True):
        s = self._c["system"]
        x0, v0, f0, i0 = self._d.download()
        out = self._d.run(nsteps, dt, ensemble, tau, nf, ktemp, r1, r2, thermo=thermo)
        x, v, f, img = self._d.download()
        U = np.array(self._d.unitcell)
        pot = oracle.make_pot(self._c["kind"], self._c["params"])
        one = np.ones(s["dim"])
        with oracle.set_cell(U):
            ref = oracle.run(x0, i0, v0, f0, s["diam"], one, self._c["cutoff"], pot, dt, nsteps, use_cells=False,
                             ensemble=1, tau=tau, ktemp=ktemp, r1=r1, r2=r2)
            f_ref = oracle.forces_brute(x, one, self._c["cutoff"], pot, s["diam"])[0]
        dx = np.abs((x - ref["x"]) + (img - ref["img"]) @ U.T).max()
        dv = np.abs(v - ref["v"]).max()
        tol_f = 1e-11 * max(1.0, float(np.abs(f_ref).max()))
        df = np.abs(f - f_ref).max()
        for key, err, bound in (("x", dx, sa.SHORT_TOL), ("v", dv, sa.SHORT_TOL), ("F", df, tol_f)):
            self.worst[key] = max(self.worst[key], err / bound)
            assert err <= bound, "segment at step %d, %d steps: |d%s| = %.3e > %.3e" % (self._step, nsteps, key, err, bound)
        self._step += nsteps
        self.segments += 1
        return out

    def deform_cell(self, F, G=None):
        import moleculardynamics.jl_amd as md
        sh = self._shear
        d = self._c["system"]["dim"]
        dg = sh.rate * (sh.every * DT)
        assert np.array_equal(F, md.simple_shear(d, dg, sh.plane)) and np.array_equal(G, md.simple_shear(d, -dg, sh.plane))
        assert np.array_equal(np.asarray(F) @ np.asarray(G), np.eye(d))
        pos_b, v_b, U_b = self._d.list_rows(0)["pos"], self._d.download()[1], np.array(self._d.unitcell)
        kept = self._d.deform_cell(F, G)
        xr, vr, Ur = dr.deform_frame(pos_b, v_b, U_b, F, G)
        assert np.array_equal(self._d.list_rows(0)["pos"], xr) and np.array_equal(self._d.download()[1], vr)
        assert np.array_equal(self._d.unitcell, Ur)
        self.maps += 1
        return kept


def test_loop_against_the_cpu_segment_by_segment(tmp_path):
    import moleculardynamics.jl_amd as md
    c = case("sheared1000")
    pot = md.LennardJones()
    params = md.Parameters(0.897, 1000, DT, pot)
    texts = []
    for rep in range(2):
        shear = md.ShearFlow(0.5, every=10)
        state = _state(c, seed=11)
        real = state.system.device
        with real:
            if rep == 0:
                proxy = _AuditingDevice(real, c, shear)
                state.system.device = proxy
            out = str(tmp_path / ("run%d" % rep))
            md.run_simulation(state, params, md.NVT(1.0, 0.1), 200, 50, out, shear=shear)
            if rep == 0:
                print("loop: %d segments, %d maps; worst x %.3f v %.3f F %.3f of their bounds; rows kept in %d of %d; builds %d"
                      % (proxy.segments, proxy.maps, proxy.worst["x"], proxy.worst["v"], proxy.worst["F"],
                         sum(k["rows_kept"] for k in shear.records), len(shear.records), real.stats()["rebuilds"]))
                assert proxy.maps == 20 and proxy.segments >= 20
                # (thermal motion alone asks for a build about every 40 steps: a coupling that meets a list near its end
                # retires it, at most every other one)
                assert sum(k["rows_kept"] for k in shear.records) >= 10
            assert np.array_equal(real.unitcell, state.unitcell)
        texts.append(_read(out, "shear.txt"))
    assert texts[0] == texts[1] and texts[0].count(b"\n") == 21
    assert abs(shear.strain - 20 * 0.5 * 10 * DT) < 1e-14 and np.isfinite(shear.viscosity())


def test_a_2d_run_flips_once_and_stays_continuous():
    """ShearFlow driven by hand through its protocol (the golden 2-D system, NVT) to a strain of 0.65 in 2000 steps."""
    import moleculardynamics.jl_amd as md
    from moleculardynamics.jl_amd import _lib
    from moleculardynamics.jl_amd.thermostat import draw_bussi
    c = case("poly1200")
    s = c["system"]
    n, d = s["n"], 2
    every, total = 10, 2000
    shear = md.ShearFlow(0.65 / (total * DT), every=every, stress_every=10, flip=True)
    rng = np.random.default_rng(2)
    nf = d * (n - 1.0)
    jumps = []
    with _started(c, steps=0) as dev:

        class Watch:
            def __getattr__(self, name):
                return getattr(dev, name)

            def set_cell(self, U, mode=0):
                xb, _, _, ib = dev.download()
                Ub = np.array(dev.unitcell)
                dev.set_cell(U, mode)
                xa, _, _, ia = dev.download()
                Ua = np.array(dev.unitcell)
                jumps.append((np.abs(cr.unwrapped(xa, ia, Ua) - cr.unwrapped(xb, ib, Ub)).max(),
                              cr.unwrapped_bound([Ub, Ua], [ib, ia]), mode))

        watch = Watch()
        dev.run(2, DT)                                          # (a prune step: the configured radius and inner skin can be read)
        conf = _conf(dev)
        assert conf["inner_skin"] is not None
        shear._begin(watch, types.SimpleNamespace(brownian=False, dim=d, total_steps=total, dt=DT))
        volume = abs(float(np.linalg.det(dev.unitcell)))
        for first in range(0, total, every):
            kt = np.full(every, 0.11)
            r1, r2 = draw_bussi(nf, rng, every)
            U, W, K = dev.run(every, DT, _lib.MD_NVT, 0.1, nf, kt, r1, r2, thermo=True)
            shear._act(watch, first + every - 1, U, W, K, volume)
        strains = np.array([r["strain"] for r in shear.records])
        flips = [r for r in shear.records if r["flips"]]
        print("2-D flip run: strain %.4f, flips at steps %s, rows kept in %d of %d couplings, jump %.3e (allowed %.3e)"
              % (strains[-1], [r["step"] for r in flips], sum(r["rows_kept"] for r in shear.records), len(shear.records),
                 jumps[0][0] if jumps else -1.0, jumps[0][1] if jumps else -1.0))
        assert abs(strains[-1] - 0.65) < 1e-12 and np.all(np.diff(strains) > 0.0)
        assert len(flips) == 1 and len(jumps) == 1 and jumps[0][2] == _lib.MD_CELL_LATTICE
        assert jumps[0][0] <= jumps[0][1]
        tilts = np.array([r["tilt"] for r in shear.records]) / dev.unitcell[1, 1]
        assert np.abs(tilts).max() <= 0.5 + 0.65 / 200 + 1e-12
        dev.compute_forces()
        x, _, f, _ = dev.download()
        fr, _, _, pairs = _brute(c, x, dev.unitcell)
        assert np.abs(f - fr).max() <= 1e-11 * max(1.0, np.abs(fr).max())
        # the pair set of the rows the handle holds at the end (kept through the last maps, not fresh from a build): the
        # entries within the cutoff at the stored positions, against the oracle's pairs
        snap = ra.snapshot_of(dev)
        ent = np.asarray(snap["outer"]).reshape(-1, 5)
        U = ra.lattice(dev.unitcell, d)
        inside = ent[ra.entry_d2(snap["pos"], ent, U) <= c["cutoff"] ** 2]
        mine = np.unique(np.sort(inside[:, :2], axis=1), axis=0)
        assert len(inside) == 2 * len(mine) and np.array_equal(mine, pairs)
        m0, m1, sig = dev.deform_state()
        assert snap["info"]["rl"] == sig[0] * conf["rl"]
        _audit("2-D flip run, end", dev, c, conf)


def test_the_shear_stress_has_the_sign_of_the_rate(tmp_path):
    """A sign, not a value: the mean sigma_ab over the second half of one unit of strain.  The mean and its standard error
    (5 blocks of 10 readings) are printed; the mean must lie at least 5 standard errors from zero for the sign to count."""
    import moleculardynamics.jl_amd as md
    c = case("lj4000")
    params = md.Parameters(0.897, 4000, DT, md.LennardJones())
    for rate in (0.5, -0.5):
        shear = md.ShearFlow(rate, every=10)
        state = _state(c, seed=7)
        with state.system.device:
            md.run_simulation(state, params, md.NVT(0.7, 0.1), 1000, 500, str(tmp_path / ("r%g" % rate)), shear=shear,
                              write_trajectory=False)
        sig = np.array([r["sigma_ab"] for r in shear.records])
        assert len(sig) == 100 and np.all(np.isfinite(sig))
        half = sig[50:]
        blocks = half.reshape(5, 10).mean(axis=1)
        mean, err = float(half.mean()), float(blocks.std(ddof=1) / np.sqrt(5))
        print("rate %+.1f: <sigma_ab> = %+.4f +- %.4f (second half of one unit of strain), %.1f standard errors; "
              "viscosity over the whole run %.3f; rows kept in %d of 100; flips %d"
              % (rate, mean, err, abs(mean) / err, shear.viscosity(), sum(r["rows_kept"] for r in shear.records),
                 sum(r["flips"] for r in shear.records)))
        assert abs(mean) >= 5.0 * err
        assert np.sign(mean) == np.sign(rate)


def test_run_simulation_with_and_without_shear(tmp_path):
    import moleculardynamics.jl_amd as md
    c = case("lj4000")
    params = md.Parameters(0.897, 4000, DT, md.LennardJones())
    outs = []
    for kw in ({}, dict(shear=None)):
        state = _state(c, seed=5)
        out = str(tmp_path / ("plain%d" % len(outs)))
        with state.system.device:
            md.run_simulation(state, params, md.NVT(1.0, 0.1), 60, 20, out, **kw)
        outs.append(({f: _read(out, f) for f in sorted(os.listdir(out))}, state.system.positions, state.velocities,
                     state.images))
    assert outs[0][0] == outs[1][0] and sorted(outs[0][0]) == ["final.xyz", "thermo.txt", "trajectory.xyz"]
    for a, b in zip(outs[0][1:], outs[1][1:]):
        assert np.array_equal(a, b)
    shear = md.ShearFlow(0.5, every=10)
    state = _state(c, seed=5)
    out = str(tmp_path / "shear")
    with state.system.device as dev:
        md.run_simulation(state, params, md.NVT(1.0, 0.1), 60, 20, out, shear=shear, rdf=md.RadialDistribution(2.5, 50))
        assert np.array_equal(dev.unitcell, state.unitcell) and state.system.unitcell is state.unitcell
    assert [r["step"] for r in shear.records] == [9, 19, 29, 39, 49, 59]
    assert [r["rows_kept"] for r in shear.records][0] == 0 and sum(r["rows_kept"] for r in shear.records) >= 3
    U = c["cell"]
    for _ in range(6):
        U = md.shear_flow_update(U, 0.5, 10 * DT, (0, 1))[2]
    assert np.array_equal(state.unitcell, U) and abs(abs(np.linalg.det(U)) - abs(np.linalg.det(c["cell"]))) < 1e-9
    assert sorted(os.listdir(out)) == ["final.xyz", "rdf.txt", "shear.txt", "thermo.txt", "trajectory.xyz"]
    # the thermo lines of steps 20 and 40 differ from the unsheared run's; step 0 (before any coupling) does not
    plain = outs[0][0]["thermo.txt"].decode().splitlines()
    mine = open(os.path.join(out, "thermo.txt")).read().splitlines()
    assert plain[:2] == mine[:2] and plain[2:] != mine[2:]
