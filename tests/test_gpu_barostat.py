"""-m gpu: md_scale_cell and the stochastic cell rescaling loop on the device, against tests/baro_reference.py, the row audit
of tests/row_audit.py, md_set_cell on a twin handle, the oracle's pair loop and the oracle's step loop.

Shapes: LJ at N = 4000 (15 full tiles + 160), rho = 0.897, cutoff 2.5; the 2-D polydisperse golden system (N = 1200,
per-particle diameters); LJ at N = 1000 in a sheared cell (3 full tiles + 232, a general cell with the full skin).

Tolerances.  The stored frame after a scale: bit for bit against numpy's mu * x.  Against md_set_cell(mu U, AFFINE) on a
twin: baro_reference.scaled_bound.  Forces, U, W against the oracle or a fresh handle: tests/test_gpu_parity.py's
(|dF| <= 1e-11 max(1, |F|), U and W relative 1e-12).  Segments of the loop: tests/step_audit.py's (forces as above, x and v
after 10 steps 1e-10).  mu against longdouble: 4 ulp.  Row audits: every invariant of tests/row_audit.py with the figures
md_list_rows reports; the knife-edge bands are capped as tests/test_gpu_row_audit.py caps them (step_audit.MAX_EXCLUDED)."""
import os
import re

import numpy as np
import pytest

from oracle import oracle
from tests import baro_reference as br
from tests import cell_reference as cr
from tests import row_audit as ra
from tests import step_audit as sa
from tests.test_gpu_hessian import frame
from tests.util import lj_system, sheared

pytestmark = pytest.mark.gpu

LJ = [1.0, 1.0, 2.5]
DT = 0.002
_CASES = {}


def case(name):
    """dict(system, kind, params, cutoff, cell) of a named input, built once."""
    if name not in _CASES:
        if name == "lj4000":
            c = dict(system=lj_system(4000), kind=sa.POT_LJ, params=LJ, cutoff=2.5)
        elif name == "poly1200":
            fr = frame("poly1200")
            c = dict(system=fr["system"], kind=fr["kind"], params=fr["params"], cutoff=fr["cutoff"])
        else:
            s = lj_system(1000)
            c = dict(system=sheared(s, s["box"][0] / 4.0), kind=sa.POT_LJ, params=LJ, cutoff=2.5)
        s = c["system"]
        c["cell"] = np.array(ra.lattice(s["box"] if s.get("cell") is None else s["cell"], s["dim"]), dtype=np.float64)
        _CASES[name] = c
    return _CASES[name]


CASES = ["lj4000", "poly1200", "sheared1000"]


def _device(c, cell=None):
    from moleculardynamics.jl_amd import MDDevice
    s = c["system"]
    dev = MDDevice(s["dim"], s["n"], c["cell"] if cell is None else cell, c["cutoff"])
    dev.set_potential(c["kind"], c["params"])
    return dev


def _started(c, steps=30):
    """A handle `steps` steps into an NVE run from the case's frame."""
    s = c["system"]
    dev = _device(c)
    dev.upload(s["x"], s["v"], np.zeros_like(s["x"]), s["img"], s["diam"])
    dev.compute_forces()
    if steps:
        dev.run(steps, DT)
    return dev


def _brute(c, x, U):
    s = c["system"]
    pot = oracle.make_pot(c["kind"], c["params"])
    if cr.is_general(U):
        with oracle.set_cell(U):
            f, u, w, pairs = oracle.forces_brute(x, np.ones(s["dim"]), c["cutoff"], pot, s["diam"], want_pairs=True)
    else:
        f, u, w, pairs = oracle.forces_brute(x, np.diag(U).copy(), c["cutoff"], pot, s["diam"], want_pairs=True)
    return f, u, w, pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))]


def _parity(what, got, ref):
    (f, u, w), (f_ref, u_ref, w_ref) = got, ref
    err = np.abs(f - f_ref).max()
    print("%s: |dF| %.3e (allowed %.3e), dU/U %.3e, dW/W %.3e"
          % (what, err, 1e-11 * max(1.0, np.abs(f_ref).max()), abs(u - u_ref) / abs(u_ref), abs(w - w_ref) / abs(w_ref)))
    assert err <= 1e-11 * max(1.0, np.abs(f_ref).max()), what
    assert abs(u - u_ref) <= 1e-12 * abs(u_ref) and abs(w - w_ref) <= 1e-12 * abs(w_ref), what


def _audit(name, dev, c, loose_o4=False):
    """check_rows on the handle's rows with the figures it reports, in the cell it holds.  loose_o4 (build paths whose O4
    bound is 16 eps): O4 replaced by d2(x0) <= rl_eff^2 (1 + 1e-12), checked here."""
    snap = ra.snapshot_of(dev)
    dim = c["system"]["dim"]
    res = ra.check_rows(snap, dev.unitcell, dim)
    print(ra.counts_line(name, res["counts"]))
    viol = res["violations"]
    if loose_o4:
        viol = [v for v in viol if v.check != "O4"]
        d2 = ra.entry_d2(snap["x0"], np.asarray(snap["outer"]).reshape(-1, 5), ra.lattice(dev.unitcell, dim))
        assert d2.max() <= snap["info"]["rl"] ** 2 * (1.0 + 1e-12), name
    assert viol == [], (name, [str(v) for v in viol])
    k = res["counts"]
    assert k["band_rl"] + k["band_rin"] + k["band_rc"] <= sa.MAX_EXCLUDED, name
    return snap, k


# ---------------------------------------------------------------------------------------------------------------------
# 1. the frame
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mu", [0.9987, 1.0021])
@pytest.mark.parametrize("name", CASES)
def test_frame_bit_for_bit_and_against_set_cell(name, mu):
    c = case(name)
    s = c["system"]
    U0 = c["cell"]
    with _started(c) as dev, _device(c) as twin:
        # (a) live rows: the stored frame and both reference frames, bit for bit; velocities; images untouched
        before = dev.list_rows(0)
        x_b, v_b, _, img_b = dev.download()
        kept = dev.scale_cell(mu, 1.0 / mu)
        after = dev.list_rows(0)
        x_a, v_a, _, img_a = dev.download()
        U1 = np.float64(mu) * U0
        assert kept == 1 and np.array_equal(dev.unitcell, U1)
        for key in ("pos", "x0", "x1"):
            assert np.array_equal(after[key], np.float64(mu) * before[key]), (name, key)
        assert np.array_equal(v_a, np.float64(1.0 / mu) * v_b)
        # what download shows is the stored frame through the new cell's lazy wrap; frac + img is kept to rounding
        un_b, un_a = cr.unwrapped(x_b, img_b, U0), cr.unwrapped(x_a, img_a, U1)
        bound = br.scaled_bound(U1, after["pos"], img_a) + cr.unwrapped_bound([U0, U1], [img_b, img_a])
        assert np.abs(un_a - np.longdouble(mu) * un_b).max() <= bound
        # (b) a frame the handle stores exactly as a download shows it: x, v, images and cell against the restatement,
        # and against md_set_cell(mu U, AFFINE) on the twin within the stated bound
        z = np.zeros_like(x_b)
        for h in (dev, twin):
            h.set_cell(U0)                      # (dev: back to the old cell; what it holds is uploaded over)
            h.upload(x_b, v_b, z, img_b, s["diam"])
        dev.scale_cell(mu, 1.0 / mu)
        twin.set_cell(U1, twin.CELL_AFFINE)
        xs, vs, _, ims = dev.download()
        xr, vr, Ur = br.scale_frame(x_b, v_b, U0, mu, 1.0 / mu)
        xw, iw = cr.export_wrap(xr, img_b, Ur)
        assert np.array_equal(Ur, U1) and np.array_equal(dev.unitcell, U1) and np.array_equal(twin.unitcell, U1)
        assert np.array_equal(xs, xw) and np.array_equal(ims, iw.astype(np.int32)) and np.array_equal(vs, vr)
        xt, _, _, imt = twin.download()
        err = np.abs(cr.unwrapped(xs, ims, U1) - cr.unwrapped(xt, imt, U1)).max()
        bound = br.scaled_bound(U1, xr, ims)
        print("%s mu %g: scale against set_cell(AFFINE): |d(x + U img)| %.3e (allowed %.3e)" % (name, mu, err, bound))
        assert err <= bound


# ---------------------------------------------------------------------------------------------------------------------
# 2. the rows are kept and stay right
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["default", "no_fused_build"])
@pytest.mark.parametrize("name", CASES)
def test_rows_kept_through_two_scales(monkeypatch, name, path):
    if path == "no_fused_build":
        monkeypatch.setenv("MDHIP_NO_FUSED_BUILD", "1")
    c = case(name)
    s = c["system"]
    loose = path != "default"
    with _started(c) as dev:
        snap, _ = _audit("%s/%s before" % (name, path), dev, c, loose)
        loose = loose or not snap["info"]["fused_build"]       # (a case the fused build cannot take: the fallback built it)
        assert snap["info"]["list_valid"] and snap["info"]["tiled"]
        had_inner = bool(snap["info"]["inner_valid"])
        builds = dev.stats()["rebuilds"]
        m = np.float64(1.0)
        for mu in (0.996, 1.003):
            assert dev.scale_cell(mu, 1.0 / mu) == 1
            m = m * np.float64(mu)
            sn, k = _audit("%s/%s after %g" % (name, path, mu), dev, c, loose)
            rl, skin, inner = br.effective(snap["info"]["rc"], snap["info"]["skin"], snap["info"]["inner_skin"], m, m)
            assert (sn["info"]["rl"], sn["info"]["skin"]) == (rl, skin)
            if sn["info"]["inner_valid"]:
                assert sn["info"]["inner_skin"] == inner and sn["info"]["d1"] >= snap["info"]["d1"] * m
        u, w = dev.compute_forces()
        assert dev.stats()["rebuilds"] == builds               # the evaluation walked the kept rows
        _audit("%s/%s after compute_forces" % (name, path), dev, c, loose)
        x, v, f, img = dev.download()
        with _device(c, cell=dev.unitcell) as fresh:
            fresh.upload(x, v, np.zeros_like(x), img, s["diam"])
            uf, wf = fresh.compute_forces()
            ff = fresh.download()[2]
        _parity("%s/%s kept rows against a fresh handle" % (name, path), (f, u, w), (ff, uf, wf))
        dev.run(20, DT)
        _audit("%s/%s after 20 further steps" % (name, path), dev, c, loose)
        x, _, f, _ = dev.download()
        fr, ur, wr, _ = _brute(c, x, dev.unitcell)
        assert np.abs(f - fr).max() <= 1e-11 * max(1.0, np.abs(fr).max())
        print("%s/%s: inner rows at the first scale: %s" % (name, path, had_inner))


# ---------------------------------------------------------------------------------------------------------------------
# 3. the displacement limit's edge, and retirement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", ["below", "above"])
def test_limit_edge(side):
    """mu is chosen from the snapshot so that skin_eff / 2 lands a relative 1e-6 below (above) the largest displacement
    from x0 as it will be after the scale, mu D: rows retired and the next evaluation builds (kept, no build)."""
    c = case("lj4000")
    with _started(c) as dev:
        snap = ra.snapshot_of(dev)
        info = snap["info"]
        D = float(np.sqrt(((snap["pos"] - snap["x0"]) ** 2).sum(axis=1)).max())
        rc, rl = info["rc"], info["rl"]
        # mu rl - rc = 2 mu D (1 -+ 1e-6)  =>  mu = rc / (rl - 2 D (1 -+ 1e-6))
        mu = rc / (rl - 2.0 * D * (1.0 - 1e-6 if side == "below" else 1.0 + 1e-6))
        assert 0.85 < mu < 1.0 and mu * rl - rc >= (2.0 / 3.0) * info["skin"], (mu, D)      # (above md_scale_cell's floor)
        builds = dev.stats()["rebuilds"]
        kept = dev.scale_cell(mu, 1.0 / mu)
        after = dev.list_rows(0)["info"]
        print("limit edge (%s): D = %.6f, mu = %.9f, skin_eff / 2 = %.9f, mu D = %.9f, kept %d"
              % (side, D, mu, 0.5 * (mu * rl - rc), mu * D, kept))
        assert kept == (0 if side == "below" else 1) and after["list_valid"] == kept
        dev.compute_forces()
        assert dev.stats()["rebuilds"] == builds + (1 if side == "below" else 0)
        sn, _ = _audit("limit edge %s" % side, dev, c)         # V3 among the rest
        x, _, f, _ = dev.download()
        fr = _brute(c, x, dev.unitcell)[0]
        assert np.abs(f - fr).max() <= 1e-11 * max(1.0, np.abs(fr).max())


@pytest.mark.parametrize("name", CASES)
def test_retirement(name):
    c = case(name)
    with _started(c) as dev:
        if name == "sheared1000":
            # (0.9 would put the face distance below three cutoffs: the largest compression the cell allows)
            mu = 3.0 * c["cutoff"] / cr.face_distances(c["cell"]).min() * 1.0005
        else:
            mu = 0.9
        assert dev.scale_cell(mu, 1.0 / mu) == 0
        info = dev.list_rows(0)["info"]
        assert not info["list_valid"] and not info["inner_valid"]
        u, w = dev.compute_forces()
        x, _, f, _ = dev.download()
        fr, ur, wr, pairs = _brute(c, x, dev.unitcell)
        assert np.array_equal(dev.neighbor_pairs(), pairs)
        _parity("%s retired at mu = %g" % (name, mu), (f, u, w), (fr, ur, wr))
        full = dev.list_rows(0)["info"]
        assert full["list_valid"] and full["skin"] == min(0.6, full["skin"]) and full["rl"] == full["rc"] + full["skin"]


@pytest.mark.parametrize("kind", ["skin_0", "user_potential", "no_tiles"])
def test_handles_without_two_level_rows_are_scaled_and_build_again(monkeypatch, kind):
    """The simple route: a handle with skin 0, a user potential, or rows that are not tiled is scaled, its list retired,
    and the next evaluation is the oracle's in the new cell."""
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
        for mu in (0.9987, 1.0021):
            assert dev.scale_cell(mu, 1.0 / mu) == 0
            info = dev.list_rows(0)
            assert not info["info"]["list_valid"]
            stored, v_b = np.float64(mu) * stored, np.float64(1.0 / mu) * v_b
            assert np.array_equal(info["pos"], stored) and np.array_equal(dev.download()[1], v_b)
            u, w = dev.compute_forces()
            x, _, f, _ = dev.download()
            fr, ur, wr, pairs = _brute(c, x, dev.unitcell)
            assert np.array_equal(dev.neighbor_pairs(), pairs)
            _parity("%s scaled by %g" % (kind, mu), (f, u, w), (fr, ur, wr))
        dev.run(10, DT)
        x, _, f, _ = dev.download()
        fr = _brute(c, x, dev.unitcell)[0]
        assert np.abs(f - fr).max() <= 1e-11 * max(1.0, np.abs(fr).max())


# ---------------------------------------------------------------------------------------------------------------------
# 4. refusals leave the handle untouched
# ---------------------------------------------------------------------------------------------------------------------
def _untouched_checker(dev, U0):
    """A closure that asserts download, compute_forces, list_rows and the cell are bit for bit what they are now."""
    u0, w0 = dev.compute_forces()
    before = dev.download()
    rows0 = dev.list_rows(0)

    def untouched(what):
        for a, b in zip(before, dev.download()):
            assert np.array_equal(a, b), what
        assert dev.compute_forces() == (u0, w0), what
        assert np.array_equal(dev.download()[2], before[2]), what
        rows = dev.list_rows(0)
        assert rows["info"] == rows0["info"] and np.array_equal(rows["entries"], rows0["entries"]), what
        for key in ("x0", "x1", "pos"):
            assert np.array_equal(rows[key], rows0[key]), what
        assert np.array_equal(dev.unitcell, U0), what

    return untouched


def test_refusals_leave_the_handle_untouched():
    """Every refusal of md_scale_cell but two.  The slab one needs several ranks (next test).  state_invalid is set only by a
    step loop, or a scale pass, that failed on the device: reaching it here would mean provoking such a failure, so its one
    line, require_state ahead of every state change as in every other entry, is left to reading."""
    from moleculardynamics.jl_amd import MdhipError
    c = case("sheared1000")
    U0 = c["cell"]
    perp = cr.face_distances(U0).min()
    with _started(c) as dev:
        untouched = _untouched_checker(dev, U0)
        for mu, vs, why in ((float("nan"), 1.0, "mu"), (float("inf"), 1.0, "mu"), (0.0, 1.0, "mu"), (-1.0, 1.0, "mu"),
                            (1.0, float("nan"), "vscale"), (1.0, float("inf"), "vscale")):
            with pytest.raises(MdhipError, match=why):
                dev.scale_cell(mu, vs)
            untouched((mu, vs))
        too_small = 3.0 * c["cutoff"] / perp * 0.999
        with pytest.raises(MdhipError, match="face distance"):
            dev.scale_cell(too_small)
        untouched("face distance")
        dev.snapshot_begin()
        with pytest.raises(MdhipError, match="in flight"):
            dev.scale_cell(1.001)
        dev.snapshot_end()
        untouched("frame in flight")
    # a face distance below 3 r_max of a pair-walk sampler, still above 3 cutoffs
    small = 3.0 * 3.2 / perp * 0.999
    assert small * perp > 3.0 * c["cutoff"]
    for setup, who in ((lambda d: d.rdf_setup(3.2, 16), "md_rdf_"), (lambda d: d.mpc_setup(3.2, 16, weights=[1.0], tmax=1.0), "md_mpc_")):
        with _started(c) as dev:
            setup(dev)
            untouched = _untouched_checker(dev, U0)
            with pytest.raises(MdhipError, match="r_max"):
                dev.scale_cell(small)
            untouched(who + " r_max")
            assert dev.scale_cell(0.9995, 1.0) == 1                # (with room for r_max the sampler is no obstacle)
    # the samplers that belong to one cell, each named in its message
    e1 = np.array([[1.0, 0.0, 0.0]])
    n1 = np.array([[1, 0, 0]], dtype=np.int32)
    for setup, who in ((lambda d: d.dyn_setup(1, 1), "md_dyn_"), (lambda d: d.sq_setup(n1), "md_sq_"),
                       (lambda d: d.cur_setup(n1, e1), "md_cur_"), (lambda d: d.chi4_setup(0.3), "md_chi4_"),
                       (lambda d: d.cage_setup(1, 1, 1.5), "md_cage_")):
        with _started(c) as dev:
            setup(dev)
            untouched = _untouched_checker(dev, U0)
            with pytest.raises(MdhipError, match="the %s sampler" % who):
                dev.scale_cell(1.001)
            untouched(who)


def test_the_slab_refusal_is_in_the_host_code():
    """A slab handle needs several ranks; the refusal is one line ahead of every state change."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "moleculardynamics", "jl_amd", "csrc", "mdhip.hip")).read()
    body = src[src.index("int md_scale_cell(md_ctx *ctx, double mu, double vscale, int *rows_kept)"):]
    assert body.index("md_scale_cell: not available on a slab-decomposition handle") < body.index("require_state(ctx")


# ---------------------------------------------------------------------------------------------------------------------
# 5. the loop
# ---------------------------------------------------------------------------------------------------------------------
class _RecordingRng:
    """state.rng with the last scalar Gaussian draw remembered (the barostat's is the one right before its scale)."""

    def __init__(self, seed):
        self._g = np.random.default_rng(seed)
        self.last_normal = None

    def standard_normal(self, *a, **kw):
        r = self._g.standard_normal(*a, **kw)
        if not a and not kw:
            self.last_normal = float(r)
        return r

    def __getattr__(self, name):
        return getattr(self._g, name)


class _AuditingDevice:
    """An MDDevice seen through run_simulation's eyes: every segment is restated by oracle.run from the handle's own
    downloaded state in the cell of the moment, every coupling's mu is recomputed in longdouble."""

    def __init__(self, dev, c, baro, rng, pot_lrc, tau):
        self._d, self._c, self._baro, self._rng, self._lrc, self._tau = dev, c, baro, rng, pot_lrc, tau
        self.worst = dict(x=0.0, v=0.0, F=0.0, mu_ulps=0.0)
        self.segments = self.couplings = 0
        self._uwk = None
        self._step = 0

    def __getattr__(self, name):
        return getattr(self._d, name)

    def run(self, nsteps, dt, ensemble=0, tau=0.0, nf=None, ktemp=None, r1=None, r2=None, thermo=True):
        s = self._c["system"]
        x0, v0, f0, i0 = self._d.download()
        self._uwk = self._d.run(nsteps, dt, ensemble, tau, nf, ktemp, r1, r2, thermo=thermo)
        x, v, f, img = self._d.download()
        U = np.array(self._d.unitcell)
        box = np.diag(U).copy()
        pot = oracle.make_pot(self._c["kind"], self._c["params"])
        ref = oracle.run(x0, i0, v0, f0, s["diam"], box, self._c["cutoff"], pot, dt, nsteps, use_cells=True, nthreads=4,
                         ensemble=1, tau=tau, ktemp=ktemp, r1=r1, r2=r2)
        dx = np.abs((x - ref["x"]) + (img - ref["img"]) @ U.T).max()
        dv = np.abs(v - ref["v"]).max()
        f_ref = oracle.forces_cells(x, box, self._c["cutoff"], pot, s["diam"], nthreads=4)[0]
        tol_f = 1e-11 * max(1.0, float(np.abs(f_ref).max()))
        df = np.abs(f - f_ref).max()
        for key, err, bound in (("x", dx, sa.SHORT_TOL), ("v", dv, sa.SHORT_TOL), ("F", df, tol_f)):
            self.worst[key] = max(self.worst[key], err / bound)
            assert err <= bound, "segment at step %d, %d steps: |d%s| = %.3e > %.3e" % (self._step, nsteps, key, err, bound)
        self._step += nsteps
        self.segments += 1
        return self._uwk

    def scale_cell(self, mu, vscale=1.0):
        b = self._baro
        Uw, Ww, Kw = self._uwk
        V = abs(float(np.linalg.det(self._d.unitcell)))
        n, d = self._c["system"]["n"], self._c["system"]["dim"]
        p_int = (2.0 * Kw + Ww) / (d * V) + self._lrc(n, V)
        xi = self._rng.last_normal if b.stochastic else 0.0
        ref = br.crescale_factor_ld(p_int, V, b._ktemp_at(self._step - 1), b.pressure, b.compressibility, b.tau_p,
                                    b.every * DT, xi, d)
        self.worst["mu_ulps"] = max(self.worst["mu_ulps"], br.ulps(mu, ref))
        assert br.ulps(mu, ref) <= 4.0 and vscale == 1.0 / mu
        self.couplings += 1
        return self._d.scale_cell(mu, vscale)


def _state(c, seed, dev=None):
    import types
    import moleculardynamics.jl_amd as md
    s = c["system"]
    n, dim = s["n"], s["dim"]
    dev = _device(c) if dev is None else dev
    system = types.SimpleNamespace(device=dev, positions=np.array(s["x"]), xpositions=None, unitcell=np.array(c["cell"]),
                                   energy_and_forces=types.SimpleNamespace(forces=np.zeros((n, dim)), energy=0.0, virial=0.0))
    return md.SimulationState(system, np.array(s["diam"]), _RecordingRng(seed), np.array(c["cell"]), np.array(s["v"]),
                              np.zeros((n, dim), dtype=np.int32), dim, dim * (n - 1.0))


def _read(path, name):
    with open(os.path.join(path, name), "rb") as io:
        return io.read()


def test_loop_against_the_cpu_segment_by_segment(tmp_path):
    import moleculardynamics.jl_amd as md
    c = case("lj4000")
    pot = md.LennardJones()
    params = md.Parameters(0.897, 4000, DT, pot)
    texts = []
    for rep in range(2):
        baro = md.StochasticCellRescaling(2.0, 0.5, 0.2, every=10)
        state = _state(c, seed=11)
        real = state.system.device
        with real:
            if rep == 0:
                proxy = _AuditingDevice(real, c, baro, state.rng, pot.pressure_lrc, 0.1)
                state.system.device = proxy
            out = str(tmp_path / ("run%d" % rep))
            md.run_simulation(state, params, md.NVT(1.0, 0.1), 200, 50, out, barostat=baro)
            if rep == 0:
                print("loop: %d segments, %d couplings; worst x %.3f v %.3f F %.3f of their bounds; mu within %.2f ulp; rows "
                      "kept in %d of %d couplings; builds %d"
                      % (proxy.segments, proxy.couplings, proxy.worst["x"], proxy.worst["v"], proxy.worst["F"],
                         proxy.worst["mu_ulps"], sum(k["rows_kept"] for k in baro.couplings), len(baro.couplings),
                         real.stats()["rebuilds"]))
                assert proxy.couplings == 20 and proxy.segments >= 20
                assert sum(k["rows_kept"] for k in baro.couplings) >= 15
            assert np.array_equal(real.unitcell, state.unitcell)
        texts.append(_read(out, "barostat.txt"))
    assert texts[0] == texts[1] and texts[0].count(b"\n") == 21


@pytest.mark.parametrize("factor", [2.0, 0.5])
def test_direction_of_the_deterministic_relaxation(tmp_path, factor):
    import moleculardynamics.jl_amd as md
    c = case("lj4000")
    s = c["system"]
    pot = md.LennardJones()
    with _started(c, steps=0) as dev:
        u, w = dev.compute_forces()
        k = 0.5 * float((s["v"] ** 2).sum())
        V0 = abs(float(np.linalg.det(c["cell"])))
        p0 = (2.0 * k + w) / (3 * V0) + pot.pressure_lrc(s["n"], V0)
    baro = md.StochasticCellRescaling(factor * p0, 0.5, 0.05, every=10, stochastic=False)
    state = _state(c, seed=3)
    with state.system.device:
        md.run_simulation(state, md.Parameters(0.897, 4000, DT, pot), md.NVT(1.0, 0.1), 300, 100, str(tmp_path), barostat=baro,
                          write_trajectory=False)
    V1 = abs(float(np.linalg.det(state.unitcell)))
    print("P0 = %.3f x the starting pressure %.4f: V %.2f -> %.2f" % (factor, p0, V0, V1))
    assert p0 > 0.0 and ((V1 < V0) if factor > 1.0 else (V1 > V0))
    assert state.rng.last_normal is not None                   # (the thermostat drew; the barostat's xi is 0)


def test_run_simulation_with_and_without_a_barostat(tmp_path):
    import moleculardynamics.jl_amd as md
    c = case("lj4000")
    pot = md.LennardJones()
    params = md.Parameters(0.897, 4000, DT, pot)
    outs = []
    for kw in ({}, dict(barostat=None)):
        state = _state(c, seed=5)
        out = str(tmp_path / ("plain%d" % len(outs)))
        with state.system.device:
            md.run_simulation(state, params, md.NVT(1.0, 0.1), 60, 20, out, **kw)
        outs.append(({f: _read(out, f) for f in sorted(os.listdir(out))}, state.system.positions, state.velocities,
                     state.images))
    assert outs[0][0] == outs[1][0] and sorted(outs[0][0]) == ["final.xyz", "thermo.txt", "trajectory.xyz"]
    for a, b in zip(outs[0][1:], outs[1][1:]):
        assert np.array_equal(a, b)

    baro = md.StochasticCellRescaling(2.0, 0.5, 0.2, every=10)
    state = _state(c, seed=5)
    out = str(tmp_path / "baro")
    with state.system.device as dev:
        md.run_simulation(state, params, md.NVT(1.0, 0.1), 60, 20, out, barostat=baro)
        assert np.array_equal(dev.unitcell, state.unitcell) and state.system.unitcell is state.unitcell
    assert params.rho == 0.897
    # final.xyz's cell is the handle's
    header = open(os.path.join(out, "final.xyz")).read().splitlines()[1]
    lat = np.array([float(t) for t in re.search(r'Lattice="([^"]+)"', header).group(1).split()])
    assert np.allclose(np.sort(lat[lat != 0.0]), np.sort(np.diag(state.unitcell)), rtol=0, atol=1e-5)
    # every frame lies inside its own cell, and the cells differ
    lines = open(os.path.join(out, "trajectory.xyz")).read().splitlines()
    starts = [i for i, l in enumerate(lines) if l == "ITEM: TIMESTEP"]
    edges = []
    for i in starts:
        assert lines[i + 4].startswith("ITEM: BOX BOUNDS")
        edge = float(lines[i + 5].split()[1])
        xyz = np.array([[float(t) for t in l.split()[3:6]] for l in lines[i + 9:i + 9 + 4000]])
        assert xyz.min() >= 0.0 and xyz.max() <= edge + 1e-6
        edges.append(edge)
    assert len(edges) == 3 and len(set(edges)) == 3
    at = [k["step"] for k in baro.couplings]
    assert at == [9, 19, 29, 39, 49, 59]
    want = [c["cell"][0, 0]] + [c["cell"][0, 0] * np.prod([k["mu"] for k in baro.couplings if k["step"] <= st]) for st in (20, 40)]
    assert np.allclose(edges, want, rtol=0, atol=2e-6)
    # the thermo line's density is n / V of the moment.  The last line (step 40) is the one whose W the state keeps:
    # pressure = W / (d V) + (n / V) T + lrc(n, V) with V after the coupling at step 39 and T as printed (six decimals
    # each); with params.rho in place of n / V the line would be off by (rho - n / V) T, which is asserted to be visible
    thermo = [l.split() for l in open(os.path.join(out, "thermo.txt")).read().splitlines()[1:]]
    assert [int(t[0]) for t in thermo] == [0, 20, 40]
    T, P = float(thermo[-1][2]), float(thermo[-1][3])
    V = [k["volume"] for k in baro.couplings if k["step"] <= 40][-1]
    W = state.system.energy_and_forces.virial
    want = W / (3 * V) + (4000 / V) * T + pot.pressure_lrc(4000, V)
    slack = 1e-6 + (4000 / V) * 1e-6
    print("thermo at step 40: P %.6f, from W, T and n / V %.6f; with params.rho %.6f" % (P, want, want + (0.897 - 4000 / V) * T))
    assert abs(P - want) <= slack and abs(0.897 - 4000 / V) * T > 100 * slack
