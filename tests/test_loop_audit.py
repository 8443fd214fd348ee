"""The Brownian and FIRE modes of the step audit (tests/step_audit.py) proved on the CPU: the oracle's two loops on a
general cell, the numpy restatements the audit leans on held to the oracle's C, steppers made of the oracle's own functions
passing every schedule with nothing excluded, and twelve sabotaged steppers -- the faults the two modes exist to find --
each failing on the check named here."""
import numpy as np
import pytest

from tests import step_audit as sa
from tests.util import blob_gas_system, lj_system, poly_system, sheared, tiny_system

LJ = [1.0, 1.0, 2.5]
SEED = 0xC0FFEE1234ABCDEF
KT = 1.5
HIGH = 2 ** 32 - 3                # three steps below the first global step with a non-zero high counter word

# name -> (system, kind, params, cutoff, Brownian dt, fire_kw)
CASES = {
    "blob": lambda: (blob_gas_system(), sa.POT_LJ, LJ, 2.5, 4e-4, dict(dt_initial=0.005, dt_max=0.03, nmin=0)),
    "poly_2d": lambda: (poly_system(), sa.POT_POLYDISPERSE, [1.25, 0.2], 1.25 * 1.2, 1e-4,
                        dict(dt_initial=0.005, dt_max=0.03, nmin=0)),
    "tiny65": lambda: (tiny_system(65), sa.POT_LJ, LJ, 2.5, 4e-4, dict(dt_initial=0.005, dt_max=0.03, nmin=0)),
    "blob_sheared": lambda: (sheared(blob_gas_system(), 6.0), sa.POT_LJ, LJ, 2.5, 4e-4,
                             dict(dt_initial=0.005, dt_max=0.03, nmin=0)),
}


@pytest.fixture(scope="module")
def blob():
    return blob_gas_system()


def _case(oracle, name):
    s, kind, params, cutoff, dt, fire_kw = CASES[name]()
    return s, oracle.make_pot(kind, params), cutoff, dt, fire_kw


def _unwrapped(r, U):
    return r["x"] + r["img"] @ np.asarray(U).T


# ------------------------------------------------------------------------------------------- the oracle on a general cell
def _both_loops(oracle, s, pot, cutoff, nsteps):
    kw = dict(use_cells=False, nthreads=1)
    bd = oracle.run_brownian(s["x"], s["img"], s["diam"], s["box"], cutoff, pot, 4e-4, KT, SEED, nsteps, **kw)
    fi = oracle.fire_minimize(s["x"], s["img"], s["diam"], s["box"], cutoff, pot, max_steps=nsteps, tol=sa.NEVER,
                              dt_initial=0.005, dt_max=0.03, nmin=0, **kw)
    return bd, fi


@pytest.mark.parametrize("make", [lambda: tiny_system(65), lambda: lj_system(200, rho=0.8, dim=2), blob_gas_system])
def test_oracle_loops_in_a_diagonal_general_cell_are_bit_identical(oracle, make):
    """set_cell(diag(L)) sends both loops through wrap_tric and the 3^d image search; the numbers do not change."""
    s = make()
    pot = oracle.make_pot(sa.POT_LJ, LJ)
    plain = _both_loops(oracle, s, pot, 2.5, 10)
    with oracle.set_cell(np.diag(s["box"])):
        celled = _both_loops(oracle, s, pot, 2.5, 10)
    for a, b in zip(plain, celled):
        for key in ("x", "img", "f"):
            assert np.array_equal(a[key], b[key]), key
    assert plain[0]["U"] == celled[0]["U"] and plain[1]["energy"] == celled[1]["energy"]


def test_oracle_loops_in_a_sheared_cell_follow_the_unsheared_run(oracle, blob):
    """A tilt of the second lattice vector by a whole first one (24) spans the same lattice: the same physical system,
    wrapped into a 45-degree cell.  The unwrapped displacements of both loops agree with the unsheared run to the suite's
    short-trajectory tolerance, and the sheared run's coordinates stay inside the sheared cell (wrap_tric, not wrap1,
    was applied).

    (sheared(blob, 6.0), the general cell of the audits, is NOT the same system: the gas sits on a JITTERED grid of
    spacing 2, gas particles one spacing inside opposite y faces interact across them, and a tilt of three grid units
    pairs each with another, differently jittered partner.  Its 10-step Brownian displacements differ from the
    unsheared run's by 3e-4.  It serves as a general cell, not as a copy.)"""
    sh = sheared(blob, 24.0)
    pot = oracle.make_pot(sa.POT_LJ, LJ)
    U = sh["cell"]
    plain = _both_loops(oracle, blob, pot, 2.5, 10)
    with oracle.set_cell(U):
        tilted = _both_loops(oracle, sh, pot, 2.5, 10)
    for a, b in zip(plain, tilted):
        da = _unwrapped(a, np.diag(blob["box"])) - blob["x"]
        db = _unwrapped(b, U) - sh["x"]
        assert np.abs(da - db).max() <= sa.SHORT_TOL
        fr = np.linalg.solve(U, b["x"].T).T
        assert fr.min() >= -1e-12 and fr.max() < 1.0 + 1e-12
        assert np.abs(a["f"] - b["f"]).max() <= 1e-9 * max(1.0, np.abs(a["f"]).max())
    assert np.abs(plain[0]["x"] - blob["x"]).max() > 1e-3 and np.abs(plain[1]["x"] - blob["x"]).max() > 1e-6
    moved = np.flatnonzero((tilted[0]["img"] != sh["img"]).any(axis=1))
    assert moved.size >= 1                           # some particle crossed a face of the sheared cell


# ------------------------------------------------------------------------------------------- the restatements
def test_philox_np_is_the_oracles_block(oracle):
    rng = np.random.default_rng(8)
    c = rng.integers(0, 2 ** 32, size=(16, 4), dtype=np.uint64)
    k = rng.integers(0, 2 ** 32, size=(16, 2), dtype=np.uint64)
    c[0], k[0] = 0, 0
    c[1], k[1] = 0xFFFFFFFF, 0xFFFFFFFF
    w = np.stack(sa.philox_np(c[:, 0], c[:, 1], c[:, 2], c[:, 3], k[:, 0], k[:, 1]), axis=1)
    for i in range(16):
        assert [int(v) for v in w[i]] == oracle.philox(c[i], k[i])


@pytest.mark.parametrize("name", ["blob", "blob_sheared"])
def test_fire_restated_follows_the_oracle(oracle, name):
    """14 steps with dt increases (nmin = 0): the numpy restatement against the C loop, at 1e-13 on x; step counts,
    images, energy and f_rms with it."""
    s, pot, cutoff, _, fire_kw = _case(oracle, name)
    cell = s.get("cell")
    U = sa.cell_matrix(s["box"], cell)
    import contextlib
    with (oracle.set_cell(cell) if cell is not None else contextlib.nullcontext()):
        ref = oracle.fire_minimize(s["x"], s["img"], s["diam"], s["box"], cutoff, pot, max_steps=14, tol=sa.NEVER,
                                   use_cells=False, nthreads=1, **fire_kw)
        got = sa.FireRestated(oracle, s["box"], cutoff, pot, s["diam"], cell).run(s["x"], s["img"], 14, sa.NEVER, **fire_kw)
    assert got["steps"] == ref["steps"] == 14 and not got["converged"] and len(got["trace"]) == 14 and len(got["hist"]) == 15
    assert np.abs(_unwrapped(got, U) - _unwrapped(ref, U)).max() <= 1e-13
    assert np.array_equal(got["img"], ref["img"])
    assert abs(got["energy"] - ref["energy"]) <= 1e-12 * abs(ref["energy"])
    assert abs(got["f_rms"] - ref["f_rms"]) <= 1e-12 * ref["f_rms"]
    assert {t["branch"] for t in got["trace"]} >= {"accelerate"} and got["trace"][-1]["dt"] > fire_kw["dt_initial"]


def test_pick_tolerance():
    r = [5.0, 4.0, 4.5, 3.0, 3.0 * (1 - 1e-8)]
    assert sa.pick_tolerance(r, 1) == 10.0
    assert sa.pick_tolerance(r, 2) == 4.5
    assert sa.pick_tolerance(r, 3) is None            # not the smallest so far: evaluation 2 would converge first
    assert sa.pick_tolerance(r, 4) == 3.5
    assert sa.pick_tolerance(r, 5) is None            # gap below 1e-6


# ------------------------------------------------------------------------------------------- the honest steppers
def _brownian(oracle, stepper_cls, name, schedule, **kw):
    s, pot, cutoff, dt, _ = _case(oracle, name)
    cell = s.get("cell")
    stepper = stepper_cls(oracle, s["box"], cutoff, pot, cell)
    kt = kw.pop("ktemp", KT)
    return sa.audit_brownian(stepper, oracle, s, pot, cutoff, dt, kt, SEED, schedule, cell=cell, **kw)


def _fire(oracle, name, restated=None, stepper_cls=sa.OracleFireStepper, schedule=sa.FIRE_MIXED, convergence=False, **kw):
    s, pot, cutoff, _, fire_kw = _case(oracle, name)
    cell = s.get("cell")
    stepper = stepper_cls(oracle, s["box"], cutoff, pot, cell, restated=restated)
    if convergence:
        return sa.audit_fire_convergence(stepper, oracle, s, pot, cutoff, fire_kw, cell=cell, **kw)
    return sa.audit_fire(stepper, oracle, s, pot, cutoff, fire_kw, schedule, cell=cell, **kw)


@pytest.mark.parametrize("schedule", ["BD_MIXED", "BD_CHUNKS"])
@pytest.mark.parametrize("name", list(CASES))
def test_oracle_brownian_stepper_passes(oracle, name, schedule):
    """Every error exactly zero -- the stepper's numpy move, wrap and Philox block are the oracle's, bit for bit --
    with no knife-edge particle and no image exception on the oracle's own trajectory (the caps are for the device)."""
    sched = getattr(sa, schedule)
    res = _brownian(oracle, sa.OracleBrownianStepper, name, sched, first_step=HIGH if name == "tiny65" else 0,
                    virial_every=7 if name == "poly_2d" else 10)
    assert res["failures"] == [] and res["excluded"] == [] and res["image_exceptions"] == []
    assert all(v == 0.0 for v in res["worst"].values()), res["worst"]
    assert res["stats"]["steps"] == sum(sched) and [g["k"] for g in res["segments"]] == list(sched)


@pytest.mark.parametrize("name", list(CASES))
def test_oracle_fire_stepper_passes(oracle, name):
    """oracle.fire_minimize against the numpy restatement: within every bound (the sums differ in their last bits), the
    restatement alone taking a dt increase and, on the blob, a reset in a segment of at most 14 steps, and the three
    convergence points found."""
    res = _fire(oracle, name)
    assert res["failures"] == [] and res["excluded"] == [] and res["image_exceptions"] == []
    assert max(res["worst"].values()) <= 0.05, res["worst"]
    if name.startswith("blob"):         # (a reset from rest needs a start near a minimum: the crystallite)
        assert any("reset" in g["branches"] for g in res["segments"] if g["k"] <= 14), res["segments"]
    assert any("accelerate" in g["branches"] for g in res["segments"])
    conv = _fire(oracle, name, convergence=True)
    assert conv["failures"] == [] and [g["steps"] for g in conv["segments"]] == [g["j"] for g in conv["segments"]]
    js = [g["j"] for g in conv["segments"]]
    assert js[0] == 1 and 2 <= js[1] < 32 and js[2] >= 2, js


# ------------------------------------------------------------------------------------------- the sabotaged steppers
class StaleRowBD(sa.OracleBrownianStepper):
    """From the third step of a call on, the forces come from a row cut at 2.4: the neighbours between 2.4 and 2.5 are
    lost once the row has aged.  One-step segments, and the first two steps of any segment, are whole."""

    def forces(self, x, t):
        if t < 2:
            return super().forces(x, t)
        f, u, w, _ = self.o.forces_brute(x, self.box, 2.4, self.pot, self.diam)
        return f, u, w


class SlotNoise(sa.OracleBrownianStepper):
    """The noise counter holds the storage slot instead of the particle id (the stepper sorts its particles)."""

    def noise_ids(self):
        return np.random.default_rng(1).permutation(len(self.x))


class FirstStepIgnored(sa.OracleBrownianStepper):
    def counter(self, g, first_step, t):
        return super().counter(t, 0, t)


class HighCounterDropped(sa.OracleBrownianStepper):
    def counter(self, g, first_step, t):
        return g & 0xFFFFFFFF, 0


class HighSeedDropped(sa.OracleBrownianStepper):
    def key(self, seed):
        return seed & 0xFFFFFFFF, 0


class TimesKT(sa.OracleBrownianStepper):
    def mobility(self, dt, ktemp, f):
        return f * dt * ktemp


class NoWrap(sa.OracleBrownianStepper):
    """The move without the wrap: the coordinates leave the cell and the image counters never change."""

    def wrap(self, x, img):
        return x, img


class LocalVirial(sa.OracleBrownianStepper):
    def samples(self, g, t, virial_every):
        return t % virial_every == 0


@pytest.mark.parametrize("label,stepper,name,kw,check,what,segment", [
    # segment 4 is the first with more than two steps (global steps 5 .. 9): its last evaluation lacks pairs -> (A)
    ("stale row", StaleRowBD, "blob", {}, "A", "F", 4),
    ("noise by slot", SlotNoise, "blob", {}, "B", "x", 0),
    # the first segment starts at 0 either way; the second continues at global step 1
    ("first_step ignored", FirstStepIgnored, "blob", {}, "B", "x", 1),
    # segments 0 and 1 are steps 2^32 - 3 and 2^32 - 2; segment 2 holds 2^32 - 1 and 2^32, the first with a high word
    ("high counter word", HighCounterDropped, "tiny65", dict(first_step=HIGH), "B", "x", 2),
    ("high seed word", HighSeedDropped, "tiny65", {}, "B", "x", 0),
    ("f dt kT", TimesKT, "blob", {}, "B", "x", 0),
    # tiny_system's particle 0 sits 0.05 from three faces and crosses one within the first steps; unwrapped, its
    # coordinate is right -- only the image counters (and the cell it claims to be in) are wrong
    ("no wrap at a face", NoWrap, "tiny65", {}, "B", "img", None),
    # segment 1 is the single global step 1: local step 0 samples, global step 1 does not
    ("virial on the local step", LocalVirial, "blob", {}, "V", "count", 1),
])
def test_sabotaged_brownian_steppers_fail(oracle, label, stepper, name, kw, check, what, segment):
    with pytest.raises(sa.AuditFailure) as e:
        _brownian(oracle, stepper, name, sa.BD_MIXED, **kw)
    assert (e.value.check, e.value.what) == (check, what), str(e.value)
    if segment is not None:
        assert ("segment %d " % segment) in str(e.value), str(e.value)


def test_brownian_kt_enters_the_audit(oracle):
    """f dt kT and f dt / kT are the same at kT = 1: the sabotage above is seen because the audit runs at 1.5."""
    res = _brownian(oracle, TimesKT, "tiny65", sa.BD_MIXED[:4], ktemp=1.0, raise_on_failure=False)
    assert max(res["worst"].values()) <= 1.0 and res["failures"] == []


class MixAfterSign(sa.FireRestated):
    """The velocity mix applied after the sign test: it sees the alpha the test has already updated."""
    mix_first = False


class OldDtDrift(sa.FireRestated):
    def drift(self, x, img, v, dt_new, dt_old):
        return super().drift(x, img, v, dt_old, dt_old)


class MovesOnConvergence(sa.FireRestated):
    def converging_step(self, x, img, v, f, dt):
        return self.drift(x, img, v + dt * f, dt, dt)


class VelocitiesLost(sa.OracleFireStepper):
    def restore_velocities(self, v):
        pass


@pytest.mark.parametrize("label,restated,stepper,convergence,check,what", [
    # with nmin = 0 alpha changes on every accelerating step; the first step's v is parallel to f, so the mix first
    # matters on the second step of a segment
    ("mix after the sign test", MixAfterSign, sa.OracleFireStepper, False, "B", "x"),
    # dt grows on the very first step: x is off by 0.2 dt^2 f
    ("drift with the old dt", OldDtDrift, sa.OracleFireStepper, False, "B", "x"),
    ("x moved on the converging step", MovesOnConvergence, sa.OracleFireStepper, True, "C", "x"),
    ("MD velocities not restored", None, VelocitiesLost, False, "B", "v"),
])
def test_sabotaged_fire_steppers_fail(oracle, label, restated, stepper, convergence, check, what):
    with pytest.raises(sa.AuditFailure) as e:
        _fire(oracle, "blob", restated=restated, stepper_cls=stepper, convergence=convergence)
    assert (e.value.check, e.value.what) == (check, what), str(e.value)


def test_restated_fire_stepper_passes_unsabotaged(oracle):
    """The sabotaged FIRE steppers run FireRestated subclasses; the plain class passes with exactly zero x error."""
    res = _fire(oracle, "tiny65", restated=sa.FireRestated)
    assert res["failures"] == [] and res["worst"]["x1"] == res["worst"]["x"] == res["worst"]["xl"] == 0.0
