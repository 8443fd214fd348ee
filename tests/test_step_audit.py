"""The step audit (tests/step_audit.py) proved on the CPU: a stepper made of the oracle's own step functions passes it with
zero error and nothing excluded, and three sabotaged steppers -- the faults the audit exists to find -- each fail it, on the
assertion stated here."""
import numpy as np
import pytest

from tests import step_audit as sa
from tests.util import blob_gas_system, poly_system

LJ = [1.0, 1.0, 2.5]
EIGHTY = sa.MIXED + (1,)      # segments end at steps 1 2 4 5 10 11 20 21 24 25 39 40 47 48 58 59 65 66 78 79 80
assert sum(EIGHTY) == 80


@pytest.fixture(scope="module")
def blob():
    return blob_gas_system()


def _audit(oracle, stepper_cls, s, kind, params, cutoff, dt, schedule=EIGHTY, **kw):
    pot = oracle.make_pot(kind, params)
    stepper = stepper_cls(oracle, s["box"], cutoff, pot)
    return sa.audit_run(stepper, oracle, s, pot, cutoff, dt, schedule, **kw)


def test_blob_gas_system_is_ragged(blob):
    """What the system is for: n = 849 is neither a multiple of the wave nor of the tile, rows of every length from empty
    to a crystal's share tiles, and it is deterministic."""
    s = blob
    assert s["n"] == 849 == 13 * 64 + 17 == 3 * 256 + 81
    d2 = sa.pair_d2(s["x"], s["box"])
    np.fill_diagonal(d2, np.inf)
    nn = (d2 <= 6.25).sum(axis=1)
    assert nn.min() == 0 and nn.max() >= 50 and 40 <= (nn == 0).sum() <= 110
    assert len(set(nn % 4)) == 4                      # inner-row tail words of every kind
    assert d2.min() >= 1.0                            # no overlaps: gas and crystallite included
    assert np.array_equal(s["x"], blob_gas_system()["x"])


@pytest.mark.parametrize("name", ["blob", "poly_2d"])
def test_oracle_stepper_passes_80_steps(oracle, blob, name):
    """The honest stepper: every error is exactly zero (the shadow step repeats the same arithmetic), no particle of the
    oracle's own 80-step trajectory sits on a knife edge, no image exception, and both thermo kinds are audited on
    one-step and on longer segments."""
    if name == "blob":
        res = _audit(oracle, sa.OracleStepper, blob, sa.POT_LJ, LJ, 2.5, 0.004)
    else:
        res = _audit(oracle, sa.OracleStepper, poly_system(), sa.POT_POLYDISPERSE, [1.25, 0.2], 1.25 * 1.2, 0.005)
    assert res["failures"] == [] and res["excluded"] == [] and res["image_exceptions"] == []
    assert all(v == 0.0 for v in res["worst"].values()), res["worst"]
    assert res["stats"]["steps"] == 80 and len(res["segments"]) == len(EIGHTY)
    flags = {(s["k"] == 1, s["thermo"]) for s in res["segments"]}
    assert flags == {(True, True), (True, False), (False, True), (False, False)}


def test_oracle_stepper_passes_under_nvt(oracle, blob):
    """The thermostat draws are sliced per segment for the stepper and for the shadow step alike."""
    nf = 3 * (blob["n"] - 1.0)
    rng = np.random.default_rng(5)
    r1, r2 = rng.standard_normal(80), 2.0 * rng.gamma((nf - 1) / 2, size=80)
    res = _audit(oracle, sa.OracleStepper, blob, sa.POT_LJ, LJ, 2.5, 0.004, ensemble=sa.NVT, tau=0.1,
                 ktemp=np.full(80, 0.8), r1=r1, r2=r2)
    assert res["failures"] == [] and res["worst"]["x1"] == 0.0 and res["worst"]["v1"] == 0.0 and res["worst"]["K"] <= 1.0


class StaleRow(sa.OracleStepper):
    """Every fourth step evaluates its forces with the list cut at 2.4 instead of 2.5: a stale inner row that has lost
    the neighbours between 2.4 and 2.5."""

    def forces(self, x):
        if (self.step + 1) % 4:
            return super().forces(x)
        f, u, w, _ = self.o.forces_brute(x, self.box, 2.4, self.pot, self.diam)
        return f, u, w


def bump_at(step, particle=0, comp=1, amount=0.039):
    class ForceBump(sa.OracleStepper):
        """|F(r_c)| = 0.039 added to one force component of one particle on one step: one neighbour too many (or few)."""

        def forces(self, x):
            f, u, w = super().forces(x)
            if self.step + 1 == step:
                f[particle, comp] += amount
            return f, u, w
    return ForceBump


def double_drift_at(step):
    class DoubleDrift(sa.OracleStepper):
        """The drift of one step applied twice (x += v dt again, wrapped): the forces are then evaluated at the drifted
        positions, so the state stays self-consistent -- only the shadow step can see it."""

        def drift(self, dt):
            super().drift(dt)
            if self.step + 1 == step:
                self.o.integrate_half(self.x, self.img, self.v, np.zeros_like(self.f), dt, self.box)
    return DoubleDrift


@pytest.mark.parametrize("label,stepper,check,what", [
    # step 4 ends the segment (3, 4): its forces are the audited ones and lack the pairs between 2.4 and 2.5 -> (A)
    ("stale row, audited step", StaleRow, "A", "F"),
    # step 5 is a one-step segment: the bumped force is the audited one -> (A)
    ("force bump, audited step", bump_at(5), "A", "F"),
    # step 7 is in the middle of the segment (6 .. 10): the forces at its end are whole again, but the bump went through
    # the second half kick of step 7 and the first of step 8, dv = 0.039 dt = 1.6e-4, and from there into x (1.9e-6 by
    # step 10) -> (B), on x and on v; x is reported first
    ("force bump, inside a segment", bump_at(7), "B", "x"),
    # step 11 is a one-step segment: x is off by v dt, against the derived bound 8 spacing(L) = 2.8e-14 -> (B) on x
    ("double drift, one-step segment", double_drift_at(11), "B", "x"),
    # step 8 is inside (6 .. 10): x off by v dt ~ 1e-2 against 1e-10 -> (B) on x; (A) cannot see it
    ("double drift, inside a segment", double_drift_at(8), "B", "x"),
])
def test_sabotaged_steppers_fail(oracle, blob, label, stepper, check, what):
    with pytest.raises(sa.AuditFailure) as e:
        _audit(oracle, stepper, blob, sa.POT_LJ, LJ, 2.5, 0.004)
    assert (e.value.check, e.value.what) == (check, what), str(e.value)
    # the whole picture without stopping at the first miss: (A) stays clean for the double drift, whatever the step
    res = _audit(oracle, stepper, blob, sa.POT_LJ, LJ, 2.5, 0.004, schedule=EIGHTY[:6], raise_on_failure=False)
    checks = {f.check for f in res["failures"]}
    assert check in checks and ("Drift" not in stepper.__name__ or "A" not in checks), [str(f) for f in res["failures"]]
    if "inside" in label:
        assert {f.what for f in res["failures"]} >= {"x", "v"}


def test_stale_row_is_seen_only_by_force_completeness_when_it_ages(oracle, blob):
    """The reason for (A): inside the 14-step segment (26 .. 39) no shadow step runs, and a stale row on the segment's
    LAST step alone (step 39) leaves x and v of that segment untouched but for the last half kick -- only the force
    comparison at the stepper's own positions finds it."""
    class StaleAt39(sa.OracleStepper):
        def forces(self, x):
            if self.step + 1 != 39:
                return super().forces(x)
            f, u, w, _ = self.o.forces_brute(x, self.box, 2.4, self.pot, self.diam)
            return f, u, w
    with pytest.raises(sa.AuditFailure) as e:
        _audit(oracle, StaleAt39, blob, sa.POT_LJ, LJ, 2.5, 0.004)
    assert e.value.check == "A" and "steps 25..38" in str(e.value)


def test_knife_edge_pairs_are_found_and_capped(oracle):
    """Two isolated dimers at d2 == cutoff^2 exactly: their four particles are left out of (A), which is more than the cap of
    two allows; one ulp-scale step further away from the threshold than 1e-9 relative, nothing is excluded."""
    box = np.full(3, 30.0)
    x = np.array([[5.0, 5.0, 5.0], [7.5, 5.0, 5.0], [20.0, 20.0, 5.0], [20.0, 22.5, 5.0]])
    thr = [6.25]
    assert list(sa.knife_edge_particles(x, box, None, thr)) == [0, 1, 2, 3]
    far = x.copy()
    far[1, 0] += 2.5 * 1e-8
    assert list(sa.knife_edge_particles(far, box, None, thr)) == [2, 3]
    # through a periodic face, and in a general cell that is the same lattice
    xf = np.array([[0.5, 5.0, 5.0], [28.0, 5.0, 5.0]])
    assert list(sa.knife_edge_particles(xf, box, None, thr)) == [0, 1]
    assert list(sa.knife_edge_particles(xf, box, np.diag(box), thr)) == [0, 1]
    s = dict(n=4, dim=3, box=box, x=x, v=np.zeros_like(x), img=np.zeros((4, 3), np.int32), diam=np.ones(4))
    with pytest.raises(sa.AuditFailure) as e:
        _audit(oracle, sa.OracleStepper, s, sa.POT_LJ, LJ, 2.5, 1e-6, schedule=(1,))
    assert e.value.check == "precondition"


def test_pair_thresholds_name_the_potentials_own_cutoff(oracle):
    diam = np.array([1.0, 0.8])
    assert sa.pair_thresholds(oracle.make_pot(sa.POT_LJ, [1.0, 1.0, 2.2]), 2.5, diam) == [6.25, 2.2 ** 2]
    assert sa.pair_thresholds(oracle.make_pot(sa.POT_PSEUDOHS, [50.0]), 1.5, diam) == [2.25, sa.PSEUDOHS_B ** 2]
    t = sa.pair_thresholds(oracle.make_pot(sa.POT_POLYDISPERSE, [1.25, 0.2]), 1.5, diam)[1]
    se = 0.9 * (1.0 - 0.2 * 0.2)
    assert t.shape == (2, 2) and abs(t[0, 1] - (1.25 * se) ** 2) < 1e-15
    # ... which is where the oracle's potential really switches off
    for r, on in ((2.2 * (1 - 1e-9), True), (2.2 * (1 + 1e-9), False)):
        assert (oracle.evaluate(oracle.make_pot(sa.POT_LJ, [1.0, 1.0, 2.2]), r, 1.0, 1.0)[1] != 0.0) == on
