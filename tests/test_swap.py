"""CPU: the properties of a swap round that together imply detailed balance, checked on the numpy +
oracle reference (tests/swap_reference.py) that the device is compared with in tests/test_gpu_swap.py; the fairness
conditions of that comparison at the committed seeds; and the host side -- SwapMonteCarlo's argument checks and
run_simulation(..., swap=...) on a fake handle, in the style of tests/test_sampler_protocol.py."""
import os

import numpy as np
import pytest

import moleculardynamics.jl_amd as md
from tests import swap_reference as sr
from tests.test_sampler_protocol import N, _fake_state

CASES = ("poly", "lj", "lj_sheared")
_cache = {}


def reference(name):
    """The case, its Frame and the 8 reference rounds from round 0 -- computed once, shared, never changed."""
    if name not in _cache:
        c = sr.case(name)
        fr = sr.Frame(c["system"], c["cutoff"], c["pot"])
        rounds = sr.run_rounds(fr, c["system"]["diam"], c["seed"], 0, sr.ROUNDS, c["fraction"], c["ktemp"])
        _cache[name] = (c, fr, rounds)
    return _cache[name]


@pytest.mark.parametrize("name", CASES)
def test_seed_meets_the_fairness_conditions(name):
    c, _, rounds = reference(name)
    ok, text = sr.conditions(rounds, c["ktemp"])
    print(name, text)
    assert ok, text


@pytest.mark.parametrize("name", CASES)
def test_selection_does_not_depend_on_the_diameters(name):
    """(a) Same positions and seed, two diameter assignments: the same proposers, partners, live and blocked sets."""
    c, fr, rounds = reference(name)
    other = np.random.default_rng(5).permutation(c["system"]["diam"])
    for r in range(3):
        p0, s0, _ = sr.selection(fr, c["seed"], r, c["fraction"])
        b = sr.swap_round(fr, other, c["seed"], r, c["fraction"], c["ktemp"])
        a = rounds[r] if r == 0 else sr.swap_round(fr, c["system"]["diam"], c["seed"], r, c["fraction"], c["ktemp"])
        for x in (a, b):
            assert np.array_equal(x["partner"], p0)
            undecided = s0 != -1
            assert np.array_equal(x["status"][undecided], s0[undecided])            # none, void, lost, blocked
            assert np.all(x["status"][~undecided] >= sr.REJECTED)                   # the survivors were decided


@pytest.mark.parametrize("name", CASES)
def test_accepted_swaps_do_not_interact(name):
    """(b) The sum of dU over a round's accepted swaps is U_after - U_before."""
    c, fr, rounds = reference(name)
    diam = c["system"]["diam"]
    for r in rounds[:4]:
        acc = r["status"] == sr.ACCEPTED
        u0 = sr.total_energy(c["system"], c["cutoff"], c["pot"], diam)
        u1 = sr.total_energy(c["system"], c["cutoff"], c["pot"], r["diam"])
        assert abs(r["du"][acc].sum() - (u1 - u0)) <= 1e-12 * r["S"][acc].sum()
        diam = r["diam"]
    assert sum((r["status"] == sr.ACCEPTED).sum() for r in rounds[:4]) >= 3


@pytest.mark.parametrize("name", CASES)
def test_a_swap_is_an_involution(name):
    """(c) Re-running a round's accepted swaps from the new state gives -dU each."""
    c, fr, rounds = reference(name)
    r = rounds[0]
    for i in np.flatnonzero(r["status"] == sr.ACCEPTED):
        j = int(r["partner"][i])
        (da, sa), (db, sb) = fr.half(int(i), j, r["diam"]), fr.half(j, int(i), r["diam"])
        assert abs((da + db) + r["du"][i]) <= 1e-12 * r["S"][i]
        assert abs((sa + sb) - r["S"][i]) <= 1e-12 * r["S"][i]


@pytest.mark.parametrize("name", ["poly", "lj"])
def test_temperature_limits(name):
    """(d) kT = 1e12 accepts every decided swap; kT = 1e-12 never raises U."""
    c, fr, _ = reference(name)
    nacc = nrej = 0
    for r in range(4):
        hot = sr.swap_round(fr, c["system"]["diam"], c["seed"], r, c["fraction"], 1e12)
        assert not np.any(hot["status"] == sr.REJECTED)
        cold = sr.swap_round(fr, c["system"]["diam"], c["seed"], r, c["fraction"], 1e-12)
        assert np.array_equal(cold["status"] >= sr.REJECTED, hot["status"] == sr.ACCEPTED)      # the same decided swaps
        assert np.all(cold["du"][cold["status"] == sr.ACCEPTED] <= 0.0)
        assert np.all(cold["du"][cold["status"] == sr.REJECTED] > 0.0)
        nacc += (hot["status"] == sr.ACCEPTED).sum()
        nrej += (cold["status"] == sr.REJECTED).sum()
    assert nacc >= 10 and nrej >= 1


def test_filter_is_applied_after_the_selection():
    c, fr, rounds = reference("poly")
    f = sr.swap_round(fr, c["system"]["diam"], c["seed"], 0, c["fraction"], c["ktemp"], max_diff=0.05)
    a = rounds[0]
    d = c["system"]["diam"]
    assert np.array_equal(f["partner"], a["partner"])
    assert np.array_equal(f["status"] <= sr.BLOCKED, a["status"] <= sr.BLOCKED)
    assert np.array_equal(f["status"][f["status"] <= sr.BLOCKED], a["status"][a["status"] <= sr.BLOCKED])
    assert np.any(f["status"] == sr.FILTERED)
    for i in np.flatnonzero(f["status"] >= sr.REJECTED):
        assert abs(d[i] - d[f["partner"][i]]) <= 0.05


def test_threshold_is_integer():
    assert sr.threshold(1.0) == 2 ** 32 - 1 and sr.threshold(0.5) == 2 ** 31 and sr.threshold(1e-12) == 0


# ---------------------------------------------------------------------------------------------------------------------
# Host API
# ---------------------------------------------------------------------------------------------------------------------
def test_argument_checks():
    for kw in (dict(every=0, rounds=1), dict(every=1, rounds=0), dict(every=1, rounds=1, fraction=0.0),
               dict(every=1, rounds=1, fraction=1.5), dict(every=1, rounds=1, max_diameter_difference=0.0),
               dict(every=1, rounds=1, ktemp=0.0), dict(every=1, rounds=1, ktemp=float("inf"))):
        with pytest.raises(ValueError):
            md.SwapMonteCarlo(**kw)
    s = md.SwapMonteCarlo(10, 4)
    assert 0.0 < s.fraction <= 1.0 and s.max_diameter_difference is None and s.rounds_done == 0 and s.blocks == []


class _SwapFake:
    """tests/test_sampler_protocol.py's fake handle plus the four swap calls."""

    def __init__(self, dev):
        self.__dict__["dev"] = dev
        self.__dict__["diam"] = np.linspace(0.8, 1.2, N)
        self.__dict__["calls"] = []

    def __getattr__(self, k):
        return getattr(self.dev, k)

    def swap_setup(self, fraction, max_diameter_difference=None, seed=0):
        self.dev.setups.append("swap_setup")
        self.calls.append(("setup", fraction, max_diameter_difference, seed))

    def swap_rounds(self, nrounds, ktemp, first_round=0):
        self.dev._log("swap_rounds", int(nrounds), float(ktemp), int(first_round))
        self.__dict__["diam"] = np.roll(self.diam, 1)
        return dict(proposed=4, void=0, lost=0, blocked=1, filtered=0, accepted=2, decided=3, du_accepted=-0.5, U=-7.0,
                    W=1.0)

    def diameters(self):
        return self.diam.copy()


def test_nve_without_ktemp_is_refused(tmp_path):
    state, dev = _fake_state()
    state.system.device = _SwapFake(dev)
    params = md.Parameters(1.0, N, 0.002, md.LennardJones())
    with pytest.raises(ValueError, match="ktemp"):
        md.run_simulation(state, params, md.NVE(), 10, 5, str(tmp_path), swap=md.SwapMonteCarlo(5, 2))


def test_run_simulation_with_and_without_swap(tmp_path):
    """swap=None leaves the call sequence alone; with swap the stops are added, the block follows every sampler of its
    step, the round counter continues, state.diameters follows the device."""
    params = md.Parameters(1.0, N, 0.002, md.LennardJones())
    total, f = 20, 7

    def go(swap, sub):
        state, dev = _fake_state()
        fake = _SwapFake(dev)
        state.system.device = fake
        with np.errstate(all="ignore"):
            md.run_simulation(state, params, md.NVE(), total, f, str(tmp_path / sub), rdf=md.RadialDistribution(1.0, 4),
                              stress=md.StressTensor(6), swap=swap)
        return state, dev, fake

    _, plain, _ = go(None, "a")
    assert not any(m.startswith("swap") for _, m, _ in plain.trace) and "swap_setup" not in plain.setups
    assert set(os.listdir(tmp_path / "a")) == {"thermo.txt", "trajectory.xyz", "final.xyz", "rdf.txt", "stress.txt"}
    assert list(np.cumsum(plain.segments) - 1) == [0, 6, 7, 12, 14, 18, 19]

    swap = md.SwapMonteCarlo(6, 3, fraction=0.25, ktemp=0.7, seed=99)
    state, dev, fake = go(swap, "b")
    assert fake.calls == [("setup", 0.25, None, 99)]
    # after steps 5, 11, 17 (6, 12, 18 steps done); step 5 and 11, 17 are new stops
    assert [t for t in dev.trace if t[1] == "swap_rounds"] == [(5, "swap_rounds", (3, 0.7, 0)), (11, "swap_rounds", (3, 0.7, 3)),
                                                                (17, "swap_rounds", (3, 0.7, 6))]
    assert list(np.cumsum(dev.segments) - 1) == [0, 5, 6, 7, 11, 12, 14, 17, 18, 19]
    assert [t for t in dev.trace if not t[1].startswith("swap")] == plain.trace
    assert swap.rounds_done == 9 and len(swap.blocks) == 3 and swap.acceptance() == pytest.approx(2 / 3)
    assert np.array_equal(state.diameters, fake.diam) and np.array_equal(fake.diam, np.roll(np.linspace(0.8, 1.2, N), 3))
    rows = open(tmp_path / "b" / "swap.txt").read().splitlines()
    assert rows[0] == "# step proposed blocked decided accepted acceptance dU_accepted U" and len(rows) == 4
    assert rows[1].split()[:5] == ["5", "4", "1", "3", "2"]
    # a shared stop: the block comes after the samplers of its step
    swap2 = md.SwapMonteCarlo(7, 1, ktemp=0.7, seed=1)
    _, dev2, _ = go(swap2, "c")
    at6 = [m for s, m, _ in dev2.trace if s == 6]
    assert at6 == ["stress_sample", "swap_rounds"]
    at13 = [m for s, m, _ in dev2.trace if s == 13]
    assert at13 == ["swap_rounds"]


def test_nvt_takes_the_target_temperature(tmp_path):
    state, dev = _fake_state()
    state.system.device = _SwapFake(dev)
    state.velocities = np.zeros((N, 3))
    params = md.Parameters(1.0, N, 0.002, md.LennardJones())
    swap = md.SwapMonteCarlo(4, 2)
    md.run_simulation(state, params, md.NVT(lambda step: 0.5 + 0.01 * step, 0.1), 8, 100, str(tmp_path), swap=swap)
    got = [a for _, m, a in dev.trace if m == "swap_rounds"]
    assert got == [(2, pytest.approx(0.5 + 0.01 * 4), 0), (2, pytest.approx(0.5 + 0.01 * 8), 2)]
    assert swap.seed is not None
