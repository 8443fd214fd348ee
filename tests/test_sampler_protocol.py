"""CPU: run_simulation with the first four device samplers at once, and with all ten and swap at once, on a fake handle that
records every call.  The expected
trace is worked out here by walking the steps with each sampler's documented rule, through public names only, so the
test says what the driver does at which step whatever the plumbing between run_simulation and the samplers looks like."""
import math
import os
import types

import numpy as np
import pytest

import moleculardynamics.jl_amd as md

N, DIM = 8, 3


class _FakeDevice:
    """Records the segment lengths and an ordered trace of (last completed step, method, args)."""

    def __init__(self):
        self.n, self.dim = N, DIM
        self.step = 0
        self.segments, self.trace, self.setups = [], [], []

    def _log(self, method, *args):
        self.trace.append((self.step - 1, method, args))

    def set_potential(self, kind, params):
        pass

    def upload(self, **kw):
        pass

    def run(self, nsteps, dt, *a, **kw):
        self.segments.append(nsteps)
        self.step += nsteps
        return 0.0, 0.0, 1.0

    def download(self):
        z = np.zeros((N, DIM))
        return z, z, z, np.zeros((N, DIM), dtype=np.int32)

    def snapshot_begin(self):
        self._log("snapshot_begin")

    def snapshot_end(self):
        return np.zeros((N, DIM)), np.zeros((N, DIM), dtype=np.int32)

    def _count(self, method):
        return sum(1 for _, m, _ in self.trace if m == method)

    # g(r)
    def rdf_setup(self, r_max, nbins):
        self.setups.append("rdf_setup")
        self.rdf_nbins = nbins

    def rdf_sample(self):
        self._log("rdf_sample")

    def rdf_read(self):
        return np.zeros(self.rdf_nbins, dtype=np.int64), self._count("rdf_sample")

    # self dynamics
    def dyn_setup(self, nslots, nrows, q=(), r_max=0.0, nbins=0):
        self.setups.append("dyn_setup")
        self.dyn_shape = (nrows, len(q), nbins)

    def dyn_sample(self, slots, rows):
        self._log("dyn_sample", tuple(int(v) for v in slots), tuple(int(v) for v in rows))

    def dyn_origin(self, slot):
        self._log("dyn_origin", int(slot))

    def dyn_read(self):
        nrows, nq, nbins = self.dyn_shape
        return np.zeros(nrows, dtype=np.int64), np.zeros((nrows, 2 + nq)), np.zeros((nrows, nbins), dtype=np.int64)

    # density modes
    def sq_setup(self, n, nslots=0, nrows=0):
        self.setups.append("sq_setup")
        self.sq_shape = (len(n), nrows)

    def sq_sample(self, static=True, slots=(), rows=(), origin=None):
        self._log("sq_sample", bool(static), tuple(int(v) for v in slots), tuple(int(v) for v in rows),
                  None if origin is None else int(origin))

    def sq_read(self):
        nvec, nrows = self.sq_shape
        return 0, np.zeros(nvec), np.zeros(nrows, dtype=np.int64), np.zeros((nrows, nvec))

    # stress
    def stress_setup(self, nlags=0):
        self.setups.append("stress_setup")
        self.stress_nlags = nlags

    def stress_sample(self):
        self._log("stress_sample")

    def stress_read(self):
        nl = self.stress_nlags
        return self._count("stress_sample"), np.zeros(6), np.zeros(6), np.zeros(nl, dtype=np.int64), np.zeros((nl, 6))

    # currents
    def cur_setup(self, n, e, nslots=0, nrows=0, vacf=False):
        self.setups.append("cur_setup")
        self.cur_shape = (len(n), nrows, vacf)

    def cur_sample(self, static=True, slots=(), rows=(), origin=None):
        self._log("cur_sample", bool(static), tuple(int(v) for v in slots), tuple(int(v) for v in rows),
                  None if origin is None else int(origin))

    def cur_read(self):
        nvec, nrows, vacf = self.cur_shape
        return (0, np.zeros(nvec), np.zeros(nvec), np.zeros(nrows, dtype=np.int64), np.zeros((nrows, nvec)),
                np.zeros((nrows, nvec)), np.zeros(nrows + 1) if vacf else None)

    # bond order, clusters, orientational correlation
    def boo_setup(self, r_neigh, order=6, nbins=100, threshold=0.7, min_conn=7, nseries=0):
        self.setups.append("boo_setup")
        self.boo_shape = (nbins, nseries)

    def boo_sample(self):
        self._log("boo_sample")

    def boo_read(self):
        nbins, nseries = self.boo_shape
        ns = self._count("boo_sample")
        return (ns, np.zeros(8), np.zeros(nbins, dtype=np.int64), np.zeros(nbins, dtype=np.int64),
                np.zeros(33, dtype=np.int64), np.zeros(33, dtype=np.int64), np.zeros((min(ns, nseries), 8)))

    def cluster_setup(self, r_bond, members=0, max_size=1024, nseries=0):
        self.setups.append("cluster_setup")
        self.cluster_shape = (max_size, nseries)

    def cluster_sample(self):
        self._log("cluster_sample")

    def cluster_read(self):
        max_size, nseries = self.cluster_shape
        ns = self._count("cluster_sample")
        return ns, np.zeros(8, dtype=np.int64), np.zeros(max_size + 1, dtype=np.int64), np.zeros((min(ns, nseries), 8), dtype=np.int64)

    def mpc_setup(self, r_max, nbins, weights=None, tmax=None):
        self.setups.append("mpc_setup")
        self.mpc_nbins = nbins

    def mpc_sample(self):
        self._log("mpc_sample")

    def mpc_read(self):
        return self._count("mpc_sample"), np.zeros(self.mpc_nbins, dtype=np.int64), np.zeros(self.mpc_nbins), 0.0, 1.0, 0

    # cage, four-point
    def cage_setup(self, nslots, nrows, r_neigh, r_break=None, scaled=False, max_neigh=16, q=()):
        self.setups.append("cage_setup")
        self.cage_shape = (nrows, len(q))

    def cage_sample(self, slots, rows):
        self._log("cage_sample", tuple(int(v) for v in slots), tuple(int(v) for v in rows))

    def cage_origin(self, slot):
        self._log("cage_origin", int(slot))

    def cage_read(self):
        nrows, nq = self.cage_shape
        return (np.zeros(nrows, dtype=np.int64), np.zeros((nrows, 2 + nq)), np.zeros((nrows, 3), dtype=np.int64),
                np.zeros((nrows, 33), dtype=np.int64), 0)

    def chi4_setup(self, a, n=None, nslots=1, nrows=1):
        self.setups.append("chi4_setup")
        self.chi4_shape = (nrows, 0 if n is None else len(n))

    def chi4_sample(self, slots, rows):
        self._log("chi4_sample", tuple(int(v) for v in slots), tuple(int(v) for v in rows))

    def chi4_origin(self, slot):
        self._log("chi4_origin", int(slot))

    def chi4_read(self):
        nrows, nvec = self.chi4_shape
        z = np.zeros(nrows, dtype=np.int64)
        return z, z.copy(), z.copy(), np.zeros((nrows, nvec))

    # swap
    def swap_setup(self, fraction, max_diameter_difference=None, seed=0):
        self.setups.append("swap_setup")

    def swap_rounds(self, nrounds, ktemp, first_round=0):
        self._log("swap_rounds", int(nrounds), float(ktemp), int(first_round))
        return dict(proposed=0, void=0, lost=0, blocked=0, filtered=0, accepted=0, decided=0, du_accepted=0.0, U=0.0, W=0.0)

    def diameters(self):
        return np.ones(N)


def _fake_state():
    dev = _FakeDevice()
    system = types.SimpleNamespace(device=dev, positions=np.zeros((N, DIM)), xpositions=None,
                                   energy_and_forces=types.SimpleNamespace(forces=np.zeros((N, DIM)), energy=0.0,
                                                                           virial=0.0))
    state = md.SimulationState(system, np.ones(N), np.random.default_rng(1), np.diag([2.0, 2.0, 2.0]),
                               np.zeros((N, DIM)), np.zeros((N, DIM), dtype=np.int32), DIM, DIM * (N - 1.0))
    return state, dev


def _split(samples):
    return tuple(a for a, _ in samples), tuple(b for _, b in samples)


@pytest.mark.parametrize("total,lags,origin_every", [(60, [2, 5], 3), (60, None, None), (1, [2, 5], 3)])
def test_all_four_samplers_in_one_run(tmp_path, monkeypatch, total, lags, origin_every):
    monkeypatch.chdir(tmp_path)                             # log_times=True writes new-log-times.txt where it runs
    f = 7
    state, dev = _fake_state()
    params = md.Parameters(1.0, N, 0.002, md.LennardJones())
    rdf = md.RadialDistribution(1.0, 4, every=2)
    dyn = md.SelfDynamics(lags=lags, origin_every=origin_every)
    # cell edge 2: |q| = pi for the 3 vectors n = e_c, pi sqrt(2) for the 6 face diagonals of the half space
    sq = md.StructureFactor(4.5, every=3, dynamic=True, lags=lags, origin_every=origin_every)
    stress = md.StressTensor(4, nlags=2)
    out = str(tmp_path / "out")
    with np.errstate(all="ignore"):                         # all-zero sums: 0 / 0 in the normalisations
        md.run_simulation(state, params, md.NVE(), total, f, out, log_times=True, rdf=rdf, dynamics=dyn, sq=sq,
                          stress=stress)
    assert sq.n.shape == (9, 3)
    assert dev.setups == ["rdf_setup", "dyn_setup", "sq_setup", "stress_setup"]

    # the reference's log-time steps inside the run: step 0 and floor(1.35^i) (the later blocks start past 1.35^40)
    snapshots = {0} | {int(math.floor(1.35 ** i)) for i in range(41)}
    dyn_events, sq_events = dyn.schedule(total)[1], sq.schedule(total)[1]
    want, stops = [], {total - 1}
    for step in range(total):
        before = len(want)
        output = step % f == 0
        if output and (step // f) % rdf.every == 0:
            want.append((step, "rdf_sample", ()))
        ev = dyn_events.get(step)
        if ev is not None:
            if ev[0]:
                want.append((step, "dyn_sample", _split(ev[0])))
            if ev[1] is not None:
                want.append((step, "dyn_origin", (ev[1],)))
        static = output and (step // f) % sq.every == 0
        ev = sq_events.get(step)
        if static or ev is not None:
            smp, org = ev if ev is not None else ([], None)
            want.append((step, "sq_sample", (static,) + _split(smp) + (org,)))
        if step % stress.every == 0:
            want.append((step, "stress_sample", ()))
        if output or step in snapshots:                     # a trajectory frame or a snapshot
            want.append((step, "snapshot_begin", ()))
        if len(want) > before or output:                    # every step with a device call, and every output step
            stops.add(step)
    assert dev.trace == want
    assert list(np.cumsum(dev.segments) - 1) == sorted(stops)
    assert rdf.nsamples == sum(1 for t in want if t[1] == "rdf_sample")
    assert stress.nsamples == sum(1 for t in want if t[1] == "stress_sample")

    present = {"thermo.txt", "trajectory.xyz", "final.xyz", "rdf.txt", "dynamics.txt", "sq.txt", "fqt.txt", "stress.txt",
               "stress_acf.txt"} | {"snapshot.%d" % s for s in snapshots if s < total}
    assert set(os.listdir(out)) == present                  # no vanhove.txt: the SelfDynamics has no bins
    thermo = open(os.path.join(out, "thermo.txt")).read().splitlines()
    assert [int(ln.split()[0]) for ln in thermo[1:]] == list(range(0, total, f))


def test_files_that_depend_on_the_sampler(tmp_path):
    """vanhove.txt needs bins, fqt.txt needs dynamic=True, stress_acf.txt needs lags."""
    state, dev = _fake_state()
    params = md.Parameters(1.0, N, 0.002, md.LennardJones())
    out = str(tmp_path)
    with np.errstate(all="ignore"):
        md.run_simulation(state, params, md.NVE(), 5, 2, out, write_trajectory=False,
                          dynamics=md.SelfDynamics(r_max=1.0, nbins=3, lags=[1], origin_every=1),
                          sq=md.StructureFactor(4.5), stress=md.StressTensor(2))
    assert set(os.listdir(out)) == {"thermo.txt", "final.xyz", "dynamics.txt", "vanhove.txt", "sq.txt", "stress.txt"}
    assert [m for _, m, _ in dev.trace if m == "snapshot_begin"] == []
    assert list(np.cumsum(dev.segments) - 1) == [0, 1, 2, 3, 4]        # an origin at every step


def _all_ten(lags, origin_every):
    """All ten samplers and swap, by run_simulation's keywords."""
    kw = dict(lags=lags, origin_every=origin_every)
    return dict(rdf=md.RadialDistribution(1.0, 4, every=2), dynamics=md.SelfDynamics(**kw),
                sq=md.StructureFactor(4.5, every=3, dynamic=True, **kw), currents=md.CurrentCorrelations(4.5, **kw),
                stress=md.StressTensor(4, nlags=2), bond_order=md.BondOrder(0.9, order=6, every=1, nbins=5),
                clusters=md.ClusterAnalysis(0.9, members="solid", every=2, max_size=8),
                cage=md.CageDynamics(0.9, **kw), four_point=md.FourPoint(0.3, q_max=4.5, **kw),
                orientational=md.OrientationalCorrelation(0.9, 3, every=3), swap=md.SwapMonteCarlo(5, 3, ktemp=0.7, seed=1))


@pytest.mark.parametrize("total,lags,origin_every", [(60, [2, 5], 3), (60, None, None), (1, [2, 5], 3)])
def test_all_ten_samplers_and_swap_in_one_run(tmp_path, monkeypatch, total, lags, origin_every):
    """The walk is tests/sampler_audit.expected_trace: per step, each sampler's documented rule through public names
    (every, schedule(), rounds, ktemp), in the order simulation.py documents for a shared step -- rdf, dynamics, sq,
    currents right after sq, stress, bond_order, clusters after bond_order, cage, four_point, orientational last, swap
    after every sampler, the frame export after the swap block."""
    from tests.sampler_audit import expected_trace
    monkeypatch.chdir(tmp_path)
    f = 7
    state, dev = _fake_state()
    params = md.Parameters(1.0, N, 0.002, md.LennardJones())
    s = _all_ten(lags, origin_every)
    out = str(tmp_path / "out")
    with np.errstate(all="ignore"):
        md.run_simulation(state, params, md.NVE(), total, f, out, log_times=True, **s)
    assert dev.setups == ["rdf_setup", "dyn_setup", "sq_setup", "cur_setup", "stress_setup", "boo_setup", "cluster_setup",
                          "cage_setup", "chi4_setup", "mpc_setup", "swap_setup"]
    want, stops = expected_trace(s, total, f, log_times=True, ensemble=md.NVE())
    assert dev.trace == want
    assert list(np.cumsum(dev.segments) - 1) == stops
    if total == 60:
        # the walk itself, pinned where the rules meet: step 0 is shared by all ten; swap acts at 4, 9, ...; at step 14
        # (an output step, a swap stop) the samplers of that step come first and the frame export last
        at0 = [m for st, m, _ in want if st == 0]
        order = ["rdf_sample", "dyn_origin", "sq_sample", "cur_sample", "stress_sample", "boo_sample", "cluster_sample",
                 "cage_origin", "chi4_origin", "mpc_sample", "snapshot_begin"]
        assert at0 == order
        assert [st for st, m, _ in want if m == "swap_rounds"] == list(range(4, 60, 5))
        assert [a[2] for _, m, a in want if m == "swap_rounds"] == [3 * k for k in range(12)]
        at14 = [m for st, m, _ in want if st == 14]
        assert at14[0] == "rdf_sample" and at14[-2:] == ["swap_rounds", "snapshot_begin"] and "boo_sample" in at14
    assert s["swap"].rounds_done == 3 * sum(1 for t in want if t[1] == "swap_rounds")
    assert s["bond_order"].nsamples == sum(1 for t in want if t[1] == "boo_sample")

    snapshots = {0} | {int(math.floor(1.35 ** i)) for i in range(41)}
    present = {"thermo.txt", "trajectory.xyz", "final.xyz", "rdf.txt", "dynamics.txt", "sq.txt", "fqt.txt", "currents.txt",
               "vacf.txt", "stress.txt", "stress_acf.txt", "bond_order.txt", "bond_order_series.txt", "clusters.txt",
               "clusters_series.txt", "cage.txt", "chi4.txt", "s4.txt", "orient_corr.txt", "swap.txt"}
    assert set(os.listdir(out)) == present | {"snapshot.%d" % t for t in snapshots if t < total}


def test_the_two_refusals(tmp_path):
    """members="solid" or orientational= without bond_order=, and an `every` that is no multiple of bond_order's."""
    params = md.Parameters(1.0, N, 0.002, md.LennardJones())

    def run(**kw):
        state, _ = _fake_state()
        with np.errstate(all="ignore"):
            md.run_simulation(state, params, md.NVE(), 5, 2, str(tmp_path), **kw)

    solid = md.ClusterAnalysis(0.9, members="solid", every=3)
    with pytest.raises(ValueError, match="needs bond_order="):
        run(clusters=solid)
    with pytest.raises(ValueError, match="needs bond_order="):
        run(orientational=md.OrientationalCorrelation(0.9, 3))
    bo = md.BondOrder(0.9, every=2)
    with pytest.raises(ValueError, match="multiple of bond_order.every"):
        run(clusters=solid, bond_order=bo)
    with pytest.raises(ValueError, match="multiple of bond_order.every"):
        run(orientational=md.OrientationalCorrelation(0.9, 3, every=3), bond_order=bo)
    run(clusters=md.ClusterAnalysis(0.9, members="solid", every=4), bond_order=bo,
        orientational=md.OrientationalCorrelation(0.9, 3, every=2))
