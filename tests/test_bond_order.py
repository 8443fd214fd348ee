"""CPU tests of the bond-orientational order layer (analysis.BondOrder / compute_bond_order, the binding,
run_simulation's bond_order= keyword): the exports, the argument checks, the stop schedule, the file formats on a fake
handle, and the numpy / scipy reference of tests/boo_reference.py -- which the GPU tests compare the device against --
on the perfect lattices.  The device sums are tested in tests/test_gpu_bond_order.py."""
import inspect
import os
import re
import types

import numpy as np
import pytest

import moleculardynamics.jl_amd as md
from moleculardynamics.jl_amd import BondOrder, _lib, analysis
from tests import boo_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("md_boo_setup", "md_boo_sample", "md_boo_particles", "md_boo_qlm", "md_boo_read", "md_boo_reset")
N, DIM = 8, 3


def test_exports():
    for name in ("BondOrder", "compute_bond_order"):
        assert name in md.__all__ and getattr(md, name) is getattr(analysis, name)
    header = open(os.path.join(ROOT, "include", "mdhip.h")).read()
    for name in NAMES:
        assert name in _lib.EXPORTS
        assert hasattr(_lib.load(), name)
        assert re.search(r"\bint\s+" + name + r"\s*\(", header)
    assert "Condon-Shortley" in header and "min((int)(value*nbins), nbins-1)" in header     # the conventions are stated
    for name in ("boo_setup", "boo_sample", "boo_particles", "boo_qlm", "boo_read", "boo_reset"):
        assert callable(getattr(md.MDDevice, name))
    mk = open(os.path.join(ROOT, "moleculardynamics", "jl_amd", "csrc", "Makefile")).read()
    assert re.search(r"^libmdhip\.so:.*\bmd_boo\.hpp\b", mk, re.M)
    sig = inspect.signature(md.run_simulation)
    assert "bond_order" in sig.parameters and sig.parameters["bond_order"].default is None
    assert list(sig.parameters)[-1] == "bond_order"
    assert list(inspect.signature(md.compute_bond_order).parameters) == ["state", "params", "r_neigh", "order", "threshold",
                                                                       "min_connections"]
    p = inspect.signature(BondOrder).parameters
    assert [(k, v.default) for k, v in p.items()][1:] == [("order", 6), ("every", 1), ("nbins", 100), ("threshold", 0.7),
                                                          ("min_connections", 7), ("nseries", None)]


def test_argument_checks():
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="r_neigh"):
            BondOrder(bad)
    for bad in (0, 13, 5.5):
        with pytest.raises(ValueError, match="order"):
            BondOrder(1.5, order=bad)
    for bad in (0, -2, 1.5):
        with pytest.raises(ValueError, match="every"):
            BondOrder(1.5, every=bad)
    for bad in (0, 8193, 2.5):
        with pytest.raises(ValueError, match="nbins"):
            BondOrder(1.5, nbins=bad)
    for bad in (float("inf"), float("nan")):
        with pytest.raises(ValueError, match="threshold"):
            BondOrder(1.5, threshold=bad)
    for bad in (-1, 33, 6.5):
        with pytest.raises(ValueError, match="min_connections"):
            BondOrder(1.5, min_connections=bad)
    for bad in (-1, (1 << 20) + 1, 0.5):
        with pytest.raises(ValueError, match="nseries"):
            BondOrder(1.5, nseries=bad)
    BondOrder(1.5, order=12, nbins=8192, min_connections=32, nseries=1 << 20)
    BondOrder(1.5, order=1, nbins=1, min_connections=0, nseries=0, threshold=-1.0)
    bo = BondOrder(1.5)
    for call in (bo.mean_q, bo.mean_qbar, bo.mean_neighbours, bo.solid_fraction, bo.global_order):
        with pytest.raises(ValueError, match="no sample"):
            call()
    with pytest.raises(ValueError, match="which"):
        bo.histogram("w6")


def test_schedule():
    assert BondOrder(1.5).schedule(21, 5) == [0, 5, 10, 15, 20]
    assert BondOrder(1.5, every=2).schedule(21, 5) == [0, 10, 20]
    assert BondOrder(1.5, every=2).schedule(20, 5) == [0, 10]
    assert BondOrder(1.5, every=3).schedule(0, 5) == []


def test_means_and_histograms():
    bo = BondOrder(1.5, nbins=4)
    fr = np.array([5.0, 3.0, 4.0, 2.0, 120.0, 60.0, 2.0, 0.25])
    series = np.stack([0.5 * fr, 0.5 * fr])
    bo._accumulate(2, fr, [0, 4, 12, 4], [0, 0, 20, 0], np.eye(33, dtype=np.int64)[12] * 20, np.eye(33, dtype=np.int64)[6] * 20,
                   series, [0, 10], 10)
    assert bo.nsamples == 2 and bo.n_particles == 10
    assert bo.mean_q() == 0.25 and bo.mean_qbar() == 0.2 and bo.mean_neighbours() == 6.0
    assert bo.solid_fraction() == 0.1 and bo.global_order() == 0.125
    r, dens, counts = bo.histogram("q")
    assert np.array_equal(r, [0.125, 0.375, 0.625, 0.875]) and list(counts) == [0, 4, 12, 4]
    assert np.sum(dens) / 4 == pytest.approx(1.0)           # integral over [0, 1]
    assert np.array_equal(bo.histogram("qbar")[1], [0.0, 0.0, 4.0, 0.0])
    c, dens, counts = bo.histogram("neighbours")
    assert c[12] == 12.0 and dens[12] == 1.0 and counts.sum() == 20
    assert bo.histogram("connections")[2][6] == 20
    steps, cols = bo.series()
    assert list(steps) == [0, 10] and cols.shape == (2, 5)
    assert np.array_equal(cols[0], [0.25, 0.2, 6.0, 0.1, 0.125])
    # sums over runs of different N have no per-particle mean: refused, until reset()
    with pytest.raises(ValueError, match="number of particles"):
        bo._accumulate(1, fr, [0, 4, 12, 4], [0, 0, 20, 0], np.zeros(33), np.zeros(33), series[:1], [0], 12)
    assert bo.nsamples == 2 and bo.n_particles == 10
    bo.reset()
    assert bo.nsamples == 0 and not bo.hist_q.any() and bo.series()[1].shape == (0, 5)
    bo._accumulate(1, fr, [0, 4, 12, 4], [0, 0, 20, 0], np.zeros(33), np.zeros(33), series[:1], [0], 12)
    assert bo.n_particles == 12 and bo.mean_neighbours() == 10.0


class _FakeDevice:
    """Records the segment lengths and the steps of the sampler's calls; reads back a fixed answer per sample."""

    def __init__(self, brownian=False):
        self.n, self.dim = N, DIM
        self.step = 0
        self.segments, self.samples, self.setup = [], [], None
        self.brownian = brownian
        self.potential = None

    def set_potential(self, kind, params):
        self.potential = ("builtin", kind)

    def set_potential_source(self, src, entry, params=()):
        self.potential = ("source", entry)

    def upload(self, **kw):
        pass

    def run(self, nsteps, dt, *a, **kw):
        assert not self.brownian
        self.segments.append(nsteps)
        self.step += nsteps
        return 0.0, 0.0, 1.0

    def run_brownian(self, nsteps, dt, ktemp, seed, first_step=0, virial_every=10):
        assert self.brownian
        self.segments.append(nsteps)
        self.step += nsteps
        return dict(U=0.0, W=0.0, virial_sum=0.0, virial_count=0.0)

    def download(self):
        z = np.zeros((N, DIM))
        return z, z, z, np.zeros((N, DIM), dtype=np.int32)

    def snapshot_begin(self):
        pass

    def snapshot_end(self):
        return np.zeros((N, DIM)), np.zeros((N, DIM), dtype=np.int32)

    def boo_setup(self, r_neigh, order=6, nbins=100, threshold=0.7, min_conn=7, nseries=0):
        self.setup = (r_neigh, order, nbins, threshold, min_conn, nseries)

    def boo_sample(self):
        self.samples.append(self.step - 1)

    FR = np.array([4.0, 2.0, 2.0, 1.0, 96.0, 40.0, 4.0, 0.5])

    def boo_read(self):
        ns, (_, _, nbins, _, _, nseries) = len(self.samples), self.setup
        hq, hb = np.zeros(nbins, dtype=np.int64), np.zeros(nbins, dtype=np.int64)
        hq[nbins // 2], hb[nbins // 4] = N * ns, N * ns
        hn, hc = np.zeros(33, dtype=np.int64), np.zeros(33, dtype=np.int64)
        hn[12], hc[5] = N * ns, N * ns
        rows = min(ns, nseries)
        return ns, self.FR * ns, hq, hb, hn, hc, np.tile(self.FR, (rows, 1))


def _fake_state(brownian=False):
    dev = _FakeDevice(brownian)
    system = types.SimpleNamespace(device=dev, positions=np.zeros((N, DIM)), xpositions=None,
                                   energy_and_forces=types.SimpleNamespace(forces=np.zeros((N, DIM)), energy=0.0,
                                                                           virial=0.0))
    state = md.SimulationState(system, np.ones(N), np.random.default_rng(1), np.diag([2.0, 2.0, 2.0]),
                               np.zeros((N, DIM)), np.zeros((N, DIM), dtype=np.int32), DIM, DIM * (N - 1.0))
    return state, dev


@pytest.mark.parametrize("every,freq,total", [(1, 5, 21), (2, 5, 21), (3, 4, 9), (1, 7, 1)])
def test_samples_at_every_nth_output_step(tmp_path, every, freq, total):
    state, dev = _fake_state()
    params = md.Parameters(1.0, N, 0.002, md.LennardJones())
    bo = BondOrder(1.5, every=every, nbins=8)
    md.run_simulation(state, params, md.NVE(), total, freq, str(tmp_path), write_trajectory=False, bond_order=bo)
    want = [s for s in range(0, total, freq) if (s // freq) % every == 0]
    assert dev.samples == want == bo.schedule(total, freq)
    # the sampler adds no stop of its own: the loop stops at the output steps and at the last step
    assert list(np.cumsum(dev.segments) - 1) == sorted(set(range(0, total, freq)) | {total - 1})
    assert dev.setup == (1.5, 6, 8, 0.7, 7, len(want))      # by default one series row per sample of the run
    assert bo.nsamples == len(want) and list(bo.steps) == want


def test_file_formats(tmp_path):
    state, dev = _fake_state()
    params = md.Parameters(1.0, N, 0.002, md.LennardJones())
    bo = BondOrder(1.35, order=4, nbins=4, threshold=0.6, min_connections=5)
    out = str(tmp_path)
    md.run_simulation(state, params, md.NVE(), 11, 5, out, write_trajectory=False, bond_order=bo)
    assert set(os.listdir(out)) == {"thermo.txt", "final.xyz", "bond_order.txt", "bond_order_series.txt"}
    lines = open(os.path.join(out, "bond_order.txt")).read().splitlines()
    assert lines[0] == "# order 4 r_neigh 1.350000 threshold 0.600000 min_connections 5 nsamples 3"
    assert lines[1] == ("# mean_q 0.50000000 mean_qbar 0.25000000 mean_neighbours 12.000000 solid_fraction 0.50000000 "
                        "global_order 0.50000000")
    assert lines[2] == "# bin q_density qbar_density count_q count_qbar"
    assert len(lines) == 3 + 4
    assert lines[3] == "0.125000 0.000000e+00 0.000000e+00 0 0"
    assert lines[4] == "0.375000 0.000000e+00 4.000000e+00 0 24"
    assert lines[5] == "0.625000 4.000000e+00 0.000000e+00 24 0"
    lines = open(os.path.join(out, "bond_order_series.txt")).read().splitlines()
    assert lines[0] == "# step <q> <qbar> <n> solid_fraction global_order"
    assert lines[1:] == ["%d 0.50000000 0.25000000 12.000000 0.50000000 0.50000000" % s for s in (0, 5, 10)]
    # a second run accumulates in the object; nseries caps the recorded rows, not the sums
    bo2 = BondOrder(1.35, nbins=4, nseries=2)
    state, dev = _fake_state()
    md.run_simulation(state, params, md.NVE(), 11, 5, out, write_trajectory=False, bond_order=bo2)
    assert dev.setup[-1] == 2 and bo2.nsamples == 3 and list(bo2.steps) == [0, 5]
    state, dev = _fake_state()
    md.run_simulation(state, params, md.NVE(), 6, 5, out, write_trajectory=False, bond_order=bo2)
    assert bo2.nsamples == 5 and list(bo2.steps) == [0, 5, 0, 5] and bo2.mean_q() == 0.5


def test_brownian_and_user_potentials_are_served(tmp_path):
    """The sampler never evaluates the potential: neither the ensemble nor the kind of potential is refused."""
    state, dev = _fake_state(brownian=True)
    params = md.Parameters(1.0, N, 0.002, md.LennardJones())
    bo = BondOrder(1.5, nbins=4)
    md.run_simulation(state, params, md.Brownian(1.0), 6, 5, str(tmp_path), write_trajectory=False, bond_order=bo)
    assert dev.samples == [0, 5] and bo.nsamples == 2

    class Mine(md.Potential):
        def device_spec(self):
            return ("source", "/* user text */", "mine", ())

        def energy_lrc(self, n, volume):
            return 0.0

        def pressure_lrc(self, n, volume):
            return 0.0

    state, dev = _fake_state()
    bo = BondOrder(1.5, nbins=4)
    md.run_simulation(state, md.Parameters(1.0, N, 0.002, Mine()), md.NVE(), 6, 5, str(tmp_path), write_trajectory=False,
                      bond_order=bo)
    assert dev.potential == ("source", "mine") and dev.samples == [0, 5]


def test_it_goes_last_among_the_samplers():
    src = inspect.getsource(md.run_simulation)
    assert re.search(r"\(rdf, dynamics, sq, stress, bond_order\)", src)


# ---------------------------------------------------------------------------------------------------------------------
# The reference on perfect lattices.  The table below was typed from memory (no network where this was written): the
# values quoted for fcc, hcp and bcc in the bond-order literature (Steinhardt, Nelson and Ronchetti 1983; the table of
# Mickel et al. 2013).  Were one of them to disagree with the reference, the reference -- Y_lm from scipy's Legendre
# functions -- decides, and the table entry is what is wrong.
LITERATURE = {"fcc": (12, 0.19094, 0.57452), "hcp": (12, 0.09722, 0.48476), "bcc": (14, 0.03637, 0.51069)}


@pytest.mark.parametrize("name", ["fcc", "hcp", "bcc"])
def test_reference_reproduces_the_lattice_values(name):
    x, box = {"fcc": ref.fcc, "hcp": ref.hcp, "bcc": ref.bcc}[name](4, 1.0)
    r_n = {"fcc": 0.85, "hcp": 1.2, "bcc": 1.2}[name]       # between the last counted shell and the next one
    pairs, de = ref.brute_pairs(x, box, r_n)
    nn, q4, q6 = LITERATURE[name]
    for l, want in ((4, q4), (6, q6)):
        r = ref.bond_order(len(x), pairs, de, l, 0.7, 7)
        assert np.all(r["nnb"] == nn)
        assert np.all(np.abs(r["q"] - want) <= 1e-5), (name, l, r["q"][0], want)
        # every site is equivalent and equally oriented: averaging changes nothing, every bond is coherent
        assert np.all(np.abs(r["qbar"] - r["q"]) <= 1e-12) and np.all(np.abs(r["sij"] - 1.0) <= 1e-12)
        assert np.all(r["conn"] == nn) and r["fr"][6] == len(x)
        assert abs(r["fr"][7] - r["q"][0]) <= 1e-12


def test_reference_hexagonal_and_phase_convention():
    x, box = ref.hexagonal(4, 3, 1.0)
    pairs, de = ref.brute_pairs(x, box, 1.3)
    r = ref.bond_order(len(x), pairs, de, 6, 0.7, 6)
    assert np.all(r["nnb"] == 6) and np.all(np.abs(r["q"] - 1.0) <= 1e-12) and np.all(r["conn"] == 6)
    assert abs(r["fr"][7] - 1.0) <= 1e-12
    r4 = ref.bond_order(len(x), pairs, de, 4, 0.7, 6)      # no four-fold order on a triangular lattice
    assert np.all(r4["q"] <= 1e-12)
    # Condon-Shortley: Y_11 = -sqrt(3 / 8 pi) sin(theta) e^{i phi}; Y_{l0} on the pole is sqrt((2l + 1) / 4 pi)
    y = ref.ylm(1, np.array([[1.0, 0.0, 0.0], [0.0, 2.0, 0.0]]))
    assert y[0, 1] == pytest.approx(-np.sqrt(3.0 / (8.0 * np.pi)))
    assert y[1, 1] == pytest.approx(-1j * np.sqrt(3.0 / (8.0 * np.pi)))
    assert ref.ylm(6, np.array([[0.0, 0.0, 3.0]]))[0, 0] == pytest.approx(np.sqrt(13.0 / (4.0 * np.pi)))
    # the addition theorem bounds both invariants by 1: a single bond gives exactly 1
    one = ref.bond_order(2, np.array([[0, 1]]), np.array([[0.3, -0.4, 0.5]]), 6, 0.7, 1)
    assert np.all(np.abs(one["q"] - 1.0) <= 1e-12)
    assert ref.bins([0.0, 0.999, 1.0, 0.5], 4).tolist() == [1, 0, 1, 2]
    assert ref.clamped_counts([0, 12, 40]).tolist()[32] == 1
