"""CPU: the cage-relative dynamics sampler's host layers -- the exported symbols and their declarations, CageDynamics'
argument checks, schedule, normalisation, file format and overflow error, its place in run_simulation's sampler order (on
a fake handle that records every call, as tests/test_sampler_protocol.py does) -- and the numpy reference of the GPU
tests (tests/cage_reference.py) against answers worked out by hand on a 3 x 3 hexagonal patch."""
import inspect
import math
import os
import re

import numpy as np
import pytest

import moleculardynamics.jl_amd as md
from moleculardynamics.jl_amd import _lib, analysis
from tests import cage_reference as ref
from tests.test_sampler_protocol import N, _FakeDevice, _fake_state, _split

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["md_cage_setup", "md_cage_origin", "md_cage_sample", "md_cage_particles", "md_cage_read", "md_cage_reset"]


def test_symbols_bindings_and_build_rule():
    assert "CageDynamics" in md.__all__ and md.CageDynamics is analysis.CageDynamics
    header = open(os.path.join(ROOT, "include", "mdhip.h")).read()
    lib = _lib.load()
    for name in NAMES:
        assert name in _lib.EXPORTS
        assert hasattr(lib, name)
        assert re.search(r"\bint\s+" + name + r"\s*\(", header)
    assert len(lib.md_cage_setup.argtypes) == 9 and len(lib.md_cage_read.argtypes) == 6
    assert "nslots*N*max_neigh*(4+8*d)" in header and "MDHIP_CAGE_ALLOC_LIMIT" in header
    for name in ("cage_setup", "cage_origin", "cage_sample", "cage_particles", "cage_read", "cage_reset"):
        assert callable(getattr(md.MDDevice, name))
    mk = open(os.path.join(ROOT, "moleculardynamics", "jl_amd", "csrc", "Makefile")).read()
    assert re.search(r"^libmdhip\.so:.*\bmd_cage\.hpp\b", mk, re.M)
    params = list(inspect.signature(md.run_simulation).parameters)
    assert params[-3:] == ["clusters", "cage", "bond_order"]   # (tests/test_bond_order.py pins bond_order as the last one)
    assert inspect.signature(md.run_simulation).parameters["cage"].default is None
    assert list(inspect.signature(md.CageDynamics).parameters) == ["r_neigh", "r_break", "scaled", "max_neighbours", "q",
                                                                    "lags", "origin_every"]
    jl = open(os.path.join(ROOT, "julia", "MDHip.jl")).read()
    for name in NAMES:
        assert "(:%s, LIB)" % name in jl
    assert "mutable struct CageDynamics" in jl and "cage::Union{Nothing,CageDynamics}=nothing" in jl


def test_a_null_handle_is_refused():
    lib = _lib.load()
    assert lib.md_cage_setup(None, 1, 1, 1.5, 1.5, 0, 16, None, 0) != 0
    assert lib.md_cage_origin(None, 0) != 0 and lib.md_cage_reset(None) != 0
    assert b"null handle" in lib.md_last_error(None)


def test_argument_checks():
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="r_neigh"):
            md.CageDynamics(bad)
    for bad in (1.49, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="r_break"):
            md.CageDynamics(1.5, r_break=bad)
    for bad in (0, 33, 2.5):
        with pytest.raises(ValueError, match="max_neighbours"):
            md.CageDynamics(1.5, max_neighbours=bad)
    with pytest.raises(ValueError, match="at most 16"):
        md.CageDynamics(1.5, q=np.arange(17.0))
    with pytest.raises(ValueError, match="finite"):
        md.CageDynamics(1.5, q=[float("nan")])
    with pytest.raises(ValueError, match="origin_every"):
        md.CageDynamics(1.5, lags=[1, 2])
    with pytest.raises(ValueError, match="origin_every needs explicit lags"):
        md.CageDynamics(1.5, origin_every=3)
    with pytest.raises(ValueError, match="at most 64"):
        md.CageDynamics(1.5, lags=[65], origin_every=1)
    c = md.CageDynamics(1.5)
    assert c.r_break == 1.5 and c.scaled is False and c.max_neighbours == 16 and list(c.q) == [2.0 * math.pi]
    c = md.CageDynamics(1.4, r_break=1.4, scaled=True, max_neighbours=32, q=(), lags=[64], origin_every=1)
    assert c.nslots == 64 and c.q.size == 0 and c.sums.shape == (1, 2) and c.hist_broken.shape == (1, 33)


@pytest.mark.parametrize("lags,origin_every,total", [(None, None, 3000), ([2, 5], 3, 60), ([1, 7, 20], 4, 45), ([3], 1, 1)])
def test_schedule_is_self_dynamics(lags, origin_every, total):
    c = md.CageDynamics(1.5, lags=lags, origin_every=origin_every)
    d = md.SelfDynamics(lags=lags, origin_every=origin_every)
    assert c.schedule(total) == d.schedule(total)
    assert np.array_equal(c.lags, d.lags) and c.nslots == d.nslots


class _CageFake(_FakeDevice):
    """tests/test_sampler_protocol.py's recording handle, with the cluster and cage calls."""
    overflow = 0

    def cluster_setup(self, *a):
        self.setups.append("cluster_setup")

    def cluster_sample(self):
        self._log("cluster_sample")

    def cluster_read(self):
        return 0, np.zeros(8, dtype=np.int64), np.zeros(1025, dtype=np.int64), np.zeros((0, 8), dtype=np.int64)

    def cage_setup(self, nslots, nrows, r_neigh, r_break, scaled, max_neigh, q):
        self.setups.append("cage_setup")
        self.cage_args = (nslots, nrows, r_neigh, r_break, scaled, max_neigh, tuple(q))

    def cage_sample(self, slots, rows):
        self._log("cage_sample", tuple(int(v) for v in slots), tuple(int(v) for v in rows))

    def cage_origin(self, slot):
        self._log("cage_origin", int(slot))

    def cage_read(self):
        nrows, nq = self.cage_args[1], len(self.cage_args[6])
        ns = np.zeros(nrows, dtype=np.int64)
        for _, m, a in self.trace:
            if m == "cage_sample":
                for r in a[1]:
                    ns[r] += 1
        cnt = np.stack([ns * N, ns * N * 6, ns * N * 3], axis=1)
        sums = np.concatenate([(ns * N * 0.5)[:, None], (ns * N * 0.75)[:, None], np.tile((ns * N * 1.5)[:, None], (1, nq))],
                              axis=1)
        hist = np.zeros((nrows, 33), dtype=np.int64)
        hist[:, 3] = ns * N
        return ns, sums, cnt, hist, self.overflow


def _cage_state():
    state, _ = _fake_state()
    dev = _CageFake()
    state.system.device = dev
    return state, dev


def test_run_simulation_drives_the_cage_sampler_last(tmp_path):
    total, f = 40, 7
    state, dev = _cage_state()
    params = md.Parameters(1.0, N, 0.002, md.LennardJones())
    dyn = md.SelfDynamics(lags=[2, 5], origin_every=3)
    cage = md.CageDynamics(1.5, r_break=1.8, scaled=True, max_neighbours=12, q=[1.0, 2.0], lags=[2, 5], origin_every=3)
    cl = md.ClusterAnalysis(1.5)
    out = str(tmp_path / "out")
    with np.errstate(all="ignore"):
        md.run_simulation(state, params, md.NVE(), total, f, out, write_trajectory=False, dynamics=dyn, clusters=cl,
                          cage=cage)
    assert dev.setups == ["dyn_setup", "cluster_setup", "cage_setup"]          # once, and after clusters
    assert dev.cage_args == (2, 2, 1.5, 1.8, True, 12, (1.0, 2.0))
    events = cage.schedule(total)[1]
    want, stops = [], {total - 1}
    for step in range(total):
        before = len(want)
        output = step % f == 0
        ev = events.get(step)
        if ev is not None and ev[0]:
            want.append((step, "dyn_sample", _split(ev[0])))
        if ev is not None and ev[1] is not None:
            want.append((step, "dyn_origin", (ev[1],)))
        if output:
            want.append((step, "cluster_sample", ()))
        if ev is not None and ev[0]:
            want.append((step, "cage_sample", _split(ev[0])))                              # the samples before the origin
        if ev is not None and ev[1] is not None:
            want.append((step, "cage_origin", (ev[1],)))
        if len(want) > before or output:
            stops.add(step)
    assert dev.trace == want
    assert list(np.cumsum(dev.segments) - 1) == sorted(stops)                              # the segments stop there
    assert any(t[1] == "cage_sample" and len(t[2][0]) > 1 for t in want)                   # several rows in one call
    assert {"cage.txt", "dynamics.txt"} <= set(os.listdir(out))
    # the fake's read-back, normalised: msd 0.5, <d4> 0.75, Fs 1.5 / d, C_B 0.5, everybody lost three bonds
    k = cage.nsamples > 0
    assert k.all() and cage.nsamples.sum() == sum(len(t[2][0]) for t in want if t[1] == "cage_sample")
    assert np.allclose(cage.msd(), 0.5) and np.allclose(cage.fs(), 0.5) and np.allclose(cage.bond_correlation(), 0.5)
    assert np.allclose(cage.alpha2(), 3 * 0.75 / (5 * 0.25) - 1.0)
    bd = cage.broken_distribution()
    assert bd.shape == (2, 33) and np.allclose(bd[:, 3], 1.0) and np.allclose(bd.sum(axis=1), 1.0)
    # a second run accumulates; reset() empties
    with np.errstate(all="ignore"):
        md.run_simulation(state, params, md.NVE(), total, f, out, write_trajectory=False, cage=cage)
    assert dev.setups[-1] == "cage_setup" and np.allclose(cage.msd(), 0.5)
    cage.reset()
    assert not cage.nsamples.any() and not cage.counts.any() and np.isnan(cage.msd()).all()


def test_cage_txt_format(tmp_path):
    c = md.CageDynamics(1.5, q=[2.0, 7.25], lags=[1, 4, 9], origin_every=3)
    ns = np.array([2, 0, 1])
    sums = np.array([[8.0, 40.0, 12.0, 6.0], [0, 0, 0, 0], [2.0, 3.0, 1.5, 0.75]])
    counts = np.array([[16, 96, 72], [0, 0, 0], [8, 40, 10]])
    hist = np.zeros((3, 33), dtype=np.int64)
    c._accumulate(ns, sums, counts, hist, 2, 0.01)
    p = str(tmp_path / "cage.txt")
    c.write(p)
    lines = open(p).read().splitlines()
    assert lines[0] == "# lag time msd_cr alpha2_cr Fs_cr(q=2) Fs_cr(q=7.25) C_B nsamples"
    assert len(lines) == 3                                     # the lag without a sample has no row
    row = lines[1].split()
    assert row[0] == "1" and row[-1] == "2" and len(row) == 8
    assert [float(v) for v in row[1:7]] == [0.01, 0.5, 2 * 2.5 / (4 * 0.25) - 1.0, 12.0 / 32, 6.0 / 32, 0.75]
    row = lines[2].split()
    assert row[0] == "9" and row[-1] == "1" and float(row[1]) == 0.09 and float(row[6]) == 0.25
    assert row[2] == "%.6e" % 0.25


def test_overflow_is_an_error_at_the_end(tmp_path):
    state, dev = _cage_state()
    dev.overflow = 5
    params = md.Parameters(1.0, N, 0.002, md.LennardJones())
    cage = md.CageDynamics(1.5, max_neighbours=4, lags=[1], origin_every=2)
    with pytest.raises(ValueError, match=r"5 neighbours did not fit max_neighbours = 4"):
        md.run_simulation(state, params, md.NVE(), 6, 2, str(tmp_path), write_trajectory=False, cage=cage)
    assert not cage.nsamples.any() and not os.path.exists(os.path.join(str(tmp_path), "cage.txt"))


# ---------------------------------------------------------------------------------------------------------------------
# the reference module against hand answers: ids   6 7 8
#                                                   3 4 5      (row 1 shifted right by half a spacing)
#                                                  0 1 2
NNB = [2, 4, 3, 5, 6, 3, 2, 4, 3]


def test_reference_on_a_hexagonal_patch_by_hand():
    x0, cell, pairs, de = ref.hexagonal_patch()
    n = len(x0)
    im0 = np.zeros((n, 2), dtype=np.int32)
    assert len(pairs) == 16 and np.allclose(ref.d2_of(de), 1.0)
    h = np.array([0.3, 0.0])
    x1 = x0.copy()
    x1[4] += h
    r = ref.cage(x0, im0, x1, im0, cell, pairs, de, np.ones(n), 1.2, q=[2.0])
    assert list(r["nnb"]) == NNB
    want = np.zeros((n, 2))
    want[4] = h                                                 # nobody around the hopper moved: its own hop
    for j in (1, 2, 3, 5, 7, 8):
        want[j] = -h / NNB[j]                                   # the hopper's neighbours: minus their share of the hop
    assert np.allclose(r["dcr"], want, rtol=0, atol=1e-15)
    d2 = 0.09 * np.array([0, 1 / 16, 1 / 9, 1 / 25, 1, 1 / 9, 0, 1 / 16, 1 / 9])
    assert np.allclose(r["d2"], d2, rtol=0, atol=1e-15)
    # the bond 3-4 along the hop stretches to 1.3 > 1.2; 1-4 and 7-4 to sqrt(0.64 + 0.75) = 1.179; the others shorten
    assert list(r["broken"]) == [0, 0, 0, 1, 1, 0, 0, 0, 0]
    assert list(r["counts"]) == [9, 32, 30]
    assert r["hist"][0] == 7 and r["hist"][1] == 2 and r["hist"].sum() == 9 and r["hist"].shape == (33,)
    assert abs(r["sums"][0] - d2.sum()) <= 1e-15 and abs(r["sums"][1] - (d2 * d2).sum()) <= 1e-15
    assert abs(r["sums"][2] - (np.cos(2.0 * want[:, 0]) + np.cos(2.0 * want[:, 1])).sum()) <= 1e-14
    # scaled by sigma_ij = 0.9: the break radius is 1.08, and 1.179 is beyond it too
    r = ref.cage(x0, im0, x1, im0, cell, pairs, de, np.full(n, 0.9), 1.2, scaled=True)
    assert list(r["broken"]) == [0, 1, 0, 1, 3, 0, 0, 1, 0] and list(r["counts"]) == [9, 32, 26]
    # ... and with unequal diameters only the pair's own mean counts: sigma_1 = 1.3 lifts bond 1-4 back under its radius
    dm = np.full(n, 0.9)
    dm[1] = 1.3
    r = ref.cage(x0, im0, x1, im0, cell, pairs, de, dm, 1.2, scaled=True)
    assert list(r["broken"]) == [0, 0, 0, 1, 2, 0, 0, 1, 0]


def test_reference_removes_a_common_drift_and_counts_images():
    x0, cell, pairs, de = ref.hexagonal_patch()
    n = len(x0)
    im0 = np.zeros((n, 2), dtype=np.int32)
    # everybody crosses the cell three times in x and comes back one short of a fourth: images 3, wrapped shift 0.25
    x1 = x0 + np.array([0.25, -0.5])
    im1 = im0 + np.array([3, 0], dtype=np.int32)
    r = ref.cage(x0, im0, x1, im1, cell, pairs, de, np.ones(n), 1.0 + 1e-9)
    assert np.allclose(r["delta"], [120.25, -0.5], rtol=0, atol=1e-12)
    assert np.abs(r["dcr"]).max() <= 1e-13 and not r["broken"].any() and list(r["counts"]) == [9, 32, 32]
    # a particle without bonds contributes to nothing
    keep = ~np.any(pairs == 0, axis=1)
    x1 = x0.copy()
    x1[0] += 5.0
    r = ref.cage(x0, im0, x1, im0, cell, pairs[keep], de[keep], np.ones(n), 1.2)
    assert r["nnb"][0] == 0 and r["d2"][0] == 0.0 and list(r["counts"]) == [8, 28, 28] and r["hist"][0] == 8
    assert not r["d2"].any()
