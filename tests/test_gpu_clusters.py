"""-m gpu: clusters sampled on the device (md_cluster_*, md_cluster.hpp).

The reference is scipy (tests/cluster_reference.py): connected_components on the oracle's pair list of the downloaded
frame, solid membership from tests/boo_reference.py -- nothing from the code under test.

Guards, asserted first (conditions, not tolerances): no pair has |d2 - rb2| <= 1e-9 rb2 (the two sides round del
differently at the 1e-16 level and would otherwise be allowed to disagree about a bond); in solid mode the bond-order
reference's own two guards.  The input conditions of a test (enough clusters, a largest cluster that is neither a
speck nor everything) are asserted on the reference before anything is compared.

Everything is compared for exact equality: labels, sizes, the frame vector, the histogram, the sums and the series are
integers and functions of the frame alone."""
import ctypes
import os

import numpy as np
import pytest

from tests import boo_reference as boo
from tests import cluster_reference as ref
from tests.test_gpu_bond_order import LJ, TRIC_U, WALKS, _handle, _neighbour_bonds, _walk_case
from tests.test_gpu_bond_order import _reference as _boo_reference
from tests.util import lj_system, poly_system

pytestmark = pytest.mark.gpu
ALL, SOLID = 0, 1


def _reference(oracle, x, cell, r_bond, member=None, max_size=1024, tric=False):
    pairs, _ = _neighbour_bonds(oracle, x, cell, r_bond, tric)     # asserts the guard on the bond radius
    return ref.clusters(len(x), pairs, member=member, max_size=max_size)


def _ramified(r, n):
    """The input condition of the tests that are about the union itself."""
    assert np.count_nonzero(r["sizes"] >= 2) >= 50, "fewer than 50 clusters of two or more: change the seed"
    assert 0.05 * n <= r["fr"][2] <= 0.60 * n, "the largest cluster is a speck or nearly everything: change the seed"


def _sample(dev, r_bond, members=ALL, max_size=1024, nseries=4):
    """One sample on a fresh setup; everything the handle reports about it."""
    dev.cluster_setup(r_bond, members, max_size, nseries)
    dev.cluster_sample()
    label, size = dev.cluster_particles()
    ns, fr, hist, series = dev.cluster_read()
    return dict(label=label, size=size, ns=ns, fr=fr, hist=hist, series=series)


def _check(d, r, label=""):
    print("%s N %d  device fr %s  reference fr %s" % (label, len(r["label"]), d["fr"].tolist(), r["fr"].tolist()))
    assert d["label"].dtype == np.int32 and d["size"].dtype == np.int32 and d["fr"].dtype == np.int64
    assert np.array_equal(d["label"], r["label"]) and np.array_equal(d["size"], r["size"])
    assert np.array_equal(d["fr"], r["fr"])
    assert np.array_equal(d["hist"], r["hist"]) and d["hist"][0] == 0 and d["hist"].sum() == r["fr"][1]
    # one sample: sum_fr is the frame vector and so is the series row
    assert d["ns"] == 1 and d["series"].shape == (1, 8) and np.array_equal(d["series"][0], d["fr"])


# ---------------------------------------------------------------------------------------------------------------------
# 1: a diluted simple-cubic lattice at the site-percolation threshold (0.3116): ramified clusters of every size, many of
# them through the periodic faces (ghost records), deep union trees.  N ~ 1300 = 5 tiles + a partial one.

def _diluted(seed):
    rng = np.random.default_rng(seed)
    g = np.arange(16)
    sites = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    keep = rng.random(len(sites)) < 0.32
    x = sites[keep] + 0.5 + rng.uniform(-0.02, 0.02, (int(keep.sum()), 3))
    rng.shuffle(x)                                          # particle ids carry no trace of the lattice order
    return x, np.full(3, 16.0)


@pytest.mark.parametrize("seed", [1, 4, 10])
def test_diluted_lattice_at_the_percolation_threshold(oracle, seed):
    x, box = _diluted(seed)
    n = len(x)
    assert n % 256 != 0
    with _handle(n, 3, box, 2.5, x) as dev:
        xd = dev.download()[0]
        d = _sample(dev, 1.1)
        assert dev.stats()["tiled"] == 1
    r = _reference(oracle, xd, box, 1.1)
    _ramified(r, n)
    _check(d, r, "diluted lattice, seed %d" % seed)


# ---------------------------------------------------------------------------------------------------------------------
# 2: the two extremes on fcc, 6^3 cells, a = 1.6 (nearest neighbours at 1.131): N = 864 = 3 tiles + 96

def test_fcc_one_cluster_and_singletons(oracle):
    x, box = boo.fcc(6, 1.6)
    n = len(x)
    assert n == 864
    with _handle(n, 3, box, 1.5, x) as dev:
        xd = dev.download()[0]
        one = _sample(dev, 1.35, max_size=64)
        none = _sample(dev, 1.0, max_size=64)
    _check(one, _reference(oracle, xd, box, 1.35, max_size=64), "fcc, r_bond above the first shell")
    assert one["fr"].tolist() == [n, 1, n, 0, 12 * n, n * n, 0, 0]
    assert one["hist"][64] == 1 and one["hist"].sum() == 1 and len(one["hist"]) == 65      # the overflow entry
    assert np.all(one["label"] == 0) and np.all(one["size"] == n)
    _check(none, _reference(oracle, xd, box, 1.0, max_size=64), "fcc, r_bond below the first shell")
    assert none["fr"].tolist() == [n, n, 1, 1, 0, n, 0, n]
    assert np.array_equal(none["label"], np.arange(n)) and none["hist"][1] == n


# ---------------------------------------------------------------------------------------------------------------------
# 3: the LJ liquid, N = 4000 = 15 tiles + 160, bonds just above the percolation threshold of the first shell

R_LIQUID = 1.025
_cache = {}


def _liquid(oracle):
    """The shared frame: lj_system(4000) after 200 NVT steps at kT = 1 on the device; the sample of that handle (inner rows
    active, list not fresh), the frame, the reference."""
    if "liq" not in _cache:
        from moleculardynamics.jl_amd import MDDevice, _lib
        from moleculardynamics.jl_amd.thermostat import draw_bussi
        s = lj_system(4000)
        with MDDevice(3, s["n"], s["box"], 2.5) as dev:
            dev.set_potential(0, LJ)
            dev.upload(s["x"], s["v"], s["f"], s["img"], s["diam"])
            nf = 3.0 * (s["n"] - 1.0)
            r1, r2 = draw_bussi(nf, np.random.default_rng(5), 200)
            dev.run(200, 0.002, _lib.MD_NVT, 0.1, nf, np.full(200, 1.0), r1, r2)
            st = dev.stats()
            d = _sample(dev, R_LIQUID)
            x = dev.download()[0]
        r = _reference(oracle, x, s["box"], R_LIQUID)
        _ramified(r, 4000)
        _cache["liq"] = dict(s=s, x=x, d=d, r=r, tiled=st["tiled"])
    return _cache["liq"]


def _same(a, b):
    for k in ("label", "size", "fr", "hist"):
        assert np.array_equal(a[k], b[k])


def test_lj_liquid_after_a_run(oracle):
    c = _liquid(oracle)
    assert c["tiled"] == 1
    _check(c["d"], c["r"], "liquid, after md_run")


def test_lj_liquid_fresh_handle(oracle):
    c = _liquid(oracle)
    with _handle(4000, 3, c["s"]["box"], 2.5, c["x"], pot=LJ) as dev:
        d = _sample(dev, R_LIQUID)                          # the first call after upload: the sample builds the list
        assert dev.stats()["tiled"] == 1
    _check(d, c["r"], "liquid, fresh handle")
    _same(d, c["d"])                                        # another slot order and row order, the same labels


def test_global_gather_path(oracle, monkeypatch):
    c = _liquid(oracle)
    monkeypatch.setenv("MDHIP_NO_TILES", "1")
    with _handle(4000, 3, c["s"]["box"], 2.5, c["x"], pot=LJ) as dev:
        d = _sample(dev, R_LIQUID)
        assert dev.stats()["tiled"] == 0
    _check(d, c["r"], "liquid, global-gather")
    _same(d, c["d"])


def test_user_potential(oracle):
    from moleculardynamics.jl_amd import MDDevice
    from tests.test_gpu_parity import USER_LJ_SRC
    c = _liquid(oracle)
    with MDDevice(3, 4000, c["s"]["box"], 2.5) as dev:
        dev.set_potential_source(USER_LJ_SRC, "user_lj", [1.0, 2.5])
        z = np.zeros_like(c["x"])
        dev.upload(c["x"], z, z, np.zeros(z.shape, dtype=np.int32), np.ones(4000))
        d = _sample(dev, R_LIQUID)
    _check(d, c["r"], "liquid, user potential")
    _same(d, c["d"])


# ---------------------------------------------------------------------------------------------------------------------
# 4, 5: two dimensions; a general cell

def test_2d_polydisperse(oracle):
    s = poly_system(1200)
    from moleculardynamics.jl_amd import MDDevice
    with MDDevice(2, s["n"], s["box"], 1.5) as dev:
        dev.set_potential(2, [1.25, 0.2])
        dev.upload(s["x"], s["v"], s["f"], s["img"], s["diam"])
        dev.run(60, 0.001)
        d = _sample(dev, 0.98)
        x = dev.download()[0]
    r = _reference(oracle, x, s["box"], 0.98)
    assert np.count_nonzero(r["sizes"] >= 2) >= 50 and 10 <= r["fr"][2] <= 600     # many clusters, none of them everything
    _check(d, r, "poly2d")


def test_general_cell(oracle):
    from moleculardynamics.jl_amd import MDDevice
    from tests.test_gpu_triclinic import _fill
    U, n = TRIC_U, 4000
    x0 = _fill(U, n, np.random.default_rng(4242))
    z = np.zeros_like(x0)
    with MDDevice(3, n, U, 2.5) as dev:
        dev.set_potential(0, LJ)
        dev.upload(x0, z, z, np.zeros((n, 3), np.int32), np.ones(n))
        d = _sample(dev, 1.1)
        x = dev.download()[0]
    r = _reference(oracle, x, U, 1.1, tric=True)
    assert np.count_nonzero(r["sizes"] >= 2) >= 50 and 10 <= r["fr"][2] <= 2000
    _check(d, r, "sheared cell")


@pytest.mark.parametrize("dim,rows", WALKS)
def test_every_walk_with_a_ragged_last_block(oracle, monkeypatch, dim, rows):
    """tests/test_gpu_bond_order.py's N = 257 lattice with vacancies; r_bond = 1.08, just below the spacing, keeps about two
    nearest-site bonds in five: tens of clusters, the largest of a few dozen sites."""
    x, box, diam = _walk_case(dim, rows, monkeypatch)
    with _handle(257, dim, box, 1.5, x, diam=diam) as dev:
        xd = dev.download()[0]
        d = _sample(dev, 1.08)
        assert dev.stats()["tiled"] == (0 if rows == "rows32" else 1)
    r = _reference(oracle, xd, box, 1.08)
    assert np.count_nonzero(r["sizes"] >= 2) >= 20 and 10 <= r["fr"][2] <= 128     # many clusters, none of them everything
    _check(d, r, "N = 257, %d-D, %s" % (dim, rows))


# ---------------------------------------------------------------------------------------------------------------------
# 6: solid mode.  Two fcc slabs of four layers with a fifth of the sites vacant, and a dilute jittered simple-cubic
# lattice (nobody there has a neighbour) in the other half of the box: N = 675 = 2 tiles + 163.

def _two_slabs():
    rng = np.random.default_rng(7)
    xc, _ = boo.fcc(6, 1.6)
    xc = xc[(xc[:, 2] < 3.2) | ((xc[:, 2] >= 4.8) & (xc[:, 2] < 8.0))]
    xc = xc[rng.random(len(xc)) >= 0.2]
    xc = xc + rng.normal(0.0, 0.03, xc.shape)
    g = np.arange(6)
    sc = (np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) + 0.5) * 1.6
    sc[:, 2] += 9.6
    sc = sc + rng.uniform(-0.1, 0.1, sc.shape)
    x = np.concatenate([xc, sc])
    x[:, 2] += 0.4
    rng.shuffle(x)
    box = np.array([9.6, 9.6, 19.2])
    return np.mod(x, box), box


def test_solid_clusters(oracle):
    x, box = _two_slabs()
    n = len(x)
    with _handle(n, 3, box, 1.5, x, pot=[1.0, 1.0, 1.5]) as dev:
        xd = dev.download()[0]
        dev.boo_setup(1.35, 6, 50, 0.7, 7, 0)
        dev.boo_sample()
        conn = dev.boo_particles()[3]
        d = _sample(dev, 1.35, SOLID)
        # the mask follows particle ids: a few steps (and the list build of the first one) between the two samples
        dev.run(5, 0.002)
        dev.cluster_setup(1.35, SOLID, 1024, 1)
        dev.cluster_sample()
        later = dict(zip(("label", "size"), dev.cluster_particles()))
        later["ns"], later["fr"], later["hist"], later["series"] = dev.cluster_read()
        x5 = dev.download()[0]
    b = _boo_reference(oracle, xd, box, 1.35, 6, 0.7, 7)   # asserts the bond-order reference's two guards
    assert 0.10 * n <= np.count_nonzero(b["solid"]) <= 0.90 * n
    assert np.array_equal(conn, b["conn"])
    r = _reference(oracle, xd, box, 1.35, member=b["solid"])
    assert r["fr"][1] >= 2 and r["fr"][0] == np.count_nonzero(b["solid"])
    _check(d, r, "solid clusters")
    assert np.all(d["label"][~b["solid"]] == -1) and np.all(d["size"][~b["solid"]] == 0)
    # the BOO frame's members, the later positions
    assert np.abs(x5 - xd).max() > 1e-6
    _check(later, _reference(oracle, x5, box, 1.35, member=b["solid"]), "solid clusters, five steps later")


# ---------------------------------------------------------------------------------------------------------------------
# 7: the sampler: accumulators, reset, the histogram's two routes, the last frame, no side effect, refusals

def test_accumulators_histogram_and_series(oracle):
    from moleculardynamics.jl_amd import MDDevice
    s = lj_system(4000)
    with MDDevice(3, s["n"], s["box"], 2.5) as dev:
        dev.set_potential(0, LJ)
        dev.upload(s["x"], s["v"], s["f"], s["img"], s["diam"])
        dev.cluster_setup(1.0, ALL, 8, 2)                  # room for two of the three frame vectors
        frames, reads = [], []
        for m in range(3):
            dev.run(10, 0.002)
            dev.cluster_sample()
            frames.append(dev.download()[0])
            reads.append(dev.cluster_read())
        dev.cluster_reset()
        ns0, fr0, hist0, series0 = dev.cluster_read()
        assert ns0 == 0 and not fr0.any() and not hist0.any() and series0.shape == (0, 8)
        dev.cluster_sample()                                # the third frame once more, into the emptied sampler
        ns1, fr1, hist1, series1 = dev.cluster_read()
        part1 = dev.cluster_particles()
        dev.cluster_setup(1.0, ALL, 3, 0)                  # setup again starts over
        ns2, fr2, hist2, series2 = dev.cluster_read()
        assert ns2 == 0 and hist2.shape == (4,) and not fr2.any() and series2.shape == (0, 8)
    refs = [_reference(oracle, x, s["box"], 1.0, max_size=8) for x in frames]
    acc, hacc = np.zeros(8, dtype=np.int64), np.zeros(9, dtype=np.int64)
    for m in range(3):
        ns, fr, hist, series = reads[m]
        acc, hacc = acc + refs[m]["fr"], hacc + refs[m]["hist"]
        assert ns == m + 1 and np.array_equal(fr, acc) and np.array_equal(hist, hacc)
        assert len(series) == min(m + 1, 2) and all(np.array_equal(series[k], refs[k]["fr"]) for k in range(len(series)))
    assert refs[2]["hist"][8] > 0 and refs[2]["sizes"].max() > 8        # the overflow entry is in use
    assert ns1 == 1 and np.array_equal(fr1, refs[2]["fr"]) and np.array_equal(hist1, refs[2]["hist"])
    assert np.array_equal(series1[0], refs[2]["fr"])
    assert np.array_equal(part1[0], refs[2]["label"]) and np.array_equal(part1[1], refs[2]["size"])


def test_a_large_histogram_takes_the_global_atomics(oracle):
    """max_size above what the per-block LDS histogram holds (1024): the same counts by the other route."""
    c = _liquid(oracle)
    with _handle(4000, 3, c["s"]["box"], 2.5, c["x"], pot=LJ) as dev:
        d = _sample(dev, R_LIQUID, max_size=2048)
    r = _reference(oracle, c["x"], c["s"]["box"], R_LIQUID, max_size=2048)
    assert r["fr"][2] > 1024                                # the largest cluster lands past the LDS route's last bin
    _check(d, r, "liquid, max_size 2048")
    assert len(d["hist"]) == 2049 and d["hist"][r["fr"][2]] >= 1


def test_the_last_frame_survives_a_list_rebuild_and_an_upload():
    from moleculardynamics.jl_amd import MDDevice
    s = lj_system(4000)
    with MDDevice(3, s["n"], s["box"], 2.5) as dev:
        dev.set_potential(0, LJ)
        dev.upload(s["x"], s["v"], s["f"], s["img"], s["diam"])
        dev.run(20, 0.002)
        dev.cluster_setup(1.0, ALL, 1024, 1)
        dev.cluster_sample()
        before = dev.cluster_particles()
        r0 = dev.stats()["rebuilds"]
        for _ in range(20):
            dev.run(50, 0.004)
            if dev.stats()["rebuilds"] > r0:
                break
        assert dev.stats()["rebuilds"] > r0
        for a, b in zip(dev.cluster_particles(), before):
            assert np.array_equal(a, b)
        dev.upload(s["x"][::-1].copy(), s["v"], s["f"], s["img"], s["diam"])
        dev.compute_forces()                                # a build on other positions
        for a, b in zip(dev.cluster_particles(), before):
            assert np.array_equal(a, b)
        assert np.unique(before[0]).size > 100 and before[1].max() > 10      # a frame that tells particles apart


@pytest.mark.parametrize("switch", [None, "MDHIP_NO_FUSED_STEP"])
def test_a_sample_changes_nothing(monkeypatch, switch):
    from moleculardynamics.jl_amd import MDDevice
    if switch:
        monkeypatch.setenv(switch, "1")
    s = lj_system(4000)
    out = []
    for sample in (False, True):
        with MDDevice(3, s["n"], s["box"], 2.5) as dev:
            dev.set_potential(0, LJ)
            dev.upload(s["x"], s["v"], s["f"], s["img"], s["diam"])
            if sample:
                dev.cluster_setup(1.0, ALL, 64, 8)
                dev.cluster_sample()                        # the first call after upload: the list-invalid path
            res = []
            for _ in range(4):
                res.append(dev.run(10, 0.002))
                if sample:
                    dev.cluster_sample()
            out.append((res, dev.download(), dev.stats()["fused"]))
    (ra, da, fa), (rb, db, fb) = out
    assert fa == fb and (fa == 0 or not switch)
    assert ra == rb
    for u, w in zip(da, db):
        assert np.array_equal(u, w)


def test_refusals():
    from moleculardynamics.jl_amd import MDDevice, MdhipError, _lib
    with MDDevice(3, 1000, 12.0, 2.5) as dev:
        for call in (dev.cluster_sample, dev.cluster_read, dev.cluster_reset, dev.cluster_particles):
            with pytest.raises(MdhipError, match="no setup"):
                call()
        with pytest.raises(MdhipError, match="exceeds the list cutoff"):
            dev.cluster_setup(2.5000001)
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            with pytest.raises(MdhipError, match="r_bond"):
                dev.cluster_setup(bad)
        for bad in (2, -1):
            with pytest.raises(MdhipError, match="members"):
                dev.cluster_setup(1.5, bad)
        for kw, msg in ((dict(max_size=0), "max_size"), (dict(max_size=65537), "max_size"), (dict(nseries=-1), "nseries"),
                        (dict(nseries=(1 << 20) + 1), "nseries")):
            with pytest.raises(MdhipError, match=msg):
                dev.cluster_setup(1.5, ALL, **kw)
        with pytest.raises(MdhipError, match="md_boo_setup first"):
            dev.cluster_setup(1.5, SOLID)
        with pytest.raises(MdhipError, match="no setup"):   # a refused setup leaves no sampler behind
            dev.cluster_sample()
        dev.cluster_setup(2.5, ALL, 65536, 1 << 20)         # the limits themselves are accepted
        dev.cluster_setup(1.5)
        with pytest.raises(MdhipError, match="no frame sampled"):
            dev.cluster_particles()
        dev.cluster_read()
        dev.boo_setup(1.5, 6)
        dev.cluster_setup(1.5, SOLID)
        with pytest.raises(MdhipError, match="md_boo_sample first"):
            dev.cluster_sample()
        dev.boo_setup(1.5, 4)                               # a new bond-order setup has no frame either
        with pytest.raises(MdhipError, match="md_boo_sample first"):
            dev.cluster_sample()
    lib = _lib.load()
    h = ctypes.c_void_p()
    n = 4000
    box = (ctypes.c_double * 9)(20, 0, 0, 0, 20, 0, 0, 0, 20)
    assert lib.md_create_domain(3, n, n, box, 2.5, -1, 0, 1, ctypes.byref(h)) == 0, lib.md_last_error(None)
    try:
        assert lib.md_cluster_setup(h, 1.5, 0, 10, 0) != 0
        assert b"slab" in lib.md_last_error(h)
        for fn in (lib.md_cluster_sample, lib.md_cluster_reset):
            assert fn(h) != 0
            assert b"slab" in lib.md_last_error(h)
    finally:
        lib.md_destroy(h)


def test_run_simulation_and_the_one_shot(tmp_path, oracle):
    """clusters= (with bond_order=) leaves the run's own files unchanged; compute_clusters returns the final frame's
    labels, sizes and frame vector, in both modes."""
    import moleculardynamics.jl_amd as md
    n = 4096
    params = md.Parameters(0.8, n, 0.002, md.LennardJones())

    def fresh(path):
        st = md.initialize_state(params, path, random_init=True, cutoff=2.5, rng=np.random.default_rng(11))
        st.velocities = md.initialize_velocities(1.5, np.random.default_rng(12), n, 3)
        return st

    def files(path):
        return {f: open(os.path.join(path, f), "rb").read() for f in ("thermo.txt", "trajectory.xyz")}

    ensemble = md.NVT(1.5, 0.05)
    pa, pb = str(tmp_path / "a"), str(tmp_path / "b")
    sa, sb = fresh(pa), fresh(pb)
    bo = md.BondOrder(1.5)
    cl = md.ClusterAnalysis(1.5, members="solid", every=2, max_size=16)
    call = md.ClusterAnalysis(1.1)
    md.run_simulation(sa, params, ensemble, 31, 10, pa, bond_order=bo, clusters=cl)
    md.run_simulation(sb, params, ensemble, 31, 10, pb)
    assert bo.nsamples == 4 and cl.nsamples == 2 and list(cl.steps) == [0, 20]
    assert files(pa) == files(pb)
    assert np.array_equal(np.asarray(sa.system.positions), np.asarray(sb.system.positions))
    assert np.array_equal(np.asarray(sa.velocities), np.asarray(sb.velocities))
    # the solid members of the cluster frames are the solid particles of the bond-order frames of the same steps
    assert np.array_equal(cl.frames[:, 0], bo.frames[[0, 2], 6].astype(np.int64))
    lines = open(os.path.join(pa, "clusters.txt")).read().splitlines()
    assert lines[0] == "# members solid r_bond 1.500000 max_size 16 nsamples 2" and lines[2] == "# s n(s)" and len(lines) == 19
    assert len(open(os.path.join(pa, "clusters_series.txt")).read().splitlines()) == 3
    assert not os.path.exists(os.path.join(pb, "clusters.txt"))
    assert cl.hist_size.sum() == cl.sum_fr[1] and cl.mean_largest() <= cl.sum_fr[0] / 2.0 + 1e-12
    md.run_simulation(sb, params, ensemble, 11, 10, pb, clusters=call)
    assert call.nsamples == 2 and call.sum_fr[0] == 2 * n and call.weight_average_size() >= 1.0
    labels, sizes, fr = md.compute_clusters(sa, params, 1.1)
    x = np.asarray(sa.system.positions)
    r = _reference(oracle, x, np.diag(np.asarray(sa.unitcell)).copy(), 1.1)
    assert np.array_equal(labels, r["label"]) and np.array_equal(sizes, r["size"]) and np.array_equal(fr, r["fr"])
    ls, ss, frs = md.compute_clusters(sa, params, 1.5, members="solid", bond_order=md.BondOrder(1.5))
    b = md.compute_bond_order(sa, params, 1.5)
    assert np.array_equal(ls >= 0, b["solid"]) and frs[0] == np.count_nonzero(b["solid"]) and np.array_equal(ss > 0, b["solid"])
    for st in (sa, sb):
        st.system.device.close()
