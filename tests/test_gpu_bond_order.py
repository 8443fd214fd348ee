"""-m gpu: bond-orientational order sampled on the device (md_boo_*, md_boo.hpp).

The reference is numpy (tests/boo_reference.py): the pair set from the oracle on the downloaded frame, del in the
oracle's canonical form, Y_lm from scipy.special.lpmv, psi_k from atan2 -- nothing from the code under test.

Guards, asserted first (conditions, not tolerances): no pair has |d2 - rn2| <= 1e-9 rn2 (the two sides round del
differently at the 1e-16 level and would otherwise be allowed to disagree about a neighbour), no reference bond has
|s_ij - threshold| <= 1e-9.

Tolerances: each Y_lm is <= 1.02 in modulus and costs a few tens of fp64 operations, n_i <= 32, so q_lm, q, qbar and
s_ij carry errors of order 1e-14, while a wrong, missing or doubled neighbour moves q_lm by |Y| / n_i >= 1e-2: 1e-12
absolute per component and per invariant, 1e-12 N on the frame sums; n_i, c_i and the solid count exact; the histograms
are the bins of the downloaded per-particle values exactly; sum_fr and series are the frame vectors bit for bit.

The image of the sampler (32-byte records) always fits a tiled handle -- the rows address the force kernel's image with
16-bit byte offsets, so a tile's halo has at most 65535 / 24 records and the sampler's image at most 87360 bytes -- so no
shape, small or large, sends a tiled handle down another walk: md_rowwalk.hpp asserts that arithmetic at compile time and the
launch checks its premise on the handle; the global-gather kernels are run here through a handle created without tiles."""
import ctypes

import numpy as np
import pytest

from tests import boo_reference as ref
from tests.util import lj_system, poly_system

pytestmark = pytest.mark.gpu
LJ = [1.0, 1.0, 2.5]
TRIC_U = np.array([[18.0, 4.5, 0.0], [0.0, 17.5, 0.0], [0.0, 0.0, 18.0]])   # tests/test_gpu_stress.py's sheared cell
NBINS = 50
TOL = 1e-12
LITERATURE = {4: 0.19094, 6: 0.57452}                   # fcc, 12 neighbours (tests/test_bond_order.py's table)


def _canon_delta(x, box, pairs):
    """oracle/md_oracle.c canon_d2's displacement for the (a < b) pairs: b translated, every operation rounded on its own."""
    a, b = x[pairs[:, 0]], x[pairs[:, 1]]
    L = np.asarray(box, dtype=np.float64)
    d0 = b - a
    half = 0.5 * L
    s = np.where(d0 > half, -1.0, np.where(d0 < -half, 1.0, 0.0))
    return (b + s * L) - a


def _tric_delta(x, U, pairs):
    """oracle/md_oracle.c tric_d2's displacement: the 3^d translations in its loop order, the first strict minimum kept."""
    d = x.shape[1]
    a, b = x[pairs[:, 0]], x[pairs[:, 1]]
    best = np.full(len(pairs), 1e300)
    out = np.zeros_like(a)
    for s2 in ((-1, 0, 1) if d == 3 else (0,)):
        for s1 in (-1, 0, 1):
            for s0 in (-1, 0, 1):
                de = np.empty_like(a)
                for r in range(d):
                    t = float(s0) * U[r, 0] + float(s1) * U[r, 1]
                    if d == 3:
                        t = t + float(s2) * U[r, 2]
                    de[:, r] = (b[:, r] + t) - a[:, r]
                d2 = _d2(de)
                better = d2 < best
                best = np.where(better, d2, best)
                out[better] = de[better]
    return out


def _d2(de):
    d2 = de[:, 0] * de[:, 0] + de[:, 1] * de[:, 1]
    if de.shape[1] == 3:
        d2 = d2 + de[:, 2] * de[:, 2]
    return d2


def _neighbour_bonds(oracle, x, cell, r_n, tric=False):
    """(pairs, del) of the neighbour relation d2 < rn2, the first guard asserted on every pair the oracle finds within a
    slightly larger radius."""
    wide = r_n * (1.0 + 1e-6)
    if tric:
        n = len(x)
        with oracle.set_cell(cell):
            _, _, _, pairs = oracle.forces_brute(x, np.ones(x.shape[1]), wide, oracle.make_pot(0, LJ), np.ones(n),
                                                 want_pairs=True)
        de = _tric_delta(x, cell, pairs)
    else:
        pairs = oracle.pairs_cells(x, cell, wide)
        de = _canon_delta(x, cell, pairs)
    d2, rn2 = _d2(de), r_n * r_n
    assert not np.any(np.abs(d2 - rn2) <= 1e-9 * rn2), "a pair sits on the neighbour radius: change the seed"
    keep = d2 < rn2
    return pairs[keep], de[keep]


def _reference(oracle, x, cell, r_n, order, threshold, min_conn, tric=False):
    pairs, de = _neighbour_bonds(oracle, x, cell, r_n, tric)
    r = ref.bond_order(len(x), pairs, de, order, threshold, min_conn)
    assert not np.any(np.abs(r["sij"] - threshold) <= 1e-9), "a bond sits on the threshold: change the seed"
    assert r["nnb"].max() <= 32
    return r


def _sample(dev, r_n, order, threshold=0.7, min_conn=7, nseries=4):
    """One sample on a fresh setup; everything the handle reports about it."""
    dev.boo_setup(r_n, order, NBINS, threshold, min_conn, nseries)
    dev.boo_sample()
    nnb, q, qbar, nconn = dev.boo_particles()
    ns, fr, hq, hb, hn, hc, series = dev.boo_read()
    return dict(nnb=nnb, q=q, qbar=qbar, conn=nconn, qlm=dev.boo_qlm(), ns=ns, fr=fr, hq=hq, hb=hb, hn=hn, hc=hc,
                series=series)


def _check(d, r, min_conn, label=""):
    """The device's sample d against the reference r."""
    n = len(r["q"])
    eq = np.abs(d["qlm"] - r["qlm"]).max()
    print("%s N %d  max |qlm - ref| %.3e  |q - ref| %.3e  |qbar - ref| %.3e  fr err %s" % (
        label, n, eq, np.abs(d["q"] - r["q"]).max(), np.abs(d["qbar"] - r["qbar"]).max(),
        np.array2string(np.abs(d["fr"] - r["fr"]), precision=2)))
    assert np.array_equal(d["nnb"], r["nnb"]) and np.array_equal(d["conn"], r["conn"])
    assert d["qlm"].shape == r["qlm"].shape
    assert np.all(np.abs(d["qlm"].real - r["qlm"].real) <= TOL) and np.all(np.abs(d["qlm"].imag - r["qlm"].imag) <= TOL)
    assert np.all(np.abs(d["q"] - r["q"]) <= TOL) and np.all(np.abs(d["qbar"] - r["qbar"]) <= TOL)
    assert np.all(d["q"] <= 1.0 + TOL) and np.all(d["qbar"] <= 1.0 + TOL)
    # the frame vector: one sample, so sum_fr is it -- and so is the series row, bit for bit
    assert d["ns"] == 1 and d["series"].shape == (1, 8) and np.array_equal(d["series"][0], d["fr"])
    assert np.all(np.abs(d["fr"][:4] - r["fr"][:4]) <= TOL * n)
    assert d["fr"][4] == r["fr"][4] == d["nnb"].sum() and d["fr"][5] == r["fr"][5] == d["conn"].sum()
    assert d["fr"][6] == r["fr"][6] == np.count_nonzero(d["conn"] >= min_conn)
    assert abs(d["fr"][7] - r["fr"][7]) <= TOL
    # the histograms: the stated bin rule on the values the device itself reports
    assert np.array_equal(d["hq"], ref.bins(d["q"], NBINS)) and np.array_equal(d["hb"], ref.bins(d["qbar"], NBINS))
    assert np.array_equal(d["hn"], ref.clamped_counts(d["nnb"])) and np.array_equal(d["hc"], ref.clamped_counts(d["conn"]))


def _agree(a, b):
    """Two handles holding the same frame agree to rounding."""
    assert np.array_equal(a["nnb"], b["nnb"]) and np.array_equal(a["conn"], b["conn"])
    for k in ("q", "qbar"):
        assert np.all(np.abs(a[k] - b[k]) <= TOL)
    assert np.all(np.abs(a["qlm"] - b["qlm"]) <= TOL)
    assert np.all(np.abs(a["fr"][:4] - b["fr"][:4]) <= TOL * len(a["q"])) and abs(a["fr"][7] - b["fr"][7]) <= TOL
    assert np.array_equal(a["fr"][4:7], b["fr"][4:7])


def _handle(n, dim, cell, cutoff, x, diam=None, kind=0, pot=None):
    from moleculardynamics.jl_amd import MDDevice
    dev = MDDevice(dim, n, cell, cutoff)
    dev.set_potential(kind, [1.0, 1.0, cutoff] if pot is None else pot)
    z = np.zeros_like(x)
    dev.upload(x, z, z, np.zeros(x.shape, dtype=np.int32), np.ones(n) if diam is None else diam)
    return dev


# ---------------------------------------------------------------------------------------------------------------------
# 1, 2: fcc, 6^3 cells, a = 1.6: N = 864 = 3 full tiles + 96; list cutoff 1.5, r_n = 1.35 (shells at 1.131 and 1.6)

@pytest.mark.parametrize("l", [6, 4])
def test_perfect_fcc(oracle, l):
    x, box = ref.fcc(6, 1.6)
    n = len(x)
    assert n == 864
    with _handle(n, 3, box, 1.5, x) as dev:
        xd = dev.download()[0]
        d = _sample(dev, 1.35, l, min_conn=12)
        assert dev.stats()["tiled"] == 1
    r = _reference(oracle, xd, box, 1.35, l, 0.7, 12)
    _check(d, r, 12, "fcc l=%d" % l)
    assert np.all(d["nnb"] == 12) and np.all(d["conn"] == 12) and d["fr"][6] == n
    assert np.all(np.abs(d["qbar"] - d["q"]) <= TOL)
    assert np.all(np.abs(d["q"] - LITERATURE[l]) <= 1e-5)
    assert abs(d["fr"][7] - d["q"][0]) <= TOL                # every site has the same orientation: global order = q_l


@pytest.mark.parametrize("l", [6, 4])
def test_jittered_fcc_every_component(oracle, l):
    x, box = ref.fcc(6, 1.6)
    x = x + np.random.default_rng(20240611).normal(0.0, 1e-2, x.shape)
    with _handle(len(x), 3, box, 1.5, x) as dev:
        xd = dev.download()[0]
        d = _sample(dev, 1.35, l)
    r = _reference(oracle, xd, box, 1.35, l, 0.7, 7)
    _check(d, r, 7, "jittered fcc l=%d" % l)
    assert d["qlm"].shape == (864, l + 1)
    assert np.abs(d["qlm"][:, 1:].imag).max() > 1e-3         # the phase convention is exercised: m > 0 is complex


# ---------------------------------------------------------------------------------------------------------------------
# 3, 4, 9: the LJ liquid, N = 4000 = 15 tiles + 160

_cache = {}


def _liquid(oracle):
    """The shared frame: lj_system(4000) after 200 NVT steps at kT = 1 on the device; the sample of that handle (inner rows
    active, list not fresh), the frame, the reference."""
    if "liq" not in _cache:
        from moleculardynamics.jl_amd import _lib
        from moleculardynamics.jl_amd.thermostat import draw_bussi
        s = lj_system(4000)
        from moleculardynamics.jl_amd import MDDevice
        with MDDevice(3, s["n"], s["box"], 2.5) as dev:
            dev.set_potential(0, LJ)
            dev.upload(s["x"], s["v"], s["f"], s["img"], s["diam"])
            nf = 3.0 * (s["n"] - 1.0)
            r1, r2 = draw_bussi(nf, np.random.default_rng(5), 200)
            dev.run(200, 0.002, _lib.MD_NVT, 0.1, nf, np.full(200, 1.0), r1, r2)
            st = dev.stats()
            d = _sample(dev, 1.5, 6)
            x, v, _, img = dev.download()
        r = _reference(oracle, x, s["box"], 1.5, 6, 0.7, 7)
        _cache["liq"] = dict(s=s, x=x, v=v, img=img, d=d, r=r, tiled=st["tiled"], rebuilds=st["rebuilds"])
    return _cache["liq"]


def test_lj_liquid_after_a_run(oracle):
    c = _liquid(oracle)
    assert c["tiled"] == 1
    _check(c["d"], c["r"], 7, "liquid, after md_run")
    assert 10.0 < c["d"]["fr"][4] / 4000 < 16.0              # a dense liquid's first shell


def test_lj_liquid_fresh_handle(oracle):
    c = _liquid(oracle)
    with _handle(4000, 3, c["s"]["box"], 2.5, c["x"], pot=LJ) as dev:
        d = _sample(dev, 1.5, 6)                           # the first call after upload: the sample builds the list
        assert dev.stats()["tiled"] == 1
    _check(d, c["r"], 7, "liquid, fresh handle")
    _agree(d, c["d"])


def test_global_gather_path(oracle, monkeypatch):
    c = _liquid(oracle)
    monkeypatch.setenv("MDHIP_NO_TILES", "1")
    with _handle(4000, 3, c["s"]["box"], 2.5, c["x"], pot=LJ) as dev:
        d = _sample(dev, 1.5, 6)
        assert dev.stats()["tiled"] == 0
        d4 = _sample(dev, 1.5, 4)
    _check(d, c["r"], 7, "liquid, global-gather")
    _agree(d, c["d"])
    _check(d4, _reference(oracle, c["x"], c["s"]["box"], 1.5, 4, 0.7, 7), 7, "liquid, global-gather l=4")


def test_user_potential(oracle):
    from moleculardynamics.jl_amd import MDDevice
    from tests.test_gpu_parity import USER_LJ_SRC
    c = _liquid(oracle)
    with MDDevice(3, 4000, c["s"]["box"], 2.5) as dev:
        dev.set_potential_source(USER_LJ_SRC, "user_lj", [1.0, 2.5])
        z = np.zeros_like(c["x"])
        dev.upload(c["x"], z, z, np.zeros(z.shape, dtype=np.int32), np.ones(4000))
        d = _sample(dev, 1.5, 6)
    _check(d, c["r"], 7, "liquid, user potential")
    _agree(d, c["d"])


# ---------------------------------------------------------------------------------------------------------------------
# 5: two dimensions

def test_perfect_hexagonal_lattice(oracle):
    x, box = ref.hexagonal(24, 14, 1.0)                     # N = 672 = 2 tiles + 160, box 24 x 24.25
    n = len(x)
    with _handle(n, 2, box, 1.5, x, kind=2, pot=[1.25, 0.2]) as dev:
        xd = dev.download()[0]
        d = _sample(dev, 1.3, 6, min_conn=6)
    r = _reference(oracle, xd, box, 1.3, 6, 0.7, 6)
    _check(d, r, 6, "hexagonal k=6")
    assert np.all(d["nnb"] == 6) and np.all(d["conn"] == 6) and d["fr"][6] == n
    assert np.all(np.abs(d["q"] - 1.0) <= TOL) and np.all(np.abs(d["qbar"] - 1.0) <= TOL) and abs(d["fr"][7] - 1.0) <= TOL
    assert d["qlm"].shape == (n, 1)


def test_2d_polydisperse_and_the_run_time_order(oracle):
    s = poly_system(1200)
    from moleculardynamics.jl_amd import MDDevice
    with MDDevice(2, s["n"], s["box"], 1.5) as dev:
        dev.set_potential(2, [1.25, 0.2])
        dev.upload(s["x"], s["v"], s["f"], s["img"], s["diam"])
        dev.run(60, 0.001)
        d6 = _sample(dev, 1.4, 6, min_conn=4)
        d4 = _sample(dev, 1.4, 4, min_conn=4)
        d1 = _sample(dev, 1.4, 1, min_conn=4)
        d12 = _sample(dev, 1.4, 12, min_conn=4)
        x = dev.download()[0]
    for k, d in ((6, d6), (4, d4), (1, d1), (12, d12)):
        _check(d, _reference(oracle, x, s["box"], 1.4, k, 0.7, 4), 4, "poly2d k=%d" % k)
    assert np.abs(d6["q"] - d4["q"]).max() > 1e-2            # the order is honoured


# ---------------------------------------------------------------------------------------------------------------------
# 6: general cell

def test_general_cell(oracle):
    from moleculardynamics.jl_amd import MDDevice
    from moleculardynamics.jl_amd.initialization import initialize_velocities
    from tests.test_gpu_triclinic import _fill
    U, n = TRIC_U, 4000
    rng = np.random.default_rng(4242)
    x0 = _fill(U, n, rng)
    v0 = initialize_velocities(1.2, rng, n, 3)
    with MDDevice(3, n, U, 2.5) as dev:
        dev.set_potential(0, LJ)
        dev.upload(x0, v0, np.zeros_like(x0), np.zeros((n, 3), np.int32), np.ones(n))
        dev.run(40, 0.002)
        d = _sample(dev, 1.5, 6)
        x = dev.download()[0]
    _check(d, _reference(oracle, x, U, 1.5, 6, 0.7, 7, tric=True), 7, "sheared cell")


# ---------------------------------------------------------------------------------------------------------------------
# 6b: every walk the samplers share (md_rowwalk.hpp), in both dimensions, at the smallest size with a ragged last block

WALKS = [(dim, rows) for dim in (3, 2) for rows in ("tile24", "tile32", "rows32")]


def _walk_case(dim, rows, monkeypatch):
    """(x, box, diam) of N = 257 = one full 256-lane tile + one lane -- the second block has 255 inactive lanes: a simple
    lattice of spacing 1.1 (7^3 or 17^2 sites, shells at 1.1 and 1.556) with vacancies and a jitter of 0.04, list cutoff 1.5.
    rows: "tile24" -- tiled rows over the 24-byte image (built-in LJ, one diameter); "tile32" -- over the 32-byte image (the
    diameters differ); "rows32" -- 32-bit global rows (a handle created without tiles)."""
    rng = np.random.default_rng(257 + dim)
    m = 7 if dim == 3 else 17
    g = np.arange(m)
    sites = np.stack(np.meshgrid(*([g] * dim), indexing="ij"), -1).reshape(-1, dim).astype(np.float64)
    x = 1.1 * (rng.permutation(sites)[:257] + 0.5) + rng.normal(0.0, 0.04, (257, dim))
    diam = rng.uniform(0.9, 1.1, 257) if rows == "tile32" else np.ones(257)
    if rows == "rows32":
        monkeypatch.setenv("MDHIP_NO_TILES", "1")
    return x, np.full(dim, 1.1 * m), diam


@pytest.mark.parametrize("dim,rows", WALKS)
def test_every_walk_with_a_ragged_last_block(oracle, monkeypatch, dim, rows):
    x, box, diam = _walk_case(dim, rows, monkeypatch)
    with _handle(257, dim, box, 1.5, x, diam=diam) as dev:
        xd = dev.download()[0]
        d6 = _sample(dev, 1.35, 6, min_conn=3)
        d4 = _sample(dev, 1.35, 4, min_conn=3)
        assert dev.stats()["tiled"] == (0 if rows == "rows32" else 1)
    for order, d in ((6, d6), (4, d4)):
        r = _reference(oracle, xd, box, 1.35, order, 0.7, 3)
        assert r["nnb"].min() > 0                            # every site has a neighbour, none has its full shell
        _check(d, r, 3, "N = 257, %d-D, %s, order %d" % (dim, rows, order))


# ---------------------------------------------------------------------------------------------------------------------
# 7: a sample changes nothing; the accumulators are the frame vectors bit for bit

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
                dev.boo_setup(1.5, 6, NBINS, 0.7, 7, 8)
                dev.boo_sample()                           # the first call after upload: the list-invalid path
            res = []
            for _ in range(4):
                res.append(dev.run(10, 0.002))
                if sample:
                    dev.boo_sample()
            out.append((res, dev.download(), dev.stats()["fused"]))
    (ra, da, fa), (rb, db, fb) = out
    assert fa == fb and (fa == 0 or not switch)
    assert ra == rb
    for u, w in zip(da, db):
        assert np.array_equal(u, w)


def test_accumulators_bit_for_bit():
    from moleculardynamics.jl_amd import MDDevice
    s = lj_system(4000)
    with MDDevice(3, s["n"], s["box"], 2.5) as dev:
        dev.set_potential(0, LJ)
        dev.upload(s["x"], s["v"], s["f"], s["img"], s["diam"])
        dev.boo_setup(1.5, 6, NBINS, 0.7, 7, 2)             # room for two of the three frame vectors
        last, sums, hists = [], [], []
        for m in range(3):
            dev.run(10, 0.002)
            dev.boo_sample()
            part = dev.boo_particles()
            ns, fr, hq, hb, hn, hc, series = dev.boo_read()
            assert ns == m + 1 and len(series) == min(m + 1, 2)
            sums.append(fr)
            hists.append((hq, hb, hn, hc, part))
            if m < 2:
                last.append(series[m].copy())
        # the same frame sampled again gives the same bits
        dev.boo_sample()
        again = dev.boo_particles()
        for a, b in zip(again, hists[2][4]):
            assert np.array_equal(a, b)
        ns, fr4, hq4, hb4, hn4, hc4, series = dev.boo_read()
        assert ns == 4
        # the third frame vector did not fit the series: the same frame once more, into an emptied one
        dev.boo_reset()
        ns0, fr0, hq0, _, _, _, series0 = dev.boo_read()
        assert ns0 == 0 and not fr0.any() and not hq0.any() and series0.shape == (0, 8)
        dev.boo_sample()
        ns1, fr1, hq1, hb1, hn1, hc1, series1 = dev.boo_read()
        assert ns1 == 1 and np.array_equal(fr1, series1[0])
        last.append(series1[0].copy())
        assert np.array_equal(series[:2], np.array(last[:2]))               # later samples are summed, not recorded
        acc = np.zeros(8)
        for m in range(3):
            acc = acc + last[m]
            assert np.array_equal(sums[m], acc)
        assert np.array_equal(fr4, acc + last[2])
        # the histograms accumulate the per-sample bins of the reported per-particle values
        tq, tn = np.zeros(NBINS, dtype=np.int64), np.zeros(33, dtype=np.int64)
        for m in range(3):
            nnb, q, qbar, conn = hists[m][4]
            tq += ref.bins(q, NBINS)
            tn += ref.clamped_counts(nnb)
            assert np.array_equal(hists[m][0], tq) and np.array_equal(hists[m][2], tn)
        assert np.array_equal(hq4, tq + ref.bins(again[1], NBINS)) and np.array_equal(hq1, ref.bins(again[1], NBINS))
        # setup again starts over
        dev.boo_setup(1.5, 4, 7, 0.5, 3, 0)
        ns, fr, hq, hb, hn, hc, series = dev.boo_read()
        assert ns == 0 and hq.shape == (7,) and not fr.any() and series.shape == (0, 8)


def test_the_last_frame_survives_a_list_rebuild():
    """md_boo_particles and md_boo_qlm return the SAMPLED frame in particle-id order whatever the handle did since: a list
    rebuild re-sorts the slots, an upload rewrites them."""
    from moleculardynamics.jl_amd import MDDevice
    s = lj_system(4000)
    with MDDevice(3, s["n"], s["box"], 2.5) as dev:
        dev.set_potential(0, LJ)
        dev.upload(s["x"], s["v"], s["f"], s["img"], s["diam"])
        dev.run(20, 0.002)
        dev.boo_setup(1.5, 6, NBINS, 0.7, 7, 1)
        dev.boo_sample()
        before, qlm = dev.boo_particles(), dev.boo_qlm()
        r0 = dev.stats()["rebuilds"]
        for _ in range(20):
            dev.run(50, 0.004)
            if dev.stats()["rebuilds"] > r0:
                break
        assert dev.stats()["rebuilds"] > r0
        for a, b in zip(dev.boo_particles(), before):
            assert np.array_equal(a, b)
        assert np.array_equal(dev.boo_qlm(), qlm)
        dev.upload(s["x"][::-1].copy(), s["v"], s["f"], s["img"], s["diam"])
        dev.compute_forces()                                # a build on other positions
        for a, b in zip(dev.boo_particles(), before):
            assert np.array_equal(a, b)
        assert np.array_equal(dev.boo_qlm(), qlm)
        assert before[0].min() > 0 and np.unique(before[1]).size > 3000     # a frame that tells particles apart


def test_many_bins_take_the_global_atomics(oracle):
    """More bins than the per-block LDS histogram holds (1024): the same counts by the other route."""
    c = _liquid(oracle)
    with _handle(4000, 3, c["s"]["box"], 2.5, c["x"], pot=LJ) as dev:
        dev.boo_setup(1.5, 6, 8192, 0.7, 7, 0)
        dev.boo_sample()
        nnb, q, qbar, conn = dev.boo_particles()
        _, _, hq, hb, hn, hc, _ = dev.boo_read()
    assert np.array_equal(hq, ref.bins(q, 8192)) and np.array_equal(hb, ref.bins(qbar, 8192))
    assert np.array_equal(hn, ref.clamped_counts(nnb)) and np.array_equal(hc, ref.clamped_counts(conn))
    assert np.all(np.abs(q - c["r"]["q"]) <= TOL)


# ---------------------------------------------------------------------------------------------------------------------
# 8: refusals

def test_refusals():
    from moleculardynamics.jl_amd import MDDevice, MdhipError, _lib
    with MDDevice(3, 1000, 12.0, 2.5) as dev:
        for call in (dev.boo_sample, dev.boo_read, dev.boo_reset, dev.boo_particles, dev.boo_qlm):
            with pytest.raises(MdhipError, match="no setup"):
                call()
        with pytest.raises(MdhipError, match="exceeds the list cutoff"):
            dev.boo_setup(2.5000001, 6)
        for bad in (5, 0, 8):
            with pytest.raises(MdhipError, match="must be 4 or 6"):
                dev.boo_setup(1.5, bad)
        for kw, msg in ((dict(nbins=0), "nbins"), (dict(nbins=8193), "nbins"), (dict(min_conn=33), "min_conn"),
                        (dict(min_conn=-1), "min_conn"), (dict(threshold=float("nan")), "threshold"),
                        (dict(nseries=-1), "nseries"), (dict(nseries=(1 << 20) + 1), "nseries")):
            with pytest.raises(MdhipError, match=msg):
                dev.boo_setup(1.5, 6, **kw)
        for bad in (0.0, -1.0, float("inf")):
            with pytest.raises(MdhipError, match="r_neigh"):
                dev.boo_setup(bad, 6)
        with pytest.raises(MdhipError, match="no setup"):   # a refused setup leaves no sampler behind
            dev.boo_sample()
        dev.boo_setup(2.5, 4, 8192, -1.0, 32, 1 << 20)      # the limits themselves are accepted
        dev.boo_setup(1.5, 6)
        for call in (dev.boo_particles, dev.boo_qlm):
            with pytest.raises(MdhipError, match="no frame sampled"):
                call()
        dev.boo_read()
    with MDDevice(2, 1000, 40.0, 1.5) as dev:
        for bad in (13, 0):
            with pytest.raises(MdhipError, match=r"order \(k\) must be in 1..12"):
                dev.boo_setup(1.4, bad)
        dev.boo_setup(1.4, 12)
        dev.boo_setup(1.4, 1)
    lib = _lib.load()
    h = ctypes.c_void_p()
    n = 4000
    box = (ctypes.c_double * 9)(20, 0, 0, 0, 20, 0, 0, 0, 20)
    assert lib.md_create_domain(3, n, n, box, 2.5, -1, 0, 1, ctypes.byref(h)) == 0, lib.md_last_error(None)
    try:
        assert lib.md_boo_setup(h, 1.5, 6, 10, 0.7, 7, 0) != 0
        assert b"slab" in lib.md_last_error(h)
        for fn in (lib.md_boo_sample, lib.md_boo_reset):
            assert fn(h) != 0
            assert b"slab" in lib.md_last_error(h)
    finally:
        lib.md_destroy(h)


def test_run_simulation_and_the_one_shot(tmp_path):
    """bond_order= leaves the run's own files unchanged, works with Brownian dynamics, and compute_bond_order returns the
    final frame's per-particle arrays."""
    import os
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
    bo = md.BondOrder(1.5, every=2)
    md.run_simulation(sa, params, ensemble, 31, 10, pa, bond_order=bo)
    md.run_simulation(sb, params, ensemble, 31, 10, pb)
    assert bo.nsamples == 2 and list(bo.steps) == [0, 20]
    assert files(pa) == files(pb)
    assert np.array_equal(np.asarray(sa.system.positions), np.asarray(sb.system.positions))
    assert np.array_equal(np.asarray(sa.velocities), np.asarray(sb.velocities))
    lines = open(os.path.join(pa, "bond_order.txt")).read().splitlines()
    assert lines[2] == "# bin q_density qbar_density count_q count_qbar" and len(lines) == 103
    assert sum(int(ln.split()[3]) for ln in lines[3:]) == 2 * n
    assert len(open(os.path.join(pa, "bond_order_series.txt")).read().splitlines()) == 3
    assert not os.path.exists(os.path.join(pb, "bond_order.txt"))
    assert 0.0 < bo.mean_qbar() < bo.mean_q() < 1.0 and 8.0 < bo.mean_neighbours() < 16.0
    r = md.compute_bond_order(sa, params, 1.5)
    assert r["q"].shape == (n,) and r["qlm"].shape == (n, 7) and r["solid"].dtype == bool
    assert np.array_equal(r["solid"], r["connections"] >= 7) and 0.0 <= r["global_order"] <= 1.0
    bo2 = md.BondOrder(1.5, order=4)
    md.run_simulation(sa, params, md.Brownian(1.5), 11, 10, pa, bond_order=bo2)
    assert bo2.nsamples == 2
    for st in (sa, sb):
        st.system.device.close()
