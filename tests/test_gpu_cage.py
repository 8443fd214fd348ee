"""-m gpu: cage-relative dynamics and bond breaking sampled on the device (md_cage_*, md_cage.hpp).

The reference is numpy (tests/cage_reference.py): the origin's pair set from the oracle on the downloaded origin frame
(tests/test_gpu_bond_order.py's construction, orthorhombic and triclinic), the displacements from the two downloaded
frames -- nothing from the code under test.

Guards, asserted first (conditions, not tolerances): no origin pair with |d2 - thr| <= 1e-9 thr, no bond at the sample
time within the same band of its break threshold (the two sides round del differently at the 1e-16 level and would
otherwise be allowed to disagree about a bond), max n_i <= max_neigh.

Tolerances: Del^CR is a sum of <= 33 fp64 terms of magnitude |Del|, error <~ 40 eps max|Del| ~ 1e-14 max|Del|, while a
wrong, missing or doubled neighbour moves it by >= |Del_j| / 32.  The handle reports d2 = |Del^CR|^2 per particle:
1e-12 max(1, max d2) per particle, 1e-12 N max(1, max d2) on a row sum of d2 (max(1, max d2)^2 on d4, d N on the cosine
sums); every integer exact: n_i, broken, counts, hist_broken, overflow.

Measured worst cases (MI355X): see DESIGN.md section 17."""
import ctypes
import math
import os
import types

import numpy as np
import pytest

from tests import boo_reference as lattices
from tests import cage_reference as ref
from tests.test_gpu_bond_order import TRIC_U, WALKS, _canon_delta, _d2, _tric_delta, _walk_case
from tests.util import lj_system, poly_system

pytestmark = pytest.mark.gpu
LJ = [1.0, 1.0, 2.5]
Q2 = [2.0 * math.pi, 7.0]
TOL = 1e-12


# ---------------------------------------------------------------------------------------------------------------------
# the reference side

def _bonds(oracle, x, cell, r, diam, scaled, tric=False):
    """(pairs, del) of the origin's bonds, d2 < (r s)^2, the first guard asserted on every pair the oracle finds within a
    slightly larger radius."""
    n = len(x)
    wide = r * (diam.max() if scaled else 1.0) * (1.0 + 1e-6)
    if tric:
        with oracle.set_cell(cell):
            _, _, _, pairs = oracle.forces_brute(x, np.ones(x.shape[1]), wide, oracle.make_pot(0, LJ), np.ones(n),
                                                 want_pairs=True)
        de = _tric_delta(x, cell, pairs)
    else:
        pairs = oracle.pairs_cells(x, cell, wide)
        de = _canon_delta(x, cell, pairs)
    d2 = _d2(de)
    thr2 = ref.threshold2(r, diam, pairs[:, 0], pairs[:, 1], scaled)
    assert not np.any(np.abs(d2 - thr2) <= 1e-9 * thr2), "a pair sits on the neighbour radius: change the seed"
    keep = d2 < thr2
    return pairs[keep], de[keep]


def _reference(oracle, f0, f1, cell, r_neigh, r_break, diam, scaled=False, q=Q2, tric=False, max_neigh=32):
    pairs, de = _bonds(oracle, f0[0], cell, r_neigh, diam, scaled, tric)
    r = ref.cage(f0[0], f0[1], f1[0], f1[1], cell, pairs, de, diam, r_break, scaled, q)
    assert not np.any(np.abs(r["b2"] - r["thr2"]) <= 1e-9 * r["thr2"]), "a bond sits on the break radius: change the seed"
    assert r["nnb"].max() <= max_neigh
    return r


def _frame(dev):
    x, _, _, img = dev.download()
    return x, img


def _result(dev, row):
    """What the handle reports about `row`, with the per-particle arrays of the last sample call."""
    nnb, d2, broken = dev.cage_particles()
    ns, sums, counts, hist, overflow = dev.cage_read()
    return dict(nnb=nnb, d2=d2, broken=broken, ns=ns[row], sums=sums[row].copy(), counts=counts[row].copy(),
                hist=hist[row].copy(), overflow=overflow)


def _check(d, r, label="", dim=3, nsamples=1):
    """The device's single-sample row d against the reference r; prints the measured worst case before asserting."""
    n = len(r["d2"])
    s1 = max(1.0, r["d2"].max())
    e = np.abs(d["d2"] - r["d2"]).max()
    es = np.abs(d["sums"] - r["sums"])
    print("%s N %d  max|Del| %.3e  max d2 %.3e  max |d2 - ref| %.3e  row err %s  broken %d of %d" % (
        label, n, np.abs(r["delta"]).max(), r["d2"].max(), e, np.array2string(es, precision=2), r["broken"].sum(),
        r["nnb"].sum()))
    assert d["overflow"] == 0 and d["ns"] == nsamples
    assert np.array_equal(d["nnb"], r["nnb"]) and np.array_equal(d["broken"], r["broken"])
    assert np.array_equal(d["counts"], r["counts"]) and np.array_equal(d["hist"], r["hist"])
    assert np.all(np.abs(d["d2"] - r["d2"]) <= TOL * s1)
    assert es[0] <= TOL * n * s1 and es[1] <= TOL * n * s1 * s1
    assert np.all(es[2:] <= TOL * n * dim)


def _agree(a, b, dim=3):
    """Two handles holding the same two frames: the integers are equal, the fp64 values agree to rounding."""
    n = len(a["d2"])
    s1 = max(1.0, a["d2"].max())
    for k in ("nnb", "broken", "counts", "hist"):
        assert np.array_equal(a[k], b[k])
    assert np.all(np.abs(a["d2"] - b["d2"]) <= TOL * s1)
    es = np.abs(a["sums"] - b["sums"])
    assert es[0] <= TOL * n * s1 and es[1] <= TOL * n * s1 * s1 and np.all(es[2:] <= TOL * n * dim)


def _device(s, cutoff=2.5, pot=LJ, kind=0):
    from moleculardynamics.jl_amd import MDDevice
    dev = MDDevice(s["dim"], s["n"], s["box"], cutoff)
    dev.set_potential(kind, pot)
    dev.upload(s["x"], s["v"], s["f"], s["img"], s["diam"])
    return dev


def _run_past_a_rebuild(dev, dt, chunk=50, tries=40):
    r0 = dev.stats()["rebuilds"]
    for _ in range(tries):
        dev.run(chunk, dt)
        if dev.stats()["rebuilds"] > r0:
            return
    raise AssertionError("no list rebuild happened")


# ---------------------------------------------------------------------------------------------------------------------
# 1: rigid drift -- every particle flies with the same velocity through a zero potential

@pytest.mark.parametrize("shear", [0.0, 4.5])
def test_rigid_drift_is_removed_exactly(shear):
    from moleculardynamics.jl_amd import MDDevice
    from tests.test_gpu_triclinic import _fill
    U = np.array([[18.0, shear, 0.0], [0.0, 17.5, 0.0], [0.0, 0.0, 18.0]])
    n, dt = 3600, 0.01                                        # 14 tiles + 16; the lattice has 3840 sites without shear
    x = _fill(U, n, np.random.default_rng(31))
    vel = np.array([9.0, -7.0, 8.0])
    v = np.tile(vel, (n, 1))
    lags = [1, 700]
    with MDDevice(3, n, U, 2.5) as dev:
        dev.set_potential(0, [0.0, 1.0, 2.5])
        dev.upload(x, v, np.zeros_like(x), np.zeros((n, 3), np.int32), np.ones(n))
        dev.dyn_setup(1, len(lags))
        dev.cage_setup(1, len(lags), 1.5, 1.5, False, 32, Q2)
        dev.dyn_origin(0)
        dev.cage_origin(0)
        done = 0
        for k, l in enumerate(lags):
            dev.run(l - done, dt)
            done = l
            dev.dyn_sample([0], [k])
            dev.cage_sample([0], [k])
            nnb, d2, broken = dev.cage_particles()
            print("shear %.1f lag %d: max d2_CR %.3e, neighbours %d..%d" % (shear, l, d2.max(), nnb.min(), nnb.max()))
            assert d2.max() <= 1e-20 and not broken.any() and nnb.min() > 0
        _, dsums, _ = dev.dyn_read()
        ns, sums, counts, hist, overflow = dev.cage_read()
        img = dev.download()[3]
    assert np.abs(img).max() >= 3                             # the cell was crossed at least three times
    assert overflow == 0 and list(ns) == [1, 1]
    for k, l in enumerate(lags):
        want = (l * dt) ** 2 * float(vel @ vel)
        assert abs(dsums[k, 0] / n - want) <= 1e-9 * want     # the plain MSD sees the whole flight ...
        assert sums[k, 0] <= n * 1e-20                        # ... the cage-relative one none of it
        assert counts[k, 0] == n and counts[k, 2] == counts[k, 1] == nnb.sum()      # C_B = 1 exactly
        assert hist[k, 0] == n and hist[k, 1:].sum() == 0
        assert np.all(np.abs(sums[k, 2:] - 3.0 * n) <= 1e-9)  # cos(q 0) on every axis


# ---------------------------------------------------------------------------------------------------------------------
# 2: one hop on a lattice, both frames given by upload

def _hop_case(dim):
    if dim == 2:
        x, box = lattices.hexagonal(24, 14, 1.0)             # N = 672 = 2 tiles + 160; neighbours at 1, then sqrt(3)
        h, r, nn = np.array([0.6, 0.0]), 1.3, 6
        # the bonds to the neighbours at (-1, 0) and (-1/2, +-sqrt(3)/2) stretch to 1.6 and 1.40 > 1.3; the others shorten
        lost = [(-1.0, 0.0), (-0.5, math.sqrt(0.75)), (-0.5, -math.sqrt(0.75))]
        kind, pot, cutoff = 2, [1.25, 0.2], 1.5
    else:
        x, box = lattices.fcc(6, 1.6)                         # N = 864 = 3 tiles + 96; neighbours at 1.131, then 1.6
        h, r, nn = np.array([0.5, 0.0, 0.0]), 1.35, 12
        # the four bonds to neighbours at x = -0.8 stretch to |(-1.3, 0.8, 0)| = 1.526 > 1.35; at x = 0 to 1.237: they hold
        lost = [(-0.8, 0.8, 0.0), (-0.8, -0.8, 0.0), (-0.8, 0.0, 0.8), (-0.8, 0.0, -0.8)]
        kind, pot, cutoff = 0, [1.0, 1.0, 1.5], 1.5
    return x, box, h, r, nn, np.array(lost), kind, pot, cutoff


@pytest.mark.parametrize("dim", [2, 3])
def test_one_hop_on_a_lattice(oracle, dim):
    from moleculardynamics.jl_amd import MDDevice
    x0, box, h, r, nn, lost, kind, pot, cutoff = _hop_case(dim)
    n = len(x0)
    p = n // 2 + 5                                            # the hopper, away from every face
    A = 0.02
    u = np.zeros_like(x0)
    u[:, 1] = A * np.sin(2.0 * math.pi * x0[:, 0] / box[0])   # a smooth transverse field every particle follows
    x1 = x0 + u
    x1[p] += h
    z, zi = np.zeros_like(x0), np.zeros(x0.shape, dtype=np.int32)
    with MDDevice(dim, n, box, cutoff) as dev:
        dev.set_potential(kind, pot)
        dev.upload(x0, z, z, zi, np.ones(n))
        dev.cage_setup(1, 1, r, r, False, 16, Q2)
        f0 = _frame(dev)
        dev.cage_origin(0)
        dev.upload(x1, None, None, zi)
        f1 = _frame(dev)
        dev.cage_sample([0], [0])
        d = _result(dev, 0)
    rr = _reference(oracle, f0, f1, box, r, r, np.ones(n), False, Q2, max_neigh=16)
    _check(d, rr, "hop %d-D" % dim, dim)
    assert np.all(d["nnb"] == nn)
    # by hand: who is where around the hopper
    off = x0 - x0[p]
    off -= box * np.rint(off / box)
    lost_ids = [int(np.argmin(np.abs(off - o).sum(axis=1))) for o in lost]
    assert all(np.abs(off[j] - o).max() < 1e-9 for j, o in zip(lost_ids, lost))
    neigh = np.flatnonzero((np.sum(off * off, axis=1) < r * r) & (np.arange(n) != p))
    assert len(neigh) == nn
    want_broken = np.zeros(n, dtype=np.int64)
    want_broken[p] = len(lost)
    want_broken[lost_ids] = 1
    assert np.array_equal(d["broken"], want_broken)           # the directed broken count, exactly
    hist = np.zeros(33, dtype=np.int64)
    hist[0], hist[1], hist[len(lost)] = n - 1 - len(lost), len(lost), 1
    assert np.array_equal(d["hist"], hist)
    assert list(d["counts"]) == [n, n * nn, n * nn - 2 * len(lost)]
    # the hopper keeps its hop (its neighbours moved with the field, which is smooth: second differences only), each
    # neighbour loses its share h / n of it.  The field's part of Del^CR is u_i - mean u_j = -(1/2) u'' <dx^2> + O(k^4):
    # at most A k^2 max dx^2 / 2; twice that is allowed
    curv = A * (2.0 * math.pi / box[0]) ** 2 * float((off[neigh, 0] ** 2).max())
    hh = float(np.sqrt(h @ h))
    assert abs(math.sqrt(d["d2"][p]) - hh) <= curv
    assert np.all(np.abs(np.sqrt(d["d2"][neigh]) - hh / nn) <= curv)
    others = np.setdiff1d(np.arange(n), np.append(neigh, p))
    assert np.all(np.sqrt(d["d2"][others]) <= curv) and np.abs(rr["delta"][others]).max() > 0.9 * A


# ---------------------------------------------------------------------------------------------------------------------
# 3: independent displacements -- free Brownian diffusion through run_simulation

@pytest.mark.parametrize("lag", [1, 5, 20])
def test_independent_displacements(tmp_path, lag):
    """Del^CR_i = Del_i - mean of n_i independent Del_j: <d2> = 2 d dt l (1 + <1 / n_i>)."""
    import moleculardynamics.jl_amd as md
    n, d, dt = 1 << 14, 2, 1e-3
    params = md.Parameters(0.5, n, dt, md.LennardJones(epsilon=0.0))
    st = md.initialize_state(params, str(tmp_path), dimension=2, random_init=True, cutoff=2.5, rng=np.random.default_rng(7))
    cage = md.CageDynamics(1.5, max_neighbours=32, lags=[lag], origin_every=lag)
    md.run_simulation(st, params, md.Brownian(1.0), lag + 1, 100000, str(tmp_path), cage=cage, write_trajectory=False)
    nnb, d2, broken = st.system.device.cage_particles()       # the run's only sample: origin at 0, sample at `lag`
    st.system.device.close()
    assert list(cage.nsamples) == [1] and os.path.isfile(os.path.join(str(tmp_path), "cage.txt"))
    has = nnb > 0
    assert cage.counts[0, 0] == np.count_nonzero(has) > 0.9 * n and cage.counts[0, 1] == nnb.sum()
    want = 2.0 * d * dt * lag * (1.0 + float(np.mean(1.0 / nnb[has])))
    sigma = float(np.std(d2[has], ddof=1)) / math.sqrt(np.count_nonzero(has))
    got = cage.msd()[0]
    print("lag %d: <d2_CR> %.6e, expected %.6e, sigma %.2e (%.2f sigma), <1/n> %.4f, C_B %.4f" % (
        lag, got, want, sigma, (got - want) / sigma, np.mean(1.0 / nnb[has]), cage.bond_correlation()[0]))
    assert abs(got - want) <= 5.0 * sigma
    assert abs(got - float(np.mean(d2[has]))) <= 1e-12 * want


# ---------------------------------------------------------------------------------------------------------------------
# 4: parity against the reference -- the LJ liquid, four handles

_cache = {}
R_N, R_B = 1.5, 1.7


def _liquid(oracle):
    """lj_system(4000) after 200 NVT steps; origins at two frames, a sample past a list rebuild; two slots and several rows
    in one call; the frames and the references."""
    if "liq" not in _cache:
        from moleculardynamics.jl_amd import _lib
        from moleculardynamics.jl_amd.thermostat import draw_bussi
        s = lj_system(4000)
        with _device(s) as dev:
            nf = 3.0 * (s["n"] - 1.0)
            r1, r2 = draw_bussi(nf, np.random.default_rng(5), 200)
            dev.run(200, 0.002, _lib.MD_NVT, 0.1, nf, np.full(200, 1.0), r1, r2)
            dev.cage_setup(2, 4, R_N, R_B, False, 32, Q2)
            fa = _frame(dev)
            dev.cage_origin(0)
            dev.run(30, 0.004)
            fb = _frame(dev)
            dev.cage_origin(1)
            _run_past_a_rebuild(dev, 0.004)
            fc = _frame(dev)
            dev.cage_sample([0, 1, 0], [0, 1, 2])
            d0 = _result(dev, 0)                               # (the per-particle arrays are the call's last entry: slot 0)
            d2 = _result(dev, 2)
            d1row = _result(dev, 1)
            dev.cage_sample([1], [3])
            d1 = _result(dev, 3)
            tiled = dev.stats()["tiled"]
        ra = _reference(oracle, fa, fc, s["box"], R_N, R_B, s["diam"])
        rb = _reference(oracle, fb, fc, s["box"], R_N, R_B, s["diam"])
        _cache["liq"] = dict(s=s, fa=fa, fb=fb, fc=fc, d0=d0, d1=d1, d2=d2, d1row=d1row, ra=ra, rb=rb, tiled=tiled)
    return _cache["liq"]


def _by_upload(dev, c):
    """The liquid's three frames given to a fresh handle by upload: the same origins and samples."""
    dev.cage_setup(2, 4, R_N, R_B, False, 32, Q2)
    dev.upload(c["fa"][0], None, None, c["fa"][1])
    dev.cage_origin(0)                                        # the first call after an upload: the origin builds the list
    dev.upload(c["fb"][0], None, None, c["fb"][1])
    dev.cage_origin(1)
    dev.upload(c["fc"][0], None, None, c["fc"][1])
    dev.cage_sample([1, 0], [1, 0])
    d0 = _result(dev, 0)
    dev.cage_sample([1], [3])
    return d0, _result(dev, 3)


def test_lj_liquid_after_a_run(oracle):
    c = _liquid(oracle)
    assert c["tiled"] == 1
    _check(c["d0"], c["ra"], "liquid, slot 0")
    _check(c["d1"], c["rb"], "liquid, slot 1")
    assert c["ra"]["broken"].sum() > 0 and 10.0 < c["ra"]["nnb"].mean() < 16.0
    # row 2 is row 0 again, bit for bit; row 1 of the three-entry call is slot 1's sample, as row 3 is
    assert c["d2"]["sums"].tobytes() == c["d0"]["sums"].tobytes() and np.array_equal(c["d2"]["counts"], c["d0"]["counts"])
    assert c["d1row"]["sums"].tobytes() == c["d1"]["sums"].tobytes() and np.array_equal(c["d1row"]["hist"], c["d1"]["hist"])
    assert np.any(c["fc"][1] != c["fa"][1])                   # some particles crossed a face between the frames


def test_lj_liquid_fresh_handle_by_upload(oracle):
    c = _liquid(oracle)
    z = np.zeros_like(c["s"]["x"])
    with _device(dict(c["s"], v=z)) as dev:
        d0, d1 = _by_upload(dev, c)
        assert dev.stats()["tiled"] == 1
    _check(d0, c["ra"], "liquid by upload, slot 0")
    _check(d1, c["rb"], "liquid by upload, slot 1")
    _agree(d0, c["d0"])
    _agree(d1, c["d1"])


def test_lj_liquid_global_gather_path(oracle, monkeypatch):
    c = _liquid(oracle)
    monkeypatch.setenv("MDHIP_NO_TILES", "1")
    with _device(c["s"]) as dev:
        d0, d1 = _by_upload(dev, c)
        assert dev.stats()["tiled"] == 0
    _check(d0, c["ra"], "liquid, global-gather, slot 0")
    _check(d1, c["rb"], "liquid, global-gather, slot 1")
    _agree(d0, c["d0"])


def test_lj_liquid_user_potential(oracle):
    from moleculardynamics.jl_amd import MDDevice
    from tests.test_gpu_parity import USER_LJ_SRC
    c = _liquid(oracle)
    s = c["s"]
    with MDDevice(3, s["n"], s["box"], 2.5) as dev:
        dev.set_potential_source(USER_LJ_SRC, "user_lj", [1.0, 2.5])
        dev.upload(s["x"], s["v"], s["f"], s["img"], s["diam"])
        d0, d1 = _by_upload(dev, c)
    _check(d0, c["ra"], "liquid, user potential, slot 0")
    _check(d1, c["rb"], "liquid, user potential, slot 1")
    _agree(d0, c["d0"])


# ---------------------------------------------------------------------------------------------------------------------
# 5: two dimensions, polydisperse, radii scaled by sigma_ij and not

@pytest.mark.parametrize("scaled,r_n,r_b", [(True, 1.2, 1.3), (False, 1.4, 1.4)])
def test_2d_polydisperse(oracle, scaled, r_n, r_b):
    s = poly_system(1200)
    with _device(s, cutoff=1.5, pot=[1.25, 0.2], kind=2) as dev:
        dev.run(60, 0.001)
        dev.cage_setup(1, 1, r_n, r_b, scaled, 32, Q2)
        f0 = _frame(dev)
        dev.cage_origin(0)
        _run_past_a_rebuild(dev, 0.001, chunk=300)
        f1 = _frame(dev)
        dev.cage_sample([0], [0])
        d = _result(dev, 0)
    r = _reference(oracle, f0, f1, s["box"], r_n, r_b, s["diam"], scaled)
    _check(d, r, "poly2d scaled=%s" % scaled, 2)
    assert r["broken"].sum() > 0


# ---------------------------------------------------------------------------------------------------------------------
# 5b: every walk of the origin store, in both dimensions, at the smallest size with a ragged last block

@pytest.mark.parametrize("dim,rows", WALKS)
def test_every_walk_with_a_ragged_last_block(oracle, monkeypatch, dim, rows):
    """tests/test_gpu_bond_order.py's N = 257 lattice with vacancies; the second frame, by upload, moves every particle by
    a normal step of 0.08 (some bonds break); the radii scale with sigma_ij where the diameters differ."""
    from moleculardynamics.jl_amd import MDDevice
    x0, box, diam = _walk_case(dim, rows, monkeypatch)
    x1 = x0 + np.random.default_rng(99).normal(0.0, 0.08, x0.shape)
    scaled = rows == "tile32"
    z, zi = np.zeros_like(x0), np.zeros(x0.shape, dtype=np.int32)
    with MDDevice(dim, 257, box, 1.5) as dev:
        dev.set_potential(0, [1.0, 1.0, 1.5])
        dev.upload(x0, z, z, zi, diam)
        dev.cage_setup(1, 1, 1.3, 1.3, scaled, 32, Q2)
        f0 = _frame(dev)
        dev.cage_origin(0)
        assert dev.stats()["tiled"] == (0 if rows == "rows32" else 1)
        dev.upload(x1, None, None, zi)
        f1 = _frame(dev)
        dev.cage_sample([0], [0])
        d = _result(dev, 0)
    r = _reference(oracle, f0, f1, box, 1.3, 1.3, diam, scaled)
    assert r["nnb"].sum() > 257 and r["broken"].sum() > 0
    _check(d, r, "N = 257, %d-D, %s" % (dim, rows), dim)


# ---------------------------------------------------------------------------------------------------------------------
# 6: the sheared cell, with boundary crossings

def test_general_cell(oracle):
    from moleculardynamics.jl_amd.initialization import initialize_velocities
    from tests.test_gpu_triclinic import _fill
    n = 4000
    rng = np.random.default_rng(4242)
    x = _fill(TRIC_U, n, rng)
    s = dict(n=n, dim=3, box=TRIC_U, x=x, v=initialize_velocities(1.2, rng, n, 3), f=np.zeros_like(x),
             img=np.zeros((n, 3), np.int32), diam=np.ones(n))
    with _device(s) as dev:
        dev.run(40, 0.002)
        dev.cage_setup(1, 1, R_N, R_B, False, 32, Q2)
        f0 = _frame(dev)
        dev.cage_origin(0)
        _run_past_a_rebuild(dev, 0.004)
        dev.run(200, 0.004)
        f1 = _frame(dev)
        dev.cage_sample([0], [0])
        d = _result(dev, 0)
    assert np.any(f1[1] != f0[1])                             # boundary crossings between the frames
    _check(d, _reference(oracle, f0, f1, TRIC_U, R_N, R_B, s["diam"], tric=True), "sheared cell")


# ---------------------------------------------------------------------------------------------------------------------
# 7: overflow

def test_overflow_is_counted_and_reported(tmp_path):
    from moleculardynamics.jl_amd import MDDevice
    import moleculardynamics.jl_amd as md
    x, box = lattices.fcc(6, 1.6)
    n = len(x)
    z = np.zeros_like(x)
    with MDDevice(3, n, box, 1.5) as dev:
        dev.set_potential(0, [1.0, 1.0, 1.5])
        dev.upload(x, z, z, np.zeros(x.shape, dtype=np.int32), np.ones(n))
        cage = md.CageDynamics(1.35, max_neighbours=4, lags=[1], origin_every=1)
        run = types.SimpleNamespace(total_steps=2, frequency=1, n=n, dim=3, dt=0.002, unitcell=np.diag(box), brownian=False)
        cage._begin(dev, run)
        dev.cage_origin(0)
        dev.cage_sample([0], [0])
        nnb, d2, broken = dev.cage_particles()
        ns, sums, counts, hist, overflow = dev.cage_read()
        assert overflow == n * (12 - 4) and np.all(nnb == 4) and list(counts[0]) == [n, 4 * n, 4 * n]
        dev.cage_reset()
        assert dev.cage_read()[4] == overflow                # the counter belongs to the stored origins: reset keeps both
        with pytest.raises(ValueError, match="max_neighbours = 4"):
            cage._finish(dev, run, str(tmp_path))
        assert not cage.nsamples.any() and not os.path.exists(os.path.join(str(tmp_path), "cage.txt"))
        dev.cage_setup(1, 1, 1.35, 1.35, False, 12)          # setup starts over
        dev.cage_origin(0)
        assert dev.cage_read()[4] == 0


# ---------------------------------------------------------------------------------------------------------------------
# 8: the accumulators; a sample changes nothing; a slot survives a rebuild and an upload

def test_accumulators_bit_for_bit():
    s = lj_system(4000)
    with _device(s) as dev:
        dev.cage_setup(1, 5, R_N, R_B, False, 32, Q2)
        dev.cage_origin(0)
        single = []
        for m in range(3):
            dev.run(10, 0.004)
            dev.cage_sample([0, 0], [m, 3])                   # row m alone, row 3 accumulates
            single.append(_result(dev, m))
        part = dev.cage_particles()
        dev.cage_sample([0], [4])                             # the same frame once more: the same bits
        again = _result(dev, 4)
        for a, b in zip(dev.cage_particles(), part):
            assert np.array_equal(a, b)
        assert again["sums"].tobytes() == single[2]["sums"].tobytes()
        assert np.array_equal(again["counts"], single[2]["counts"]) and np.array_equal(again["hist"], single[2]["hist"])
        tot = _result(dev, 3)
        acc, cnt, hist = np.zeros(2 + len(Q2)), np.zeros(3, dtype=np.int64), np.zeros(33, dtype=np.int64)
        for m in range(3):
            acc = acc + single[m]["sums"]
            cnt += single[m]["counts"]
            hist += single[m]["hist"]
            assert single[m]["ns"] == 1 and single[m]["hist"].sum() == single[m]["counts"][0] == 4000
        assert tot["ns"] == 3 and tot["sums"].tobytes() == acc.tobytes()
        assert np.array_equal(tot["counts"], cnt) and np.array_equal(tot["hist"], hist)
        assert single[2]["sums"][0] > single[0]["sums"][0] > 0.0
        dev.cage_reset()                                      # zeroes the rows, keeps the setup and the origin
        ns, sums, counts, hist, _ = dev.cage_read()
        assert not ns.any() and not sums.any() and not counts.any() and not hist.any()
        dev.cage_sample([0], [1])
        assert _result(dev, 1)["sums"].tobytes() == single[2]["sums"].tobytes()


@pytest.mark.parametrize("switch", [None, "MDHIP_NO_FUSED_STEP"])
def test_a_sample_changes_nothing(monkeypatch, switch):
    if switch:
        monkeypatch.setenv(switch, "1")
    s = lj_system(4000)
    out = []
    for sample in (False, True):
        with _device(s) as dev:
            if sample:
                dev.cage_setup(2, 2, R_N, R_B, False, 32, Q2)
                dev.cage_origin(0)                            # the first call after upload: the list-invalid path
            res = []
            for m in range(4):
                res.append(dev.run(10, 0.002))
                if sample:
                    dev.cage_sample([0, m % 2], [0, 1])
                    dev.cage_origin(1 - m % 2)
            out.append((res, dev.download(), dev.stats()["fused"]))
    (ra, da, fa), (rb, db, fb) = out
    assert fa == fb and (fa == 0 or not switch)
    assert ra == rb
    for u, w in zip(da, db):
        assert np.array_equal(u, w)


def test_a_slot_survives_a_rebuild_and_an_upload():
    """The table is keyed by particle id: a list rebuild re-sorts the handle's slots and an upload rewrites them, the stored
    origin answers as before."""
    s = lj_system(4000)
    with _device(s) as dev:
        dev.run(20, 0.002)
        dev.cage_setup(2, 2, R_N, R_B, False, 32, Q2)
        dev.cage_origin(1)
        _run_past_a_rebuild(dev, 0.004)
        fb = _frame(dev)
        dev.cage_sample([1], [0])
        before = _result(dev, 0)
        dev.upload(s["x"][::-1].copy(), s["v"], s["f"], s["img"], s["diam"])
        dev.compute_forces()                                  # a build on other positions
        dev.upload(fb[0], None, None, fb[1])
        dev.cage_sample([1], [1])
        after = _result(dev, 1)
    for k in ("nnb", "d2", "broken", "counts", "hist"):
        assert np.array_equal(before[k], after[k])
    assert before["sums"].tobytes() == after["sums"].tobytes()
    assert before["broken"].sum() > 0 and np.unique(before["d2"]).size > 3000     # a sample that tells particles apart


# ---------------------------------------------------------------------------------------------------------------------
# 9: refusals

def test_refusals(monkeypatch):
    from moleculardynamics.jl_amd import MDDevice, MdhipError, _lib
    n = 1000
    with MDDevice(3, n, 12.0, 2.5) as dev:
        for call in (lambda: dev.cage_origin(0), lambda: dev.cage_sample([0], [0]), dev.cage_particles, dev.cage_read,
                     dev.cage_reset):
            with pytest.raises(MdhipError, match="no setup"):
                call()
        for kw, msg in ((dict(nslots=0), "nslots"), (dict(nslots=65), "nslots"), (dict(nrows=0), "nrows"),
                        (dict(r_neigh=0.0), "r_neigh"), (dict(r_neigh=float("inf")), "r_neigh"),
                        (dict(r_neigh=float("nan")), "r_neigh"), (dict(r_break=1.4), "r_break"),
                        (dict(r_break=float("inf")), "r_break"), (dict(max_neigh=0), "max_neigh"),
                        (dict(max_neigh=33), "max_neigh"), (dict(q=np.arange(17.0)), "nq"), (dict(q=[float("nan")]), "finite")):
            a = dict(nslots=1, nrows=1, r_neigh=1.5, r_break=1.5, scaled=False, max_neigh=16, q=())
            a.update(kw)
            with pytest.raises(MdhipError, match=msg):
                dev.cage_setup(**a)
        lib = _lib.load()
        assert lib.md_cage_setup(dev._h, 1, 1, 1.5, 1.5, 2, 16, None, 0) != 0 and b"scaled" in lib.md_last_error(dev._h)
        with pytest.raises(MdhipError, match="no setup"):     # a refused setup leaves no sampler behind
            dev.cage_read()
        dev.cage_setup(64, 1, 2.5, 2.5, True, 32, np.arange(16.0))       # the limits themselves are accepted
        dev.cage_setup(2, 3, 1.5)
        for bad in (-1, 2):
            with pytest.raises(MdhipError, match=r"slot -?\d is out of range 0..1"):
                dev.cage_origin(bad)
        with pytest.raises(MdhipError, match="slot 0 is empty"):
            dev.cage_sample([0], [0])
        with pytest.raises(MdhipError, match="no sample taken"):
            dev.cage_particles()
        s = lj_system(n, rho=n / 12.0 ** 3)
        dev.set_potential(0, LJ)
        dev.upload(s["x"], s["v"], s["f"], s["img"], s["diam"])
        dev.cage_origin(0)
        with pytest.raises(MdhipError, match="slot 1 is empty"):
            dev.cage_sample([0, 1], [0, 0])
        with pytest.raises(MdhipError, match=r"row 3 is out of range 0..2"):
            dev.cage_sample([0], [3])
        with pytest.raises(MdhipError, match=r"slot 2 is out of range 0..1"):
            dev.cage_sample([2], [0])
        assert not dev.cage_read()[0].any()                   # a refused call adds nothing
        # the rows are complete only up to the list cutoff: the origin names both numbers
        dev.cage_setup(1, 1, 2.6)
        with pytest.raises(MdhipError, match=r"2\.6\d* .*exceeds the list cutoff 2\.5"):
            dev.cage_origin(0)
        dev.cage_setup(1, 1, 2.2, scaled=True)
        dev.cage_origin(0)                                    # diameters 1: 2.2 is within the cutoff
        dev.upload(None, None, None, None, np.linspace(0.8, 1.2, n))
        with pytest.raises(MdhipError, match=r"2\.64\d* \(r_neigh times the largest diameter\) exceeds the list cutoff 2\.5"):
            dev.cage_origin(0)
        # the table allocation: nslots N max_neigh (4 + 8 d) bytes
        monkeypatch.setenv("MDHIP_CAGE_ALLOC_LIMIT", "1000000")
        with pytest.raises(MdhipError, match=r"cannot allocate %d bytes .*3\*1000\*16\*\(4\+8\*3\)" % (3 * n * 16 * 28)):
            dev.cage_setup(3, 1, 1.5)
        with pytest.raises(MdhipError, match="no setup"):
            dev.cage_read()
        dev.cage_setup(1, 1, 1.5, max_neigh=2)                # 1000 * 2 * 28 bytes fit the limit
        monkeypatch.delenv("MDHIP_CAGE_ALLOC_LIMIT")
    lib = _lib.load()
    h = ctypes.c_void_p()
    box = (ctypes.c_double * 9)(20, 0, 0, 0, 20, 0, 0, 0, 20)
    assert lib.md_create_domain(3, 4000, 4000, box, 2.5, -1, 0, 1, ctypes.byref(h)) == 0, lib.md_last_error(None)
    try:
        assert lib.md_cage_setup(h, 1, 1, 1.5, 1.5, 0, 16, None, 0) != 0
        assert b"slab" in lib.md_last_error(h)
        for fn in (lambda: lib.md_cage_origin(h, 0), lambda: lib.md_cage_reset(h)):
            assert fn() != 0
            assert b"slab" in lib.md_last_error(h)
    finally:
        lib.md_destroy(h)


# ---------------------------------------------------------------------------------------------------------------------
# 10: run_simulation

def test_run_simulation_writes_cage_txt_and_nothing_else_changes(tmp_path):
    import moleculardynamics.jl_amd as md
    n = 4096
    params = md.Parameters(0.8, n, 0.002, md.LennardJones())

    def fresh(path):
        st = md.initialize_state(params, path, random_init=True, cutoff=2.5, rng=np.random.default_rng(11))
        st.velocities = md.initialize_velocities(1.5, np.random.default_rng(12), n, 3)
        return st

    ensemble = md.NVT(1.5, 0.05)
    pa, pb = str(tmp_path / "a"), str(tmp_path / "b")
    sa, sb = fresh(pa), fresh(pb)
    sched = dict(lags=[3, 10], origin_every=8)
    cage = md.CageDynamics(1.5, r_break=1.8, max_neighbours=32, **sched)
    md.run_simulation(sa, params, ensemble, 41, 10, pa, dynamics=md.SelfDynamics(**sched), cage=cage)
    md.run_simulation(sb, params, ensemble, 41, 10, pb, dynamics=md.SelfDynamics(**sched))
    assert set(os.listdir(pa)) == set(os.listdir(pb)) | {"cage.txt"}
    for f in os.listdir(pb):
        assert open(os.path.join(pa, f), "rb").read() == open(os.path.join(pb, f), "rb").read(), f
    assert np.array_equal(np.asarray(sa.system.positions), np.asarray(sb.system.positions))
    assert np.array_equal(np.asarray(sa.velocities), np.asarray(sb.velocities))
    lines = open(os.path.join(pa, "cage.txt")).read().splitlines()
    assert lines[0] == "# lag time msd_cr alpha2_cr Fs_cr(q=6.28319) C_B nsamples" and len(lines) == 3
    assert list(cage.nsamples) == [5, 4]                      # origins at 0, 8, .., 40; samples at m 8 + lag < 41
    cb, msd = cage.bond_correlation(), cage.msd()
    assert np.all((0.0 < cb) & (cb <= 1.0)) and 0.0 < msd[0] < msd[1]
    assert np.all(cage.counts[:, 0] <= cage.nsamples * n) and np.all(cage.counts[:, 0] > 0.99 * cage.nsamples * n)
    for st in (sa, sb):
        st.system.device.close()


# ---------------------------------------------------------------------------------------------------------------------
# the split of a call's pairs into launches of MD_CAGE_MAX_BATCH = 8

@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("npairs", [9, 16])
def test_one_call_with_more_pairs_than_a_batch_equals_one_call_per_pair(dim, npairs):
    """9 pairs (a ragged second launch) and 16 (two full ones) on three origins and five rows, at N = 257: handle A samples
    them in one call, handle B in calls of one pair, in order.  k_dyn_reduce adds a batch's entries to their rows in call
    order and the counts are integers, so every read-back is equal bit for bit -- the per-particle arrays included: `keep`
    marks the call's last entry alone, in a ragged last launch and in a full one."""
    from tests.test_gpu_dynamics import _assert_identical, _ragged_frames, _ragged_handle
    frames, box = _ragged_frames(dim)
    zi = np.zeros((257, dim), dtype=np.int32)
    slots, rows = [i % 3 for i in range(npairs)], [(2 * i) % 5 for i in range(npairs)]
    out = []
    for one_call in (True, False):
        with _ragged_handle(dim, box, frames[0]) as dev:
            dev.cage_setup(3, 5, 1.3, 1.3, False, 32, Q2)
            for s in range(3):
                dev.upload(frames[s], None, None, zi)
                dev.cage_origin(s)
            dev.upload(frames[3], None, None, zi)
            if one_call:
                dev.cage_sample(slots, rows)
            else:
                for a, b in zip(slots, rows):
                    dev.cage_sample([a], [b])
            out.append(list(dev.cage_read()) + list(dev.cage_particles()))
    _assert_identical(out[0], out[1])
    cnt, sums, counts, hist, overflow, nnb, d2cr, broken = out[0]
    assert list(cnt) == list(np.bincount(rows, minlength=5)) and overflow == 0
    assert np.all(sums[cnt > 0, 0] > 0.0) and nnb.sum() > 257 and d2cr.max() > 0.0
