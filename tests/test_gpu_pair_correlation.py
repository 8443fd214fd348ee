"""-m gpu: marked pair correlations sampled on the device (md_mpc_*, md_mpc.hpp).

The reference is numpy (tests/mpc_reference.py): the pair set from the oracle on the downloaded frame, d2 in the oracle's
canonical form, the bin from the edge table, the terms as int64 -- nothing from the code under test.

User marks are dyadic (m / 256, |m| <= 256) with unit weights: every product, every partial sum and every scaled term is
exactly representable, so cnt, sum and self are compared EXACTLY.  With the bond-order frame as marks the reference takes
the device's own q_lm bits (md_boo_qlm) and forms t without a fused multiply-add, so a term may round to the
neighbouring integer: |sum - ref| <= 2 cnt[k] quanta, while a missing, doubled or mis-attached pair moves a bin by about
2^31 |t|; each such test asserts first that the median |ref sum| / (2 cnt) over the occupied bins exceeds 1000, so the
bound discriminates.  The same bound holds against marks from tests/boo_reference.py (they agree with the device's to
1e-12, which moves a term by at most 14 * 2 * 2 * 1e-12 * 2^31 < 0.2 quanta).

Not reachable at test sizes, reviewed by reading the code: the drain of the LDS words after 2^23 adds per lane, and the
2^31-pairs-per-bin check of k_mpc_finish (both need more than 10^9 pairs in one sample)."""
import ctypes
import os

import numpy as np
import pytest

from tests import boo_reference as boo
from tests import mpc_reference as ref
from tests.test_gpu_bond_order import LJ, TRIC_U, _handle, _reference
from tests.util import lj_system, poly_system

pytestmark = pytest.mark.gpu
Q = 2.0 ** -31                                              # the quantum at tmax = 1


def _pairs_d2(oracle, x, cell, r_max, tric=False):
    if tric:
        with oracle.set_cell(cell):
            _, _, _, pairs = oracle.forces_brute(x, np.ones(x.shape[1]), r_max, oracle.make_pot(0, LJ), np.ones(len(x)),
                                                 want_pairs=True)
        return pairs, ref.tric_d2(x, cell, pairs)
    pairs = oracle.pairs_cells(x, cell, r_max)
    return pairs, ref.canon_d2(x, cell, pairs)


def _dyadic(n, nc, seed):
    return np.random.default_rng(seed).integers(-256, 257, (n, nc)).astype(np.float64) / 256.0


def _user_sample(dev, marks, r_max, nbins, tmax=4.0):
    dev.mpc_setup(r_max, nbins, weights=np.ones(marks.shape[1]), tmax=tmax)
    dev.mpc_marks(marks)
    dev.mpc_sample()
    ns, acnt, asum, aself, tm, err = dev.mpc_read()
    cnt, tot, own = dev.mpc_last()
    assert ns == 1 and err == 0 and tm == ref.round_up_pow2(tmax)
    assert np.array_equal(acnt, cnt) and np.array_equal(asum, tot.astype(np.float64)) and aself == float(own)
    return cnt, tot, own


def _exact(oracle, dev, x, cell, marks, r_max, nbins, tric=False):
    cnt, tot, own = _user_sample(dev, marks, r_max, nbins)
    pairs, d2 = _pairs_d2(oracle, x, cell, r_max, tric)
    rc, rs, rself, ok = ref.correlate(pairs, d2, marks, np.ones(marks.shape[1]), 4.0, r_max, nbins)
    print("N %d NC %d pairs %d  cnt diff %d  sum diff %d  self %d / %d" % (
        len(x), marks.shape[1], rc.sum(), np.abs(cnt - rc).sum(), np.abs(tot - rs).max(), own, rself))
    assert ok and np.abs(rs).max() > 2 ** 27
    assert np.array_equal(cnt, rc) and np.array_equal(tot, rs) and own == rself
    return cnt


# ---------------------------------------------------------------------------------------------------------------------
# 1 - 4: exact integers, user marks

def test_exact_user_marks_3d(oracle):
    s = lj_system(4000)
    r_max, nbins = 3.0, 300
    with _handle(4000, 3, s["box"], 2.5, s["x"], pot=LJ) as dev:
        dev.upload(s["x"], s["v"], s["f"], s["img"], s["diam"])
        dev.run(40, 0.002)
        x = dev.download()[0]
        cnt = _exact(oracle, dev, x, s["box"], _dyadic(4000, 3, 101), r_max, nbins)
        dev.rdf_setup(r_max, nbins)                         # both samplers set up at once: buffers of their own
        dev.rdf_sample()
        dev.mpc_sample()
        counts, _ = dev.rdf_read()
        again = dev.mpc_last()[0]
    assert cnt.sum() > 20 * 4000
    assert np.array_equal(cnt, counts) and np.array_equal(again, cnt)


def test_exact_user_marks_2d(oracle):
    s = poly_system()
    with _handle(s["n"], 2, s["box"], 1.5, s["x"], diam=s["diam"], kind=2, pot=[1.25, 0.2]) as dev:
        dev.upload(s["x"], s["v"], s["f"], s["img"], s["diam"])
        dev.run(100, 0.001)
        x = dev.download()[0]
        cnt = _exact(oracle, dev, x, s["box"], _dyadic(s["n"], 2, 102), 5.0, 250)
    assert cnt.sum() > 20 * s["n"]


def test_exact_general_cell(oracle):
    """The sheared cell of tests/test_gpu_rdf.py::test_bit_exact_general_cell at the largest r_max the face rule allows:
    3 cells per direction, about 150 particles per cell -- the 64-wide home and neighbour chunk loops run more than once,
    with a ragged tail."""
    from moleculardynamics.jl_amd import MDDevice
    from moleculardynamics.jl_amd.initialization import initialize_velocities
    from tests.test_gpu_triclinic import _fill
    U, n = TRIC_U, 4000
    rng = np.random.default_rng(4242)
    x0 = _fill(U, n, rng)
    v = initialize_velocities(1.2, rng, n, 3)
    perp = 1.0 / np.linalg.norm(np.linalg.inv(U), axis=1)
    r_max = perp.min() / 3.0 * (1.0 - 1e-12)
    with MDDevice(3, n, U, 2.5) as dev:
        dev.set_potential(0, LJ)
        dev.upload(x0, v, np.zeros_like(x0), np.zeros((n, 3), np.int32), np.ones(n))
        dev.run(40, 0.002)
        x = dev.download()[0]
        cnt = _exact(oracle, dev, x, U, _dyadic(n, 1, 103), r_max, 500, tric=True)
        with pytest.raises(Exception, match="face distance"):
            dev.mpc_setup(perp.min() / 3.0 * (1.0 + 1e-12), 10, weights=[1.0], tmax=1.0)
    assert cnt.sum() > 20 * n


def test_exact_smallest_walk(oracle):
    """The smallest grid the walk allows: 3 x 3 x 3 cells of edge r_max, three particles in each."""
    from moleculardynamics.jl_amd import MDDevice
    rng = np.random.default_rng(81)
    cells = np.stack(np.meshgrid(*[np.arange(3)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    x = np.ascontiguousarray((np.repeat(cells, 3, axis=0) + rng.uniform(0.02, 0.98, (81, 3))) * 3.0)
    x = x[rng.permutation(81)]
    box = np.full(3, 9.0)
    with MDDevice(3, 81, box, 2.5) as dev:
        dev.upload(x=x)
        xd = dev.download()[0]
        cnt = _exact(oracle, dev, xd, box, _dyadic(81, 1, 104), 3.0, 64)
        many = _exact(oracle, dev, xd, box, _dyadic(81, 3, 105), 3.0, 4096)    # the bin limit: the largest LDS request
    assert cnt.sum() == many.sum() > 81


# ---------------------------------------------------------------------------------------------------------------------
# 5 - 7: the bond-order frame as marks

def _boo_check(oracle, dev, x, cell, dim, order, r_n, r_max, nbins, qlm, label, min_conn=7):
    """The device's last sample against the reference built from the frame x and the marks qlm (complex, by id)."""
    ns, acnt, asum, aself, tmax, err = dev.mpc_read()
    cnt, tot, own = dev.mpc_last()
    assert err == 0 and tmax == 1.0
    pairs, d2 = _pairs_d2(oracle, x, cell, r_max)
    w = ref.boo_weights(dim, order)
    rc, rs, rself, ok = ref.correlate(pairs, d2, ref.boo_marks(qlm), w, 1.0, r_max, nbins)
    occ = rc > 0
    sharp = np.median(np.abs(rs[occ]) / (2.0 * rc[occ]))
    print("%s: pairs %d  max |sum - ref| / cnt %.3f  median |ref| / tol %.3e  self diff %d" % (
        label, rc.sum(), (np.abs(tot - rs)[occ] / rc[occ]).max(), sharp, own - rself))
    assert ok and sharp > 1000.0
    assert np.array_equal(cnt, rc)
    assert np.all(np.abs(tot - rs) <= 2 * rc)
    assert abs(own - rself) <= 2 * len(x)
    return cnt, tot, rc, rs


def _boo_case(oracle, dev, cell, dim, order, r_n, r_max, nbins, label, min_conn=7):
    x = dev.download()[0]
    dev.boo_setup(r_n, order, 10, 0.7, min_conn, 0)
    dev.boo_sample()
    dev.mpc_setup(r_max, nbins)
    dev.mpc_sample()
    _boo_check(oracle, dev, x, cell, dim, order, r_n, r_max, nbins, dev.boo_qlm(), label + ", device marks")
    r = _reference(oracle, x, cell, r_n, order, 0.7, min_conn)
    assert np.abs(dev.boo_qlm() - r["qlm"]).max() <= 1e-12
    return _boo_check(oracle, dev, x, cell, dim, order, r_n, r_max, nbins, r["qlm"], label + ", reference marks")


@pytest.mark.parametrize("l", [6, 4])
def test_boo_source_jittered_fcc(oracle, l):
    x, box = boo.fcc(6, 1.6)
    x = x + np.random.default_rng(20240611).normal(0.0, 1e-2, x.shape)
    with _handle(len(x), 3, box, 1.5, x) as dev:
        cnt, tot, _, _ = _boo_case(oracle, dev, box, 3, l, 1.35, 3.0, 100, "jittered fcc l=%d" % l)
    occ = cnt > 0
    G = tot[occ] * Q / cnt[occ]
    assert np.all(G > 0.5 * boo_literature(l) ** 2) and np.all(G <= 1.0)      # a crystal: the order does not decay


def boo_literature(l):
    return {4: 0.19094, 6: 0.57452}[l]                     # q_l of fcc (tests/test_bond_order.py's table)


def test_boo_source_lj_liquid(oracle):
    s = lj_system(4000)
    with _handle(4000, 3, s["box"], 2.5, s["x"], pot=LJ) as dev:
        dev.upload(s["x"], s["v"], s["f"], s["img"], s["diam"])
        dev.run(100, 0.002)
        _boo_case(oracle, dev, s["box"], 3, 6, 1.5, 3.0, 150, "LJ liquid l=6")


def test_boo_source_2d(oracle):
    s = poly_system(1200)
    with _handle(s["n"], 2, s["box"], 1.5, s["x"], diam=s["diam"], kind=2, pot=[1.25, 0.2]) as dev:
        dev.upload(s["x"], s["v"], s["f"], s["img"], s["diam"])
        dev.run(60, 0.001)
        _boo_case(oracle, dev, s["box"], 2, 6, 1.4, 5.0, 250, "poly2d k=6", min_conn=4)


def test_perfect_hexagonal_lattice():
    x, box = boo.hexagonal(24, 14, 1.0)
    n = len(x)
    with _handle(n, 2, box, 1.5, x, kind=2, pot=[1.25, 0.2]) as dev:
        dev.boo_setup(1.3, 6, 10, 0.7, 6, 0)
        dev.boo_sample()
        dev.mpc_setup(5.0, 97)
        dev.mpc_sample()
        cnt, tot, own = dev.mpc_last()
        assert dev.mpc_read()[5] == 0
    occ = cnt > 0
    assert cnt.sum() > 30 * n and 10 < occ.sum() < 97
    assert np.all(np.abs(tot[occ] * Q / cnt[occ] - 1.0) <= 1e-9)
    assert not tot[~occ].any() and abs(own * Q / n - 1.0) <= 1e-9


def test_marks_follow_particles_not_slots(oracle):
    s = lj_system(4000)
    with _handle(4000, 3, s["box"], 2.5, s["x"], pot=LJ) as dev:
        dev.upload(s["x"], s["v"], s["f"], s["img"], s["diam"])
        dev.run(20, 0.002)
        dev.boo_setup(1.5, 6, 10, 0.7, 7, 0)
        dev.boo_sample()
        qlm = dev.boo_qlm()
        r0 = dev.stats()["rebuilds"]
        for _ in range(20):
            dev.run(60, 0.004)
            if dev.stats()["rebuilds"] > r0:
                break
        assert dev.stats()["rebuilds"] > r0                 # the list was rebuilt: the slots were re-sorted
        assert np.array_equal(dev.boo_qlm(), qlm)
        dev.mpc_setup(3.0, 150)
        dev.mpc_sample()
        x = dev.download()[0]
        _boo_check(oracle, dev, x, s["box"], 3, 6, 1.5, 3.0, 150, qlm, "old marks, new positions")
        # marks attached by slot instead would be a different answer: the bound tells them apart
        cnt, tot, _ = dev.mpc_last()
        pairs, d2 = _pairs_d2(oracle, x, s["box"], 3.0)
        shuffled = qlm[np.random.default_rng(3).permutation(4000)]
        _, rs, _, _ = ref.correlate(pairs, d2, ref.boo_marks(shuffled), ref.boo_weights(3, 6), 1.0, 3.0, 150)
        assert np.any(np.abs(tot - rs) > 2 * cnt)


# ---------------------------------------------------------------------------------------------------------------------
# 8 - 10: accumulators, side effects, the range error

def test_accumulators_and_reset():
    s = lj_system(4000)
    marks = _dyadic(4000, 1, 108) * 0.999                   # not dyadic any more: the terms themselves are rounded
    with _handle(4000, 3, s["box"], 2.5, s["x"], pot=LJ) as dev:
        dev.upload(s["x"], s["v"], s["f"], s["img"], s["diam"])
        dev.mpc_setup(3.0, 120, weights=[3.0], tmax=3.0)
        dev.mpc_marks(marks)
        acc_c, acc_s, acc_o = np.zeros(120, dtype=np.int64), np.zeros(120), 0.0
        lasts = []
        for m in range(3):
            dev.run(10, 0.002)
            dev.mpc_sample()
            cnt, tot, own = dev.mpc_last()
            lasts.append((cnt, tot, own))
            acc_c = acc_c + cnt
            acc_s = acc_s + tot.astype(np.float64)
            acc_o = acc_o + float(own)
            ns, acnt, asum, aself, tmax, err = dev.mpc_read()
            assert ns == m + 1 and err == 0 and tmax == 4.0
            assert np.array_equal(acnt, acc_c) and np.array_equal(asum, acc_s) and aself == acc_o
        assert not np.array_equal(lasts[0][1], lasts[1][1]) and np.abs(lasts[0][1]).max() > 2 ** 31
        dev.mpc_sample()                                    # the same frame again: the same integers
        again = dev.mpc_last()
        assert np.array_equal(again[0], lasts[2][0]) and np.array_equal(again[1], lasts[2][1]) and again[2] == lasts[2][2]
        dev.mpc_reset()
        ns, acnt, asum, aself, tmax, err = dev.mpc_read()
        assert ns == 0 and not acnt.any() and not asum.any() and aself == 0.0 and tmax == 4.0 and err == 0
        with pytest.raises(Exception, match="no sample yet"):
            dev.mpc_last()
        dev.mpc_sample()                                    # the setup and the marks were kept
        once = dev.mpc_last()
        assert np.array_equal(once[1], lasts[2][1]) and dev.mpc_read()[0] == 1


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
                dev.boo_setup(1.5, 6, 10, 0.7, 7, 0)
                dev.mpc_setup(3.0, 100)
                dev.boo_sample()
                dev.mpc_sample()
            res = []
            for _ in range(5):
                res.append(dev.run(10, 0.002))
                if sample:
                    dev.boo_sample()
                    dev.mpc_sample()
            if sample:
                assert dev.mpc_read()[0] == 6
            out.append((res, dev.download(), dev.stats()["fused"]))
    (ra, da, fa), (rb, db, fb) = out
    assert fa == fb and (fa == 0 or not switch)
    assert ra == rb
    for u, w in zip(da, db):
        assert np.array_equal(u, w)


def test_range_error_is_reported_and_the_handle_stays_usable(oracle):
    s = lj_system(4000)
    with _handle(4000, 3, s["box"], 2.5, s["x"], pot=LJ) as dev:
        x = dev.download()[0]
        dev.mpc_setup(3.0, 60, weights=[1.0], tmax=1.0)
        dev.mpc_marks(np.full(4000, 2.0))                   # t = 4 > tmax (1 + 2^-10)
        dev.mpc_sample()
        ns, acnt, asum, aself, tmax, err = dev.mpc_read()
        pairs, d2 = _pairs_d2(oracle, x, s["box"], 3.0)
        rc, _, _, ok = ref.correlate(pairs, d2, np.full(4000, 2.0), [1.0], 1.0, 3.0, 60)
        assert err == 1 and not ok and ns == 1
        assert np.array_equal(acnt, rc) and not asum.any() and aself == 0.0        # counted, never wrapped
        dev.mpc_sample()
        assert dev.mpc_read()[5] == 1                       # sticky
        dev.mpc_marks(np.full(4000, 1.0 + 2.0 ** -12))      # t = 1 + 2^-11 + 2^-24: within the margin
        dev.mpc_reset()
        dev.mpc_sample()
        ns, acnt, asum, aself, tmax, err = dev.mpc_read()
        assert err == 0 and ns == 1 and np.array_equal(acnt, rc)
        I = int(np.rint((1.0 + 2.0 ** -12) ** 2 * 2.0 ** 31))
        assert np.array_equal(asum, (rc * I).astype(np.float64)) and aself == 4000.0 * I
        dev.run(5, 0.002)                                   # the handle goes on


# ---------------------------------------------------------------------------------------------------------------------
# 11: refusals

def test_refusals():
    from moleculardynamics.jl_amd import MDDevice, MdhipError, _lib
    s = lj_system(1000)
    with MDDevice(3, 1000, s["box"], 2.5) as dev:
        dev.set_potential(0, LJ)
        dev.upload(s["x"], s["v"], s["f"], s["img"], s["diam"])
        for call in (dev.mpc_sample, dev.mpc_last, dev.mpc_read, dev.mpc_reset, lambda: dev.mpc_marks(np.zeros(1000))):
            with pytest.raises(MdhipError, match="no setup"):
                call()
        user = dict(weights=[1.0], tmax=1.0)
        L = s["box"][0]
        with pytest.raises(MdhipError, match=r"face distance .*3\*r_max"):
            dev.mpc_setup(L / 3.0 * 1.0001, 10, **user)
        for bad in (0, 4097, -1):
            with pytest.raises(MdhipError, match="nbins"):
                dev.mpc_setup(3.0, bad, **user)
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            with pytest.raises(MdhipError, match="r_max"):
                dev.mpc_setup(bad, 10, **user)
            with pytest.raises(MdhipError, match="tmax"):
                dev.mpc_setup(3.0, 10, weights=[1.0], tmax=bad)
        for bad in ([], [1.0] * 4):
            with pytest.raises(MdhipError, match="nc must be in 1..3"):
                dev.mpc_setup(3.0, 10, weights=bad, tmax=1.0)
        for bad in (float("inf"), float("nan")):
            with pytest.raises(MdhipError, match="weight"):
                dev.mpc_setup(3.0, 10, weights=[1.0, bad], tmax=1.0)
        with pytest.raises(MdhipError, match="md_boo_setup first"):
            dev.mpc_setup(3.0, 10)                          # the bond-order source before its sampler exists
        with pytest.raises(MdhipError, match="no setup"):   # a refused setup leaves no sampler behind
            dev.mpc_sample()
        dev.mpc_setup(3.0, 4096, weights=[1.0, -2.0, 0.5], tmax=1e-3)      # the limits themselves are accepted
        assert dev.mpc_read()[4] == 2.0 ** -9               # 1e-3 rounded up to a power of two
        with pytest.raises(MdhipError, match="md_mpc_marks first"):
            dev.mpc_sample()
        with pytest.raises(MdhipError, match="no sample yet"):
            dev.mpc_last()
        for bad in (float("inf"), float("nan")):
            m = np.zeros((1000, 3))
            m[999, 2] = bad
            with pytest.raises(MdhipError, match="mark must be finite"):
                dev.mpc_marks(m)
        with pytest.raises(ValueError):
            dev.mpc_marks(np.zeros((1000, 2)))              # the wrong number of components
        with pytest.raises(MdhipError, match="md_mpc_marks first"):       # a refused upload leaves no marks behind
            dev.mpc_sample()
        dev.boo_setup(1.5, 6)
        dev.mpc_setup(3.0, 10)
        with pytest.raises(MdhipError, match="md_boo_sample first"):
            dev.mpc_sample()
        with pytest.raises(MdhipError, match="bond-order frame"):
            dev.mpc_marks(np.zeros((1000, 14)))
        dev.boo_sample()
        dev.mpc_sample()
        dev.boo_setup(1.5, 4)                               # another order: the weights of the setup no longer fit
        dev.boo_sample()
        with pytest.raises(MdhipError, match="md_mpc_setup again"):
            dev.mpc_sample()
        assert dev.mpc_read()[0] == 1
    lib = _lib.load()
    h = ctypes.c_void_p()
    n = 4000
    box = (ctypes.c_double * 9)(20, 0, 0, 0, 20, 0, 0, 0, 20)
    assert lib.md_create_domain(3, n, n, box, 2.5, -1, 0, 1, ctypes.byref(h)) == 0, lib.md_last_error(None)
    try:
        w = (ctypes.c_double * 1)(1.0)
        assert lib.md_mpc_setup(h, 1, 2.0, 10, 1, w, 1.0) != 0
        assert b"slab" in lib.md_last_error(h)
        for fn in (lib.md_mpc_sample, lib.md_mpc_reset):
            assert fn(h) != 0
            assert b"slab" in lib.md_last_error(h)
    finally:
        lib.md_destroy(h)


# ---------------------------------------------------------------------------------------------------------------------
# 12: run_simulation and the one-shot functions

def test_run_simulation_and_the_one_shots(tmp_path):
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
    pa, pb, pc = str(tmp_path / "a"), str(tmp_path / "b"), str(tmp_path / "c")
    sa, sb, sc = fresh(pa), fresh(pb), fresh(pc)
    oc = md.OrientationalCorrelation(4.0, 100, every=2)
    md.run_simulation(sa, params, ensemble, 31, 10, pa, bond_order=md.BondOrder(1.5), orientational=oc)
    md.run_simulation(sb, params, ensemble, 31, 10, pb)
    assert oc.nsamples == 2 and oc.order == 6 and oc.tmax == 1.0
    assert files(pa) == files(pb)
    assert np.array_equal(np.asarray(sa.system.positions), np.asarray(sb.system.positions))
    lines = open(os.path.join(pa, "orient_corr.txt")).read().splitlines()
    assert lines[0] == "# l 6 r_neigh 1.500000 tmax 1 nsamples 2" and lines[1] == "# r_mid count g(r) G(r) g_l(r)"
    assert len(lines) == 103 and lines[-1].startswith("# <t_ii> ")
    assert sum(int(ln.split()[1]) for ln in lines[2:-1]) == oc.counts.sum() > 100 * n
    assert 0.0 < oc.mean_self() < 1.0
    assert not os.path.exists(os.path.join(pb, "orient_corr.txt"))
    with pytest.raises(ValueError, match="needs bond_order="):
        md.run_simulation(sb, params, ensemble, 1, 10, pb, orientational=md.OrientationalCorrelation(4.0, 100))
    # one step: the sample at step 0 is of the final state, and so is the one-shot's
    one = md.OrientationalCorrelation(4.0, 100)
    md.run_simulation(sc, params, ensemble, 1, 10, pc, bond_order=md.BondOrder(1.5), orientational=one)
    again = md.compute_orientational_correlation(sc, params, 1.5, 6, 4.0, 100)
    assert one.nsamples == again.nsamples == 1
    # the same pairs; the marks of a fresh list build agree with the run's to 1e-12 (tests/test_gpu_bond_order.py): the
    # header's bound
    assert np.array_equal(one.counts, again.counts) and np.all(np.abs(one.sums - again.sums) <= 2 * one.counts)
    assert abs(one.self_sum - again.self_sum) <= 2 * n and np.allclose(one.G(), again.G(), rtol=0, atol=1e-8, equal_nan=True)
    # the same marks uploaded by the caller: the general entry gives the same integers
    r = md.compute_bond_order(sc, params, 1.5)
    mk = md.compute_marked_correlation(sc, params, ref.boo_marks(r["qlm"])[:, :2], 4.0, 100,
                                       weights=ref.boo_weights(3, 6)[:2], tmax=1.0)
    assert np.array_equal(mk["count"], one.counts) and mk["tmax"] == 1.0
    vv = md.compute_marked_correlation(sc, params, np.asarray(sc.velocities), 4.0, 100)
    assert np.array_equal(vv["count"], one.counts) and vv["tmax"] >= 1.0
    occ = vv["count"] > 0
    assert np.all(np.abs(vv["C"][occ]) <= vv["tmax"]) and np.isnan(vv["C"][~occ]).all()
    assert abs(vv["self"] * vv["quantum"] / n - (np.asarray(sc.velocities) ** 2).sum() / n) <= 1e-6
    for st in (sa, sb, sc):
        st.system.device.close()
