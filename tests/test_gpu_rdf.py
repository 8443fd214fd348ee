"""-m gpu: g(r) sampled on the device (md_rdf_*, md_rdf.hpp).

A histogram of pair distances is integer-valued and independent of the order the pairs are visited in, so the device
counts are checked EXACTLY: against the oracle's pair set with d2 formed in the reference's arithmetic (canon_d2 /
tric_d2, restated in numpy) and binned on the same edge table, and against two answers that need no oracle -- the shell
counts of a lattice and the virial rebuilt from the histogram.  A sample must also leave everything else the handle
computes unchanged."""
import ctypes
import math
import os

import numpy as np
import pytest

from tests.util import lj_system, poly_system

pytestmark = pytest.mark.gpu
LJ = [1.0, 1.0, 2.5]


def _edges2(r_max, nbins):
    delta = r_max / nbins
    rk = np.arange(nbins + 1, dtype=np.float64) * delta
    return rk * rk


def _bin(d2, r_max, nbins):
    e2 = _edges2(r_max, nbins)
    d2 = d2[d2 < e2[-1]]
    k = np.searchsorted(e2, d2, "right") - 1
    return np.bincount(k, minlength=nbins).astype(np.int64)


def _canon_d2(x, box, pairs):
    """oracle/md_oracle.c canon_d2 for the (a < b) pairs: b translated, every operation rounded on its own."""
    a, b = x[pairs[:, 0]], x[pairs[:, 1]]
    L = np.asarray(box, dtype=np.float64)
    d0 = b - a
    half = 0.5 * L
    s = np.where(d0 > half, -1.0, np.where(d0 < -half, 1.0, 0.0))
    de = (b + s * L) - a
    d2 = de[:, 0] * de[:, 0] + de[:, 1] * de[:, 1]
    if x.shape[1] == 3:
        d2 = d2 + de[:, 2] * de[:, 2]
    return d2


def _tric_d2(x, U, pairs):
    """oracle/md_oracle.c tric_d2: 3^d translations t_r = (s0 U_r0 + s1 U_r1) + s2 U_r2, strict < in its loop order."""
    d = x.shape[1]
    a, b = x[pairs[:, 0]], x[pairs[:, 1]]
    best = np.full(len(pairs), 1e300)
    for s2 in ((-1, 0, 1) if d == 3 else (0,)):
        for s1 in (-1, 0, 1):
            for s0 in (-1, 0, 1):
                de = np.empty_like(a)
                for r in range(d):
                    t = float(s0) * U[r, 0] + float(s1) * U[r, 1]
                    if d == 3:
                        t = t + float(s2) * U[r, 2]
                    de[:, r] = (b[:, r] + t) - a[:, r]
                d2 = de[:, 0] * de[:, 0] + de[:, 1] * de[:, 1]
                if d == 3:
                    d2 = d2 + de[:, 2] * de[:, 2]
                best = np.where(d2 < best, d2, best)
    return best


def _device(s, cutoff=2.5, pot=LJ, kind=0):
    from moleculardynamics.jl_amd import MDDevice
    dev = MDDevice(s["dim"], s["n"], s["box"], cutoff)
    dev.set_potential(kind, pot)
    dev.upload(s["x"], s["v"], s["f"], s["img"], s["diam"])
    return dev


def _sample(dev, r_max, nbins):
    dev.rdf_setup(r_max, nbins)
    dev.rdf_sample()
    counts, ns = dev.rdf_read()
    assert ns == 1
    return counts


@pytest.mark.parametrize("n,r_max,nbins", [(32768, 3.5, 350), (262144, 3.0, 300)])
def test_bit_exact_against_the_oracle_orthorhombic(oracle, n, r_max, nbins):
    s = lj_system(n)
    with _device(s) as dev:
        dev.run(60, 0.002)
        x = dev.download()[0]
        counts = _sample(dev, r_max, nbins)
    pairs = oracle.pairs_cells(x, s["box"], r_max)
    ref = _bin(_canon_d2(x, s["box"], pairs), r_max, nbins)
    assert counts.sum() > 10 * n
    assert np.array_equal(counts, ref)
    assert counts.sum() == ref.sum()


def test_bit_exact_in_2d(oracle):
    s = poly_system()
    with _device(s, cutoff=1.5, pot=[1.25, 0.2], kind=2) as dev:
        dev.run(100, 0.001)
        x = dev.download()[0]
        counts = _sample(dev, 5.0, 250)
    pairs = oracle.pairs_cells(x, s["box"], 5.0)
    ref = _bin(_canon_d2(x, s["box"], pairs), 5.0, 250)
    assert counts.sum() > 20 * s["n"]
    assert np.array_equal(counts, ref)


def test_bit_exact_general_cell(oracle):
    from moleculardynamics.jl_amd import MDDevice
    from moleculardynamics.jl_amd.initialization import initialize_velocities
    from tests.test_gpu_triclinic import _fill
    U = np.array([[18.0, 4.5, 0.0], [0.0, 17.5, 0.0], [0.0, 0.0, 18.0]])
    n = 4000
    rng = np.random.default_rng(4242)
    x0 = _fill(U, n, rng)
    v = initialize_velocities(1.2, rng, n, 3)
    perp = 1.0 / np.linalg.norm(np.linalg.inv(U), axis=1)
    r_max = perp.min() / 3.0 * (1.0 - 1e-12)               # as large as the face rule allows
    nbins = 500
    with MDDevice(3, n, U, 2.5) as dev:
        dev.set_potential(0, LJ)
        dev.upload(x0, v, np.zeros_like(x0), np.zeros((n, 3), np.int32), np.ones(n))
        dev.run(40, 0.002)
        x = dev.download()[0]
        counts = _sample(dev, r_max, nbins)
        with pytest.raises(Exception, match="face distance"):
            dev.rdf_setup(perp.min() / 3.0 * (1.0 + 1e-12), 10)
    with oracle.set_cell(U):
        pot = oracle.make_pot(0, LJ)
        _, _, _, pairs = oracle.forces_brute(x, np.ones(3), r_max, pot, np.ones(n), want_pairs=True)
    ref = _bin(_tric_d2(x, U, pairs), r_max, nbins)
    assert counts.sum() > 20 * n
    assert np.array_equal(counts, ref)


def _lattice_check(dim, m, a, shells, per_n):
    from moleculardynamics.jl_amd import MDDevice
    n = m ** dim
    g = np.stack(np.meshgrid(*[np.arange(m)] * dim, indexing="ij"), -1).reshape(-1, dim)
    x = np.ascontiguousarray((g + 0.25) * a)
    r_max = 2.6 * a
    nbins = 245
    e = np.arange(nbins + 1) * (r_max / nbins)
    rs = np.sqrt(np.array(shells, dtype=float)) * a
    gap = np.abs(e[None, :] - rs[:, None]).min()
    assert gap > 1e-3 * a, gap                              # no edge near a shell radius
    with MDDevice(dim, n, np.full(dim, m * a), 2.5) as dev:
        dev.upload(x=x)
        counts = _sample(dev, r_max, nbins)
    k = np.searchsorted(e, rs, "right") - 1
    expect = np.zeros(nbins, np.int64)
    for kk, c in zip(k, per_n):
        expect[kk] += c * n
    assert np.array_equal(counts, expect)


def test_lattice_shells_exact():
    # simple cubic: 6, 12, 8, 6, 24, 24 neighbours at a, sqrt2 a, sqrt3 a, 2a, sqrt5 a, sqrt6 a (unordered: half)
    _lattice_check(3, 16, 1.1, [1, 2, 3, 4, 5, 6], [3, 6, 4, 3, 12, 12])
    # square: 4, 4, 4, 8 at a, sqrt2 a, 2a, sqrt5 a
    _lattice_check(2, 40, 1.05, [1, 2, 4, 5], [2, 2, 2, 4])


def test_virial_route():
    """sum_k counts_k h(r_k), h = r f(r) at the bin centre, against the device's own W of the same configurations."""
    import moleculardynamics.jl_amd as md
    s = lj_system(32768)
    r_max, nbins = 2.5, 5000
    wsum, nsamp = 0.0, 6
    with _device(s) as dev:
        dev.rdf_setup(r_max, nbins)
        for _ in range(nsamp):
            _, W, _ = dev.run(20, 0.002)
            dev.rdf_sample()
            wsum += W
        counts, ns = dev.rdf_read()
    assert ns == nsamp
    r = (np.arange(nbins) + 0.5) * (r_max / nbins)
    h = np.array([rr * md.evaluate(md.LennardJones(), float(rr), 1.0, 1.0)[1] for rr in r])
    west = float(np.dot(counts.astype(np.float64), h))
    assert abs(west - wsum) <= 3e-3 * abs(wsum), (west, wsum)


def test_no_side_effects():
    s = lj_system(32768)
    out = []
    for sample in (True, False):
        with _device(s) as dev:
            if sample:
                dev.rdf_setup(3.5, 200)
            r1 = dev.run(50, 0.002)
            if sample:
                dev.rdf_sample()
                dev.snapshot_begin()                # a frame in flight beside a sample
                dev.rdf_sample()
                dev.snapshot_end()
            r2 = dev.run(50, 0.002)
            out.append((r1, r2, dev.download(), dev.rdf_read() if sample else None))
    (a1, a2, da, ca), (b1, b2, db, _) = out
    assert a1 == b1 and a2 == b2
    for u, w in zip(da, db):
        assert np.array_equal(u, w)
    # two samples of one configuration: exactly twice one
    with _device(s) as dev:
        dev.run(50, 0.002)
        one = _sample(dev, 3.5, 200)
    assert ca[1] == 2 and np.array_equal(ca[0], 2 * one)


def test_ideal_gas_normalisation():
    from moleculardynamics.jl_amd import MDDevice, RadialDistribution
    n, rho, r_max, nbins = 200000, 0.897, 4.0, 100
    L = (n / rho) ** (1.0 / 3.0)
    x = np.random.default_rng(777).random((n, 3)) * L
    with MDDevice(3, n, np.full(3, L), 2.5) as dev:
        dev.upload(x=x)
        counts = _sample(dev, r_max, nbins)
    rdf = RadialDistribution(r_max, nbins)
    rdf._accumulate(counts, 1, n, np.diag([L, L, L]))
    V = L ** 3
    expect = n * (n - 1) / (2.0 * V) * rdf.shell_volumes()
    assert np.all(np.abs(counts - expect) <= 5.0 * np.sqrt(expect))
    assert abs(counts.sum() - expect.sum()) <= 5.0 * math.sqrt(expect.sum())
    g = rdf.g()
    assert abs(np.average(g, weights=expect) - 1.0) < 2e-3


def _files(path):
    return {f: open(os.path.join(path, f), "rb").read() for f in ("thermo.txt", "trajectory.xyz")}


@pytest.mark.parametrize("ens", ["nvt", "brownian"])
def test_run_simulation_integration(tmp_path, ens):
    import moleculardynamics.jl_amd as md
    n = 4096
    params = md.Parameters(0.8, n, 0.002 if ens == "nvt" else 1e-4, md.LennardJones())

    def fresh(path):
        st = md.initialize_state(params, path, random_init=True, cutoff=2.5, rng=np.random.default_rng(11))
        st.velocities = md.initialize_velocities(1.5, np.random.default_rng(12), n, 3)
        return st

    ensemble = md.NVT(1.5, 0.05) if ens == "nvt" else md.Brownian(1.5)
    pa, pb = str(tmp_path / "a"), str(tmp_path / "b")
    sa, sb = fresh(pa), fresh(pb)
    rdf = md.RadialDistribution(4.0, 200)
    md.run_simulation(sa, params, ensemble, 31, 10, pa, rdf=rdf)
    md.run_simulation(sb, params, ensemble, 31, 10, pb)
    assert rdf.nsamples == 4 and rdf.counts.sum() > 0
    assert _files(pa) == _files(pb)
    assert np.array_equal(np.asarray(sa.system.positions), np.asarray(sb.system.positions))
    lines = open(os.path.join(pa, "rdf.txt")).read().splitlines()
    assert lines[0] == "# r g(r) count" and len(lines) == 201
    assert not os.path.exists(os.path.join(pb, "rdf.txt"))
    # one step: the sample at step 0 is of the final state
    pc = str(tmp_path / "c")
    sc = fresh(pc)
    one = md.RadialDistribution(4.0, 200)
    md.run_simulation(sc, params, ensemble, 1, 10, pc, rdf=one)
    assert one.nsamples == 1
    again = md.compute_rdf(sc, params, 4.0, 200)
    assert again.nsamples == 1 and np.array_equal(again.counts, one.counts)
    for st in (sa, sb, sc):
        st.system.device.close()


def test_errors():
    from moleculardynamics.jl_amd import MDDevice, MdhipError, _lib
    with MDDevice(3, 1000, 12.0, 2.5) as dev:
        with pytest.raises(MdhipError, match="no setup"):
            dev.rdf_sample()
        with pytest.raises(MdhipError, match="no setup"):
            dev.rdf_read()
        with pytest.raises(MdhipError, match=r"face distance 12 .*3\*r_max.*limit r_max <= 4"):
            dev.rdf_setup(4.0001, 10)
        with pytest.raises(MdhipError, match="nbins"):
            dev.rdf_setup(3.0, 0)
        with pytest.raises(MdhipError, match="nbins"):
            dev.rdf_setup(3.0, 8193)
        with pytest.raises(MdhipError, match="r_max"):
            dev.rdf_setup(0.0, 10)
        dev.rdf_setup(4.0, 8192)                           # the limits themselves are accepted
        dev.rdf_setup(4.0, 1)
    lib = _lib.load()
    h = ctypes.c_void_p()
    n = 4000
    box = (ctypes.c_double * 9)(20, 0, 0, 0, 20, 0, 0, 0, 20)
    assert lib.md_create_domain(3, n, n, box, 2.5, -1, 0, 1, ctypes.byref(h)) == 0, lib.md_last_error(None)
    try:
        assert lib.md_rdf_setup(h, 2.0, 10) != 0
        assert b"slab" in lib.md_last_error(h)
        assert lib.md_rdf_sample(h) != 0
    finally:
        lib.md_destroy(h)
