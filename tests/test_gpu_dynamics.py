"""-m gpu: self dynamics sampled on the device (md_dyn_*, md_dyn.hpp).

The sums are checked against a numpy restatement of the contract from the two downloaded frames (the histogram exactly,
the fp64 sums to 1e-12), against each other across handles with different list histories (bit for bit: the frames alone
decide them), and against three answers that need no restatement: ballistic flight through a periodic cell (which pins the
unwrapping), free Brownian diffusion with the project's uniform noise, and the MSD of the log-time snapshot files that
run_simulation(log_times=True) writes.  Sampling must leave everything else the handle and run_simulation compute
unchanged."""
import ctypes
import glob
import math
import os

import numpy as np
import pytest

from tests.dyn_reference import bin_counts as _bin, restate as _restate
from tests.util import lj_system, poly_system

pytestmark = pytest.mark.gpu
LJ = [1.0, 1.0, 2.5]
Q4 = [1.0, 2.0 * math.pi, 7.0, 11.3]


def _device(s, cutoff=2.5, pot=LJ, kind=0):
    from moleculardynamics.jl_amd import MDDevice
    dev = MDDevice(s["dim"], s["n"], s["box"], cutoff)
    dev.set_potential(kind, pot)
    dev.upload(s["x"], s["v"], s["f"], s["img"], s["diam"])
    return dev


def _sheared(n=4000, seed=4242):
    from moleculardynamics.jl_amd.initialization import initialize_velocities
    from tests.test_gpu_triclinic import _fill
    U = np.array([[18.0, 4.5, 0.0], [0.0, 17.5, 0.0], [0.0, 0.0, 18.0]])
    rng = np.random.default_rng(seed)
    x = _fill(U, n, rng)
    v = initialize_velocities(1.2, rng, n, 3)
    return dict(n=n, dim=3, box=U, x=x, v=v, f=np.zeros_like(x), img=np.zeros((n, 3), np.int32), diam=np.ones(n))


def _cell(s):
    b = np.asarray(s["box"], dtype=np.float64)
    return b if b.ndim == 2 else np.diag(b)


CASES = {   # system, device keywords, steps, dt, r_max of the fine histogram (8192 bins)
    "orthorhombic": (lambda: lj_system(32768), dict(), 400, 0.005, 1.5),
    "poly2d": (poly_system, dict(cutoff=1.5, pot=[1.25, 0.2], kind=2), 1500, 0.001, 1.5),
    "sheared": (_sheared, dict(), 400, 0.004, 2.0),
}


def _origin_and_sample(case):
    """Store an origin, run until the list has been rebuilt, sample; returns the frames, the results and the handle."""
    make, kw, steps, dt, r_max = CASES[case]
    s = make()
    dev = _device(s, **kw)
    dev.run(20, dt)
    dev.dyn_setup(1, 2, Q4, r_max, 8192)            # (row 1 stays empty)
    x0, _, _, n0 = dev.download()
    r0 = dev.stats()["rebuilds"]
    dev.dyn_origin(0)
    dev.run(steps, dt)
    x1, _, _, n1 = dev.download()
    assert dev.stats()["rebuilds"] > r0             # the particles were reordered between the frames
    dev.dyn_sample([0], [0])
    cnt, sums, hist = dev.dyn_read()
    de, d2 = _restate(x0, n0, x1, n1, _cell(s))
    return s, dev, (x0, n0, x1, n1), (de, d2, r_max), (cnt, sums, hist)


@pytest.mark.parametrize("case", list(CASES))
def test_exact_against_a_numpy_restatement(case):
    s, dev, (x0, n0, x1, n1), (de, d2, r_max), (cnt, sums, hist) = _origin_and_sample(case)
    with dev:
        d = s["dim"]
        n = s["n"]
        assert np.any(n1 != n0)                     # some particles crossed a face: the image counts matter
        assert list(cnt) == [1, 0]
        assert np.array_equal(hist[0], _bin(d2, r_max, 8192))
        assert hist[0].sum() > 0.5 * n and not hist[1].any()
        ref2 = math.fsum(d2)
        ref4 = math.fsum(d2 * d2)
        assert abs(sums[0, 0] - ref2) <= 1e-12 * ref2
        assert abs(sums[0, 1] - ref4) <= 1e-12 * ref4
        for j, q in enumerate(Q4):
            sq = np.cos(q * de[:, 0])
            for c in range(1, d):
                sq = sq + np.cos(q * de[:, c])
            ref = math.fsum(sq) / (d * n)
            assert abs(sums[0, 2 + j] / (d * n) - ref) <= 1e-12, (q, sums[0, 2 + j] / (d * n), ref)
        assert not sums[1].any()


@pytest.mark.parametrize("case", ["orthorhombic", "sheared"])
def test_the_frames_alone_decide_the_bits(case):
    """Handle B is given A's two frames by upload, with another skin: another list history, the same sums bit for bit."""
    from moleculardynamics.jl_amd import MDDevice
    s, dev, (x0, n0, x1, n1), (de, d2, r_max), (cnt, sums, hist) = _origin_and_sample(case)
    dev.close()
    with MDDevice(s["dim"], s["n"], s["box"], 2.5) as b:
        b.set_potential(0, LJ)
        b.set_skin(0.45)
        b.upload(s["x"], s["v"], s["f"], s["img"], s["diam"])
        b.run(30, 0.002)                            # a history of its own
        b.dyn_setup(3, 2, Q4, r_max, 8192)
        b.upload(x0, None, None, n0)
        xb, _, _, nb = b.download()
        assert np.array_equal(xb, x0) and np.array_equal(nb, n0)
        b.dyn_origin(2)
        b.run(25, 0.002)
        b.upload(x1, None, None, n1)
        b.dyn_sample([2], [1])
        cb, sb, hb = b.dyn_read()
    assert list(cb) == [0, 1]
    assert sb[1].tobytes() == sums[0].tobytes()
    assert np.array_equal(hb[1], hist[0])


def _free_flight(U, n, speed, seed):
    rng = np.random.default_rng(seed)
    x = rng.random((n, 3)) @ U.T                    # uniform in the cell (no potential: overlaps are harmless)
    v = rng.normal(size=(n, 3))
    v *= speed / np.linalg.norm(v, axis=1)[:, None] * rng.uniform(0.5, 1.0, size=(n, 1))
    return x, v


@pytest.mark.parametrize("shear", [0.0, 4.5])
def test_ballistic_flight_pins_the_unwrapping(shear):
    """An identically zero potential: x(t) = x(0) + v t.  Particles cross the cell several times, so without the image
    counters the MSD would saturate at the cell size."""
    from moleculardynamics.jl_amd import MDDevice
    U = np.array([[16.0, shear, 0.0], [0.0, 15.5, 0.0], [0.0, 0.0, 16.5]])
    n, dt, speed = 4096, 0.01, 10.0
    x, v = _free_flight(U, n, speed, 99)
    lags = [1, 300, 1000]
    with MDDevice(3, n, U, 2.5) as dev:
        dev.set_potential(0, [0.0, 1.0, 2.5])
        dev.upload(x, v, np.zeros_like(x), np.zeros((n, 3), np.int32), np.ones(n))
        dev.dyn_setup(1, len(lags), Q4)
        dev.dyn_origin(0)
        done = 0
        for k, l in enumerate(lags):
            dev.run(l - done, dt)
            done = l
            dev.dyn_sample([0], [k])
        ns, sums, _ = dev.dyn_read()
        img = dev.download()[3]
    assert np.abs(img).max() >= 3                   # several crossings
    v2 = float(np.mean(np.sum(v * v, axis=1)))
    for k, l in enumerate(lags):
        t = l * dt
        assert ns[k] == 1
        msd = sums[k, 0] / n
        assert abs(msd - t * t * v2) <= 1e-9 * t * t * v2, (l, msd, t * t * v2)
        for j, q in enumerate(Q4):
            ref = float(np.mean(np.sum(np.cos(q * v * t), axis=1) / 3.0))
            assert abs(sums[k, 2 + j] / (3 * n) - ref) <= 1e-8, (l, q)


def test_brownian_free_diffusion_known_answer(tmp_path):
    """Zero potential, uniform noise of half-width a = sqrt(3) sqrt(2 dt) per axis and step: MSD = 2 d dt l,
    F_s = phi(q)^l with phi = sin(a q) / (a q), alpha2 = -1.2 / (l (d + 2)); each within 5 sigma."""
    import moleculardynamics.jl_amd as md
    n, d, dt = 1 << 18, 3, 1e-3
    params = md.Parameters(0.5, n, dt, md.LennardJones(epsilon=0.0))
    st = md.initialize_state(params, str(tmp_path), random_init=True, cutoff=2.5, rng=np.random.default_rng(5))
    q = [2.0 * math.pi, 4.0, 9.0]
    dyn = md.SelfDynamics(q=q)
    T = 800
    md.run_simulation(st, params, md.Brownian(1.0), T, 100000, str(tmp_path), dynamics=dyn, write_trajectory=False)
    st.system.device.close()
    reached = dyn.nsamples > 0
    assert np.array_equal(dyn.lags[reached], [l for l in dyn.lags if l < T])
    a = math.sqrt(3.0) * math.sqrt(2.0 * dt)
    msd, a2, fs = dyn.msd(), dyn.alpha2(), dyn.fs()
    for k in np.nonzero(reached)[0]:
        l = int(dyn.lags[k])
        s2 = 2.0 * dt * l                           # per-axis variance
        m = d * s2
        assert abs(msd[k] - m) <= 5.0 * math.sqrt(2.0 * d) * s2 / math.sqrt(n), (l, msd[k], m)
        # alpha2: delta-method sigma for a Gaussian displacement (d = 3: var = 0.533 / N)
        ea2 = -1.2 / (l * (d + 2))
        assert abs(a2[k] - ea2) <= 5.0 * math.sqrt(0.533 / n), (l, a2[k], ea2)
        for j, qq in enumerate(q):
            phi = math.sin(a * qq) / (a * qq)
            phi2 = math.sin(2 * a * qq) / (2 * a * qq)
            ef = phi ** l
            var = (0.5 * (1.0 + phi2 ** l) - ef * ef) / d
            assert abs(fs[k, j] - ef) <= 5.0 * math.sqrt(var / n) + 1e-12, (l, qq, fs[k, j], ef)
    assert os.path.isfile(os.path.join(str(tmp_path), "dynamics.txt"))


def test_no_side_effects():
    s = lj_system(32768)
    out = []
    for sample in (True, False):
        with _device(s) as dev:
            r1 = dev.run(50, 0.002)
            before = dev.download()
            if sample:
                dev.dyn_setup(2, 3, Q4, 2.0, 100)
                dev.dyn_origin(1)
                mid = dev.download()
                for u, w in zip(before, mid):
                    assert np.array_equal(u, w)
                dev.run(10, 0.002)
                dev.dyn_sample([1, 1], [0, 2])
                dev.snapshot_begin()                # a frame in flight beside a sample
                dev.dyn_sample([1], [1])
                dev.snapshot_end()
                d1 = dev.download()
            else:
                dev.run(10, 0.002)
                d1 = dev.download()
            r2 = dev.run(50, 0.002)
            out.append((r1, r2, d1, dev.download(), dev.dyn_read() if sample else None))
    (a1, a2, ad1, da, ya), (b1, b2, bd1, db, _) = out
    assert a1 == b1 and a2 == b2
    for u, w in zip(ad1 + da, bd1 + db):
        assert np.array_equal(u, w)
    ns, sums, hist = ya
    assert list(ns) == [1, 1, 1]
    assert sums[0].tobytes() == sums[1].tobytes() == sums[2].tobytes()
    assert np.array_equal(hist[0], hist[1]) and np.array_equal(hist[0], hist[2])


def _files(path, names):
    return {f: open(os.path.join(path, f), "rb").read() for f in names}


def _snapshot_msd(path, lag_steps):
    """MSD from the xu yu zu columns of snapshot.0 and snapshot.<lag> (the reference's analysis route), and the bound of
    its difference from the device's value: two %f roundings per coordinate (|e| <= 1e-6 on a displacement component
    moves its square by <= 2 |del| 1e-6 + 1e-12), and the %.6e of dynamics.txt."""
    def xu(step):
        with open(os.path.join(path, f"snapshot.{step}")) as f:
            lines = f.read().splitlines()
        n = int(lines[3])
        a = np.array([l.split() for l in lines[9:9 + n]], dtype=np.float64)
        return a[:, -3:]
    u0 = xu(0)
    out = {}
    for l in lag_steps:
        dd = xu(l) - u0
        msd = float(np.mean(np.sum(dd * dd, axis=1)))
        out[l] = (msd, 2e-6 * float(np.mean(np.sum(np.abs(dd), axis=1))) + 3e-12 + 1e-6 * msd)
    return out


@pytest.mark.parametrize("ens", ["nvt", "brownian"])
def test_run_simulation_integration(tmp_path, ens):
    import moleculardynamics.jl_amd as md
    n, T, freq = 4096, 31, 10
    params = md.Parameters(0.8, n, 0.002 if ens == "nvt" else 1e-4, md.LennardJones())

    def fresh(path):
        st = md.initialize_state(params, path, random_init=True, cutoff=2.5, rng=np.random.default_rng(11))
        st.velocities = md.initialize_velocities(1.5, np.random.default_rng(12), n, 3)
        return st

    ensemble = md.NVT(1.5, 0.05) if ens == "nvt" else md.Brownian(1.5)
    pa, pb, pc = str(tmp_path / "a"), str(tmp_path / "b"), str(tmp_path / "c")
    sa, sb, sc = fresh(pa), fresh(pb), fresh(pc)
    dyn = md.SelfDynamics(q=(2.0 * math.pi, 5.0), r_max=1.0, nbins=50)
    md.run_simulation(sa, params, ensemble, T, freq, pa, log_times=True, dynamics=dyn)
    md.run_simulation(sb, params, ensemble, T, freq, pb, log_times=True)
    md.run_simulation(sc, params, ensemble, T, freq, pc, dynamics=md.SelfDynamics())
    snaps = sorted(os.path.basename(p) for p in glob.glob(os.path.join(pb, "snapshot.*")))
    assert snaps == sorted(os.path.basename(p) for p in glob.glob(os.path.join(pa, "snapshot.*")))
    assert len(snaps) == 11
    names = ["thermo.txt", "trajectory.xyz", "final.xyz"] + snaps
    assert _files(pa, names) == _files(pb, names)
    for attr in ("positions",):
        assert np.array_equal(np.asarray(getattr(sa.system, attr)), np.asarray(getattr(sb.system, attr)))
    assert np.array_equal(sa.images, sb.images)
    # the same stops without log_times: the same segments, the same thermo and trajectory
    assert _files(pc, ["thermo.txt", "trajectory.xyz"]) == _files(pa, ["thermo.txt", "trajectory.xyz"])
    assert not glob.glob(os.path.join(pc, "snapshot.*")) and not os.path.exists(os.path.join(pc, "vanhove.txt"))
    # dynamics.txt: the lags below T, their MSD against the snapshots' %f columns
    lines = open(os.path.join(pa, "dynamics.txt")).read().splitlines()
    assert lines[0] == "# lag time msd alpha2 Fs(q=6.28319) Fs(q=5) nsamples"
    rows = [l.split() for l in lines[1:]]
    lags = [int(r[0]) for r in rows]
    assert lags == [1, 2, 3, 4, 6, 8, 11, 14, 20, 27]
    ref = _snapshot_msd(pa, lags)
    for r in rows:
        l = int(r[0])
        assert float(r[1]) == pytest.approx(l * params.dt, rel=1e-6)
        assert int(r[-1]) == 1
        msd, bound = ref[l]
        assert msd > 0.0 and abs(float(r[2]) - msd) <= bound, (l, r[2], msd, bound)
    vh = open(os.path.join(pa, "vanhove.txt")).read().split("\n\n")
    assert len(vh) == len(lags)
    # two calls: the samples accumulate
    md.run_simulation(sa, params, ensemble, T, freq, pa, dynamics=dyn)
    assert list(dyn.nsamples[:10]) == [2] * 10 and not dyn.nsamples[10:].any()
    for st in (sa, sb, sc):
        st.system.device.close()


def test_errors(monkeypatch):
    from moleculardynamics.jl_amd import MDDevice, MdhipError, _lib
    with MDDevice(3, 1000, 12.0, 2.5) as dev:
        dev.upload(x=np.random.default_rng(1).random((1000, 3)) * 12.0)
        for call in (lambda: dev.dyn_origin(0), lambda: dev.dyn_sample([0], [0]), dev.dyn_read, dev.dyn_reset):
            with pytest.raises(MdhipError, match="no setup"):
                call()
        with pytest.raises(MdhipError, match="nslots"):
            dev.dyn_setup(0, 1)
        with pytest.raises(MdhipError, match="nslots"):
            dev.dyn_setup(65, 1)
        with pytest.raises(MdhipError, match="nrows"):
            dev.dyn_setup(1, 0)
        with pytest.raises(MdhipError, match="nq"):
            dev.dyn_setup(1, 1, np.ones(17))
        with pytest.raises(MdhipError, match="finite"):
            dev.dyn_setup(1, 1, [1.0, float("nan")])
        with pytest.raises(MdhipError, match="nbins"):
            dev.dyn_setup(1, 1, [1.0], 1.0, 8193)
        with pytest.raises(MdhipError, match="nbins"):
            dev.dyn_setup(1, 1, [1.0], 1.0, -1)
        with pytest.raises(MdhipError, match="r_max"):
            dev.dyn_setup(1, 1, [1.0], 0.0, 10)
        with pytest.raises(MdhipError, match="r_max"):
            dev.dyn_setup(1, 1, [1.0], float("inf"), 10)
        monkeypatch.setenv("MDHIP_DYN_ALLOC_LIMIT", "1000")
        # (the switch is read at every setup)
        with pytest.raises(MdhipError, match=r"cannot allocate 72000 bytes for 2 origin slots"):
            dev.dyn_setup(2, 1, [1.0])
        monkeypatch.delenv("MDHIP_DYN_ALLOC_LIMIT")
        dev.dyn_setup(64, 3, np.ones(16), 2.0, 8192)           # the limits themselves are accepted
        dev.dyn_setup(2, 3, [], 0.0, 0)
        with pytest.raises(MdhipError, match="slot 2 is out of range"):
            dev.dyn_origin(2)
        with pytest.raises(MdhipError, match="slot -1 is out of range"):
            dev.dyn_origin(-1)
        with pytest.raises(MdhipError, match="empty"):
            dev.dyn_sample([1], [0])
        dev.dyn_origin(1)
        with pytest.raises(MdhipError, match="row 3 is out of range"):
            dev.dyn_sample([1], [3])
        with pytest.raises(MdhipError, match="slot 5 is out of range"):
            dev.dyn_sample([5], [0])
        dev.dyn_sample([1, 1], [0, 0])
        ns, sums, hist = dev.dyn_read()
        assert list(ns) == [2, 0, 0] and sums.shape == (3, 2) and hist.shape == (3, 0)
        assert np.all(sums == 0.0)                              # the frame against itself
        dev.dyn_reset()
        ns, sums, _ = dev.dyn_read()
        assert not ns.any()
        dev.dyn_sample([1], [2])                                # reset keeps the stored origins
        assert list(dev.dyn_read()[0]) == [0, 0, 1]
        dev.dyn_setup(2, 3)                                     # a new setup starts over: the origins are gone
        with pytest.raises(MdhipError, match="empty"):
            dev.dyn_sample([1], [0])
    lib = _lib.load()
    h = ctypes.c_void_p()
    n = 4000
    box = (ctypes.c_double * 9)(20, 0, 0, 0, 20, 0, 0, 0, 20)
    assert lib.md_create_domain(3, n, n, box, 2.5, -1, 0, 1, ctypes.byref(h)) == 0, lib.md_last_error(None)
    try:
        assert lib.md_dyn_setup(h, 1, 1, None, 0, 0.0, 0) != 0
        assert b"slab" in lib.md_last_error(h)
        assert lib.md_dyn_origin(h, 0) != 0
        assert b"slab" in lib.md_last_error(h)
        assert lib.md_dyn_sample(h, None, None, 0) != 0
        assert lib.md_dyn_read(h, None, None, None) != 0
        assert lib.md_dyn_reset(h) != 0
    finally:
        lib.md_destroy(h)


# ---------------------------------------------------------------------------------------------------------------------
# the split of a call's pairs into launches of MD_DYN_MAX_BATCH = 32

def _ragged_frames(dim, nframes=4):
    """(frames, box) of N = 257 -- one full 256-lane block and one lane: a simple lattice of spacing 1.1 with vacancies and
    a jitter of 0.04, then every further frame the one before it moved by a normal step of 0.08 per particle."""
    rng = np.random.default_rng(257 + dim)
    m = 7 if dim == 3 else 17
    sites = np.stack(np.meshgrid(*([np.arange(m)] * dim), indexing="ij"), -1).reshape(-1, dim).astype(np.float64)
    frames = [1.1 * (rng.permutation(sites)[:257] + 0.5) + rng.normal(0.0, 0.04, (257, dim))]
    for _ in range(nframes - 1):
        frames.append(frames[-1] + rng.normal(0.0, 0.08, (257, dim)))
    return frames, np.full(dim, 1.1 * m)


def _ragged_handle(dim, box, x):
    from moleculardynamics.jl_amd import MDDevice
    dev = MDDevice(dim, 257, box, 1.5)
    dev.set_potential(0, [1.0, 1.0, 1.5])
    dev.upload(x, np.zeros_like(x), np.zeros_like(x), np.zeros(x.shape, dtype=np.int32), np.ones(257))
    return dev


def _assert_identical(a, b):
    """Every array of two read-backs: the same dtype, the same shape, the same values (no tolerance)."""
    assert len(a) == len(b)
    for u, v in zip(a, b):
        u, v = np.asarray(u), np.asarray(v)
        assert u.dtype == v.dtype and u.shape == v.shape and np.array_equal(u, v)


@pytest.mark.parametrize("dim", [3, 2])
def test_one_call_with_more_pairs_than_a_batch_equals_one_call_per_pair(dim):
    """33 pairs, one more than a launch takes, on three origins and five rows (so rows receive entries of both launches):
    handle A samples them in one call, handle B in 33 calls of one pair, in order.  k_dyn_reduce adds a batch's entries
    to their rows in call order and the histogram counts are integers, so every read-back is equal bit for bit."""
    frames, box = _ragged_frames(dim)
    zi = np.zeros((257, dim), dtype=np.int32)
    slots, rows = [i % 3 for i in range(33)], [(2 * i) % 5 for i in range(33)]
    out = []
    for one_call in (True, False):
        with _ragged_handle(dim, box, frames[0]) as dev:
            dev.dyn_setup(3, 5, Q4, 1.0, 64)
            for s in range(3):
                dev.upload(frames[s], None, None, zi)
                dev.dyn_origin(s)
            dev.upload(frames[3], None, None, zi)
            if one_call:
                dev.dyn_sample(slots, rows)
            else:
                for a, b in zip(slots, rows):
                    dev.dyn_sample([a], [b])
            out.append(dev.dyn_read())
    _assert_identical(out[0], out[1])
    cnt, sums, hist = out[0]
    assert list(cnt) == list(np.bincount(rows, minlength=5)) and np.all(sums[:, 0] > 0.0)
    assert np.array_equal(hist.sum(axis=1), 257 * cnt)         # (no displacement reaches r_max = 1)
