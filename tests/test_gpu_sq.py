"""-m gpu: density modes, S(q) and coherent F(q, t) sampled on the device (md_sq_*, md_sq.hpp).

rho(q) cannot be bit-exact against a host libm, so it is bounded: per vector and component
|rho - rho_true| <= N (32 kappa |n|_1 + 128) 2^-53, kappa = || |U^-1| |U| ||_inf, rho_true evaluated in extended precision
from the downloaded frame (DESIGN.md section 12 derives the bound).  Given the rho values, the accumulators are exact
no-fma expressions of them and are compared bit for bit; the frame alone decides the bits of rho on any handle.  Known
answers that need no restatement: a simple cubic lattice (Bragg peaks), an ideal gas (S = 1), a uniformly translating
lattice (F(q, t) = N cos(q.v t) at the Bragg vectors).  Sampling must leave everything else the handle and run_simulation
compute unchanged."""
import ctypes
import glob
import math
import os

import numpy as np
import pytest

from tests.sq_reference import LD, PI_LD, bound as _bound, inv_ld as _inv_ld, rho_true as _rho_true  # noqa: F401
from tests.util import lj_system

pytestmark = pytest.mark.gpu
LJ = [1.0, 1.0, 2.5]
SHEARED = np.array([[18.0, 4.5, 1.0], [0.0, 17.5, -2.0], [0.0, 0.0, 18.0]])


def _cell(box):
    b = np.asarray(box, dtype=np.float64)
    return b if b.ndim == 2 else np.diag(b)


def _points(U, n, seed):
    rng = np.random.default_rng(seed)
    return rng.random((n, U.shape[0])) @ U.T


def _handle(U, x, cutoff=2.5, pot=(0.0, 1.0, 2.5), v=None):
    from moleculardynamics.jl_amd import MDDevice
    n, d = x.shape
    dev = MDDevice(d, n, U, cutoff)
    dev.set_potential(0, list(pot))
    dev.upload(x, np.zeros_like(x) if v is None else v, np.zeros_like(x), np.zeros((n, d), np.int32), np.ones(n))
    return dev


CELLS = {
    "orthorhombic": np.diag([15.0, 17.0, 19.0]),
    "sheared": SHEARED,
    "2d": np.array([[70.0, 0.0], [0.0, 60.0]]),
    "2d-sheared": np.array([[70.0, 11.0], [0.0, 60.0]]),
}


@pytest.mark.parametrize("cell", list(CELLS))
def test_rho_within_the_bound_of_extended_precision(cell):
    from moleculardynamics.jl_amd import select_wave_vectors
    U = CELLS[cell]
    N = 4096
    x = _points(U, N, 2024)
    n, q, _ = select_wave_vectors(U, 12.0)
    assert n.shape[0] >= 249 and np.sum(np.abs(n), axis=1).max() >= 30
    with _handle(U, x) as dev:
        dev.sq_setup(n)
        dev.sq_sample()
        rho = dev.sq_rho()
        frame = dev.download()[0]
    re, im = _rho_true(frame, U, n)
    bound = _bound(N, U, n)
    ere, eim = np.abs(rho.real - re), np.abs(rho.imag - im)
    print(f"{cell}: nvec {n.shape[0]}, max |n|_1 {np.sum(np.abs(n), axis=1).max()}, worst error / bound "
          f"{max((ere / bound).max(), (eim / bound).max()):.3e}, bound {bound.min():.2e}..{bound.max():.2e}")
    assert np.all(ere <= bound) and np.all(eim <= bound)        # every vector, both components
    assert np.abs(rho).max() > 10.0                              # (not all zeros)


def test_the_accumulators_are_exact_in_rho():
    s = lj_system(32768)
    from moleculardynamics.jl_amd import MDDevice, select_wave_vectors
    n, _, _ = select_wave_vectors(_cell(s["box"]), 9.0, max_per_bin=3, seed=5)
    nvec = n.shape[0]
    with MDDevice(3, s["n"], s["box"], 2.5) as dev:
        dev.set_potential(0, LJ)
        dev.upload(s["x"], s["v"], s["f"], s["img"], s["diam"])
        dev.sq_setup(n, 3, 4)
        s2, corr, ns, nst = np.zeros(nvec), np.zeros((4, nvec)), np.zeros(4, np.int64), 0
        org = {}
        # (static, [(slot, row)], origin): statics, correlations against several slots, two samples on one row in one
        # call, a slot read and overwritten in the same call (the samples come first)
        plan = [(True, [], 0), (False, [(0, 0)], 1), (True, [(0, 1), (1, 0)], None), (True, [(1, 2), (1, 2), (0, 3)], 1),
                (False, [(1, 0), (0, 0)], 2), (True, [(2, 3)], None)]
        for static, smp, origin in plan:
            dev.run(15, 0.004)
            dev.sq_sample(static, [a for a, _ in smp], [b for _, b in smp], origin)
            rho = dev.sq_rho()
            re, im = rho.real.copy(), rho.imag.copy()
            if static:
                s2 = s2 + (re * re + im * im)
                nst += 1
            for slot, row in smp:
                o = org[slot]
                corr[row] = corr[row] + (re * o.real + im * o.imag)
                ns[row] += 1
            if origin is not None:
                org[origin] = rho.copy()
        got_nst, got_s2, got_ns, got_corr = dev.sq_read()
        assert got_nst == nst and list(got_ns) == list(ns)
        assert got_s2.tobytes() == s2.tobytes()
        assert got_corr.tobytes() == corr.tobytes()
        assert np.all(s2 > 0.0) and np.all(np.any(corr != 0.0, axis=1))
        # reset zeroes the accumulators and the counts and keeps the origins
        dev.sq_reset()
        z_nst, z_s2, z_ns, z_corr = dev.sq_read()
        assert z_nst == 0 and not z_ns.any() and not z_s2.any() and not z_corr.any()
        dev.sq_sample(False, [2], [1])
        rho = dev.sq_rho()
        _, _, r_ns, r_corr = dev.sq_read()
        assert list(r_ns) == [0, 1, 0, 0]
        assert r_corr[1].tobytes() == (0.0 + (rho.real * org[2].real + rho.imag * org[2].imag)).tobytes()


def _sheared_lj(n=4000, seed=4242):
    from moleculardynamics.jl_amd.initialization import initialize_velocities
    from tests.test_gpu_triclinic import _fill
    U = np.array([[18.0, 4.5, 0.0], [0.0, 17.5, 0.0], [0.0, 0.0, 18.0]])
    rng = np.random.default_rng(seed)
    x = _fill(U, n, rng)
    v = initialize_velocities(1.2, rng, n, 3)
    return dict(n=n, dim=3, box=U, x=x, v=v, f=np.zeros_like(x), img=np.zeros((n, 3), np.int32), diam=np.ones(n))


@pytest.mark.parametrize("case", ["orthorhombic", "sheared"])
def test_the_frame_alone_decides_the_bits(case):
    from moleculardynamics.jl_amd import MDDevice, select_wave_vectors
    s = lj_system(32768) if case == "orthorhombic" else _sheared_lj()
    U = _cell(s["box"])
    n, _, _ = select_wave_vectors(U, 10.0, max_per_bin=4)
    with MDDevice(3, s["n"], s["box"], 2.5) as a:
        a.set_potential(0, LJ)
        a.upload(s["x"], s["v"], s["f"], s["img"], s["diam"])
        r0 = a.stats()["rebuilds"]
        a.run(400, 0.004)
        assert a.stats()["rebuilds"] > r0           # the particles were reordered since the upload
        a.sq_setup(n)
        a.sq_sample()
        rho_a = a.sq_rho()
        x1, _, _, n1 = a.download()
    with MDDevice(3, s["n"], s["box"], 2.5) as b:
        b.set_potential(0, LJ)
        b.set_skin(0.45)
        b.upload(s["x"], s["v"], s["f"], s["img"], s["diam"])
        b.run(30, 0.002)                            # a history of its own
        b.sq_setup(n, 1, 1)
        b.sq_sample(True, [], [], 0)
        assert b.sq_rho().tobytes() != rho_a.tobytes()
        b.upload(x1, None, None, n1)
        xb = b.download()[0]
        assert np.array_equal(xb, x1)
        b.sq_sample()
        rho_b = b.sq_rho()
    assert rho_b.tobytes() == rho_a.tobytes()
    re, im = _rho_true(x1, U, n)
    bound = _bound(s["n"], U, n)
    assert np.all(np.abs(rho_a.real - re) <= bound) and np.all(np.abs(rho_a.imag - im) <= bound)


def _lattice16(U=None):
    """Simple cubic 16^3 at fractional coordinates (i + 1/4) / 16 (exact); x = U f."""
    i = np.arange(16, dtype=np.float64)
    f = np.array(np.meshgrid(i, i, i, indexing="ij")).reshape(3, -1).T
    f = (f + 0.25) / 16.0
    if U is None:
        return f * 16.0
    return f @ U.T


BRAGG = np.array([[16, 0, 0], [0, 16, 0], [0, 0, 16], [16, 16, 0], [16, -16, 16], [32, 16, 0], [0, -16, 48], [-16, 0, 32],
                  [48, 48, 48]], dtype=np.int32)


def test_lattice_known_answer():
    from moleculardynamics.jl_amd import select_wave_vectors
    U = np.eye(3) * 16.0
    x = _lattice16()
    N = 4096
    sel, _, _ = select_wave_vectors(U, 14.0)
    n = np.concatenate([BRAGG, sel, np.array([[16, 1, 0], [15, 0, 0], [16, 16, 8], [1, 1, 1]], np.int32)])
    with _handle(U, x) as dev:
        dev.sq_setup(n)
        dev.sq_sample()
        rho = dev.sq_rho()
        nst, s2, _, _ = dev.sq_read()
    is_bragg = np.all(n % 16 == 0, axis=1)
    assert is_bragg.sum() >= len(BRAGG) and (~is_bragg).sum() > 200
    # N exp(2 pi i (n_0 + n_1 + n_2) / 64) at a Bragg vector -- the sum is a multiple of 16, the phase of pi / 2 -- else 0
    expect = np.zeros(n.shape[0], dtype=np.complex128)
    expect[is_bragg] = N * np.array([[1, 1j, -1, -1j][int(k) % 4] for k in np.sum(n[is_bragg], axis=1) // 16])
    bound = _bound(N, U, n)
    assert np.all(np.abs(rho.real - expect.real) <= bound) and np.all(np.abs(rho.imag - expect.imag) <= bound)
    assert nst == 1
    assert np.all(np.abs(s2[is_bragg] / N - N) <= 4.0 * bound[is_bragg])        # S at a Bragg vector = N


def test_ideal_gas():
    from moleculardynamics.jl_amd import select_wave_vectors
    N = 200000
    L = (N / 0.5) ** (1.0 / 3.0)
    U = np.eye(3) * L
    x = _points(U, N, 31337)
    n, _, _ = select_wave_vectors(U, 3.0)
    M = n.shape[0]
    assert M >= 512
    with _handle(U, x) as dev:
        dev.sq_setup(n)
        dev.sq_sample()
        _, s2, _, _ = dev.sq_read()
    sq = s2 / N
    print(f"ideal gas: M = {M}, mean S = {sq.mean():.5f}, 5 / sqrt(M) = {5.0 / math.sqrt(M):.5f}")
    assert abs(sq.mean() - 1.0) <= 5.0 / math.sqrt(M)
    assert sq.min() >= 0.0 and sq.max() < 20.0


@pytest.mark.parametrize("shear", [0.0, 4.5])
def test_uniform_translation_pins_f(shear):
    """Zero potential, one velocity for all: rho(q, t) = rho(q, 0) exp(i q.v t), so at a Bragg vector
    Re rho(t0 + t) rho*(t0) = N^2 cos(q.v t) and |rho|^2 stays N^2.  The particles cross the cell a dozen times."""
    U = np.array([[16.0, shear, 0.0], [0.0, 16.0, 0.0], [0.0, 0.0, 16.0]])
    x = _lattice16(U)
    N, dt = 4096, 0.01
    vel = np.array([7.31, -5.17, 3.73])
    v = np.tile(vel, (N, 1))
    n = BRAGG
    qv = 2.0 * math.pi * (n.astype(np.float64) @ np.linalg.inv(U)) @ vel         # q_n . v
    # (step, [(slot, row)], origin): two origins, so a mixed-up slot shows as a wrong lag
    plan = [(0, [], 0), (1, [(0, 0)], None), (300, [(0, 1)], 1), (1000, [(0, 2), (1, 3)], None), (2000, [(0, 4), (1, 5)], None)]
    lag = [1, 300, 1000, 700, 2000, 1700]
    with _handle(U, x, v=v) as dev:
        dev.sq_setup(n, 2, len(lag))
        done = 0
        for step, smp, origin in plan:
            if step > done:
                dev.run(step - done, dt)
            done = step
            dev.sq_sample(True, [a for a, _ in smp], [b for _, b in smp], origin)
            rho = dev.sq_rho()
            assert np.all(np.abs(np.abs(rho) ** 2 - N * N) <= 1e-8 * N * N), step
        nst, s2, ns, corr = dev.sq_read()
        img = dev.download()[3]
    assert np.abs(img).max() >= 3                   # several crossings
    assert nst == len(plan) and list(ns) == [1] * len(lag)
    assert np.all(np.abs(s2 - nst * float(N * N)) <= nst * 1e-8 * N * N)
    distinct = 0
    for k, l in enumerate(lag):
        expect = N * N * np.cos(qv * l * dt)
        err = np.abs(corr[k] - expect).max()
        print(f"shear {shear}: lag {l}, worst |corr - N^2 cos| / N^2 = {err / (N * N):.3e}")
        assert err <= 1e-8 * N * N, (l, err / (N * N))
        distinct += int(np.abs(np.cos(qv * l * dt)).min() < 0.9)
    assert distinct >= 4                            # the expected values are not trivially +-1


def test_no_side_effects():
    from moleculardynamics.jl_amd import MDDevice, select_wave_vectors
    s = lj_system(32768)
    n, _, _ = select_wave_vectors(_cell(s["box"]), 8.0, max_per_bin=4)
    out = []
    for sample in (True, False):
        with MDDevice(3, s["n"], s["box"], 2.5) as dev:
            dev.set_potential(0, LJ)
            dev.upload(s["x"], s["v"], s["f"], s["img"], s["diam"])
            dev.rdf_setup(2.5, 100)
            dev.dyn_setup(1, 2, [2.0 * math.pi], 2.0, 50)
            r1 = dev.run(50, 0.002)
            before = dev.download()
            dev.dyn_origin(0)
            if sample:
                dev.sq_setup(n, 2, 3)
                dev.sq_sample(True, [], [], 1)
                mid = dev.download()
                for u, w in zip(before, mid):
                    assert np.array_equal(u, w)
            dev.run(10, 0.002)
            dev.rdf_sample()
            if sample:
                dev.sq_sample(True, [1, 1], [0, 2], 0)
                dev.snapshot_begin()                # a frame in flight beside a sample
                dev.sq_sample(False, [0], [1])
                dev.snapshot_end()
            dev.dyn_sample([0], [0])
            d1 = dev.download()
            f1 = dev.compute_forces()
            r2 = dev.run(50, 0.002)
            dev.rdf_sample()
            dev.dyn_sample([0], [1])
            st = dev.stats()
            out.append((r1, r2, f1, d1, dev.download(), dev.rdf_read(), dev.dyn_read(), (st["rebuilds"], st["prunes"]),
                        dev.sq_read() if sample else None))
    (a1, a2, af, ad1, da, ar, ay, ast, sq), (b1, b2, bf, bd1, db, br, by, bst, _) = out
    assert a1 == b1 and a2 == b2 and af == bf and ast == bst
    for u, w in zip(ad1 + da, bd1 + db):
        assert np.array_equal(u, w)                 # trajectory, velocities, forces, images
    assert np.array_equal(ar[0], br[0]) and ar[1] == br[1] == 2
    assert np.array_equal(ay[0], by[0]) and ay[1].tobytes() == by[1].tobytes() and np.array_equal(ay[2], by[2])
    nst, s2, ns, corr = sq
    assert nst == 2 and list(ns) == [1, 1, 1]
    assert corr[0].tobytes() == corr[2].tobytes()   # the same frame against the same origin
    assert np.all(corr[1] > 0.0) and np.all(corr[1] < s2)      # row 1: the second frame against itself, |rho|^2


def _files(path, names):
    return {f: open(os.path.join(path, f), "rb").read() for f in names}


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
    paths = [str(tmp_path / k) for k in "abcd"]
    pa, pb, pc, pd = paths
    sa, sb, sc, sd = (fresh(p) for p in paths)
    static = md.StructureFactor(12.0, max_per_bin=8, every=2)
    dynamic = md.StructureFactor(12.0, max_per_bin=8, dynamic=True)
    md.run_simulation(sa, params, ensemble, T, freq, pa)
    md.run_simulation(sb, params, ensemble, T, freq, pb, sq=static)
    md.run_simulation(sc, params, ensemble, T, freq, pc, log_times=True)
    md.run_simulation(sd, params, ensemble, T, freq, pd, sq=dynamic)
    names = ["thermo.txt", "trajectory.xyz", "final.xyz"]
    assert _files(pa, names) == _files(pb, names)               # a static-only sampler cuts no extra segment
    assert np.array_equal(np.asarray(sa.system.positions), np.asarray(sb.system.positions))
    assert np.array_equal(sa.images, sb.images)
    assert not os.path.exists(os.path.join(pb, "fqt.txt")) and not os.path.exists(os.path.join(pa, "sq.txt"))
    # the default dynamic schedule stops where log_times=True stops: the same segments, thermo and trajectory
    assert _files(pc, ["thermo.txt", "trajectory.xyz"]) == _files(pd, ["thermo.txt", "trajectory.xyz"])
    assert not glob.glob(os.path.join(pd, "snapshot.*"))
    # sq.txt: steps 0 and 20 of 0, 10, 20, 30 (every = 2)
    assert static.nstatic == 2 and static.n_particles == n
    lines = open(os.path.join(pb, "sq.txt")).read().splitlines()
    assert lines[0] == "# q S(q) nvectors nsamples" and len(lines) == 1 + static.q.size
    S = static.s()
    for b, line in enumerate(lines[1:]):
        assert line == "%.6f %.6e %d %d" % (static.q[b], S[b], static.nvectors[b], 2)
    assert np.all(S > 0.0)
    # the dynamic sampler: a static sample at every output step, the log-time lags below T once each
    assert dynamic.nstatic == 4
    reached = [1, 2, 3, 4, 6, 8, 11, 14, 20, 27]
    assert list(dynamic.lags[dynamic.nsamples > 0]) == reached and set(dynamic.nsamples) == {0, 1}
    text = open(os.path.join(pd, "fqt.txt")).read()
    head = "# lag time q F F/S nsamples\n"
    assert text.startswith(head)
    blocks = text[len(head):].split("\n\n")
    assert len(blocks) == len(reached)
    F, Fn = dynamic.f(), dynamic.f_normalised()
    for blk, l in zip(blocks, reached):
        k = int(np.nonzero(dynamic.lags == l)[0][0])
        rows = blk.strip("\n").split("\n")
        assert len(rows) == dynamic.q.size
        for b, row in enumerate(rows):
            assert row == "%d %.6e %.6f %.6e %.6e %d" % (l, l * params.dt, dynamic.q[b], F[k, b], Fn[k, b], 1)
    # two calls: the samples accumulate
    md.run_simulation(sd, params, ensemble, T, freq, pd, sq=dynamic)
    assert dynamic.nstatic == 8 and list(dynamic.nsamples[:10]) == [2] * 10 and not dynamic.nsamples[10:].any()
    # compute_sq: one static sample of a state
    one = md.compute_sq(sa, params, 12.0, max_per_bin=8)
    assert one.nstatic == 1 and np.array_equal(one.n, static.n) and np.all(one.s() > 0.0)
    for st in (sa, sb, sc, sd):
        st.system.device.close()


def test_errors():
    from moleculardynamics.jl_amd import MDDevice, MdhipError, _lib
    ok = np.array([[1, 0, 0], [0, -2, 5]], np.int32)
    with MDDevice(3, 1000, 12.0, 2.5) as dev:
        dev.upload(x=np.random.default_rng(1).random((1000, 3)) * 12.0)
        for call in (lambda: dev.sq_sample(), dev.sq_rho, dev.sq_read, dev.sq_reset):
            with pytest.raises(MdhipError, match="no setup"):
                call()
        with pytest.raises(MdhipError, match="nvec"):
            dev.sq_setup(np.zeros((0, 3), np.int32))
        with pytest.raises(MdhipError, match="nvec"):
            dev.sq_setup(np.ones((16385, 3), np.int32))
        with pytest.raises(MdhipError, match="vector 1 is n = 0"):
            dev.sq_setup(np.array([[1, 0, 0], [0, 0, 0]], np.int32))
        with pytest.raises(MdhipError, match="component 2 of vector 0 is 32768"):
            dev.sq_setup(np.array([[1, 0, 32768]], np.int32))
        with pytest.raises(MdhipError, match="component 0 of vector 1 is -32768"):
            dev.sq_setup(np.array([[1, 0, 0], [-32768, 0, 0]], np.int32))
        with pytest.raises(MdhipError, match="nslots"):
            dev.sq_setup(ok, 65, 1)
        with pytest.raises(MdhipError, match="nslots"):
            dev.sq_setup(ok, -1, 1)
        with pytest.raises(MdhipError, match="nrows"):
            dev.sq_setup(ok, 1, -1)
        with pytest.raises(ValueError, match="shape"):
            dev.sq_setup(np.ones((4, 2), np.int32))
        with pytest.raises(MdhipError, match="no setup"):      # a refused setup leaves no sampler behind
            dev.sq_read()
        dev.sq_setup(np.array([[32767, -32767, 32767]], np.int32), 64, 5)   # the limits themselves are accepted
        dev.sq_setup(np.ones((16384, 3), np.int32), 0, 0)
        dev.sq_setup(ok, 2, 3)
        with pytest.raises(MdhipError, match="no frame"):
            dev.sq_rho()
        with pytest.raises(MdhipError, match="origin slot 2 is out of range"):
            dev.sq_sample(True, [], [], 2)
        with pytest.raises(MdhipError, match="origin slot -2 is out of range"):
            dev.sq_sample(True, [], [], -2)
        with pytest.raises(MdhipError, match="empty"):
            dev.sq_sample(True, [1], [0])
        with pytest.raises(ValueError, match="same length"):
            dev.sq_sample(True, [1], [0, 1])
        dev.sq_sample(False, [], [], 1)
        with pytest.raises(MdhipError, match="empty"):          # (the samples come before the origin)
            dev.sq_sample(True, [0], [0], 0)
        with pytest.raises(MdhipError, match="row 3 is out of range"):
            dev.sq_sample(True, [1], [3])
        with pytest.raises(MdhipError, match="row -1 is out of range"):
            dev.sq_sample(True, [1], [-1])
        with pytest.raises(MdhipError, match="slot 5 is out of range"):
            dev.sq_sample(True, [5], [0])
        nst, s2, ns, corr = dev.sq_read()                       # a refused call has counted nothing
        assert nst == 0 and not ns.any() and not s2.any() and corr.shape == (3, 2)
        dev.sq_sample(True, [1, 1], [0, 0])
        rho = dev.sq_rho()
        nst, s2, ns, corr = dev.sq_read()
        assert nst == 1 and list(ns) == [2, 0, 0]
        a2 = rho.real * rho.real + rho.imag * rho.imag
        assert s2.tobytes() == (0.0 + a2).tobytes() and corr[0].tobytes() == ((0.0 + a2) + a2).tobytes()
        dev.sq_setup(ok, 2, 3)                                  # a new setup starts over: the origins are gone
        with pytest.raises(MdhipError, match="empty"):
            dev.sq_sample(True, [1], [0])
        # more correlations in one call than one launch takes
        dev.sq_sample(False, [], [], 0)
        dev.sq_sample(False, [0] * 150, [k % 3 for k in range(150)])
        rho = dev.sq_rho()
        a2 = rho.real * rho.real + rho.imag * rho.imag
        acc = np.zeros(2)
        for _ in range(50):
            acc = acc + a2
        _, _, ns, corr = dev.sq_read()
        assert list(ns) == [50, 50, 50]
        for r in range(3):
            assert corr[r].tobytes() == acc.tobytes()
    lib = _lib.load()
    h = ctypes.c_void_p()
    n = 4000
    box = (ctypes.c_double * 9)(20, 0, 0, 0, 20, 0, 0, 0, 20)
    assert lib.md_create_domain(3, n, n, box, 2.5, -1, 0, 1, ctypes.byref(h)) == 0, lib.md_last_error(None)
    try:
        vec = (ctypes.c_int32 * 3)(1, 0, 0)
        assert lib.md_sq_setup(h, vec, 1, 0, 0) != 0
        assert b"slab" in lib.md_last_error(h)
        assert lib.md_sq_sample(h, 1, None, None, 0, -1) != 0
        assert b"slab" in lib.md_last_error(h)
        assert lib.md_sq_rho(h, None) != 0
        assert lib.md_sq_read(h, None, None, None, None) != 0
        assert lib.md_sq_reset(h) != 0
    finally:
        lib.md_destroy(h)


# ---------------------------------------------------------------------------------------------------------------------
# the split of a call's pairs into launches of MD_SQ_MAX_BATCH = 64

def _ragged_vectors(dim):
    """19 integer wave vectors with components in -2..2, none of them zero: two tiles of 8 and a ragged third."""
    g = np.arange(-2, 3)
    n = np.stack(np.meshgrid(*([g] * dim), indexing="ij"), -1).reshape(-1, dim)
    return np.ascontiguousarray(n[np.any(n != 0, axis=1)][::(5 if dim == 3 else 1)][:19], dtype=np.int32)


@pytest.mark.parametrize("dim", [3, 2])
def test_one_call_with_more_pairs_than_a_batch_equals_one_call_per_pair(dim):
    """65 pairs, one more than a launch takes, on three origins and five rows, at N = 257: handle A samples them in one
    call together with the static sample and a new origin; handle B in 65 calls of one pair, in order, the static sample
    with the first and the origin with the last.  k_sq_reduce adds a batch's entries to their rows in call order, so
    every read-back, rho and the stored origin (read through one more correlation) are equal bit for bit."""
    from tests.test_gpu_dynamics import _assert_identical, _ragged_frames, _ragged_handle
    frames, box = _ragged_frames(dim)
    zi = np.zeros((257, dim), dtype=np.int32)
    slots, rows = [i % 3 for i in range(65)], [(2 * i) % 5 for i in range(65)]
    out = []
    for one_call in (True, False):
        with _ragged_handle(dim, box, frames[0]) as dev:
            dev.sq_setup(_ragged_vectors(dim), 4, 6)
            for s in range(3):
                dev.upload(frames[s], None, None, zi)
                dev.sq_sample(False, origin=s)
            dev.upload(frames[3], None, None, zi)
            if one_call:
                dev.sq_sample(True, slots, rows, origin=3)
            else:
                for i, (a, b) in enumerate(zip(slots, rows)):
                    dev.sq_sample(i == 0, [a], [b], origin=3 if i == 64 else None)
            res = list(dev.sq_read()) + [dev.sq_rho()]
            dev.sq_sample(False, [3], [5])                      # row 5: this frame against the origin stored last
            out.append(res + list(dev.sq_read()))
    _assert_identical(out[0], out[1])
    nst, s2, cnt, corr, rho = out[0][:5]
    assert nst == 1 and list(cnt) == list(np.bincount(rows, minlength=6)) and np.all(s2 > 0.0) and np.all(corr[:5] != 0.0)
    assert np.all(np.abs(rho) > 0.0) and np.all(out[0][8][5] > 0.0)
