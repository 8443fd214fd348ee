"""-m gpu: the self overlap Q, chi4 and S4(q, t) sampled on the device (md_chi4_*, md_chi4.hpp).

Q, the mask of slow particles and the integer rows are functions of the two frames alone and are compared exactly with
tests/chi4_reference.py.  W cannot be bit-exact against a host libm, so it is bounded as rho is (DESIGN.md sections 12 and
18): |W - W_true| <= N (32 kappa |n|_1 + 128) 2^-53 per component, W_true in extended precision over the same slow set of
the same origin frame; given W, s4 is a no-fma expression of it and is compared bit for bit.  Known answers that need no
restatement: displacements on the threshold itself, a lattice whose odd layers translate, free Brownian diffusion (Q is
binomial, |W|^2 / N exponential with mean p).  Sampling must leave everything else unchanged."""
import ctypes
import glob
import math
import os

import numpy as np
import pytest

from tests.chi4_reference import _bound, overlap, w_true
from tests.test_gpu_sq import BRAGG, CELLS, _cell, _handle, _lattice16
from tests.util import lj_system

pytestmark = pytest.mark.gpu
LJ = [1.0, 1.0, 2.5]


def _frame(dev):
    x, _, _, img = dev.download()
    return x, img


def _put(dev, frame):
    dev.upload(frame[0], None, None, frame[1])
    assert np.array_equal(dev.download()[0], frame[0])


# ---------------------------------------------------------------------------------------------------------------------
# 1: the threshold and the image counts, exact

def _threshold_case(dim):
    """(x0, x1, n1, slow): one particle per row of `moves` and axis; L = 16, a = 0.375 (a*a = 0.140625 exact)."""
    below = np.nextafter(0.375, 0.0)
    face = 0.25 - 2.0 ** -49          # (0.25 - 2^-49) - 15.875 is exact: the largest face displacement below 0.375
    # (x0, x1, image, slow) along one axis, the other axes unmoved
    moves = [(0.0, 0.0, 0, 1),                  # unmoved
             (0.0, 0.375, 0, 0),                # exactly a: not slow (strict)
             (0.0, below, 0, 1),                # one ulp below a
             (0.375, 0.0, 0, 0),                # -a
             (below, 0.0, 0, 1),
             (15.875, 0.25, 1, 0),              # a across the face: (0.25 - 15.875) + 16 = 0.375
             (15.875, face, 1, 1),
             (0.25, 15.875, -1, 0),             # -a across the face
             (face, 15.875, -1, 1),
             (3.0, 3.0, 1, 0),                  # the wrapped position returns exactly, one cell further: d = 16
             (3.0, 3.0, -1, 0),
             (15.875, 0.25, 0, 0)]              # the same wrapped pair without the image: d = -15.625
    x0, x1, n1, slow = [], [], [], []
    for axis in range(dim):
        for a0, a1, im, s in moves:
            k = len(x0)
            p = np.full(dim, 1.0 + 0.34375 * k)      # the other axes: distinct, exact, unmoved
            q, m = p.copy(), np.zeros(dim, np.int32)
            p[axis], q[axis], m[axis] = a0, a1, im
            x0.append(p), x1.append(q), n1.append(m), slow.append(s)
    # off-axis: d2 = 2 * 0.0625 (slow), and in 3-D 0.0625 + 0.0625 + 0.015625 = 0.140625 = a*a exactly (not slow)
    extra = [((0.25, 0.25, 0.0), 1), ((0.25, 0.25, 0.125), 0 if dim == 3 else 1), ((0.375, 2.0 ** -20, 0.0), 0)]
    for de, s in extra:
        k = len(x0)
        p = np.full(dim, 1.0 + 0.34375 * k)
        x0.append(p), x1.append(p + np.array(de[:dim])), n1.append(np.zeros(dim, np.int32)), slow.append(s)
    assert len(x0) <= 40 and 1.0 + 0.34375 * len(x0) + 0.5 < 16.0
    return np.array(x0), np.array(x1), np.array(n1, dtype=np.int32), np.array(slow, dtype=np.uint8)


@pytest.mark.parametrize("dim", [3, 2])
def test_threshold_and_images_exact(dim):
    from moleculardynamics.jl_amd import MDDevice
    x0, x1, n1, want = _threshold_case(dim)
    n = len(x0)
    with MDDevice(dim, n, np.full(dim, 16.0), 2.5) as dev:
        dev.set_potential(0, [0.0, 1.0, 2.5])
        dev.upload(x0, np.zeros_like(x0), np.zeros_like(x0), np.zeros((n, dim), np.int32), np.ones(n))
        assert np.array_equal(dev.download()[0], x0)
        dev.chi4_setup(0.375, None, 1, 1)
        dev.chi4_origin(0)
        dev.upload(x1, None, None, n1)
        f1 = _frame(dev)
        assert np.array_equal(f1[0], x1) and np.array_equal(f1[1], n1)
        dev.chi4_sample([0], [0])
        q, w, slow = dev.chi4_last()
        ns, sq, sq2, s4 = dev.chi4_read()
    print(f"{dim}-D: slow {slow.tolist()}")
    assert slow.tolist() == want.tolist()
    assert q == int(want.sum()) and w.shape == (0,) and s4.shape == (1, 0)
    assert list(ns) == [1] and list(sq) == [q] and list(sq2) == [q * q]
    ref, qref = overlap(x0, np.zeros_like(n1), x1, n1, np.full(dim, 16.0), 0.375)     # (the restatement agrees too)
    assert ref.tolist() == want.tolist() and qref == q


# ---------------------------------------------------------------------------------------------------------------------
# 2, 3: against the reference on ragged shapes; the frames alone decide the bits

N_RAGGED = 4197                     # two mode blocks of 4096 ids, the last wave of the second one partial (4197 = 65 * 64 + 37)
NVEC_RAGGED = 13                    # two tiles of 8 vectors, the second one padded


def _liquid(U, seed=99):
    """N_RAGGED particles on a jittered lattice commensurate with the cell U, Maxwell velocities."""
    from moleculardynamics.jl_amd.initialization import initialize_velocities
    d = U.shape[0]
    rng = np.random.default_rng(seed)
    s = (abs(np.linalg.det(U)) / N_RAGGED) ** (1.0 / d)
    while True:
        m = np.maximum(1, np.floor(np.linalg.norm(U, axis=0) / s).astype(int))
        if np.prod(m) >= N_RAGGED:
            break
        s *= 0.995
    g = np.stack(np.meshgrid(*[np.arange(k) for k in m], indexing="ij"), -1).reshape(-1, d)
    g = g[rng.permutation(len(g))[:N_RAGGED]].astype(float)
    x = ((g + 0.5) / m) @ U.T + rng.uniform(-0.02, 0.02, (N_RAGGED, d))
    v = initialize_velocities(1.0, rng, N_RAGGED, d)
    return dict(n=N_RAGGED, dim=d, box=U, x=x, v=v, f=np.zeros_like(x), img=np.zeros((N_RAGGED, d), np.int32),
                diam=np.ones(N_RAGGED))


def _device(s, skin=None):
    from moleculardynamics.jl_amd import MDDevice
    dev = MDDevice(s["dim"], s["n"], s["box"], 2.5)
    dev.set_potential(0, LJ)
    if skin is not None:
        dev.set_skin(skin)
    dev.upload(s["x"], s["v"], s["f"], s["img"], s["diam"])
    return dev


def _vectors(U):
    from moleculardynamics.jl_amd import select_wave_vectors
    n, _, _ = select_wave_vectors(U, 6.0, max_per_bin=2, seed=3)
    assert n.shape[0] >= NVEC_RAGGED
    pick = np.linspace(0, n.shape[0] - 1, NVEC_RAGGED).astype(int)
    return np.ascontiguousarray(n[pick])


_ragged = {}


def _ragged_run(cell):
    """One run per cell, shared: origins at step 0 (slot 0) and T (slot 1), the sampled frame at 2 T, a rebuild in
    between; every (slot) sampled on its own into row 2, then -- after a reset -- three samples in one call."""
    if cell in _ragged:
        return _ragged[cell]
    U = CELLS[cell]
    s = _liquid(U)
    dt, chunk = (0.004 if U.shape[0] == 3 else 0.002), 50
    # a first pass finds T (a rebuild has happened by then) and a: the median displacement over 2 T, so Q / N ~ 1/2
    with _device(s) as dev:
        f0 = _frame(dev)
        dev.run(chunk, dt)
        r0, T = dev.stats()["rebuilds"], chunk
        while dev.stats()["rebuilds"] == r0:
            dev.run(chunk, dt)
            T += chunk
            assert T <= 4000
        dev.run(T, dt)
        f2 = _frame(dev)
    from tests.chi4_reference import displacement
    a = float(np.sqrt(np.median(displacement(f0[0], f0[1], f2[0], f2[1], U)[1])))
    n = _vectors(U)
    out = dict(U=U, a=a, n=n, s=s, T=T, dt=dt)
    with _device(s) as dev:
        dev.chi4_setup(a, n, 2, 3)
        dev.chi4_origin(0)
        out["f0"] = _frame(dev)
        dev.run(chunk, dt)
        r0 = dev.stats()["rebuilds"]
        dev.run(T - chunk, dt)
        dev.chi4_origin(1)
        out["f1"] = _frame(dev)
        dev.run(T, dt)
        out["f2"] = _frame(dev)
        assert dev.stats()["rebuilds"] > r0             # the particles were reordered since the origins were stored
        single = []
        for slot in (0, 1):
            dev.chi4_sample([slot], [2])
            single.append(dev.chi4_last())
        out["single"] = single
        out["read_single"] = dev.chi4_read()
        dev.chi4_reset()
        out["read_reset"] = dev.chi4_read()
        dev.chi4_sample([0, 1, 0], [0, 0, 1])           # two share row 0, two use different slots
        out["last"] = dev.chi4_last()
        out["read"] = dev.chi4_read()
    _ragged[cell] = out
    return out


@pytest.mark.parametrize("cell", list(CELLS))
def test_against_the_reference_on_ragged_shapes(cell):
    r = _ragged_run(cell)
    U, n, N = r["U"], r["n"], N_RAGGED
    bound = _bound(N, U, n)
    refs = []
    for slot, org in enumerate((r["f0"], r["f1"])):
        q, w, slow = r["single"][slot]
        ref_slow, ref_q = overlap(org[0], org[1], r["f2"][0], r["f2"][1], U, r["a"])
        wt = w_true(org[0], U, n, ref_slow)
        ere, eim = np.abs(w.real - wt.real), np.abs(w.imag - wt.imag)
        print(f"{cell} slot {slot}: a {r['a']:.4f}, T {r['T']}, Q/N {ref_q / N:.4f}, mismatched ids "
              f"{np.flatnonzero(slow != ref_slow)[:8].tolist()}, worst W error / bound "
              f"{max((ere / bound).max(), (eim / bound).max()):.3e}")
        assert np.array_equal(slow, ref_slow) and q == ref_q
        assert np.all(ere <= bound) and np.all(eim <= bound)
        assert np.abs(w).max() > 1.0
        refs.append((q, w))
    (q0, w0), (q1, w1) = refs
    assert 0.2 < q0 / N < 0.8 and 0 < q1 < N and q1 != q0
    # the rows: integers exact, s4 the no-fma expression of the returned W, in call order
    a0 = w0.real * w0.real + w0.imag * w0.imag
    a1 = w1.real * w1.real + w1.imag * w1.imag
    ns, sq, sq2, s4 = r["read_single"]
    assert list(ns) == [0, 0, 2] and list(sq) == [0, 0, q0 + q1] and list(sq2) == [0, 0, q0 * q0 + q1 * q1]
    assert s4[2].tobytes() == ((0.0 + a0) + a1).tobytes() and not s4[:2].any()
    ns, sq, sq2, s4 = r["read_reset"]
    assert not ns.any() and not sq.any() and not sq2.any() and not s4.any()
    ns, sq, sq2, s4 = r["read"]
    assert list(ns) == [2, 1, 0] and list(sq) == [q0 + q1, q0, 0] and list(sq2) == [q0 * q0 + q1 * q1, q0 * q0, 0]
    assert s4[0].tobytes() == ((0.0 + a0) + a1).tobytes() and s4[1].tobytes() == (0.0 + a0).tobytes() and not s4[2].any()
    ql, wl, sl = r["last"]
    assert ql == q0 and wl.tobytes() == w0.tobytes() and np.array_equal(sl, r["single"][0][2])


@pytest.mark.parametrize("cell", ["orthorhombic", "2d-sheared"])
def test_the_frames_alone_decide_the_bits(cell):
    r = _ragged_run(cell)
    with _device(r["s"], skin=0.45) as b:
        b.run(30, 0.002)                                # a history of its own
        b.chi4_setup(r["a"], r["n"], 2, 2)
        _put(b, r["f1"])
        b.chi4_origin(1)
        _put(b, r["f0"])
        b.chi4_origin(0)
        _put(b, r["f2"])
        b.chi4_sample([0, 1, 0], [0, 0, 1])
        ql, wl, sl = b.chi4_last()
        ns, sq, sq2, s4 = b.chi4_read()
        b.chi4_sample([1], [1])
        q1, w1, s1 = b.chi4_last()
    ans, asq, asq2, as4 = r["read"]
    assert list(ns) == list(ans[:2]) and list(sq) == list(asq[:2]) and list(sq2) == list(asq2[:2])
    assert s4.tobytes() == as4[:2].tobytes()
    assert ql == r["last"][0] and wl.tobytes() == r["last"][1].tobytes() and np.array_equal(sl, r["last"][2])
    assert q1 == r["single"][1][0] and w1.tobytes() == r["single"][1][1].tobytes()
    assert np.array_equal(s1, r["single"][1][2])


# ---------------------------------------------------------------------------------------------------------------------
# 4: a known answer with no restatement

def test_translating_layers_known_answer():
    """Simple cubic 16^3 at (i + 1/4), zero potential, NVE: the odd z layers move with v = (4, 0, 0), dt = 2^-6 (0.0625 per
    step, every position exact); a = 0.375.  Lag 4: 0.25 < a, Q = N.  Lag 8: 0.5 > a, Q = N / 2.  Lag 256: 16 = one cell
    length (three origins, at steps 0, 2 and 3), the wrapped frame is the origin's and only the image counts differ, Q = N / 2.  The slow set of the last two is
    the even layers: W = S(n_0) S(n_1) E(n_2), S(n) = e^(2 pi i n / 64) 16 [16 | n], E(n) = e^(2 pi i n / 64) 8 [8 | n]."""
    from moleculardynamics.jl_amd import FourPoint, select_wave_vectors
    U = np.eye(3) * 16.0
    x = _lattice16()
    N, dt = 4096, 2.0 ** -6
    odd = (np.rint(x[:, 2] - 0.25).astype(int) % 2) == 1
    assert odd.sum() == N // 2
    v = np.zeros_like(x)
    v[odd, 0] = 4.0
    sel, _, _ = select_wave_vectors(U, 10.0, max_per_bin=4)
    half = np.array([[0, 0, 8], [16, 0, 24], [0, 16, -8], [16, 16, 40], [1, 0, 8], [0, 0, 4]], np.int32)
    n = np.concatenate([BRAGG, half, sel])
    assert np.sum(~np.all(n % 8 == 0, axis=1)) >= 100
    bound = _bound(N, U, n)
    ph = np.exp(2j * np.pi * n.astype(np.float64) / 64.0)
    full = 16.0 * (n % 16 == 0)
    w_all = np.prod(ph * full, axis=1)                                          # every particle slow
    w_even = np.prod((ph * full)[:, :2], axis=1) * ph[:, 2] * 8.0 * (n[:, 2] % 8 == 0)
    assert np.count_nonzero(w_even) >= len(BRAGG) + 4

    def close(w, want):
        return np.all(np.abs(w.real - want.real) <= bound) and np.all(np.abs(w.imag - want.imag) <= bound)

    # (step, origin to store | None, [(slot, row)])
    plan = [(0, 0, []), (2, 1, []), (3, 2, []), (4, None, [(0, 0)]), (6, None, [(1, 0)]), (7, None, [(2, 0)]),
            (8, None, [(0, 1)]), (10, None, [(1, 1)]), (11, None, [(2, 1)]), (256, None, [(0, 2)]), (258, None, [(1, 2)]),
            (259, None, [(2, 2)])]
    fp = FourPoint(0.375, lags=[4, 8, 256], origin_every=4)         # (used as the accumulator only)
    with _handle(U, x, v=v) as dev:
        dev.chi4_setup(0.375, n, 3, 3)
        done = 0
        for step, origin, smp in plan:
            if step > done:
                dev.run(step - done, dt)
            done = step
            if step == 256:                             # one cell length: the wrapped frame is the origin's, bit for bit
                xw, img = _frame(dev)
                assert np.array_equal(xw, x) and np.array_equal(img[odd, 0], np.ones(N // 2, np.int32))
            for slot, row in smp:
                dev.chi4_sample([slot], [row])
                q, w, slow = dev.chi4_last()
                if row == 0:
                    assert q == N and slow.all()
                    if slot == 0:
                        assert close(w, w_all), step
                else:
                    assert q == N // 2 and np.array_equal(slow.astype(bool), ~odd), step
                    assert close(w, w_even), step
            if origin is not None:
                dev.chi4_origin(origin)
        xw, img = _frame(dev)
        ns, sq, sq2, s4 = dev.chi4_read()
    assert np.array_equal(img[odd, 0], np.ones(N // 2, np.int32)) and not img[~odd].any()
    assert list(ns) == [3, 3, 3] and list(sq) == [3 * N, 3 * N // 2, 3 * N // 2]       # three origins per lag
    fp._accumulate(ns, sq, sq2, np.zeros((3, 0)), N, dt)
    assert fp.chi4().tolist() == [0.0, 0.0, 0.0] and fp.overlap().tolist() == [1.0, 0.5, 0.5]


# ---------------------------------------------------------------------------------------------------------------------
# 5: free Brownian diffusion through run_simulation

def test_free_brownian_diffusion(tmp_path):
    """Independent particles: Q is binomial(N, p), chi4 = p (1 - p); the positions stay uniform, so |W|^2 / N is exponential
    with mean p at every q.  p is the measured <Q> / N, itself pinned integer for integer by the van Hove counts below
    the bin edge a.  Tolerances: a variance over ns samples has the relative error sqrt(2 / (ns - 1)); a mean of M ns
    exponentials has 1 / sqrt(M ns); five of each.  Both need independent SAMPLES, not only independent weights:
    W = sum (w_i - p) e^(iq.x_i) + p rho(q), and rho(q) of free diffusion persists for 1 / (D q^2), D = 1.  So the time
    between origins, E dt = 30, is three relaxation times of the smallest vector (q^2 = 0.097): the zero potential allows
    any time step (dt = 3, every step a list rebuild), the lag is one step and a = 1.53 sigma of its displacement."""
    import moleculardynamics.jl_amd as md
    n, dt, lag, every, ns = 4096, 3.0, 1, 10, 400
    r_max, nbins, k = 17.0, 50, 11
    params = md.Parameters(0.5, n, dt, md.LennardJones(epsilon=0.0))
    st = md.initialize_state(params, str(tmp_path), random_init=True, cutoff=2.5, rng=np.random.default_rng(5))
    # the ideal gas in equilibrium: independent uniform positions (initialize_state starts from a lattice, whose S(q) < 1
    # at small q survives the run: <|W|^2> / N = p (1 - p) + p^2 S(q) for independent weights)
    x = np.random.default_rng(6).random((n, 3)) * np.diagonal(np.asarray(st.unitcell))
    st.system.positions = st.system.xpositions = np.ascontiguousarray(x)
    dyn = md.SelfDynamics(r_max=r_max, nbins=nbins, lags=[lag], origin_every=every)
    fp = md.FourPoint(k * (r_max / nbins), q_max=2.2, max_per_bin=16, lags=[lag], origin_every=every)
    md.run_simulation(st, params, md.Brownian(1.0), 0, 1000000, str(tmp_path), write_trajectory=False)
    assert np.array_equal(st.system.device.download()[0], x)   # a run of no steps: the device holds the uniform positions
    md.run_simulation(st, params, md.Brownian(1.0), (ns - 1) * every + lag + 1, 1000000, str(tmp_path), dynamics=dyn, four_point=fp,
                      write_trajectory=False)
    st.system.device.close()
    assert list(fp.nsamples) == [ns] and list(dyn.nsamples) == [ns]
    assert int(fp.sum_q[0]) == int(dyn.hist[0, :k].sum())                       # integer for integer
    p = fp.overlap()[0]
    assert 0.3 < p < 0.8
    assert math.exp(-float(fp.qvec.min()) ** 2 * every * dt) < 0.06            # rho(q) of one origin is gone at the next
    chi4 = fp.chi4()[0]
    tol = 5.0 * math.sqrt(2.0 / (ns - 1))
    M = fp.n.shape[0]
    s4v, s4 = fp.s4_vectors()[0], fp.s4()[0]
    print(f"brownian: p {p:.5f}, chi4 / (p (1 - p)) - 1 = {chi4 / (p * (1 - p)) - 1:+.4f} (tolerance {tol:.4f}); "
          f"M {M}, <S4> / p - 1 = {s4v.mean() / p - 1:+.5f} (tolerance {5 / math.sqrt(M * ns):.5f}); per bin "
          f"{np.abs(s4 / p - 1).max():.5f}")
    assert abs(chi4 / (p * (1.0 - p)) - 1.0) <= tol
    assert M >= 64 and abs(s4v.mean() / p - 1.0) <= 5.0 / math.sqrt(M * ns)
    assert np.all(np.abs(s4 / p - 1.0) <= 5.0 / np.sqrt(fp.nvectors * ns))      # flat in q
    assert os.path.isfile(os.path.join(str(tmp_path), "chi4.txt")) and os.path.isfile(os.path.join(str(tmp_path), "s4.txt"))


# ---------------------------------------------------------------------------------------------------------------------
# 6: no side effects, integration

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
            dev.sq_setup(n, 1, 1)
            dev.cage_setup(1, 1, 1.5)
            dev.stress_setup(2)
            dev.boo_setup(1.5, 6, 50, 0.2, 2, 4)        # a low threshold: the liquid has solid particles to cluster
            dev.cluster_setup(1.5, 1, 1024, 4)          # members = solid: reads the bond-order frame of the same step
            r1 = dev.run(50, 0.002)
            before = dev.download()
            dev.dyn_origin(0)
            dev.sq_sample(True, [], [], 0)
            dev.cage_origin(0)
            dev.stress_sample()
            if sample:
                dev.chi4_setup(0.05, n[:100], 2, 3)
                dev.chi4_origin(1)
                mid = dev.download()
                for u, w in zip(before, mid):
                    assert np.array_equal(u, w)
            dev.run(10, 0.002)
            dev.rdf_sample()
            if sample:
                dev.chi4_sample([1, 1], [0, 2])
                dev.chi4_origin(0)
                dev.snapshot_begin()                    # a frame in flight beside a sample
                dev.chi4_sample([0], [1])
                dev.snapshot_end()
            dev.stress_sample()                         # each of these after a chi4 origin and sample, and before more
            dev.boo_sample()
            dev.cluster_sample()
            mid_particles = (dev.boo_particles(), dev.cluster_particles())
            dev.dyn_sample([0], [0])
            d1 = dev.download()
            f1 = dev.compute_forces()
            r2 = dev.run(50, 0.002)
            dev.rdf_sample()
            dev.dyn_sample([0], [1])
            dev.sq_sample(True, [0], [0])
            dev.cage_sample([0], [0])
            if sample:
                dev.chi4_sample([0, 1], [1, 2])
            dev.stress_sample()
            dev.boo_sample()
            dev.cluster_sample()
            others = (dev.stress_read(), dev.stress_tensor(), dev.boo_read(), dev.boo_particles(), dev.boo_qlm(),
                      dev.cluster_read(), dev.cluster_particles(), mid_particles)
            st = dev.stats()
            out.append((r1, r2, f1, d1, dev.download(), dev.rdf_read(), dev.dyn_read(), (st["rebuilds"], st["prunes"]),
                        dev.sq_read(), dev.cage_read(), dev.chi4_read() if sample else None, others))
    (a1, a2, af, ad1, da, ar, ay, ast, asq, acg, c4, ao), (b1, b2, bf, bd1, db, br, by, bst, bsq, bcg, _, bo) = out
    assert a1 == b1 and a2 == b2 and af == bf and ast == bst
    for u, w in zip(ad1 + da, bd1 + db):
        assert np.array_equal(u, w)                     # trajectory, velocities, forces, images
    assert np.array_equal(ar[0], br[0]) and ar[1] == br[1] == 2
    assert np.array_equal(ay[0], by[0]) and ay[1].tobytes() == by[1].tobytes() and np.array_equal(ay[2], by[2])
    assert asq[0] == bsq[0] and all(np.asarray(u).tobytes() == np.asarray(w).tobytes() for u, w in zip(asq[1:], bsq[1:]))
    assert all(np.asarray(u).tobytes() == np.asarray(w).tobytes() for u, w in zip(acg, bcg))

    def flat(t):                                        # the leaves of a nested read-back, as bytes
        if isinstance(t, (tuple, list)):
            return [b for u in t for b in flat(u)]
        return [np.asarray(t).tobytes()]

    assert len(flat(ao)) == len(flat(bo)) >= 25 and flat(ao) == flat(bo)    # stress, bond order, clusters: byte for byte
    assert ao[0][0] == 3 and ao[2][0] == 2 and ao[5][0] == 2               # samples taken: stress, bond order, clusters
    assert ao[6][1].max() > 1 and ao[7][1][1].max() > 1                     # (the solid clusters are not empty)
    ns, sq, sq2, s4 = c4
    N = s["n"]
    assert list(ns) == [1, 2, 2]
    assert 0 < sq[0] < N and sq[0] < sq[2] < 2 * N      # rows 0 and 2 hold the same first sample
    assert sq[1] >= N and sq2[1] >= N * N               # row 1 holds a frame against itself: Q = N
    assert s4[0].tobytes() != s4[2].tobytes() and np.all(s4 > 0.0)


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
    a = 0.05 if ens == "nvt" else 0.04
    paths = [str(tmp_path / k) for k in "abcd"]
    pa, pb, pc, pd = paths
    sa, sb, sc, sd = (fresh(p) for p in paths)
    both = md.FourPoint(a, q_max=6.0, max_per_bin=4)
    only = md.FourPoint(a)
    md.run_simulation(sa, params, ensemble, T, freq, pa, log_times=True, dynamics=md.SelfDynamics())
    md.run_simulation(sb, params, ensemble, T, freq, pb, log_times=True, dynamics=md.SelfDynamics(), four_point=both)
    md.run_simulation(sc, params, ensemble, T, freq, pc, log_times=True)
    md.run_simulation(sd, params, ensemble, T, freq, pd, four_point=only)
    # with log_times=True every other file of the run is byte-identical with and without the sampler
    assert set(os.listdir(pb)) == set(os.listdir(pa)) | {"chi4.txt", "s4.txt"}
    assert _files(pa, os.listdir(pa)) == _files(pb, os.listdir(pa))
    assert np.array_equal(np.asarray(sa.system.positions), np.asarray(sb.system.positions))
    assert np.array_equal(sa.images, sb.images)
    # the default schedule alone stops where log_times=True stops: the same segments, thermo and trajectory
    assert _files(pc, ["thermo.txt", "trajectory.xyz"]) == _files(pd, ["thermo.txt", "trajectory.xyz"])
    assert not glob.glob(os.path.join(pd, "snapshot.*")) and not os.path.exists(os.path.join(pd, "s4.txt"))
    reached = [1, 2, 3, 4, 6, 8, 11, 14, 20, 27]
    for fp, path in ((both, pb), (only, pd)):
        assert list(fp.lags[fp.nsamples > 0]) == reached and set(fp.nsamples) == {0, 1} and fp.n_particles == n
        lines = open(os.path.join(path, "chi4.txt")).read().splitlines()
        assert lines[0] == "# lag time Q/N chi4 nsamples" and len(lines) == 1 + len(reached)
        ov, c4 = fp.overlap(), fp.chi4()
        for line, l in zip(lines[1:], reached):
            k = int(np.nonzero(fp.lags == l)[0][0])
            assert line == "%d %.6e %.6e %.6e %d" % (l, l * params.dt, ov[k], c4[k], 1)
            assert c4[k] == 0.0                          # one sample: no variance
        got = ov[fp.nsamples > 0]
        assert got[0] > 0.5 and got[-1] < got[0]          # the overlap decays
    assert both.sum_q.tolist() == only.sum_q.tolist()   # the same trajectory, with and without vectors
    text = open(os.path.join(pb, "s4.txt")).read()
    head = "# lag time q S4 nvectors nsamples\n"
    assert text.startswith(head)
    blocks = text[len(head):].split("\n\n")
    assert len(blocks) == len(reached)
    S4 = both.s4()
    for blk, l in zip(blocks, reached):
        k = int(np.nonzero(both.lags == l)[0][0])
        rows = blk.strip("\n").split("\n")
        assert len(rows) == both.q.size
        for b, row in enumerate(rows):
            assert row == "%d %.6e %.6f %.6e %d %d" % (l, l * params.dt, both.q[b], S4[k, b], both.nvectors[b], 1)
    assert np.all(S4[both.nsamples > 0] >= 0.0)
    # two calls: the samples accumulate
    md.run_simulation(sd, params, ensemble, T, freq, pd, four_point=only)
    assert list(only.nsamples[:10]) == [2] * 10 and not only.nsamples[10:].any()
    for st in (sa, sb, sc, sd):
        st.system.device.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7: refusals

def test_refusals(monkeypatch):
    from moleculardynamics.jl_amd import MDDevice, MdhipError, _lib
    n = 1000
    ok = np.array([[1, 0, 0], [0, -2, 5]], np.int32)
    with MDDevice(3, n, 12.0, 2.5) as dev:
        dev.upload(x=np.random.default_rng(1).random((n, 3)) * 12.0)
        for call in (lambda: dev.chi4_origin(0), lambda: dev.chi4_sample([0], [0]), dev.chi4_last, dev.chi4_read,
                     dev.chi4_reset):
            with pytest.raises(MdhipError, match="no setup"):
                call()
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            with pytest.raises(MdhipError, match="a must be finite and > 0"):
                dev.chi4_setup(bad, ok, 1, 1)
        with pytest.raises(MdhipError, match="nvec"):
            dev.chi4_setup(0.3, np.ones((4097, 3), np.int32), 1, 1)
        with pytest.raises(MdhipError, match="vector 1 is n = 0"):
            dev.chi4_setup(0.3, np.array([[1, 0, 0], [0, 0, 0]], np.int32), 1, 1)
        with pytest.raises(MdhipError, match="component 2 of vector 0 is 32768"):
            dev.chi4_setup(0.3, np.array([[1, 0, 32768]], np.int32), 1, 1)
        with pytest.raises(MdhipError, match="component 0 of vector 1 is -32768"):
            dev.chi4_setup(0.3, np.array([[1, 0, 0], [-32768, 0, 0]], np.int32), 1, 1)
        for bad in (0, 65, -1):
            with pytest.raises(MdhipError, match="nslots"):
                dev.chi4_setup(0.3, ok, bad, 1)
        for bad in (0, -1):
            with pytest.raises(MdhipError, match="nrows"):
                dev.chi4_setup(0.3, ok, 1, bad)
        with pytest.raises(ValueError, match="shape"):
            dev.chi4_setup(0.3, np.ones((4, 2), np.int32))
        lib = _lib.load()
        assert lib.md_chi4_setup(dev._h, 0.3, None, 2, 1, 1) != 0 and b"n is null" in lib.md_last_error(dev._h)
        with pytest.raises(MdhipError, match="no setup"):      # a refused setup leaves no sampler behind
            dev.chi4_read()
        dev.chi4_setup(0.3, np.array([[32767, -32767, 32767]], np.int32), 64, 5)    # the limits themselves are accepted
        dev.chi4_setup(0.3, np.ones((4096, 3), np.int32), 1, 1)
        dev.chi4_setup(0.3, None, 1, 1)
        dev.chi4_setup(0.3, ok, 2, 3)
        for bad in (-1, 2):
            with pytest.raises(MdhipError, match=r"slot -?\d is out of range 0..1"):
                dev.chi4_origin(bad)
        with pytest.raises(MdhipError, match="slot 0 is empty"):
            dev.chi4_sample([0], [0])
        with pytest.raises(MdhipError, match="no sample taken"):
            dev.chi4_last()
        with pytest.raises(ValueError, match="same length"):
            dev.chi4_sample([1], [0, 1])
        dev.chi4_origin(0)
        with pytest.raises(MdhipError, match="slot 1 is empty"):
            dev.chi4_sample([0, 1], [0, 0])
        with pytest.raises(MdhipError, match=r"row 3 is out of range 0..2"):
            dev.chi4_sample([0], [3])
        with pytest.raises(MdhipError, match=r"row -1 is out of range"):
            dev.chi4_sample([0], [-1])
        with pytest.raises(MdhipError, match=r"slot 2 is out of range 0..1"):
            dev.chi4_sample([2], [0])
        ns, sq, sq2, s4 = dev.chi4_read()                       # a refused call has added nothing
        assert not ns.any() and not sq.any() and not sq2.any() and not s4.any() and s4.shape == (3, 2)
        with pytest.raises(MdhipError, match="no sample taken"):
            dev.chi4_last()
        # the overflow guard: (nsamples[row] + 1) N^2 must not pass the limit; the whole call is refused
        monkeypatch.setenv("MDHIP_CHI4_SUMQ2_LIMIT", str(2 * n * n))
        dev.chi4_sample([0, 0], [1, 1])
        with pytest.raises(MdhipError, match=r"row 1 already holds 2 samples.*overflow sum_q2"):
            dev.chi4_sample([0], [1])
        with pytest.raises(MdhipError, match=r"row 0 already holds 2 samples"):      # counted within the call
            dev.chi4_sample([0, 0, 0], [0, 0, 0])
        ns, sq, sq2, _ = dev.chi4_read()
        assert list(ns) == [0, 2, 0] and list(sq) == [0, 2 * n, 0] and list(sq2) == [0, 2 * n * n, 0]
        dev.chi4_reset()                                        # the reset makes room and keeps the origin
        dev.chi4_sample([0], [1])
        assert list(dev.chi4_read()[0]) == [0, 1, 0]
        monkeypatch.delenv("MDHIP_CHI4_SUMQ2_LIMIT")
        dev.chi4_sample([0, 0], [1, 1])
        assert list(dev.chi4_read()[0]) == [0, 3, 0]
        dev.chi4_setup(0.3, ok, 2, 3)                           # a new setup starts over: the origins are gone
        with pytest.raises(MdhipError, match="slot 0 is empty"):
            dev.chi4_sample([0], [0])
        # the slot allocation: N d 20 bytes per slot with vectors, N d 12 without
        monkeypatch.setenv("MDHIP_CHI4_ALLOC_LIMIT", "100000")
        with pytest.raises(MdhipError, match=r"cannot allocate %d bytes .*2\*1000\*3\*20" % (2 * n * 3 * 20)):
            dev.chi4_setup(0.3, ok, 2, 1)
        with pytest.raises(MdhipError, match=r"cannot allocate %d bytes .*3\*1000\*3\*12" % (3 * n * 3 * 12)):
            dev.chi4_setup(0.3, None, 3, 1)
        with pytest.raises(MdhipError, match="no setup"):
            dev.chi4_read()
        dev.chi4_setup(0.3, ok, 1, 1)                           # 60000 bytes fit the limit
        dev.chi4_setup(0.3, None, 2, 1)                         # 72000 bytes
        monkeypatch.delenv("MDHIP_CHI4_ALLOC_LIMIT")
    h = ctypes.c_void_p()
    box = (ctypes.c_double * 9)(20, 0, 0, 0, 20, 0, 0, 0, 20)
    assert lib.md_create_domain(3, 4000, 4000, box, 2.5, -1, 0, 1, ctypes.byref(h)) == 0, lib.md_last_error(None)
    try:
        assert lib.md_chi4_setup(h, 0.3, None, 0, 1, 1) != 0
        assert b"slab" in lib.md_last_error(h)
        for fn in (lambda: lib.md_chi4_origin(h, 0), lambda: lib.md_chi4_sample(h, None, None, 0),
                   lambda: lib.md_chi4_last(h, None, None, None), lambda: lib.md_chi4_read(h, None, None, None, None),
                   lambda: lib.md_chi4_reset(h)):
            assert fn() != 0
            assert b"slab" in lib.md_last_error(h)
    finally:
        lib.md_destroy(h)


# ---------------------------------------------------------------------------------------------------------------------
# a call of several pairs: one launch triple per pair, in call order

@pytest.mark.parametrize("dim", [3, 2])
def test_one_call_of_several_pairs_equals_one_call_per_pair(dim):
    """3 pairs on three origins, two of them into one row, at N = 257 with 19 wave vectors: handle A samples them in one
    call, handle B in three calls, in order.  The sampler does not batch, so this pins the order of a call's pairs: every
    read-back, and Q, W and the slow particles of the last pair, are equal bit for bit."""
    from tests.test_gpu_dynamics import _assert_identical, _ragged_frames, _ragged_handle
    from tests.test_gpu_sq import _ragged_vectors
    frames, box = _ragged_frames(dim)
    zi = np.zeros((257, dim), dtype=np.int32)
    slots, rows = [0, 1, 2], [1, 0, 1]
    out = []
    for one_call in (True, False):
        with _ragged_handle(dim, box, frames[0]) as dev:
            dev.chi4_setup(0.12, _ragged_vectors(dim), 3, 2)
            for s in range(3):
                dev.upload(frames[s], None, None, zi)
                dev.chi4_origin(s)
            dev.upload(frames[3], None, None, zi)
            if one_call:
                dev.chi4_sample(slots, rows)
            else:
                for a, b in zip(slots, rows):
                    dev.chi4_sample([a], [b])
            out.append(list(dev.chi4_read()) + list(dev.chi4_last()))
    _assert_identical(out[0], out[1])
    cnt, sum_q, sum_q2, s4, q, w, slow = out[0]
    assert list(cnt) == [1, 2] and q == slow.sum() and 0 < q < 257      # (some particles moved 0.12 in one step, not all)
    assert np.all(sum_q > 0) and np.all(s4 > 0.0)
