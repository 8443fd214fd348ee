"""-m gpu: current correlations and the VACF sampled on the device (md_cur_*, md_cur.hpp).

j(q) cannot be bit-exact against a host libm, so it is bounded: per vector, component a and part
|j_a - j_a,true| <= V_a (32 kappa |n|_1 + 128) 2^-53, V_a = sum_i |v_i,a|, j_true evaluated in extended precision from the
downloaded frame (DESIGN.md section 19 derives the bound).  Given the j values, the accumulators are exact no-fma
expressions of them and are compared bit for bit; the frame alone decides the bits of j and Z on any handle.  Known answers
that need no restatement: uniform and sinusoidal velocity fields on a simple cubic lattice (the longitudinal / transverse
split), a uniformly translating lattice, a Maxwell gas.  Sampling must leave everything else the handle and run_simulation
compute unchanged."""
import ctypes
import math
import os

import numpy as np
import pytest

from tests import cur_reference as ref
from tests.util import lj_system

pytestmark = pytest.mark.gpu
LJ = [1.0, 1.0, 2.5]
U53 = 2.0 ** -53
TILE = 4                                                        # MD_CUR_TILE
BATCH = 64                                                      # MD_CUR_MAX_BATCH
CELLS = {
    "orthorhombic": np.diag([15.0, 17.0, 19.0]),
    "sheared": np.array([[18.0, 4.5, 1.0], [0.0, 17.5, -2.0], [0.0, 0.0, 18.0]]),
    "2d": np.array([[70.0, 0.0], [0.0, 60.0]]),
    "2d-sheared": np.array([[70.0, 11.0], [0.0, 60.0]]),
}
BRAGG = np.array([[16, 0, 0], [0, 16, 0], [0, 0, 16], [16, 16, 0], [16, -16, 16], [32, 16, 0], [0, -16, 48], [-16, 0, 32],
                  [48, 48, 48]], dtype=np.int32)


def _points(U, n, seed):
    return np.random.default_rng(seed).random((n, U.shape[0])) @ U.T


def _handle(U, x, v, cutoff=2.5, pot=(0.0, 1.0, 2.5)):
    """A handle on the cell U holding (x, v); the default potential is Lennard-Jones with epsilon = 0: no forces."""
    from moleculardynamics.jl_amd import MDDevice
    n, d = x.shape
    dev = MDDevice(d, n, U, cutoff)
    dev.set_potential(0, list(pot))
    dev.upload(x, v, np.zeros_like(x), np.zeros((n, d), np.int32), np.ones(n))
    return dev


def _lattice16(U=None):
    """Simple cubic 16^3 at fractional coordinates (i + 1/4) / 16 (exact); x = U f."""
    i = np.arange(16, dtype=np.float64)
    f = np.array(np.meshgrid(i, i, i, indexing="ij")).reshape(3, -1).T
    f = (f + 0.25) / 16.0
    return f * 16.0 if U is None else f @ U.T


def _within(j, jt, bound):
    return np.all(np.abs(j.real - jt.real) <= bound) and np.all(np.abs(j.imag - jt.imag) <= bound)


def _worst(j, jt, bound):
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.maximum(np.abs(j.real - jt.real), np.abs(j.imag - jt.imag)) / bound
    return float(np.nanmax(r))


# ---------------------------------------------------------------------------------------------------------------------
# 1. the bound against extended precision

@pytest.mark.parametrize("cell", list(CELLS))
def test_j_within_the_bound_of_extended_precision(cell):
    from moleculardynamics.jl_amd import select_wave_vectors
    U = CELLS[cell]
    d = U.shape[0]
    N = 4096 + 65                                               # two particle blocks, a tail that is no multiple of 64
    x = _points(U, N, 2024)
    v = np.random.default_rng(77).standard_normal((N, d))
    n, _, _ = select_wave_vectors(U, 12.0)
    if n.shape[0] % TILE == 0:
        n = n[:-1]
    assert n.shape[0] >= 248 and n.shape[0] % TILE != 0 and np.sum(np.abs(n), axis=1).max() >= 30
    with _handle(U, x, v) as dev:
        dev.cur_setup(n, ref.directions(U, n))
        dev.cur_sample()
        j = dev.cur_last()
        fx, fv = dev.download()[:2]
    assert np.array_equal(fv, v)
    jt = ref.j_true(fx, fv, U, n)
    bound = ref.j_bound(fv, U, n)
    print(f"{cell}: nvec {n.shape[0]}, max |n|_1 {np.sum(np.abs(n), axis=1).max()}, worst error / bound "
          f"{_worst(j, jt, bound):.3e}, bound {bound.min():.2e}..{bound.max():.2e}, max |j| {np.abs(j).max():.1f}")
    assert j.shape == (n.shape[0], d)
    assert _within(j, jt, bound)                                # every vector, component and part
    assert np.abs(j).max() > 10.0                               # (not all zeros)


@pytest.mark.parametrize("nvec", [1, TILE + 1])
def test_j_with_one_vector_and_one_more_than_a_tile(nvec):
    U = CELLS["sheared"]
    N = 1000
    x = _points(U, N, 5)
    v = np.random.default_rng(6).standard_normal((N, 3))
    n = np.array([[3, -1, 2], [0, 5, 0], [-7, 0, 1], [1, 1, 1], [2, 0, -9]], np.int32)[:nvec]
    with _handle(U, x, v) as dev:
        dev.cur_setup(n, ref.directions(U, n))
        dev.cur_sample()
        j = dev.cur_last()
        fx, fv = dev.download()[:2]
    jt, bound = ref.j_true(fx, fv, U, n), ref.j_bound(fv, U, n)
    print(f"nvec {nvec}: worst error / bound {_worst(j, jt, bound):.3e}")
    assert j.shape == (nvec, 3) and _within(j, jt, bound) and np.abs(j).max() > 1.0


# ---------------------------------------------------------------------------------------------------------------------
# 2. the accumulators, bit for bit

def test_the_accumulators_are_exact_in_j():
    from moleculardynamics.jl_amd import MDDevice, select_wave_vectors
    s = lj_system(4096)
    U = np.diag(s["box"])
    n, _, _ = select_wave_vectors(U, 9.0, max_per_bin=3, seed=5)
    e = ref.directions(U, n)
    # (static, [(slot, row)], origin): statics, correlations against several slots, two samples on one row in one call,
    # a slot read and overwritten in the same call (the samples come first), more pairs than one launch takes
    many = [(k % 3, (2 * k) % 4) for k in range(BATCH + 6)]
    plan = [(True, [], 0), (False, [(0, 0)], 1), (True, [(0, 1), (1, 0)], None), (True, [(1, 2), (1, 2), (0, 3)], 1),
            (False, [(1, 0), (0, 0)], 2), (True, many, 0), (True, [(2, 3), (0, 1)], None)]
    with MDDevice(3, s["n"], s["box"], 2.5) as dev:
        dev.set_potential(0, LJ)
        dev.upload(s["x"], s["v"], s["f"], s["img"], s["diam"])
        dev.cur_setup(n, e, 3, 4)
        acc = ref.Accumulators(e, 4)
        for static, smp, origin in plan:
            dev.run(15, 0.004)
            dev.cur_sample(static, [a for a, _ in smp], [b for _, b in smp], origin)
            acc.sample(dev.cur_last(), static, smp, origin)
        nst, s_tot, s_long, ns, c_tot, c_long, z = dev.cur_read()
        assert z is None
        assert nst == acc.nstatic and list(ns) == list(acc.nsamples)
        assert s_tot.tobytes() == acc.s_tot.tobytes() and s_long.tobytes() == acc.s_long.tobytes()
        assert c_tot.tobytes() == acc.c_tot.tobytes() and c_long.tobytes() == acc.c_long.tobytes()
        assert np.all(s_tot > 0.0) and np.all(s_long > 0.0) and np.all(s_long <= s_tot)
        assert np.all(np.any(c_tot != 0.0, axis=1)) and np.all(np.any(c_long != 0.0, axis=1))
        # reset zeroes the sums and the counts and keeps the origins
        dev.cur_reset()
        z_nst, z_st, z_sl, z_ns, z_ct, z_cl, _ = dev.cur_read()
        assert z_nst == 0 and not z_ns.any() and not z_st.any() and not z_sl.any() and not z_ct.any() and not z_cl.any()
        dev.cur_sample(False, [2], [1])
        j = dev.cur_last()
        _, _, _, r_ns, r_ct, r_cl, _ = dev.cur_read()
        assert list(r_ns) == [0, 1, 0, 0]
        assert r_ct[1].tobytes() == (0.0 + ref.tot_term(j, acc.org[2])).tobytes()
        assert r_cl[1].tobytes() == (0.0 + ref.long_term(j, acc.org[2], e)).tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# 3. the frame alone decides the bits

def test_the_frame_alone_decides_the_bits():
    from moleculardynamics.jl_amd import MDDevice, select_wave_vectors
    s = lj_system(4096)
    U = np.diag(s["box"])
    n, _, _ = select_wave_vectors(U, 10.0, max_per_bin=4)
    e = ref.directions(U, n)

    def sample(dev):
        dev.cur_setup(n, e, 1, 1, vacf=True)
        dev.cur_sample(True, [], [], 0)
        dev.cur_sample(False, [0], [0])
        return dev.cur_last(), dev.cur_read()[6]

    with MDDevice(3, s["n"], s["box"], 2.5) as a:
        a.set_potential(0, LJ)
        a.upload(s["x"], s["v"], s["f"], s["img"], s["diam"])
        r0 = a.stats()["rebuilds"]
        a.run(400, 0.004)
        assert a.stats()["rebuilds"] > r0           # the particles were reordered since the upload
        j_a, z_a = sample(a)
        x1, v1, _, n1 = a.download()
    with MDDevice(3, s["n"], s["box"], 2.5) as b:
        b.set_potential(0, LJ)
        b.set_skin(0.45)
        b.upload(s["x"], s["v"], s["f"], s["img"], s["diam"])
        b.run(30, 0.002)                            # a history of its own
        j_0, z_0 = sample(b)
        assert j_0.tobytes() != j_a.tobytes() and z_0.tobytes() != z_a.tobytes()
        b.upload(x1, v1, None, n1)
        assert np.array_equal(b.download()[0], x1) and np.array_equal(b.download()[1], v1)
        j_b, z_b = sample(b)
    assert j_b.tobytes() == j_a.tobytes() and z_b.tobytes() == z_a.tobytes()
    assert z_a[0] == z_a[1] != 0.0                  # the frame against itself as a lag sample and as the static sample
    assert _within(j_a, ref.j_true(x1, v1, U, n), ref.j_bound(v1, U, n))


# ---------------------------------------------------------------------------------------------------------------------
# 4. known answers on a simple cubic lattice

def _lattice_vectors():
    from moleculardynamics.jl_amd import select_wave_vectors
    sel, _, _ = select_wave_vectors(np.eye(3) * 16.0, 14.0)
    return np.concatenate([BRAGG, sel, np.array([[16, 1, 0], [15, 0, 0], [16, 16, 8], [1, 1, 1]], np.int32)])


def test_lattice_with_one_velocity_for_all():
    """j_a = v0_a rho: N v0_a exp(2 pi i (n_0 + n_1 + n_2) / 64) at a Bragg vector, 0 elsewhere."""
    U = np.eye(3) * 16.0
    x, N = _lattice16(), 4096
    v0 = np.array([1.0, -2.0, 0.5])
    v = np.tile(v0, (N, 1))
    n = _lattice_vectors()
    with _handle(U, x, v) as dev:
        dev.cur_setup(n, ref.directions(U, n))
        dev.cur_sample()
        j = dev.cur_last()
    is_bragg = np.all(n % 16 == 0, axis=1)
    assert is_bragg.sum() >= len(BRAGG) and (~is_bragg).sum() > 200
    rho = np.zeros(n.shape[0], dtype=np.complex128)
    rho[is_bragg] = N * np.array([[1, 1j, -1, -1j][int(k) % 4] for k in np.sum(n[is_bragg], axis=1) // 16])
    expect = rho[:, None] * v0[None, :]
    bound = ref.j_bound(v, U, n)
    print(f"uniform velocity: worst error / bound {_worst(j, expect, bound):.3e}")
    assert _within(j, expect, bound)


@pytest.mark.parametrize("along", ["y", "x"])
def test_lattice_with_a_sinusoidal_velocity_field(along):
    """v_i = A u sin(q0.x_i), q0 = 2 pi (3, 0, 0) / L: j_u(q0) = A sum (sin cos + i sin^2) = i A N / 2 (the 2 q0 sums
    vanish on the lattice).  u = y (transverse to q0): C_L(q0, 0) = 0, C_T(q0, 0) = A^2 N / (4 (d - 1)); u = x
    (longitudinal): C_L = A^2 N / 4, C_T = 0.  The wrong way round fails both.  Tolerance: the bound b of j propagated
    through the squares, sum over the parts of 2 |j| b + b^2, plus 8 roundings of the value."""
    U = np.eye(3) * 16.0
    x, N, A, d = _lattice16(), 4096, 1.7, 3
    a = "xyz".index(along)
    n = np.array([[3, 0, 0], [5, 0, 0]], np.int32)
    v = np.zeros((N, 3))
    v[:, a] = A * np.sin(2.0 * math.pi * 3.0 * x[:, 0] / 16.0)
    e = ref.directions(U, n)
    assert np.array_equal(e, [[1.0, 0, 0], [1.0, 0, 0]])
    with _handle(U, x, v) as dev:
        dev.cur_setup(n, e)
        dev.cur_sample()
        j = dev.cur_last()
        fv = dev.download()[1]
        nst, s_tot, s_long, _, _, _, _ = dev.cur_read()
    # the velocities are sin() of the host: the expected sum uses the uploaded values' own mean square
    b = ref.j_bound(fv, U, n)
    expect = np.zeros((2, 3), dtype=np.complex128)
    expect[0, a] = 1j * A * N / 2.0
    slack = A * N * 64 * U53 + b                                # (sin of the host rounds each v_i: <= A u each, N of them)
    assert np.all(np.abs(j.real - expect.real) <= slack) and np.all(np.abs(j.imag - expect.imag) <= slack)
    cl0 = s_long / (nst * N)
    ct0 = (s_tot - s_long) / ((d - 1) * nst * N)
    mag = A * N / 2.0
    tol = (2.0 * mag * slack[0, a] + slack[0, a] ** 2) * 2 / N + 8 * U53 * A * A * N / 4.0
    want_l, want_t = (0.0, A * A * N / (4.0 * (d - 1))) if along == "y" else (A * A * N / 4.0, 0.0)
    print(f"{along}: C_L {cl0[0]:.9e} (want {want_l:.9e}), C_T {ct0[0]:.9e} (want {want_t:.9e}), tol {tol:.2e}")
    assert abs(cl0[0] - want_l) <= tol and abs(ct0[0] - want_t) <= tol
    assert abs(cl0[1]) <= tol and abs(ct0[1]) <= tol            # nothing at another q


# ---------------------------------------------------------------------------------------------------------------------
# 5. a translating lattice

@pytest.mark.parametrize("shear", [0.0, 4.5])
def test_uniform_translation_pins_the_correlations(shear):
    """Zero potential, one velocity v0 for all: j(q, t) = v0 rho(q, 0) exp(i q.v0 t), so at a Bragg vector
    c_tot = |v0|^2 N^2 cos(q.v0 l dt) and c_long = (e.v0)^2 N^2 cos(q.v0 l dt).  Tolerance, as for md_sq's translating
    lattice: the velocities never change (f = 0), a step rounds x_c by at most u 32 (|x| < 32) in each of at most 4
    operations (drift, wrap), so after S steps |dx_c| <= 128 u S in each of the two frames, the phase q.x is off by at most
    |q|_1 128 u S per frame, and the cosine by at most twice that; j's own bound adds a relative 1e-12."""
    U = np.array([[16.0, shear, 0.0], [0.0, 16.0, 0.0], [0.0, 0.0, 16.0]])
    x = _lattice16(U)
    N, dt = 4096, 0.02
    v0 = np.array([7.31, -5.17, 3.73])
    v = np.tile(v0, (N, 1))
    n = BRAGG
    q = 2.0 * math.pi * (n.astype(np.float64) @ np.linalg.inv(U))
    qv = q @ v0
    e = ref.directions(U, n)
    plan = [(0, [], 0), (1, [(0, 0)], None), (100, [(0, 1)], 1), (250, [(0, 2), (1, 3)], None), (400, [(0, 4), (1, 5)], None)]
    lag = [1, 100, 250, 150, 400, 300]
    with _handle(U, x, v) as dev:
        dev.cur_setup(n, e, 2, len(lag))
        done = 0
        for step, smp, origin in plan:
            if step > done:
                dev.run(step - done, dt)
            done = step
            dev.cur_sample(True, [a for a, _ in smp], [b for _, b in smp], origin)
        nst, s_tot, s_long, ns, c_tot, c_long, _ = dev.cur_read()
        _, fv, _, img = dev.download()
    assert np.array_equal(fv, v) and np.abs(img).max() >= 3     # the velocities are untouched; several crossings
    assert nst == len(plan) and list(ns) == [1] * len(lag)
    rel = 2.0 * np.sum(np.abs(q), axis=1) * 128 * U53 * done + 1e-12
    v2, ev2 = float(v0 @ v0), (e @ v0) ** 2
    assert np.all(np.abs(s_tot - nst * v2 * N * N) <= nst * rel * v2 * N * N)
    distinct = 0
    for k, l in enumerate(lag):
        c = np.cos(qv * l * dt)
        et, el = np.abs(c_tot[k] - v2 * N * N * c), np.abs(c_long[k] - ev2 * N * N * c)
        print(f"shear {shear}: lag {l}, worst error / tolerance {max((et / (rel * v2 * N * N)).max(), (el / (rel * v2 * N * N)).max()):.3e}")
        assert np.all(et <= rel * v2 * N * N) and np.all(el <= rel * v2 * N * N), l
        distinct += int(np.abs(c).min() < 0.9)
    assert distinct >= 4                            # the expected values are not trivially +-1


# ---------------------------------------------------------------------------------------------------------------------
# 6. a Maxwell gas at equal time

def test_maxwell_gas():
    """Uniform points, Gaussian velocities at kT = 1.5: e.j and each transverse component of j are sums of N independent
    terms of variance kT / 2 per part, so |e.j|^2 / (N kT) is a unit-mean exponential per vector and the transverse mean
    (over d - 1 = 2 components) a narrower one; the mean over M vectors lies in 1 +- 5 / sqrt(M).  tests/cur_reference.py
    (j_true in extended precision on the CPU, the same seeds) gives, for these seeds and M = 557 vectors, longitudinal
    1.00906 and transverse 1.05199: inside 1 +- 0.21186."""
    from moleculardynamics.jl_amd import select_wave_vectors
    N, kT = 200000, 1.5
    L = (N / 0.5) ** (1.0 / 3.0)
    U = np.eye(3) * L
    x = _points(U, N, 31337)
    v = math.sqrt(kT) * np.random.default_rng(4711).standard_normal((N, 3))
    n, _, _ = select_wave_vectors(U, 3.0)
    M = n.shape[0]
    assert M >= 500
    with _handle(U, x, v) as dev:
        dev.cur_setup(n, ref.directions(U, n))
        dev.cur_sample()
        _, s_tot, s_long, _, _, _, _ = dev.cur_read()
    lo = s_long.mean() / (N * kT)
    tr = ((s_tot - s_long) / 2.0).mean() / (N * kT)
    print(f"Maxwell gas: M = {M}, longitudinal {lo:.5f}, transverse {tr:.5f}, 5 / sqrt(M) = {5.0 / math.sqrt(M):.5f}")
    assert abs(lo - 1.0) <= 5.0 / math.sqrt(M) and abs(tr - 1.0) <= 5.0 / math.sqrt(M)


# ---------------------------------------------------------------------------------------------------------------------
# 7. the velocity autocorrelation

def test_vacf_within_the_bound():
    U = CELLS["orthorhombic"]
    N = 4096 + 65
    x = _points(U, N, 9)
    rng = np.random.default_rng(10)
    v, w = rng.standard_normal((N, 3)), rng.standard_normal((N, 3))
    with _handle(U, x, v) as dev:
        dev.cur_setup(None, None, 1, 1, vacf=True)              # no vectors: Z only
        dev.cur_sample(True, [], [], 0)
        dev.upload(v=w)
        dev.cur_sample(False, [0], [0])
        nst, s_tot, s_long, ns, c_tot, c_long, z = dev.cur_read()
        assert dev.cur_last().shape == (0, 3)
    assert nst == 1 and list(ns) == [1] and s_tot.size == 0 and c_tot.shape == (1, 0) and z.shape == (2,)
    for got, (zt, A) in ((z[0], ref.z_true(w, v)), (z[1], ref.z_true(v, v))):
        print(f"Z {got:.9e}, error / bound {abs(got - zt) / (A * 64 * U53):.3e}")
        assert abs(got - zt) <= A * 64 * U53
    assert z[1] > 0.9 * 3 * N


def test_vacf_of_free_particles_is_constant_and_odd_in_v():
    """Zero potential in NVE: v never changes, so every lag row with one sample holds the bytes of the static Z(0); after
    v -> -v between origin and sample, Z = -Z(0) to the bit."""
    U = CELLS["sheared"]
    N = 4096 + 65
    x = _points(U, N, 19)
    v = np.random.default_rng(20).standard_normal((N, 3))
    with _handle(U, x, v) as dev:
        dev.cur_setup(None, None, 2, 4, vacf=True)
        dev.cur_sample(True, [], [], 0)
        dev.run(7, 0.003)
        dev.cur_sample(False, [0], [0], 1)
        dev.run(5, 0.003)
        dev.cur_sample(False, [0, 1], [1, 2])
        dev.upload(v=-v)
        dev.cur_sample(False, [1], [3])
        nst, _, _, ns, _, _, z = dev.cur_read()
    assert nst == 1 and list(ns) == [1, 1, 1, 1]
    z0 = z[4:5]
    assert z0[0] > 0.0
    for k in range(3):
        assert z[k:k + 1].tobytes() == z0.tobytes()
    assert z[3:4].tobytes() == (-z0).tobytes()


def test_z_is_refused_without_vacf():
    from moleculardynamics.jl_amd import MdhipError
    U = CELLS["orthorhombic"]
    x = _points(U, 1000, 1)
    n = np.array([[1, 0, 0]], np.int32)
    with _handle(U, x, np.ones_like(x)) as dev:
        dev.cur_setup(n, ref.directions(U, n), 1, 1, vacf=False)
        dev.cur_sample()
        assert dev.cur_read()[6] is None
        z = np.zeros(2)
        rc = dev._L.md_cur_read(dev._h, None, None, None, None, None, None, z.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
        assert rc != 0 and b"vacf" in dev._L.md_last_error(dev._h)
        with pytest.raises(MdhipError, match="nvec"):
            dev.cur_setup(None, None, 1, 1, vacf=False)        # nothing to sample


# ---------------------------------------------------------------------------------------------------------------------
# 8. no side effects

@pytest.mark.parametrize("ens", ["nve", "nvt"])
def test_no_side_effects(ens):
    from moleculardynamics.jl_amd import MDDevice, select_wave_vectors
    s = lj_system(4096)
    U = np.diag(s["box"])
    n, _, _ = select_wave_vectors(U, 8.0, max_per_bin=4)
    e = ref.directions(U, n)
    nf = 3.0 * (s["n"] - 1)

    def run(dev, k, seed):
        if ens == "nve":
            return dev.run(k, 0.002)
        rng = np.random.default_rng(seed)
        return dev.run(k, 0.002, 1, 0.05, nf, np.full(k, 1.2), rng.standard_normal(k), rng.chisquare(nf - 1, k), thermo=True)

    out = []
    for sample in (True, False):
        with MDDevice(3, s["n"], s["box"], 2.5) as dev:
            dev.set_potential(0, LJ)
            dev.upload(s["x"], s["v"], s["f"], s["img"], s["diam"])
            dev.sq_setup(n, 1, 1)
            dev.dyn_setup(1, 2, [2.0 * math.pi], 2.0, 50)
            dev.stress_setup(2)
            if sample:
                dev.cur_setup(n, e, 2, 3, vacf=True)
            r1 = run(dev, 50, 1)
            before = dev.download()
            dev.dyn_origin(0)
            dev.sq_sample(True, [], [], 0)
            dev.stress_sample()
            if sample:
                dev.cur_sample(True, [], [], 1)
                for u, w in zip(before, dev.download()):
                    assert np.array_equal(u, w)
            r2 = run(dev, 10, 2)
            if sample:
                dev.cur_sample(True, [1, 1], [0, 2], 0)
                dev.snapshot_begin()                # a frame in flight beside a sample
                dev.cur_sample(False, [0], [1])
                dev.snapshot_end()
            dev.dyn_sample([0], [0])
            dev.sq_sample(True, [0], [0])
            dev.stress_sample()
            d1 = dev.download()
            r3 = run(dev, 50, 3)
            dev.dyn_sample([0], [1])
            dev.stress_sample()
            st = dev.stats()
            out.append((r1, r2, r3, d1 + dev.download(), dev.sq_read(), dev.dyn_read(), dev.stress_read(),
                        (st["rebuilds"], st["prunes"]), dev.cur_read() if sample else None))
    (a1, a2, a3, da, asq, ady, astr, ast, cur), (b1, b2, b3, db, bsq, bdy, bstr, bst, _) = out
    assert a1 == b1 and a2 == b2 and a3 == b3 and ast == bst     # U, W, K of every segment; rebuilds and prunes
    for u, w in zip(da, db):
        assert np.array_equal(u, w)                 # trajectory, velocities, forces, images
    for got, want in ((asq, bsq), (ady, bdy), (astr, bstr)):
        for u, w in zip(got, want):
            assert np.asarray(u).tobytes() == np.asarray(w).tobytes()
    nst, s_tot, s_long, ns, c_tot, c_long, z = cur
    assert nst == 2 and list(ns) == [1, 1, 1]
    assert c_tot[0].tobytes() == c_tot[2].tobytes() and z[0] == z[2]       # the same frame against the same origin
    assert np.all(c_tot[1] > 0.0) and z[1] > 0.0    # row 1: the second frame against itself


# ---------------------------------------------------------------------------------------------------------------------
# 9. refusals

def test_errors():
    from moleculardynamics.jl_amd import MDDevice, MdhipError, _lib
    ok = np.array([[1, 0, 0], [0, -2, 5]], np.int32)
    ek = np.array([[1.0, 0, 0], [0, -0.4, 0.9]])
    with MDDevice(3, 1000, 12.0, 2.5) as dev:
        rng = np.random.default_rng(1)
        dev.upload(x=rng.random((1000, 3)) * 12.0, v=rng.standard_normal((1000, 3)))
        for call in (lambda: dev.cur_sample(), dev.cur_last, dev.cur_read, dev.cur_reset):
            with pytest.raises(MdhipError, match="no setup"):
                call()
        with pytest.raises(MdhipError, match="nvec"):
            dev.cur_setup(np.zeros((0, 3), np.int32), np.zeros((0, 3)))
        with pytest.raises(MdhipError, match="nvec"):
            dev.cur_setup(np.ones((16385, 3), np.int32), np.ones((16385, 3)))
        with pytest.raises(MdhipError, match="vector 1 is n = 0"):
            dev.cur_setup(np.array([[1, 0, 0], [0, 0, 0]], np.int32), ek)
        with pytest.raises(MdhipError, match="component 2 of vector 0 is 32768"):
            dev.cur_setup(np.array([[1, 0, 32768]], np.int32), ek[:1])
        with pytest.raises(MdhipError, match="direction 1 must be finite and not all zero"):
            dev.cur_setup(ok, np.array([[1.0, 0, 0], [0, 0, 0]]))
        with pytest.raises(MdhipError, match="direction 0 must be finite"):
            dev.cur_setup(ok, np.array([[float("nan"), 0, 0], [0, 1.0, 0]]))
        with pytest.raises(MdhipError, match="nslots"):
            dev.cur_setup(ok, ek, 65, 1)
        with pytest.raises(MdhipError, match="nslots"):
            dev.cur_setup(ok, ek, -1, 1)
        with pytest.raises(MdhipError, match="nrows"):
            dev.cur_setup(ok, ek, 1, -1)
        with pytest.raises(ValueError, match="shape"):
            dev.cur_setup(np.ones((4, 2), np.int32), np.ones((4, 2)))
        with pytest.raises(ValueError, match="shape"):
            dev.cur_setup(ok, np.ones((3, 3)))
        with pytest.raises(MdhipError, match="no setup"):      # a refused setup leaves no sampler behind
            dev.cur_read()
        os.environ["MDHIP_CUR_ALLOC_LIMIT"] = "1000"
        try:
            with pytest.raises(MdhipError, match=r"cannot allocate 48000 bytes for 2 velocity origin slots"):
                dev.cur_setup(ok, ek, 2, 3, vacf=True)
        finally:
            del os.environ["MDHIP_CUR_ALLOC_LIMIT"]
        dev.cur_setup(ok, ek, 2, 3, vacf=True)
        with pytest.raises(MdhipError, match="no frame"):
            dev.cur_last()
        with pytest.raises(MdhipError, match="origin slot 2 is out of range"):
            dev.cur_sample(True, [], [], 2)
        with pytest.raises(MdhipError, match="origin slot -2 is out of range"):
            dev.cur_sample(True, [], [], -2)
        with pytest.raises(MdhipError, match="empty"):
            dev.cur_sample(True, [1], [0])
        with pytest.raises(ValueError, match="same length"):
            dev.cur_sample(True, [1], [0, 1])
        dev.cur_sample(False, [], [], 1)
        with pytest.raises(MdhipError, match="empty"):          # (the samples come before the origin)
            dev.cur_sample(True, [0], [0], 0)
        with pytest.raises(MdhipError, match="row 3 is out of range"):
            dev.cur_sample(True, [1], [3])
        with pytest.raises(MdhipError, match="row -1 is out of range"):
            dev.cur_sample(True, [1], [-1])
        with pytest.raises(MdhipError, match="slot 5 is out of range"):
            dev.cur_sample(True, [5], [0])
        nst, s_tot, _, ns, c_tot, _, z = dev.cur_read()         # a refused call has counted nothing
        assert nst == 0 and not ns.any() and not s_tot.any() and c_tot.shape == (3, 2) and not z.any()
        dev.cur_setup(ok, ek, 2, 3)                             # a new setup starts over: the origins are gone
        with pytest.raises(MdhipError, match="empty"):
            dev.cur_sample(True, [1], [0])
    lib = _lib.load()
    h = ctypes.c_void_p()
    box = (ctypes.c_double * 9)(20, 0, 0, 0, 20, 0, 0, 0, 20)
    assert lib.md_create_domain(3, 4000, 4000, box, 2.5, -1, 0, 1, ctypes.byref(h)) == 0, lib.md_last_error(None)
    try:
        vec = (ctypes.c_int32 * 3)(1, 0, 0)
        dr = (ctypes.c_double * 3)(1.0, 0.0, 0.0)
        assert lib.md_cur_setup(h, vec, dr, 1, 0, 0, 0) != 0
        assert b"slab" in lib.md_last_error(h)
        assert lib.md_cur_sample(h, 1, None, None, 0, -1) != 0
        assert b"slab" in lib.md_last_error(h)
        assert lib.md_cur_last(h, None) != 0
        assert lib.md_cur_read(h, None, None, None, None, None, None, None) != 0
        assert lib.md_cur_reset(h) != 0
    finally:
        lib.md_destroy(h)


# ---------------------------------------------------------------------------------------------------------------------
# 10. run_simulation(..., currents=...)

def _files(path, names):
    return {f: open(os.path.join(path, f), "rb").read() for f in names}


def test_run_simulation_integration(tmp_path, monkeypatch):
    import moleculardynamics.jl_amd as md
    monkeypatch.chdir(tmp_path)                                 # log_times=True writes new-log-times.txt where it runs
    n, T, freq, kT = 4096, 31, 10, 1.5
    params = md.Parameters(0.8, n, 0.002, md.LennardJones())

    def fresh(path):
        st = md.initialize_state(params, path, random_init=True, cutoff=2.5, rng=np.random.default_rng(11))
        st.velocities = md.initialize_velocities(kT, np.random.default_rng(12), n, 3)
        return st

    ensemble = md.NVT(kT, 0.05)
    pa, pb, pc = (str(tmp_path / k) for k in "abc")
    sa, sb, sc = fresh(pa), fresh(pb), fresh(pc)
    cur = md.CurrentCorrelations(12.0, max_per_bin=8)
    md.run_simulation(sa, params, ensemble, T, freq, pa, log_times=True)
    md.run_simulation(sb, params, ensemble, T, freq, pb, currents=cur)
    # the default schedule stops where log_times=True stops: the same segments, thermo, trajectory and final state
    names = ["thermo.txt", "trajectory.xyz", "final.xyz"]
    assert _files(pa, names) == _files(pb, names)
    assert np.array_equal(np.asarray(sa.system.positions), np.asarray(sb.system.positions))
    assert np.array_equal(np.asarray(sa.velocities), np.asarray(sb.velocities)) and np.array_equal(sa.images, sb.images)
    # explicit lags add their stops; a run with a SelfDynamics on the same schedule has the same stops
    cur2 = md.CurrentCorrelations(None, lags=[3, 7], origin_every=5)
    sd = fresh(str(tmp_path / "d"))
    md.run_simulation(sc, params, ensemble, T, freq, pc, currents=cur2)
    md.run_simulation(sd, params, ensemble, T, freq, str(tmp_path / "d"), dynamics=md.SelfDynamics(lags=[3, 7], origin_every=5))
    assert _files(pc, names) == _files(str(tmp_path / "d"), names)
    assert "vacf.txt" in os.listdir(pc) and "currents.txt" not in os.listdir(pc)
    # the files and the equal-time values: C_L(q, 0) = C_T(q, 0) = kT_kinetic for independent velocities; a bin of M
    # vectors and nst frames averages M nst exponentials (2 M nst for the transverse part): a few sigma
    assert cur.nstatic == 1 and cur.n_particles == n           # one origin stop (step 0) in 31 steps
    reached = [1, 2, 3, 4, 6, 8, 11, 14, 20, 27]
    assert list(cur.lags[cur.nsamples > 0]) == reached and set(cur.nsamples) == {0, 1}
    temp = cur.vacf0() / 3.0                                    # Z(0) / d of the sampled frame (the state after step 0)
    assert abs(temp - kT) <= 0.02 * kT
    cl0, ct0 = cur.cl0(), cur.ct0()
    sig_l = temp / np.sqrt(cur.nvectors)
    print(f"kinetic T {temp:.4f}: C_L(q,0) {cl0.min():.3f}..{cl0.max():.3f}, C_T(q,0) {ct0.min():.3f}..{ct0.max():.3f}, "
          f"worst deviation in sigma {np.abs((cl0 - temp) / sig_l).max():.2f} (L), "
          f"{np.abs((ct0 - temp) / (sig_l / math.sqrt(2))).max():.2f} (T)")
    assert np.all(np.abs(cl0 - temp) <= 5.0 * sig_l) and np.all(np.abs(ct0 - temp) <= 5.0 * sig_l / math.sqrt(2.0))
    assert abs(cl0.mean() - temp) <= 5.0 * temp * math.sqrt(np.sum(1.0 / cur.nvectors)) / cur.q.size
    text = open(os.path.join(pb, "currents.txt")).read()
    head = "# lag time q C_L C_T nsamples\n"
    assert text.startswith(head)
    blocks = text[len(head):].split("\n\n")
    assert len(blocks) == 1 + len(reached)
    CL, CT = cur.cl(), cur.ct()
    for blk, l in zip(blocks, [0] + reached):
        rows = blk.strip("\n").split("\n")
        assert len(rows) == cur.q.size
        for b, row in enumerate(rows):
            if l == 0:
                assert row == "%d %.6e %.6f %.6e %.6e %d" % (0, 0.0, cur.q[b], cl0[b], ct0[b], 1)
            else:
                k = int(np.nonzero(cur.lags == l)[0][0])
                assert row == "%d %.6e %.6f %.6e %.6e %d" % (l, l * params.dt, cur.q[b], CL[k, b], CT[k, b], 1)
    zl = open(os.path.join(pb, "vacf.txt")).read().splitlines()
    assert zl[0] == "# lag time Z Z/Z(0) nsamples" and [int(r.split()[0]) for r in zl[1:]] == [0] + reached
    z = cur.vacf()
    assert z[0] < cur.vacf0() and z[0] > 0.9 * cur.vacf0()      # one step later: barely decayed
    for st in (sa, sb, sc, sd):
        st.system.device.close()
