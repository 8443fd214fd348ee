"""-m gpu: the pressure tensor and its lag correlations sampled on the device (md_stress_*, md_stress.hpp).

The virial tensor W_ab = sum over accepted pairs of (f/r) del_a del_b is checked against the oracle's pair set with del in
the reference's canonical form, (u, f) from the oracle's evaluate and math.fsum as the summation, to 1e-12 of the
absolute-term scale A = sum |f/r| d2 (the project's stated relative tolerance for U and W, tests/test_gpu_parity.py; applied
to A because off-diagonal sums cancel); against two answers that need no oracle (the trace is the W of compute_forces; the
tensor is minus the strain derivative of the energy); the ring arithmetic is restated bit for bit; and a sample must leave
everything else the handle computes unchanged."""
import ctypes
import math
import os

import numpy as np
import pytest

from tests.pair_reference import canon_delta as _canon_delta, d2_of as _d2, tric_delta as _tric_delta
from tests.util import lj_system, poly_system

pytestmark = pytest.mark.gpu
LJ = [1.0, 1.0, 2.5]
LJ_FS = [1.0, 1.0, 2.5, 1.0, 0.0]                       # MD_POT_LJ_MODIFIED mode 1: force-shifted, u and f continuous at r_cut
TRIC_U = np.array([[18.0, 4.5, 0.0], [0.0, 17.5, 0.0], [0.0, 0.0, 18.0]])   # test_gpu_rdf.py::test_bit_exact_general_cell's


def _comp(d):
    return [(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)] if d == 3 else [(0, 0), (1, 1), (0, 1)]


def _virial_ref(oracle, pot, de, pairs, diam):
    """(W_ref[nc], A): components summed with math.fsum over the pairs, (u, f) from the oracle per pair; A = sum |f/r| d2."""
    d = de.shape[1]
    d2 = _d2(de)
    r = np.sqrt(d2)
    fpr = np.empty(len(pairs))
    s1, s2 = diam[pairs[:, 0]], diam[pairs[:, 1]]
    for k in range(len(pairs)):
        fpr[k] = oracle.evaluate(pot, float(r[k]), float(s1[k]), float(s2[k]))[1]
    fpr = fpr / r
    W = np.array([math.fsum(fpr * de[:, a] * de[:, b]) for a, b in _comp(d)])
    A = math.fsum(np.abs(fpr) * d2)
    return W, A


def _kinetic_ref(v):
    d = v.shape[1]
    return np.array([math.fsum(v[:, a] * v[:, b]) for a, b in _comp(d)]), math.fsum((v * v).sum(axis=1))


def _device(s, cutoff=2.5, pot=LJ, kind=0):
    from moleculardynamics.jl_amd import MDDevice
    dev = MDDevice(s["dim"], s["n"], s["box"], cutoff)
    dev.set_potential(kind, pot)
    dev.upload(s["x"], s["v"], s["f"], s["img"], s["diam"])
    return dev


def _check(kin, vir, x, v, Wref, A, label=""):
    Kref, v2 = _kinetic_ref(v)
    errw = np.abs(vir - Wref).max() / A
    errk = np.abs(kin - Kref).max() / v2
    print("%s virial err/A %.3e  kinetic err/sum v^2 %.3e  A %.6e" % (label, errw, errk, A))
    assert A > 0.0 and np.all(np.abs(vir - Wref) <= 1e-12 * A), (vir, Wref, A)
    assert np.all(np.abs(kin - Kref) <= 1e-12 * v2), (kin, Kref)


_cache = {}


def _lj4000(oracle):
    """The shared N = 4000 LJ frame (15 full tiles + 160): device state after 60 steps, its tensor, the oracle's answer."""
    if "lj4000" not in _cache:
        s = lj_system(4000)
        with _device(s) as dev:
            dev.run(60, 0.002)
            x, v, _, img = dev.download()
            dev.stress_setup(0)
            dev.stress_sample()
            kin, vir = dev.stress_tensor()
            _, w = dev.compute_forces()
            tiled = dev.stats()["tiled"]
        pairs = oracle.pairs_cells(x, s["box"], 2.5)
        Wref, A = _virial_ref(oracle, oracle.make_pot(0, LJ), _canon_delta(x, s["box"], pairs), pairs, s["diam"])
        _cache["lj4000"] = dict(s=s, x=x, v=v, img=img, kin=kin, vir=vir, w=w, Wref=Wref, A=A, tiled=tiled)
    return _cache["lj4000"]


def test_against_the_oracle_4000(oracle):
    c = _lj4000(oracle)
    assert c["tiled"] == 1
    _check(c["kin"], c["vir"], c["x"], c["v"], c["Wref"], c["A"], "lj4000")


def test_against_the_oracle_32768(oracle):
    s = lj_system(32768)
    with _device(s) as dev:
        dev.run(60, 0.002)
        x, v, _, _ = dev.download()
        dev.stress_setup(0)
        dev.stress_sample()
        kin, vir = dev.stress_tensor()
    pairs = oracle.pairs_cells(x, s["box"], 2.5)
    Wref, A = _virial_ref(oracle, oracle.make_pot(0, LJ), _canon_delta(x, s["box"], pairs), pairs, s["diam"])
    _check(kin, vir, x, v, Wref, A, "lj32768")


def test_against_the_oracle_2d_polydisperse(oracle):
    s = poly_system()
    with _device(s, cutoff=1.5, pot=[1.25, 0.2], kind=2) as dev:
        dev.run(60, 0.001)
        x, v, _, _ = dev.download()
        dev.stress_setup(0)
        dev.stress_sample()
        kin, vir = dev.stress_tensor()
    assert kin.shape == (3,) and vir.shape == (3,)
    pairs = oracle.pairs_cells(x, s["box"], 1.5)
    Wref, A = _virial_ref(oracle, oracle.make_pot(2, [1.25, 0.2]), _canon_delta(x, s["box"], pairs), pairs, s["diam"])
    _check(kin, vir, x, v, Wref, A, "poly2d")


def test_against_the_oracle_general_cell(oracle):
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
        x, v, _, _ = dev.download()
        dev.stress_setup(0)
        dev.stress_sample()
        kin, vir = dev.stress_tensor()
    with oracle.set_cell(U):
        pot = oracle.make_pot(0, LJ)
        _, _, _, pairs = oracle.forces_brute(x, np.ones(3), 2.5, pot, np.ones(n), want_pairs=True)
    Wref, A = _virial_ref(oracle, pot, _tric_delta(x, U, pairs), pairs, np.ones(n))
    assert abs(Wref[3]) > 1e-9 * A                       # a sheared cell: the off-diagonal sum is not an accident of symmetry
    _check(kin, vir, x, v, Wref, A, "tric")


def test_global_gather_path(oracle, monkeypatch):
    c = _lj4000(oracle)
    s = c["s"]
    monkeypatch.setenv("MDHIP_NO_TILES", "1")
    from moleculardynamics.jl_amd import MDDevice
    with MDDevice(3, s["n"], s["box"], 2.5) as dev:
        dev.set_potential(0, LJ)
        # the shared frame itself: what the tiled handle downloaded
        dev.upload(c["x"], c["v"], np.zeros_like(c["x"]), c["img"], s["diam"])
        dev.stress_setup(0)
        dev.stress_sample()
        kin, vir = dev.stress_tensor()
        assert dev.stats()["tiled"] == 0
    _check(kin, vir, c["x"], c["v"], c["Wref"], c["A"], "lj4000 global-gather")
    assert np.all(np.abs(vir - c["vir"]) <= 2e-12 * c["A"])
    assert np.all(np.abs(kin - c["kin"]) <= 2e-12 * _kinetic_ref(c["v"])[1])


def test_identities(oracle):
    c = _lj4000(oracle)
    vir, kin = c["vir"], c["kin"]
    assert abs(((vir[0] + vir[1]) + vir[2]) - c["w"]) <= 1e-12 * c["A"]
    v2 = math.fsum((c["v"] * c["v"]).sum(axis=1))
    assert abs(((kin[0] + kin[1]) + kin[2]) - v2) <= 1e-12 * v2


def test_strain_derivative():
    """W_ab = -dU/d eps_ab under x -> (I + eps E_ab) x, cell -> (I + eps E_ab) cell, by a central difference of
    compute_forces()[0] on fresh handles, h = 1e-4, force-shifted LJ (plain truncated LJ jumps by u(r_c) per crossing pair).
    Bound 1e-6 A = 7 x the worst truncation + rounding error of this difference measured on the reference alone
    (forces_brute under set_cell, N = 1000 jittered lattice, the same potential, h = 1e-4: 7.5e-11 A for xy, 5.5e-11 A for
    yz, 1.4e-7 A for xx -- pure h^2 truncation, 1.3e-8 A at h = 3e-5)."""
    from moleculardynamics.jl_amd import MDDevice
    n, h = 4000, 1e-4
    s = lj_system(n)
    with _device(s, pot=LJ_FS, kind=3) as dev:
        dev.run(60, 0.002)                               # a short melt
        x, v, _, _ = dev.download()
        dev.stress_setup(0)
        dev.stress_sample()
        _, vir = dev.stress_tensor()
    U0 = np.diag(s["box"])
    A = _abs_scale_fs(x, s["box"])                    # the absolute-term scale, from the frame alone (numpy)

    def energy(E, eps):
        F = np.eye(3) + eps * E
        with MDDevice(3, n, F @ U0, 2.5) as d:
            d.set_potential(3, LJ_FS)
            d.upload(x @ F.T, v, np.zeros_like(x), np.zeros((n, 3), np.int32), s["diam"])
            return d.compute_forces()[0]

    for (a, b), w in zip([(0, 1), (1, 2), (0, 0)], [vir[3], vir[5], vir[0]]):
        E = np.zeros((3, 3))
        E[a, b] = 1.0
        fd = (energy(E, h) - energy(E, -h)) / (2.0 * h)
        print("strain E_%d%d: FD %.10e  W %.10e  |FD + W| / A %.3e" % (a, b, fd, w, abs(fd + w) / A))
        assert abs(fd + w) <= 1e-6 * A, (a, b, fd, w, A)


def _abs_scale_fs(x, box, rc=2.5):
    """A = sum over pairs of |f/r| d2 = sum |f| r for the force-shifted LJ (eps = sigma = 1), pairs by a chunked brute
    search with the minimum image of the cubic box."""
    n = len(x)
    L = np.asarray(box)
    fc = 24.0 * (2.0 * rc ** -12 - rc ** -6) / rc
    tot = 0.0
    for i0 in range(0, n, 500):
        d = x[None, :, :] - x[i0:i0 + 500, None, :]
        d -= L * np.rint(d / L)
        r2 = (d * d).sum(axis=2)
        i = np.arange(i0, min(i0 + 500, n))[:, None]
        m = (r2 < rc * rc) & (np.arange(n)[None, :] > i)
        r = np.sqrt(r2[m])
        f = 24.0 * (2.0 * r ** -12 - r ** -6) / r - fc
        tot += float(np.sum(np.abs(f) * r))
    return tot


def _channels(sig, d):
    if d == 3:
        return np.array([sig[3], sig[4], sig[5], (sig[0] - sig[1]) * 0.5, (sig[1] - sig[2]) * 0.5,
                         ((sig[0] + sig[1]) + sig[2]) / 3.0])
    return np.array([sig[2], (sig[0] - sig[1]) * 0.5, (sig[0] + sig[1]) / 2.0])


def test_ring_bit_for_bit():
    s = lj_system(4000)
    nlags, nsmp = 4, 7
    with _device(s) as dev:
        dev.stress_setup(nlags)
        frames = []
        for _ in range(nsmp):
            dev.run(5, 0.002)
            dev.stress_sample()
            frames.append(dev.stress_tensor())
        ns, sk, sv, ncorr, corr = dev.stress_read()
        # the restatement: float64, the stated order, product rounded then added
        rk, rv = np.zeros(6), np.zeros(6)
        rc, rn = np.zeros((nlags, 6)), np.zeros(nlags, dtype=np.int64)
        ring = np.zeros((nlags, 6))
        for m, (kin, vir) in enumerate(frames):
            rk = rk + kin
            rv = rv + vir
            ch = _channels(kin + vir, 3)
            ring[m % nlags] = ch
            for k in range(0, min(m, nlags - 1) + 1):
                rc[k] = rc[k] + ch * ring[(m - k) % nlags]
                rn[k] += 1
        assert ns == nsmp and np.array_equal(ncorr, rn) and list(rn) == [7, 6, 5, 4]
        assert np.array_equal(sk, rk) and np.array_equal(sv, rv)
        assert np.array_equal(corr, rc)
        assert np.all(corr[0, :5] > 0.0)
        # after a reset the ring is empty: the next sample contributes to lag 0 only
        dev.stress_reset()
        ns, sk, sv, ncorr, corr = dev.stress_read()
        assert ns == 0 and not sk.any() and not sv.any() and not corr.any() and not ncorr.any()
        dev.stress_sample()
        kin, vir = dev.stress_tensor()
        assert np.array_equal(kin, frames[-1][0]) and np.array_equal(vir, frames[-1][1])   # the same frame, the same bits
        ns, sk, sv, ncorr, corr = dev.stress_read()
        ch = _channels(kin + vir, 3)
        assert ns == 1 and list(ncorr) == [1, 0, 0, 0]
        assert np.array_equal(sk, kin) and np.array_equal(sv, vir)
        assert np.array_equal(corr[0], ch * ch) and not corr[1:].any()
        # setup again starts over, nlags = 0 keeps the tensor and the means only
        dev.stress_setup(0)
        dev.stress_sample()
        ns, sk, sv, ncorr, corr = dev.stress_read()
        assert ns == 1 and ncorr.shape == (0,) and corr.shape == (0, 6) and np.array_equal(sk, kin)


@pytest.mark.parametrize("first,switch", [(False, None), (True, None), (False, "MDHIP_NO_FUSED_STEP"),
                                          (True, "MDHIP_NO_FUSED_STEP")])
def test_a_sample_changes_nothing(monkeypatch, first, switch):
    if switch:
        monkeypatch.setenv(switch, "1")
    s = lj_system(4000)
    out = []
    for sample in (False, True):
        with _device(s) as dev:
            if sample:
                dev.stress_setup(3)
                if first:
                    dev.stress_sample()                 # the first call after upload: the list-invalid path
            r1 = dev.run(40, 0.002)
            if sample:
                dev.stress_sample()
            r2 = dev.run(40, 0.002)
            if sample:
                dev.stress_sample()
            out.append((r1, r2, dev.download(), dev.stats()["fused"]))
    (a1, a2, da, fa), (b1, b2, db, fb) = out
    assert fa == fb and (fa == 0 or not switch)
    assert a1 == b1 and a2 == b2
    for u, w in zip(da, db):
        assert np.array_equal(u, w)


def test_potential_change_after_setup():
    """The sampler dispatches on the potential in force at sample time."""
    s = lj_system(4000)
    with _device(s) as dev:
        dev.stress_setup(0)
        dev.stress_sample()
        _, vir_lj = dev.stress_tensor()
        _, w_lj = dev.compute_forces()
        dev.set_potential(3, LJ_FS)
        dev.stress_sample()
        _, vir_fs = dev.stress_tensor()
        _, w_fs = dev.compute_forces()
    assert w_lj != w_fs
    for vir, w in ((vir_lj, w_lj), (vir_fs, w_fs)):
        assert abs(((vir[0] + vir[1]) + vir[2]) - w) <= 1e-11 * abs(w)


def _files(path):
    return {f: open(os.path.join(path, f), "rb").read() for f in ("thermo.txt", "trajectory.xyz")}


def test_run_simulation_integration(tmp_path):
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
    stress = md.StressTensor(10, nlags=3)
    md.run_simulation(sa, params, ensemble, 31, 10, pa, stress=stress)
    md.run_simulation(sb, params, ensemble, 31, 10, pb)
    assert stress.nsamples == 4 and list(stress.ncorr) == [4, 3, 2]
    assert _files(pa) == _files(pb)
    assert np.array_equal(np.asarray(sa.system.positions), np.asarray(sb.system.positions))
    assert np.array_equal(np.asarray(sa.velocities), np.asarray(sb.velocities))
    lines = open(os.path.join(pa, "stress.txt")).read().splitlines()
    assert lines[0] == "# component kinetic virial pressure" and len(lines) == 8 and lines[-1] == "# nsamples 4"
    lines = open(os.path.join(pa, "stress_acf.txt")).read().splitlines()
    assert lines[0].startswith("# lag time C_shear") and len(lines) == 4
    assert not os.path.exists(os.path.join(pb, "stress.txt"))
    # the thermo line's pressure is the trace of the tensor (no tail correction on this potential)
    V = n / 0.8
    assert stress.volume == pytest.approx(V, rel=1e-12)
    thermo = [ln.split() for ln in open(os.path.join(pa, "thermo.txt")).read().splitlines()[1:]]
    assert stress.temperature() == pytest.approx(np.mean([float(r[2]) for r in thermo]), rel=1e-5)
    p_thermo = np.mean([float(r[3]) for r in thermo])
    # (thermo uses rho T with T = 2K/nf: the kinetic parts differ by the factor N / (N - 1))
    assert stress.pressure() == pytest.approx(p_thermo, rel=1e-3)
    # the one-shot twin: the final state's tensor, its trace the W the handle reports
    K, W = md.compute_stress(sa, params)
    assert K.shape == (3, 3) and W.shape == (3, 3) and np.array_equal(W, W.T)
    _, w = sa.system.device.compute_forces()
    assert abs(np.trace(W) - w) <= 1e-11 * abs(w)
    assert np.trace(K) == pytest.approx(float((np.asarray(sa.velocities) ** 2).sum()), rel=1e-12)
    for st in (sa, sb):
        st.system.device.close()


def test_errors():
    from moleculardynamics.jl_amd import MDDevice, MdhipError, _lib
    from tests.test_gpu_parity import USER_LJ_SRC
    with MDDevice(3, 1000, 12.0, 2.5) as dev:
        for call in (dev.stress_sample, dev.stress_read, dev.stress_reset, dev.stress_tensor):
            with pytest.raises(MdhipError, match="no setup"):
                call()
        for bad in (-1, 65537):
            with pytest.raises(MdhipError, match="nlags must be in 0..65536"):
                dev.stress_setup(bad)
        with pytest.raises(MdhipError, match="no setup"):   # a refused setup leaves no sampler behind
            dev.stress_sample()
        dev.stress_setup(65536)                            # the limits themselves are accepted
        dev.stress_setup(0)
        with pytest.raises(MdhipError, match="no frame sampled"):
            dev.stress_tensor()
        dev.stress_read()
        dev.set_potential_source(USER_LJ_SRC, "user_lj", [1.0, 2.5])
        with pytest.raises(MdhipError, match="MD_POT_CUSTOM"):
            dev.stress_sample()
        with pytest.raises(MdhipError, match="MD_POT_CUSTOM"):
            dev.stress_setup(4)
    lib = _lib.load()
    h = ctypes.c_void_p()
    n = 4000
    box = (ctypes.c_double * 9)(20, 0, 0, 0, 20, 0, 0, 0, 20)
    assert lib.md_create_domain(3, n, n, box, 2.5, -1, 0, 1, ctypes.byref(h)) == 0, lib.md_last_error(None)
    try:
        assert lib.md_stress_setup(h, 4) != 0
        assert b"slab" in lib.md_last_error(h)
        for fn in (lib.md_stress_sample, lib.md_stress_reset):
            assert fn(h) != 0
            assert b"slab" in lib.md_last_error(h)
    finally:
        lib.md_destroy(h)
