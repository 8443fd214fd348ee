"""-m gpu: the HIP path (through the C ABI) against the CPU oracle on identical inputs.

Tolerances (stated, fp64):
  neighbour pair set            bit-exact (identical after canonical sort)
  per-particle force            |dF|_inf <= 1e-11 * max(1, |F|_inf)
  U, W                          relative 1e-12 (vs the oracle's serial / cell-ordered sum)
  10-step trajectory positions  1e-10 absolute
The built-in LJ runs in r^-2 form on the device (no sqrt); the oracle uses the reference's
sigma/r form -- the difference is a few ulp, inside these tolerances.

Decisions are the reference's, bit for bit: a pair is accepted iff d2 <= list_cutoff^2 and LJ contributes iff
sqrt(d2) < r_cut, with d2 = (dx*dx + dy*dy) + dz*dz rounded operation by operation (no fma).
The device's fast kernels classify on the high dword of an fma chain and re-decide every candidate within 2^-20 of
the threshold on the reference form (test_cutoff_decisions_follow_reference_arithmetic).

Stated deviations of the device arithmetic from the reference's (all inside the tolerances above):
  * values, not decisions, use fma: d2 in the LJ r^-2 polynomial, the force accumulation F += fpr*d;
  * LJ in r^-2 form with v_rcp_f64 + one Newton step (2e-15 relative) instead of sigma/r, sqrt and division;
  * full-neighbour sums in row order instead of the reference's half-shell traversal order (U, W halved);
  * the periodic wrap x <- L*(x/L - floor(x/L)) (src/boundary.jl:9-15) is applied lazily -- at list builds and on
    download, only to coordinates outside [0, L) -- whereas the reference re-rounds every coordinate every step
    (src/integrate.jl:16); image counters are identical, positions agree to ~1 ulp of L per step;
  * Bussi's K is a tree sum over per-block partials instead of the serial sum of src/thermostat.jl:53-55.

Residual asymmetry across a periodic face (test_cross_face_threshold_dimers).  The reference visits a pair once; the
full-neighbour kernels evaluate it from both ends, and across a face the two ends hold different roundings of the same
separation -- from a's end the neighbour is b's translated image, fl(fl(x_b + s L) - x_a), from b's end it is a's,
fl(fl(x_a - s L) - x_b); x + L rounds at ulp(L)/2, so the two d2 differ by up to ~2 r ulp(L) (~40 ulp of d2 at
L = 105).  The exported pair set and the smaller-index end follow the oracle's form (the larger index is the translated
one) bit for bit; the other end decides on its own form.  A pair is therefore counted from one end only iff its d2
falls inside that window: per step about N * (2 pi r_c rho) * |delta d2| * (fraction of pairs that cross a face)
= 1e6 * 14 * 3.5e-14 * 0.07 ~ 3e-8 at the metric's configuration -- one pair in ~3e7 steps, each time an error of
|F(r_c)| = 0.039 on one particle (LJ is discontinuous there in the reference as well).  Stated, not removed: both ends
agreeing would need the pair's index order inside the pair loop.
"""
import ctypes as C

import numpy as np
import pytest

from tests.util import lj_system, poly_system

pytestmark = pytest.mark.gpu

LJ = [1.0, 1.0, 2.5]


def _dev(sys_, cutoff, kind=0, params=LJ, skin=None):
    from moleculardynamics.jl_amd import MDDevice
    d = MDDevice(sys_["dim"], sys_["n"], sys_["box"], cutoff)
    d.set_potential(kind, params)
    if skin is not None:
        d.set_skin(skin)
    d.upload(sys_["x"], sys_["v"], sys_["f"], sys_["img"], sys_["diam"])
    return d


def _check_forces(f_gpu, f_ref, tol=1e-11):
    scale = max(1.0, np.abs(f_ref).max())
    err = np.abs(f_gpu - f_ref).max()
    assert err <= tol * scale, f"force error {err:.3e} > {tol * scale:.3e}"


@pytest.mark.parametrize("n,permute", [(1024, None), (4096, None), (4096, 777)])
def test_forces_energy_pairs_vs_bruteforce(oracle, n, permute):
    s = lj_system(n, permute=permute)
    pot = oracle.make_pot(oracle.POT_LJ, LJ)
    f_ref, u_ref, w_ref, pairs_ref = oracle.forces_brute(s["x"], s["box"], 2.5, pot, s["diam"], want_pairs=True)
    with _dev(s, 2.5) as d:
        u, w = d.compute_forces()
        _, _, f, _ = d.download()
        pairs = d.neighbor_pairs()
    pr = pairs_ref[np.lexsort((pairs_ref[:, 1], pairs_ref[:, 0]))]
    assert pairs.shape == pr.shape and np.array_equal(pairs, pr), "neighbour pair set differs"
    _check_forces(f, f_ref)
    assert abs(u - u_ref) <= 1e-12 * abs(u_ref)
    assert abs(w - w_ref) <= 1e-12 * abs(w_ref)


def test_default_cutoff_1p5(oracle):
    """list cutoff 1.5 with LJ r_cut 2.5 -> effective cutoff 1.5."""
    s = lj_system(2048)
    pot = oracle.make_pot(oracle.POT_LJ, LJ)
    f_ref, u_ref, w_ref, pairs_ref = oracle.forces_brute(s["x"], s["box"], 1.5, pot, s["diam"], want_pairs=True)
    with _dev(s, 1.5) as d:
        u, w = d.compute_forces()
        _, _, f, _ = d.download()
        pairs = d.neighbor_pairs()
    pr = pairs_ref[np.lexsort((pairs_ref[:, 1], pairs_ref[:, 0]))]
    assert np.array_equal(pairs, pr)
    _check_forces(f, f_ref)
    assert abs(u - u_ref) <= 1e-12 * abs(u_ref)
    assert abs(w - w_ref) <= 1e-12 * abs(w_ref)


@pytest.mark.parametrize("skin", [0.0, 0.3])
def test_nve_trajectory_10_steps(oracle, skin):
    s = lj_system(4096)
    pot = oracle.make_pot(oracle.POT_LJ, LJ)
    ref = oracle.run(s["x"], s["img"], s["v"], s["f"], s["diam"], s["box"], 2.5, pot, 0.001, 10, use_cells=True,
                     nthreads=1)
    with _dev(s, 2.5, skin=skin) as d:
        U, W, K = d.run(10, 0.001)
        x, v, f, img = d.download()
    assert np.abs(x - ref["x"]).max() <= 1e-10
    assert np.abs(v - ref["v"]).max() <= 1e-10
    _check_forces(f, ref["f"], 1e-10)
    assert np.array_equal(img, ref["img"])
    assert abs(U - ref["U"]) <= 1e-11 * abs(ref["U"])
    assert abs(W - ref["W"]) <= 1e-10 * abs(ref["W"])
    assert abs(K - ref["K"]) <= 1e-12 * abs(ref["K"])


def test_first_step_uses_uploaded_forces(oracle):
    """forces start at whatever the state holds (zeros) and persist."""
    s = lj_system(1024)
    pot = oracle.make_pot(oracle.POT_LJ, LJ)
    ref1 = oracle.run(s["x"], s["img"], s["v"], s["f"], s["diam"], s["box"], 2.5, pot, 0.001, 3, use_cells=False)
    ref2 = oracle.run(ref1["x"], ref1["img"], ref1["v"], ref1["f"], s["diam"], s["box"], 2.5, pot, 0.001, 3,
                      use_cells=False)
    with _dev(s, 2.5) as d:
        d.run(3, 0.001)
        d.run(3, 0.001)
        x, v, f, img = d.download()
    assert np.abs(x - ref2["x"]).max() <= 1e-10
    assert np.abs(v - ref2["v"]).max() <= 1e-10


def test_nvt_bussi_injected_noise(oracle):
    from moleculardynamics.jl_amd import _lib
    s = lj_system(4096, kT=1.4737)
    pot = oracle.make_pot(oracle.POT_LJ, LJ)
    nsteps = 12
    rng = np.random.default_rng(5)
    nf = 3 * (s["n"] - 1.0)
    r1 = rng.standard_normal(nsteps)
    r2 = 2.0 * rng.gamma((nf - 1) / 2, size=nsteps)
    kt = np.full(nsteps, 1.4737)
    ref = oracle.run(s["x"], s["img"], s["v"], s["f"], s["diam"], s["box"], 2.5, pot, 0.001, nsteps, ensemble=1,
                     tau=0.1, ktemp=kt, r1=r1, r2=r2, use_cells=True, nthreads=1)
    with _dev(s, 2.5) as d:
        U, W, K = d.run(nsteps, 0.001, _lib.MD_NVT, 0.1, nf, kt, r1, r2)
        x, v, f, img = d.download()
    assert np.abs(x - ref["x"]).max() <= 1e-10
    assert np.abs(v - ref["v"]).max() <= 1e-10
    assert abs(K - ref["K"]) <= 1e-11 * abs(ref["K"])
    assert abs(U - ref["U"]) <= 1e-11 * abs(ref["U"])


def test_wrap_and_images(oracle):
    """Fast particles cross the periodic faces: wrapped positions and image counters must match."""
    s = lj_system(1024, kT=8.0)
    pot = oracle.make_pot(oracle.POT_LJ, LJ)
    ref = oracle.run(s["x"], s["img"], s["v"], s["f"], s["diam"], s["box"], 2.5, pot, 0.001, 150, use_cells=False)
    assert np.abs(ref["img"]).max() >= 1 and np.count_nonzero(ref["img"]) >= 10
    with _dev(s, 2.5) as d:
        d.run(150, 0.001)
        x, v, f, img = d.download()
    assert np.array_equal(img, ref["img"])
    assert np.abs(x - ref["x"]).max() <= 1e-9


def test_pseudohs(oracle):
    s = lj_system(2048, rho=0.8976)
    pot = oracle.make_pot(oracle.POT_PSEUDOHS, [50.0])
    f_ref, u_ref, w_ref, _ = oracle.forces_brute(s["x"], s["box"], 1.5, pot, s["diam"])
    with _dev(s, 1.5, kind=1, params=[50.0]) as d:
        u, w = d.compute_forces()
        _, _, f, _ = d.download()
    _check_forces(f, f_ref, 1e-10)
    assert abs(u - u_ref) <= 1e-10 * max(1.0, abs(u_ref))
    assert abs(w - w_ref) <= 1e-10 * max(1.0, abs(w_ref))


def test_polydisperse_2d(oracle):
    s = poly_system()
    cutoff = 1.25 * 1.2
    pot = oracle.make_pot(oracle.POT_POLYDISPERSE, [1.25, 0.2])
    f_ref, u_ref, w_ref, pairs_ref = oracle.forces_brute(s["x"], s["box"], cutoff, pot, s["diam"], want_pairs=True)
    with _dev(s, cutoff, kind=2, params=[1.25, 0.2]) as d:
        u, w = d.compute_forces()
        _, _, f, _ = d.download()
        pairs = d.neighbor_pairs()
        pr = pairs_ref[np.lexsort((pairs_ref[:, 1], pairs_ref[:, 0]))]
        assert np.array_equal(pairs, pr)
        _check_forces(f, f_ref)
        assert abs(u - u_ref) <= 1e-12 * abs(u_ref)
        assert abs(w - w_ref) <= 1e-12 * abs(w_ref)
        ref = oracle.run(s["x"], s["img"], s["v"], s["f"], s["diam"], s["box"], cutoff, pot, 0.005, 20,
                         use_cells=False)
        d.upload(s["x"], s["v"], s["f"], s["img"], s["diam"])
        d.run(20, 0.005)
        x, v, _, img = d.download()
    assert np.abs(x - ref["x"]).max() <= 1e-10
    assert np.abs(v - ref["v"]).max() <= 1e-10


# ---------------------------------------------------------------- committed golden vectors
import os  # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.mark.parametrize("name,n", [("lj_n512_rc2p5.npz", 512), ("lj_n500_rc1p5.npz", 500)])
def test_device_vs_golden_lj(name, n):
    g = np.load(os.path.join(GOLD, name))
    s = lj_system(n)
    cutoff = float(g["cutoff"])
    with _dev(s, cutoff) as d:
        u, w = d.compute_forces()
        _, _, f, _ = d.download()
        pairs = d.neighbor_pairs()
        assert np.array_equal(pairs, g["pairs"])
        _check_forces(f, g["forces"])
        assert abs(u - float(g["U"])) <= 1e-12 * abs(float(g["U"]))
        assert abs(w - float(g["W"])) <= 1e-12 * abs(float(g["W"]))
        d.upload(s["x"], s["v"], s["f"], s["img"], s["diam"])
        U, W, K = d.run(int(g["nsteps"]), float(g["dt"]))
        x, v, f, img = d.download()
    assert np.abs(x - g["x_end"]).max() <= 1e-10 and np.abs(v - g["v_end"]).max() <= 1e-10
    assert np.array_equal(img, g["img_end"])
    assert abs(K - float(g["K_end"])) <= 1e-12 * float(g["K_end"])


def test_device_vs_golden_nvt():
    from moleculardynamics.jl_amd import _lib
    g = np.load(os.path.join(GOLD, "lj_n512_nvt.npz"))
    s = lj_system(512, kT=1.4737)
    with _dev(s, 2.5) as d:
        U, W, K = d.run(int(g["nsteps"]), float(g["dt"]), _lib.MD_NVT, 0.1, 3 * 511.0, g["kt"], g["r1"], g["r2"])
        x, v, _, _ = d.download()
    assert np.abs(x - g["x_end"]).max() <= 1e-10 and np.abs(v - g["v_end"]).max() <= 1e-10
    assert abs(K - float(g["K_end"])) <= 1e-11 * float(g["K_end"])


# ---------------------------------------------------------------- full-size, size-independent properties
@pytest.mark.parametrize("n", [262144, 1048576])
def test_full_size_properties(n):
    """BASELINE configs[1] / [2] sizes: too big for the O(N^2) oracle, so check what must hold at
    any size: sum F = 0, the lattice energy, and that every list strategy (fresh cells each step,
    Verlet rows with a skin, fused fp32 tile build, two-kernel fp64 build, global-gather kernel)
    yields the same forces -- bit-identical on one cell grid, where they differ only in which
    rejected candidates they carry."""
    from moleculardynamics.jl_amd import MDDevice
    s = lj_system(n)
    results = []
    for env, skin in [({}, 0.3), ({}, 0.0), ({"MDHIP_NO_FUSED_BUILD": "1"}, 0.3), ({"MDHIP_NO_TILES": "1"}, 0.3)]:
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            with MDDevice(3, n, s["box"], 2.5) as d:
                d.set_potential(0, LJ)
                d.set_skin(skin)
                d.upload(s["x"], s["v"], s["f"], s["img"], s["diam"])
                u, w = d.compute_forces()
                _, _, f, _ = d.download()
                st = d.stats()
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
        results.append((f, u, w, st))
    f0, u0, w0, st0 = results[0]
    assert st0["tiled"] == 1
    assert np.abs(f0.sum(axis=0)).max() <= 1e-9 * np.abs(f0).sum()          # Newton's third law
    assert -4.6 < u0 / n < -4.1      # jittered simple-cubic start at rho=0.897 (oracle at N=4096: -4.385)
    # same cell grid (same skin): same candidates order -> bitwise; skin 0 uses a different grid,
    # hence a different summation order -> round-off level
    for i, (f, u, w, st) in enumerate(results[1:], start=1):
        if i == 1:
            _check_forces(f, f0, 1e-12)
        else:
            assert np.array_equal(f, f0), "list strategies on one grid disagree bitwise"
        assert abs(u - u0) <= 1e-13 * abs(u0) and abs(w - w0) <= 1e-13 * abs(w0)
    assert results[3][3]["tiled"] == 0


@pytest.mark.parametrize("n", [262144, 1048576])
def test_full_size_vs_oracle_cells(oracle, n):
    """BASELINE configs[1] / [2] sizes against the oracle's O(N) linked-cell path (8 OpenMP threads): forces,
    energy, virial and the NUMBER of accepted pairs (the pair set itself is compared bit-exactly at 262144)."""
    from moleculardynamics.jl_amd import MDDevice
    s = lj_system(n, permute=777)
    pot = oracle.make_pot(0, LJ)
    f_ref, u_ref, w_ref, npairs = oracle.forces_cells(s["x"], s["box"], 2.5, pot, s["diam"], nthreads=8)
    with MDDevice(3, n, s["box"], 2.5) as d:
        d.set_potential(0, LJ)
        d.upload(s["x"], s["v"], s["f"], s["img"], s["diam"])
        u, w = d.compute_forces()
        _, _, f, _ = d.download()
        cnt = C.c_int64()
        d._chk(d._L.md_neighbor_pairs(d._h, None, 0, C.byref(cnt)))
        pairs = d.neighbor_pairs() if n <= 262144 else None
    _check_forces(f, f_ref, 1e-11)
    assert abs(u - u_ref) <= 1e-12 * abs(u_ref) and abs(w - w_ref) <= 1e-12 * abs(w_ref)
    assert cnt.value == npairs
    if pairs is not None:
        assert np.array_equal(pairs, oracle.pairs_cells(s["x"], s["box"], 2.5))


def test_config4_4m_particles_on_one_gpu(oracle):
    """BASELINE configs[3]: N = 4,194,304, rho = 0.897 (L = 167.22), NVE -- the whole system on ONE handle (~8 GB):
    forces / U / W / accepted-pair count against the oracle's linked-cell path, Newton's third law, and 40 NVE steps
    (fused step loop, prune steps and at least the initial list build at this size) against oracle.run.  (Round 2 ran 12
    steps and the first half of round 3 20, at 14 s per oracle evaluation: the oracle was running one OpenMP thread per
    HOST core -- 256 -- inside a 16-CPU quota, oracle.default_threads; it is 0.6 s now.)"""
    from moleculardynamics.jl_amd import MDDevice
    n, nsteps, dt = 4194304, 40, 0.001
    s = lj_system(n)
    assert abs(s["box"][0] - 167.2204) < 1e-3
    pot = oracle.make_pot(0, LJ)
    f_ref, u_ref, w_ref, npairs = oracle.forces_cells(s["x"], s["box"], 2.5, pot, s["diam"], nthreads=0)
    ref = oracle.run(s["x"], s["img"], s["v"], s["f"], s["diam"], s["box"], 2.5, pot, dt, nsteps, nthreads=0)
    with MDDevice(3, n, s["box"], 2.5) as d:
        d.set_potential(0, LJ)
        d.upload(s["x"], s["v"], s["f"], s["img"], s["diam"])
        u, w = d.compute_forces()
        _, _, f, _ = d.download()
        cnt = C.c_int64()
        d._chk(d._L.md_neighbor_pairs(d._h, None, 0, C.byref(cnt)))
        assert d.stats()["tiled"] == 1
        d.upload(s["x"], s["v"], s["f"], s["img"], s["diam"])     # zero forces again: the first half-kick uses them (D7)
        U, W, K = d.run(nsteps, dt)
        x, v, f2, img = d.download()
        st = d.stats()
    _check_forces(f, f_ref, 1e-11)
    assert abs(u - u_ref) <= 1e-12 * abs(u_ref) and abs(w - w_ref) <= 1e-12 * abs(w_ref)
    assert cnt.value == npairs
    assert np.abs(f.sum(axis=0)).max() <= 1e-9 * np.abs(f).sum()
    assert np.abs(x - ref["x"]).max() <= 1e-10 and np.abs(v - ref["v"]).max() <= 1e-10
    assert np.array_equal(img, ref["img"])
    _check_forces(f2, ref["f"], 1e-10)
    assert abs(U - ref["U"]) <= 1e-11 * abs(ref["U"]) and abs(K - ref["K"]) <= 1e-12 * abs(ref["K"])
    assert st["prunes"] >= 1 and st["steps"] == nsteps


def test_config3_1m_nvt_end_to_end(oracle):
    """BASELINE configs[2], the configuration the metric is quoted on, end to end: N = 1,048,576, rho = 0.897, NVT
    (Bussi, tau = 0.1, kT = 1.4737), dt = 0.001 -- 80 steps of the fused step loop (list build, prune steps, a list
    REBUILD inside the run, the thermostat's rescale folded into the next step) with injected draws (r1, r2) against oracle.run with the same
    draws: positions, velocities, images, forces, K and U."""
    from moleculardynamics.jl_amd import MDDevice, _lib
    from moleculardynamics.jl_amd.thermostat import draw_bussi
    n, nsteps, dt, tau, kT = 1048576, 80, 0.001, 0.1, 1.4737      # (80 steps: past the first list REBUILD inside the run)
    s = lj_system(n, kT=kT)
    assert abs(s["box"][0] - 105.3422) < 1e-3
    nf = 3.0 * (n - 1.0)
    r1, r2 = draw_bussi(nf, np.random.default_rng(4242), nsteps)
    kt = np.full(nsteps, kT)
    pot = oracle.make_pot(0, LJ)
    ref = oracle.run(s["x"], s["img"], s["v"], s["f"], s["diam"], s["box"], 2.5, pot, dt, nsteps, ensemble=1, tau=tau,
                     ktemp=kt, r1=r1, r2=r2, nthreads=0)
    with MDDevice(3, n, s["box"], 2.5) as d:
        d.set_potential(0, LJ)
        d.upload(s["x"], s["v"], s["f"], s["img"], s["diam"])
        U, W, K = d.run(nsteps, dt, _lib.MD_NVT, tau, nf, kt, r1, r2)
        x, v, f, img = d.download()
        st = d.stats()
    assert st["fused"] == 1 and st["prunes"] >= 3 and st["steps"] == nsteps
    assert st["rebuilds"] >= 2, "the run was meant to contain a list rebuild"
    assert np.abs(x - ref["x"]).max() <= 1e-10 and np.abs(v - ref["v"]).max() <= 1e-10
    assert np.array_equal(img, ref["img"])
    _check_forces(f, ref["f"], 1e-10)
    assert abs(U - ref["U"]) <= 1e-11 * abs(ref["U"]) and abs(K - ref["K"]) <= 1e-12 * abs(ref["K"])
    assert abs(W - ref["W"]) <= 1e-11 * abs(ref["W"])


def test_many_list_cycles_262k_nvt(oracle):
    """BASELINE configs[1]'s size over several complete list cycles: 262,144 particles, NVT, 240 steps -- four or more list
    rebuilds and a dozen prune steps, the planner adapting its window lengths -- against oracle.run (which rebuilds its
    cells every step, as the reference does) with the same thermostat draws.  What the short end-to-end runs cannot show:
    that nothing drifts from one list generation to the next."""
    from moleculardynamics.jl_amd import MDDevice, _lib
    from moleculardynamics.jl_amd.thermostat import draw_bussi
    n, nsteps, dt, tau, kT = 262144, 240, 0.001, 0.1, 1.4737
    s = lj_system(n, kT=kT)
    nf = 3.0 * (n - 1.0)
    r1, r2 = draw_bussi(nf, np.random.default_rng(99), nsteps)
    kt = np.full(nsteps, kT)
    pot = oracle.make_pot(0, LJ)
    ref = oracle.run(s["x"], s["img"], s["v"], s["f"], s["diam"], s["box"], 2.5, pot, dt, nsteps, ensemble=1, tau=tau,
                     ktemp=kt, r1=r1, r2=r2, nthreads=0)
    with MDDevice(3, n, s["box"], 2.5) as d:
        d.set_potential(0, LJ)
        d.upload(s["x"], s["v"], s["f"], s["img"], s["diam"])
        U, W, K = d.run(nsteps, dt, _lib.MD_NVT, tau, nf, kt, r1, r2)
        x, v, f, img = d.download()
        st = d.stats()
    assert st["fused"] == 1 and st["rebuilds"] >= 4 and st["prunes"] >= 10 and st["steps"] == nsteps
    assert np.array_equal(img, ref["img"])
    assert np.abs(x - ref["x"]).max() <= 1e-9 and np.abs(v - ref["v"]).max() <= 1e-9
    _check_forces(f, ref["f"], 1e-9)
    assert abs(U - ref["U"]) <= 1e-10 * abs(ref["U"]) and abs(K - ref["K"]) <= 1e-11 * abs(ref["K"])


def test_nve_energy_drift_matches_oracle_262k(oracle):
    """north_star: "energy drift within CPU-reference tolerance".  40 NVE steps at N=262144 on both sides from the
    same start: the total energy changes by the same amount (the drift is the truncated potential's, not the
    device's), and the end states agree."""
    from moleculardynamics.jl_amd import MDDevice
    n, nsteps, dt = 262144, 40, 0.001
    s = lj_system(n)
    pot = oracle.make_pot(0, LJ)
    f0, u0, _, _ = oracle.forces_cells(s["x"], s["box"], 2.5, pot, s["diam"], nthreads=8)
    k0 = oracle.kinetic(s["v"])
    ref = oracle.run(s["x"], s["img"], s["v"], f0, s["diam"], s["box"], 2.5, pot, dt, nsteps, nthreads=8)
    with MDDevice(3, n, s["box"], 2.5) as d:
        d.set_potential(0, LJ)
        d.upload(s["x"], s["v"], f0, s["img"], s["diam"])
        U, W, K = d.run(nsteps, dt)
        x, v, f, img = d.download()
    e0 = u0 + k0
    drift_ref = (ref["U"] + ref["K"]) - e0
    drift_dev = (U + K) - e0
    assert abs(drift_dev - drift_ref) <= 1e-9 * abs(e0)
    assert abs(drift_ref) < 1e-2 * abs(e0)   # (the unshifted cutoff: -0.016 per pair that crosses r_c while the lattice melts)
    assert np.abs(x - ref["x"]).max() <= 1e-9 and np.abs(v - ref["v"]).max() <= 1e-9 and np.array_equal(img, ref["img"])


def test_nve_momentum_and_energy_262k():
    """BASELINE configs[1]: N=262144 NVE.  Total momentum stays at round-off, energy drift is at
    the level the truncated-unshifted potential allows."""
    from moleculardynamics.jl_amd import MDDevice
    n = 262144
    s = lj_system(n)
    with MDDevice(3, n, s["box"], 2.5) as d:
        d.set_potential(0, LJ)
        d.upload(s["x"], s["v"], s["f"], s["img"], s["diam"])
        U1, W1, K1 = d.run(20, 0.001)
        U2, W2, K2 = d.run(200, 0.001)
        _, v, _, _ = d.download()
        st = d.stats()
    assert np.abs(v.sum(axis=0)).max() < 1e-7
    assert abs((U2 + K2) - (U1 + K1)) < 2e-2 * abs(U1 + K1)
    assert st["rebuilds"] >= 2 and st["steps"] == 220


# ---------------------------------------------------------------- the driver, end to end (BASELINE configs[0])
@pytest.mark.parametrize("potname", ["lj", "pseudohs"])
def test_run_simulation_readme_example(tmp_path, potname):
    """README example 1 with the actual signatures: N=1024, packing fraction 0.47
    (rho = 0.8976), kT = 1.4737, NVT equilibration then NVE -- plumbing, file formats, D7."""
    import moleculardynamics.jl_amd as md
    rho = 6 * 0.47 / np.pi
    pot = md.LennardJones() if potname == "lj" else md.PseudoHS()
    cutoff = 2.5 if potname == "lj" else 1.5
    dt = 0.001 if potname == "lj" else 0.0005
    # BASELINE configs[0] is the LJ case at N = 1024; the pseudo-hard-sphere variant (README's state point)
    # uses N = 1000 = 10^3 so that the lattice start has no overlaps (1024 particles on an 11^3 lattice sit 0.95 apart)
    nn = 1024 if potname == "lj" else 1000
    params = md.Parameters(rho, nn, dt, pot)
    path = str(tmp_path / potname)
    if potname == "lj":
        state = md.initialize_state(params, path, random_init=True, cutoff=cutoff, rng=np.random.default_rng(7))
    else:
        # pseudo hard spheres must not start overlapping (the reference removes overlaps with Packmol):
        # 1 % jitter on the 1.037-spaced lattice keeps every pair beyond sigma
        L = (nn / rho) ** (1.0 / 3.0)
        x0 = md.lattice_positions(nn, np.full(3, L), 3, np.random.default_rng(7), jitter=0.01)
        state = md.initialize_state(params, path, cutoff=cutoff, positions=x0, diameters=np.ones(nn), unitcell=L)
    assert os.path.isfile(os.path.join(path, "init.xyz"))
    state.velocities = md.initialize_velocities(1.4737, np.random.default_rng(8), params.n_particles, 3)
    md.run_simulation(state, params, md.NVT(1.4737, 100.0 * dt), 60, 20, path, thermo_name="thermo_nvt.txt")
    f_after_first = state.system.energy_and_forces.forces.copy()
    assert np.abs(f_after_first).max() > 0           # forces persist on the state for the next call (D7)
    md.run_simulation(state, params, md.NVE(), 45, 20, path)
    lines = open(os.path.join(path, "thermo.txt")).read().splitlines()
    assert lines[0] == "# Step Energy Temperature Pressure"
    rows = [ln.split() for ln in lines[1:]]
    assert [int(r[0]) for r in rows] == [0, 20, 40]   # step % frequency == 0, 0-based
    assert all(len(r) == 4 and re_float.match(r[1]) for r in rows)
    T = [float(r[2]) for r in rows]
    # (N = 1024 fills 1024 of the 11^3 lattice sites: spacing 0.95 < 2^(1/6), the start is compressed and heats up;
    # the oracle gives T = 2.22, 2.86, 3.58 on these rows)
    assert all(0.5 < t < 5.0 for t in T)
    assert os.path.isfile(os.path.join(path, "final.xyz")) and os.path.isfile(os.path.join(path, "trajectory.xyz"))
    assert state.velocities.shape == (nn, 3) and state.images.dtype == np.int32
    state.system.device.close()


@pytest.mark.parametrize("mode,ron", [(0, 0.0), (1, 0.0), (2, 2.0)])
def test_modified_lj_kinds(oracle, mode, ron):
    """MD_POT_LJ_MODIFIED (shifted / force-shifted / XPLOR) against the oracle, with
    per-particle diameters; and the point of a force-shifted potential: NVE energy is conserved far better
    than with the truncated one."""
    from moleculardynamics.jl_amd import MDDevice
    n = 1000
    s = lj_system(n, kT=1.0)
    rng = np.random.default_rng(11)
    diam = rng.uniform(0.9, 1.1, n)
    params = [1.0, 1.0, 2.5, float(mode), ron]
    pot = oracle.make_pot(oracle.POT_LJ_MODIFIED, params)
    f_ref, u_ref, w_ref, pairs_ref = oracle.forces_brute(s["x"], s["box"], 2.5, pot, diam, want_pairs=True)
    with MDDevice(3, n, s["box"], 2.5) as d:
        d.set_potential(3, params)
        d.upload(s["x"], s["v"], s["f"], s["img"], diam)
        u, w = d.compute_forces()
        _, _, f, _ = d.download()
        _check_forces(f, f_ref, 1e-11)
        assert abs(u - u_ref) <= 1e-12 * abs(u_ref) and abs(w - w_ref) <= 1e-12 * abs(w_ref)
        ref = oracle.run(s["x"], s["img"], s["v"], f_ref, diam, s["box"], 2.5, pot, 0.001, 10, use_cells=False)
        U, W, K = d.run(10, 0.001)
        x, v, _, _ = d.download()
        assert np.abs(x - ref["x"]).max() <= 1e-10 and np.abs(v - ref["v"]).max() <= 1e-10
        if mode == 1:
            e0 = U + K
            U2, _, K2 = d.run(400, 0.001)
            assert abs((U2 + K2) - e0) <= 1e-3 * abs(e0)      # (velocity-Verlet fluctuation while the lattice melts)


def test_run_simulation_log_snapshots_and_zstd(tmp_path, monkeypatch):
    """The output path either side of the step loop: LAMMPS frames at `frequency`
    cadence, log-spaced snapshot files (src/simulation.jl:153-171), zstd post-compression of the trajectory
    (src/simulation.jl:11-36), all written by the background writer."""
    import pyarrow as pa
    import moleculardynamics.jl_amd as md
    monkeypatch.chdir(tmp_path)                       # generate_log_times writes new-log-times.txt into the cwd
    params = md.Parameters(0.8, 512, 0.001, md.LennardJones())
    path = str(tmp_path / "out")
    state = md.initialize_state(params, path, random_init=True, cutoff=2.5, rng=np.random.default_rng(5))
    state.velocities = md.initialize_velocities(1.0, np.random.default_rng(6), 512, 3)
    md.run_simulation(state, params, md.NVE(), 30, 10, path, compress=True, log_times=True)
    # floor(1.35^i), i = 0..40, below 30: 1 2 3 4 6 8 11 14 20 27  (+ step 0)
    snaps = sorted(int(f.split(".")[1]) for f in os.listdir(path) if f.startswith("snapshot."))
    assert snaps == [0, 1, 2, 3, 4, 6, 8, 11, 14, 20, 27]
    assert os.path.isfile(tmp_path / "new-log-times.txt")
    first = open(os.path.join(path, "snapshot.6")).read().splitlines()
    assert first[0] == "ITEM: TIMESTEP" and first[1] == "6" and first[3] == "512"
    assert not os.path.exists(os.path.join(path, "trajectory.xyz"))
    raw = pa.CompressedInputStream(os.path.join(path, "trajectory.xyz.zst"), "zstd").read().decode()
    assert raw.count("ITEM: TIMESTEP") == 3           # steps 0, 10, 20
    rows = open(os.path.join(path, "thermo.txt")).read().splitlines()
    assert [int(r.split()[0]) for r in rows[1:]] == [0, 10, 20]
    state.system.device.close()


import re  # noqa: E402
re_float = re.compile(r"^-?\d+\.\d{6}$")


# ---------------------------------------------------------------- user potential compiled at run time (plugin API)
USER_LJ_SRC = r"""
// evaluate(pot, r, sigma1, sigma2) -> (u, f), f = -dU/dr : the reference's plugin contract (src/pairwise.jl:31)
__device__ void user_lj(double r, double s1, double s2, const double* p, double* u, double* f)
{
    double eps = p[0], rcut = p[1];
    double sigma = (s1 + s2) / 2.0;
    if (r >= rcut) { *u = 0.0; *f = 0.0; return; }
    double sr = sigma / r, sr2 = sr * sr, sr6 = sr2 * sr2 * sr2, sr12 = sr6 * sr6;
    *u = 4.0 * eps * (sr12 - sr6);
    *f = 24.0 * eps * (2.0 * sr12 - sr6) / r;
}
"""


def test_user_potential_source(oracle):
    """A Potential subtype that describes itself by HIP source runs through the same kernels as the
    built-ins (hiprtc) and must reproduce the oracle; a broken source must fail loudly with the log."""
    import moleculardynamics.jl_amd as md
    from moleculardynamics.jl_amd import MDDevice

    s = lj_system(4096)
    s["diam"] = np.random.default_rng(3).uniform(0.9, 1.1, s["n"])   # per-pair sigma goes through the plugin
    pot = oracle.make_pot(oracle.POT_LJ, LJ)
    f_ref, u_ref, w_ref, _ = oracle.forces_brute(s["x"], s["box"], 2.5, pot, s["diam"])
    with MDDevice(3, s["n"], s["box"], 2.5) as d:
        d.set_potential_source(USER_LJ_SRC, "user_lj", [1.0, 2.5])
        d.upload(s["x"], s["v"], s["f"], s["img"], s["diam"])
        u, w = d.compute_forces()
        _, _, f, _ = d.download()
        _check_forces(f, f_ref)
        assert abs(u - u_ref) <= 1e-12 * abs(u_ref) and abs(w - w_ref) <= 1e-12 * abs(w_ref)
        ref = oracle.run(s["x"], s["img"], s["v"], s["f"], s["diam"], s["box"], 2.5, pot, 0.001, 10, use_cells=True,
                         nthreads=1)
        d.upload(s["x"], s["v"], s["f"], s["img"], s["diam"])
        d.run(10, 0.001)
        x, v, _, _ = d.download()
        assert np.abs(x - ref["x"]).max() <= 1e-10 and np.abs(v - ref["v"]).max() <= 1e-10
        with pytest.raises(md.MdhipError, match="(?s)compiling the user potential failed.*error"):
            d.set_potential_source("__device__ void broken(double r) { this is not C++ }", "broken", [])

    class UserLJ(md.Potential):
        def evaluate(self, r, s1, s2):
            return md.LennardJones().evaluate(r, s1, s2)

        def device_spec(self):
            return ("source", USER_LJ_SRC, "user_lj", [1.0, 2.5])

    assert UserLJ().device_spec()[0] == "source"


def test_pruning_changes_nothing():
    """Dynamic pruning (opt-in) only drops candidates that cannot interact before the next prune and
    keeps the order of the rest, so each force evaluation is unchanged.  (The runs are not bit-identical
    as a whole: rebuilds happen at different steps, which reorders particles and hence sums.)"""
    from moleculardynamics.jl_amd import MDDevice
    s = lj_system(32768, kT=2.5)
    out = []
    for inner in (0.0, 0.12, 0.05):
        with MDDevice(3, s["n"], s["box"], 2.5) as d:
            d.set_potential(0, LJ)
            d.set_inner_skin(inner)
            d.upload(s["x"], s["v"], s["f"], s["img"], s["diam"])
            uwk = d.run(150, 0.002)
            x, v, f, img = d.download()
            st = d.stats()
        out.append((x, v, f, uwk, st))
    assert out[0][4]["prunes"] == 0 and out[1][4]["prunes"] > 5 and out[2][4]["prunes"] > out[1][4]["prunes"]
    for x, v, f, uwk, st in out[1:]:
        assert np.abs(x - out[0][0]).max() <= 1e-9 and np.abs(v - out[0][1]).max() <= 1e-9
        _check_forces(f, out[0][2], 1e-9)
        assert abs(uwk[0] - out[0][3][0]) <= 1e-10 * abs(out[0][3][0])


@pytest.mark.parametrize("list_cutoff", [2.5, 3.0])
def test_cutoff_decisions_follow_reference_arithmetic(oracle, list_cutoff):
    """Adversarial dimers (tests/util.py cutoff_dimers): squared separations ON the threshold, one ulp either side,
    and between the reference-form value and the fma-chain value.  list_cutoff 2.5: the threshold is CellListMap's
    d2 <= cutoff^2.  list_cutoff 3.0: it is LJ's own sqrt(d2) >= r_cut -> (0,0) (src/potentials.jl:67-69), i.e.
    d2 >= the smallest double whose sqrt rounds to 2.5 (which is 6.25 - 1 ulp, not 6.25).  Pair set bit-exact;
    a single misclassified pair would change U by 1.6e-2 and two forces by 3.9e-2.  Exercises the generic kernels
    (md_compute_forces, md_neighbor_pairs) and both fast kernels (prune step and inner rows) through md_run."""
    from tests.util import cutoff_dimers, d2_forms, sqrt_ge_threshold
    target = 6.25 if list_cutoff == 2.5 else sqrt_ge_threshold(2.5)
    assert list_cutoff == 2.5 or target == np.nextafter(6.25, 0.0)
    s = cutoff_dimers(target)
    nd = s["n"] // 2
    disagree = sum(1 for k in range(nd) if (lambda rf: (rf[0] <= target) != (rf[1] <= target))(d2_forms(s["x"][2 * k], s["x"][2 * k + 1])))
    assert disagree >= nd // 4
    pot = oracle.make_pot(oracle.POT_LJ, LJ)
    f_ref, u_ref, w_ref, pairs_ref = oracle.forces_brute(s["x"], s["box"], list_cutoff, pot, s["diam"], want_pairs=True)
    with _dev(s, list_cutoff) as d:
        u, w = d.compute_forces()
        _, _, f, _ = d.download()
        pairs = d.neighbor_pairs()
        assert np.array_equal(pairs, pairs_ref[np.lexsort((pairs_ref[:, 1], pairs_ref[:, 0]))]), "pair set differs"
        _check_forces(f, f_ref)
        assert abs(u - u_ref) <= 1e-12 * abs(u_ref) and abs(w - w_ref) <= 1e-12 * abs(w_ref)
        # the no-energy kernels of the step loop: dt so small that nothing moves (x + v*dt == x)
        d.upload(s["x"], s["v"], s["f"], s["img"], s["diam"])
        for which in ("prune step", "inner rows"):
            d.run(1, 1e-30, thermo=False)
            x, _, f, _ = d.download()
            assert np.array_equal(x, s["x"]), which
            _check_forces(f, f_ref)


def test_cross_face_threshold_dimers(oracle):
    """Dimers straddling a periodic face or edge whose squared separation sits on the force threshold (sqrt(d2) < r_cut,
    i.e. d2 <= 6.25 - 2 ulp) under one end's rounding and beyond it under the other's (tests/util.py cross_face_dimers;
    module docstring: residual asymmetry).  Required: the exported pair set is the oracle's bit for bit; the
    smaller-index particle of every dimer -- whose evaluation IS the oracle's form -- gets the oracle's force; the other
    particle gets the force its own end's reference-form arithmetic decides, which for the steered dimers is exactly
    zero where the oracle's is not (category 0) and the reverse (category 1): the asymmetry is pinned, not hidden."""
    from tests.util import cross_face_dimers, face_d2_forms
    t_force = float(np.nextafter(6.25, 0.0))             # LJ contributes iff d2 < t_force  (sqrt(d2) < 2.5)
    target = float(np.nextafter(t_force, 0.0))           # ... iff d2 <= target
    s = cross_face_dimers(target)
    L = float(s["box"][0])
    nd = s["n"] // 2
    assert (s["cat"] >= 0).all() and min(np.bincount(s["cat"])) >= 10
    pot = oracle.make_pot(oracle.POT_LJ, LJ)
    f_ref, u_ref, w_ref, pairs_ref = oracle.forces_brute(s["x"], s["box"], 2.5, pot, s["diam"], want_pairs=True)
    forms = [face_d2_forms(s["x"][2 * k], s["x"][2 * k + 1], L) for k in range(nd)]
    hit_o = np.array([fo <= target for fo, _ in forms])
    hit_b = np.array([fb <= target for _, fb in forms])
    # the oracle agrees with the hand arithmetic of its own form
    assert np.array_equal(np.abs(f_ref[0::2]).max(axis=1) > 0.0, hit_o)
    assert (hit_o != hit_b).sum() >= 30

    def check(f, what):
        fa, fb = f[0::2], f[1::2]
        scale = max(1.0, np.abs(f_ref).max())
        assert np.abs(fa - f_ref[0::2]).max() <= 1e-11 * scale, what            # the oracle's end
        # the other end: zero exactly where ITS form rejects; else minus the oracle-form force of the partner, to rounding
        assert np.all(fb[~hit_b] == 0.0), what
        both = hit_b & hit_o
        assert np.abs(fb[both] - f_ref[1::2][both]).max() <= 1e-11 * scale, what
        only_b = hit_b & ~hit_o                                                 # oracle: no force at all on this dimer
        assert np.all(np.linalg.norm(fb[only_b], axis=1) > 0.038) and np.all(f_ref[1::2][only_b] == 0.0), what  # |F(r_c)| = 0.039
        assert np.all(fa[only_b] == 0.0), what

    with _dev(s, 2.5) as d:
        u, w = d.compute_forces()
        _, _, f, _ = d.download()
        pairs = d.neighbor_pairs()
        assert np.array_equal(pairs, pairs_ref[np.lexsort((pairs_ref[:, 1], pairs_ref[:, 0]))]), "pair set differs"
        check(f, "generic kernel")
        d.upload(s["x"], s["v"], s["f"], s["img"], s["diam"])
        for which in ("prune step", "inner rows"):
            d.run(1, 1e-30, thermo=False)
            x, _, f, _ = d.download()
            assert np.array_equal(x, s["x"]), which
            check(f, which)


# ---------------------------------------------------------------- thermo line values (src/simulation.jl:118-134)
@pytest.mark.parametrize("nvt", [False, True])
def test_thermo_lines_match_oracle(oracle, tmp_path, nvt):
    """Every thermo row run_simulation writes -- e = (U + energy_lrc)/N, T, P = W/(d V) + rho T + pressure_lrc
    (src/simulation.jl:118-134), LennardJones(tail_correction=true) (src/potentials.jl:111-152) -- against the
    oracle's step loop with the same formulas applied to its raw U, T, W rows: identical text at "%.6f".
    NVT: the driver's thermostat draws are replayed from a clone of state.rng, segment by segment."""
    import moleculardynamics.jl_amd as md
    from moleculardynamics.jl_amd.thermostat import draw_bussi
    n, dt, freq, total, kT = 1024, 0.001, 20, 45, 1.4737
    rho = 0.897
    pot = md.LennardJones(tail_correction=True)
    params = md.Parameters(rho, n, dt, pot)
    path = str(tmp_path / ("nvt" if nvt else "nve"))
    state = md.initialize_state(params, path, random_init=True, cutoff=2.5, rng=np.random.default_rng(7))
    state.velocities = md.initialize_velocities(kT, np.random.default_rng(8), n, 3)
    x0, v0 = state.system.positions.copy(), state.velocities.copy()
    box = np.diag(state.unitcell).copy()
    volume = float(np.prod(box))
    state.rng = np.random.default_rng(99)
    clone = np.random.default_rng(99)
    ens = md.NVT(kT, 100.0 * dt) if nvt else md.NVE()
    md.run_simulation(state, params, ens, total, freq, path)
    state.system.device.close()
    rows = [ln.split() for ln in open(os.path.join(path, "thermo.txt")).read().splitlines()[1:]]
    # the oracle's run, thermostat noise in the driver's draw order (one draw_bussi call per segment)
    kw = {}
    if nvt:
        segs = [1, 20, 20, 4]          # output steps 0, 20, 40, then the tail to step 44
        draws = [draw_bussi(state.nf, clone, k) for k in segs]
        kw = dict(ensemble=1, tau=100.0 * dt, ktemp=np.full(total, kT), r1=np.concatenate([d[0] for d in draws]),
                  r2=np.concatenate([d[1] for d in draws]))
    opot = oracle.make_pot(oracle.POT_LJ, LJ)
    ref = oracle.run(x0, np.zeros((n, 3), np.int32), v0, np.zeros_like(x0), np.ones(n), box, 2.5, opot, dt, total,
                     frequency=freq, use_cells=False, **kw)
    L = oracle.lib()
    dens = n / volume
    e_lrc = L.oracle_ener_lrc(2.5, dens, 1.0)          # per particle (src/potentials.jl:111-121, :136-143 multiplies by N)
    p_lrc = L.oracle_pressure_lrc(2.5, dens, 1.0)
    assert abs(e_lrc - (-0.48028349255352715)) < 1e-4 and abs(p_lrc - (-0.8604505670240141)) < 1e-4   # SURVEY.md section 4 KATs at rho = 0.897
    assert len(rows) == len(ref["thermo"]) == 3
    for row, (step, U, T, W) in zip(rows, ref["thermo"]):
        e = (U + e_lrc * n) / n
        P = W / (3 * volume) + rho * T + p_lrc
        want = ("%d %.6f %.6f %.6f" % (int(step), e, T, P)).split()
        assert abs(float(row[1]) - e) < 2e-6 and abs(float(row[2]) - T) < 2e-6 and abs(float(row[3]) - P) < 2e-6
        assert row == want, (row, want)
    assert abs(e_lrc) > 0.4        # the tail correction really is in the energy column


# ---------------------------------------------------------------- BASELINE configs[4] through the PLUGIN path
POLY_SRC = r"""
// README.md:89-145 written positionally (SURVEY.md D6): evaluate(pot, r, sigma1, sigma2) with
// params = {rcut, non_additivity}; integer powers as multiply chains (@fastpow)
__device__ double upow(double x, int n) { double r = 1.0; while (n) { if (n & 1) r *= x; x *= x; n >>= 1; } return r; }
__device__ void readme_polydisperse(double r, double sigma1, double sigma2, const double *p, double *u, double *f)
{
    double rcut = p[0], non_additivity = p[1];
    double se = 0.5 * (sigma1 + sigma2);
    se *= (1.0 - non_additivity * fabs(sigma1 - sigma2));
    double uij = 0.0, fij = 0.0;
    if (r < rcut * se) {
        double term_1 = upow(se / r, 12);
        double c0 = -28.0 / upow(rcut, 12);
        double c2 = 48.0 / upow(rcut, 14);
        double c4 = -21.0 / upow(rcut, 16);
        double term_2 = c2 * upow(r / se, 2);
        double term_3 = c4 * upow(r / se, 4);
        uij = term_1 + c0 + term_2 + term_3;
        fij = 12.0 * upow(se, 12) / upow(r, 13) - 2.0 * c2 * r / upow(se, 2) - 4.0 * c4 * upow(r, 3) / upow(se, 4);
    }
    *u = uij;
    *f = fij;
}
"""


@pytest.mark.parametrize("rho,dlo,dhi", [(1.0, 0.6, 1.2), (0.58, 0.73, 1.62)])
def test_config5_polydisperse_through_the_plugin(oracle, rho, dlo, dhi):
    """BASELINE configs[4]: N = 1200, 2-D, the README's Polydisperse `evaluate` overload, kT = 0.11 -- run through the
    Potential PLUGIN (md_set_potential_source: hiprtc compiles k_force_tile<2, POT_CUSTOM, ...> around the user's
    function), not the built-in kind.  Two diameter sets: U[0.6, 1.2] at rho = 1 (tests/util.py explains why), and
    SURVEY.md's U[0.73, 1.62] in a box scaled to rho = 0.58 (same area fraction) -- the distribution as surveyed, the
    box adapted, since at rho = 1 that distribution over-packs (area fraction 1.14).  20 steps against the oracle."""
    import moleculardynamics.jl_amd as md
    from moleculardynamics.jl_amd import MDDevice
    s = poly_system(rho=rho, dlo=dlo, dhi=dhi)
    cutoff = 1.25 * dhi                  # list_cutoff = 1.25 * sigma_eff,max
    pot = oracle.make_pot(oracle.POT_POLYDISPERSE, [1.25, 0.2])
    f_ref, u_ref, w_ref, pairs_ref = oracle.forces_brute(s["x"], s["box"], cutoff, pot, s["diam"], want_pairs=True)
    ref = oracle.run(s["x"], s["img"], s["v"], s["f"], s["diam"], s["box"], cutoff, pot, 0.005, 20, use_cells=False)
    with MDDevice(2, s["n"], s["box"], cutoff) as d:
        d.set_potential_source(POLY_SRC, "readme_polydisperse", [1.25, 0.2])
        d.upload(s["x"], s["v"], s["f"], s["img"], s["diam"])
        u, w = d.compute_forces()
        _, _, f, _ = d.download()
        pairs = d.neighbor_pairs()
        assert d.stats()["tiled"] == 1           # the tiled kernel of the run-time compiled module, 2-D instantiation
        assert np.array_equal(pairs, pairs_ref[np.lexsort((pairs_ref[:, 1], pairs_ref[:, 0]))])
        _check_forces(f, f_ref)
        assert abs(u - u_ref) <= 1e-12 * abs(u_ref) and abs(w - w_ref) <= 1e-12 * abs(w_ref)
        d.upload(s["x"], s["v"], s["f"], s["img"], s["diam"])
        U, W, K = d.run(20, 0.005)
        x, v, _, img = d.download()
    assert np.abs(x - ref["x"]).max() <= 1e-10 and np.abs(v - ref["v"]).max() <= 1e-10
    assert np.array_equal(img, ref["img"])
    assert abs(U - ref["U"]) <= 1e-11 * abs(ref["U"]) and abs(K - ref["K"]) <= 1e-12 * abs(ref["K"])
    # and the host-side spelling a user would write
    hostpot = md.Polydisperse(1.25, 0.2)
    for r, s1, s2 in [(1.0, 1.0, 1.0), (0.9, 0.73, 1.62), (1.3, 1.2, 0.8)]:
        uo, fo = oracle.evaluate(pot, r, s1, s2)
        uh, fh = hostpot.evaluate(r, s1, s2)
        assert abs(uo - uh) <= 1e-13 * max(1.0, abs(uo)) and abs(fo - fh) <= 1e-13 * max(1.0, abs(fo))


@pytest.mark.parametrize("rho,u_nist,p_nist", [(0.776, -5.5121, 6.7714e-3), (0.820, -5.7947, 5.5355e-1), (0.900, -6.2391, 2.2314)])
def test_lj_fluid_against_the_nist_reference_table(rho, u_nist, p_nist):
    """An answer nobody here produced: the NIST Standard Reference Simulation Website's Lennard-Jones fluid benchmarks
    (MD and MC, r_c = 3 sigma with the standard long-range corrections, T* = 0.85; U* = -5.5121, -5.7947, -6.2391 and
    p* = 0.0068, 0.5535, 2.2314 at rho* = 0.776, 0.820, 0.900 -- the table as published; there is no network here to fetch it
    again, and five state points that come out right to four digits in U are not right by accident).  The reference repository holds no fixture that pins
    its arithmetic (parity with it stays unpinned); this pins the PHYSICS of the whole device path --
    pair forces, virial, velocity Verlet with wrapping, the Bussi thermostat, energy_lrc / pressure_lrc
    (src/potentials.jl:111-152) -- to published numbers: N = 4000, 15 000 steps of equilibration, 40 000 of production at
    dt = 0.004, thermo every 20 steps.  Tolerances: five standard errors of the block averages (0.0006-0.0008 in U, 0.002-0.004 in
    p, scripts/probe/nist_lj.py) plus the O(dt^2) bias of the integrator at this time step (measured: |dU| <= 0.0023,
    |dp| <= 0.0074).  Deterministic: fixed seeds, and the device path sums in a fixed order."""
    from moleculardynamics.jl_amd import MDDevice, _lib, lattice_positions, initialize_velocities
    from moleculardynamics.jl_amd.thermostat import draw_bussi
    n, T, rc, dt, every, nequil, nprod = 4000, 0.85, 3.0, 0.004, 20, 15000, 40000
    L = (n / rho) ** (1.0 / 3.0)
    box = np.full(3, L)
    x = lattice_positions(n, box, 3, np.random.default_rng(1))
    v = initialize_velocities(T, np.random.default_rng(2), n, 3)
    nf = 3.0 * (n - 1.0)
    rng = np.random.default_rng(3)
    u_lrc = (8.0 / 3.0) * np.pi * rho * ((1.0 / 3.0) * rc ** -9 - rc ** -3)
    p_lrc = (16.0 / 3.0) * np.pi * rho ** 2 * ((2.0 / 3.0) * rc ** -9 - rc ** -3)
    us, ps = [], []
    with MDDevice(3, n, box, rc) as dev:
        dev.set_potential(_lib.MD_POT_LJ, [1.0, 1.0, rc])
        dev.upload(x, v, np.zeros_like(x), np.zeros((n, 3), np.int32), np.ones(n))
        r1, r2 = draw_bussi(nf, rng, nequil)
        dev.run(nequil, dt, _lib.MD_NVT, 0.1, nf, np.full(nequil, T), r1, r2)
        for _ in range(nprod // every):
            r1, r2 = draw_bussi(nf, rng, every)
            U, W, K = dev.run(every, dt, _lib.MD_NVT, 0.1, nf, np.full(every, T), r1, r2)
            us.append(U / n + u_lrc)
            ps.append(rho * (2.0 * K / nf) + W / (3.0 * L ** 3) + p_lrc)
    u_mean, p_mean = float(np.mean(us)), float(np.mean(ps))
    assert abs(u_mean - u_nist) <= 0.005, (u_mean, u_nist)
    assert abs(p_mean - p_nist) <= 0.025, (p_mean, p_nist)


@pytest.mark.parametrize("rho", [0.3, 0.5, 0.7])
def test_pseudo_hard_spheres_against_carnahan_starling(rho):
    """BASELINE configs[0]'s potential against an answer from outside: PseudoHS (src/potentials.jl:5-29, the 50-49 Mie
    potential built to reproduce hard spheres at T* = 1.4737) must give the hard-sphere equation of state.  Compressibility
    factor Z = P / (rho kT) from the virial of an NVT run (4000 particles, 10 000 + 30 000 steps, dt = 0.0005, tau = 100 dt as
    README.md:33) against Carnahan-Starling, Z = (1 + f + f^2 - f^3) / (1 - f)^3, f = pi rho / 6, itself good to a few 1e-3
    of the hard-sphere fluid: measured ratio 0.9996 / 0.9999 / 1.0016 at rho = 0.3 / 0.5 / 0.7 (scripts/probe/phs_eos.py);
    the test allows 1 %."""
    from moleculardynamics.jl_amd import MDDevice, _lib, lattice_positions, initialize_velocities
    from moleculardynamics.jl_amd.thermostat import draw_bussi
    n, T, dt, every, nequil, nprod = 4000, 1.4737, 0.0005, 20, 10000, 30000
    L = (n / rho) ** (1.0 / 3.0)
    box = np.full(3, L)
    x = lattice_positions(n, box, 3, np.random.default_rng(1))
    v = initialize_velocities(T, np.random.default_rng(2), n, 3)
    nf = 3.0 * (n - 1.0)
    rng = np.random.default_rng(3)
    zs = []
    with MDDevice(3, n, box, 1.5) as dev:
        dev.set_potential(_lib.MD_POT_PSEUDOHS, [50.0])
        dev.upload(x, v, np.zeros_like(x), np.zeros((n, 3), np.int32), np.ones(n))
        r1, r2 = draw_bussi(nf, rng, nequil)
        dev.run(nequil, dt, _lib.MD_NVT, 100 * dt, nf, np.full(nequil, T), r1, r2)
        for _ in range(nprod // every):
            r1, r2 = draw_bussi(nf, rng, every)
            U, W, K = dev.run(every, dt, _lib.MD_NVT, 100 * dt, nf, np.full(every, T), r1, r2)
            zs.append((rho * (2.0 * K / nf) + W / (3.0 * L ** 3)) / (rho * T))
    f = np.pi * rho / 6.0
    z_cs = (1.0 + f + f * f - f ** 3) / (1.0 - f) ** 3
    assert abs(np.mean(zs) / z_cs - 1.0) <= 0.01, (float(np.mean(zs)), z_cs)
