"""-m gpu: the Hessian of the pair energy on the device (md_hess_*, moleculardynamics/jl_amd/vibrations.py) against
tests/hess_reference.py, on every list layout the handle can take.

Frames: lj500 (the lj_n500_rc1p5 system relaxed by the device's own FIRE; 3-D, uniform diameters, 24-byte records, a partial
last tile and wave), poly1200 (the poly2d_n1200 system; 2-D, per-particle diameters, a per-pair cutoff), tric512 (N = 512
Lennard-Jones in a sheared cell) and xplor500 (LennardJonesXPLOR with per-particle diameters, N = 500).

Tolerance of every comparison with the reference: 10 x the frame's fp64 rounding floor, the reference against itself in
numpy.longdouble (hess_reference.rounding_floor), relative to max |H|.  It is computed here, never from the device."""
import ctypes as C
import types

import numpy as np
import pytest

from tests import hess_reference as hr
from tests.util import lj_system, poly_system, sheared, with_diameters

pytestmark = pytest.mark.gpu

LAYOUTS = {"default": {}, "no_fused_build": {"MDHIP_NO_FUSED_BUILD": "1"}, "no_tiles": {"MDHIP_NO_TILES": "1"}}
_FRAMES, _REFS = {}, {}


def _potential(name):
    import moleculardynamics.jl_amd as md
    if name in ("lj500", "tric512", "lj_raw"):
        return md.LennardJones()
    if name in ("poly1200", "poly256", "poly256_raw"):
        return md.Polydisperse(1.25, 0.2)
    return md.LennardJonesXPLOR(epsilon=1.0, sigma=1.0, r_cut=2.0, r_on=1.5)


def _relax(s, cutoff, pot):
    """The frame the device's own FIRE stops at (positions by particle id, wrapped as the device holds them)."""
    from moleculardynamics.jl_amd import MDDevice
    spec = pot.device_spec()
    with MDDevice(s["dim"], s["n"], s.get("cell", s["box"]), cutoff) as dev:
        dev.set_potential(spec[1], spec[2])
        dev.upload(s["x"], np.zeros_like(s["x"]), np.zeros_like(s["x"]), s["img"], s["diam"])
        r = dev.fire_minimize(max_steps=30000, tol=1e-9, dt_initial=0.002, dt_max=0.02)
        x = dev.download()[0]
    out = dict(s)
    out["x"] = np.ascontiguousarray(x)
    out["fire"] = r
    return out


def frame(name):
    """dict(system, cutoff, pot, kind, params) of a named frame, built once per session."""
    if name not in _FRAMES:
        pot = _potential(name)
        if name == "lj500":
            s, cutoff = _relax(lj_system(500), 1.5, pot), 1.5
        elif name == "lj_raw":
            s, cutoff = lj_system(500), 1.5
        elif name == "poly1200":
            s, cutoff = poly_system(), 1.5
        elif name == "poly256":
            s, cutoff = _relax(poly_system(n=256), 1.5, pot), 1.5
        elif name == "poly256_raw":
            s, cutoff = poly_system(n=256), 1.5
        elif name == "tric512":
            s = lj_system(512)
            s, cutoff = sheared(s, 3.0 * s["box"][0] / 8.0), 2.5
        elif name == "xplor500":
            s, cutoff = with_diameters(lj_system(500), 0.9, 1.1), 2.0
        else:
            raise KeyError(name)
        spec = pot.device_spec()
        _FRAMES[name] = dict(name=name, system=s, cutoff=cutoff, pot=pot, kind=spec[1], params=list(spec[2]))
    return _FRAMES[name]


def reference(name):
    """(floor, H) of a frame: hess_reference.rounding_floor, once per session."""
    if name not in _REFS:
        fr = frame(name)
        s = fr["system"]
        _REFS[name] = hr.rounding_floor(s["x"], hr.lattice(s.get("cell", s["box"]), s["dim"]), fr["cutoff"], fr["kind"],
                                        fr["params"], s["diam"])
        print("%s: fp64 rounding floor of the reference %.3e (relative to max |H| = %.6g)"
              % (name, _REFS[name][0], np.abs(_REFS[name][1]).max()))
    return _REFS[name]


def state_of(fr, x=None):
    """(state, params) around a fresh MDDevice, as initialize_state would hand them to the vibrations module."""
    import moleculardynamics.jl_amd as md
    s = fr["system"]
    n, dim = s["n"], s["dim"]
    dev = md.MDDevice(dim, n, s.get("cell", s["box"]), fr["cutoff"])
    x = np.array(s["x"] if x is None else x)
    system = types.SimpleNamespace(device=dev, positions=x, xpositions=None,
                                   energy_and_forces=types.SimpleNamespace(forces=np.zeros((n, dim)), energy=0.0, virial=0.0))
    state = md.SimulationState(system, np.array(s["diam"]), np.random.default_rng(1), hr.lattice(s.get("cell", s["box"]), dim),
                               np.zeros((n, dim)), np.zeros((n, dim), dtype=np.int32), dim, dim * (n - 1.0))
    return state, md.Parameters(1.0, n, 0.002, fr["pot"])


def _matvec_error(Y, X, Href):
    """max over the elements of |Y - Href X| / (max |H| * sum over the row's non-zero entries of |X|): the elementwise bound
    on H carried through one row.  A row without entries (a particle without neighbours) must give exactly 0."""
    m = X.shape[0]
    diff = np.abs(Y.reshape(m, -1) - X.reshape(m, -1) @ Href)
    bound = np.abs(Href).max() * (np.abs(X.reshape(m, -1)) @ (Href != 0.0))
    assert not np.any(diff[bound == 0.0] != 0.0)
    return float((diff[bound > 0.0] / bound[bound > 0.0]).max())


def _set_layout(monkeypatch, layout):
    for k, v in LAYOUTS[layout].items():
        monkeypatch.setenv(k, v)


def _check_layout(dev, layout):
    info = dev.list_rows(0)["info"]
    assert info["list_valid"] == 1
    assert info["tiled"] == (0 if layout == "no_tiles" else 1) and info["rows32"] == (1 if layout == "no_tiles" else 0), info
    if layout == "no_fused_build":
        assert info["fused_build"] == 0, info
    return info


# ---------------------------------------------------------------------------------------------------------------------
# checks 1 and 2: the dense matrix against the reference; the exact properties
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("name", ["lj500", "poly1200", "tric512", "xplor500"])
def test_dense_matrix_and_exact_properties(monkeypatch, name, layout):
    import moleculardynamics.jl_amd as md
    _set_layout(monkeypatch, layout)
    fr = frame(name)
    floor, Href = reference(name)
    s = fr["system"]
    n, d = s["n"], s["dim"]
    scale = np.abs(Href).max()
    state, params = state_of(fr)
    with state.system.device as dev:
        op = md.HessianOperator(state, params)
        info = _check_layout(dev, layout)
        rng = np.random.default_rng(5)
        X = rng.standard_normal((8, n, d))
        Y = op.matvec(X)
        # (an element of H X: the elementwise bound on H summed over the row's non-zero entries against |X|)
        err_mv = _matvec_error(Y, X, Href)
        H = op.dense()
        err = np.abs(H - Href).max() / scale
        blocks = op.blocks()
        err_b = np.abs(blocks - hr.diagonal_blocks(Href, n, d)).max() / scale
        print("%s/%s (fused_build %d): dense |H - Href| / max|H| = %.3e, blocks %.3e, matvec %.3e; floor %.3e, allowed %.3e"
              % (name, layout, info["fused_build"], err, err_b, err_mv, floor, 10 * floor))
        # 1. against the reference (one missing or doubled pair would be O(1) of a block: tests/test_hessian.py)
        assert err <= 10 * floor and err_b <= 10 * floor and err_mv <= 10 * floor
        assert np.abs(blocks - hr.diagonal_blocks(H, n, d)).max() <= 10 * floor * scale
        # 2. exact: symmetric bit for bit, translations give 0.0, repeatable, a column does not depend on its block
        assert np.array_equal(H, H.T)
        T = op.matvec(np.sqrt(n) * hr.translations(n, d))
        assert np.array_equal(T, np.zeros_like(T))
        assert np.array_equal(op.matvec(X), Y)
        for c in range(8):
            assert np.array_equal(op.matvec(X[c]), Y[c]), c
        with pytest.raises(ValueError):
            op.matvec(np.zeros((n + 1, d)))


# ---------------------------------------------------------------------------------------------------------------------
# check 3: a pair next to the cutoff
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_pair_straddling_the_cutoff(monkeypatch, layout):
    """Two particles at r = rc (1 -+ 2^-40): the block is there, then it is not -- the force kernel's decision."""
    from moleculardynamics.jl_amd import MDDevice
    _set_layout(monkeypatch, layout)
    rc = 2.5
    for side, r in (("inside", rc * (1.0 - 2.0 ** -40)), ("outside", rc * (1.0 + 2.0 ** -40))):
        x = np.array([[1.0, 1.0, 1.0], [1.0 + r, 1.0, 1.0]])
        z = np.zeros_like(x)
        with MDDevice(3, 2, np.full(3, 9.0), rc) as dev:
            dev.set_potential(0, [1.0, 1.0, rc])
            dev.upload(x, z, z, np.zeros((2, 3), dtype=np.int32), np.ones(2))
            dev.compute_forces()
            f = dev.download()[2]
            dev.hess_setup()
            blocks = dev.hess_blocks()
            Y = dev.hess_apply(np.array([[[1.0, 0.0, 0.0], [0.0, 0.0, 0.0]]]))
        present = bool(np.any(blocks != 0.0))
        print("%s/%s: r - rc = %.3e, |f| = %.6g, block xx = %.6g" % (layout, side, r - rc, np.abs(f).max(), blocks[0, 0, 0]))
        assert present == bool(np.any(f != 0.0)) == (side == "inside")
        if present:
            d = x[1, 0] - x[0, 0]
            t, k, _ = hr.pair_tk(hr.POT_LJ, [1.0, 1.0, rc], d, 1.0, 1.0)
            assert abs(blocks[0, 0, 0] - k) <= 1e-14 * abs(k) and abs(blocks[0, 1, 1] - t) <= 1e-14 * abs(t)
            assert np.array_equal(blocks[0], blocks[1]) and Y[0, 0, 0] == blocks[0, 0, 0] and Y[0, 1, 0] == -blocks[0, 0, 0]
        else:
            assert not np.any(Y != 0.0)


# ---------------------------------------------------------------------------------------------------------------------
# check 4: -H v against a central difference of the device's own forces
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["poly1200", "xplor500"])
def test_force_consistency(oracle, name):
    """Both potentials are smooth at their cutoff.  Tolerance: 10 x the error of the same central difference of the oracle's
    forces against the reference's analytic H v, on this frame and epsilon."""
    import moleculardynamics.jl_amd as md
    fr = frame(name)
    _, Href = reference(name)
    s = fr["system"]
    n, d = s["n"], s["dim"]
    eps = 1e-5
    v = np.random.default_rng(9).uniform(-1.0, 1.0, (n, d))
    pot = oracle.make_pot(fr["kind"], fr["params"])
    fp = oracle.forces_brute(s["x"] + eps * v, s["box"], fr["cutoff"], pot, s["diam"])[0]
    fm = oracle.forces_brute(s["x"] - eps * v, s["box"], fr["cutoff"], pot, s["diam"])[0]
    ref_err = np.abs((fp - fm) / (2 * eps) + (Href @ v.reshape(-1)).reshape(n, d)).max()
    state, params = state_of(fr)
    z = np.zeros((n, d))
    with state.system.device as dev:
        op = md.HessianOperator(state, params)
        hv = op.matvec(v)
        F = []
        for sign in (1.0, -1.0):
            dev.upload(s["x"] + sign * eps * v, z, z, s["img"], s["diam"])
            dev.compute_forces()
            F.append(dev.download()[2])
        with pytest.raises(md.MdhipError, match="md_hess_setup"):
            op.matvec(v)                                                       # (the uploads moved the frame)
    err = np.abs((F[0] - F[1]) / (2 * eps) + hv).max()
    print("%s: |dF/2eps + H v| device %.3e, reference %.3e (allowed %.3e), max |H v| %.4g"
          % (name, err, ref_err, 10 * ref_err, np.abs(hv).max()))
    assert err <= 10 * ref_err


# ---------------------------------------------------------------------------------------------------------------------
# check 5: invalidation and refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_invalidation():
    import moleculardynamics.jl_amd as md
    fr = frame("lj500")
    floor, Href = reference("lj500")
    s = fr["system"]
    n, d = s["n"], s["dim"]
    X = np.random.default_rng(3).standard_normal((2, n, d))
    state, params = state_of(fr)
    with state.system.device as dev:
        op = md.HessianOperator(state, params)
        Y = op.matvec(X)
        dev.compute_forces()                                                   # (a valid list: nothing moves)
        assert np.array_equal(op.matvec(X), Y)
        dev.upload(v=s["v"])
        for call in (lambda: op.matvec(X), op.blocks, lambda: dev.hess_lanczos(4), lambda: dev.hess_ritz(np.eye(4), np.ones(4))):
            with pytest.raises(md.MdhipError, match="md_hess_setup"):
                call()
        dev.hess_setup()
        assert np.array_equal(op.matvec(X), Y)                                 # (velocities only: the same frame)
        dev.run(1, 0.002)
        with pytest.raises(md.MdhipError, match="md_hess_setup"):
            op.matvec(X)
        dev.hess_setup()
        x1 = dev.download()[0]
        Y1 = dev.hess_apply(X)
        H1 = hr.dense(x1, hr.lattice(s["box"], d), fr["cutoff"], fr["kind"], fr["params"], s["diam"])
        err = _matvec_error(Y1, X, H1)
        print("after one step and a new setup: matvec error %.3e (allowed %.3e)" % (err, 10 * floor))
        assert err <= 10 * floor and not np.array_equal(Y1, Y)
        dev.fire_minimize(max_steps=2, tol=1e-300)
        with pytest.raises(md.MdhipError, match="md_hess_setup"):
            dev.hess_blocks()
        with pytest.raises(ValueError):
            dev.hess_apply(np.zeros((9, n, d)))


def test_user_potentials_and_slab_handles_are_refused():
    from moleculardynamics.jl_amd import MDDevice, MdhipError
    from moleculardynamics.jl_amd.domain import DomainDevice
    from tests.test_gpu_parity import USER_LJ_SRC
    s = lj_system(500)
    with MDDevice(3, 500, s["box"], 2.5) as dev:
        dev.set_potential_source(USER_LJ_SRC, "user_lj", [1.0, 2.5])
        dev.upload(s["x"], s["v"], s["f"], s["img"], s["diam"])
        with pytest.raises(MdhipError, match="user potential"):
            dev.hess_setup()
        dev.set_potential(0, [1.0, 1.0, 2.5])
        dev.hess_setup()
        dev.set_potential_source(USER_LJ_SRC, "user_lj", [1.0, 2.5])
        with pytest.raises(MdhipError, match="user potential"):
            dev.hess_blocks()

    class TwoRanks:
        rank, world = 0, 2

    s = lj_system(4096)
    with DomainDevice(3, s["n"], s["box"], 2.5, TwoRanks()) as dom:
        assert dom._L.md_hess_setup(dom._h) != 0
        assert "md_hess_setup: not available on a slab-decomposition handle" in dom._L.md_last_error(dom._h).decode()
        buf = (C.c_double * 9)()
        assert dom._L.md_hess_blocks(dom._h, buf) != 0
        assert "md_hess_blocks: not available on a slab-decomposition handle" in dom._L.md_last_error(dom._h).decode()


# ---------------------------------------------------------------------------------------------------------------------
# check 6: the lowest modes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["poly256", "lj500"])
def test_lowest_modes(name):
    import moleculardynamics.jl_amd as md
    fr = frame(name)
    floor, Href = reference(name)
    s = fr["system"]
    n, d = s["n"], s["dim"]
    state, params = state_of(fr)
    with state.system.device:
        res = md.lowest_modes(state, params, 8)
    lam, modes, resid = res["eigenvalues"], res["modes"].reshape(8, -1), res["residuals"]
    T = hr.translations(n, d).reshape(d, -1)
    normH = float(np.abs(np.linalg.eigvalsh(Href)).max())
    # the reference's spectrum without the d translations: they are moved to 10 |H|, above everything else
    wk, Vk = np.linalg.eigh(Href + 10.0 * normH * (T.T @ T))
    print("%s: FIRE %s; k = %d, converged %s, stable %s\n  lambda  %s\n  resid   %s\n  exact   %s"
          % (name, fr["system"].get("fire"), res["ksteps"], res["converged"], res["stable"], lam, resid, wk[:8]))
    assert res["converged"]
    match = np.array([int(np.argmin(np.abs(wk - l))) for l in lam])
    # (the residual bound of a symmetric matrix, plus check 1's floor times |H|)
    assert np.all(np.abs(wk[match] - lam) <= resid + floor * normH), np.abs(wk[match] - lam) - resid
    assert np.array_equal(match, np.arange(8)), match                        # the 8 lowest, none skipped or doubled
    G = modes @ modes.T
    assert np.abs(G - np.eye(8)).max() <= 1e-10 and np.abs(modes @ T.T).max() <= 1e-10
    # participation ratio where the eigenvalue is non-degenerate: the Ritz vector is within (residual / gap) of the
    # eigenvector (sin theta theorem), and P changes by at most a few times that (its derivative along a unit vector is
    # bounded by 4 P / max|e| ... 8 P); 20 x covers both
    gap = np.minimum(np.diff(wk[:9]), np.concatenate([[np.inf], np.diff(wk[:8])]))
    pr_ref = md.participation_ratio(Vk[:, :8].T.reshape(8, n, d))
    for c in range(8):
        if gap[c] > 1e-6 * normH:
            assert abs(res["participation"][c] - pr_ref[c]) <= 20.0 * (resid[c] + 10 * floor * normH) / gap[c] + 1e-12, c
    assert np.array_equal(res["frequencies"][lam >= 0], np.sqrt(lam[lam >= 0]))


@pytest.mark.parametrize("name", ["poly256_raw", "lj_raw"])
def test_a_frame_that_was_not_minimised_is_a_saddle(name):
    import moleculardynamics.jl_amd as md
    fr = frame(name)
    state, params = state_of(fr)
    with state.system.device:
        res = md.lowest_modes(state, params, 4)
    print("%s: lambda %s resid %s stable %s" % (name, res["eigenvalues"], res["residuals"], res["stable"]))
    assert res["stable"] is False and res["eigenvalues"][0] < 0.0


def test_lanczos_start_vector_does_not_depend_on_slot_order():
    """The same frame under two skins: different cell grids, so different slot orders and row orders.  alpha and beta of the
    first steps agree to rounding (1e-9 relative: eight steps amplify the 1e-15 differences of the sums only mildly), which
    they could not if the Philox start vector were keyed by slot."""
    fr = frame("poly256")
    s = fr["system"]
    out = []
    for skin in (None, 0.3):
        state, params = state_of(fr)
        with state.system.device as dev:
            dev.set_potential(fr["kind"], fr["params"])
            if skin is not None:
                dev.set_skin(skin)
            dev.upload(s["x"], np.zeros_like(s["x"]), np.zeros_like(s["x"]), s["img"], s["diam"])
            dev.hess_setup()
            a, b = dev.hess_lanczos(8, seed=3)
            a2, b2 = dev.hess_lanczos(8, seed=3)
            assert np.array_equal(a, a2) and np.array_equal(b, b2)              # reused basis, same bits
            a3, _ = dev.hess_lanczos(8, seed=4)
            assert not np.array_equal(a, a3)
            rows = dev.list_rows(0)["entries"][:, 0]
            out.append((a, b, rows[np.concatenate([[True], rows[1:] != rows[:-1]])]))
    (a0, b0, r0), (a1, b1, r1) = out
    assert not np.array_equal(r0, r1), "the two skins gave the same slot order: the test shows nothing"
    assert np.abs(a0 - a1).max() <= 1e-9 * np.abs(a0).max() and np.abs(b0 - b1).max() <= 1e-9 * np.abs(b0).max()


def test_a_basis_that_does_not_fit_is_refused_with_its_size(monkeypatch):
    import moleculardynamics.jl_amd as md
    fr = frame("poly256")
    state, params = state_of(fr)
    with state.system.device as dev:
        md.HessianOperator(state, params)
        monkeypatch.setenv("MDHIP_HESS_LIMIT", "1000")
        with pytest.raises(md.MdhipError, match=r"cannot allocate %d bytes for a Lanczos basis of 4 vectors of 512 doubles" % (4 * 512 * 8)):
            dev.hess_lanczos(4)
        monkeypatch.delenv("MDHIP_HESS_LIMIT")
        dev.hess_lanczos(4)
        with pytest.raises(md.MdhipError, match="holds 4 vectors"):
            dev.hess_ritz(np.eye(5)[:, :2], np.ones(2))
        with pytest.raises(md.MdhipError, match="ksteps"):
            dev.hess_lanczos(2 * 256 - 1)
