"""CPU: proves tests/hess_reference.py (the yardstick of tests/test_gpu_hessian.py) against the oracle, pins two known
answers, and drives the Python layer (moleculardynamics/jl_amd/vibrations.py) through a stub device.

What a wrong pair set would look like: leaving one pair out of the reference changes entries of H by that pair's block,
at least 1e-5 of max |H| on these frames, against a comparison tolerance (10 x the fp64 rounding floor) near 1e-14
(test_one_missing_pair_is_far_above_the_tolerance)."""
import types

import numpy as np
import pytest

import moleculardynamics.jl_amd as md
from moleculardynamics.jl_amd import vibrations
from tests import hess_reference as hr
from tests.util import lj_system, poly_system, with_diameters

# (kind, params, branch points, diameters): every built-in potential and mode
POTENTIALS = {
    "lj": (hr.POT_LJ, [1.0, 1.0, 2.5], [2.5], (1.0, 1.0)),
    "lj_mixed": (hr.POT_LJ, [1.3, 1.0, 2.2], [2.2], (0.9, 1.2)),
    "pseudohs": (hr.POT_PSEUDOHS, [50.0], [hr.PHS_B], (1.0, 1.0)),
    "pseudohs_mixed": (hr.POT_PSEUDOHS, [50.0], [hr.PHS_B], (0.95, 1.0)),
    "polydisperse": (hr.POT_POLYDISPERSE, [1.25, 0.2], [1.25 * 0.5 * (0.8 + 1.1) * (1.0 - 0.2 * 0.3)], (0.8, 1.1)),
    "lj_shifted": (hr.POT_LJ_MODIFIED, [1.0, 1.0, 2.5, 0.0, 0.0], [2.5], (1.0, 1.1)),
    "lj_force_shifted": (hr.POT_LJ_MODIFIED, [1.0, 1.0, 2.5, 1.0, 0.0], [2.5], (1.0, 1.1)),
    "lj_xplor": (hr.POT_LJ_MODIFIED, [1.0, 1.0, 2.5, 2.0, 2.0], [2.0, 2.5], (1.0, 1.1)),
}


@pytest.mark.parametrize("name", sorted(POTENTIALS))
def test_second_derivative_against_the_oracles_force(oracle, name):
    """k = -df/dr against a central difference of oracle.evaluate's force, t = -f/r against the force itself, at radii on
    both sides of every branch point.  Step h = 1e-6: the truncation h^2 |f'''| / 6 is below 1e-7 |k|; the rounding
    eps |terms of f| / h is 1e-10 of the core terms, which near a smooth cutoff cancel to a much smaller f and k -- hence
    the second, absolute part of the tolerance, 1e-9 of |k| at the smallest radius."""
    kind, params, branches, (s1, s2) = POTENTIALS[name]
    pot = oracle.make_pot(kind, params)
    h = 1e-6
    radii = [0.93, 1.0, 1.1]
    kcore = abs(float(hr.pair_tk(kind, params, radii[0], s1, s2)[1]))
    for b in branches:
        radii += [b * (1.0 - 1e-3), b * (1.0 - 1e-9), b * (1.0 + 1e-9), b * (1.0 + 1e-3)]
    rcut = max(branches)
    for r in radii:
        t, k, inside = (float(v) for v in hr.pair_tk(kind, params, r, s1, s2))
        f = oracle.evaluate(pot, r, s1, s2)[1]
        assert bool(inside) == (r < rcut) and (f != 0.0 or r >= rcut or kind == hr.POT_LJ_MODIFIED)
        if r >= rcut:
            assert t == 0.0 and k == 0.0 and f == 0.0
            continue
        assert abs(t + f / r) <= 1e-13 * abs(f / r), (name, r)
        if min(abs(r - b) for b in branches) < 2 * h:
            continue                                              # (the difference would straddle the branch point)
        fd = -(oracle.evaluate(pot, r + h, s1, s2)[1] - oracle.evaluate(pot, r - h, s1, s2)[1]) / (2 * h)
        assert abs(k - fd) <= 1e-7 * (abs(k) + abs(f) / r) + 1e-9 * kcore, (name, r, k, fd)


def _frames():
    lj = lj_system(256)
    return {
        "poly": (poly_system(n=256), 1.5, hr.POT_POLYDISPERSE, [1.25, 0.2]),
        "xplor": (with_diameters(lj, 0.9, 1.1), 2.0, hr.POT_LJ_MODIFIED, [1.0, 1.0, 2.0, 2.0, 1.5]),
        "lj": (lj, 2.5, hr.POT_LJ, [1.0, 1.0, 2.5]),
    }


_DENSE = {}


def _dense(name):
    if name not in _DENSE:
        s, cutoff, kind, params = _frames()[name]
        _DENSE[name] = (s, cutoff, kind, params) + hr.rounding_floor(s["x"], np.diag(s["box"]), cutoff, kind, params, s["diam"])
    return _DENSE[name]


@pytest.mark.parametrize("name", ["poly", "xplor", "lj"])
def test_dense_reference_is_symmetric_and_translation_invariant(name):
    s, _, _, _, floor, H = _dense(name)
    n, d = s["n"], s["dim"]
    scale = np.abs(H).max()
    assert np.abs(H - H.T).max() <= 1e-14 * scale
    HT = hr.translations(n, d).reshape(d, -1) @ H
    assert np.abs(HT).max() <= 1e-12 * scale
    print("%s: N = %d, max |H| = %.6g, fp64 rounding floor %.3e" % (name, n, scale, floor))
    assert floor < 1e-13


@pytest.mark.parametrize("name", ["poly", "xplor"])
def test_hv_against_a_central_difference_of_the_oracles_forces(oracle, name):
    """Both potentials are smooth at their cutoff.  -H v = dF/d(eps) along v; eps = 1e-5 leaves a truncation error of
    eps^2 |F'''| / 6 ~ 1e-10 x the third derivative's scale (about 1e5 |H v| here at close contacts): 1e-6 relative."""
    s, cutoff, kind, params, _, H = _dense(name)
    n, d = s["n"], s["dim"]
    pot = oracle.make_pot(kind, params)
    v = np.random.default_rng(2).uniform(-1.0, 1.0, (n, d))
    eps = 1e-5
    fp = oracle.forces_brute(s["x"] + eps * v, s["box"], cutoff, pot, s["diam"])[0]
    fm = oracle.forces_brute(s["x"] - eps * v, s["box"], cutoff, pot, s["diam"])[0]
    hv = (H @ v.reshape(-1)).reshape(n, d)
    err = np.abs((fp - fm) / (2 * eps) + hv).max()
    print("%s: |dF/2eps + H v| = %.3e, max |H v| = %.4g" % (name, err, np.abs(hv).max()))
    assert err <= 1e-6 * np.abs(hv).max()


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("name", ["lj", "polydisperse", "lj_xplor", "pseudohs"])
def test_isolated_dimer(name, dim):
    """H = [[B, -B], [-B, B]] with B = (k - t) n n^T + t I: eigenvalues 2 k, 2 t (d - 1 times) and d zeros -- k and t of the
    relative coordinate, doubled by the two equal masses."""
    kind, params, branches, (s1, s2) = POTENTIALS[name]
    r = 0.97 if kind != hr.POT_POLYDISPERSE else 0.9
    dirn = np.array([0.6, 0.8, 0.0])[:dim] if dim == 2 else np.array([2.0, -1.0, 2.0]) / 3.0
    x = np.stack([np.full(dim, 3.0), np.full(dim, 3.0) + r * dirn])
    H = hr.dense(x, np.eye(dim) * 20.0, 3.0, kind, params, [s1, s2])
    t, k, _ = (float(v) for v in hr.pair_tk(kind, params, np.linalg.norm(x[1] - x[0]), s1, s2))
    w = np.sort(np.linalg.eigvalsh(H))
    want = np.sort([2 * k] + [2 * t] * (dim - 1) + [0.0] * dim)
    assert np.abs(w - want).max() <= 1e-12 * max(abs(k), abs(t)), (w, want)


def test_fcc_crystal_site_blocks_are_equal_and_isotropic():
    """A perfect fcc Lennard-Jones crystal: every site has the same surroundings with cubic symmetry, so H_ii = c I."""
    m, rho = 4, 1.0
    a = (4.0 / rho) ** (1.0 / 3.0)
    base = np.array([[0, 0, 0], [0.5, 0.5, 0], [0.5, 0, 0.5], [0, 0.5, 0.5]])
    cells = np.stack(np.meshgrid(*[np.arange(m)] * 3, indexing="ij"), -1).reshape(-1, 1, 3)
    x = ((cells + base[None]) * a).reshape(-1, 3)
    n = len(x)
    H = hr.dense(x, np.eye(3) * (m * a), 2.5, hr.POT_LJ, [1.0, 1.0, 2.5], np.ones(n))
    B = hr.diagonal_blocks(H, n, 3)
    c = B[0, 0, 0]
    assert c > 0.0
    assert np.abs(B - c * np.eye(3)[None]).max() <= 1e-11 * c


@pytest.mark.parametrize("name", ["poly", "xplor", "lj"])
def test_one_missing_pair_is_far_above_the_tolerance(name):
    """Leaving a pair out moves entries of H by that pair's block: O(1) of a block.  Relative to max |H| -- which the
    closest contact of these jittered lattices sets -- the weakest pair of a frame (the one nearest the cutoff) still moves H
    by more than 1e-5, nine orders above the comparison tolerance of 10 x the rounding floor."""
    s, cutoff, kind, params, floor, H = _dense(name)
    U = np.diag(s["box"])
    pairs = hr.pair_list(s["x"], U, cutoff)
    B, inside = hr.pair_blocks(kind, params, s["diam"], *pairs)
    scale = np.abs(H).max()
    effect = np.abs(B).max(axis=(1, 2)) / scale
    live = np.flatnonzero(inside)
    weakest = int(live[np.argmin(effect[live])])
    Hd = hr.dense(s["x"], U, cutoff, kind, params, s["diam"], drop=weakest, pairs=pairs)
    seen = np.abs(Hd - H).max() / scale
    print("%s: %d pairs; leaving out the weakest changes H by %.3e of max |H| (median pair %.3e); tolerance %.3e"
          % (name, len(live), seen, np.median(effect[live]), 10 * floor))
    assert abs(seen - effect[live].min()) <= 1e-12
    assert seen >= 1e-5 and seen >= 1e8 * (10 * floor)


# ---------------------------------------------------------------------------------------------------------------------
# the Python layer on a stub device
# ---------------------------------------------------------------------------------------------------------------------
class _StubDevice:
    """hess_* in numpy on a given dense H: what MDDevice promises, nothing of how it computes it."""
    HESS_MAX_BLOCK = 8

    def __init__(self, H, n, dim):
        self.H, self.n, self.dim = H, n, dim
        self.frozen = False
        self.calls = []

    def set_potential(self, kind, params):
        self.calls.append(("set_potential", kind))

    def upload(self, **kw):
        self.calls.append(("upload", tuple(sorted(kw))))
        self.frozen = False

    def hess_setup(self):
        self.calls.append(("hess_setup",))
        self.frozen = True

    def _need(self):
        if not self.frozen:
            raise md.MdhipError("md_hess_apply: no operator for the frame the handle holds now: call md_hess_setup")

    def hess_apply(self, X):
        self._need()
        assert X.ndim == 3 and 1 <= X.shape[0] <= 8
        self.calls.append(("hess_apply", X.shape[0]))
        return (X.reshape(X.shape[0], -1) @ self.H).reshape(X.shape)

    def hess_blocks(self):
        self._need()
        return hr.diagonal_blocks(self.H, self.n, self.dim)

    def hess_lanczos(self, k, seed=0):
        self._need()
        nd = self.n * self.dim
        Q = [t for t in hr.translations(self.n, self.dim).reshape(self.dim, -1)]
        w = np.random.default_rng(seed).uniform(-1, 1, nd)
        V, alpha, beta = [], np.zeros(k), np.zeros(k)
        for _ in range(2):
            w = w - sum((q @ w) * q for q in Q)
        V.append(w / np.linalg.norm(w))
        for j in range(k):
            w = self.H @ V[j]
            for p in range(2):
                c = [q @ w for q in Q + V]
                alpha[j] += c[-1]
                w = w - sum(ci * q for ci, q in zip(c, Q + V))
            beta[j] = np.linalg.norm(w)
            if j + 1 < k:
                V.append(w / beta[j])
        self.V = np.array(V)
        self.calls.append(("hess_lanczos", k, seed))
        return alpha, beta

    def hess_ritz(self, S, theta):
        self._need()
        Y = S.T @ self.V
        R = Y @ self.H - theta[:, None] * Y
        return Y.reshape(-1, self.n, self.dim), np.linalg.norm(R, axis=1)


def _stub_state(name="poly", H=None):
    s, cutoff, kind, params, _, Href = _dense(name)
    n, d = s["n"], s["dim"]
    dev = _StubDevice(Href if H is None else H, n, d)
    system = types.SimpleNamespace(device=dev, positions=np.array(s["x"]), xpositions=None,
                                   energy_and_forces=types.SimpleNamespace(forces=np.zeros((n, d)), energy=0.0, virial=0.0))
    state = md.SimulationState(system, np.array(s["diam"]), np.random.default_rng(1), np.diag(s["box"]), np.zeros((n, d)),
                               np.zeros((n, d), dtype=np.int32), d, d * (n - 1.0))
    pot = md.Polydisperse(1.25, 0.2) if name == "poly" else md.LennardJones()
    return state, md.Parameters(1.0, n, 0.002, pot), dev, Href


def test_operator_on_a_stub_device(monkeypatch):
    state, params, dev, H = _stub_state()
    n, d = dev.n, dev.dim
    op = md.HessianOperator(state, params)
    assert [c[0] for c in dev.calls] == ["set_potential", "upload", "hess_setup"] and op.shape == (n * d, n * d)
    X = np.random.default_rng(0).standard_normal((19, n, d))
    dev.calls.clear()
    Y = op.matvec(X)
    assert [c[1] for c in dev.calls] == [8, 8, 3]                               # any m, in blocks of 8
    assert np.allclose(Y.reshape(19, -1), X.reshape(19, -1) @ H, rtol=0, atol=1e-9)
    assert op.matvec(X[0]).shape == (n, d) and np.allclose(op.matvec(X[0]), Y[0], rtol=0, atol=1e-9)
    assert np.allclose(op.dense(), H, rtol=0, atol=1e-9) and np.array_equal(op.blocks(), hr.diagonal_blocks(H, n, d))
    for bad in (np.zeros((n, d + 1)), np.zeros((2, n + 1, d)), np.zeros(n * d)):
        with pytest.raises(ValueError):
            op.matvec(bad)
    monkeypatch.setattr(vibrations, "DENSE_MAX_DOF", n * d - 1)
    with pytest.raises(ValueError, match="dense"):
        op.dense()
    dev.upload(x=state.system.positions)                                         # the frame changes on the handle
    with pytest.raises(md.MdhipError, match="md_hess_setup"):
        op.matvec(X[0])


def test_user_potentials_are_refused_by_the_python_layer():
    state, params, dev, _ = _stub_state()

    class UserPotential(md.Potential):
        def device_spec(self):
            return ("source", "src", "entry", ())

    with pytest.raises(ValueError, match="built-in"):
        md.HessianOperator(state, md.Parameters(1.0, dev.n, 0.002, UserPotential()))
    assert dev.calls == []


def test_lowest_modes_on_a_stub_device():
    state, params, dev, H = _stub_state()
    n, d = dev.n, dev.dim
    T = hr.translations(n, d).reshape(d, -1)
    normH = np.abs(np.linalg.eigvalsh(H)).max()
    w = np.linalg.eigvalsh(H + 10 * normH * T.T @ T)
    res = md.lowest_modes(state, params, 6, tol=1e-9, k0=16)
    ks = [c[1] for c in dev.calls if c[0] == "hess_lanczos"]
    assert ks == [min(16 * 2 ** i, n * d - d) for i in range(len(ks))] and res["ksteps"] == ks[-1]    # doubling, same seed
    assert len({c[2] for c in dev.calls if c[0] == "hess_lanczos"}) == 1
    assert res["converged"] and np.all(res["residuals"] <= 1e-9 * res["norm"])
    assert np.abs(res["eigenvalues"] - w[:6]).max() <= 1e-8 * normH
    assert res["stable"] is False and res["eigenvalues"][0] < 0.0               # the lattice start is no minimum
    assert np.isnan(res["frequencies"][0]) and res["modes"].shape == (6, n, d)
    assert np.allclose(res["participation"], md.participation_ratio(res["modes"])) and np.all(res["participation"] <= 1.0)
    # a positive definite operator (apart from the translations) is stable
    P = np.eye(n * d) - T.T @ T
    state2, params2, dev2, _ = _stub_state(H=P @ (H + (1.0 - w[0]) * np.eye(n * d)) @ P)
    res2 = md.lowest_modes(state2, params2, 3, k0=32)
    assert res2["stable"] is True and np.all(res2["frequencies"] > 0.0)
    assert abs(res2["eigenvalues"][0] - 1.0) <= 1e-7 * normH
    # kmax reached without convergence is reported, not raised
    res3 = md.lowest_modes(state, params, 6, tol=1e-14, k0=8, kmax=8)
    assert res3["ksteps"] == 8 and res3["converged"] is False
    for kw in (dict(nmodes=0), dict(nmodes=n * d), dict(nmodes=4, tol=0.0), dict(nmodes=4, kmax=3), dict(nmodes=4, k0=2)):
        with pytest.raises(ValueError):
            md.lowest_modes(state, params, **kw)


def test_participation_ratio_limits():
    n = 50
    one = np.zeros((n, 3))
    one[7, 1] = 1.0
    allp = np.full((n, 3), 1.0)
    assert md.participation_ratio(one[None])[0] == pytest.approx(1.0 / n)
    assert md.participation_ratio(allp[None])[0] == pytest.approx(1.0)
