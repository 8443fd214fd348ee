"""-m gpu: md_set_cell (both modes), md_nonaffine_* and the AQS loop on the device against tests/cell_reference.py, the
oracle's brute-force pair loop and the linear-response prediction of tests/elas_reference.py.

Frames (tests/test_gpu_hessian.py's): lj_raw (N = 500, a ragged last tile), tric512 (N = 512 in a sheared cell), poly1200
(2-D, per-particle diameters), poly256 (2-D, relaxed by the device's FIRE).

Tolerances.  Positions and images after a cell change: bit for bit against the restatement.  Forces, U, W against the
oracle: tests/test_gpu_parity.py's (|dF| <= 1e-11 max(1, |F|), U and W relative 1e-12).  Unwrapped positions across a flip:
cell_reference.unwrapped_bound.  Non-affine displacements: test_deformation.u_bound.  Both derived where they are defined."""
import numpy as np
import pytest

from oracle import oracle
from tests import cell_reference as cr
from tests import elas_reference as er
from tests import hess_reference as hr
from tests.test_deformation import u_bound
from tests.test_gpu_hessian import frame, state_of

pytestmark = pytest.mark.gpu

EPS = cr.EPS


def _device(fr, cell=None):
    from moleculardynamics.jl_amd import MDDevice
    s = fr["system"]
    dev = MDDevice(s["dim"], s["n"], hr.lattice(s.get("cell", s["box"]), s["dim"]) if cell is None else cell, fr["cutoff"])
    dev.set_potential(fr["kind"], fr["params"])
    return dev


def _cell0(fr):
    s = fr["system"]
    return np.array(hr.lattice(s.get("cell", s["box"]), s["dim"]), dtype=np.float64)


def _brute(fr, x, U):
    """(f, u, w, sorted pairs) of the oracle's brute-force loop for wrapped positions x in the cell U"""
    s = fr["system"]
    pot = oracle.make_pot(fr["kind"], fr["params"])
    if cr.is_general(U):
        with oracle.set_cell(U):
            f, u, w, pairs = oracle.forces_brute(x, np.ones(s["dim"]), fr["cutoff"], pot, s["diam"], want_pairs=True)
    else:
        f, u, w, pairs = oracle.forces_brute(x, np.diag(U).copy(), fr["cutoff"], pot, s["diam"], want_pairs=True)
    return f, u, w, pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))]


def _check_against_oracle(fr, dev, U, what):
    """md_neighbor_pairs equal to the oracle's pair set in the cell U; forces, U, W within test_gpu_parity.py's tolerance"""
    u, w = dev.compute_forces()
    x, _, f, _ = dev.download()
    pairs = dev.neighbor_pairs()
    f_ref, u_ref, w_ref, pairs_ref = _brute(fr, x, U)
    assert np.array_equal(pairs, pairs_ref), what
    err = np.abs(f - f_ref).max()
    print("%s: %d pairs; |dF| %.3e (allowed %.3e), dU/U %.3e, dW/W %.3e"
          % (what, len(pairs), err, 1e-11 * max(1.0, np.abs(f_ref).max()), abs(u - u_ref) / abs(u_ref), abs(w - w_ref) / abs(w_ref)))
    assert err <= 1e-11 * max(1.0, np.abs(f_ref).max()), what
    assert abs(u - u_ref) <= 1e-12 * abs(u_ref) and abs(w - w_ref) <= 1e-12 * abs(w_ref), what
    return u, w, f


def _scattered(fr, seed=4):
    """The frame as a lazy wrap may hold it: a fifth of the particles moved out of the cell by whole lattice vectors, image
    counts non-zero everywhere and +-10^6 for every seventh particle."""
    s = fr["system"]
    n, d = s["n"], s["dim"]
    rng = np.random.default_rng(seed)
    U = _cell0(fr)
    k = rng.integers(-2, 3, (n, d)) * (rng.random((n, 1)) < 0.2)
    x = s["x"] + k @ U.T
    img = rng.integers(-3, 4, (n, d))
    img[::7] = rng.choice([-10 ** 6, 10 ** 6], (len(img[::7]), d))
    return np.ascontiguousarray(x), img.astype(np.int32)


def _new_cells(fr):
    """A diagonal and a general cell near the frame's own: a few per cent of strain, every face distance >= 3 cutoffs"""
    U = _cell0(fr)
    d = U.shape[0]
    L = np.abs(np.diag(U))
    D = np.diag(L * np.array([1.02, 0.99, 1.01])[:d])
    G = D.copy()
    G[0, 1] = 0.17 * L[1]
    if d == 3:
        G[0, 2], G[1, 2] = -0.05 * L[2], 0.08 * L[2]
    for W in (D, G):
        assert cr.face_distances(W).min() >= 3.0 * fr["cutoff"]
    return D, G


# ---------------------------------------------------------------------------------------------------------------------
# 1. the affine mode, bit for bit, through all four transitions in 2-D and 3-D
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,start", [("lj_raw", "diag"), ("tric512", "general"), ("poly1200", "diag"), ("poly1200", "general")])
def test_affine_mode_bit_for_bit(name, start):
    fr = frame(name)
    s = fr["system"]
    d = s["dim"]
    U0 = _cell0(fr)
    D, G = _new_cells(fr)
    x, img = _scattered(fr)
    z = np.zeros_like(x)
    with _device(fr) as dev:
        if start == "general" and not cr.is_general(U0):
            # (poly1200 has no general cell of its own: give it one, affinely, and start from what the handle then holds)
            U0 = G * 0.995
            dev.upload(s["x"], z, z, np.zeros_like(img), s["diam"])
            dev.set_cell(U0)
            x0 = dev.download()[0]
            k = np.random.default_rng(9).integers(-2, 3, x.shape) * (np.random.default_rng(10).random((len(x), 1)) < 0.2)
            x = np.ascontiguousarray(x0 + k @ U0.T)
        assert cr.is_general(U0) == (start == "general")
        for target, U1 in (("general" if start == "diag" else "diag", G if start == "diag" else D),
                           (start, D * 1.003 if start == "diag" else G * 1.003)):
            if not np.array_equal(dev.unitcell, U0):
                dev.set_cell(U0, dev.CELL_AFFINE)
            dev.upload(x, z, z, img, s["diam"])
            dev.set_cell(U1, dev.CELL_AFFINE)
            xd, _, _, imd = dev.download()
            xr, ir = cr.export_wrap(*cr.affine(x, img, U0, U1), U1)
            what = "%s %s -> %s" % (name, start, target)
            assert np.array_equal(imd, ir.astype(np.int32)), what
            assert np.array_equal(xd, xr), (what, np.abs(xd - xr).max())
            assert np.abs(imd).max() >= 10 ** 6 - 4
            assert np.array_equal(dev.unitcell, U1) and cr.is_general(U1) == (target == "general")
            _check_against_oracle(fr, dev, U1, what)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the lattice mode
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("target", ["general", "diag"])
@pytest.mark.parametrize("name", ["lj_raw", "poly1200"])
def test_lattice_flip(name, target):
    """target "general": sheared past half a box length, flipped to the reduced (still general) cell.  target "diag": sheared
    by exactly one lattice vector (both boxes have equal edges), so the reduced cell is the orthorhombic box itself and the
    kernel takes its diagonal wrap.  Forces, U and W before and after the flip: tests/test_gpu_parity.py's tolerance."""
    import moleculardynamics.jl_amd as md
    from moleculardynamics.jl_amd import MdhipError
    fr = frame(name)
    s = fr["system"]
    d = s["dim"]
    U0 = _cell0(fr)
    if target == "diag":
        assert U0[0, 0] == U0[1, 1]
        U1 = md.simple_shear(d, 1.0) @ U0
    else:
        U1 = md.simple_shear(d, 0.7) @ U0                              # past half a box length
        if d == 3:
            U1 = md.simple_shear(d, -0.6, plane=(1, 2)) @ U1
    assert cr.face_distances(U1).min() >= 3.0 * fr["cutoff"]
    W, M = md.gauss_reduce(U1)
    assert not np.array_equal(M, np.eye(d, dtype=np.int64))
    assert cr.is_general(W) == (target == "general") and (target == "general" or np.array_equal(W, U0))
    x, img = _scattered(fr)
    z = np.zeros_like(x)
    with _device(fr) as dev:
        dev.upload(x, z, z, img, s["diam"])
        dev.set_cell(U1, dev.CELL_AFFINE)
        xa, _, _, ia = dev.download()
        dev.upload(xa, z, z, ia, s["diam"])          # (the handle now stores exactly the frame a download shows)
        u0, w0, f0 = _check_against_oracle(fr, dev, U1, "%s sheared (%s)" % (name, target))
        half = U1.copy()
        half[:, 1] += 0.5 * U1[:, 0]
        for bad, why in ((2.0 * U1, "det"), (half, "integer"), (W * (1.0 + 1e-7), "integer")):
            with pytest.raises(MdhipError, match="MD_CELL_LATTICE") as ei:
                dev.set_cell(bad, dev.CELL_LATTICE)
            assert why in str(ei.value)
            xb, _, fb, ib = dev.download()
            assert np.array_equal(xb, xa) and np.array_equal(ib, ia) and np.array_equal(fb, f0) and np.array_equal(dev.unitcell, U1)
        dev.set_cell(W, dev.CELL_LATTICE)
        xd, _, _, imd = dev.download()
        u1, w1, f1 = _check_against_oracle(fr, dev, W, "%s flipped (%s)" % (name, target))
    xr, ir, _ = cr.lattice(xa, ia, U1, W)
    assert np.array_equal(imd, ir.astype(np.int32))
    bound = cr.unwrapped_bound([U1, W], [ia, imd])
    err = np.abs(cr.unwrapped(xd, imd, W) - cr.unwrapped(xa, ia, U1)).max()
    print("%s: flip M = %s; |x + U img| changed by %.3e (allowed %.3e); |dF| %.3e, dU/U %.3e, dW/W %.3e"
          % (name, M.tolist(), err, bound, np.abs(f1 - f0).max(), abs(u1 - u0) / abs(u0), abs(w1 - w0) / abs(w0)))
    assert err <= bound
    assert np.abs(f1 - f0).max() <= 1e-11 * max(1.0, np.abs(f0).max())
    assert abs(u1 - u0) <= 1e-12 * abs(u0) and abs(w1 - w0) <= 1e-12 * abs(w0)


def test_python_layer_on_a_live_state():
    """set_unitcell / deform / reduce_cell: the handle stays the same object, the host copies follow, params is untouched"""
    import moleculardynamics.jl_amd as md
    fr = frame("poly1200")
    state, params = state_of(fr)
    rho = params.ρ
    U0 = np.array(state.unitcell)
    x0 = np.array(state.system.positions)
    with state.system.device as dev:
        assert md.reduce_cell(state, params) is None
        md.deform(state, params, md.simple_shear(2, 0.7))
        assert state.system.device is dev and np.array_equal(state.unitcell, md.simple_shear(2, 0.7) @ U0)
        xr, ir = cr.export_wrap(*cr.affine(x0, np.zeros(x0.shape, dtype=np.int64), U0, state.unitcell), state.unitcell)
        assert np.array_equal(state.system.positions, xr) and np.array_equal(state.images, ir)
        M = md.reduce_cell(state, params)
        assert np.array_equal(M, np.array([[1, -1], [0, 1]]))
        assert abs(state.unitcell[0, 1] - (0.7 - 1.0) * U0[1, 1]) <= 4 * EPS * U0[1, 1]
        assert np.array_equal(dev.unitcell, state.unitcell) and params.ρ == rho
        # back: the sheared cell again (the same lattice, not reduced), then the strain undone
        U1 = md.simple_shear(2, 0.7) @ U0
        md.set_unitcell(state, params, U1, remap="lattice")
        md.set_unitcell(state, params, U0, remap="affine")
        back = np.abs(cr.unwrapped(state.system.positions, state.images, U0) - x0).max()
        assert back <= cr.unwrapped_bound([U0, U1, state.unitcell, U1, U0], [state.images + 1] * 5)
        with pytest.raises(ValueError):
            md.set_unitcell(state, params, U0, remap="rigid")


# ---------------------------------------------------------------------------------------------------------------------
# 3. refusals leave the handle untouched
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_untouched():
    import moleculardynamics.jl_amd as md
    from moleculardynamics.jl_amd import MdhipError
    fr = frame("lj_raw")
    s = fr["system"]
    U0 = _cell0(fr)
    x, img = _scattered(fr)
    z = np.zeros_like(x)
    with _device(fr) as dev:
        dev.upload(x, s["v"], z, img, s["diam"])
        u0, w0 = dev.compute_forces()
        before = dev.download()
        pairs0 = dev.neighbor_pairs()

        def untouched(what):
            after = dev.download()
            for a, b in zip(before, after):
                assert np.array_equal(a, b), what
            assert dev.compute_forces() == (u0, w0), what
            assert np.array_equal(dev.download()[2], before[2]), what
            assert np.array_equal(dev.unitcell, U0), what

        too_far = md.simple_shear(3, 2.0) @ U0
        assert cr.face_distances(too_far).min() < 3.0 * fr["cutoff"]
        for mode in (dev.CELL_AFFINE, dev.CELL_LATTICE):
            with pytest.raises(MdhipError, match="face distance"):
                dev.set_cell(too_far, mode)
            untouched("face distance")
            with pytest.raises(MdhipError, match="singular"):
                dev.set_cell(np.array([[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [0.0, 0.0, 5.0]]), mode)
            untouched("singular")
            with pytest.raises(MdhipError, match="finite"):
                dev.set_cell(np.array([[np.nan, 0.0, 0.0], [0.0, 8.0, 0.0], [0.0, 0.0, 8.0]]), mode)
            untouched("not finite")
        with pytest.raises(MdhipError, match="mode"):
            dev.set_cell(U0, 7)
        dev.snapshot_begin()
        with pytest.raises(MdhipError, match="in flight"):
            dev.set_cell(1.01 * U0)
        dev.snapshot_end()
        untouched("snapshot")
        dev.dyn_setup(1, 1)
        with pytest.raises(MdhipError, match="md_dyn"):
            dev.set_cell(1.01 * U0)
        untouched("md_dyn")
        assert np.array_equal(dev.neighbor_pairs(), pairs0)
        with pytest.raises(MdhipError, match="no mark"):
            dev.nonaffine()
        dev.nonaffine_mark()
        dev.nonaffine()
        dev.upload(x=x)
        with pytest.raises(MdhipError, match="no mark"):                 # an upload of positions discards the mark
            dev.nonaffine()


def test_image_overflow_is_refused_before_anything_is_written():
    """MD_CELL_LATTICE with an image count that would leave int32 in the new basis: the pass that writes nothing finds it,
    the call is refused and the handle (frame, forces, cell and mark) is as before -- once for the state's own images,
    once for the images a mark holds."""
    import moleculardynamics.jl_amd as md
    from moleculardynamics.jl_amd import MdhipError
    fr = frame("lj_raw")
    s = fr["system"]
    n, d = s["n"], s["dim"]
    U0 = _cell0(fr)
    U1 = md.simple_shear(d, 0.7) @ U0
    W, M = md.gauss_reduce(U1)
    Mi = cr.integer_inverse(M)
    assert np.array_equal(Mi[0], [1, 1, 0])                             # img'_x = img_x + img_y
    small = np.random.default_rng(2).integers(-3, 4, (n, d)).astype(np.int32)
    big = small.copy()
    big[n - 1] = [2 ** 31 - 2, 5, 0]                                    # (the last particle: the ragged tile's)
    z = np.zeros_like(s["x"])
    with pytest.raises(OverflowError):
        cr.lattice(s["x"] @ md.simple_shear(d, 0.7).T, big, U1, W)
    with _device(fr) as dev:
        dev.upload(s["x"], z, z, big, s["diam"])
        dev.set_cell(U1)
        u0, w0 = dev.compute_forces()
        before = dev.download()
        assert before[3][n - 1, 0] == 2 ** 31 - 2

        def untouched(what):
            after = dev.download()
            for a, b in zip(before[:3], after[:3]):
                assert np.array_equal(a, b), what
            assert dev.compute_forces() == (u0, w0) and np.array_equal(dev.unitcell, U1), what
            return after[3]

        with pytest.raises(MdhipError, match="int32"):
            dev.set_cell(W, dev.CELL_LATTICE)
        assert np.array_equal(untouched("state images"), before[3])
        # the same through the mark: it keeps the large counts, the state gets small ones
        dev.nonaffine_mark()
        dev.upload(images=small)
        na0 = dev.nonaffine(fields=True)
        with pytest.raises(MdhipError, match="int32"):
            dev.set_cell(W, dev.CELL_LATTICE)
        assert np.array_equal(untouched("mark images"), small)
        na1 = dev.nonaffine(fields=True)
        assert np.array_equal(na0["u"], na1["u"]) and np.array_equal(na0["sums"], na1["sums"])
        # a new mark on the small counts, and the flip goes through
        dev.nonaffine_mark()
        dev.set_cell(W, dev.CELL_LATTICE)
        _, ir, _ = cr.lattice(before[0], small, U1, W)
        assert np.array_equal(dev.download()[3], ir.astype(np.int32))
        assert np.abs(dev.nonaffine(fields=True)["u"]).max() <= u_bound(W, 1.0, np.abs(Mi).max()) + u_bound(U1, 1.0)


def test_frame_samplers_follow_the_cell():
    """g(r) and the pressure tensor sampled after a cell change are those of a fresh handle in the new cell"""
    fr = frame("lj_raw")
    s = fr["system"]
    U0 = _cell0(fr)
    _, G = _new_cells(fr)
    z = np.zeros_like(s["x"])
    with _device(fr) as dev:
        dev.rdf_setup(1.4, 40)
        dev.stress_setup(0)
        dev.upload(s["x"], s["v"], z, s["img"], s["diam"])
        dev.set_cell(G)
        dev.rdf_sample()
        dev.stress_sample()
        counts, ns = dev.rdf_read()
        kin, vir = dev.stress_tensor()
        xg = dev.download()[0]
    with _device(fr, cell=G) as ref:
        ref.rdf_setup(1.4, 40)
        ref.stress_setup(0)
        ref.upload(xg, s["v"], z, s["img"], s["diam"])
        ref.rdf_sample()
        ref.stress_sample()
        counts_ref, _ = ref.rdf_read()
        kin_ref, vir_ref = ref.stress_tensor()
    assert ns == 1 and np.array_equal(counts, counts_ref) and counts.sum() > 0
    assert np.array_equal(kin, kin_ref)
    assert np.abs(vir - vir_ref).max() <= 1e-11 * np.abs(vir_ref).max()


# ---------------------------------------------------------------------------------------------------------------------
# 4. the non-affine displacement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gamma", [0.6, 1.0])
@pytest.mark.parametrize("name", ["lj_raw", "poly1200"])
def test_nonaffine_displacement(name, gamma):
    """gamma 0.6: the flip goes to a general cell; gamma 1.0 (one whole lattice vector): back to the orthorhombic box"""
    import moleculardynamics.jl_amd as md
    fr = frame(name)
    s = fr["system"]
    n, d = s["n"], s["dim"]
    U0 = _cell0(fr)
    U1 = md.simple_shear(d, gamma) @ U0
    W, M = md.gauss_reduce(U1)
    assert cr.is_general(W) == (gamma != 1.0)
    Mi = cr.integer_inverse(M)
    x, img = _scattered(fr)
    with _device(fr) as dev:
        dev.upload(x, s["v"], np.zeros_like(x), img, s["diam"])
        dev.nonaffine_mark()
        dev.set_cell(U1)
        na0 = dev.nonaffine(fields=True)
        dev.run(20, 0.002)
        xa, _, _, ia = dev.download()
        na1 = dev.nonaffine(fields=True)
        dev.set_cell(W, dev.CELL_LATTICE)
        xb, _, _, ib = dev.download()
        na2 = dev.nonaffine(fields=True)
        na3 = dev.nonaffine()
    mark = cr.mark_of(x, img, U0)
    fmax = max(np.abs(mark[0]).max(), 3.0)
    b0 = u_bound(U1, fmax)
    print("%s: max |u| right after the affine strain %.3e (allowed %.3e)" % (name, np.abs(na0["u"]).max(), b0))
    assert np.abs(na0["u"]).max() <= b0 and na0["n"] == n
    # after the run, before the flip: the restatement on the downloaded frame (the device holds the same particles up to
    # whole lattice vectors the lazy wrap has not applied yet, which frac + img does not see beyond rounding)
    u_ref, sums_ref = cr.nonaffine(xa, ia, U1, mark)
    assert np.abs(na1["u"] - u_ref).max() <= 2 * b0
    assert np.abs(u_ref).max() > 1e-3                                  # (twenty steps moved everybody)
    # after the flip
    xr, ir, mark2 = cr.lattice(xa, ia, U1, W, mark=mark)
    assert np.array_equal(ib, ir.astype(np.int32))
    u_ref2, sums_ref2 = cr.nonaffine(xb, ib, W, mark2)
    b2 = 2 * b0 + u_bound(W, max(fmax, np.abs(mark2[0]).max()), np.abs(Mi).max())
    err = np.abs(na2["u"] - u_ref2).max()
    print("%s: |u - restatement| after the flip %.3e, |u after - u before| %.3e (allowed %.3e)"
          % (name, err, np.abs(na2["u"] - na1["u"]).max(), b2))
    assert err <= b2 and np.abs(na2["u"] - na1["u"]).max() <= b2
    # the sums: every term within its particle's bound, plus the rounding of a sum of n terms
    sd, umax = na2["sums"], np.sqrt(sums_ref2[5])
    assert na2["argmax"] == int(sums_ref2[6]) and na2["n"] == n and sd[7] == n
    assert np.abs(sd[:d] - sums_ref2[:d]).max() <= n * b2 + n * EPS * np.abs(u_ref2).sum()
    assert abs(sd[3] - sums_ref2[3]) <= n * (2 * d * umax * b2) + n * EPS * sums_ref2[3]
    assert abs(sd[4] - sums_ref2[4]) <= n * (4 * d * umax ** 3 * b2) + n * EPS * sums_ref2[4]
    assert abs(sd[5] - sums_ref2[5]) <= 2 * d * umax * b2 + 4 * EPS * sums_ref2[5]
    if d == 2:
        assert sd[2] == 0.0
    assert sd[5] == (na2["u"] ** 2).sum(axis=1).max() or abs(sd[5] - (na2["u"] ** 2).sum(axis=1).max()) <= 4 * EPS * sd[5]
    assert np.array_equal(na3["sums"], na2["sums"])                   # reproducible, with and without the field


# ---------------------------------------------------------------------------------------------------------------------
# 5. the elastic branch against linear response, on one handle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["poly256", "xplor_tric"])
def test_second_difference_in_place(name):
    """tests/test_gpu_elasticity.py::test_second_difference_through_fire with md_set_cell in place of fresh handles: its h
    values, its prediction and its acceptance rule (10 x the error of the same difference taken with the reference's relaxer
    and the reference's C).  The fresh-handle energies must agree with the in-place ones to the same rule."""
    import moleculardynamics.jl_amd as md
    from tests.test_gpu_elasticity import _fire, _ref_args, _vec, eframe, moduli_ref
    fr = eframe(name)
    m = moduli_ref(name)
    s = fr["system"]
    n, d = s["n"], s["dim"]
    U0 = np.array(hr.lattice(s.get("cell", s["box"]), d), dtype=np.float64)
    V, a = m["a64"]["volume"], m["a64"]
    spec = fr["pot"].device_spec()
    z = np.zeros((n, d))
    zi = np.zeros((n, d), dtype=np.int32)

    def fresh(x, cell):
        with md.MDDevice(d, n, cell, fr["cutoff"]) as dev:
            dev.set_potential(spec[1], spec[2])
            dev.upload(x, z, z, zi, s["diam"])
            r = _fire(dev, name)
            assert r["converged"], r
            return r["energy"]

    state, params = state_of(fr)
    with state.system.device:
        res = md.elastic_moduli(state, params)
    assert res["stable"]
    e0_ref = er.energy_forces(*_ref_args(fr), dtype=np.longdouble)[0]
    shear = np.zeros((d, d))
    shear[0, 1] = 1.0
    rows = []
    with md.MDDevice(d, n, U0, fr["cutoff"]) as dev:
        dev.set_potential(spec[1], spec[2])

        def in_place(F):
            dev.set_cell(U0)                              # back to the frame's own cell, then the frame, then the strain
            dev.upload(s["x"], z, z, zi, s["diam"])
            dev.set_cell(F @ U0)
            r = _fire(dev, name)
            assert r["converged"], r
            return r["energy"]

        e0 = in_place(np.eye(d))
        assert abs(e0 - float(e0_ref)) <= 1e-10 * abs(e0)
        for label, E in (("shear", shear), ("isotropic", np.eye(d))):
            pred_dev = er.second_difference_prediction(res["moduli"], _vec(res["stress"], d), E, res["volume"], d)
            pred_ref = er.second_difference_prediction(m["C"], a["stress"], E, V, d)
            for h in (1e-3, 3e-4):
                ed, ef, erf = [], [], []
                for sign in (1.0, -1.0):
                    F = np.eye(d) + sign * h * E
                    xs, Us = er.strained(s["x"], U0, F)
                    xr, g, _ = er.relax(*_ref_args(fr, xs, Us))
                    assert g <= 1e-12
                    erf.append(er.energy_forces(*_ref_args(fr, xr, Us), dtype=np.longdouble)[0])
                    ed.append(in_place(F))
                    ef.append(fresh(xs, Us))
                hh = np.longdouble(h)
                err_ref = abs(float((erf[0] - 2 * e0_ref + erf[1]) / hh ** 2) - pred_ref) / abs(pred_ref)
                sd_dev = (ed[0] - 2.0 * e0 + ed[1]) / h ** 2
                sd_fresh = (ef[0] - 2.0 * e0 + ef[1]) / h ** 2
                err_dev = abs(sd_dev - pred_dev) / abs(pred_dev)
                err_ff = abs(sd_dev - sd_fresh) / abs(pred_dev)
                print("%s/%s h = %g: prediction %.8g; relative error in place %.3e, reference %.3e (allowed %.3e); in place "
                      "against fresh handles %.3e" % (name, label, h, pred_dev, err_dev, err_ref, 10 * err_ref, err_ff))
                rows.append((label, h, err_dev, err_ff, err_ref))
    for label, h, err_dev, err_ff, err_ref in rows:
        assert err_dev <= 10 * err_ref, (label, h)
        assert err_ff <= 10 * err_ref, (label, h)
    for label, h, err_dev, err_ff, err_ref in rows:
        if h == 3e-4:
            assert err_ref <= 1e-3, (label, h)


# ---------------------------------------------------------------------------------------------------------------------
# 6. the AQS loop against the CPU reference
# ---------------------------------------------------------------------------------------------------------------------
def test_aqs_against_the_cpu_reference(tmp_path):
    """Energy, stress and d2_nonaffine of every increment against cell_reference.aqs_reference on the poly256 frame.
    Allowed: 10 x |reference at tol - reference at tol / 10| plus the rounding floor of the sums (U relative 1e-12 as in
    tests/test_gpu_parity.py; the stress 1e-12 of the sum of its |terms|; d2 1e-12 relative), from the reference alone."""
    import moleculardynamics.jl_amd as md
    fr = frame("poly256")
    s = fr["system"]
    n, d = s["n"], s["dim"]
    U0 = _cell0(fr)
    args = (s["x"], s["diam"], U0, fr["cutoff"], fr["kind"], fr["params"], cr.AQS_STEP, cr.AQS_NSTEPS)
    ref = cr.aqs_reference(*args, cr.AQS_TOL)
    fine = cr.aqs_reference(*args, cr.AQS_TOL / 10)
    assert ref["converged"].all() and fine["converged"].all()
    sabs = er.affine(ref["x"], ref["cell"], fr["cutoff"], fr["kind"], fr["params"], s["diam"])["stress_abs"].max()
    b_e = 10 * np.abs(ref["energy"] - fine["energy"]) + 1e-12 * np.abs(ref["energy"])
    b_s = 10 * np.abs(ref["stress"] - fine["stress"]).max(axis=1) + 1e-12 * sabs
    b_d = 10 * np.abs(ref["d2"] - fine["d2"]) + 1e-12 * ref["d2"]
    state, params = state_of(fr)
    with state.system.device as dev:
        out = md.athermal_quasistatic_shear(state, params, str(tmp_path), cr.AQS_STEP, cr.AQS_NSTEPS, tol=cr.AQS_TOL,
                                            **cr.AQS_FIRE)
        assert state.system.device is dev
    stress = np.stack([out[c] for c in ("stress_xx", "stress_yy", "stress_xy")], axis=1)
    for k in range(cr.AQS_NSTEPS):
        e_e, e_s, e_d = abs(out["energy"][k] - ref["energy"][k]), np.abs(stress[k] - ref["stress"][k]).max(), abs(out["d2_nonaffine"][k] - ref["d2"][k])
        print("increment %d: |dE/N| %.3e (allowed %.3e), |dsigma| %.3e (allowed %.3e), |dd2| %.3e (allowed %.3e); FIRE steps "
              "%d (reference %d)" % (k + 1, e_e, b_e[k], e_s, b_s[k], e_d, b_d[k], out["fire_steps"][k], ref["steps"][k]))
    for k in range(cr.AQS_NSTEPS):
        assert out["converged"][k] == 1
        assert abs(out["energy"][k] - ref["energy"][k]) <= b_e[k], k
        assert np.abs(stress[k] - ref["stress"][k]).max() <= b_s[k], k
        assert abs(out["d2_nonaffine"][k] - ref["d2"][k]) <= b_d[k], k
    assert np.allclose(out["strain"], cr.AQS_STEP * np.arange(1, cr.AQS_NSTEPS + 1), rtol=1e-15, atol=0)
    assert np.allclose(out["pressure"], -(out["stress_xx"] + out["stress_yy"]) / 2, rtol=1e-14, atol=0)
    assert np.all(out["flips"] == 0) and np.all((out["participation"] > 0) & (out["participation"] <= 1))
    table = np.loadtxt(tmp_path / "aqs.txt")
    assert table.shape == (cr.AQS_NSTEPS, len(md.deformation.aqs_columns(d)))
    assert open(tmp_path / "aqs.txt").readline().split()[1:] == md.deformation.aqs_columns(d)
    assert np.array_equal(table[:, 2], out["energy"]) and np.array_equal(table[:, 1], out["strain"])
    # the one download at the end: the state holds the last minimum, in the strained cell
    assert np.allclose(state.unitcell, ref["cell"], rtol=0, atol=4 * EPS * np.abs(U0).max())
    dx = (cr.frac(state.system.positions, state.unitcell) + state.images) - (cr.frac(ref["x"], ref["cell"]) + ref["img"])
    assert np.abs(dx @ state.unitcell.T).max() <= 1e-5


# ---------------------------------------------------------------------------------------------------------------------
# 7. past half a box
# ---------------------------------------------------------------------------------------------------------------------
def test_aqs_past_half_a_box(tmp_path):
    """Simple shear of the 2-D N = 1200 frame to a strain of 0.65 in steps of 0.05, the cell reduced on the way.  FIRE gets
    1500 steps per increment: an increment that does not reach 1e-6 by then is recorded as not converged and the run goes on
    (plastic events at steps this large need more; the loop's bookkeeping is what is checked here)."""
    import moleculardynamics.jl_amd as md
    fr = frame("poly1200")
    s = fr["system"]
    U0 = _cell0(fr)
    state, params = state_of(fr)
    seen = []
    with state.system.device as dev:
        out = md.athermal_quasistatic_shear(state, params, str(tmp_path), 0.05, 13, tol=1e-6, max_steps=1500,
                                            dt_initial=0.002, dt_max=0.02, mark="start", on_step=seen.append)
        pairs = dev.neighbor_pairs()
        x = dev.download()[0]
        na = dev.nonaffine()
    assert len(seen) == 13 and seen[4]["step"] == 5
    assert out["flips"].sum() >= 1 and out["flips"][:9].sum() == 0      # the tilt passes half a box at increment 11
    table = np.loadtxt(tmp_path / "aqs.txt")
    assert np.all(np.diff(table[:, 1]) > 0) and abs(table[-1, 1] - 0.65) < 1e-12
    assert set(np.unique(out["converged"])) <= {0, 1} and np.all(out["fire_steps"] <= 1500)
    U = np.array(state.unitcell)
    assert abs(abs(np.linalg.det(U)) - abs(np.linalg.det(U0))) <= 1e-12 * abs(np.linalg.det(U0))
    assert abs(U[0, 1]) <= 0.5 * U0[0, 0] * (1 + 1e-12)                 # reduced
    assert np.array_equal(x, state.system.positions)
    _, _, _, pairs_ref = _brute(fr, x, U)
    assert np.array_equal(pairs, pairs_ref)
    assert na["sum_u2"] / s["n"] == pytest.approx(out["d2_nonaffine"][-1], rel=1e-12)   # mark="start": u accumulates
    print("strain 0.65 in 13 increments: flips %s, converged %s, d2 %s" % (out["flips"], out["converged"], out["d2_nonaffine"]))
