"""Cell changes of a live handle (md_set_cell), the non-affine displacement since a mark (md_nonaffine_*) and the AQS loop,
without a device: known answers proved on the numpy restatement tests/cell_reference.py, the deliberate mistakes it must
catch, the bindings, and the CPU reference loop tests/test_gpu_deformation.py compares the device with.

Rounding bounds (derived where they are used): cell_reference.unwrapped_bound for x + U img through remaps, u_bound below
for the non-affine displacement."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import moleculardynamics.jl_amd as md
from moleculardynamics.jl_amd import _lib, deformation
from tests import cell_reference as cr
from tests.util import poly_system

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = cr.EPS


def u_bound(U, frac_max, m_max=1.0):
    """Bound per component on the rounding of u = U ((frac - frac0) + dimg), and on its change under a lattice flip.

    frac = U^-1 x is d products and d - 1 sums of terms |U^-1| |x| <= about |frac| each, with a cofactor inverse good to a few
    ulp: off by <= 8 eps (1 + |frac|).  A flip replaces frac0 by M^-1 frac0 (d products, d - 1 sums, terms up to |M^-1|
    |frac0|) against a frac taken in the new cell: <= 8 eps |M^-1| (1 + |frac|) more.  The difference of the two fracs and the
    exact integer add one rounding each, U d is d terms of |U| |d| with the error of d carried through |U| per term.  In all
    32 eps d max|U| max|M^-1| (1 + max|frac|)."""
    d = np.asarray(U).shape[0]
    return 32.0 * EPS * d * float(np.abs(U).max()) * float(m_max) * (1.0 + float(frac_max))


def _frame(d, n=300, seed=3, spread=3.0, big_images=True):
    rng = np.random.default_rng(seed)
    L = np.array([7.0, 8.5, 9.25])[:d]
    x = rng.uniform(-spread, spread + 1.0, (n, d)) * L            # the wrap is lazy: stored positions may be anywhere
    img = rng.integers(-3, 4, (n, d))
    if big_images:
        img[::7] = rng.choice([-10 ** 6, 10 ** 6], (len(img[::7]), d))
    return x, img.astype(np.int64), np.diag(L)


def _cells(d):
    """(diagonal, another diagonal, general, another general) cells of dimension d"""
    D0 = np.diag([7.0, 8.5, 9.25][:d])
    D1 = np.diag([7.5, 8.0, 9.0][:d])
    G0 = D0.copy()
    G0[0, 1] = 2.1
    G1 = D1.copy()
    G1[0, 1] = -1.3
    if d == 3:
        G0[0, 2], G0[1, 2] = 0.7, -1.1
        G1[1, 2] = 1.9
    return D0, D1, G0, G1


# ---------------------------------------------------------------------------------------------------------------------
# known answers on the restatement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("trans", ["diag_diag", "diag_general", "general_general", "general_diag"])
def test_affine_keeps_fractional_coordinate_plus_image(d, trans):
    """frac' + img' = frac + img with frac' = frac - floor(frac), img' = img + floor(frac): the integer part moves exactly;
    frac - floor(frac) is exact for frac >= 0 (the difference is a multiple of ulp(frac) below 1) and rounded once, by at
    most 2^-53, for frac < 0 (a number in [0, 1) that need not be a double).  Checked in exact rational arithmetic."""
    D0, D1, G0, G1 = _cells(d)
    U_old, U_new = dict(diag_diag=(D0, D1), diag_general=(D0, G0), general_general=(G0, G1), general_diag=(G0, D1))[trans]
    x, img, _ = _frame(d)
    fr = cr.frac(x, U_old)
    x2, img2 = cr.affine(x, img, U_old, U_new)
    nn = np.floor(fr)
    assert np.array_equal(img2 - img, nn.astype(np.int64))
    fm = fr - nn
    assert np.all((fm >= 0.0) & (fm <= 1.0))
    assert np.array_equal(x2, cr.cart(fm, U_new))
    worst = Fraction(0)
    for (i, c), f in np.ndenumerate(fr):
        err = abs((Fraction(float(fm[i, c])) + int(img2[i, c])) - (Fraction(float(f)) + int(img[i, c])))
        if f >= 0.0:
            assert err == 0
        worst = max(worst, err)
    assert worst <= Fraction(1, 2 ** 53)
    # the mistake "frac taken with the new inverse" does not keep it
    x3, img3 = cr.affine(x, img, U_old, U_new, variant="new_inverse")
    assert not np.array_equal(img3, img2) or not np.array_equal(x3, x2)
    kept = (cr.frac(x3, U_new) + img3) - (fr + img)
    assert np.abs(kept).max() > 1e-3


def _flip_cells(d):
    """A cell sheared past half a box length, and the reduced cell of the same lattice"""
    U_old = np.diag([7.0, 8.5, 9.25][:d])
    U_old[0, 1] = 0.7 * 7.0
    if d == 3:
        U_old[1, 2] = -0.6 * 8.5
    W, M = deformation.gauss_reduce(U_old)
    assert not np.array_equal(M, np.eye(d, dtype=np.int64))
    return U_old, W, M


@pytest.mark.parametrize("d", [2, 3])
def test_lattice_flip_keeps_unwrapped_positions(d):
    """x + U img before and after a flip, within cell_reference.unwrapped_bound (derived there): with images of +-10^6 the
    bound is dominated by the rounding of the new cell's entries times the image count."""
    U_old, U_new, M = _flip_cells(d)
    assert np.array_equal(cr.lattice_matrix(U_old, U_new), M)
    x, img, _ = _frame(d)
    x2, img2, _ = cr.lattice(x, img, U_old, U_new)
    bound = cr.unwrapped_bound([U_old, U_new], [img, img2])
    err = np.abs(cr.unwrapped(x2, img2, U_new) - cr.unwrapped(x, img, U_old)).max()
    print("d = %d: |x + U img| changed by %.3e (allowed %.3e)" % (d, err, bound))
    assert err <= bound
    fr = cr.frac(x2, U_new)
    assert np.all((fr > -1e-12) & (fr < 1.0 + 1e-12))
    # the two mistakes of the image map move particles by whole lattice vectors
    for variant in ("wrong_sign", "m_not_inverse"):
        x3, img3, _ = cr.lattice(x, img, U_old, U_new, variant=variant)
        bad = np.abs(cr.unwrapped(x3, img3, U_new) - cr.unwrapped(x, img, U_old)).max()
        assert bad > 1.0 and bad > 1e3 * bound, variant


@pytest.mark.parametrize("d", [2, 3])
def test_shear_there_and_back_returns_the_frame(d):
    U0 = np.diag([7.0, 8.5, 9.25][:d])
    x, img, _ = _frame(d)
    F, Fb = deformation.simple_shear(d, 0.0123), deformation.simple_shear(d, -0.0123)
    U1 = F @ U0
    U2 = Fb @ U1                                               # (U0 again but for the rounding of gamma L - gamma L)
    assert np.abs(U2 - U0).max() <= 2 * EPS * np.abs(U0).max()
    x1, img1 = cr.affine(x, img, U0, U1)
    x2, img2 = cr.affine(x1, img1, U1, U2)
    bound = cr.unwrapped_bound([U0, U1, U2], [img, img1, img2])
    err = np.abs(cr.unwrapped(x2, img2, U2) - cr.unwrapped(x, img, U0)).max()
    print("d = %d: there and back %.3e (allowed %.3e)" % (d, err, bound))
    assert err <= bound
    moved = np.abs(cr.unwrapped(x1, img1, U1) - cr.unwrapped(x, img, U0)).max()
    assert moved > 0.01 and moved > 1e3 * bound                # (the strain itself is no rounding)


def test_gauss_reduce_is_unimodular_and_never_narrows_a_face_distance():
    rng = np.random.default_rng(8)
    cells = []
    for d in (2, 3):
        L = np.array([7.0, 8.5, 9.25])[:d]
        for gamma in (0.2, 0.51, 0.7, 1.6, -2.4):
            cells.append(deformation.simple_shear(d, gamma) @ np.diag(L))
        U = np.diag(L)
        U[0, d - 1] = 5.0
        U[0, 1] += 4.9
        cells.append(U)
        for _ in range(20):
            cells.append(np.diag(L) + rng.uniform(-4.0, 4.0, (d, d)) * (1.0 - np.eye(d)))
    nflip = 0
    for U in cells:
        W, M = deformation.gauss_reduce(U)
        d = U.shape[0]
        assert M.dtype == np.int64 and round(float(np.linalg.det(M.astype(float)))) in (1, -1)
        assert np.allclose(W, U @ M, rtol=0, atol=8 * EPS * np.abs(U).max() * max(1, np.abs(M).max()))
        assert np.all(cr.face_distances(W) >= cr.face_distances(U) * (1.0 - 1e-12)), (U, M)
        W2, M2 = deformation.gauss_reduce(W)
        assert np.array_equal(M2, np.eye(d, dtype=np.int64))                       # reduced is a fixed point
        if not np.array_equal(M, np.eye(d, dtype=np.int64)):
            nflip += 1
            assert np.array_equal(cr.lattice_matrix(U, W), M)                       # and the host's rules accept it
            assert np.array_equal(cr.integer_inverse(M) @ M, np.eye(d, dtype=np.int64))
    assert nflip >= 10
    # a simply sheared box: the usual flip by one lattice vector once the tilt passes half a box length
    U = deformation.simple_shear(2, 0.49) @ np.diag([7.0, 7.0])
    assert np.array_equal(deformation.gauss_reduce(U)[1], np.eye(2, dtype=np.int64))
    W, M = deformation.gauss_reduce(deformation.simple_shear(2, 0.51) @ np.diag([7.0, 7.0]))
    assert np.array_equal(M, np.array([[1, -1], [0, 1]])) and abs(W[0, 1] - (0.51 - 1.0) * 7.0) < 1e-14


def test_lattice_matrix_refuses_what_the_host_refuses():
    U = np.diag([7.0, 8.5])
    for bad in (np.diag([14.0, 8.5]), np.array([[7.0, 3.0], [0.0, 8.5]]), np.diag([7.0, 8.5 * (1 + 1e-6)])):
        with pytest.raises(ValueError):
            cr.lattice_matrix(U, bad)
    with pytest.raises(ValueError):                                    # an entry of M above 2^10
        cr.lattice_matrix(U, np.array([[7.0, 7.0 * 1025], [0.0, 8.5]]))
    assert cr.lattice_matrix(U, np.array([[7.0, 7.0 * 1024], [0.0, 8.5]]))[0, 1] == 1024
    with pytest.raises(OverflowError):
        cr.lattice(np.zeros((1, 2)) + 1.0, np.array([[2 ** 31 - 2, 5]]), U, np.array([[7.0, -7.0], [0.0, 8.5]]))


# ---------------------------------------------------------------------------------------------------------------------
# the non-affine displacement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [2, 3])
def test_nonaffine_displacement_on_the_restatement(d):
    """Zero to rounding after a pure affine strain; a known displacement comes back; a flip leaves u unchanged to rounding
    only when the mark goes through the same integer matrix."""
    rng = np.random.default_rng(21)
    U0 = np.diag([7.0, 8.5, 9.25][:d])
    x, img, _ = _frame(d, big_images=True)
    mark = cr.mark_of(x, img, U0)
    fmax = np.abs(mark[0]).max()
    U1 = deformation.simple_shear(d, 0.7) @ U0
    if d == 3:
        U1 = deformation.simple_shear(d, -0.6, plane=(1, 2)) @ U1
    x1, img1 = cr.affine(x, img, U0, U1)
    u, sums = cr.nonaffine(x1, img1, U1, mark)
    b1 = u_bound(U1, fmax)
    print("d = %d: max |u| after an affine strain %.3e (allowed %.3e)" % (d, np.abs(u).max(), b1))
    assert np.abs(u).max() <= b1 and sums[7] == len(x)
    disp = rng.normal(0.0, 0.3, x.shape)
    disp[17] = 2.5                                                    # the maximum, across a face for most particles
    x2 = x1 + disp
    u2, sums2 = cr.nonaffine(x2, img1, U1, mark)
    assert np.abs(u2 - disp).max() <= b1 + 4 * EPS * np.abs(x2).max()
    assert int(sums2[6]) == 17 and abs(sums2[5] - d * 2.5 ** 2) <= 1e-12
    assert abs(sums2[3] - (disp ** 2).sum()) <= 1e-9 and np.abs(sums2[:d] - disp.sum(axis=0)).max() <= 1e-9
    # the flip
    W, M = deformation.gauss_reduce(U1)
    assert not np.array_equal(M, np.eye(d, dtype=np.int64))
    x3, img3, mark3 = cr.lattice(x2, img1, U1, W, mark=mark)
    u3, sums3 = cr.nonaffine(x3, img3, W, mark3)
    b3 = b1 + u_bound(W, max(fmax, np.abs(mark3[0]).max()), np.abs(cr.integer_inverse(M)).max())
    print("d = %d: |u| changed by the flip %.3e (allowed %.3e)" % (d, np.abs(u3 - u2).max(), b3))
    assert np.abs(u3 - u2).max() <= b3 and int(sums3[6]) == 17
    _, _, mark_bad = cr.lattice(x2, img1, U1, W, mark=mark, variant="mark_untouched")
    u4, _ = cr.nonaffine(x3, img3, W, mark_bad)
    assert np.abs(u4 - u2).max() > 1.0 and 1e3 * b3 < 1.0


# ---------------------------------------------------------------------------------------------------------------------
# the Python layer
# ---------------------------------------------------------------------------------------------------------------------
def test_gradient_helpers():
    for d in (2, 3):
        F = md.simple_shear(d, 0.3)
        assert F[0, 1] == 0.3 and np.array_equal(F - np.eye(d), np.where(np.arange(d * d).reshape(d, d) == 1, 0.3, 0.0))
        assert abs(np.linalg.det(md.pure_shear(d, 0.2)) - 1.0) < 1e-15
        assert md.pure_shear(d, 0.2)[0, 0] == 1.2 and md.pure_shear(d, 0.2)[1, 1] == 1.0 / 1.2
        assert np.array_equal(md.volumetric(d, 0.1), np.eye(d) * 1.1)
    F = md.simple_shear(3, -0.5, plane=(1, 2))
    assert F[1, 2] == -0.5 and F[0, 1] == 0.0
    for bad in ((0, 0), (0, 2)):
        with pytest.raises(ValueError):
            md.simple_shear(2, 0.1, plane=bad)
    with pytest.raises(ValueError):
        md.pure_shear(2, -1.0)
    with pytest.raises(ValueError):
        md.volumetric(3, -2.0)
    assert deformation.aqs_columns(2) == ["step", "strain", "energy", "stress_xx", "stress_yy", "stress_xy", "pressure",
                                          "fire_steps", "converged", "d2_nonaffine", "participation", "max_u", "flips"]
    assert deformation.aqs_columns(3)[3:9] == ["stress_xx", "stress_yy", "stress_zz", "stress_xy", "stress_xz", "stress_yz"]


def test_symbols_bindings_header_makefile_and_julia():
    for name in ("md_set_cell", "md_nonaffine_mark", "md_nonaffine"):
        assert name in _lib.EXPORTS
    for name in ("simple_shear", "pure_shear", "volumetric", "set_unitcell", "deform", "reduce_cell",
                 "athermal_quasistatic_shear"):
        assert name in md.__all__ and getattr(md, name) is getattr(deformation, name)
    for name in ("set_cell", "nonaffine_mark", "nonaffine"):
        assert callable(getattr(md.MDDevice, name))
    header = open(os.path.join(ROOT, "include", "mdhip.h")).read()
    defs = dict(re.findall(r"^#define (MD_CELL_[A-Z_]+) (\d+)", header, flags=re.M))
    assert {k: int(v) for k, v in defs.items()} == {"MD_CELL_AFFINE": _lib.MD_CELL_AFFINE, "MD_CELL_LATTICE": _lib.MD_CELL_LATTICE} \
        == {"MD_CELL_AFFINE": 0, "MD_CELL_LATTICE": 1}
    assert (md.MDDevice.CELL_AFFINE, md.MDDevice.CELL_LATTICE) == (0, 1)
    assert re.search(r"int md_set_cell\(md_ctx \*ctx, const double \*box, int mode\);", header)
    assert re.search(r"int md_nonaffine_mark\(md_ctx \*ctx\);", header)
    assert re.search(r"int md_nonaffine\(md_ctx \*ctx, double \*sums, double \*u\);", header)
    assert "STALE" in header and "N * D * 12 bytes" in header
    make = open(os.path.join(ROOT, "moleculardynamics", "jl_amd", "csrc", "Makefile")).read()
    rule = [l for l in make.splitlines() if l.startswith("libmdhip.so:")][0]
    assert "md_cell.hpp" in rule.split()
    lib = _lib.load()
    dp = C.POINTER(C.c_double)
    assert lib.md_set_cell.argtypes == [C.c_void_p, dp, C.c_int] and lib.md_set_cell.restype is C.c_int
    assert lib.md_nonaffine_mark.argtypes == [C.c_void_p] and lib.md_nonaffine_mark.restype is C.c_int
    assert lib.md_nonaffine.argtypes == [C.c_void_p, dp, dp] and lib.md_nonaffine.restype is C.c_int
    julia = open(os.path.join(ROOT, "julia", "MDHip.jl")).read()
    for name in ("set_unitcell!", "deform!", "reduce_cell!", "athermal_quasistatic_shear!"):
        assert re.search(r"^function %s\(|^%s\(" % (re.escape(name), re.escape(name)), julia, flags=re.M), name
        assert name in julia.split("const LIB")[0]                                    # exported
    for sym in ("md_set_cell", "md_nonaffine_mark", "md_nonaffine"):
        assert "(:%s, LIB)" % sym in julia
    for kw in ("mode::Symbol=:simple", "plane=(1, 2)", "tol::Float64=1e-9", "reduce::Bool=true", "mark::Symbol=:previous",
               "on_step=nothing"):
        assert kw in julia
    assert "aqs.txt" in julia
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert re.search(r"^## 25\.", design, flags=re.M) and "md_set_cell" in design


def test_a_null_handle_is_refused():
    lib = _lib.load()
    assert lib.md_set_cell(None, None, 0) != 0
    assert b"null handle" in lib.md_last_error(None)
    assert lib.md_nonaffine_mark(None) != 0
    assert lib.md_nonaffine(None, None, None) != 0
    assert b"null handle" in lib.md_last_error(None)


# ---------------------------------------------------------------------------------------------------------------------
# the CPU reference AQS loop
# ---------------------------------------------------------------------------------------------------------------------
def test_reference_aqs_loop_has_no_plastic_event_at_its_strain_step():
    """The poly256 system (tests/test_gpu_hessian.py: poly_system(n=256), Polydisperse(1.25, 0.2), cutoff 1.5), relaxed here
    by the oracle's FIRE as that file relaxes it by the device's.  AQS_NSTEPS increments of AQS_STEP against twice as many
    of half the step: at equal strain both runs must sit in the same minimum.  Two minima of a glass differ by a
    rearrangement, |dx| of 1e-2 .. 1 of a diameter for some particle; two FIRE stops in one minimum by at most
    2 tol sqrt(N d) / lambda_min, below 1e-6 for lambda_min >= 0.05 at tol = 1e-9.  The line is drawn at 1e-5; the energies
    per particle must then agree to 1e-10 (a displacement dx of the minimum changes them by lambda dx^2 / N at most).
    (The oracle's brute-force loop is serial: this test takes some twenty seconds, nearly all of it there.)"""
    from oracle import oracle
    s = poly_system(n=256)
    pot = md.Polydisperse(1.25, 0.2)
    kind, params = pot.device_spec()[1], list(pot.device_spec()[2])
    r = oracle.fire_minimize(s["x"], s["img"], s["diam"], s["box"], 1.5, oracle.make_pot(kind, params), tol=cr.AQS_TOL,
                             use_cells=True, **cr.AQS_FIRE)
    assert r["converged"]
    U0 = np.diag(s["box"])
    a = cr.aqs_reference(r["x"], s["diam"], U0, 1.5, kind, params, cr.AQS_STEP, cr.AQS_NSTEPS, cr.AQS_TOL)
    b = cr.aqs_reference(r["x"], s["diam"], U0, 1.5, kind, params, cr.AQS_STEP / 2, 2 * cr.AQS_NSTEPS, cr.AQS_TOL)
    assert a["converged"].all() and b["converged"].all()
    assert np.allclose(a["cell"], b["cell"], rtol=0, atol=4 * EPS * np.abs(U0).max())
    de = np.abs(a["energy"] - b["energy"][1::2]).max()
    ds = np.abs(a["stress"] - b["stress"][1::2]).max()
    fa = cr.frac(a["x"], a["cell"]) + a["img"]
    fb = cr.frac(b["x"], a["cell"]) + b["img"]
    dx = np.abs((fa - fb) @ a["cell"].T).max()
    print("step %g x %d against %g x %d: |dE/N| %.3e, |dsigma| %.3e, max |dx| %.3e; d2 %s; FIRE steps %s"
          % (cr.AQS_STEP, cr.AQS_NSTEPS, cr.AQS_STEP / 2, 2 * cr.AQS_NSTEPS, de, ds, dx, a["d2"], a["steps"]))
    assert dx <= 1e-5 and de <= 1e-10
    assert np.all(np.diff(a["energy"]) > 0.0)                       # an elastic branch: the energy rises with the strain
    assert np.all(a["d2"] < 1e-4)                                   # and nobody jumped: |u| stays far below a diameter
