"""CPU tests of the collective-structure layer (analysis.select_wave_vectors / StructureFactor / compute_sq, the binding,
the Julia twin): the wave-vector selection, the schedules, the normalisations, the file formats and the argument checks.
The device sums themselves are tested in tests/test_gpu_sq.py."""
import inspect
import math
import os
import re
import time

import numpy as np
import pytest

import moleculardynamics.jl_amd as md
from moleculardynamics.jl_amd import SelfDynamics, StructureFactor, _lib, select_wave_vectors
from moleculardynamics.jl_amd import analysis

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("md_sq_setup", "md_sq_sample", "md_sq_rho", "md_sq_read", "md_sq_reset")
SHEARED = np.array([[10.0, 2.0, 1.0], [0.0, 9.0, 1.5], [0.0, 0.0, 11.0]])


def test_exports():
    for name in ("StructureFactor", "compute_sq", "select_wave_vectors"):
        assert name in md.__all__ and getattr(md, name) is getattr(analysis, name)
    for name in NAMES:
        assert name in _lib.EXPORTS
        assert hasattr(_lib.load(), name)
    header = open(os.path.join(ROOT, "include", "mdhip.h")).read()
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header)
    assert "exp(+i q.x)" in header                  # the sign convention is stated
    for name in ("sq_setup", "sq_sample", "sq_rho", "sq_read", "sq_reset"):
        assert callable(getattr(md.MDDevice, name))
    mk = open(os.path.join(ROOT, "moleculardynamics", "jl_amd", "csrc", "Makefile")).read()
    assert re.search(r"^libmdhip\.so:.*\bmd_sq\.hpp\b", mk, re.M)


def _first_nonzero(n):
    out = np.zeros(n.shape[0], dtype=np.int64)
    for c in range(n.shape[1] - 1, -1, -1):
        out = np.where(n[:, c] != 0, n[:, c], out)
    return out


def _brute(U, q_max, m):
    d = U.shape[0]
    g = np.array(np.meshgrid(*[np.arange(-m, m + 1)] * d, indexing="ij")).reshape(d, -1).T
    q = 2.0 * math.pi * np.linalg.norm(g @ np.linalg.inv(U), axis=1)
    return g[(q <= q_max) & (_first_nonzero(g) > 0)]


@pytest.mark.parametrize("cell", ["sheared", "orthorhombic", "2d", "2d-sheared"])
def test_selection_is_the_half_space_inside_q_max(cell):
    U = {"sheared": SHEARED, "orthorhombic": np.diag([9.0, 11.0, 13.0]), "2d": np.diag([20.0, 30.0]),
         "2d-sheared": np.array([[20.0, 6.0], [0.0, 17.0]])}[cell]
    q_max = 4.0 if U.shape[0] == 3 else 3.0
    # no thinning: exactly the brute-force set
    n, q, b = select_wave_vectors(U, q_max, max_per_bin=10 ** 9)
    assert n.dtype == np.int32 and n.shape[1] == U.shape[0]
    expect = _brute(U, q_max, 16)
    assert np.abs(expect).max() < 16                # the brute-force cube was large enough
    assert set(map(tuple, n)) == set(map(tuple, expect)) and len(n) == len(expect)
    assert np.all(_first_nonzero(n) > 0)            # half space: never n = 0, never both of +-n
    both = set(map(tuple, n)) & set(map(tuple, -n))
    assert not both
    # |q| = 2 pi |U^-T n|
    ref = 2.0 * math.pi * np.linalg.norm(np.linalg.inv(U).T @ n.T.astype(np.float64), axis=0)
    assert np.allclose(q, ref, rtol=1e-13, atol=0.0) and q.max() <= q_max
    assert np.allclose(analysis.wave_vector_lengths(U, n), ref, rtol=1e-13, atol=0.0)
    # bins: width 2 pi / smallest face distance by default
    face = 1.0 / np.linalg.norm(np.linalg.inv(U), axis=1)
    dq = 2.0 * math.pi / face.min()
    assert np.array_equal(b, np.floor(q / dq).astype(np.int64))
    assert np.all(np.diff(b) >= 0)


def test_selection_thins_by_a_seeded_permutation():
    full = select_wave_vectors(SHEARED, 5.0, max_per_bin=10 ** 9)
    a = select_wave_vectors(SHEARED, 5.0, max_per_bin=6, seed=3)
    a2 = select_wave_vectors(SHEARED, 5.0, max_per_bin=6, seed=3)
    c = select_wave_vectors(SHEARED, 5.0, max_per_bin=6, seed=4)
    for u, w in zip(a, a2):
        assert np.array_equal(u, w)                 # deterministic for given arguments
    assert not np.array_equal(a[0], c[0])           # the seed matters
    have = np.bincount(full[2])
    got = np.bincount(a[2], minlength=have.size)
    assert np.array_equal(got, np.minimum(have, 6))  # every bin keeps min(size, max_per_bin)
    assert set(map(tuple, a[0])) <= set(map(tuple, full[0]))
    assert a[1].max() <= 5.0
    # an explicit dq changes the binning only
    w = select_wave_vectors(SHEARED, 5.0, dq=0.5, max_per_bin=10 ** 9)
    assert set(map(tuple, w[0])) == set(map(tuple, full[0]))
    assert np.array_equal(w[2], np.floor(w[1] / 0.5).astype(np.int64))
    # a diagonal given as a vector is a diagonal cell
    d1 = select_wave_vectors([9.0, 11.0, 13.0], 3.0)
    d2 = select_wave_vectors(np.diag([9.0, 11.0, 13.0]), 3.0)
    assert np.array_equal(d1[0], d2[0])


def test_selection_of_the_large_box_is_quick():
    L = (2 ** 20 / 0.897) ** (1.0 / 3.0)
    t0 = time.time()
    n, q, b = select_wave_vectors(np.eye(3) * L, 8.0)
    took = time.time() - t0
    assert 1024 <= n.shape[0] <= 16384 and np.bincount(b).max() == 16
    assert took < 5.0, took                         # (about a quarter of a second; 5 * 10^6 candidates)


def test_argument_checks():
    with pytest.raises(ValueError, match="q_max"):
        select_wave_vectors(SHEARED, 0.0)
    with pytest.raises(ValueError, match="q_max"):
        select_wave_vectors(SHEARED, float("inf"))
    with pytest.raises(ValueError, match="dq"):
        select_wave_vectors(SHEARED, 3.0, dq=0.0)
    with pytest.raises(ValueError, match="max_per_bin"):
        select_wave_vectors(SHEARED, 3.0, max_per_bin=0)
    with pytest.raises(ValueError, match="unitcell"):
        select_wave_vectors(np.eye(4), 3.0)
    with pytest.raises(ValueError, match="no wave vector"):
        select_wave_vectors(SHEARED, 0.1)
    with pytest.raises(ValueError, match="at most 16384"):
        select_wave_vectors(np.eye(3) * 40.0, 8.0, max_per_bin=10 ** 9)
    with pytest.raises(ValueError, match="q_max"):
        StructureFactor(-1.0)
    with pytest.raises(ValueError, match="every"):
        StructureFactor(3.0, every=0)
    with pytest.raises(ValueError, match="max_per_bin"):
        StructureFactor(3.0, max_per_bin=0)
    with pytest.raises(ValueError, match="dq"):
        StructureFactor(3.0, dq=-1.0)
    with pytest.raises(ValueError, match="dynamic=True"):
        StructureFactor(3.0, lags=(1, 2), origin_every=1)
    # the dynamic schedule takes SelfDynamics' arguments and refuses what it refuses
    for kw in (dict(origin_every=3), dict(lags=(1, 2)), dict(lags=(0, 1), origin_every=1), dict(lags=(1, 1), origin_every=1),
               dict(lags=(1, 650), origin_every=10), dict(lags=(1.5,), origin_every=1)):
        with pytest.raises(ValueError) as e1:
            SelfDynamics(**kw)
        with pytest.raises(ValueError) as e2:
            StructureFactor(3.0, dynamic=True, **kw)
        assert str(e1.value) == str(e2.value)
    dev_sig = inspect.signature(md.MDDevice.sq_sample)
    assert list(dev_sig.parameters)[1:] == ["static", "slots", "rows", "origin"]


@pytest.mark.parametrize("kw", [dict(), dict(lags=(1, 2, 5), origin_every=3), dict(lags=(7, 100, 3), origin_every=10)])
@pytest.mark.parametrize("T", [1, 30, 200, 163437 + 50])
def test_the_schedule_is_selfdynamics_schedule(kw, T):
    if kw and T > 1000:
        T = 1000
    dyn = SelfDynamics(**kw)
    sq = StructureFactor(3.0, dynamic=True, **kw)
    assert sq.nslots == dyn.nslots and list(sq.lags) == list(dyn.lags)
    assert sq.schedule(T) == dyn.schedule(T)
    st = StructureFactor(3.0)
    assert st.schedule(T) == ([], {}) and st.nslots == 0 and len(st.lags) == 0


def _synthetic(dynamic=True):
    sq = StructureFactor(4.0, max_per_bin=5, seed=1, dynamic=dynamic, **(dict(lags=(1, 2, 4), origin_every=2) if dynamic else {}))
    sq._select(SHEARED)
    nvec = sq.n.shape[0]
    rng = np.random.default_rng(7)
    s2 = rng.uniform(10.0, 500.0, nvec)
    corr = rng.normal(size=(3, nvec)) * 100.0
    ns = np.array([3, 0, 2])
    sq._accumulate(4, s2, ns, corr, 100, 0.01)
    return sq, s2, corr, ns


def test_normalisations():
    sq, s2, corr, ns = _synthetic()
    nvec = sq.n.shape[0]
    assert sq.nstatic == 4 and sq.n_particles == 100
    assert sq.bin.shape == (nvec,) and sq.bin.max() == sq.q.size - 1 and sq.nvectors.sum() == nvec
    assert sq.nvectors.max() <= 5
    s, f, fn = sq.s(), sq.f(), sq.f_normalised()
    assert s.shape == (sq.q.size,) and f.shape == (3, sq.q.size) and fn.shape == f.shape
    for b in range(sq.q.size):
        members = np.nonzero(sq.bin == b)[0]
        assert sq.nvectors[b] == members.size
        assert sq.q[b] == pytest.approx(np.mean(sq.qvec[members]), rel=1e-14)
        assert s[b] == pytest.approx(sum(s2[v] for v in members) / (4 * 100 * members.size), rel=1e-13)
        for k in (0, 2):
            assert f[k, b] == pytest.approx(sum(corr[k, v] for v in members) / (ns[k] * 100 * members.size), rel=1e-12,
                                            abs=1e-14)
            assert fn[k, b] == pytest.approx(f[k, b] / s[b], rel=1e-13)
    assert np.all(np.isnan(f[1])) and np.all(np.isnan(fn[1]))      # a lag without a sample
    assert np.allclose(sq.s_vectors(), s2 / 400.0, rtol=1e-15)
    assert np.allclose(sq.f_vectors()[2], corr[2] / 200.0, rtol=1e-15)
    # a second collection accumulates
    sq._accumulate(1, s2, ns, corr, 100, 0.01)
    assert sq.nstatic == 5 and list(sq.nsamples) == [6, 0, 4]
    assert np.allclose(sq.s(), s * 2.0 * 4.0 / 5.0, rtol=1e-13)
    # another cell is refused until reset(); reset forgets vectors and samples
    with pytest.raises(ValueError, match="unit cell"):
        sq._select(SHEARED * 1.01)
    sq._select(SHEARED)
    sq.reset()
    assert sq.nstatic == 0 and not sq.nsamples.any() and sq.n is None
    sq._select(SHEARED * 1.01)
    assert sq.s2.shape == (sq.n.shape[0],) and not sq.s2.any()
    empty = StructureFactor(4.0)
    empty._select(SHEARED)
    assert np.all(np.isnan(empty.s()))              # no sample yet


def test_file_formats(tmp_path):
    sq, s2, corr, ns = _synthetic()
    p = str(tmp_path / "sq.txt")
    sq.write(p)
    lines = open(p).read().splitlines()
    assert lines[0] == "# q S(q) nvectors nsamples" and len(lines) == 1 + sq.q.size
    s, f, fn = sq.s(), sq.f(), sq.f_normalised()
    for b, line in enumerate(lines[1:]):
        assert line == "%.6f %.6e %d %d" % (sq.q[b], s[b], sq.nvectors[b], 4)
    p = str(tmp_path / "fqt.txt")
    sq.write_fqt(p)
    text = open(p).read()
    head = "# lag time q F F/S nsamples\n"
    assert text.startswith(head)
    blocks = text[len(head):].split("\n\n")
    assert len(blocks) == 2                         # lag 2 was never reached: left out
    for blk, k, lag in zip(blocks, (0, 2), (1, 4)):
        rows = blk.strip("\n").split("\n")
        assert len(rows) == sq.q.size
        for b, row in enumerate(rows):
            assert row == "%d %.6e %.6f %.6e %.6e %d" % (lag, lag * 0.01, sq.q[b], f[k, b], fn[k, b], ns[k])
    sq.write_fqt(p, dt=0.5)                         # an explicit dt overrides the one run_simulation recorded
    assert open(p).read().splitlines()[1].split()[1] == "%.6e" % 0.5


def test_run_simulation_has_the_keyword():
    sig = inspect.signature(md.run_simulation)
    assert "sq" in sig.parameters and sig.parameters["sq"].default is None
    assert list(inspect.signature(md.compute_sq).parameters)[:3] == ["state", "params", "q_max"]


def test_julia_twin_binds_the_entries():
    src = open(os.path.join(ROOT, "julia", "MDHip.jl")).read()
    for name in NAMES:
        assert re.search(r"\(:" + name + r",\s*LIB\)", src), name
    assert "mutable struct StructureFactor" in src
    assert re.search(r"sq::Union\{Nothing,\s*StructureFactor\}\s*=\s*nothing", src)
    assert re.search(r"^function sofq\(", src, re.M) or re.search(r"^sofq\(", src, re.M)
    assert "select_wave_vectors" in src and "sq.txt" in src and "fqt.txt" in src
