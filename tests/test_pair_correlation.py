"""CPU: the marked-pair-correlation sampler's host layers -- the exported symbols and their declarations, the Julia twin,
the build rule, OrientationalCorrelation's argument checks, its place in run_simulation's sampler order and the device
calls it issues (on a fake handle that records every call, as tests/test_sampler_protocol.py does), its file format --
and the numpy reference of the GPU tests (tests/mpc_reference.py) on two lattices whose answer is known."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import moleculardynamics.jl_amd as md
from moleculardynamics.jl_amd import _lib, analysis
from tests import boo_reference as boo
from tests import mpc_reference as ref
from tests.test_sampler_protocol import N, _FakeDevice, _fake_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["md_mpc_setup", "md_mpc_marks", "md_mpc_sample", "md_mpc_last", "md_mpc_read", "md_mpc_reset"]


def test_symbols_bindings_and_build_rule():
    for name in ("OrientationalCorrelation", "compute_orientational_correlation", "compute_marked_correlation"):
        assert name in md.__all__ and getattr(md, name) is getattr(analysis, name)
    header = open(os.path.join(ROOT, "include", "mdhip.h")).read()
    lib = _lib.load()
    for name in NAMES:
        assert name in _lib.EXPORTS
        assert hasattr(lib, name)
        assert re.search(r"\bint\s+" + name + r"\s*\(", header)
    vp, ip, dp, i64p = C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int64)
    assert lib.md_mpc_setup.argtypes == [vp, C.c_int, C.c_double, C.c_int, C.c_int, dp, C.c_double]
    assert lib.md_mpc_marks.argtypes == [vp, dp]
    assert lib.md_mpc_sample.argtypes == [vp]
    assert lib.md_mpc_last.argtypes == [vp, i64p, i64p, i64p]
    assert lib.md_mpc_read.argtypes == [vp, i64p, i64p, dp, dp, dp, ip]
    assert lib.md_mpc_reset.argtypes == [vp]
    assert (_lib.MD_MPC_BOO, _lib.MD_MPC_USER) == (0, 1)
    assert re.search(r"#define\s+MD_MPC_BOO\s+0\b", header) and re.search(r"#define\s+MD_MPC_USER\s+1\b", header)
    for name in ("mpc_setup", "mpc_marks", "mpc_sample", "mpc_last", "mpc_read", "mpc_reset"):
        assert callable(getattr(md.MDDevice, name))
    mk = open(os.path.join(ROOT, "moleculardynamics", "jl_amd", "csrc", "Makefile")).read()
    assert re.search(r"^libmdhip\.so:.*\bmd_mpc\.hpp\b", mk, re.M)
    sig = inspect.signature(md.run_simulation).parameters
    assert "orientational" in sig and sig["orientational"].default is None
    p = inspect.signature(md.OrientationalCorrelation).parameters
    assert [(k, v.default) for k, v in p.items()] == [("r_max", inspect.Parameter.empty), ("nbins", inspect.Parameter.empty),
                                                      ("every", 1)]
    assert list(inspect.signature(md.compute_orientational_correlation).parameters) == ["state", "params", "r_neigh", "order",
                                                                                       "r_max", "nbins"]
    cm = inspect.signature(md.compute_marked_correlation).parameters
    assert list(cm) == ["state", "params", "marks", "r_max", "nbins", "weights", "tmax"]
    assert cm["weights"].default is None and cm["tmax"].default is None
    jl = open(os.path.join(ROOT, "julia", "MDHip.jl")).read()
    for name in NAMES:
        assert "(:%s, LIB)" % name in jl


def test_a_null_handle_is_refused():
    lib = _lib.load()
    assert lib.md_mpc_setup(None, 0, 1.0, 10, 0, None, 0.0) != 0
    assert lib.md_mpc_marks(None, None) != 0
    assert lib.md_mpc_sample(None) != 0
    assert lib.md_mpc_last(None, None, None, None) != 0
    assert lib.md_mpc_read(None, None, None, None, None, None, None) != 0
    assert lib.md_mpc_reset(None) != 0
    assert b"null handle" in lib.md_last_error(None)


def test_argument_checks():
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="r_max"):
            md.OrientationalCorrelation(bad, 10)
    for bad in (0, 4097, 2.5):
        with pytest.raises(ValueError, match="nbins"):
            md.OrientationalCorrelation(3.0, bad)
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match="every"):
            md.OrientationalCorrelation(3.0, 10, every=bad)
    md.OrientationalCorrelation(3.0, 4096)
    assert analysis.default_tmax(np.array([[0.5, -3.0]]), [1.0, -2.0]) == 32.0        # 0.25 + 18 = 18.25 -> 32
    assert analysis.default_tmax(np.array([[2.0]]), [1.0]) == 4.0 and analysis.default_tmax(np.zeros((3, 2)), [1, 1]) == 1.0
    assert ref.round_up_pow2(3.0) == 4.0 and ref.round_up_pow2(4.0) == 4.0 and ref.round_up_pow2(0.3) == 0.5


class _Fake(_FakeDevice):
    """tests/test_sampler_protocol.py's recording handle with the bond-order and the pair-correlation calls."""
    NBINS_BOO = 0

    def boo_setup(self, r_neigh, order, nbins, threshold, min_conn, nseries):
        self.setups.append("boo_setup")
        self.boo_shape = (nbins, nseries)

    def boo_sample(self):
        self._log("boo_sample")

    def boo_read(self):
        nb, ns = self.boo_shape
        k = self._count("boo_sample")
        return (k, np.zeros(8), np.zeros(nb, dtype=np.int64), np.zeros(nb, dtype=np.int64), np.zeros(33, dtype=np.int64),
                np.zeros(33, dtype=np.int64), np.zeros((min(k, ns), 8)))

    def mpc_setup(self, r_max, nbins, weights=None, tmax=None):
        self.setups.append("mpc_setup")
        self.mpc_args = (r_max, nbins, weights, tmax)

    def mpc_sample(self):
        self._log("mpc_sample")

    def mpc_read(self):
        nb = self.mpc_args[1]
        k = self._count("mpc_sample")
        cnt = np.arange(nb, dtype=np.int64) * k                # bin 0 stays empty
        return k, cnt, cnt * 2.0 ** 30, 0.75 * N * k * 2.0 ** 31, 1.0, self.range_error

    range_error = 0


def _fake_run(tmp_path, total, f, **samplers):
    state, dev0 = _fake_state()
    dev = _Fake()
    state.system.device = dev
    params = md.Parameters(1.0, N, 0.002, md.LennardJones())
    out = str(tmp_path / "out")
    with np.errstate(all="ignore"):
        md.run_simulation(state, params, md.NVE(), total, f, out, write_trajectory=False, **samplers)
    return dev, out


def test_protocol_calls_and_the_segmentation(tmp_path):
    total, f = 50, 5
    bo = md.BondOrder(1.0, every=2)
    oc = md.OrientationalCorrelation(0.6, 4, every=4)
    rdf = md.RadialDistribution(0.6, 4, every=3)
    dev, out = _fake_run(tmp_path, total, f, orientational=oc, bond_order=bo, rdf=rdf)
    assert dev.setups == ["rdf_setup", "boo_setup", "mpc_setup"]          # set up after the bond-order sampler ...
    assert dev.mpc_args == (0.6, 4, None, None)                           # ... with its frame as the marks
    want = []
    for step in range(0, total, f):
        k = step // f
        if k % 3 == 0:
            want.append((step, "rdf_sample", ()))
        if k % 2 == 0:
            want.append((step, "boo_sample", ()))
        if k % 4 == 0:
            want.append((step, "mpc_sample", ()))                         # ... and acts after it at a shared step
    assert dev.trace == want
    assert list(np.cumsum(dev.segments) - 1) == list(range(0, total, f)) + [total - 1]    # no stop of its own
    assert oc.nsamples == 3 and oc.order == 6 and oc.r_neigh == 1.0 and oc.tmax == 1.0
    assert "orient_corr.txt" in os.listdir(out)


def test_refusals_of_a_run(tmp_path):
    with pytest.raises(ValueError, match="needs bond_order="):
        _fake_run(tmp_path, 10, 5, orientational=md.OrientationalCorrelation(0.6, 4))
    with pytest.raises(ValueError, match="multiple of bond_order.every"):
        _fake_run(tmp_path, 10, 5, orientational=md.OrientationalCorrelation(0.6, 4, every=3),
                  bond_order=md.BondOrder(1.0, every=2))
    _Fake.range_error = 1
    try:
        with pytest.raises(RuntimeError, match="range_error = 1"):
            _fake_run(tmp_path, 10, 5, orientational=md.OrientationalCorrelation(0.6, 4), bond_order=md.BondOrder(1.0))
    finally:
        _Fake.range_error = 0


def test_file_format(tmp_path):
    oc = md.OrientationalCorrelation(0.6, 4)
    dev, out = _fake_run(tmp_path, 11, 5, orientational=oc, bond_order=md.BondOrder(1.0, order=4))
    lines = open(os.path.join(out, "orient_corr.txt")).read().splitlines()
    assert lines[0] == "# l 4 r_neigh 1.000000 tmax 1 nsamples 3"
    assert lines[1] == "# r_mid count g(r) G(r) g_l(r)" and len(lines) == 2 + 4 + 1
    assert lines[-1] == "# <t_ii> 0.75000000"
    rows = [ln.split() for ln in lines[2:-1]]
    assert [r[0] for r in rows] == ["0.075000", "0.225000", "0.375000", "0.525000"]
    assert [int(r[1]) for r in rows] == [0, 3, 6, 9]
    assert rows[0][3] == "nan" and float(rows[0][4]) == 0.0               # an empty bin: no G, g_l = 0
    g = oc.g()
    for k in (1, 2, 3):
        assert float(rows[k][3]) == 0.5                                    # sum 2^30 per pair, quantum 2^-31
        assert abs(float(rows[k][2]) - g[k]) <= 5e-7 and abs(float(rows[k][4]) - 0.5 * g[k]) <= 5e-9
    # the same numbers from the object
    assert np.isnan(oc.G()[0]) and np.array_equal(oc.G()[1:], [0.5, 0.5, 0.5]) and oc.mean_self() == 0.75
    assert oc.quantum == 2.0 ** -31 and oc.dimension == 3


# ---------------------------------------------------------------------------------------------------------------------
# the reference of the GPU tests on two lattices

def test_reference_perfect_hexagonal_lattice():
    """psi_6 is the same at every site of a triangular lattice: Re psi_6(i) psi_6*(j) = 1 for every pair."""
    x, box = boo.hexagonal(24, 14, 1.0)
    n = len(x)
    nn, de = boo.brute_pairs(x, box, 1.3)
    r = boo.bond_order(n, nn, de, 6, 0.7, 6)
    assert np.all(r["nnb"] == 6)
    marks = ref.boo_marks(r["qlm"])
    assert marks.shape == (n, 2)
    r_max, nbins = 5.0, 97
    pairs, dd = boo.brute_pairs(x, box, r_max)
    d2 = (dd * dd).sum(axis=1)
    cnt, tot, own, ok = ref.correlate(pairs, d2, marks, ref.boo_weights(2, 6), 1.0, r_max, nbins)
    assert ok and cnt.sum() == len(pairs) and cnt.sum() > 30 * n
    occ = cnt > 0
    assert 10 < occ.sum() < nbins                                           # shells: most bins are empty
    assert np.all(np.abs(tot[occ] * 2.0 ** -31 / cnt[occ] - 1.0) <= 1e-9)
    assert not tot[~occ].any()
    assert abs(own * 2.0 ** -31 / n - 1.0) <= 1e-9


def test_reference_alternating_marks_on_a_square_lattice():
    """a(i) = (-1)^(ix + iy): -1 between nearest neighbours, +1 between next-nearest, exactly."""
    m, a = 12, 1.0
    g = np.stack(np.meshgrid(np.arange(m), np.arange(m), indexing="ij"), -1).reshape(-1, 2)
    x = (g + 0.25) * a
    marks = np.where(g.sum(axis=1) % 2 == 0, 1.0, -1.0)
    box = np.full(2, m * a)
    r_max, nbins = 1.6, 16                                                  # r = 1 in bin 10, sqrt(2) in bin 14
    pairs, dd = boo.brute_pairs(x, box, r_max)
    cnt, tot, own, ok = ref.correlate(pairs, (dd * dd).sum(axis=1), marks, [1.0], 1.0, r_max, nbins)
    n = m * m
    expect = np.zeros(nbins, dtype=np.int64)
    expect[10] = expect[14] = 2 * n
    assert ok and np.array_equal(cnt, expect)
    assert tot[10] == -2 * n * 2 ** 31 and tot[14] == 2 * n * 2 ** 31 and own == n * 2 ** 31
    assert not tot[cnt == 0].any()
    # a term beyond tmax (1 + 2^-10) is dropped and reported
    _, tot2, _, ok2 = ref.correlate(pairs, (dd * dd).sum(axis=1), 2.0 * marks, [1.0], 1.0, r_max, nbins)
    assert not ok2 and not tot2.any()
    # tmax is rounded up to a power of two: 3 -> 4
    _, tot3, _, ok3 = ref.correlate(pairs, (dd * dd).sum(axis=1), marks, [1.0], 3.0, r_max, nbins)
    assert ok3 and tot3[14] == 2 * n * 2 ** 29
