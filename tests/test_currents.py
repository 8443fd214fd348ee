"""CPU: the current-correlation sampler's host layers -- the exported symbols and their declarations, CurrentCorrelations'
argument checks, its place in run_simulation's signature and sampler order and the device calls it issues (on a fake
handle that records every call, as tests/test_sampler_protocol.py does), its normalisation and file formats -- and the
numpy reference of the GPU tests (tests/cur_reference.py) against a case of four particles worked out by hand."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import moleculardynamics.jl_amd as md
from moleculardynamics.jl_amd import _lib, analysis
from tests import cur_reference as ref
from tests.test_sampler_protocol import N, _FakeDevice, _fake_state, _split

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["md_cur_setup", "md_cur_sample", "md_cur_last", "md_cur_read", "md_cur_reset"]


def test_symbols_bindings_and_build_rule():
    assert "CurrentCorrelations" in md.__all__ and md.CurrentCorrelations is analysis.CurrentCorrelations
    header = open(os.path.join(ROOT, "include", "mdhip.h")).read()
    lib = _lib.load()
    for name in NAMES:
        assert name in _lib.EXPORTS
        assert hasattr(lib, name)
        assert re.search(r"\bint\s+" + name + r"\s*\(", header)
    vp, ip, dp, i64p = C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int64)
    assert lib.md_cur_setup.argtypes == [vp, ip, dp, C.c_int, C.c_int, C.c_int, C.c_int]
    assert lib.md_cur_sample.argtypes == [vp, C.c_int, ip, ip, C.c_int, C.c_int]
    assert lib.md_cur_last.argtypes == [vp, dp]
    assert lib.md_cur_read.argtypes == [vp, i64p, dp, dp, i64p, dp, dp, dp]
    assert lib.md_cur_reset.argtypes == [vp]
    assert "MDHIP_CUR_ALLOC_LIMIT" in header and "V_a * (32*kappa*|n|_1 + 128) * 2^-53" in header
    for name in ("cur_setup", "cur_sample", "cur_last", "cur_read", "cur_reset"):
        assert callable(getattr(md.MDDevice, name))
    mk = open(os.path.join(ROOT, "moleculardynamics", "jl_amd", "csrc", "Makefile")).read()
    assert re.search(r"^libmdhip\.so:.*\bmd_cur\.hpp\b", mk, re.M)
    sig = inspect.signature(md.run_simulation).parameters
    params = list(sig)
    k = params.index("currents")
    assert params[k - 1] == "sq" and params[k + 1] == "stress" and sig["currents"].default is None
    assert params[-5:] == ["stress", "four_point", "clusters", "cage", "bond_order"]
    cs = inspect.signature(md.CurrentCorrelations).parameters
    assert list(cs) == ["q_max", "dq", "max_per_bin", "seed", "lags", "origin_every", "vacf"]
    assert [cs[p].default for p in list(cs)[1:]] == [None, 16, 0, None, None, True]
    jl = open(os.path.join(ROOT, "julia", "MDHip.jl")).read()
    for name in NAMES:
        assert "(:%s, LIB)" % name in jl
    assert "mutable struct CurrentCorrelations" in jl
    assert "currents::Union{Nothing,CurrentCorrelations}=nothing" in jl


def test_a_null_handle_is_refused():
    lib = _lib.load()
    assert lib.md_cur_setup(None, None, None, 0, 1, 1, 1) != 0
    assert lib.md_cur_sample(None, 1, None, None, 0, -1) != 0
    assert lib.md_cur_last(None, None) != 0
    assert lib.md_cur_read(None, None, None, None, None, None, None, None) != 0
    assert lib.md_cur_reset(None) != 0
    assert b"null handle" in lib.md_last_error(None)


def test_argument_checks():
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="q_max"):
            md.CurrentCorrelations(bad)
        with pytest.raises(ValueError, match="dq"):
            md.CurrentCorrelations(5.0, dq=bad)
    with pytest.raises(ValueError, match="dq needs q_max"):
        md.CurrentCorrelations(None, dq=0.5)
    with pytest.raises(ValueError, match="nothing to sample"):
        md.CurrentCorrelations(None, vacf=False)
    with pytest.raises(ValueError, match="max_per_bin"):
        md.CurrentCorrelations(5.0, max_per_bin=0)
    with pytest.raises(ValueError, match="origin_every"):
        md.CurrentCorrelations(5.0, lags=[1, 2])
    with pytest.raises(ValueError, match="origin_every needs explicit lags"):
        md.CurrentCorrelations(5.0, origin_every=3)
    with pytest.raises(ValueError, match="at most 64"):
        md.CurrentCorrelations(5.0, lags=[65], origin_every=1)
    c = md.CurrentCorrelations(None)
    assert c.q_max is None and c.with_vacf and c.nslots == 1 and c.n is None and len(c.lags) == 39
    with pytest.raises(ValueError, match="no wave vectors"):
        c.cl()
    c = md.CurrentCorrelations(6.0, vacf=False, lags=[2], origin_every=1)
    with pytest.raises(ValueError, match="vacf=True"):
        c.vacf()
    d = md.SelfDynamics(lags=[2, 5], origin_every=3)
    c = md.CurrentCorrelations(6.0, lags=[2, 5], origin_every=3)
    assert c.schedule(60) == d.schedule(60) and c.nslots == d.nslots


class _CurFake(_FakeDevice):
    """The recording handle with the cur calls.  Its read-back: per static sample s_tot = 3 N and s_long = N on every
    vector, per lag sample c_tot = 1.5 N, c_long = 0.5 N; Z(0) = 3 N per static sample and Z = N / (row + 1) per sample."""

    def cur_setup(self, n, e, nslots=0, nrows=0, vacf=False):
        self.setups.append("cur_setup")
        self.cur_args = (None if n is None else np.array(n), None if e is None else np.array(e), nslots, nrows, vacf)

    def cur_sample(self, static=True, slots=(), rows=(), origin=None):
        self._log("cur_sample", bool(static), tuple(int(v) for v in slots), tuple(int(v) for v in rows),
                  None if origin is None else int(origin))

    def cur_read(self):
        n, _, _, nrows, vacf = self.cur_args
        nvec = 0 if n is None else len(n)
        ns, nst = np.zeros(nrows, dtype=np.int64), 0
        for _, m, a in self.trace:
            if m == "cur_sample":
                nst += int(a[0])
                for r in a[2]:
                    ns[r] += 1
        one = np.ones(nvec)
        z = np.append(ns * N / (np.arange(nrows) + 1.0), nst * 3.0 * N) if vacf else None
        return (nst, nst * 3.0 * N * one, nst * 1.0 * N * one, ns, np.outer(ns * 1.5 * N, one),
                np.outer(ns * 0.5 * N, one), z)


def _cur_state():
    state, _ = _fake_state()
    dev = _CurFake()
    state.system.device = dev
    return state, dev


@pytest.mark.parametrize("total,lags,origin_every", [(40, [3, 6], 3), (40, None, None), (1, [3, 6], 3)])
def test_run_simulation_issues_the_scheduled_calls(tmp_path, total, lags, origin_every):
    f = 7
    state, dev = _cur_state()
    params = md.Parameters(1.0, N, 0.002, md.LennardJones())
    sched = dict(lags=lags, origin_every=origin_every)
    sq = md.StructureFactor(4.5, dynamic=True, **sched)
    cur = md.CurrentCorrelations(4.5, **sched)                  # cell edge 2: 9 vectors (tests/test_sampler_protocol.py)
    st = md.StressTensor(5)
    out = str(tmp_path / "out")
    with np.errstate(all="ignore"):
        md.run_simulation(state, params, md.NVE(), total, f, out, write_trajectory=False, sq=sq, currents=cur, stress=st)
    assert dev.setups == ["sq_setup", "cur_setup", "stress_setup"]                 # after sq, before stress
    n, e, nslots, nrows, vacf = dev.cur_args
    assert n.shape == (9, 3) and n.dtype == np.int32 and (nslots, nrows, vacf) == (cur.nslots, len(cur.lags), True)
    assert e.shape == (9, 3) and e.dtype == np.float64 and np.allclose(np.linalg.norm(e, axis=1), 1.0)
    assert np.array_equal(e, ref.directions(state.unitcell, n))
    events = cur.schedule(total)[1]
    want = []
    for step in range(total):
        ev = events.get(step)
        if step % f == 0 or ev is not None:
            smp, org = ev if ev is not None else ([], None)
            want.append((step, "sq_sample", (step % f == 0,) + _split(smp) + (org,)))
        if ev is not None:
            want.append((step, "cur_sample", (ev[1] is not None,) + _split(ev[0]) + (ev[1],)))
        if step % 5 == 0:
            want.append((step, "stress_sample", ()))
    assert dev.trace == want
    calls = [t[2] for t in dev.trace if t[1] == "cur_sample"]
    assert calls and all(static == (origin is not None) for static, _, _, origin in calls)
    if total > 1 and lags is not None:
        assert any(len(c[1]) > 1 for c in calls) and any(c[1] and c[3] is not None for c in calls)
    files = set(os.listdir(out))
    assert {"currents.txt", "vacf.txt", "sq.txt", "stress.txt"} <= files
    # the fake's read-back, normalised
    k = cur.nsamples > 0
    assert cur.nstatic == sum(c[0] for c in calls) and cur.nsamples.sum() == sum(len(c[1]) for c in calls)
    assert np.allclose(cur.cl0(), 1.0) and np.allclose(cur.ct0(), 1.0) and cur.vacf0() == 3.0
    assert cur.cl().shape == (len(cur.lags), cur.q.size) and cur.cl_vectors().shape == (len(cur.lags), 9)
    assert np.allclose(cur.cl()[k], 0.5) and np.allclose(cur.ct()[k], 0.5) and np.isnan(cur.cl()[~k]).all()
    assert np.allclose(cur.vacf()[k], (1.0 / (np.arange(len(cur.lags)) + 1.0))[k]) and np.isnan(cur.vacf()[~k]).all()
    # lags never reached are left out of the files
    rows = [l.split() for l in open(os.path.join(out, "vacf.txt")) if not l.startswith("#")]
    assert [int(r[0]) for r in rows] == [0] + [int(l) for l in cur.lags[k]]
    blocks = open(os.path.join(out, "currents.txt")).read().split("\n\n")
    assert len(blocks) == 1 + int(k.sum())
    # a second run accumulates; reset() empties
    before, nst = cur.nsamples.copy(), cur.nstatic
    del dev.trace[:]
    with np.errstate(all="ignore"):
        md.run_simulation(state, params, md.NVE(), total, f, out, write_trajectory=False, currents=cur)
    assert np.array_equal(cur.nsamples, 2 * before) and cur.nstatic == 2 * nst
    cur.reset()
    assert not cur.nsamples.any() and cur.nstatic == 0 and cur.n is None and np.isnan(cur.vacf()).all()


def test_vacf_only_and_currents_only(tmp_path):
    params = md.Parameters(1.0, N, 0.002, md.LennardJones())
    state, dev = _cur_state()
    cur = md.CurrentCorrelations(None, lags=[1], origin_every=2)
    out = str(tmp_path / "a")
    md.run_simulation(state, params, md.NVE(), 6, 2, out, write_trajectory=False, currents=cur)
    assert dev.cur_args[0] is None and dev.cur_args[4] is True
    assert "vacf.txt" in os.listdir(out) and "currents.txt" not in os.listdir(out)
    assert list(cur.nsamples) == [3] and cur.nstatic == 3
    state, dev = _cur_state()
    cur = md.CurrentCorrelations(4.5, vacf=False, lags=[1], origin_every=2)
    out = str(tmp_path / "b")
    md.run_simulation(state, params, md.NVE(), 6, 2, out, write_trajectory=False, currents=cur)
    assert dev.cur_args[4] is False
    assert "currents.txt" in os.listdir(out) and "vacf.txt" not in os.listdir(out)


def test_brownian_is_refused(tmp_path):
    state, dev = _cur_state()
    params = md.Parameters(1.0, N, 0.002, md.LennardJones())
    with pytest.raises(ValueError, match="Brownian"):
        md.run_simulation(state, params, md.Brownian(1.0), 6, 2, str(tmp_path / "o"), write_trajectory=False,
                          currents=md.CurrentCorrelations(4.5))
    assert "cur_setup" not in dev.setups


def test_file_formats(tmp_path):
    c = md.CurrentCorrelations(4.0, lags=[2, 5, 9], origin_every=5)
    U = np.diag([4.0, 4.0, 4.0])
    c._select(U)
    nvec, nb = c.n.shape[0], c.q.size
    ns = np.array([3, 0, 1])
    c._accumulate(4, np.full(nvec, 4 * 8 * 6.0), np.full(nvec, 4 * 8 * 2.0), ns, np.outer(ns * 8 * 3.0, np.ones(nvec)),
                  np.outer(ns * 8 * 1.0, np.ones(nvec)), np.array([3 * 8 * 1.5, 0.0, 8 * -0.75, 4 * 8 * 3.0]), 8, 3, 0.01)
    assert np.allclose(c.cl0(), 2.0) and np.allclose(c.ct0(), 2.0) and c.vacf0() == 3.0
    assert np.allclose(c.cl()[[0, 2]], 1.0) and np.allclose(c.ct()[[0, 2]], 1.0)
    p, pz = str(tmp_path / "currents.txt"), str(tmp_path / "vacf.txt")
    c.write(p)
    c.write_vacf(pz)
    text = open(p).read()
    assert text.startswith("# lag time q C_L C_T nsamples\n")
    blocks = text[text.index("\n") + 1:].split("\n\n")
    assert len(blocks) == 3                                     # lag 0 from the static sums, lags 2 and 9; 5 is left out
    for blk, (lag, n_s, val) in zip(blocks, [(0, 4, 2.0), (2, 3, 1.0), (9, 1, 1.0)]):
        lines = blk.strip("\n").split("\n")
        assert len(lines) == nb
        for b, line in enumerate(lines):
            w = line.split()
            assert int(w[0]) == lag and float(w[1]) == pytest.approx(lag * 0.01) and float(w[2]) == pytest.approx(c.q[b], abs=1e-6)
            assert float(w[3]) == pytest.approx(val) and float(w[4]) == pytest.approx(val) and int(w[5]) == n_s
    zl = open(pz).read().split("\n")
    assert zl[0] == "# lag time Z Z/Z(0) nsamples"
    rows = [l.split() for l in zl[1:] if l]
    assert [int(r[0]) for r in rows] == [0, 2, 9] and [int(r[4]) for r in rows] == [4, 3, 1]
    assert [float(r[2]) for r in rows] == [3.0, 1.5, -0.75] and [float(r[3]) for r in rows] == [1.0, 0.5, -0.25]


def test_reference_on_four_particles_by_hand():
    """L = 4; x = 0, 1, 2 on the x axis and (0, 2, 0); n = (1,0,0) gives the phase factors 1, i, -1, 1 and n = (0,1,0)
    gives 1, 1, 1, -1.  v = (1,0,0), (0,2,0), (3,0,0), (0,0,1):
      j(1,0,0) = v1 + i v2 - v3 + v4 = (-2, 2i, 1),  pL = -2,  |j|^2 = 9,  C_L = 4/4 = 1,  C_T = (9 - 4)/(2*4) = 0.625
      j(0,1,0) = v1 + v2 + v3 - v4 = (4, 2, -1),     pL = 2,   |j|^2 = 21, C_L = 4/4 = 1,  C_T = (21 - 4)/(2*4) = 2.125"""
    U = np.diag([4.0, 4.0, 4.0])
    x = np.array([[0.0, 0, 0], [1.0, 0, 0], [2.0, 0, 0], [0.0, 2.0, 0]])
    v = np.array([[1.0, 0, 0], [0, 2.0, 0], [3.0, 0, 0], [0, 0, 1.0]])
    n = np.array([[1, 0, 0], [0, 1, 0]], dtype=np.int32)
    j = ref.j_true(x, v, U, n)
    assert np.allclose(j, [[-2.0, 2.0j, 1.0], [4.0, 2.0, -1.0]], atol=1e-15, rtol=0)
    j = np.array([[-2.0, 2.0j, 1.0], [4.0, 2.0, -1.0]])
    e = ref.directions(U, n)
    assert np.array_equal(e, [[1.0, 0, 0], [0, 1.0, 0]])
    assert np.array_equal(ref.p_long(e, j.real), [-2.0, 2.0]) and np.array_equal(ref.p_long(e, j.imag), [0.0, 0.0])
    acc = ref.Accumulators(e, 1)
    acc.sample(j, True, [], 0)
    acc.sample(-0.5 * j, False, [(0, 0)], None)
    assert np.array_equal(acc.s_tot, [9.0, 21.0]) and np.array_equal(acc.s_long, [4.0, 4.0])
    assert np.array_equal(acc.c_tot[0], [-4.5, -10.5]) and np.array_equal(acc.c_long[0], [-2.0, -2.0])
    c = md.CurrentCorrelations(2.0, lags=[1], origin_every=1)
    c._set_vectors(U, n, analysis.wave_vector_lengths(U, n), np.array([0, 0]))
    c._accumulate(acc.nstatic, acc.s_tot, acc.s_long, acc.nsamples, acc.c_tot, acc.c_long,
                  np.array([ref.z_true(-0.5 * v, v)[0], ref.z_true(v, v)[0]]), 4, 3, 0.1)
    assert np.array_equal(c.e, e)
    assert np.array_equal(c.cl_vectors()[0], [-0.5, -0.5]) and np.array_equal(c.ct_vectors()[0], [-0.3125, -1.0625])
    assert np.array_equal(c.cl0(), [1.0]) and np.array_equal(c.ct0(), [(0.625 + 2.125) / 2])
    assert ref.z_true(v, v) == (15.0, 15.0) and c.vacf0() == 15.0 / 4 and list(c.vacf()) == [-7.5 / 4]
