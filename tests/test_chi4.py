"""CPU: the four-point sampler's host layers -- the exported symbols and their declarations, FourPoint's argument checks,
schedule, exact normalisation and file formats, its place in run_simulation's signature and sampler order (on a fake
handle that records every call, as tests/test_sampler_protocol.py does) -- and the numpy reference of the GPU tests
(tests/chi4_reference.py) against a case of four particles worked out by hand."""
import inspect
import os
import re

import numpy as np
import pytest

import moleculardynamics.jl_amd as md
from moleculardynamics.jl_amd import _lib, analysis
from tests import chi4_reference as ref
from tests.test_cage import _CageFake
from tests.test_sampler_protocol import N, _fake_state, _split

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["md_chi4_setup", "md_chi4_origin", "md_chi4_sample", "md_chi4_last", "md_chi4_read", "md_chi4_reset"]


def test_symbols_bindings_and_build_rule():
    assert "FourPoint" in md.__all__ and md.FourPoint is analysis.FourPoint
    header = open(os.path.join(ROOT, "include", "mdhip.h")).read()
    lib = _lib.load()
    for name in NAMES:
        assert name in _lib.EXPORTS
        assert hasattr(lib, name)
        assert re.search(r"\bint\s+" + name + r"\s*\(", header)
    assert len(lib.md_chi4_setup.argtypes) == 6 and len(lib.md_chi4_last.argtypes) == 4
    assert len(lib.md_chi4_read.argtypes) == 5
    assert "N*d*20" in header and "N*d*12" in header and "MDHIP_CHI4_ALLOC_LIMIT" in header and "2^63 - 1" in header
    for name in ("chi4_setup", "chi4_origin", "chi4_sample", "chi4_last", "chi4_read", "chi4_reset"):
        assert callable(getattr(md.MDDevice, name))
    mk = open(os.path.join(ROOT, "moleculardynamics", "jl_amd", "csrc", "Makefile")).read()
    assert re.search(r"^libmdhip\.so:.*\bmd_chi4\.hpp\b", mk, re.M)
    sig = inspect.signature(md.run_simulation).parameters
    params = list(sig)
    assert params[-4:] == ["four_point", "clusters", "cage", "bond_order"] and params[-5] == "stress"
    assert sig["four_point"].default is None
    assert list(inspect.signature(md.FourPoint).parameters) == ["a", "q_max", "dq", "max_per_bin", "seed", "lags",
                                                                 "origin_every"]
    jl = open(os.path.join(ROOT, "julia", "MDHip.jl")).read()
    for name in NAMES:
        assert "(:%s, LIB)" % name in jl
    assert "mutable struct FourPoint" in jl and "four_point::Union{Nothing,FourPoint}=nothing" in jl


def test_a_null_handle_is_refused():
    lib = _lib.load()
    assert lib.md_chi4_setup(None, 0.3, None, 0, 1, 1) != 0
    assert lib.md_chi4_origin(None, 0) != 0 and lib.md_chi4_sample(None, None, None, 0) != 0
    assert lib.md_chi4_last(None, None, None, None) != 0 and lib.md_chi4_read(None, None, None, None, None) != 0
    assert lib.md_chi4_reset(None) != 0
    assert b"null handle" in lib.md_last_error(None)


def test_argument_checks():
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="a must be finite"):
            md.FourPoint(bad)
        with pytest.raises(ValueError, match="q_max"):
            md.FourPoint(0.3, q_max=bad)
        with pytest.raises(ValueError, match="dq"):
            md.FourPoint(0.3, q_max=5.0, dq=bad)
    with pytest.raises(ValueError, match="dq needs q_max"):
        md.FourPoint(0.3, dq=0.5)
    with pytest.raises(ValueError, match="max_per_bin"):
        md.FourPoint(0.3, q_max=5.0, max_per_bin=0)
    with pytest.raises(ValueError, match="origin_every"):
        md.FourPoint(0.3, lags=[1, 2])
    with pytest.raises(ValueError, match="origin_every needs explicit lags"):
        md.FourPoint(0.3, origin_every=3)
    with pytest.raises(ValueError, match="at most 64"):
        md.FourPoint(0.3, lags=[65], origin_every=1)
    f = md.FourPoint(0.3)
    assert f.q_max is None and f.nslots == 1 and f.n is None and len(f.lags) == 39
    with pytest.raises(ValueError, match="no wave vectors"):
        f.s4()
    f = md.FourPoint(0.25, q_max=7.0, dq=0.5, max_per_bin=3, seed=9, lags=[64], origin_every=1)
    assert f.nslots == 64 and (f.a, f.q_max, f.dq, f.max_per_bin, f.seed) == (0.25, 7.0, 0.5, 3, 9)
    # more vectors than the device sampler takes
    f = md.FourPoint(0.3, q_max=5.0, max_per_bin=100000)        # ~8400 vectors: fine for S(q), too many here
    with pytest.raises(ValueError, match="at most 4096"):
        f._select(np.diag([20.0, 20.0, 20.0]))


@pytest.mark.parametrize("lags,origin_every,total", [(None, None, 3000), ([2, 5], 3, 60), ([1, 7, 20], 4, 45), ([3], 1, 1)])
def test_schedule_is_self_dynamics(lags, origin_every, total):
    f = md.FourPoint(0.3, lags=lags, origin_every=origin_every)
    d = md.SelfDynamics(lags=lags, origin_every=origin_every)
    assert f.schedule(total) == d.schedule(total)
    assert np.array_equal(f.lags, d.lags) and f.nslots == d.nslots
    if lags is None:
        assert f.nslots == 1                                    # samples before the origin: one slot is enough


class _Chi4Fake(_CageFake):
    """The recording handle with the chi4 calls: every sample reads Q = N on even rows and N - 1 on odd ones."""

    def chi4_setup(self, a, n, nslots, nrows):
        self.setups.append("chi4_setup")
        self.chi4_args = (a, None if n is None else np.array(n), nslots, nrows)

    def chi4_sample(self, slots, rows):
        self._log("chi4_sample", tuple(int(v) for v in slots), tuple(int(v) for v in rows))

    def chi4_origin(self, slot):
        self._log("chi4_origin", int(slot))

    def chi4_read(self):
        n, nrows = self.chi4_args[1], self.chi4_args[3]
        nvec = 0 if n is None else len(n)
        ns = np.zeros(nrows, dtype=np.int64)
        for _, m, a in self.trace:
            if m == "chi4_sample":
                for r in a[1]:
                    ns[r] += 1
        q = N - np.arange(nrows) % 2
        return ns, ns * q, ns * q * q, np.tile((ns * N * 0.5)[:, None], (1, nvec))


def _chi4_state():
    state, _ = _fake_state()
    dev = _Chi4Fake()
    state.system.device = dev
    return state, dev


@pytest.mark.parametrize("lags,origin_every", [([3, 6], 3), (None, None)])
def test_run_simulation_drives_the_four_point_sampler_last(tmp_path, lags, origin_every):
    total, f = 40, 7
    state, dev = _chi4_state()
    params = md.Parameters(1.0, N, 0.002, md.LennardJones())
    sched = dict(lags=lags, origin_every=origin_every)
    dyn = md.SelfDynamics(**sched)
    cage = md.CageDynamics(1.5, **sched)
    fp = md.FourPoint(0.3, q_max=4.5, **sched)                  # cell edge 2: 9 vectors (tests/test_sampler_protocol.py)
    out = str(tmp_path / "out")
    with np.errstate(all="ignore"):
        md.run_simulation(state, params, md.NVE(), total, f, out, write_trajectory=False, dynamics=dyn, four_point=fp,
                          cage=cage)
    assert dev.setups == ["dyn_setup", "cage_setup", "chi4_setup"]              # once, and after cage
    a, n, nslots, nrows = dev.chi4_args
    assert a == 0.3 and n.shape == (9, 3) and n.dtype == np.int32 and (nslots, nrows) == (fp.nslots, len(fp.lags))
    events = fp.schedule(total)[1]
    want, stops = [], {total - 1}
    for step in range(total):
        before = len(want)
        output = step % f == 0
        ev = events.get(step)
        for name in ("dyn", "cage", "chi4"):                    # four_point's calls come last at a shared step
            if ev is not None and ev[0]:
                want.append((step, name + "_sample", _split(ev[0])))                       # the samples before the origin
            if ev is not None and ev[1] is not None:
                want.append((step, name + "_origin", (ev[1],)))
        if len(want) > before or output:
            stops.add(step)
    assert dev.trace == want
    assert list(np.cumsum(dev.segments) - 1) == sorted(stops)                              # the segments stop there
    assert any(t[1] == "chi4_sample" for t in want) and any(t[1] == "chi4_origin" for t in want)
    if lags is not None:
        assert any(t[1] == "chi4_sample" and len(t[2][0]) > 1 for t in want)               # several rows in one call
        shared = [s for s in range(total) if events.get(s) and events[s][0] and events[s][1] is not None]
        assert shared                                                                      # a step with both exists
        names = [t[1] for t in want if t[0] == shared[0] and t[1].startswith("chi4")]
        assert names == ["chi4_sample", "chi4_origin"]
    else:
        assert fp.nslots == 1 and all(len(t[2][0]) == 1 for t in want if t[1] == "chi4_sample")
    assert {"chi4.txt", "s4.txt", "cage.txt", "dynamics.txt"} <= set(os.listdir(out))
    # the fake's read-back, normalised: Q = N on even rows and N - 1 on odd ones, no variance within a row; S4 = 1/2
    k = fp.nsamples > 0
    assert fp.nsamples.sum() == sum(len(t[2][0]) for t in want if t[1] == "chi4_sample")
    q = (N - np.arange(len(fp.lags)) % 2) / N
    assert np.array_equal(fp.overlap()[k], q[k]) and not fp.chi4()[k].any() and np.isnan(fp.chi4()[~k]).all()
    assert np.allclose(fp.s4()[k], 0.5) and fp.s4().shape == (len(fp.lags), fp.q.size)
    assert np.allclose(fp.s4_vectors()[k], 0.5) and fp.s4_vectors().shape == (len(fp.lags), 9)
    # a second run accumulates; reset() empties
    before = fp.nsamples.copy()
    del dev.trace[:]                                            # (the fake counts its samples from the trace)
    with np.errstate(all="ignore"):
        md.run_simulation(state, params, md.NVE(), total, f, out, write_trajectory=False, four_point=fp)
    assert dev.setups[-1] == "chi4_setup" and np.array_equal(fp.nsamples, 2 * before)
    fp.reset()
    assert not fp.nsamples.any() and fp.n is None and np.isnan(fp.chi4()).all() and np.isnan(fp.overlap()).all()


def test_chi4_only_writes_one_file(tmp_path):
    state, dev = _chi4_state()
    params = md.Parameters(1.0, N, 0.002, md.LennardJones())
    fp = md.FourPoint(0.3, lags=[1], origin_every=2)
    out = str(tmp_path / "out")
    md.run_simulation(state, params, md.NVE(), 6, 2, out, write_trajectory=False, four_point=fp)
    assert dev.chi4_args[1] is None and "chi4.txt" in os.listdir(out) and "s4.txt" not in os.listdir(out)
    assert list(fp.nsamples) == [3]


def test_normalisation_is_exact_in_integers():
    """ns = 3, Q = 2^40 + {0, 1, 2}: sum Q^2 = 3 2^80 + 6 2^40 + 5 and (sum Q)^2 / 3 = 3 2^80 + 6 2^40 + 3 agree to 2 in
    2^82 -- nothing of the variance survives an fp64 evaluation; in integers chi4 = 6 / (9 N) exactly."""
    n_particles = 1 << 41
    qs = [(1 << 40) + k for k in range(3)]
    f = md.FourPoint(0.3, lags=[1, 2], origin_every=2)
    f._accumulate([3, 0], [sum(qs), 0], [sum(q * q for q in qs), 0], None, n_particles, 0.01)
    c = f.chi4()
    assert c[0] == 6 / (9 * n_particles) and c[0] > 0.0 and np.isnan(c[1])
    assert f.overlap()[0] == (3 * (1 << 40) + 3) / (3 * n_particles) and np.isnan(f.overlap()[1])
    naive = (float(sum(q * q for q in qs)) / 3 - (float(sum(qs)) / 3) ** 2) / n_particles
    assert naive != c[0]                                        # (what the integer numerator is for)
    # the sums of several runs pass 2^63: they are kept as integers of any size
    for _ in range(40):
        f._accumulate([3, 0], [sum(qs), 0], [sum(q * q for q in qs), 0], None, n_particles, 0.01)
    assert int(f.sum_q2[0]) == 41 * sum(q * q for q in qs) > 1 << 63
    assert f.chi4()[0] == 6 / (9 * n_particles)


def test_file_formats(tmp_path):
    f = md.FourPoint(0.3, q_max=4.5, dq=1.0, lags=[1, 4, 9], origin_every=3)
    f._select(np.diag([2.0, 2.0, 2.0]))                          # 3 vectors |q| = pi, 6 of pi sqrt(2)
    assert list(f.nvectors) == [3, 6] and f.sum_s4.shape == (3, 9)
    n_particles = 8
    s4 = np.zeros((3, 9))
    s4[0, :3], s4[0, 3:] = 16.0, 4.0
    s4[2] = np.arange(9.0)
    f._accumulate([2, 0, 1], [12, 0, 3], [80, 0, 9], s4, n_particles, 0.01)
    p1, p2 = str(tmp_path / "chi4.txt"), str(tmp_path / "s4.txt")
    f.write(p1)
    f.write_s4(p2)
    lines = open(p1).read().splitlines()
    assert lines[0] == "# lag time Q/N chi4 nsamples" and len(lines) == 3  # the lag without a sample has no row
    # Q = 4 and 8: <Q> / N = 0.75, chi4 = (2 * 80 - 144) / (4 * 8) = 0.5
    assert lines[1] == "1 %.6e %.6e %.6e 2" % (0.01, 0.75, 0.5)
    assert lines[2] == "9 %.6e %.6e %.6e 1" % (0.09, 0.375, 0.0)
    text = open(p2).read()
    head = "# lag time q S4 nvectors nsamples\n"
    assert text.startswith(head)
    blocks = text[len(head):].split("\n\n")
    assert len(blocks) == 2
    rows = blocks[0].strip("\n").split("\n")
    assert rows == ["1 %.6e %.6f %.6e 3 2" % (0.01, np.pi, 1.0), "1 %.6e %.6f %.6e 6 2" % (0.01, np.pi * np.sqrt(2.0), 0.25)]
    rows = blocks[1].strip("\n").split("\n")
    assert rows == ["9 %.6e %.6f %.6e 3 1" % (0.09, np.pi, 1.0 / 8), "9 %.6e %.6f %.6e 6 1" % (0.09, np.pi * np.sqrt(2.0), 5.5 / 8)]
    sv = f.s4_vectors()
    assert sv.shape == (3, 9) and np.isnan(sv[1]).all() and np.array_equal(sv[2], np.arange(9.0) / 8)


def test_reference_on_four_particles_by_hand():
    """L = 4, a = 0.5.  Particle 0 rests; 1 moves 0.5 along x (d2 == a2: not slow); 2 moves (0.25, 0.25, 0.25) (d2 = 0.1875 < 0.25);
    3 leaves through the x face and returns to its wrapped position, image +1 (d = 4)."""
    U = np.diag([4.0, 4.0, 4.0])
    x0 = np.array([[0.5, 0.5, 0.5], [1.0, 2.0, 3.0], [2.0, 1.0, 0.0], [3.5, 3.0, 1.0]])
    x1 = x0.copy()
    x1[1, 0] += 0.5
    x1[2] += [0.25, 0.25, 0.25]
    n0 = np.zeros((4, 3), np.int32)
    n1 = n0.copy()
    n1[3, 0] = 1
    de, d2 = ref.displacement(x0, n0, x1, n1, U)
    assert d2.tolist() == [0.0, 0.25, 0.1875, 16.0] and de[3].tolist() == [4.0, 0.0, 0.0]
    slow, q = ref.overlap(x0, n0, x1, n1, U, 0.5)
    assert slow.tolist() == [1, 0, 1, 0] and q == 2 and slow.dtype == np.uint8
    assert ref.overlap(x0, n0, x1, n1, U, np.nextafter(0.5, 1.0))[1] == 3       # just above the threshold: 1 is slow too
    assert ref.overlap(x0, n0, x1, n1, np.array([4.0, 4.0, 4.0]), 0.5)[1] == 2   # (a diagonal cell given as its edges)
    # W over particles 0 and 2, origin positions: f = x / 4
    n = np.array([[1, 0, 0], [0, 2, 0], [1, 1, 1], [4, 0, -4]], np.int32)
    w = ref.w_true(x0, U, n, slow)
    # n.f: particle 0 -> 1/8, 1/4, 3/8, 0; particle 2 -> 1/2, 1/2, 3/4, 2
    s = np.sqrt(0.5)
    want = np.array([(s - 1.0) + 1j * s, -1.0 + 1j, -s + 1j * (s - 1.0), 2.0 + 0j])
    assert np.abs(w - want).max() <= 4e-16
    assert np.all(ref._bound(4, U, n) >= 4 * 128 * 2.0 ** -53)
