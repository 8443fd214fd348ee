"""CPU tests of the self-dynamics layer (analysis.SelfDynamics, the binding, the Julia twin): the schedules, the
normalisations, the file formats and the argument checks.  The device sums themselves are tested in
tests/test_gpu_dynamics.py."""
import math
import os
import re

import numpy as np
import pytest

import moleculardynamics.jl_amd as md
from moleculardynamics.jl_amd import SelfDynamics, _lib, io as mdio
from moleculardynamics.jl_amd.analysis import SelfDynamics as SD2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("md_dyn_setup", "md_dyn_origin", "md_dyn_sample", "md_dyn_read", "md_dyn_reset")


def test_exports():
    assert SelfDynamics is SD2 and "SelfDynamics" in md.__all__
    for name in NAMES:
        assert name in _lib.EXPORTS
        assert hasattr(_lib.load(), name)
    header = open(os.path.join(ROOT, "include", "mdhip.h")).read()
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header)
    for name in ("dyn_setup", "dyn_origin", "dyn_sample", "dyn_read", "dyn_reset"):
        assert callable(getattr(md.MDDevice, name))


@pytest.mark.parametrize("T", [1, 2, 30, 200, 163437 + 50])
def test_log_schedule_is_the_snapshot_schedule(T):
    dyn = SelfDynamics()
    assert dyn.nslots == 1 and len(dyn.lags) == 39
    assert list(dyn.lags[:10]) == [1, 2, 3, 4, 6, 8, 11, 14, 20, 27] and dyn.lags[-1] == 163437
    assert dyn.lags[-1] == math.floor(1.35 ** 40)
    stops, events = dyn.schedule(T)
    expect = sorted({0} | {s for s in mdio.generate_log_times(filename=None) if s < T})
    assert stops == expect
    maxlog = 163437
    for s in stops:
        smp, org = events[s]
        assert org == (0 if s % maxlog == 0 else None)
        if s == 0:
            assert smp == []
        else:
            j = (s - 1) // maxlog
            assert smp == [(0, int(np.nonzero(dyn.lags == s - j * maxlog)[0][0]))]
    if T == 30:
        assert stops == [0, 1, 2, 3, 4, 6, 8, 11, 14, 20, 27]
    if T > maxlog:
        # the step maxlog: origin 0 at lag maxlog, sampled BEFORE origin 1 is stored in the same (only) slot
        assert events[maxlog] == ([(0, 38)], 0)
        assert events[maxlog + 1] == ([(0, 0)], None)


def test_explicit_schedule_by_hand():
    dyn = SelfDynamics(lags=(1, 2, 5), origin_every=3)
    assert dyn.nslots == 2 and list(dyn.lags) == [1, 2, 5]
    stops, events = dyn.schedule(12)
    origins = [(s, events[s][1]) for s in stops if events[s][1] is not None]
    assert origins == [(0, 0), (3, 1), (6, 0), (9, 1)]
    triples = [(s, slot, row) for s in stops for slot, row in events[s][0]]
    assert triples == [(1, 0, 0), (2, 0, 1), (4, 1, 0), (5, 0, 2), (5, 1, 1), (7, 0, 0), (8, 1, 2), (8, 0, 1),
                       (10, 1, 0), (11, 0, 2), (11, 1, 1)]
    # a slot is never overwritten while one of its samples is pending
    last_use = {}
    for s in stops:
        smp, org = events[s]
        for slot, _ in smp:
            last_use[slot] = s
        if org is not None:
            assert last_use.get(org, -1) <= s
    assert SelfDynamics(lags=(7,), origin_every=7).nslots == 1
    assert SelfDynamics(lags=(640,), origin_every=10).nslots == 64


def test_argument_checks():
    with pytest.raises(ValueError, match="16"):
        SelfDynamics(q=np.ones(17))
    with pytest.raises(ValueError, match="finite"):
        SelfDynamics(q=(1.0, math.inf))
    with pytest.raises(ValueError, match="nbins"):
        SelfDynamics(nbins=8193, r_max=1.0)
    with pytest.raises(ValueError, match="r_max"):
        SelfDynamics(nbins=10)
    with pytest.raises(ValueError, match="r_max"):
        SelfDynamics(nbins=10, r_max=-1.0)
    with pytest.raises(ValueError, match="origin_every"):
        SelfDynamics(origin_every=5)
    with pytest.raises(ValueError, match="origin_every"):
        SelfDynamics(lags=(1, 2))
    with pytest.raises(ValueError, match="positive"):
        SelfDynamics(lags=(0, 2), origin_every=1)
    with pytest.raises(ValueError, match="distinct"):
        SelfDynamics(lags=(2, 2), origin_every=1)
    with pytest.raises(ValueError, match="65 origin slots"):
        SelfDynamics(lags=(641,), origin_every=10)
    d = SelfDynamics(q=(), nbins=0)
    assert d.q.size == 0 and d.sums.shape == (39, 2)


def _synthetic(dim=3):
    """Sums of a known answer: every particle displaced by the same vector in every sample."""
    n, ns = 1000, np.array([2, 0, 3])
    q = np.array([1.5, 4.0])
    dyn = SelfDynamics(q=q, r_max=2.0, nbins=4, lags=(1, 2, 4), origin_every=4)
    disp = np.array([[0.3, -0.4, 0.0], [0.0, 0.0, 0.0], [1.0, 0.5, -0.5]])[:, :dim]
    d2 = (disp ** 2).sum(1)
    sums = np.zeros((3, 4))
    sums[:, 0] = n * ns * d2
    sums[:, 1] = n * ns * d2 * d2
    for j, qq in enumerate(q):
        sums[:, 2 + j] = n * ns * np.cos(qq * disp).sum(1)
    hist = np.zeros((3, 4), np.int64)
    k = np.searchsorted(dyn.edges ** 2, d2, "right") - 1
    for r in range(3):
        if ns[r] and k[r] < 4:
            hist[r, k[r]] = n * ns[r]
    dyn._accumulate(ns, sums, hist, n, dim, 0.01)
    return dyn, n, ns, disp, d2, q, k


@pytest.mark.parametrize("dim", [2, 3])
def test_normalisations(dim):
    dyn, n, ns, disp, d2, q, k = _synthetic(dim)
    msd = dyn.msd()
    assert np.allclose(msd[[0, 2]], d2[[0, 2]], rtol=1e-14) and math.isnan(msd[1])
    # every particle moved by the same vector: d <d4> / ((d + 2) <d2>^2) - 1 = d / (d + 2) - 1
    assert np.allclose(dyn.alpha2()[[0, 2]], dim / (dim + 2.0) - 1.0, rtol=1e-13)
    fs = dyn.fs()
    assert fs.shape == (3, 2)
    for j, qq in enumerate(q):
        assert np.allclose(fs[[0, 2], j], np.cos(qq * disp[[0, 2]]).sum(1) / dim, rtol=1e-14)
    g = dyn.van_hove()
    assert g.shape == (3, 4)
    e = dyn.edges
    vk = 4.0 * math.pi / 3.0 * (e[1:] ** 3 - e[:-1] ** 3) if dim == 3 else math.pi * (e[1:] ** 2 - e[:-1] ** 2)
    assert np.allclose(g[0], dyn.hist[0] / (ns[0] * n * vk), rtol=1e-14)
    # G_s integrates to the fraction counted: sum_k G_s V_k = 1 for a row whose displacement is inside r_max
    assert abs(float(np.sum(g[0] * vk)) - 1.0) < 1e-14
    assert np.all(np.isnan(g[1]))
    # samples accumulate; reset empties them
    dyn._accumulate(ns, dyn.sums.copy(), dyn.hist.copy(), n, dim, 0.01)
    assert list(dyn.nsamples) == [4, 0, 6] and np.allclose(dyn.msd()[[0, 2]], d2[[0, 2]] * 1.0)
    dyn.reset()
    assert not dyn.nsamples.any() and not dyn.sums.any() and not dyn.hist.any()


def test_file_formats(tmp_path):
    dyn, n, ns, disp, d2, q, k = _synthetic(3)
    p = str(tmp_path / "dynamics.txt")
    dyn.write(p)
    lines = open(p).read().splitlines()
    assert lines[0] == "# lag time msd alpha2 Fs(q=1.5) Fs(q=4) nsamples"
    assert len(lines) == 3                          # lag 2 was never reached: left out
    msd, a2, fs = dyn.msd(), dyn.alpha2(), dyn.fs()
    for line, r, lag in zip(lines[1:], (0, 2), (1, 4)):
        expect = ("%d %.6e %.6e %.6e" + " %.6e" * 2 + " %d") % ((lag, lag * 0.01, msd[r], a2[r]) + tuple(fs[r]) + (ns[r],))
        assert line == expect
    v = str(tmp_path / "vanhove.txt")
    dyn.write_van_hove(v)
    text = open(v).read()
    assert text.startswith("# lag r G_s count\n")
    blocks = text[len("# lag r G_s count\n"):].split("\n\n")
    assert len(blocks) == 2
    g = dyn.van_hove()
    for blk, r, lag in zip(blocks, (0, 2), (1, 4)):
        rows = blk.strip("\n").split("\n")
        assert len(rows) == 4
        for b, row in enumerate(rows):
            assert row == "%d %.6f %.6e %d" % (lag, dyn.r[b], g[r, b], dyn.hist[r, b])
    # an explicit dt overrides the one run_simulation recorded
    dyn.write(p, dt=0.5)
    assert open(p).read().splitlines()[1].split()[1] == "%.6e" % 0.5


def test_run_simulation_has_the_keyword():
    import inspect
    sig = inspect.signature(md.run_simulation)
    assert "dynamics" in sig.parameters and sig.parameters["dynamics"].default is None


def test_julia_twin_binds_the_entries():
    src = open(os.path.join(ROOT, "julia", "MDHip.jl")).read()
    for name in NAMES:
        assert re.search(r"\(:" + name + r",\s*LIB\)", src), name
    assert "struct SelfDynamics" in src or "mutable struct SelfDynamics" in src
    assert re.search(r"dynamics::Union\{Nothing,\s*SelfDynamics\}\s*=\s*nothing", src)
    assert "dynamics.txt" in src and "vanhove.txt" in src
