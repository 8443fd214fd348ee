"""GPU: swap Monte Carlo (md_swap_*) against the numpy + oracle reference of tests/swap_reference.py.

Systems (swap_reference.case): `poly` -- poly_system(), 2-D, N = 1200 (five tiles, the last one ragged), Polydisperse,
cutoff 1.5, kT 0.11, fraction 0.02; `lj` -- with_diameters(lj_system(1000), 0.9, 1.1), 3-D, cutoff 2.5, kT 1, fraction 0.01;
`lj_sheared` -- the same in a general cell.  Each on both row formats a handle can have: 16-bit tiled rows (the default
build) and 32-bit global rows (MDHIP_NO_TILES=1, the switch tests/test_gpu_row_audit.py uses; real ghost copies).

Parity is exact in everything that is an integer or a permuted double (partner, status, diameters) and 1e-12 S in dU, S the
sum of the magnitudes the difference is made of -- the relative tolerance tests/test_gpu_parity.py puts on U.  Equal
statuses are a fair demand only away from a tie of the Metropolis test: every test that compares statuses first asserts,
on the reference alone, swap_reference.conditions() (a 1000-fold cushion over the tolerance; at least 10 decided swaps and
one each accepted, rejected, blocked, lost)."""
import os

import numpy as np
import pytest

from tests import swap_reference as sr
from tests.test_swap import reference

pytestmark = pytest.mark.gpu

FORMATS = ("tiled", "rows32")


def _device(c, fmt, monkeypatch, skin=None, upload=True):
    from moleculardynamics.jl_amd import MDDevice
    if fmt == "rows32":
        monkeypatch.setenv("MDHIP_NO_TILES", "1")
    s = c["system"]
    d = MDDevice(s["dim"], s["n"], s.get("cell", s["box"]), c["cutoff"])
    d.set_potential(c["kind"], c["params"])
    if skin is not None:
        d.set_skin(skin)
    if upload:
        d.upload(s["x"], s["v"], s["f"], s["img"], s["diam"])
    return d


def _check_format(d, fmt):
    info = d.list_rows(0)["info"]
    assert info["list_valid"] == 1
    assert (info["tiled"], info["rows32"]) == ((1, 0) if fmt == "tiled" else (0, 1)), info
    if fmt == "rows32":
        assert info["n_ghost"] > 0 and info["virtual_ghosts"] == 0          # real ghost copies of the diameters


def _fair(name):
    c, fr, rounds = reference(name)
    ok, text = sr.conditions(rounds, c["ktemp"])
    assert ok, text
    return c, fr, rounds


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("name", ["poly", "lj", "lj_sheared"])
def test_rounds_match_the_reference(monkeypatch, name, fmt):
    """8 rounds, one md_swap_rounds(1) at a time: partner and status by particle id equal, the diameters bit-equal after
    every round, |dU_dev - dU_ref| <= 1e-12 S per decided swap."""
    c, fr, rounds = _fair(name)
    with _device(c, fmt, monkeypatch) as d:
        d.swap_setup(c["fraction"], None, c["seed"])
        for r, ref in enumerate(rounds):
            res = d.swap_rounds(1, c["ktemp"], first_round=r)
            partner, status, du = d.swap_last()
            diam = d.diameters()
            st = ref["status"]
            assert np.array_equal(partner, ref["partner"]), (name, r)
            assert np.array_equal(status, st), (name, r, np.flatnonzero(status != st))
            assert np.array_equal(diam, ref["diam"]), (name, r)
            dec = st >= sr.REJECTED
            err = np.abs(du - ref["du"])
            rel = err[dec] / np.maximum(ref["S"][dec], 1e-300)         # (S = 0: a swap of two particles nothing touches)
            print(name, fmt, "round", r, "decided", int(dec.sum()), "max |dU err| / S %.3g" % (rel.max() if dec.any() else 0.0))
            assert np.all(err[dec] <= 1e-12 * ref["S"][dec]) and np.all(du[~dec] == 0.0)
            want = [int((st >= sr.VOID).sum())] + [int((st == k).sum()) for k in (sr.VOID, sr.LOST, sr.BLOCKED, sr.FILTERED,
                                                                                  sr.ACCEPTED)]
            assert [res[k] for k in d.SWAP_COUNTS] == want and res["decided"] == int(dec.sum())
        _check_format(d, fmt)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("name", ["poly", "lj"])
def test_batching_and_non_interaction(monkeypatch, name, fmt):
    """8 rounds in one call equal 8 calls of one round (and 3 + 5 with first_round continuing the stream), in counts and
    diameters; du_accepted of the call equals the md_compute_forces energy after minus before to 1e-12 sum S."""
    c, fr, rounds = _fair(name)
    acc_s = sum(r["S"][r["status"] == sr.ACCEPTED].sum() for r in rounds)
    acc_du = sum(r["du"][r["status"] == sr.ACCEPTED].sum() for r in rounds)
    with _device(c, fmt, monkeypatch) as d:
        u0, _ = d.compute_forces()
        d.swap_setup(c["fraction"], None, c["seed"])
        whole = d.swap_rounds(sr.ROUNDS, c["ktemp"])
        diam = d.diameters()
        u1, w1 = d.compute_forces()
        assert np.array_equal(diam, rounds[-1]["diam"])
        assert whole["U"] == u1 and whole["W"] == w1                   # the call's own force refresh
        print(name, fmt, "du_accepted %.15g  U1 - U0 %.15g  sum S %.6g" % (whole["du_accepted"], u1 - u0, acc_s))
        assert abs(whole["du_accepted"] - (u1 - u0)) <= 1e-12 * acc_s
        assert abs(whole["du_accepted"] - acc_du) <= 1e-12 * acc_s
        for k in ("accepted", "blocked", "decided"):
            code = dict(accepted=sr.ACCEPTED, blocked=sr.BLOCKED).get(k)
            want = sum(int(((r["status"] == code) if code else (r["status"] >= sr.REJECTED)).sum()) for r in rounds)
            assert whole[k] == want
        # again from the start, in two calls
        d.upload(diameters=c["system"]["diam"])
        a = d.swap_rounds(3, c["ktemp"], first_round=0)
        b = d.swap_rounds(sr.ROUNDS - 3, c["ktemp"], first_round=3)
        assert np.array_equal(d.diameters(), diam)
        for k in d.SWAP_COUNTS + ("decided",):
            assert a[k] + b[k] == whole[k], k
        assert b["U"] == u1


STALE = [("poly", "tiled", None, "nve"), ("poly", "tiled", None, "nvt"), ("poly", "tiled", 0.0, "nve"),
         ("poly", "tiled", 0.0, "nvt"), ("poly", "rows32", None, "nve"), ("lj", "rows32", None, "nvt")]


@pytest.mark.parametrize("name,fmt,skin,ens", STALE)
def test_no_stale_copy_of_a_diameter(oracle, monkeypatch, name, fmt, skin, ens):
    """After MD steps (inner rows in use where the build has them) and swap rounds: U, W and the forces the call left are
    those of oracle.forces_brute with the swapped diameters (test_polydisperse_2d's tolerances), and 20 further md_run
    steps match oracle.run from the downloaded state with those diameters to 1e-10.  The poly diameters span 0.6 - 1.2: a
    stale copy moves forces by O(1)."""
    from moleculardynamics.jl_amd import _lib
    c, _, _ = reference(name)
    s = c["system"]
    dt = 0.005 if name == "poly" else 0.002
    nsteps = 20
    from moleculardynamics.jl_amd.thermostat import draw_bussi
    kt = np.full(nsteps, c["ktemp"])
    r1, r2 = draw_bussi(s["dim"] * (s["n"] - 1.0), np.random.default_rng(3), nsteps)
    with _device(c, fmt, monkeypatch, skin=skin) as d:
        d.run(12, dt)
        st0 = d.stats()
        if fmt == "tiled" and skin is None:
            assert st0["prunes"] > 0                                   # pruning is on: the force kernel walks inner rows
        d.swap_setup(0.05, None, 77)
        res = d.swap_rounds(4, c["ktemp"])
        assert res["accepted"] >= 5
        diam = d.diameters()
        assert not np.array_equal(diam, s["diam"]) and np.array_equal(np.sort(diam), np.sort(s["diam"]))
        x, v, f, img = d.download()
        f_ref, u_ref, w_ref = sr.forces(s, c["cutoff"], c["pot"], diam, x=x)
        scale = max(1.0, np.abs(f_ref).max())
        print(name, fmt, skin, ens, "force err %.3g of %.3g  dU %.3g  dW %.3g" % (
            np.abs(f - f_ref).max(), scale, abs(res["U"] - u_ref) / abs(u_ref), abs(res["W"] - w_ref) / abs(w_ref)))
        assert np.abs(f - f_ref).max() <= 1e-11 * scale
        assert abs(res["U"] - u_ref) <= 1e-12 * abs(u_ref) and abs(res["W"] - w_ref) <= 1e-12 * abs(w_ref)
        with sr._cell_of(s):
            if ens == "nvt":
                ref = oracle.run(x, img, v, f, diam, s["box"], c["cutoff"], c["pot"], dt, nsteps, ensemble=1, tau=0.1,
                                 ktemp=kt, r1=r1, r2=r2, use_cells=False)
                d.run(nsteps, dt, _lib.MD_NVT, 0.1, None, kt, r1, r2)
            else:
                ref = oracle.run(x, img, v, f, diam, s["box"], c["cutoff"], c["pot"], dt, nsteps, use_cells=False)
                d.run(nsteps, dt)
        x2, v2, _, _ = d.download()
        print("   trajectory err x %.3g v %.3g" % (np.abs(x2 - ref["x"]).max(), np.abs(v2 - ref["v"]).max()))
        assert np.abs(x2 - ref["x"]).max() <= 1e-10 and np.abs(v2 - ref["v"]).max() <= 1e-10
        assert np.array_equal(d.diameters(), diam)
        _check_format(d, fmt)


@pytest.mark.parametrize("fmt", FORMATS)
def test_rows_untouched(monkeypatch, fmt):
    c, _, _ = reference("poly")
    with _device(c, fmt, monkeypatch) as d:
        d.compute_forces()
        before, rows0 = d.stats()["rebuilds"], d.list_rows(0)
        d.swap_setup(c["fraction"], None, c["seed"])
        d.swap_rounds(sr.ROUNDS, c["ktemp"])
        rows1 = d.list_rows(0)
        assert d.stats()["rebuilds"] == before == 1
        assert np.array_equal(rows0["entries"], rows1["entries"]) and rows0["info"] == rows1["info"]
        assert np.array_equal(rows0["pos"], rows1["pos"])


def test_filter(monkeypatch):
    """max_diameter_difference = 0.05: no accepted swap exceeds it; the proposer, live and blocked sets are those of the
    unfiltered run."""
    c, fr, rounds = _fair("poly")
    d0 = c["system"]["diam"]
    ref = sr.swap_round(fr, d0, c["seed"], 0, c["fraction"], c["ktemp"], max_diff=0.05)
    with _device(c, "tiled", monkeypatch) as d:
        d.swap_setup(c["fraction"], 0.05, c["seed"])
        res = d.swap_rounds(1, c["ktemp"])
        partner, status, du = d.swap_last()
        assert np.array_equal(partner, rounds[0]["partner"]) and np.array_equal(status, ref["status"])
        for code in (sr.NONE, sr.VOID, sr.LOST, sr.BLOCKED):
            assert np.array_equal(status == code, rounds[0]["status"] == code)
        assert res["filtered"] == int((status == sr.FILTERED).sum()) >= 1
        acc = np.flatnonzero(status == sr.ACCEPTED)
        assert len(acc) >= 1 and np.all(np.abs(d0[acc] - d0[partner[acc]]) <= 0.05)
        assert np.array_equal(d.diameters(), ref["diam"])


def test_run_simulation_with_swaps(tmp_path):
    import moleculardynamics.jl_amd as md
    c, _, _ = reference("poly")
    s = c["system"]
    params = md.Parameters(1.0, s["n"], 0.005, md.Polydisperse(1.25, 0.2))
    state = md.initialize_state(params, None, dimension=2, cutoff=c["cutoff"], unitcell=s["box"], positions=s["x"],
                                diameters=s["diam"], rng=np.random.default_rng(4))
    state.velocities = s["v"].copy()
    swap = md.SwapMonteCarlo(25, 4, fraction=0.02)
    out = str(tmp_path)
    md.run_simulation(state, params, md.NVT(c["ktemp"], 0.1), 300, 100, out, swap=swap)
    dev = state.system.device
    try:
        rows = np.loadtxt(os.path.join(out, "swap.txt"), ndmin=2)
        assert rows.shape == (12, 8) and list(rows[:, 0]) == list(range(24, 300, 25))
        assert swap.rounds_done == 48 and rows[:, 4].sum() >= 10 and np.all(rows[:, 3] >= rows[:, 4])
        assert np.array_equal(state.diameters, dev.diameters())
        assert np.array_equal(np.sort(state.diameters), np.sort(s["diam"])) and not np.array_equal(state.diameters, s["diam"])
        _, _, final = md.io.read_file(os.path.join(out, "final.xyz"), dimension=2)
        assert np.abs(final - state.diameters).max() <= 1.01e-6         # radius printed with six decimals
        assert np.abs(final - s["diam"]).max() > 0.01
    finally:
        dev.close()


def test_refusals(monkeypatch):
    from moleculardynamics.jl_amd import MDDevice, MdhipError
    c, _, _ = reference("poly")
    s = c["system"]
    with _device(c, "tiled", monkeypatch) as d:
        with pytest.raises(MdhipError, match="md_swap_setup first"):
            d.swap_rounds(1, 0.1)
        with pytest.raises(MdhipError, match="md_swap_setup first"):
            d.swap_last()
        for bad in (0.0, -0.1, 1.5, float("nan")):
            with pytest.raises(MdhipError, match="fraction"):
                d.swap_setup(bad)
        d.swap_setup(1.0)                                              # the closed end
        d.swap_setup(c["fraction"], None, 1)
        with pytest.raises(MdhipError, match="no round"):
            d.swap_last()
        for bad in (0.0, -1.0, float("nan")):
            with pytest.raises(MdhipError, match="ktemp"):
                d.swap_rounds(1, bad)
        d.upload(diameters=np.full(s["n"], 0.9))
        with pytest.raises(MdhipError, match="diameters are equal"):
            d.swap_rounds(1, 0.1)
        d.upload(diameters=s["diam"])
        src = ("__device__ void soft(double r, double s1, double s2, const double* p, double* u, double* f)"
               "{ double s = 0.5 * (s1 + s2); double t = 1.0 - r / s; *u = r < s ? t * t : 0.0; *f = r < s ? 2.0 * t / s : 0.0; }")
        d.set_potential_source(src, "soft")
        with pytest.raises(MdhipError, match="run-time compiled potential"):
            d.swap_rounds(1, 0.1)
        d.set_potential(c["kind"], c["params"])
        assert d.swap_rounds(1, c["ktemp"])["proposed"] >= 1           # and the handle is still good


def test_slab_handles_are_refused():
    import ctypes as C
    from moleculardynamics.jl_amd.domain import DomainDevice
    from tests.util import lj_system

    class TwoRanks:
        rank, world = 0, 2

    s = lj_system(4096)
    with DomainDevice(3, s["n"], s["box"], 2.5, TwoRanks()) as dom:
        assert dom._L.md_swap_setup(dom._h, 0.01, 0.0, C.c_uint64(1)) != 0
        assert "md_swap_setup: not available on a slab-decomposition handle" in dom._L.md_last_error(dom._h).decode()
        assert dom._L.md_swap_rounds(dom._h, 1, 1.0, 0, None, None, None, None, None) != 0
        assert "md_swap_rounds: not available on a slab-decomposition handle" in dom._L.md_last_error(dom._h).decode()
