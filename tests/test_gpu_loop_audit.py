"""-m gpu: the Brownian and FIRE modes of the step audit (tests/step_audit.py) on an MDDevice -- md_run_brownian and
md_fire_minimize, one short segment at a time, on the ragged, tiny, 2-D, polydisperse, pseudo-hard-sphere, user-potential
and sheared systems of tests/test_gpu_step_audit.py, through the path switches that reach these two loops.

Measured margins (MI355X; records, not tolerances): the worst error of each quantity as a fraction of its bound.
Brownian ("bd"): F U W -- the last evaluation's forces, energy and virial, segments of <= 10 steps; Fl -- forces, > 10
steps; V -- virial sum; x1 -- one step (8 spacing(L) + (dt / kT) tol_F); x -- <= 10 steps and general cell (1e-10); xl --
> 10 steps (1e-9).  FIRE: F U R -- forces, energy and f_rms of the closing evaluation at the held positions; x1 = 8
spacing(L) + dt_initial^2 tol_F; "conv": the three convergence points (energy of the converging evaluation, positions
after j - 1 moves).  No case missed a bound and none left a particle out.  The no_fused_build and inner_skin_0 rows equal
their default rows digit for digit (neither switch reaches these loops' kernels, which walk the outer rows) and are
left out.

  bd blob                F 8.3e-04 U 8.8e-03 W 7.3e-03 Fl 0.0e+00 V 1.4e-02 x1 5.0e-02 x 2.5e-04 xl 0.0e+00 | excl 0 img 0
  bd tiny2               F 2.8e-03 U 6.9e-03 W 1.9e-02 Fl 0.0e+00 V 1.4e-02 x1 3.3e-03 x 3.6e-05 xl 0.0e+00 | excl 0 img 0
  bd tiny3               F 2.8e-03 U 6.9e-03 W 1.9e-02 Fl 0.0e+00 V 1.4e-02 x1 5.0e-02 x 3.6e-05 xl 0.0e+00 | excl 0 img 0
  bd tiny65              F 2.8e-03 U 1.0e-03 W 2.5e-02 Fl 0.0e+00 V 5.2e-02 x1 3.6e-02 x 7.1e-05 xl 0.0e+00 | excl 0 img 0
  bd tiny257             F 1.3e-03 U 2.3e-03 W 4.9e-03 Fl 0.0e+00 V 1.0e-02 x1 3.6e-02 x 8.0e-05 xl 0.0e+00 | excl 0 img 0
  bd lj_diam             F 1.2e-03 U 1.0e-02 W 9.5e-03 Fl 0.0e+00 V 3.0e-03 x1 7.0e-03 x 8.0e-05 xl 0.0e+00 | excl 0 img 0
  bd lj_095              F 1.3e-03 U 6.3e-03 W 1.3e-02 Fl 0.0e+00 V 1.3e-02 x1 1.7e-02 x 8.0e-05 xl 0.0e+00 | excl 0 img 0
  bd ljmod2              F 1.8e-03 U 6.7e-03 W 8.7e-03 Fl 0.0e+00 V 5.6e-03 x1 6.4e-03 x 8.9e-05 xl 0.0e+00 | excl 0 img 0
  bd lj_2d               F 4.2e-03 U 4.3e-03 W 2.3e-02 Fl 0.0e+00 V 2.3e-02 x1 6.3e-02 x 2.5e-04 xl 0.0e+00 | excl 0 img 0
  bd phs                 F 1.7e-03 U 7.5e-05 W 5.0e-05 Fl 0.0e+00 V 7.0e-04 x1 5.5e-02 x 6.2e-05 xl 0.0e+00 | excl 0 img 0
  bd phs_diam            F 1.2e-03 U 7.4e-05 W 1.9e-04 Fl 0.0e+00 V 3.2e-04 x1 5.5e-02 x 6.2e-05 xl 0.0e+00 | excl 0 img 0
  bd poly_2d             F 3.4e-03 U 2.1e-03 W 2.2e-03 Fl 0.0e+00 V 2.0e-03 x1 5.2e-02 x 3.2e-04 xl 0.0e+00 | excl 0 img 0
  bd poly_3d             F 8.2e-04 U 2.4e-03 W 1.6e-03 Fl 0.0e+00 V 1.6e-03 x1 3.5e-02 x 8.9e-05 xl 0.0e+00 | excl 0 img 0
  bd blob_sheared        F 6.9e-04 U 9.3e-03 W 6.4e-03 Fl 0.0e+00 V 1.3e-02 x1 0.0e+00 x 3.2e-04 xl 0.0e+00 | excl 0 img 0
  bd user_lj             F 1.4e-03 U 1.1e-02 W 7.9e-03 Fl 0.0e+00 V 4.9e-03 x1 7.0e-03 x 7.1e-05 xl 0.0e+00 | excl 0 img 0
  bd blob/chunks         F 0.0e+00 U 4.9e-07 W 1.5e-07 Fl 2.3e-05 V 4.1e-02 x1 0.0e+00 x 0.0e+00 xl 8.7e-05 | excl 0 img 0
  bd poly_2d/chunks      F 0.0e+00 U 4.5e-07 W 8.0e-08 Fl 2.5e-05 V 3.6e-03 x1 0.0e+00 x 0.0e+00 xl 1.5e-04 | excl 0 img 0
  bd blob/no_tiles       F 8.3e-04 U 8.8e-03 W 8.0e-03 Fl 0.0e+00 V 1.1e-02 x1 5.0e-02 x 2.5e-04 xl 0.0e+00 | excl 0 img 0
  bd blob/skin_0         F 8.4e-04 U 9.0e-03 W 8.1e-03 Fl 0.0e+00 V 1.2e-02 x1 5.0e-02 x 2.5e-04 xl 0.0e+00 | excl 0 img 0
  bd lj_diam/no_tiles    F 1.2e-03 U 1.0e-02 W 9.5e-03 Fl 0.0e+00 V 3.0e-03 x1 7.0e-03 x 8.0e-05 xl 0.0e+00 | excl 0 img 0
  bd lj_diam/skin_0      F 1.3e-03 U 1.1e-02 W 9.7e-03 Fl 0.0e+00 V 3.6e-03 x1 7.0e-03 x 8.9e-05 xl 0.0e+00 | excl 0 img 0
  fire blob              F 1.8e-03 U 7.8e-03 R 8.5e-04 x1 1.1e-01 x 1.8e-04 xl 5.7e-05 | excl 0 img 0
  fire blob conv         U 2.9e-04 x1 0.0e+00 x 0.0e+00 xl 3.2e-05 | excl 0 img 0
  fire tiny2             F 4.1e-03 U 7.3e-03 R 2.0e-02 x1 4.9e-04 x 1.8e-05 xl 1.8e-06 | excl 0 img 0
  fire tiny2 conv        U 6.9e-03 x1 0.0e+00 x 0.0e+00 xl 5.3e-06 | excl 0 img 0
  fire tiny65            F 3.0e-03 U 1.1e-03 R 3.0e-03 x1 4.4e-02 x 5.3e-05 xl 2.0e-05 | excl 0 img 0
  fire tiny65 conv       U 3.1e-04 x1 0.0e+00 x 3.6e-05 xl 0.0e+00 | excl 0 img 0
  fire lj_diam           F 5.2e-03 U 6.7e-03 R 1.8e-03 x1 3.5e-02 x 8.0e-05 xl 1.8e-05 | excl 0 img 0
  fire lj_diam conv      U 3.7e-03 x1 0.0e+00 x 0.0e+00 xl 8.4e-05 | excl 0 img 0
  fire lj_2d             F 2.6e-02 U 4.4e-03 R 8.0e-03 x1 4.7e-02 x 2.5e-04 xl 7.1e-05 | excl 0 img 0
  fire lj_2d conv        U 1.0e-03 x1 0.0e+00 x 0.0e+00 xl 3.6e-05 | excl 0 img 0
  fire phs               F 4.1e-03 U 3.0e-05 R 1.3e-02 x1 3.7e-03 x 6.2e-05 xl 1.4e-05 | excl 0 img 0
  fire phs conv          U 5.8e-06 x1 0.0e+00 x 0.0e+00 xl 1.2e-05 | excl 0 img 0
  fire poly_2d           F 1.6e-02 U 2.6e-03 R 1.1e-03 x1 1.5e-02 x 3.6e-04 xl 1.1e-04 | excl 0 img 0
  fire poly_2d conv      U 1.2e-03 x1 0.0e+00 x 0.0e+00 xl 9.2e-05 | excl 0 img 0
  fire poly_3d           F 3.1e-03 U 3.5e-03 R 5.2e-04 x1 1.5e-02 x 1.1e-04 xl 2.6e-05 | excl 0 img 0
  fire poly_3d conv      U 1.1e-03 x1 0.0e+00 x 0.0e+00 xl 2.1e-05 | excl 0 img 0
  fire blob_sheared      F 2.1e-03 U 4.8e-03 R 6.2e-04 x1 0.0e+00 x 7.3e-04 xl 0.0e+00 | excl 0 img 0
  fire blob_sheared conv U 1.5e-04 x1 0.0e+00 x 4.6e-04 xl 0.0e+00 | excl 0 img 0
  fire blob/no_tiles     F 1.8e-03 U 7.8e-03 R 8.5e-04 x1 1.1e-01 x 1.8e-04 xl 5.7e-05 | excl 0 img 0
  fire blob/no_tiles conv U 2.9e-04 x1 0.0e+00 x 0.0e+00 xl 3.2e-05 | excl 0 img 0
  fire blob/skin_0       F 1.8e-03 U 7.8e-03 R 6.8e-04 x1 1.1e-01 x 1.8e-04 xl 5.5e-05 | excl 0 img 0
  fire blob/skin_0 conv  U 2.9e-04 x1 0.0e+00 x 0.0e+00 xl 3.2e-05 | excl 0 img 0
  fire lj_diam/no_tiles  F 5.2e-03 U 6.7e-03 R 1.8e-03 x1 3.5e-02 x 8.0e-05 xl 1.8e-05 | excl 0 img 0
  fire lj_diam/no_tiles conv U 3.7e-03 x1 0.0e+00 x 0.0e+00 xl 8.4e-05 | excl 0 img 0
  fire lj_diam/skin_0    F 5.9e-03 U 6.7e-03 R 1.8e-03 x1 3.5e-02 x 7.1e-05 xl 1.5e-05 | excl 0 img 0
  fire lj_diam/skin_0 conv U 3.6e-03 x1 0.0e+00 x 0.0e+00 xl 9.1e-05 | excl 0 img 0

A finding, fixed here: under MDHIP_NO_TILES=1 both loops failed check (A) on the first force evaluation after a move
(Brownian blob, segment 2: |dF|inf = 3.0e-2 against 1.6e-8; lj_diam 1.3e+2; FIRE blob, segment 1: 8.5e-6; lj_diam 3.2e+1).
Without tiles (and with tiles from 2^26 slots on) ghosts are real copies in the position array, which md_run refreshes
after every drift (launch_ghost_update); md_run_brownian and md_fire_minimize moved the owners only, so every pair across
a periodic face was evaluated at the ghost's position of the last list build.  Both loops now refresh the copies after
the move.  The long-trajectory tests never ran these loops without tiles.
"""
import numpy as np
import pytest

from tests import step_audit as sa
from tests.test_gpu_parity import USER_LJ_SRC
from tests.test_gpu_step_audit import SWITCHES, build_case
from tests.util import lj_system

pytestmark = pytest.mark.gpu

SEED = 0xC0FFEE1234ABCDEF
KT = 1.5
HIGH = 2 ** 32 - 3

# Brownian time step and skin per case.  The largest move of a step is sqrt(2 dt) sqrt(3) per component plus the drift
# f dt / kT; a Brownian liquid whose noise is uniform (not Gaussian) still blows up once two particles land on top of
# each other, which limits dt to 4e-4 for the LJ liquids (3e-5 pseudo hard spheres, 1e-4 polydisperse).  At those steps the
# default skin of 0.6 would outlast most segments, so the skin is set where the largest displacement of some particle
# (about twice the rms sqrt(2 d dt m) after m steps) passes skin / 2 within three to five steps: every call starts from a
# list build, so only then do segments of k > 1 see the violation redo and rows aged through several moves.
LJ_BD = dict(dt=4e-4, skin=0.3)
BD = {
    "blob": LJ_BD, "tiny2": LJ_BD, "tiny3": LJ_BD, "tiny65": LJ_BD, "tiny257": LJ_BD, "lj_diam": LJ_BD, "lj_095": LJ_BD,
    "ljmod2": LJ_BD, "lj_2d": LJ_BD, "blob_sheared": LJ_BD, "user_lj": LJ_BD,
    "phs": dict(dt=3e-5, skin=0.12), "phs_diam": dict(dt=3e-5, skin=0.12),
    "poly_2d": dict(dt=1e-4, skin=0.12), "poly_3d": dict(dt=1e-4, skin=0.3),
}
BD_EXTRA = {"tiny65": dict(first_step=HIGH), "poly_3d": dict(virial_every=7)}

# FIRE parameters and skin per case (f_inc, f_dec, alpha0 at the reference's defaults).  nmin = 0 makes every step with
# P > 0 raise dt, so the drift with the NEW dt differs from one with the old dt from the first step on.  dt_max comes
# from grids on which the restatement, run alone on the CPU, stays bounded over the schedule (no particle moves by more
# than 1 in a segment); the skin is small enough for the moves of a segment to violate it.
#
# A reset (P <= 0) within a segment of at most 14 steps, from rest, needs a start close to a minimum: the crystallite of
# the blob, the 2-D lattice (the dimer too, once it has arrived: see tiny2 below).  The 3-D liquids, the polydisperse cases and the dense hard spheres start far
# from one, and from rest their kinetic energy only grows for as long as a stable run lasts: on grids of dt_initial
# (0.002 .. 0.04), dt_max (up to 0.14) and nmin (0 .. 5) -- and with alpha0 = 0 over 60 steps -- the CPU restatement
# takes a reset only once dt has passed the stability limit, where particles are thrown across the box, forces reach
# 1e8 and no trajectory bound means anything.  RESET_WITHIN_14 lists the cases that do take one; the others assert
# that their shadow takes none (should that change, the case belongs in the list), and the acceleration.
#
# tiny2 runs gently on purpose.  With dt_max = 0.04 the dimer reaches its minimum within the schedule (and resets there),
# f_rms falls to 2e-3 and then 2e-10, and f_rms "to 1e-12 relative" asks for the cancelling pair force to 1e-12 of what is
# left of it: the device missed it at f_rms = 2.3e-3 by 1.4e-11 relative, which is one rounding of the download wrap
# (spacing(9) = 1.8e-15) through the pair's stiffness (57): 1e-13 absolute, inside the force tolerance.  At dt_max =
# 0.0015 the 85 steps take the dimer a third of the way and f_rms stays above 1.
LJ_FIRE = dict(dt_initial=0.01, dt_max=0.03, nmin=0)
FIRE = {
    "blob": dict(kw=dict(dt_initial=0.005, dt_max=0.03, nmin=0), skin=0.3),
    "blob_sheared": dict(kw=dict(dt_initial=0.005, dt_max=0.03, nmin=0), skin=0.3),
    "tiny2": dict(kw=dict(dt_initial=0.001, dt_max=0.0015, nmin=0), skin=0.004),
    "tiny65": dict(kw=dict(dt_initial=0.01, dt_max=0.04, nmin=0), skin=0.3),
    "lj_diam": dict(kw=LJ_FIRE, skin=0.3),
    "lj_2d": dict(kw=dict(dt_initial=0.01, dt_max=0.05, nmin=0), skin=0.3),
    "phs": dict(kw=dict(dt_initial=4e-4, dt_max=2e-3, nmin=0), skin=0.03),
    "poly_2d": dict(kw=dict(dt_initial=0.02, dt_max=0.03, nmin=0), skin=0.3),
    "poly_3d": dict(kw=dict(dt_initial=0.02, dt_max=0.03, nmin=0), skin=0.3),
}
RESET_WITHIN_14 = ("blob", "blob_sheared", "lj_2d")


def _case(name):
    """build_case, plus "user_lj": lj_diam's system under the run-time compiled potential of
    tests/test_gpu_parity.py::test_user_potential_source (the oracle's Lennard-Jones)."""
    c = build_case("lj_diam" if name == "user_lj" else name)
    c["user"] = name == "user_lj"
    return c


def _device(c, skin, inner_skin=None):
    from moleculardynamics.jl_amd import MDDevice
    s = c["system"]
    cell = s.get("cell")
    dev = MDDevice(s["dim"], s["n"], s["box"] if cell is None else cell, c["cutoff"])
    if c["user"]:
        dev.set_potential_source(USER_LJ_SRC, "user_lj", [1.0, 2.5])
    else:
        dev.set_potential(c["kind"], c["params"])
    dev.set_skin(skin)
    if inner_skin is not None:
        dev.set_inner_skin(inner_skin)
    return dev


def run_brownian_case(oracle, name, schedule, skin=None, inner_skin=None):
    c = _case(name)
    s = c["system"]
    with _device(c, BD[name]["skin"] if skin is None else skin, inner_skin) as dev:
        return sa.audit_brownian(dev, oracle, s, oracle.make_pot(c["kind"], c["params"]), c["cutoff"], BD[name]["dt"], KT,
                                 SEED, schedule, cell=s.get("cell"), **BD_EXTRA.get(name, {}))


def _report(name, res):
    print()
    print(sa.loop_margins_line(name, res))
    print("    stats %s  segments with a violation %s" % (
        {k: res["stats"][k] for k in ("rebuilds", "violations")}, [g["k"] for g in res["segments"] if g["violations"]]))


def _check_caps(res):
    assert len(res["excluded"]) <= sa.MAX_EXCLUDED and len(res["image_exceptions"]) <= sa.MAX_IMAGE_EXCEPTIONS


def _check_brownian_coverage(res):
    """Without these a pass means little: rows aged through several moves and the violation redo exist only inside
    segments of more than one step."""
    assert res["stats"]["violations"] >= 1, res["stats"]
    assert sum(1 for g in res["segments"] if g["k"] > 1 and g["violations"]) >= 2, res["segments"]
    assert sum(1 for g in res["segments"] if g["k"] == 1) >= 1
    assert all(g["rebuilds"] >= 1 for g in res["segments"])          # every call starts from a list build


BD_CASES = ["blob", "tiny2", "tiny3", "tiny65", "tiny257", "lj_diam", "lj_095", "ljmod2", "lj_2d", "phs", "phs_diam",
            "poly_2d", "poly_3d", "blob_sheared", "user_lj"]


@pytest.mark.parametrize("name", BD_CASES)
def test_brownian_mixed_schedule(oracle, name):
    res = run_brownian_case(oracle, name, sa.BD_MIXED)
    _report("bd " + name, res)
    _check_caps(res)
    _check_brownian_coverage(res)
    assert res["stats"]["steps"] == sum(sa.BD_MIXED)


@pytest.mark.parametrize("name", ["blob", "poly_2d"])
def test_brownian_across_the_host_chunk(oracle, name):
    """31, 32, 33, 64 and 65 steps per call: the 32-step host chunk with and without a remainder, each with violation
    redos inside it."""
    res = run_brownian_case(oracle, name, sa.BD_CHUNKS)
    _report("bd " + name + "/chunks", res)
    _check_caps(res)
    assert all(g["violations"] >= 1 for g in res["segments"]), res["segments"]


@pytest.mark.parametrize("switch", ["no_tiles", "no_fused_build", "skin_0", "inner_skin_0"])
@pytest.mark.parametrize("name", ["blob", "lj_diam"])
def test_brownian_path_switches(oracle, monkeypatch, name, switch):
    sw = SWITCHES[switch]
    for k, v in sw.get("env", {}).items():
        monkeypatch.setenv(k, v)
    res = run_brownian_case(oracle, name, sa.BD_MIXED, skin=sw.get("skin"), inner_skin=sw.get("inner_skin"))
    _report("bd " + name + "/" + switch, res)
    _check_caps(res)
    st = res["stats"]
    if switch == "skin_0":
        assert st["rebuilds"] >= sum(sa.BD_MIXED), st         # the reference cadence: a list build every step
    else:
        _check_brownian_coverage(res)
    if switch == "no_fused_build":
        assert st["fused_build"] == 0, st


def fire_start(name):
    """The case's system; for phs the same lattice at rho = 0.95 instead of 0.5.  At 0.5 no pair is inside the potential's
    range (U = 0, F = 0: nothing to minimise, and f_rms = 0 meets any tolerance); at 0.95 the jittered lattice (spacing
    1.036 against the potential's cutoff 1.0204) holds overlapping pairs that 85 steps do not resolve."""
    c = _case(name)
    if name == "phs":
        c["system"] = lj_system(500, rho=0.95, kT=1.4737)
    return c


def run_fire_case(oracle, name, skin=None, inner_skin=None):
    c = fire_start(name)
    s = c["system"]
    pot = oracle.make_pot(c["kind"], c["params"])
    fire_kw = dict(FIRE[name]["kw"])
    with _device(c, FIRE[name]["skin"] if skin is None else skin, inner_skin) as dev:
        res = sa.audit_fire(dev, oracle, s, pot, c["cutoff"], fire_kw, sa.FIRE_MIXED, cell=s.get("cell"))
        conv = sa.audit_fire_convergence(dev, oracle, s, pot, c["cutoff"], fire_kw, cell=s.get("cell"))
    return res, conv


def _report_fire(name, res, conv):
    print()
    print(sa.loop_margins_line(name, res))
    print(sa.loop_margins_line(name + " conv", conv))
    print("    stats %s  branches %s  converged at %s" % (
        {k: res["stats"][k] for k in ("rebuilds", "violations")},
        [(g["k"], "".join(sorted({b[0] for b in g["branches"]}))) for g in res["segments"]],
        [(g["j"], g["violations"]) for g in conv["segments"]]))


def _check_fire(name, res, conv, want_violation=True):
    _check_caps(res)
    _check_caps(conv)
    reset = any("reset" in g["branches"] for g in res["segments"] if g["k"] <= 14)
    assert reset == (name in RESET_WITHIN_14), "reset in a segment of <= 14 steps: %s" % reset
    assert any("accelerate" in g["branches"] for g in res["segments"]), "no dt increase"
    if want_violation:
        assert res["stats"]["violations"] >= 1, res["stats"]
    js = [g["j"] for g in conv["segments"]]
    assert js[0] == 1 and 2 <= js[1] < 32 and js[2] >= 2, js
    assert all(g["converged"] and g["steps"] == g["j"] for g in conv["segments"])


FIRE_CASES = ["blob", "tiny2", "tiny65", "lj_diam", "lj_2d", "phs", "poly_2d", "poly_3d", "blob_sheared"]


@pytest.mark.parametrize("name", FIRE_CASES)
def test_fire_mixed_schedule_and_convergence(oracle, name):
    res, conv = run_fire_case(oracle, name)
    _report_fire("fire " + name, res, conv)
    _check_fire(name, res, conv)


@pytest.mark.parametrize("switch", ["no_tiles", "no_fused_build", "skin_0", "inner_skin_0"])
@pytest.mark.parametrize("name", ["blob", "lj_diam"])
def test_fire_path_switches(oracle, monkeypatch, name, switch):
    sw = SWITCHES[switch]
    for k, v in sw.get("env", {}).items():
        monkeypatch.setenv(k, v)
    res, conv = run_fire_case(oracle, name, skin=sw.get("skin"), inner_skin=sw.get("inner_skin"))
    _report_fire("fire " + name + "/" + switch, res, conv)
    _check_fire(name, res, conv, want_violation=switch != "skin_0")
    st = res["stats"]
    if switch == "skin_0":
        # a list build before every force evaluation: one per step, and one for each call's closing evaluation
        assert st["rebuilds"] >= sum(sa.FIRE_MIXED), st
    if switch == "no_fused_build":
        assert st["fused_build"] == 0, st


def test_both_loops_refuse_a_slab_handle():
    import ctypes as C
    from moleculardynamics.jl_amd.domain import DomainDevice
    from tests.util import lj_system

    class TwoRanks:
        rank, world = 0, 2

    s = lj_system(4096)
    with DomainDevice(3, s["n"], s["box"], 2.5, TwoRanks()) as dom:
        dom.set_potential(0, [1.0, 1.0, 2.5])
        dom.upload_global(s["x"], s["v"], s["f"], s["img"], s["diam"])
        out = (C.c_double * 4)()
        assert dom._L.md_run_brownian(dom._h, 1, 1e-4, 1.0, 1, 0, 10, out) != 0
        assert "md_run_brownian: not available on a slab-decomposition handle" in \
            dom._L.md_last_error(dom._h).decode()
        st, cv, en, fr = C.c_int64(), C.c_int(), C.c_double(), C.c_double()
        assert dom._L.md_fire_minimize(dom._h, 1, 1e-6, 0.001, 0.01, 0.1, 1.2, 0.2, 5, C.byref(st), C.byref(cv),
                                       C.byref(en), C.byref(fr)) != 0
        assert "md_fire_minimize: not available on a slab-decomposition handle" in \
            dom._L.md_last_error(dom._h).decode()
