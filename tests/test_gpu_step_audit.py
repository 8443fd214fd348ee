"""-m gpu: the step audit (tests/step_audit.py) on an MDDevice -- every step-loop kernel, one short segment at a time, on
the ragged, tiny and mixed systems, through every path switch.

Measured margins (MI355X; records, not tolerances): the worst error of each quantity as a fraction of its bound.  F, U,
W, K: check (A) (1e-11 max(1, |F|inf), pseudo hard spheres 1e-10; 1e-12 relative, pseudo hard spheres 1e-10); one step: the
derived bounds 8 spacing(L) and 0.5 dt tol_F + 4 spacing(|v|inf); <= 10 steps: 1e-10 (general cell: its one-step segments
too); last column: particles the knife-edge precondition left out.  No case missed a bound, so none had to be
reported as loose; the one-step x error is one or two spacings of L throughout.

  case                              (A)                                 | one step        | <= 10 steps         | excl
  blob                              F 0.001  U 0.009  W 0.009  K 0.002 | x 0.250  v 0.010 | x 3.55e-04  v 2.15e-03 | 0
  tiny2                             F 0.001  U 0.001  W 0.003  K 0.000 | x 0.250  v 0.004 | x 4.44e-05  v 1.33e-05 | 0
  tiny3                             F 0.003  U 0.007  W 0.011  K 0.000 | x 0.125  v 0.006 | x 5.33e-05  v 5.11e-05 | 0
  tiny65                            F 0.001  U 0.001  W 0.020  K 0.000 | x 0.125  v 0.006 | x 7.11e-05  v 6.71e-04 | 0
  tiny257                           F 0.001  U 0.005  W 0.006  K 0.001 | x 0.125  v 0.004 | x 9.77e-05  v 9.02e-04 | 0
  lj_diam                           F 0.001  U 0.009  W 0.010  K 0.002 | x 0.250  v 0.005 | x 1.07e-04  v 2.87e-03 | 0
  lj_095                            F 0.002  U 0.004  W 0.009  K 0.003 | x 0.250  v 0.007 | x 1.24e-04  v 2.45e-03 | 0
  ljmod0                            F 0.001  U 0.007  W 0.009  K 0.002 | x 0.250  v 0.005 | x 1.07e-04  v 3.59e-03 | 0
  ljmod1                            F 0.001  U 0.009  W 0.008  K 0.002 | x 0.250  v 0.006 | x 1.07e-04  v 2.80e-03 | 0
  ljmod2                            F 0.001  U 0.011  W 0.003  K 0.002 | x 0.250  v 0.004 | x 1.24e-04  v 2.55e-03 | 0
  lj_2d                             F 0.005  U 0.004  W 0.013  K 0.002 | x 0.125  v 0.014 | x 2.84e-04  v 6.39e-03 | 0
  phs                               F 0.000  U 0.000  W 0.000  K 0.001 | x 0.125  v 0.001 | x 8.88e-05  v 4.97e-03 | 0
  phs_diam                          F 0.000  U 0.000  W 0.000  K 0.001 | x 0.125  v 0.001 | x 8.88e-05  v 6.84e-03 | 0
  poly_2d                           F 0.005  U 0.003  W 0.003  K 0.003 | x 0.250  v 0.013 | x 4.26e-04  v 5.27e-03 | 0
  poly_3d                           F 0.001  U 0.002  W 0.002  K 0.001 | x 0.250  v 0.006 | x 1.42e-04  v 1.02e-03 | 0
  blob_sheared                      F 0.001  U 0.009  W 0.009  K 0.001 | x 0.000  v 0.000 | x 3.20e-04  v 1.71e-03 | 0
  blob/ones                         F 0.002  U 0.007  W 0.185  K 0.001 | x 0.250  v 0.014 | x 0.00e+00  v 0.00e+00 | 0
  lj_diam/ones                      F 0.002  U 0.012  W 0.010  K 0.002 | x 0.250  v 0.006 | x 0.00e+00  v 0.00e+00 | 2
  blob/no_fused_step                F 0.001  U 0.008  W 0.011  K 0.002 | x 0.125  v 0.006 | x 3.55e-04  v 1.06e-03 | 0
  blob/no_fused_step_inner_halo     F 0.001  U 0.008  W 0.011  K 0.002 | x 0.125  v 0.006 | x 3.55e-04  v 1.06e-03 | 0
  blob/no_tiles                     F 0.001  U 0.008  W 0.012  K 0.001 | x 0.125  v 0.006 | x 3.55e-04  v 1.03e-03 | 0
  blob/no_fused_build               F 0.001  U 0.009  W 0.009  K 0.002 | x 0.250  v 0.010 | x 3.55e-04  v 2.15e-03 | 0
  blob/inner_skin_0                 F 0.001  U 0.009  W 0.009  K 0.001 | x 0.250  v 0.010 | x 3.55e-04  v 1.74e-03 | 0
  blob/skin_0                       F 0.001  U 0.008  W 0.011  K 0.001 | x 0.125  v 0.006 | x 3.55e-04  v 9.95e-04 | 0
  lj_diam/no_fused_step             F 0.001  U 0.008  W 0.010  K 0.002 | x 0.125  v 0.003 | x 7.99e-05  v 1.75e-03 | 0
  lj_diam/no_fused_step_inner_halo  F 0.001  U 0.008  W 0.010  K 0.002 | x 0.125  v 0.003 | x 7.99e-05  v 1.75e-03 | 0
  lj_diam/no_tiles                  F 0.001  U 0.008  W 0.010  K 0.002 | x 0.125  v 0.003 | x 7.99e-05  v 1.75e-03 | 0
  lj_diam/no_fused_build            F 0.001  U 0.009  W 0.010  K 0.002 | x 0.250  v 0.005 | x 1.07e-04  v 2.87e-03 | 0
  lj_diam/inner_skin_0              F 0.001  U 0.009  W 0.011  K 0.002 | x 0.250  v 0.005 | x 1.07e-04  v 2.87e-03 | 0
  lj_diam/skin_0                    F 0.001  U 0.008  W 0.010  K 0.002 | x 0.125  v 0.003 | x 7.99e-05  v 2.08e-03 | 0
  blob/nvt                          F 0.001  U 0.007  W 0.009  K 0.001 | x 0.250  v 0.001 | x 2.49e-04  v 2.17e-03 | 0
  poly_2d/nvt                       F 0.007  U 0.002  W 0.002  K 0.001 | x 0.250  v 0.006 | x 4.97e-04  v 3.04e-03 | 0

lj_diam/ones leaves out one pair (particles 897, 978) at step 13: d2 - r_c^2 = 2.8e-9, 4.4e-10 relative -- inside the 1e-9
window by chance, far from a real knife edge (the oracle's own trajectory has the same pair), and at the cap of two.

(The mixed schedule was specified as the tuple below "90 steps in total"; the tuple, used unchanged, totals 79.)
"""
import numpy as np
import pytest

from tests import step_audit as sa
from tests.util import blob_gas_system, lj_system, poly_system, sheared, tiny_system, with_diameters

pytestmark = pytest.mark.gpu

MIXED, ONES = sa.MIXED, sa.ONES      # 79 steps in 20 segments; 60 one-step calls
LJ = [1.0, 1.0, 2.5]


def build_case(name):
    """dict(system, kind, params, cutoff, dt[, skin, inner_skin]) of a named case.

    skin / inner_skin (default 0.6 / 0.16, tuned for the liquid's largest displacement per step |v|inf dt = 0.022): the slow
    pseudo-hard-sphere and 3-D polydisperse cases get smaller ones in proportion, so that their lists turn over within the
    schedule.  Which steps are prune steps is the planner's decision; with the default inner skin some cases put none, or
    none of one thermo kind, on the schedule's eleven one-step segments -- the only ones whose kind is known exactly.  Those
    cases (the tiny systems, lj_095, poly_2d, phs_diam) run with a smaller inner skin, and the two smallest at kT = 16
    instead of 1 (at kT = 1 a dimer's list is built twice in 79 steps), which makes every second or third step a prune
    step.  A change to the planner in md_run may move the prune steps off the audited ones again: the coverage
    assertions then say so, and the remedy is another skin or temperature here, never a dropped assertion."""
    if name == "blob":
        return dict(system=blob_gas_system(), kind=sa.POT_LJ, params=LJ, cutoff=2.5, dt=0.004)
    if name == "blob_sheared":
        # (the gas grid has spacing 2: a tilt of 6 keeps its images on the grid; faces 23.3 apart >= 3 list radii)
        return dict(system=sheared(blob_gas_system(), 6.0), kind=sa.POT_LJ, params=LJ, cutoff=2.5, dt=0.004)
    if name.startswith("tiny"):
        n = int(name[4:])
        # (skin: the 9^3 box clips the default 0.6 to 0.4995)
        return dict(system=tiny_system(n, kT=16.0 if n <= 3 else 1.0), kind=sa.POT_LJ, params=LJ, cutoff=2.5, dt=0.004,
                    inner_skin=0.08 if n <= 3 else 0.06)
    if name == "lj_diam":          # 32-byte LDS records, the ds_read_b128 path
        return dict(system=with_diameters(lj_system(1000, kT=2.0), 0.9, 1.1), kind=sa.POT_LJ, params=LJ, cutoff=2.5,
                    dt=0.004)
    if name == "lj_095":           # one diameter != 1: the sigma-folded ljA / ljB
        return dict(system=with_diameters(lj_system(1000, kT=2.0), 0.95), kind=sa.POT_LJ, params=LJ, cutoff=2.5, dt=0.004,
                    inner_skin=0.10)
    if name.startswith("ljmod"):
        mode = int(name[5:])
        return dict(system=with_diameters(lj_system(1000, kT=2.0), 0.9, 1.1), kind=sa.POT_LJ_MODIFIED,
                    params=[1.0, 1.0, 2.5, float(mode), 2.0 if mode == 2 else 0.0], cutoff=2.5, dt=0.004)
    if name == "lj_2d":
        return dict(system=lj_system(900, rho=0.8, dim=2, kT=2.0), kind=sa.POT_LJ, params=LJ, cutoff=2.5, dt=0.004)
    if name in ("phs", "phs_diam"):
        s = lj_system(500, rho=0.5, kT=1.4737)
        if name == "phs_diam":
            s = with_diameters(s, 0.9, 1.05)
        return dict(system=s, kind=sa.POT_PSEUDOHS, params=[50.0], cutoff=1.5, dt=0.001, skin=0.12,
                    inner_skin=0.025 if name == "phs_diam" else 0.03)
    if name == "poly_2d":
        return dict(system=poly_system(), kind=sa.POT_POLYDISPERSE, params=[1.25, 0.2], cutoff=1.25 * 1.2, dt=0.005,
                    inner_skin=0.08)
    if name == "poly_3d":
        return dict(system=with_diameters(lj_system(1000, rho=0.9, kT=0.5), 0.75, 1.1), kind=sa.POT_POLYDISPERSE,
                    params=[1.25, 0.2], cutoff=1.5, dt=0.004, skin=0.3, inner_skin=0.08)
    raise KeyError(name)


DEFAULT_CASES = ["blob", "tiny2", "tiny3", "tiny65", "tiny257", "lj_diam", "lj_095", "ljmod0", "ljmod1", "ljmod2", "lj_2d",
                 "phs", "phs_diam", "poly_2d", "poly_3d", "blob_sheared"]
SWITCHES = {
    "no_fused_step": dict(env={"MDHIP_NO_FUSED_STEP": "1"}),
    "no_fused_step_inner_halo": dict(env={"MDHIP_NO_FUSED_STEP": "1", "MDHIP_INNER_HALO": "1"}),
    "no_tiles": dict(env={"MDHIP_NO_TILES": "1"}),
    "no_fused_build": dict(env={"MDHIP_NO_FUSED_BUILD": "1"}),
    "inner_skin_0": dict(inner_skin=0.0),
    "skin_0": dict(skin=0.0),
}


def run_case(oracle, name, schedule, skin=None, inner_skin=None, nvt=False, raise_on_failure=True):
    """audit_run of a named case on a fresh MDDevice (environment switches are read when the handle is created: the caller
    sets them first)."""
    from moleculardynamics.jl_amd import MDDevice
    from moleculardynamics.jl_amd.thermostat import draw_bussi
    c = build_case(name)
    s = c["system"]
    cell = s.get("cell")
    skin = c.get("skin") if skin is None else skin
    inner_skin = c.get("inner_skin") if inner_skin is None else inner_skin
    kw = {}
    if nvt:
        total = sum(schedule)
        nf = s["dim"] * (s["n"] - 1.0)
        r1, r2 = draw_bussi(nf, np.random.default_rng(17), total)
        kT = 2.0 * float(oracle.kinetic(s["v"])) / nf
        kw = dict(ensemble=sa.NVT, tau=0.1, ktemp=np.full(total, kT), r1=r1, r2=r2)
    with MDDevice(s["dim"], s["n"], s["box"] if cell is None else cell, c["cutoff"]) as dev:
        dev.set_potential(c["kind"], c["params"])
        if skin is not None:
            dev.set_skin(skin)
        if inner_skin is not None:
            dev.set_inner_skin(inner_skin)
        return sa.audit_run(dev, oracle, s, oracle.make_pot(c["kind"], c["params"]), c["cutoff"], c["dt"], schedule,
                            cell=cell, raise_on_failure=raise_on_failure, **kw)


def _report(name, res):
    print(sa.margins_line(name, res))
    print("    kinds %s  stats %s" % (sorted(sa.coverage(res).items()),
                                      {k: res["stats"][k] for k in ("fused", "prunes", "rebuilds", "violations")}))


def _check_default_coverage(res):
    """Without these a pass means little: the fused loop ran, its lists turned over, and the audited last steps include
    prune steps and ordinary inner-row steps of both thermo kinds, and the first step after a list build."""
    st, cov = res["stats"], sa.coverage(res)
    assert st["fused"] == 1 and st["prunes"] >= 3 and st["rebuilds"] >= 2, st
    for thermo in (True, False):
        assert cov.get(("prune", thermo), 0) >= 1, ("no audited prune step with thermo=%s" % thermo, cov)
        assert cov.get(("ordinary", thermo), 0) >= 1, ("no audited ordinary step with thermo=%s" % thermo, cov)
    assert sum(v for (kind, _), v in cov.items() if kind == "after_rebuild") >= 1, cov


@pytest.mark.parametrize("name", DEFAULT_CASES)
def test_default_path_mixed_schedule(oracle, name):
    res = run_case(oracle, name, MIXED)
    _report(name, res)
    assert len(res["excluded"]) <= sa.MAX_EXCLUDED
    _check_default_coverage(res)


@pytest.mark.parametrize("name", ["blob", "lj_diam"])
def test_one_step_calls_rebuild_through_the_violation_branch(oracle, name):
    """60 calls of one step: no scheduled build can fire, every list build is the redo of a violated step."""
    res = run_case(oracle, name, ONES)
    _report(name + "/ones", res)
    assert len(res["excluded"]) <= sa.MAX_EXCLUDED
    st = res["stats"]
    assert st["violations"] >= 1 and st["rebuilds"] >= 2, st
    assert any(s["kind"] == "after_rebuild" and s["violations"] for s in res["segments"]), sa.coverage(res)


@pytest.mark.parametrize("switch", list(SWITCHES))
@pytest.mark.parametrize("name", ["blob", "lj_diam"])
def test_path_switches_mixed_schedule(oracle, monkeypatch, name, switch):
    sw = SWITCHES[switch]
    for k, v in sw.get("env", {}).items():
        monkeypatch.setenv(k, v)
    res = run_case(oracle, name, MIXED, skin=sw.get("skin"), inner_skin=sw.get("inner_skin"))
    _report(name + "/" + switch, res)
    assert len(res["excluded"]) <= sa.MAX_EXCLUDED
    st = res["stats"]
    assert st["steps"] == sum(MIXED) and st["rebuilds"] >= 2, st
    if "NO_FUSED_STEP" in "".join(sw.get("env", {})) or switch in ("no_tiles", "skin_0"):
        assert st["fused"] == 0, st
    if switch == "skin_0":
        assert st["rebuilds"] >= sum(MIXED), st      # the reference cadence: a list build every step
    if switch == "no_fused_build":
        assert st["fused_build"] == 0, st
    if switch in ("inner_skin_0", "skin_0", "no_tiles"):
        assert st["prunes"] == 0, st                 # no inner rows on these paths
    else:
        assert st["prunes"] >= 3, st


@pytest.mark.parametrize("name,inner_skin", [("blob", None), ("poly_2d", 0.16)])
def test_nvt_mixed_schedule(oracle, name, inner_skin):
    """Bussi thermostat (tau = 0.1, draws from draw_bussi, target = the starting temperature).  (Under the thermostat
    poly_2d puts prune steps of both thermo kinds on the one-step segments with the default inner skin.)"""
    res = run_case(oracle, name, MIXED, nvt=True, inner_skin=inner_skin)
    _report(name + "/nvt", res)
    assert len(res["excluded"]) <= sa.MAX_EXCLUDED
    _check_default_coverage(res)
