"""CPU: the stochastic cell rescaling barostat without a device -- the scale factor against longdouble, the drift / noise
relation on a scalar model whose stationary law is known, the Verlet rows under a scale on the numpy row model of
tests/test_row_audit.py, the order of run_simulation's device calls on a fake handle, and the plumbing of md_scale_cell.

The scalar model.  P_int = N kT / V has the free energy F = -N kT ln V, so the target exp(-(F + P0 V) / kT) is
Gamma(N + 1, kT / P0) in V, mean (N + 1) kT / P0 = 11 for N = 10, kT = P0 = 1.  The update is the Ito form in eps = ln V; the
V-form's kT / V term, added to it with either sign, moves the mean by one unit of kT / P0 (to 12 or 10): twelve standard
errors at the run length used here, so the 4-sigma assertion tells the two forms apart."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import moleculardynamics.jl_amd as md
from moleculardynamics.jl_amd import _lib, barostat
from tests import baro_reference as br
from tests import row_audit as ra
from tests.test_row_audit import MODEL_SYSTEMS, _model
from tests.test_sampler_protocol import N, DIM, _FakeDevice, _fake_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------------
# 1. crescale_factor
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_known_answers_of_crescale_factor(dim):
    f = md.crescale_factor
    assert f(1.3, 250.0, 0.8, 1.3, 0.05, 2.0, 0.02, 0.0, dim) == 1.0            # no drift, no noise: exactly 1
    assert f(2.0, 250.0, 0.8, 1.3, 0.05, 2.0, 0.02, 0.0, dim) > 1.0             # P_int > P0: the cell grows
    assert f(0.5, 250.0, 0.8, 1.3, 0.05, 2.0, 0.02, 0.0, dim) < 1.0             # P_int < P0: it shrinks
    assert f(1.3, 250.0, 0.8, 1.3, 0.05, 2.0, 0.02, 1.0, dim) > 1.0 > f(1.3, 250.0, 0.8, 1.3, 0.05, 2.0, 0.02, -1.0, dim)
    rng = np.random.default_rng(7)
    worst = 0.0
    for _ in range(200):
        a = (rng.uniform(-2, 8), rng.uniform(50, 5e4), rng.uniform(0.1, 2), rng.uniform(-1, 6), rng.uniform(0.01, 0.5),
             rng.uniform(0.1, 5), rng.uniform(0.001, 0.1), rng.standard_normal(), dim)
        worst = max(worst, br.ulps(f(*a), br.crescale_factor_ld(*a)))
    print("crescale_factor against longdouble, d = %d: at most %.2f ulp" % (dim, worst))
    assert worst <= 4.0
    # the closed form, spelled out once: d eps = -(beta / tau)(P0 - P) dt + sqrt(2 kT beta dt / (V tau)) xi
    deps = -(0.05 / 2.0) * (1.3 - 2.0) * 0.02 + np.sqrt(2 * 0.8 * 0.05 * 0.02 / (250.0 * 2.0)) * 0.7
    assert abs(f(2.0, 250.0, 0.8, 1.3, 0.05, 2.0, 0.02, 0.7, dim) - np.exp(deps / dim)) <= 4 * br.EPS


def test_constructor_refusals():
    for bad in (dict(pressure=float("nan")), dict(tau_p=0.0), dict(compressibility=-1.0), dict(every=0), dict(ktemp=0.0)):
        kw = dict(pressure=1.0, tau_p=1.0, compressibility=0.1)
        kw.update(bad)
        with pytest.raises(ValueError):
            md.StochasticCellRescaling(**kw)


# ---------------------------------------------------------------------------------------------------------------------
# 2. drift and noise belong together
# ---------------------------------------------------------------------------------------------------------------------
_RUNS = {}


def _scalar_run(v_form):
    if v_form not in _RUNS:
        v = br.scalar_model(10, 1.0, 1.0, 0.01, 400_000, np.random.default_rng(1), v_form=v_form)
        _RUNS[v_form] = br.block_mean_and_error(v[20_000:], 38)
    return _RUNS[v_form]


def test_the_scalar_model_samples_its_gamma_law():
    mean, err = _scalar_run(0.0)
    print("<V> = %.4f +- %.4f (target 11)" % (mean, err))
    assert 0.04 < err < 0.16                                 # (measured 0.08: the assertion below means what it says)
    assert abs(mean - 11.0) <= 4.0 * err


@pytest.mark.parametrize("v_form", [1.0, -1.0])
def test_the_v_form_term_in_the_eps_update_is_caught(v_form):
    mean, err = _scalar_run(v_form)
    print("with %+.0f kT / V in the drift of eps: <V> = %.4f +- %.4f" % (v_form, mean, err))
    assert abs(mean - 11.0) > 4.0 * err
    assert abs(mean - (11.0 + v_form)) <= 4.0 * err


# ---------------------------------------------------------------------------------------------------------------------
# 3. the rows under a scale
# ---------------------------------------------------------------------------------------------------------------------
def _checks(res):
    return {v.check for v in res["violations"]}


@pytest.mark.parametrize("mu", [0.998, 1.002])
@pytest.mark.parametrize("with_inner", [True, False])
@pytest.mark.parametrize("name", MODEL_SYSTEMS)
def test_scaled_rows_pass_the_audit_with_the_effective_figures(name, with_inner, mu):
    snap, U, dim, cell, _ = _model(name, with_inner)
    scaled, U2 = br.scale_snapshot(snap, U, mu)
    res = ra.check_rows(scaled, U2, dim)
    print(ra.counts_line("%s/scaled by %g" % (name, mu), res["counts"]))
    assert res["violations"] == [], res["violations"]
    info = scaled["info"]
    rl, skin, inner = br.effective(info["rc"], snap["info"]["skin"], snap["info"]["inner_skin"], np.float64(mu), np.float64(mu))
    assert (info["rl"], info["skin"]) == (rl, skin) and (not with_inner or info["inner_skin"] == inner)
    assert (info["skin"] < snap["info"]["skin"]) == (mu < 1.0)


# what each mistake must be reported as (among whatever else it breaks): rows about an x0 that did not move are wider
# than the radius reported for them; an x1 that did not move is farther from the scaled positions than the inner limit;
# the old radius after a compression claims pairs the rows never held; an unscaled d1 after an expansion under-reports
# the distance between the two reference frames; the old inner skin after a compression claims inner entries never kept
SABOTAGES = [("x0_unscaled", 0.998, "O4"), ("x1_unscaled", 0.998, "V2"), ("old_radius", 0.998, "O1"),
             ("d1_unscaled", 1.002, "V2"), ("inner_limit_kept", 0.998, "I3")]


@pytest.mark.parametrize("variant,mu,expected", SABOTAGES)
@pytest.mark.parametrize("name", MODEL_SYSTEMS)
def test_every_scaling_mistake_is_reported(name, variant, mu, expected):
    snap, U, dim, cell, _ = _model(name, True)
    scaled, U2 = br.scale_snapshot(snap, U, mu, variant=variant)
    got = _checks(ra.check_rows(scaled, U2, dim))
    print("%s %s: %s" % (name, variant, sorted(got)))
    assert expected in got


# ---------------------------------------------------------------------------------------------------------------------
# 4. run_simulation's call order on a fake handle
# ---------------------------------------------------------------------------------------------------------------------
class _FakeBaroDevice(_FakeDevice):
    def scale_cell(self, mu, vscale=1.0):
        self._log("scale_cell", float(mu), float(vscale))
        return 1

    def compute_forces(self):
        self._log("compute_forces")
        return 0.0, 0.0


class _CountingRng:
    """Counts the Gaussian draws; everything else is the generator's."""

    def __init__(self, seed):
        self._g = np.random.default_rng(seed)
        self.normals = 0

    def standard_normal(self, *a, **kw):
        self.normals += 1 if not a and not kw else int(np.prod(a[0]))
        return self._g.standard_normal(*a, **kw)

    def __getattr__(self, name):
        return getattr(self._g, name)


def _fake_baro_state():
    state, _ = _fake_state()
    dev = _FakeBaroDevice()
    state.system.device = dev
    state.rng = _CountingRng(1)
    return state, dev


@pytest.mark.parametrize("stochastic", [True, False])
def test_call_order_with_a_barostat(tmp_path, stochastic):
    total, f = 40, 7
    state, dev = _fake_baro_state()
    U0 = np.array(state.unitcell)
    params = md.Parameters(1.0, N, 0.002, md.LennardJones())
    baro = md.StochasticCellRescaling(0.5, 1.0, 0.1, every=5, ktemp=0.7, stochastic=stochastic)
    swap = md.SwapMonteCarlo(10, 2, ktemp=0.7, seed=1)
    boo = md.BondOrder(0.9, order=6, every=1, nbins=5)          # (a sampler that may share a run with a barostat)
    out = str(tmp_path / "out")
    with np.errstate(all="ignore"):
        md.run_simulation(state, params, md.NVE(), total, f, out, bond_order=boo, swap=swap, barostat=baro)
    stops = list(range(4, total, 5))
    assert [st for st, m, _ in dev.trace if m == "scale_cell"] == stops
    assert state.rng.normals == (len(stops) if stochastic else 0)
    by_step = {}
    for st, m, _ in dev.trace:
        by_step.setdefault(st, []).append(m)
    for st in stops:
        ms = by_step[st]
        i = ms.index("scale_cell")
        assert ms[i + 1] == "compute_forces"                                    # scale, then forces
        assert "swap_rounds" not in ms[i:] and "boo_sample" not in ms[i:]        # after every sampler and after swap
        assert ((st + 1) % 10 == 0) == ("swap_rounds" in ms[:i])
        assert "snapshot_begin" not in ms[:i]                                    # before the frame export of that step
    # step 14: an output step the barostat shares -- sampler, then the coupling, then the frame export
    assert by_step[14] == ["boo_sample", "scale_cell", "compute_forces", "snapshot_begin"]
    assert sorted(set(np.cumsum(dev.segments) - 1)) == sorted(set(stops) | set(range(0, total, f)) | {total - 1})
    # mu and 1 / mu, and the host's cell follows coupling by coupling
    U = U0
    for (_, m, a), c in zip([t for t in dev.trace if t[1] == "scale_cell"], baro.couplings):
        assert a[1] == 1.0 / a[0] and c["mu"] == a[0]
        U = a[0] * U
        assert c["volume"] == abs(float(np.linalg.det(U))) and c["density"] == N / c["volume"] and c["rows_kept"] == 1
    assert np.array_equal(state.unitcell, U) and state.system.unitcell is state.unitcell and params.rho == 1.0
    assert baro.n_couplings == len(stops) and baro.mean_volume() > 0.0
    if not stochastic:
        # K = 1, W = 0 from the fake: P_int = 2 / (3 V) is below or above P0 = 0.5 as V tells
        assert all((c["mu"] < 1.0) == (c["p_int"] < 0.5) for c in baro.couplings)
    lines = open(os.path.join(out, "barostat.txt")).read().splitlines()
    assert lines[0] == "# step volume density p_int mu rows_kept" and len(lines) == 1 + len(stops)
    assert [int(l.split()[0]) for l in lines[1:]] == stops
    assert float(lines[-1].split()[1]) == baro.couplings[-1]["volume"]
    # the thermo line's density is n / V of the moment: with W = 0 the pressure column is rho T = (n / V)(2 K / nf)
    thermo = [l.split() for l in open(os.path.join(out, "thermo.txt")).read().splitlines()[1:]]
    last = thermo[-1]
    assert int(last[0]) == 35
    v35 = [c["volume"] for c in baro.couplings if c["step"] <= 35][-1]
    assert abs(float(last[3]) / float(last[2]) - N / v35) <= 2e-6 * N / v35       # (both columns have six decimals)
    # every frame carries the cell of its own moment: the edge after the couplings up to and including its step, though
    # the frame is written only after later couplings have moved state.unitcell on
    lines = open(os.path.join(out, "trajectory.xyz")).read().splitlines()
    at = [int(lines[i + 1]) for i, l in enumerate(lines) if l == "ITEM: TIMESTEP"]
    edge = [float(lines[i + 1].split()[1]) for i, l in enumerate(lines) if l.startswith("ITEM: BOX BOUNDS")]
    assert at == list(range(0, total, f))
    for s, e in zip(at, edge):
        want = U0[0, 0] * np.prod([c["mu"] for c in baro.couplings if c["step"] <= s])
        assert abs(e - want) <= 1e-6, (s, e, want)
    assert len(set(edge)) == len(edge)


def test_refusals_of_the_host_layer(tmp_path):
    params = md.Parameters(1.0, N, 0.002, md.LennardJones())
    baro = md.StochasticCellRescaling(0.5, 1.0, 0.1)
    state, _ = _fake_baro_state()
    with pytest.raises(ValueError, match="ktemp"):
        md.run_simulation(state, params, md.NVE(), 5, 2, str(tmp_path), barostat=baro)
    state, _ = _fake_baro_state()
    with pytest.raises(ValueError, match="Brownian"):
        md.run_simulation(state, params, md.Brownian(1.0), 5, 2, str(tmp_path), barostat=baro)


def test_samplers_of_one_cell_or_one_volume_are_refused_before_anything_is_opened(tmp_path):
    """dynamics, sq, currents, four_point, cage: md_scale_cell would refuse them on the device at the first coupling.  rdf,
    stress, orientational: their sums are normalised with one volume.  The refusal comes before the output directory
    exists."""
    params = md.Parameters(1.0, N, 0.002, md.LennardJones())
    kw = dict(lags=[1], origin_every=1)
    combos = dict(dynamics=md.SelfDynamics(**kw), sq=md.StructureFactor(4.5), currents=md.CurrentCorrelations(4.5, **kw),
                  four_point=md.FourPoint(0.3, **kw), cage=md.CageDynamics(0.9, **kw), rdf=md.RadialDistribution(1.0, 4),
                  stress=md.StressTensor(2), orientational=md.OrientationalCorrelation(0.9, 3))
    for name, smp in combos.items():
        state, dev = _fake_baro_state()
        out = tmp_path / name
        with pytest.raises(ValueError, match="barostat= cannot be combined with %s=" % name):
            md.run_simulation(state, params, md.NVT(1.0, 0.1), 5, 2, str(out), barostat=md.StochasticCellRescaling(0.5, 1.0, 0.1),
                              **{name: smp})
        assert not out.exists() and dev.trace == [] and dev.setups == []


def test_without_a_barostat_the_run_is_the_keywordless_one(tmp_path):
    """On the fake handle: the same trace, the same segments, the same files, byte for byte."""
    outs = []
    for kw in ({}, dict(barostat=None)):
        state, dev = _fake_baro_state()
        params = md.Parameters(1.0, N, 0.002, md.LennardJones())
        out = str(tmp_path / ("a" if not kw else "b"))
        with np.errstate(all="ignore"):
            md.run_simulation(state, params, md.NVE(), 20, 3, out, stress=md.StressTensor(4), **kw)
        outs.append((dev.trace, dev.segments, {f: open(os.path.join(out, f), "rb").read() for f in sorted(os.listdir(out))}))
    assert outs[0] == outs[1] and "barostat.txt" not in outs[0][2]


# ---------------------------------------------------------------------------------------------------------------------
# 5. plumbing
# ---------------------------------------------------------------------------------------------------------------------
def test_symbols_bindings_header_makefile_and_julia():
    assert "md_scale_cell" in _lib.EXPORTS
    for name in ("StochasticCellRescaling", "crescale_factor"):
        assert name in md.__all__ and getattr(md, name) is getattr(barostat, name)
    assert callable(md.MDDevice.scale_cell)
    header = open(os.path.join(ROOT, "include", "mdhip.h")).read()
    assert re.search(r"int md_scale_cell\(md_ctx \*ctx, double mu, double vscale, int \*rows_kept\);", header)
    assert "skin_eff" in header and "rows_kept" in header
    make = open(os.path.join(ROOT, "moleculardynamics", "jl_amd", "csrc", "Makefile")).read()
    rule = [l for l in make.splitlines() if l.startswith("libmdhip.so:")][0]
    assert "md_baro.hpp" in rule.split()
    assert os.path.isfile(os.path.join(ROOT, "moleculardynamics", "jl_amd", "csrc", "md_baro.hpp"))
    lib = _lib.load()
    assert lib.md_scale_cell.argtypes == [C.c_void_p, C.c_double, C.c_double, C.POINTER(C.c_int)]
    assert lib.md_scale_cell.restype is C.c_int
    julia = open(os.path.join(ROOT, "julia", "MDHip.jl")).read()
    assert "(:md_scale_cell, LIB)" in julia and re.search(r"^function scale_cell!\(", julia, flags=re.M)
    assert "scale_cell!" in julia.split("const LIB")[0]
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert re.search(r"^## 26\.", design, flags=re.M) and "md_scale_cell" in design


def test_a_null_handle_is_refused():
    lib = _lib.load()
    kept = C.c_int(7)
    assert lib.md_scale_cell(None, 1.0, 1.0, C.byref(kept)) != 0
    assert b"null handle" in lib.md_last_error(None)
