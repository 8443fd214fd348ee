"""-m gpu: a run with every sampler attached at once, audited against its own frames (tests/sampler_audit.py).

Per case three kinds of run from identical initial states and seeds: TOGETHER (all samplers), ALONE (one run per sampler, cut into TOGETHER's
segments by a stops-only object; bond_order accompanies clusters-solid and orientational; in B every run keeps the swap object, and one run has swap
only), RECORDED (all samplers under the Recorder).  Asserted: (a) the run files and the final state are bit-identical in
all runs; (b) every sampler file and every public accumulator of TOGETHER equals that sampler's ALONE run bit for bit;
(c) RECORDED equals TOGETHER (the recorder changes nothing); (d) audit(RECORDED) passes: the documented call order, the
pre-swap diameters, and after every sampler call the accumulators a CPU restatement computes from the recorded frames;
(e) TOGETHER once more on the same handle after reset() gives the same files.

The inputs (stated here, chosen on the CPU with the oracle's trajectory and the references so that the preconditions the
test asserts hold and no cage overflow or range error occurs):

A  lj_system(1000) (3-D, rho 0.897, N = 15 * 64 + 40), LJ cutoff 2.5, NVT kT 2.5 tau 0.1, dt 0.005, 64 steps, output every
   8; ten lags 1..10 with origin_every 1 (10 pairs a call, 10 slots, 64 origins); rdf / sq / clusters / orientational at
   every 2nd output step, so steps 0, 16, 32, 48 are shared by all ten.
B  poly_system() (2-D, N = 1200 = 18 * 64 + 48), Polydisperse(1.25, 0.2) cutoff 1.5, NVT kT 1 tau 0.1, dt 0.004, 60 steps,
   output every 3; psi_6, g6(r), clusters of the solid particles, CageDynamics(scaled=True); swap after every 10th step
   (steps 9, 19, ...: 9 and 39 are output steps, shared with every sampler); lags 1, 2, 3, 4, 5, 6, 8, 9, 11.
C  A's particles, shifted by 0.47 lattice spacings so that a layer sits next to every face, in the cell sheared by three
   lattice spacings, Brownian kT 1.5, dt 4e-4 (the largest stable step of the LJ liquid, tests/test_gpu_loop_audit.py), 48
   steps, output every 4, the eight samplers Brownian dynamics allows (no currents, no stress).
D  A with MDHIP_NO_FUSED_STEP=1."""
import bisect
import copy
import os

import numpy as np
import pytest

from tests.sampler_audit import AuditGuard, Recorder, Restatement, _object_fields, audit, expected_trace, margins_lines
from tests.util import lj_system, poly_system, sheared

pytestmark = pytest.mark.gpu

RUN_FILES = ("thermo.txt", "trajectory.xyz", "final.xyz")
FILES = {"rdf": ("rdf.txt",), "dynamics": ("dynamics.txt", "vanhove.txt"), "sq": ("sq.txt", "fqt.txt"),
         "currents": ("currents.txt", "vacf.txt"), "stress": ("stress.txt", "stress_acf.txt"),
         "bond_order": ("bond_order.txt", "bond_order_series.txt"), "clusters": ("clusters.txt", "clusters_series.txt"),
         "cage": ("cage.txt",), "four_point": ("chi4.txt", "s4.txt"), "orientational": ("orient_corr.txt",),
         "swap": ("swap.txt",)}
LAGS_A = list(range(1, 11))
LAGS_B = [1, 2, 3, 4, 5, 6, 8, 9, 11]


def _case(name):
    import moleculardynamics.jl_amd as md
    if name in ("A", "C", "D"):
        s = lj_system(1000)
        c = dict(system=s, kind=0, pot_params=[1.0, 1.0, 2.5], cutoff=2.5, force_range=2.5, potential=md.LennardJones(),
                 rho=0.897, lags=LAGS_A, swap=None)
        if name == "C":
            a = s["box"][0] / 10.0                  # the lattice spacing; the shift puts a layer of particles next to every face
            c.update(system=sheared(dict(s, x=s["x"] + 0.47 * a), 3.0 * a), ensemble=lambda: md.Brownian(1.5), dt=4e-4,
                     total=48, f=4)
        else:
            c.update(ensemble=lambda: md.NVT(2.5, 0.1), dt=0.005, total=64, f=8)
        c["env"] = "MDHIP_NO_FUSED_STEP" if name == "D" else None
    else:
        c = dict(system=poly_system(), kind=2, pot_params=[1.25, 0.2], cutoff=1.5, force_range=1.5,
                 potential=md.Polydisperse(1.25, 0.2), rho=1.0, lags=LAGS_B, ensemble=lambda: md.NVT(1.0, 0.1), dt=0.004,
                 total=60, f=3, env=None, swap=lambda: md.SwapMonteCarlo(10, 2, fraction=0.02, seed=7))
    c["name"] = name
    return c


def _samplers(c):
    import moleculardynamics.jl_amd as md
    kw = dict(lags=c["lags"], origin_every=1)
    two_d = c["system"]["dim"] == 2
    if two_d:
        s = dict(rdf=md.RadialDistribution(4.0, 80), sq=md.StructureFactor(6.0, max_per_bin=4, dynamic=True, **kw),
                 bond_order=md.BondOrder(1.45, order=6, nbins=50, threshold=0.5, min_connections=3),
                 clusters=md.ClusterAnalysis(1.3, members="solid", max_size=64),
                 cage=md.CageDynamics(1.2, r_break=1.4, scaled=True, max_neighbours=32, q=[6.0], **kw),
                 four_point=md.FourPoint(0.15, q_max=2.0, max_per_bin=4, **kw),
                 orientational=md.OrientationalCorrelation(4.0, 40),
                 currents=md.CurrentCorrelations(3.0, max_per_bin=4, **kw), stress=md.StressTensor(3, nlags=3))
    else:
        s = dict(rdf=md.RadialDistribution(3.0, 60, every=2),
                 sq=md.StructureFactor(8.0, max_per_bin=4, every=2, dynamic=True, **kw),
                 bond_order=md.BondOrder(1.5, order=6, nbins=50), clusters=md.ClusterAnalysis(1.02, every=2, max_size=64),
                 cage=md.CageDynamics(1.5, r_break=1.7, max_neighbours=32, q=[6.0], **kw),
                 four_point=md.FourPoint(0.3, q_max=3.0, max_per_bin=4, **kw),
                 orientational=md.OrientationalCorrelation(3.0, 30, every=2))
        if c["name"] != "C":
            s.update(currents=md.CurrentCorrelations(4.0, max_per_bin=4, **kw), stress=md.StressTensor(8, nlags=3))
    s["dynamics"] = md.SelfDynamics(q=[2.0 * np.pi, 3.0], r_max=1.5, nbins=60, **kw)
    if c["swap"] is not None:
        s["swap"] = c["swap"]()
    return s


def _state(c, device=None):
    import moleculardynamics.jl_amd as md
    s = c["system"]
    params = md.Parameters(c["rho"], s["n"], c["dt"], c["potential"])
    state = md.initialize_state(params, None, dimension=s["dim"], cutoff=c["cutoff"], unitcell=s.get("cell", s["box"]),
                                positions=s["x"].copy(), diameters=s["diam"].copy(), rng=np.random.default_rng(4))
    state.velocities = s["v"].copy()
    if device is not None:
        state.system.device.close()
        state.system.device = device
    return state, params


def _run(c, path, samplers, state=None, params=None, record=False):
    import moleculardynamics.jl_amd as md
    if state is None:
        state, params = _state(c)
    rec = None
    if record:
        rec = state.system.device = Recorder(state.system.device)
    md.run_simulation(state, params, c["ensemble"](), c["total"], c["f"], str(path), **samplers)
    if record:
        state.system.device = rec._dev
    dev = state.system.device
    final = dev.download() + (dev.diameters(),)
    return state, rec, final


class _StopsOnly:
    """Speaks run_simulation's sampler protocol and does nothing but end a segment at the given steps: an ALONE run is cut
    into the segments of TOGETHER.  The segmentation decides when the list is rebuilt and with it the order of the force
    sums, so only runs with equal stops can be compared bit for bit."""

    def __init__(self, stops):
        self.stops = sorted(stops)

    def _begin(self, dev, run):
        pass

    def _next(self, step):
        i = bisect.bisect_left(self.stops, step)
        return self.stops[i] if i < len(self.stops) else None

    def _act(self, dev, step):
        pass

    def _finish(self, dev, run, pathname):
        pass


def _same_files(pa, pb, names, what):
    for f in names:
        a, b = os.path.join(str(pa), f), os.path.join(str(pb), f)
        assert os.path.exists(a) == os.path.exists(b), (what, f)
        if os.path.exists(a):
            assert open(a, "rb").read() == open(b, "rb").read(), (what, f)


def _same_final(fa, fb, what):
    for k, (u, w) in enumerate(zip(fa, fb)):
        assert u.tobytes() == w.tobytes(), (what, ("x", "v", "f", "images", "diameters")[k])


def _same_fields(name, a, b, what):
    for k, (u, w) in enumerate(zip(_object_fields(name, a), _object_fields(name, b))):
        if u is None or w is None:
            assert u is None and w is None, (what, name, k)
        else:
            assert np.asarray(u).tobytes() == np.asarray(w).tobytes() and np.shape(u) == np.shape(w), (what, name, k)


def _pair_force(oracle, c):
    pot = oracle.make_pot(c["kind"], c["pot_params"])

    def force(r, si, sj):
        return np.array([oracle.evaluate(pot, float(a), float(b), float(d))[1] for a, b, d in zip(r, si, sj)])
    return force


def _swap_truth(oracle, c, swap):
    """tests/swap_reference.py on the recorded frame: the diameters and the counts a block must produce."""
    from tests import swap_reference as sr
    pot = oracle.make_pot(c["kind"], c["pot_params"])
    ens = c["ensemble"]()

    def truth(fr, diam, step, first_round):
        system = dict(c["system"], x=fr.x)
        ktemp = swap.ktemp if swap.ktemp is not None else float(ens.ktemp(step + 1))
        rounds = sr.run_rounds(sr.Frame(system, c["cutoff"], pot, x=fr.x), diam, swap.seed, first_round, swap.rounds,
                               swap.fraction, ktemp, swap.max_diameter_difference)
        for r in rounds:                # a decision on the knife edge of the Metropolis test is a guard (conditions())
            for i in np.flatnonzero(r["status"] >= sr.REJECTED):
                if abs(np.log(r["u3"][i]) + r["du"][i] / ktemp) <= 1e-9 * (1.0 + r["S"][i] / ktemp):
                    raise AuditGuard("step %d: a swap decision sits on the acceptance threshold" % step)
        st = np.concatenate([r["status"] for r in rounds])
        counts = dict(proposed=(st >= sr.VOID).sum(), void=(st == sr.VOID).sum(), lost=(st == sr.LOST).sum(),
                      blocked=(st == sr.BLOCKED).sum(), filtered=(st == sr.FILTERED).sum(),
                      accepted=(st == sr.ACCEPTED).sum(), decided=(st >= sr.REJECTED).sum())
        return rounds[-1]["diam"], counts
    return truth


def _preconditions(c, rec, s):
    name, total = c["name"], c["total"]
    calls = [rec.calls[i] for i in sorted(rec.calls)]
    first_stop, last_stop = calls[0]["step"], calls[-1]["step"]
    after_first = max(k["rebuilds"][1] for k in calls if k["step"] == first_stop)
    before_last = min(k["rebuilds"][0] for k in calls if k["step"] == last_stop)
    inside = rec.rebuilding_calls()
    print("%s: rebuilds after the first stop %d, before the last %d; rebuilding sampler calls %s; pairs per call %d"
          % (name, after_first, before_last, inside[:4], rec.pairs_per_call()))
    if name == "C":
        # the list is invalid at every stop: the first row walker (bond order; the cage origin where bond order does not
        # act) rebuilds, after rdf / dynamics / sq of that stop and before clusters, cage, orientational
        stops = sorted({k["step"] for k in calls})
        assert {st for st, _ in inside} == set(stops)
        assert {m for _, m in inside} <= {"boo_sample", "cage_origin"}
        for st, m in inside:
            at = [k["method"] for k in calls if k["step"] == st]
            assert set(at[:at.index(m)]) <= {"rdf_sample", "dyn_sample", "dyn_origin", "sq_sample", "cage_sample"}, (st, at)
        shared = [k["method"] for k in calls if k["step"] == 8]
        assert shared.index("sq_sample") < shared.index("boo_sample") < shared.index("cluster_sample") < shared.index("mpc_sample")
        assert (8, "boo_sample") in inside
    else:
        assert before_last > after_first            # a rebuild strictly between the first and the last sampler stop
    dyn = s["dynamics"]
    assert sum(1 for ev in dyn.schedule(total)[1].values() if ev[1] is not None) > dyn.nslots      # the ring wrapped
    assert rec.pairs_per_call() > 8
    crossed = any(np.any(rec.frames[st + l].img != rec.frames[st].img)
                  for st in rec.frames for l in dyn.lags if st + l in rec.frames)
    assert crossed                                  # an image count changed between an origin and a sample
    methods = {}
    for st, m, _ in rec.trace:
        methods.setdefault(st, set()).add(m)
    everyone = {"rdf_sample", "dyn_sample", "sq_sample", "boo_sample", "cluster_sample", "cage_sample", "chi4_sample",
                "mpc_sample"} | (set() if name == "C" else {"cur_sample", "stress_sample"})
    assert any(everyone <= v and (c["swap"] is None or "swap_rounds" in v) for v in methods.values())
    if c["swap"] is not None:
        assert sum(b["accepted"] for b in s["swap"].blocks) >= 1
        solid = s["bond_order"].frames[:, 6]
        assert np.all(solid > 0) and np.all(solid < c["system"]["n"])       # the solid set: not empty, not everything
        assert np.array_equal(s["clusters"].frames[:, 0], solid[: len(s["clusters"].frames)])


@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_every_sampler_at_once(tmp_path, monkeypatch, oracle, name):
    c = _case(name)
    if c["env"]:
        monkeypatch.setenv(c["env"], "1")
    n = c["system"]["n"]
    assert 1000 <= n <= 4096 and n % 64 != 0

    # together, and once more on the same handle after reset (e)
    s = _samplers(c)
    state, _, final = _run(c, tmp_path / "together", s)
    first = copy.deepcopy(s)
    for v in s.values():
        v.reset()
    state2, params2 = _state(c, device=state.system.device)
    _, _, final2 = _run(c, tmp_path / "again", s, state2, params2)
    _same_files(tmp_path / "together", tmp_path / "again", RUN_FILES + sum(FILES.values(), ()), "second pass")
    # (files only: on a handle that has run before the final state agrees with the first pass's to rounding, not to the bit
    # -- DESIGN.md section 15.1)
    for k, (u, w) in enumerate(zip(final, final2)):
        assert np.allclose(u, w, rtol=0.0, atol=1e-9), ("second pass", k)
    state.system.device.close()
    s = first

    # recorded (c), audited (d)
    sr_ = _samplers(c)
    st_r, rec, final_r = _run(c, tmp_path / "recorded", sr_, record=True)
    st_r.system.device.close()
    _same_files(tmp_path / "together", tmp_path / "recorded", RUN_FILES + sum(FILES.values(), ()), "recorded")
    _same_final(final, final_r, "recorded")
    for k in sr_:
        if k != "swap":
            _same_fields(k, s[k], sr_[k], "recorded")
    _preconditions(c, rec, sr_)
    U = np.asarray(c["system"].get("cell", c["system"]["box"]), dtype=np.float64)
    R = Restatement(n, c["system"]["dim"], U, pair_force=_pair_force(oracle, c), force_range=c["force_range"])
    truth = _swap_truth(oracle, c, sr_["swap"]) if c["swap"] is not None else None
    margins = audit(rec, sr_, R, c["total"], c["f"], ensemble=c["ensemble"](), swap_truth=truth)
    lines = margins_lines(name, margins)
    print("\n".join(lines))
    if os.environ.get("SAMPLER_AUDIT_MARGINS"):
        with open(os.environ["SAMPLER_AUDIT_MARGINS"], "a") as io:
            io.write("\n".join(lines) + "\n")

    # alone (a), (b)
    groups = [[k] for k in s if k not in ("swap", "bond_order")] + [["bond_order"]]
    if c["swap"] is not None:
        groups.append([])
    stops = expected_trace(s, c["total"], c["f"], ensemble=c["ensemble"]())[1]
    for group in groups:
        if group and group[0] == "orientational" or (group == ["clusters"] and s["clusters"].members == "solid"):
            group = ["bond_order"] + group
        every = _samplers(c)
        alone = {k: every[k] for k in group + (["swap"] if c["swap"] is not None else [])}
        alone["dynamics" if "rdf" in group else "rdf"] = _StopsOnly(stops)
        what = "alone: " + "+".join(group or ["swap"])
        st_a, _, final_a = _run(c, tmp_path / "alone", alone)
        st_a.system.device.close()
        _same_files(tmp_path / "together", tmp_path / "alone", RUN_FILES + FILES["swap"], what)
        _same_final(final, final_a, what)
        for k in group:
            _same_files(tmp_path / "together", tmp_path / "alone", FILES[k], what)
            _same_fields(k, s[k], alone[k], what)
        for f in os.listdir(str(tmp_path / "alone")):
            os.remove(os.path.join(str(tmp_path / "alone"), f))
