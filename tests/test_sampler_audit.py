"""CPU: the sampler audit (tests/sampler_audit.py) proved on a model handle.

ModelDevice has MDDevice's surface.  run / run_brownian step along a scripted frame sequence (no MD: small random
displacements with wraps and image counts, fresh velocities with a last "thermostat" scale, occasional diameter
exchanges); the sampler methods are the auditor's own Restatement behind the device interface, with what a device keeps
per slot (the bond-order frame) stored by slot together with that build's slot -> id permutation; a list rebuild is a
random re-permutation of the slots.  Driven through the real run_simulation with all ten samplers and swap, the audit
passes clean; with one of twelve sabotages built into the model it fails and names the right sampler and step."""
import math
import types

import numpy as np
import pytest

import moleculardynamics.jl_amd as md
from tests.sampler_audit import (AuditGuard, Recorder, Restatement, SamplerAuditFailure, _object_fields, audit, expected,
                                 expected_trace)

N = 96
CELLS = {
    "3d-general": np.array([[5.0, 0.8, 0.3], [0.0, 4.8, -0.5], [0.0, 0.0, 5.2]]),
    "2d": np.array([[10.0, 0.0], [0.0, 9.5]]),
}
SWAP_EVERY = 5


def _soft_force(r, si, sj):
    """A short-ranged repulsion f(r) = 24 (1 - r / s)^2 / s for r < s = 1.25 (s_i + s_j) / 2: the model's potential."""
    s = 1.25 * (si + sj) / 2.0
    return np.where(r < s, 24.0 * (1.0 - r / s) ** 2 / s, 0.0)


class ModelDevice(Restatement):
    def __init__(self, unitcell, seed=5, sabotage=0):
        U = np.asarray(unitcell, dtype=np.float64)
        super().__init__(N, U.shape[0], U, pair_force=_soft_force, force_range=1.25 * 1.2)
        self.unitcell, self.list_cutoff = U, 1.5
        self.rng = np.random.default_rng(seed)
        self.sabotage = sabotage
        self.step, self.rebuilds, self.list_valid = 0, 0, False
        self.perm = np.arange(N)
        self.prev_stop = None
        self.pending_cage = []

    # -- state -------------------------------------------------------------------------------------------------------
    def set_potential(self, kind, params):
        pass

    def upload(self, x=None, v=None, f=None, images=None, diameters=None):
        self.x = np.array(x, dtype=np.float64)
        self.v = np.zeros_like(self.x) if v is None else np.array(v, dtype=np.float64)
        self.v_unscaled = self.v.copy()
        self.f = np.zeros_like(self.x)
        self.img = np.array(images, dtype=np.int32)
        self.diam = np.array(diameters, dtype=np.float64)
        self.step, self.list_valid = 0, False
        self._new_frame()

    def _new_frame(self):
        self.fr = types.SimpleNamespace(step=self.step - 1, x=self.x.copy(), v=self.v.copy(), f=self.f.copy(),
                                        img=self.img.copy(), diam=self.diam.copy())
        self._cache = {}

    def download(self):
        return self.x.copy(), self.v.copy(), self.f.copy(), self.img.copy()

    def diameters(self):
        return self.diam.copy()

    def stats(self):
        return dict(rebuilds=self.rebuilds)

    def snapshot_begin(self):
        self._snap = (self.x.copy(), self.img.copy())

    def snapshot_end(self):
        return self._snap

    def _rebuild(self):
        self.perm = self.rng.permutation(N)
        self.rebuilds += 1
        self.list_valid = True

    def _ensure_list(self):
        if not self.list_valid:
            self._rebuild()

    def _advance(self, nsteps, brownian):
        self._flush_cage()
        self.prev_stop = self.fr
        uinv = np.linalg.inv(self.U)
        for _ in range(int(nsteps)):
            self.x += self.rng.normal(0.0, 0.06, self.x.shape)
            shift = np.floor(self.x @ uinv.T)
            self.img += shift.astype(np.int32)
            self.x -= shift @ self.U.T
        self.v_unscaled = self.rng.normal(0.0, 1.0, self.x.shape)
        self.v = self.v_unscaled * 1.03                         # the thermostat's scale of the last step
        self.step += int(nsteps)
        if brownian:
            self.list_valid = False
        elif not self.list_valid or self.rng.random() < 0.4:    # a rebuild inside the segment
            self._rebuild()
        if self.sabotage == 7 and self.step % SWAP_EVERY == 0:
            self._exchange()
        self._new_frame()

    def run(self, nsteps, dt, *a, **kw):
        self._advance(nsteps, False)
        return 0.0, 0.0, 1.0

    def run_brownian(self, nsteps, dt, ktemp, seed, first_step=0, virial_every=10):
        self._advance(nsteps, True)
        return dict(U=0.0, W=0.0, virial_sum=0.0, virial_count=1.0)

    # -- swap --------------------------------------------------------------------------------------------------------
    def swap_setup(self, fraction, max_diameter_difference=None, seed=0):
        pass

    def _exchange(self):
        for _ in range(6):
            i, j = self.rng.choice(N, 2, replace=False)
            self.diam[i], self.diam[j] = self.diam[j], self.diam[i]

    def swap_rounds(self, nrounds, ktemp, first_round=0):
        if self.sabotage != 7:
            self._exchange()
        self._flush_cage()
        self.fr = types.SimpleNamespace(**{**vars(self.fr), "diam": self.diam.copy()})
        self._cache = {}
        return dict(proposed=9, void=0, lost=0, blocked=1, filtered=0, accepted=6, decided=8, du_accepted=0.0, U=0.0, W=0.0)

    # -- the sabotages -----------------------------------------------------------------------------------------------
    def frame_for(self, prefix):
        fr = self.fr
        if self.sabotage == 1 and prefix == "rdf" and self.prev_stop is not None:
            return self.prev_stop                               # 1: the previous stop's frame
        if self.sabotage == 9 and prefix == "cur":              # 9: the velocities before the thermostat's scale
            return types.SimpleNamespace(**{**vars(fr), "v": self.v_unscaled.copy()})
        if self.sabotage == 10 and prefix == "chi4":            # 10: the image counts ignored
            return types.SimpleNamespace(**{**vars(fr), "img": np.zeros_like(fr.img)})
        return fr

    def dyn_setup(self, nslots, *a, **kw):
        super().dyn_setup(nslots, *a, **kw)
        if self.sabotage == 2:                                  # (a slot read before it was written holds the upload)
            self.dyn.org = {k: (self.fr.x.copy(), self.fr.img.copy()) for k in range(nslots)}

    def dyn_origin(self, slot):
        self._stored = getattr(self, "_stored", {})
        if self.sabotage == 2:                                  # 2: the origin in slot + 1 mod nslots
            slot = (slot + 1) % self.dyn.nslots
        self._stored[slot] = self._stored.get(slot, 0) + 1
        super().dyn_origin(slot)

    def _count_sample(self, prefix, slot, row):
        if (self.sabotage == 12 and prefix == "dyn" and self._stored.get(slot, 0) > 1
                and not getattr(self, "_dropped", False)):
            self._dropped = True                                # 12: nsamples of one lag row off by one at the ring wrap
            return
        super()._count_sample(prefix, slot, row)

    def sq_sample(self, static=True, slots=(), rows=(), origin=None):
        super().sq_sample(True if self.sabotage == 8 else static, slots, rows, origin)      # 8: a static sample anywhere

    def stress_sample(self):
        self._ensure_list()
        self._nstress = getattr(self, "_nstress", 0) + 1
        super().stress_sample()
        if self.sabotage == 6 and self._nstress == 3:           # 6: a sample taken twice
            super().stress_sample()

    def boo_sample(self):
        self._ensure_list()
        self._nboo = getattr(self, "_nboo", 0) + 1
        if self.sabotage == 5 and self._nboo == 2:              # 5: a sample skipped
            return
        super().boo_sample()
        # what the device keeps: the frame per slot, with that build's slot -> id permutation
        self._boo_perm = self.perm.copy()
        self._boo_solid_slot = self.boo_last["solid"][self.perm]
        self._boo_qlm_slot = self.boo_last["qlm"][self.perm]
        self._boo_qlm_history = getattr(self, "_boo_qlm_history", []) + [(self._boo_perm, self._boo_qlm_slot)]

    def solid_members(self):
        member = np.zeros(N, dtype=bool)
        if self.sabotage == 3:                                  # 3: by slot, after a re-permutation inside the stop
            self._rebuild()
            member[self.perm] = self._boo_solid_slot
        else:
            member[self._boo_perm] = self._boo_solid_slot
        return member

    def cluster_sample(self):
        self._ensure_list()
        super().cluster_sample()

    def mpc_marks_qlm(self):
        perm, slot = self._boo_qlm_history[-1]
        if self.sabotage == 4 and len(self._boo_qlm_history) > 1:   # 4: the bond-order frame of an earlier sample
            perm, slot = self._boo_qlm_history[-2]
        qlm = np.empty_like(slot)
        qlm[perm] = slot
        return qlm

    def mpc_sample(self):
        self._ensure_list()
        super().mpc_sample()

    def cage_origin(self, slot):
        self._ensure_list()
        if self.sabotage == 11:                                 # 11: the neighbour table built after the swap block
            self.pending_cage.append((slot, self.fr))
        else:
            super().cage_origin(slot)

    def _flush_cage(self):
        for slot, fr in self.pending_cage:
            self.cage_store(slot, types.SimpleNamespace(**{**vars(fr), "diam": self.diam.copy()}))
        self.pending_cage = []

    def cage_sample(self, slots, rows):
        self._flush_cage()
        super().cage_sample(slots, rows)


def _lattice(U, rng):
    d = U.shape[0]
    m = int(math.ceil(N ** (1.0 / d)))
    grid = np.stack(np.meshgrid(*[np.arange(m)] * d, indexing="ij"), -1).reshape(-1, d)[:N]
    fr = (grid + 0.5 + rng.uniform(-0.2, 0.2, grid.shape)) / m
    return fr @ U.T


def _run(cell, sabotage, tmp_path, brownian=False):
    U = CELLS[cell]
    d = U.shape[0]
    rng = np.random.default_rng(11)
    x = _lattice(U, rng)
    diam = rng.uniform(0.8, 1.2, N)
    dev = ModelDevice(U, sabotage=sabotage)
    rec = Recorder(dev)
    system = types.SimpleNamespace(device=rec, positions=x, xpositions=None,
                                   energy_and_forces=types.SimpleNamespace(forces=np.zeros((N, d)), energy=0.0, virial=0.0))
    state = md.SimulationState(system, diam, np.random.default_rng(1), U, rng.normal(size=(N, d)),
                               np.zeros((N, d), dtype=np.int32), d, d * (N - 1.0))
    params = md.Parameters(N / abs(np.linalg.det(U)), N, 0.002, md.LennardJones())
    lags, E = [1, 2, 3, 5, 6, 8, 9, 11, 12], 1                  # 12 slots, 40 origins: the ring wraps; 9 pairs a call
    order = 6
    s = dict(rdf=md.RadialDistribution(1.5, 30, every=2), dynamics=md.SelfDynamics(q=[2.0, 5.0], r_max=2.0, nbins=40,
                                                                                   lags=lags, origin_every=E),
             sq=md.StructureFactor(4.0, every=2, dynamic=True, lags=lags, origin_every=E),
             bond_order=md.BondOrder(1.45, order=order, nbins=20, threshold=0.3, min_connections=2),
             clusters=md.ClusterAnalysis(1.2, members="solid", every=2, max_size=16),
             cage=md.CageDynamics(1.2, r_break=1.35, scaled=True, max_neighbours=32, q=[3.0], lags=lags, origin_every=E),
             four_point=md.FourPoint(0.3, q_max=3.0, lags=lags, origin_every=E),
             orientational=md.OrientationalCorrelation(1.5, 15, every=2),
             swap=md.SwapMonteCarlo(SWAP_EVERY, 3, seed=9))
    if brownian:
        ens = md.Brownian(1.0)
    else:
        ens = md.NVT(lambda t: 1.0, 0.1)
        s["currents"] = md.CurrentCorrelations(4.0, lags=lags, origin_every=E)
        s["stress"] = md.StressTensor(4, nlags=3)
    total, f = 40, 4
    with np.errstate(all="ignore"):
        md.run_simulation(state, params, ens, total, f, str(tmp_path), **s)
    R = Restatement(N, d, U, pair_force=_soft_force, force_range=1.25 * 1.2)
    return rec, s, lambda: audit(rec, s, R, total, f, ensemble=ens)


@pytest.mark.parametrize("cell", list(CELLS))
def test_the_clean_model_run_passes(tmp_path, cell):
    rec, s, go = _run(cell, 0, tmp_path)
    margins = go()
    assert all(m == 0.0 for m in margins.values())              # the model is the restatement: not a bit differs
    U = CELLS[cell]
    end = expected(rec.frames, rec.setups, s, Restatement(N, U.shape[0], U, pair_force=_soft_force, force_range=1.5), 40, 4,
                   ensemble=md.NVT(lambda t: 1.0, 0.1))
    assert set(end) == set(s) - {"swap"}
    for name, rows in end.items():                              # the objects hold what expected() restates
        for (q, val, _), got in zip(rows, _object_fields(name, s[name])):
            assert np.array_equal(np.asarray(val), np.asarray(got)), (name, q)
    # the run was worth auditing: all ten samplers and swap met at one stop, the ring wrapped, a call carried > 8 pairs,
    # images changed, a rebuild fell between two samplers' stops, diameters were exchanged
    methods = {}
    for step, m, _ in rec.trace:
        methods.setdefault(step, set()).add(m)
    assert any(len(v) >= 14 and "swap_rounds" in v for v in methods.values())
    assert rec.pairs_per_call() > 8
    assert len(s["dynamics"].schedule(40)[1]) > s["dynamics"].nslots
    first, last = min(rec.frames), max(rec.frames)
    assert any(rec.frames[last].img.ravel() != rec.frames[first].img.ravel())
    assert not np.array_equal(rec.frames[last].diam, rec.frames[first].diam)
    assert 0 < s["clusters"].sum_fr[0] < N * s["clusters"].nsamples
    assert all(v.nsamples.min() > 0 for k, v in s.items() if k in ("dynamics", "cage", "four_point", "currents"))


def test_the_clean_brownian_model_run_passes(tmp_path):
    """The list is invalid at every stop: the first row walker rebuilds between two other samplers' calls."""
    rec, s, go = _run("3d-general", 0, tmp_path, brownian=True)
    go()
    calls = rec.rebuilding_calls()
    assert calls and {m for _, m in calls} <= {"boo_sample", "cage_origin"}


SABOTAGES = {   # number: (the sampler the audit must name, the quantity it must name first or None)
    1: ("rdf", "counts"), 2: ("dynamics", None), 3: ("clusters", None), 4: ("orientational", None),
    5: ("bond_order", "nsamples"), 6: ("stress", "nsamples"), 7: ("swap", None), 8: ("sq", "nstatic"),
    9: ("currents", None), 10: ("four_point", None), 11: ("cage", None), 12: ("dynamics", "nsamples"),
}


@pytest.mark.parametrize("sabotage", sorted(SABOTAGES))
def test_each_sabotage_is_caught_with_sampler_and_step(tmp_path, sabotage):
    rec, s, go = _run("3d-general", sabotage, tmp_path)
    with pytest.raises(SamplerAuditFailure) as e:
        go()
    name, quantity = SABOTAGES[sabotage]
    assert e.value.sampler == name, str(e.value)
    if quantity is not None:
        assert e.value.quantity == quantity, str(e.value)
    # the step: the first stop at which the sabotaged model departs from the restatement, found independently by
    # comparing the sabotaged recording with a clean one call by call
    clean, _, _ = _run("3d-general", 0, tmp_path / "clean")
    assert e.value.step == _first_departure(rec, clean, sabotage), str(e.value)


def _first_departure(rec, clean, sabotage):
    if sabotage == 7:           # the frames differ, not the reads: the first stop whose frame carries other diameters
        return min(s for s in clean.frames if not np.array_equal(clean.frames[s].diam, rec.frames[s].diam))
    for i in sorted(clean.calls):
        a, b = clean.calls[i], rec.calls[i]
        for u, v in zip(a["read"], b["read"]):
            if (u is None) != (v is None) or (u is not None and not np.array_equal(np.asarray(u), np.asarray(v))):
                return a["step"]
    raise AssertionError("the sabotage changed nothing")


def test_expected_trace_is_the_drivers_trace(tmp_path):
    rec, s, _ = _run("2d", 0, tmp_path)
    want, stops = expected_trace(s, 40, 4, ensemble=md.NVT(lambda t: 1.0, 0.1))
    assert rec.trace == want and stops[-1] == 39


def test_a_knife_edge_is_a_guard_not_a_failure():
    U = np.diag([6.0, 6.0, 6.0])
    R = Restatement(2, 3, U)
    R.boo_setup(1.0, order=6)
    R.set_frame(types.SimpleNamespace(step=0, x=np.array([[1.0, 1.0, 1.0], [2.0 - 1e-13, 1.0, 1.0]])))
    with pytest.raises(AuditGuard):
        R.boo_sample()
