"""The slab audit's harness proved on the CPU: tests/domain_audit_worker.py and its command protocol under gloo with 2 and
3 ranks, on a MODEL of DomainDevice (every rank holds the global state and advances it with step_audit.OracleStepper; what
a rank contributes to the gathered state is its slab's share, selected by owner_of).  The clean model passes; with one
rank sabotaged -- one slab fault per run -- the audit fails on the check and quantity named here.  No GPU is touched.

The model, in full: after every run() the ranks assemble the state from their shares (ownership by owner_of at the end of
the run, each rank judging by its own copy) and all adopt it, as the real thing's particles live on exactly one rank; the
returned U, W, K are the mean of the ranks' figures (the real thing all-reduces per-rank sums), so one rank's wrong figure
shows.  Also here: the thermo= keyword of DomainDevice.run / run_async / run_native, checked on a recording stand-in for
the library (argument plumbing only), and a follower that raises.
"""
import contextlib
import json
import os
import time
import types

import numpy as np
import pytest

from tests import step_audit as sa
from tests.domain_audit_worker import launch

FACTORY = "tests.test_slab_audit:model_factory"


# ---------------------------------------------------------------------------------------------
# the model and its sabotaged steppers (run inside the worker's ranks)
# ---------------------------------------------------------------------------------------------
class SlabStepper(sa.OracleStepper):
    """OracleStepper that knows its slab."""
    rank = world = 0
    Lx = 1.0

    def mine(self, x=None):
        from moleculardynamics.jl_amd.domain import owner_of
        return owner_of((self.x if x is None else x)[:, 0], self.Lx, self.world) == self.rank

    def brute(self, x, diam=None):
        return self.o.forces_brute(x, self.box, self.cutoff, self.pot, self.diam if diam is None else diam)


class DroppedPair(SlabStepper):
    """Its share's forces with one cross-face pair inside r_c left out: the farthest such pair (|F(r_c)| = 0.039 for LJ),
    outside the knife-edge window."""

    def forces(self, x):
        f, u, w = super().forces(x)
        m = self.mine(x)
        d2 = sa.pair_d2(x, self.box)
        d2 = np.minimum(d2, d2.T)           # (either orientation of the reference form)
        ok = m[:, None] & ~m[None, :] & (d2 < self.cutoff ** 2 * (1.0 - 1e-6))
        assert ok.any(), "no pair across the face"
        i, j = np.unravel_index(np.argmax(np.where(ok, d2, -1.0)), d2.shape)
        fs = self.brute(np.delete(x, j, axis=0), np.delete(self.diam, j))[0]
        f[i] = fs[i if i < j else i - 1]
        return f, u, w


class CrossEnergyTwice(SlabStepper):
    """U counted twice for the pairs across its face."""

    def forces(self, x):
        f, u, w = super().forces(x)
        m = self.mine(x)
        cross = u - self.brute(x[m], self.diam[m])[1] - self.brute(x[~m], self.diam[~m])[1]
        return f, u + cross, w


class SeamImageKept(SlabStepper):
    """The x image counter not changed for a particle that crosses the seam into its slab."""

    def drift(self, dt):
        before = self.img[:, 0].copy()
        super().drift(dt)
        hit = self.mine() & (self.img[:, 0] != before)
        self.img[hit, 0] = before[hit]


class MigrantVelocityLost(SlabStepper):
    """A migrant arrives with the content of a free slot (zero) for a velocity."""

    def drift(self, dt):
        was_mine = self.mine()
        super().drift(dt)
        self.v[self.mine() & ~was_mine] = 0.0


class StaleHalo(SlabStepper):
    """Its share's forces evaluated with the other slabs' particles where they were one step ago."""

    def drift(self, dt):
        self.x_prev = self.x.copy()
        super().drift(dt)

    def forces(self, x):
        f, u, w = super().forces(x)
        m = self.mine(x)
        xs = x.copy()
        xs[~m] = self.x_prev[~m]
        f[m] = self.brute(xs)[0][m]
        return f, u, w


class LocalKScale(SlabStepper):
    """Under NVT its share is rescaled with the scale formed from its local K."""

    def run(self, nsteps, dt, ensemble=sa.NVE, tau=0.0, nf=None, ktemp=None, r1=None, r2=None, thermo=True):
        u = w = 0.0
        for t in range(nsteps):
            self.drift(dt)
            self.f, u, w = self.forces(self.x)
            self.o.integrate_second_half(self.v, self.f, dt)
            if ensemble == sa.NVT:
                m = self.mine()
                vm = np.ascontiguousarray(self.v[m])
                self.o.bussi(vm, float(ktemp[t]), nf, dt, tau, float(r1[t]), float(r2[t]))
                self.o.bussi(self.v, float(ktemp[t]), nf, dt, tau, float(r1[t]), float(r2[t]))
                self.v[m] = vm
            self.step += 1
        return (u, w, self.o.kinetic(self.v)) if thermo else None


class Raises(SlabStepper):
    def run(self, *a, **kw):
        raise RuntimeError("follower sabotage: this rank fails inside run")


SABOTAGE = {c.__name__: c for c in (DroppedPair, CrossEnergyTwice, SeamImageKept, MigrantVelocityLost, StaleHalo,
                                    LocalKScale, Raises)}


class ModelSlab:
    """What the worker uses of a DomainDevice, on the CPU (see the module docstring)."""

    def __init__(self, case, world, path):
        import torch.distributed as dist
        from oracle import oracle as orc
        self.dist, self.rank, self.world = dist, dist.get_rank(), world
        s = case["system"]
        name, _, bad = os.environ.get("SLAB_SABOTAGE", "").partition(":")
        cls = SABOTAGE[name] if name and int(bad) == self.rank else SlabStepper
        self.st = cls(orc, s["box"], case["cutoff"], orc.make_pot(case["kind"], case["params"]))
        self.st.rank, self.st.world, self.st.Lx = self.rank, world, float(s["box"][0])
        self.builds = self.violations = 0

    def close(self):
        pass

    def upload_global(self, x, v, f, images, diameters):
        self.st.upload(x, v, f, images, diameters)

    def stats(self):
        return self.st.stats()

    def counts(self):
        return dict(n_own=int(self.st.mine().sum()))

    def run(self, nsteps, dt, ensemble=sa.NVE, tau=0.0, nf=None, ktemp=None, r1=None, r2=None, thermo=True):
        import torch
        st = self.st
        uwk = st.run(nsteps, dt, ensemble, tau, nf, ktemp, r1, r2, thermo=True)
        shares = [None] * self.world
        self.dist.all_gather_object(shares, (np.flatnonzero(st.mine()), st.x, st.v, st.f, st.img))
        x, v, f, img = (a.copy() for a in shares[0][1:])
        for ids, x_, v_, f_, im_ in reversed(shares):
            x[ids], v[ids], f[ids], img[ids] = x_[ids], v_[ids], f_[ids], im_[ids]
        st.x, st.v, st.f, st.img = x, v, f, img
        t = torch.tensor(uwk, dtype=torch.float64)
        self.dist.all_reduce(t)
        return tuple((t / self.world).tolist()) if thermo else None

    run_async = run_native = run

    def gather_global(self):
        return self.st.download()

    def download_local(self):
        return (np.flatnonzero(self.st.mine()),)


def model_factory(case, world, path):
    return ModelSlab(case, world, path)


# ---------------------------------------------------------------------------------------------
# the tests
# ---------------------------------------------------------------------------------------------
def _run(tmp_path, world, cases, port, schedule="MIXED", nvt=0, sabotage="", path="sync", timeout=150):
    env = {"SLAB_CASES": ",".join(cases), "SLAB_PATH": path, "SLAB_NVT": str(nvt), "SLAB_SCHEDULE": schedule,
           "SLAB_OUT": str(tmp_path), "SLAB_FACTORY": FACTORY, "SLAB_SABOTAGE": sabotage, "DOM_BACKEND": "gloo",
           "SLAB_WATCHDOG": str(timeout - 20)}
    rc, out, err = launch(world, env, port, timeout)
    assert rc == 0, err[-3000:]
    res = {}
    for c in cases:
        with open(os.path.join(str(tmp_path), c + ".json")) as fh:
            res[c] = json.load(fh)
    return res


@pytest.mark.parametrize("world,schedule,nvt,path", [(2, "MIXED", 0, "sync"), (3, "ONES", 1, "async-prune"),
                                                     (3, "MIXED", 1, "native-prune"), (2, "ONES", 0, "sync")])
def test_clean_model_passes(tmp_path, world, schedule, nvt, path):
    """The unsabotaged model: no failure, nothing excluded, particles change owner across an interior face and across the
    seam within the schedule (what the device module's coverage assertions rely on)."""
    res = _run(tmp_path, world, ["blob", "lj_2d"], 29700 + 10 * world + nvt + (5 if schedule == "ONES" else 0),
               schedule=schedule, nvt=nvt, path=path)
    for name, r in res.items():
        print(sa.margins_line("%s/%s/%d" % (name, schedule, world), r))
        assert r["failures"] == [], r["failures"][:3]
        assert r["excluded"] == [] and r["image_exceptions"] == []
        assert max(r["worst"][k] for k in ("F", "x1", "v1", "x", "v")) == 0.0, r["worst"]
        assert max(r["worst"][k] for k in ("U", "W", "K")) <= 1e-3, r["worst"]       # (the mean over the ranks rounds)
        assert len(r["segments"]) == len(sa.MIXED if schedule == "MIXED" else sa.ONES)
        print("    face moves %d, seam moves %d" % (r["face_moves"], r["seam_moves"]))
        if schedule == "MIXED":
            assert r["face_moves"] >= 1 and r["seam_moves"] >= 1, (r["face_moves"], r["seam_moves"])
        assert sum(r["n_own"]) == r["n"]


@pytest.mark.parametrize("sabotage,rank,nvt,check,what", [
    ("DroppedPair", 1, 0, "A", "F"),
    ("CrossEnergyTwice", 1, 0, "A", "U"),
    ("SeamImageKept", 0, 0, "B", "img"),
    ("MigrantVelocityLost", 1, 0, "B", "v"),
    ("StaleHalo", 1, 0, "A", "F"),
    ("LocalKScale", 1, 1, "B", "v"),
])
def test_sabotaged_rank_fails_the_audit(tmp_path, sabotage, rank, nvt, check, what):
    """One rank of two or three carries one slab fault; the leader's audit names it."""
    world = 3 if sabotage in ("StaleHalo", "SeamImageKept") else 2
    res = _run(tmp_path, world, ["blob"], 29760 + sorted(SABOTAGE).index(sabotage), nvt=nvt,
               sabotage="%s:%d" % (sabotage, rank))["blob"]
    heads = {f.split(":")[0] for f in res["failures"]}
    assert "(%s) %s" % (check, what) in heads, (sorted(heads), res["failures"][:4])
    if sabotage in ("DroppedPair", "StaleHalo", "CrossEnergyTwice"):
        # seen by force completeness at the very first segment, before anything has aged
        assert res["failures"][0].startswith("(%s) %s: segment 0 " % (check, what)), res["failures"][0]
    if sabotage == "SeamImageKept":
        assert "(A) F" not in heads and "(B) v" not in heads, sorted(heads)     # the state is otherwise whole


def test_a_follower_that_raises_ends_the_job(tmp_path):
    """Rank 1 raises inside run while rank 0 waits for it in a collective: the launcher ends the job with a non-zero
    status well inside the time limit, and no record is written."""
    env = {"SLAB_CASES": "blob", "SLAB_PATH": "sync", "SLAB_OUT": str(tmp_path), "SLAB_FACTORY": FACTORY,
           "SLAB_SABOTAGE": "Raises:1", "DOM_BACKEND": "gloo", "SLAB_WATCHDOG": "100"}
    t0 = time.time()
    rc, out, err = launch(2, env, 29790, 120, check=False)
    assert rc != 0 and "follower sabotage" in err, err[-2000:]
    assert time.time() - t0 < 90 and "dump_traceback" not in err
    assert not os.path.exists(os.path.join(str(tmp_path), "blob.json"))


# ---------------------------------------------------------------------------------------------
# thermo= on the three run methods: the argument plumbing, on a recording stand-in for the library
# ---------------------------------------------------------------------------------------------
NOVIOL = 0x7FFFFFFF


class _Recorder:
    """Every entry point returns 0 and is logged as (name, args); the ones that report through pointers fill them in."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            if name == "md_dom_step_begin":
                args[2]._obj.value = 0
            if name == "md_dom_run_window":
                args[12]._obj.value = NOVIOL
                args[13][0], args[13][1], args[13][2] = 1.0, 2.0, 3.0
                args[14][6] = 2.0
            if name == "md_dom_async_end":
                args[2]._obj.value = NOVIOL
                args[3][0], args[3][1], args[3][2] = 1.0, 2.0, 3.0
            if name in ("md_dom_step_end", "md_dom_forces"):
                args[-1][0], args[-1][1], args[-1][2] = 1.0, 2.0, 3.0
            return 0
        return fn

    def args_of(self, name):
        return [a for n, a in self.calls if n == name]


def _plumbing_device():
    from moleculardynamics.jl_amd.domain import DomainDevice
    lib = _Recorder()
    reduced = []

    class _Buf(list):
        def data_ptr(self):
            return 0

    class _Ex:
        on_device = True
        torch = types.SimpleNamespace(cuda=types.SimpleNamespace(stream=lambda s: contextlib.nullcontext()))

        def allreduce(self, vals, op="sum"):
            reduced.append(("host", len(vals)))
            return list(vals)

        def allreduce_async(self, vals, op="sum"):
            return lambda: float(vals[0])

        def allreduce_dev(self, t, op="sum"):
            reduced.append(("dev", op))

        def sendrecv_dev(self, *a):
            pass

    d = object.__new__(DomainDevice)
    d.dim, d.n_global, d._h, d._L, d.ex = 3, 1000, None, lib, _Ex()
    d.builds, d.violations, d.steps_since_build, d.target_interval = 1, 0, 0, 1000
    d._nsend_halo = d._nrecv_halo = (0, 0)
    d._exchange_fixed = lambda *a, **k: None
    d._native_ready = True
    d._flag, d._kuw, d._stream, d._zbufs = _Buf(), _Buf(), None, [_Buf()] * 4
    return d, lib, reduced


@pytest.mark.parametrize("nvt", [False, True])
@pytest.mark.parametrize("thermo", [True, False])
def test_thermo_keyword_reaches_the_library(thermo, nvt):
    """thermo=False: want_uw is 0 on the last step of run (md_dom_step_end) and run_async (md_dom_step_b, md_dom_step_c),
    report_last is 0 in md_dom_run_window while apply_pending_scale keeps its value, None is returned, and under NVT the
    K all-reduce still happens on every step.  thermo=True (the default) asks for U and W on the last step only."""
    from moleculardynamics.jl_amd import _lib
    n = 5
    kw = dict(ensemble=_lib.MD_NVT, tau=0.1, ktemp=np.ones(n), r1=np.zeros(n), r2=np.full(n, 2997.0)) if nvt else {}
    extra = {} if thermo else {"thermo": False}
    want_last = 1 if thermo else 0

    d, lib, red = _plumbing_device()
    out = d.run(n, 0.001, **kw, **extra)
    assert [a[2] for a in lib.args_of("md_dom_step_end")] == [0] * (n - 1) + [want_last]
    assert (out[:2] == (1.0, 2.0)) if thermo else (out is None)
    assert len(red) == (n if nvt else want_last)
    assert len(lib.args_of("md_scale_velocities")) == (1 if nvt else 0)      # the state stays downloadable

    d, lib, red = _plumbing_device()
    out = d.run_native(n, 0.001, **kw, **extra)
    (w,) = lib.args_of("md_dom_run_window")
    assert (w[1], w[9], w[10]) == (n, want_last, 1)                          # report_last, apply_pending_scale
    assert (out == (1.0, 2.0, 3.0)) if thermo else (out is None)

    d, lib, red = _plumbing_device()
    out = d.run_async(n, 0.001, **kw, **extra)
    assert [a[3] for a in lib.args_of("md_dom_step_b")] == [0] * (n - 1) + [want_last]
    assert [a[2] for a in lib.args_of("md_dom_step_c")] == ([want_last] if (nvt or thermo) else [])
    assert red.count(("dev", "sum")) == (n if nvt else want_last)
    assert [a[1] for a in lib.args_of("md_dom_async_end")] == [1]
    assert (out == (1.0, 2.0, 3.0)) if thermo else (out is None)


def test_last_step_redo_leaves_no_pending_scale():
    """What the device audit found (async-prune, NVT, three ranks): a run whose LAST step is redone through the classic
    violation branch applies that step's Bussi scale with md_scale_velocities, while the window's scale word still holds
    the scale the violating drift consumed -- the next run's first kick-drift applied it again (|dv| = 4.5e-2 on the
    following one-step segment).  The branch now ends with md_dom_set_scale(1.0); a violation at an earlier step still
    leaves its scale pending for the next kick-drift."""
    from moleculardynamics.jl_amd import _lib
    n = 4
    for viol_at in (n - 1, 1):
        d, lib, red = _plumbing_device()
        d.build = lambda: None
        state = {"first": True}

        def window(wlen, dt, ensemble, tau, nf, arrs, nvt, ends_run, prune_interval, fv, uwk, info):
            info[6] = 0.0                                    # a classic window
            fv.value = viol_at if state.pop("first", False) else NOVIOL
            uwk[0], uwk[1], uwk[2] = 1.0, 2.0, 3.0

        d._run_planned(window, n, 0.001, _lib.MD_NVT, 0.1, None, np.ones(n), np.zeros(n), np.full(n, 2997.0))
        tail = [(name, a[1]) for name, a in lib.calls if name in ("md_scale_velocities", "md_dom_set_scale")]
        if viol_at == n - 1:
            assert [t[0] for t in tail] == ["md_scale_velocities", "md_dom_set_scale"] and tail[1][1] == 1.0, tail
        else:
            assert [t[0] for t in tail] == ["md_dom_set_scale"] and tail[0][1] != 1.0, tail
