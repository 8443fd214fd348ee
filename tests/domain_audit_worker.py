"""Worker of the slab audit (tests/test_gpu_slab_audit.py on the device, tests/test_slab_audit.py on a CPU model): the
stepper interface of tests/step_audit.py on top of the real multi-process slab run.

Launched as tests/domain_gpu_worker.py is (torch.distributed.run, gloo, MDHIP_DOM_STAGE=device, all ranks on GPU 0,
tests/shim/libncclshim.so for the native loop; or one rank on the real RCCL).  Rank 0 runs step_audit.audit_run on a
LeaderStepper whose upload / run / download broadcast a command tuple; every rank, rank 0 included, then executes it on
its DomainDevice (upload_global with builds = 0; run, run_async or run_native; gather_global).  The other ranks loop on
commands until `quit`, which rank 0 sends from a `finally`.  stats() takes the prune count as the largest over the ranks' handles.  A rank that raises exits non-zero without waiting for anyone:
the launcher ends its peers.

Environment: SLAB_CASES (comma list of build_slab_case names), SLAB_PATH (sync | async-prune | native-prune), SLAB_NVT,
SLAB_SCHEDULE (MIXED | ONES), SLAB_OUT (directory: one <case>.json each), SLAB_FACTORY ("module:function", a replacement
for device_factory -- the CPU model), SLAB_WATCHDOG (seconds), SLAB_INNER_STEPS and SLAB_SKIN (see build_slab_case), DOM_BACKEND.
"""
import importlib
import json
import os
import signal
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LJ = [1.0, 1.0, 2.5]
PHS3_KT = 6.0
RUNNERS = {"sync": "run", "async-prune": "run_async", "native-prune": "run_native"}


# ---------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------
def elongated_liquid(world, kT=2.0):
    """One cube of the lj_diam liquid per rank, the box `world` cubes long in x (the geometry DOM_ELONG builds in
    tests/domain_gpu_worker.py).  1000 particles per cube with two ranks; 686 with three, which keeps the brute-force
    oracle's N at about 2000 (the cube's 9.14 then clips the skin to 0.546)."""
    from moleculardynamics.jl_amd import initialize_velocities, lattice_positions
    from tests.util import with_diameters
    per = 1000 if world <= 2 else 686
    n = per * world
    L1 = (per / 0.897) ** (1.0 / 3.0)
    parts = []
    for r in range(world):
        xr = lattice_positions(per, np.full(3, L1), 3, np.random.default_rng(100 + r))
        xr[:, 0] += r * L1
        parts.append(xr)
    x = np.ascontiguousarray(np.concatenate(parts)[np.random.default_rng(777).permutation(n)])
    v = initialize_velocities(kT, np.random.default_rng(67890), n, 3)
    s = dict(n=n, dim=3, box=np.array([world * L1, L1, L1]), x=x, v=v, f=np.zeros_like(x),
             img=np.zeros((n, 3), dtype=np.int32), diam=np.ones(n))
    return with_diameters(s, 0.9, 1.1)


def build_slab_case(name, world):
    """dict(system, kind, params, cutoff, dt[, skin, inner_skin]): tests/test_gpu_step_audit.py::build_case wherever the
    geometry fits (slab width >= 2 list cutoffs, y and z >= 3; the library clips the skin to what the slab leaves), the
    liquid cases that do not fit in the elongated box, and `void`, the crystallite of blob_gas_system() without its gas:
    with four ranks the slabs [0, 6) and [18, 24) own no particle."""
    c = _unshifted_case(name, world)
    # The slab planner (DomainDevice._plan) schedules a prune every max(2, floor(0.97 * 0.5 * inner / (1.1 * rate)) + 1)
    # steps, rate = the largest displacement per step.  build_case's inner skins are tuned to md_run's planner; here the
    # inner skin is three of the fastest particle's steps, which makes that interval 2 -- prune and ordinary steps
    # alternate, so both kinds and both thermo values land on the schedule's one-step segments.
    # SLAB_INNER_STEPS ("case=steps,..."): another multiple for a case whose one-step segments missed a kind with three.
    steps = dict(kv.split("=") for kv in os.environ.get("SLAB_INNER_STEPS", "").split(",") if kv)
    c["inner_skin"] = float(steps.get(name, 3.0)) * float(np.abs(c["system"]["v"]).max()) * c["dt"]
    skins = dict(kv.split("=") for kv in os.environ.get("SLAB_SKIN", "").split(",") if kv)
    if name in skins:                    # SLAB_SKIN ("case=skin,..."): another rebuild interval, so another phase
        c["skin"] = float(skins[name])
    shift = XSHIFT.get((name, world), 0.0)
    if shift:
        s = c["system"] = dict(c["system"])
        x = s["x"].copy()
        x[:, 0] = np.mod(x[:, 0] + shift, s["box"][0])
        x[:, 0][x[:, 0] >= s["box"][0]] = 0.0
        s["x"] = x
    return c


# Translations along x, (case, ranks) -> offset.  The liquids start from a jittered lattice and stay caged for the 79 steps
# of the schedule: where the seam or every interior face lies between two lattice planes no particle reaches it, and the
# audit would never see a migrant.  A translation is no change to the system (the box is periodic); each offset is the
# smallest of a fixed candidate list with which the CPU oracle's own trajectory, under every schedule and ensemble the
# device module runs the case with, has at least one particle change owner across an interior face and at least one cross
# the seam.  blob keeps |offset| <= 0.05: the face at x = 12 still cuts the crystallite's centre layer.
XSHIFT = {("blob", 2): 0.02, ("lj_diam_long", 2): 0.02, ("lj_2d", 3): -0.02, ("poly_2d", 3): -0.1, ("phs", 2): -0.4,
          ("phs_diam", 2): -0.4, ("phs", 3): 0.83, ("phs_diam", 3): 0.83, ("poly_3d", 2): -0.1, ("poly_3d", 3): -0.02}


def _unshifted_case(name, world):
    from tests.test_gpu_step_audit import build_case
    from tests.util import blob_gas_system, lj_system, with_diameters
    if name in ("phs", "phs_diam") and world >= 3:
        # slabs of 3.33 against lattice planes 1.25 apart: no translation brings a plane to the seam and one to a face, so
        # the particles have to travel the 0.2 themselves -- kT = 6 instead of 1.4737 (and XSHIFT puts both 0.21 away)
        c = build_case(name)
        s = lj_system(500, rho=0.5, kT=PHS3_KT)
        c["system"] = with_diameters(s, 0.9, 1.05) if name == "phs_diam" else s
        return c
    if name == "lj_diam_long":
        return dict(system=elongated_liquid(world), kind=0, params=LJ, cutoff=2.5, dt=0.004)
    if name.startswith("ljmod"):
        mode = int(name[5:])
        return dict(system=elongated_liquid(world), kind=3, params=[1.0, 1.0, 2.5, float(mode), 2.0 if mode == 2 else 0.0],
                    cutoff=2.5, dt=0.004)
    if name == "void":
        s = blob_gas_system()
        d2 = ((s["x"] - 12.0) ** 2).max(axis=1)
        keep = np.flatnonzero(d2 <= (4 * 1.08 + 0.05) ** 2)          # the 9^3 crystallite: |x - 12|inf <= 4.32 + jitter
        assert keep.size == 729
        out = dict(n=729, dim=3, box=s["box"])
        for key in ("x", "v", "f", "img", "diam"):
            out[key] = np.ascontiguousarray(s[key][keep])
        return dict(system=out, kind=0, params=LJ, cutoff=2.5, dt=0.004)
    return build_case(name)


def device_factory(case, world, path):
    """The real thing: a DomainDevice on GPU 0, configured for the case."""
    from moleculardynamics.jl_amd.domain import DomainDevice, Exchanger
    global _EXCHANGER
    if _EXCHANGER is None:
        _EXCHANGER = Exchanger(device_index=0)
    s = case["system"]
    d = DomainDevice(s["dim"], s["n"], s["box"], case["cutoff"], _EXCHANGER, device_id=0)
    d.set_potential(case["kind"], case["params"])
    if path.endswith("prune"):
        d.enable_pruning(skin=case.get("skin") or 0.6, inner_skin=case.get("inner_skin") or 0.16)
    elif case.get("skin") is not None:
        d.set_skin(case["skin"])
    return d


_EXCHANGER = None


# ---------------------------------------------------------------------------------------------
# the command protocol
# ---------------------------------------------------------------------------------------------
class Ranks:
    """What every rank holds: the device of the current case and how to execute a command on it."""

    def __init__(self, dist, factory, path):
        self.dist, self.factory, self.path = dist, factory, path
        self.rank, self.world = dist.get_rank(), dist.get_world_size()
        self.dev = None

    def command(self, cmd=None):
        """Rank 0 passes the command; the others receive it.  Every rank executes it and returns (cmd, result)."""
        box = [cmd]
        self.dist.broadcast_object_list(box, src=0)
        cmd = box[0]
        return cmd, getattr(self, "do_" + cmd[0])(*cmd[1:])

    def do_case(self, name):
        self.do_close()
        self.case = build_slab_case(name, self.world)
        self.dev = self.factory(self.case, self.world, self.path)

    def do_close(self):
        if self.dev is not None:
            self.dist.barrier()          # nobody frees a mailbox a peer may still write to
            self.dev.close()
            self.dev = None
            self.dist.barrier()

    def do_upload(self, x, v, f, img, diam):
        self.dev.upload_global(x, v, f, img, diam)
        self.dev.builds = 0

    def do_run(self, k, dt, thermo, kw):
        return getattr(self.dev, RUNNERS[self.path])(k, dt, thermo=thermo, **kw)

    def do_download(self):
        """(gather_global's state, the ids every rank's handle holds): the second says where the DEVICE keeps a particle."""
        held = [None] * self.world
        self.dist.all_gather_object(held, np.asarray(self.dev.download_local()[0]))
        return self.dev.gather_global(), held

    def do_stats(self):
        """(prunes, inner rows in use) of every rank's handle: the leader's own slab may own no particle."""
        out = [None] * self.world
        self.dist.all_gather_object(out, (int(self.dev.stats()["prunes"]), bool(self.dev.counts().get("pruning", False))))
        return out

    def do_counts(self):
        out = [None] * self.world
        self.dist.all_gather_object(out, self.dev.counts())
        return out

    def do_quit(self):
        self.do_close()


class LeaderStepper:
    """upload / run / download / stats for audit_run, on rank 0; also keeps the slab coverage from the gathered states."""

    def __init__(self, ranks, Lx):
        self.r, self.Lx = ranks, float(Lx)
        self.prev = None
        self.face_moves = self.seam_moves = 0
        self.owned_min = self.owned_max = None
        # what the device did about it: a particle changes HANDLE only at a list build (migrate pack / unpack)
        self.held = self.held_img = None
        self.face_migrations = self.seam_migrations = 0

    def upload(self, x, v, f, images, diameters):
        self.r.command(("upload", x, v, f, images, diameters))
        self.prev = self.held = None

    def run(self, k, dt, thermo=True, **kw):
        return self.r.command(("run", int(k), float(dt), bool(thermo), kw))[1]

    def download(self):
        from moleculardynamics.jl_amd.domain import owner_of
        (X, V, F, IM), ids = self.r.command(("download",))[1]
        held = np.empty(len(X), dtype=np.int64)
        for rank, i in enumerate(ids):
            held[i] = rank
        if self.held is None:
            self.held_img = IM[:, 0].copy()
        else:
            moved = held != self.held                     # migrated since the last download; through the seam if the x
            seam = moved & (IM[:, 0] != self.held_img)    # image counter differs from the one it last changed handle with
            self.seam_migrations += int(seam.sum())
            self.face_migrations += int((moved & ~seam).sum())
            self.held_img[moved] = IM[moved, 0]
        self.held = held
        own = owner_of(X[:, 0], self.Lx, self.r.world)
        if self.prev is not None:
            own0, imx0 = self.prev
            seam = IM[:, 0] != imx0                       # the x image counter changes at the seam and nowhere else
            self.seam_moves += int(seam.sum())
            self.face_moves += int(((own != own0) & ~seam).sum())
        self.prev = (own, IM[:, 0].copy())
        cnt = np.bincount(own, minlength=self.r.world)
        self.owned_min = cnt if self.owned_min is None else np.minimum(self.owned_min, cnt)
        self.owned_max = cnt if self.owned_max is None else np.maximum(self.owned_max, cnt)
        return X, V, F, IM

    def stats(self):
        d = self.r.dev
        per_rank = self.r.command(("stats",))[1]
        return dict(prunes=max(p for p, _ in per_rank), pruning=[on for _, on in per_rank],
                    rebuilds=int(d.builds), violations=int(d.violations),
                    windows=int(getattr(d, "windows", 0)), fused_windows=int(getattr(d, "fused_windows", 0)),
                    direct_windows=int(getattr(d, "direct_windows", 0)), counts=d.counts())


def audit_case(ranks, name, schedule, nvt):
    """Rank 0: audit_run of one case on the leader stepper -> the JSON-ready record."""
    from oracle import oracle as orc
    from tests import step_audit as sa
    ranks.command(("case", name))
    c = ranks.case
    s = c["system"]
    kw = {}
    if nvt:
        from moleculardynamics.jl_amd.thermostat import draw_bussi
        total = sum(schedule)
        nf = s["dim"] * (s["n"] - 1.0)
        r1, r2 = draw_bussi(nf, np.random.default_rng(17), total)
        kT = 2.0 * float(orc.kinetic(s["v"])) / nf
        kw = dict(ensemble=sa.NVT, tau=0.1, ktemp=np.full(total, kT), r1=r1, r2=r2)
    stepper = LeaderStepper(ranks, s["box"][0])
    res = sa.audit_run(stepper, orc, s, orc.make_pot(c["kind"], c["params"]), c["cutoff"], c["dt"], schedule,
                       raise_on_failure=False, **kw)
    rank_counts = ranks.command(("counts",))[1]
    return dict(case=name, world=ranks.world, n=int(s["n"]), worst=res["worst"], segments=res["segments"],
                excluded=res["excluded"], image_exceptions=res["image_exceptions"],
                failures=[str(f) for f in res["failures"]], stats=res["stats"],
                face_moves=stepper.face_moves, seam_moves=stepper.seam_moves,
                face_migrations=stepper.face_migrations, seam_migrations=stepper.seam_migrations,
                owned_min=stepper.owned_min.tolist(), owned_max=stepper.owned_max.tolist(),
                n_own=[int(rc["n_own"]) for rc in rank_counts])


def main():
    # a rank stuck in a collective (its peer failed, or the ranks disagree about what comes next) says where, and ends
    import faulthandler
    faulthandler.dump_traceback_later(float(os.environ.get("SLAB_WATCHDOG", "100")), exit=True)
    import torch.distributed as dist
    from tests import step_audit as sa

    backend = os.environ.get("DOM_BACKEND", "gloo")
    if backend == "nccl":
        import torch
        torch.cuda.set_device(0)
    dist.init_process_group(backend=backend)
    factory = device_factory
    if os.environ.get("SLAB_FACTORY"):
        mod, fn = os.environ["SLAB_FACTORY"].split(":")
        factory = getattr(importlib.import_module(mod), fn)
    ranks = Ranks(dist, factory, os.environ.get("SLAB_PATH", "sync"))
    if ranks.rank == 0:
        schedule = {"MIXED": sa.MIXED, "ONES": sa.ONES}[os.environ.get("SLAB_SCHEDULE", "MIXED")]
        failed = True
        try:
            for name in os.environ["SLAB_CASES"].split(","):
                rec = audit_case(ranks, name, schedule, os.environ.get("SLAB_NVT", "0") == "1")
                with open(os.path.join(os.environ["SLAB_OUT"], name + ".json"), "w") as fh:
                    json.dump(rec, fh)
            failed = False
        finally:
            try:
                ranks.command(("quit",))        # an exception in the audit releases the peers
            except Exception:
                if not failed:                  # (after a failure the first exception is the one to report)
                    raise
    else:
        while ranks.command()[0][0] != "quit":
            pass
    dist.destroy_process_group()


# ---------------------------------------------------------------------------------------------
# the launcher (the parent side; the process-group kill of tests/test_domain_gpu.py::_launch)
# ---------------------------------------------------------------------------------------------
def launch(nproc, env_extra, port, timeout, check=True):
    """Runs the worker under torch.distributed.run in a process group of its own: ranks stuck in a collective are ended
    with the launcher when the time limit runs out (subprocess.TimeoutExpired is raised: a hang, not a failing test).
    Returns (returncode, stdout, stderr)."""
    env = dict(os.environ)
    env.update(env_extra)
    env["OMP_NUM_THREADS"] = "2"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)]
    p = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, start_new_session=True)
    try:
        out, err = p.communicate(timeout=timeout)
    except subprocess.TimeoutExpired:
        os.killpg(p.pid, signal.SIGKILL)
        out, err = p.communicate()
        sys.stdout.write(out[-3000:])
        sys.stderr.write(err[-3000:])
        raise
    if check and p.returncode != 0:
        sys.stdout.write(out[-3000:])
        sys.stderr.write(err[-3000:])
    return p.returncode, out, err


if __name__ == "__main__":
    main()
