"""Time a shear-flow run on the bench system: N = 2^20 LJ, rho = 0.897, d = 3, NVT, `steps` steps in segments of
`every`, three ways on ONE handle, alternated round by round (so that clock and thermal drift hit all three alike):
  nvt           no shear: md_run segments only
  deform_cell   after every segment the flow operator through md_deform_cell (F the simple shear of rate * every * dt,
                G = F^-1; the rows are kept) and md_compute_forces
  set_cell      the same cell change through md_set_cell(F U, AFFINE) (the lists are invalidated) and md_compute_forces;
                the velocities are not mapped on this path (md_set_cell leaves them), which costs it nothing
The two sheared ways are run at every rate of RATES.  Every way starts each round from the same uploaded frame in the same
(already sheared, general) cell, runs `every * 5` untimed steps, and is timed with device events on a stream handed to the
handle (md_set_stream) around the whole loop, host work included.  Also timed, whole calls, 20 each after 3:
deform_cell alone (to and fro by 1e-4), md_compute_forces on a valid list, and a device-to-device copy of the bytes the
pass moves per particle (pos 32 + x0 24 + x1 24 + v 24, read and written: 208), the ceiling it is compared with.  The
kernel's own time comes from a kernel trace of this script in a run of its own.  Prints one JSON line and writes it to `out`.
python scripts/probe/deform_rate.py [N] [steps] [every] [rounds] [out]"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np

from moleculardynamics.jl_amd import (LennardJones, MDDevice, _lib, initialize_velocities, lattice_positions,
                                      simple_shear)
from moleculardynamics.jl_amd.thermostat import draw_bussi

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 20
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
every = int(sys.argv[3]) if len(sys.argv) > 3 else 10
rounds = int(sys.argv[4]) if len(sys.argv) > 4 else 3
path = sys.argv[5] if len(sys.argv) > 5 else os.path.join(ROOT, "profiles", "deform_rate.txt")
rho, d, dt, kT, tau = 0.897, 3, 0.001, 1.4737, 0.1
L = (n / rho) ** (1.0 / 3.0)
U0 = np.eye(3) * L
U0[0, 1] = 0.05 * L                                                          # (general from the start: no transition build)
RATES = (1e-3, 1e-2, 1e-1)
x = lattice_positions(n, np.full(3, L), 3, np.random.default_rng(12345))
x[:, 0] += 0.05 * x[:, 1]                                                     # (the lattice sheared with its cell)
v = initialize_velocities(kT, np.random.default_rng(67890), n, 3)
pot = LennardJones()
nf = 3.0 * (n - 1.0)

try:
    hip = C.CDLL("libamdhip64.so")
except OSError:
    hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
vp = C.c_void_p


def hipchk(rc):
    if rc != 0:
        raise RuntimeError("HIP error %d" % rc)


class Events:
    def __init__(self, stream):
        self.stream, self.a, self.b = stream, vp(), vp()
        hipchk(hip.hipEventCreate(C.byref(self.a)))
        hipchk(hip.hipEventCreate(C.byref(self.b)))

    def time(self, call):
        hipchk(hip.hipEventRecord(self.a, self.stream))
        call()
        hipchk(hip.hipEventRecord(self.b, self.stream))
        hipchk(hip.hipEventSynchronize(self.b))
        ms = C.c_float()
        hipchk(hip.hipEventElapsedTime(C.byref(ms), self.a, self.b))
        return float(ms.value)


def summary(ms):
    a = np.sort(np.asarray(ms))
    return dict(median=float(np.median(a)), min=float(a[0]), max=float(a[-1]), n=len(a))


stream = vp()
hipchk(hip.hipStreamCreateWithFlags(C.byref(stream), 1))                      # hipStreamNonBlocking
out = dict(n=n, rho=rho, steps=steps, every=every, rounds=rounds, bytes_per_particle=208)
with MDDevice(3, n, U0, 2.5) as dev:
    hipchk(dev._L.md_set_stream(dev._h, stream))
    ev = Events(stream)
    dev.set_potential(_lib.MD_POT_LJ, [1.0, 1.0, 2.5])
    dev.upload(x, v, np.zeros_like(x), np.zeros((n, 3), np.int32), np.ones(n))
    dev.run(200, dt)
    x, v, f, img = dev.download()
    ones = np.ones(n)

    def loop(way, rate, nsteps, rng, info):
        dg = rate * every * dt
        F, G = simple_shear(3, dg), simple_shear(3, -dg)
        for a in range(0, nsteps, every):
            r1, r2 = draw_bussi(nf, rng, every)
            dev.run(every, dt, _lib.MD_NVT, tau, nf, np.full(every, kT), r1, r2)
            if way == "nvt":
                continue
            if way == "deform_cell":
                info["kept"] += dev.deform_cell(F, G)
            else:
                dev.set_cell(F @ dev.unitcell, dev.CELL_AFFINE)
            dev.compute_forces()
            info["couplings"] += 1

    ways = [("nvt", 0.0)] + [(w, r) for r in RATES for w in ("deform_cell", "set_cell")]
    key = lambda w, r: w if w == "nvt" else "%s@%g" % (w, r)
    res = {key(*w): [] for w in ways}
    counts = {key(*w): dict(kept=0, couplings=0, rebuilds=0, prunes=0) for w in ways}
    for r in range(rounds + 1):                                               # (round 0 is the warm-up of every kernel)
        for way, rate in ways:
            if not np.array_equal(dev.unitcell, U0):
                dev.set_cell(U0, dev.CELL_AFFINE)
            dev.upload(x, v, f, img, ones)
            rng = np.random.default_rng(100 + r)
            loop(way, rate, 5 * every, rng, dict(kept=0, couplings=0))
            before = dev.stats()
            info = counts[key(way, rate)] if r else dict(kept=0, couplings=0, rebuilds=0, prunes=0)
            ms = ev.time(lambda: loop(way, rate, steps, rng, info))
            after = dev.stats()
            info["rebuilds"] += after["rebuilds"] - before["rebuilds"]
            info["prunes"] += after["prunes"] - before["prunes"]
            if r:
                res[key(way, rate)].append(ms)
    # the call alone, and the copy ceiling for its bytes
    if not np.array_equal(dev.unitcell, U0):
        dev.set_cell(U0, dev.CELL_AFFINE)
    dev.upload(x, v, f, img, ones)
    dev.run(20, dt)
    flip = [0]

    def scale():
        flip[0] ^= 1
        g = 1e-4 if flip[0] else -1e-4
        dev.deform_cell(simple_shear(3, g), simple_shear(3, -g))

    call = [ev.time(scale) for _ in range(23)][3:]
    forces = [ev.time(dev.compute_forces) for _ in range(23)][3:]
    nbytes = 104 * n
    a, b = vp(), vp()
    hipchk(hip.hipMalloc(C.byref(a), C.c_size_t(nbytes)))
    hipchk(hip.hipMalloc(C.byref(b), C.c_size_t(nbytes)))
    copy = [ev.time(lambda: hipchk(hip.hipMemcpyAsync(b, a, C.c_size_t(nbytes), 3, stream))) for _ in range(23)][3:]
    hipchk(hip.hipFree(a))
    hipchk(hip.hipFree(b))

names = list(res)
out["loop_ms"] = {w: summary(res[w]) for w in names}
out["ms_per_step"] = {w: out["loop_ms"][w]["median"] / steps for w in names}
out["ratio_to_nvt"] = {w: out["loop_ms"][w]["median"] / out["loop_ms"]["nvt"]["median"] for w in names}
out["counts_over_timed_rounds"] = counts
out["kept_share"] = {w: counts[w]["kept"] / max(counts[w]["couplings"], 1) for w in names if w.startswith("deform_cell")}
out["call_ms"] = dict(deform_cell=summary(call), compute_forces_valid_list=summary(forces), copy_208B=summary(copy))
out["copy_GBps"] = 208.0 * n / out["call_ms"]["copy_208B"]["median"] * 1e-6
line = json.dumps(out)
print(line, flush=True)
os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
with open(path, "w") as fh:
    fh.write("scripts/probe/deform_rate.py %d %d %d %d (device events on the handle's stream around whole loops and whole "
             "calls, host work included; ms)\n%s\n" % (n, steps, every, rounds, line))
