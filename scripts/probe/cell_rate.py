"""Time the cell change of a live handle and what goes with it on the bench system: N = 2^20 LJ, rho = 0.897, d = 3, a
liquid after 200 steps.  Device events on a stream handed to the handle (md_set_stream), `warm` untimed calls, then `reps`
timed ones per item, the median and the spread reported (ms):
  set_cell_affine / set_cell_lattice   md_set_cell, the whole call (validation, grid, capacity, the pass, the wait); the
                                       lattice change flips a cell sheared to 0.7 to its reduced form and back
  mark / nonaffine / nonaffine_u       md_nonaffine_mark, md_nonaffine without and with the per-particle field
  first_forces                         md_compute_forces right after a cell change: the list build and the force pass
  forces                               md_compute_forces on a valid list, for scale
  step                                 one md_run step (from a run of 100), for scale
  increment_in_place                   one AQS increment on the handle: strain, `fire_steps` steps of FIRE (a tolerance it
                                       cannot reach, so both ways do the same work), stress, non-affine sums
  increment_fresh_handle               the same increment the old way: download, strain on the host, a new handle, upload,
                                       the same FIRE, stress; the old handle destroyed (host clock: it is host work)
and the bytes each pass moves per particle, from the record layout, against the copy ceiling measured by a
device-to-device copy of the same size.  The kernels' own times come from a kernel trace of this script (rocprofv3
--kernel-trace --stats -- python scripts/probe/cell_rate.py N 3 1 out).  Prints one JSON line and writes it to `out`
(default profiles/cell_rate.txt).
python scripts/probe/cell_rate.py [N] [reps] [warm] [out] [fire_steps]"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np

from moleculardynamics.jl_amd import MDDevice, _lib, gauss_reduce, initialize_velocities, lattice_positions, simple_shear

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 20
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
warm = int(sys.argv[3]) if len(sys.argv) > 3 else 3
path = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "cell_rate.txt")
fire_steps = int(sys.argv[5]) if len(sys.argv) > 5 else 100
rho, d = 0.897, 3
L = (n / rho) ** (1.0 / 3.0)
U0 = np.eye(3) * L
x = lattice_positions(n, np.full(3, L), 3, np.random.default_rng(12345))
v = initialize_velocities(1.4737, np.random.default_rng(67890), n, 3)
LJ = [1.0, 1.0, 2.5]
FIRE = dict(max_steps=fire_steps, tol=1e-300, dt_initial=0.002, dt_max=0.02)

try:
    hip = C.CDLL("libamdhip64.so")
except OSError:
    hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
vp = C.c_void_p


def hipchk(rc):
    if rc != 0:
        raise RuntimeError("HIP error %d" % rc)


class Events:
    """Two device events on the handle's stream around a call; elapsed ms after the second has completed."""

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


def series(ev, call, before=None):
    out = []
    for k in range(warm + reps):
        if before is not None:
            before()
        ms = ev.time(call)
        if k >= warm:
            out.append(ms)
    return out


def summary(ms):
    a = np.sort(np.asarray(ms))
    return dict(median=float(np.median(a)), min=float(a[0]), max=float(a[-1]), n=len(a))


# bytes per particle, d = 3, from the record layout (pos double4, img 3 x int32, id int32, mark 3 x (double + int32))
BYTES = dict(set_cell_affine=32 + 32 + 12 + 12, set_cell_lattice=32 + 4 + 12 + 12 + 2 * 36, mark=32 + 4 + 12 + 36,
             nonaffine=32 + 4 + 12 + 36, nonaffine_u=32 + 4 + 12 + 36 + 24)
out = dict(n=n, rho=rho, reps=reps, warm=warm, fire_steps=fire_steps, bytes_per_particle=BYTES)

stream = vp()
hipchk(hip.hipStreamCreateWithFlags(C.byref(stream), 1))                      # hipStreamNonBlocking
with MDDevice(3, n, U0, 2.5) as dev:
    hipchk(dev._L.md_set_stream(dev._h, stream))
    ev = Events(stream)
    dev.set_potential(_lib.MD_POT_LJ, LJ)
    dev.upload(x, v, np.zeros_like(x), np.zeros((n, 3), np.int32), np.ones(n))
    dev.run(200, 0.001)
    dev.stress_setup(0)
    res = {}
    # the copy ceiling: a device-to-device copy of 88 bytes per particle each way's worth (read + write counted)
    nbytes = 44 * n
    a, b = vp(), vp()
    hipchk(hip.hipMalloc(C.byref(a), C.c_size_t(nbytes)))
    hipchk(hip.hipMalloc(C.byref(b), C.c_size_t(nbytes)))
    res["copy_88B"] = series(ev, lambda: hipchk(hip.hipMemcpyAsync(b, a, C.c_size_t(nbytes), 3, stream)))
    hipchk(hip.hipFree(a))
    hipchk(hip.hipFree(b))
    # the affine change: to and fro between the cube and a cell sheared by 1e-3
    U1 = simple_shear(3, 1e-3) @ U0
    flip = [0]

    def affine():
        flip[0] ^= 1
        dev.set_cell(U1 if flip[0] else U0, dev.CELL_AFFINE)

    res["set_cell_affine"] = series(ev, affine)
    if flip[0]:
        affine()
    res["forces"] = series(ev, dev.compute_forces, before=None)
    res["first_forces"] = series(ev, dev.compute_forces, before=affine)
    if flip[0]:
        affine()
    # mark and non-affine sums
    res["mark"] = series(ev, dev.nonaffine_mark)
    res["nonaffine"] = series(ev, dev.nonaffine)
    res["nonaffine_u"] = series(ev, lambda: dev.nonaffine(fields=True))
    # the lattice change, with the mark carried along: sheared to 0.7, then reduced and back
    US = simple_shear(3, 0.7) @ U0
    W, M = gauss_reduce(US)
    dev.set_cell(US, dev.CELL_AFFINE)

    def lattice():
        flip[0] ^= 1
        dev.set_cell(W if flip[0] else US, dev.CELL_LATTICE)

    flip[0] = 0
    res["set_cell_lattice"] = series(ev, lattice)
    if flip[0]:
        lattice()
    dev.set_cell(U0, dev.CELL_AFFINE)
    t = ev.time(lambda: dev.run(100, 0.001))
    res["step"] = [t / 100.0]
    dev.compute_forces()
    # one increment in place
    state = dict(U=U0.copy())

    def increment():
        state["U"] = simple_shear(3, 1e-3) @ state["U"]
        dev.set_cell(state["U"], dev.CELL_AFFINE)
        dev.nonaffine_mark()
        dev.fire_minimize(**FIRE)
        dev.stress_sample()
        dev.stress_tensor()
        dev.nonaffine()

    inc_reps = max(3, reps // 4)
    res["increment_in_place"] = [ev.time(increment) for _ in range(1 + inc_reps)][1:]
    cell = state["U"]
    xs, _, _, ims = dev.download()
# the same increment the old way: every increment a new handle (host clock around synchronising calls)
fresh = []
cur = MDDevice(3, n, cell, 2.5)
cur.set_potential(_lib.MD_POT_LJ, LJ)
cur.upload(xs, np.zeros_like(xs), np.zeros_like(xs), ims, np.ones(n))
cur.compute_forces()
for k in range(1 + inc_reps):
    t0 = time.perf_counter()
    xd, _, _, imd = cur.download()
    F = simple_shear(3, 1e-3)
    cell = F @ cell
    xn = xd @ F.T
    nxt = MDDevice(3, n, cell, 2.5)
    nxt.set_potential(_lib.MD_POT_LJ, LJ)
    nxt.upload(xn, np.zeros_like(xn), np.zeros_like(xn), imd, np.ones(n))
    nxt.fire_minimize(**FIRE)
    nxt.stress_setup(0)
    nxt.stress_sample()
    nxt.stress_tensor()
    cur.close()
    cur = nxt
    if k:
        fresh.append((time.perf_counter() - t0) * 1e3)
cur.close()
res["increment_fresh_handle"] = fresh
out["ms"] = {k: summary(val) for k, val in res.items()}
copy_ms = out["ms"]["copy_88B"]["median"]
out["copy_GBps"] = 88.0 * n / copy_ms * 1e-6
out["call_GBps"] = {k: BYTES[k] * n / out["ms"][k]["median"] * 1e-6 for k in BYTES}
out["call_fraction_of_copy"] = {k: g / out["copy_GBps"] for k, g in out["call_GBps"].items()}
line = json.dumps(out)
print(line, flush=True)
os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
with open(path, "w") as fh:
    fh.write("scripts/probe/cell_rate.py %d %d %d (device events on the handle's stream, whole calls; ms)\n%s\n" % (n, reps, warm, line))
