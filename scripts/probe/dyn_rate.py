"""Time the device self-dynamics sampler (md_dyn_*) on the bench system: N = 2^20 LJ, rho = 0.897, d = 3, nq = 4,
400 van Hove bins, after a short equilibration -- one origin store, one sample at a short lag (nearly every d2 in bins
0-1) and at a long lag (after a run), and the same samples without the histogram and without wavenumbers.  Then a
run_simulation of `steps` steps three ways: with the default (log-time) dynamics schedule, with log_times=True and no
dynamics (the same stops), and with neither.  Prints one JSON line.
python scripts/probe/dyn_rate.py [N] [nsamples] [steps] [rounds]"""
import json
import math
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np

import moleculardynamics.jl_amd as md
from moleculardynamics.jl_amd import MDDevice, _lib, lattice_positions, initialize_velocities

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 20
nsamp = int(sys.argv[2]) if len(sys.argv) > 2 else 50
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 20000
rounds = int(sys.argv[4]) if len(sys.argv) > 4 else 2
rho, nbins, r_max = 0.897, 400, 4.0
q = [2.0 * math.pi, 4.0, 8.0, 12.0]
L = (n / rho) ** (1.0 / 3.0)
box = np.full(3, L)
x = lattice_positions(n, box, 3, np.random.default_rng(12345))
v = initialize_velocities(1.4737, np.random.default_rng(67890), n, 3)
out = dict(n=n, rho=rho, nq=len(q), nbins=nbins, r_max=r_max)


def timed(dev, fn, k):
    dev.dyn_read()                                   # waits for the stream
    t0 = time.perf_counter()
    for _ in range(k):
        fn()
    dev.dyn_read()
    return (time.perf_counter() - t0) * 1e3 / k


with MDDevice(3, n, box, 2.5) as dev:
    dev.set_potential(_lib.MD_POT_LJ, [1.0, 1.0, 2.5])
    dev.upload(x, v, np.zeros_like(x), np.zeros((n, 3), np.int32), np.ones(n))
    dev.run(200, 0.001)
    res = {}
    for label, qq, nb in (("full", q, nbins), ("no_hist", q, 0), ("no_q", [], nbins), ("bare", [], 0)):
        dev.dyn_setup(1, 2, qq, r_max, nb)
        dev.dyn_origin(0)
        dev.run(5, 0.001)                            # a short lag: d2 ~ 1e-5, bins 0-1
        for _ in range(3):
            dev.dyn_sample([0], [0])
        r = dict(origin_ms=timed(dev, lambda: dev.dyn_origin(0), nsamp))
        dev.run(5, 0.001)
        r["sample_short_ms"] = timed(dev, lambda: dev.dyn_sample([0], [0]), nsamp)
        r["sample_batch4_ms"] = timed(dev, lambda: dev.dyn_sample([0] * 4, [0, 1, 0, 1]), nsamp // 2) / 4
        ns, sums, hist = dev.dyn_read()
        r["msd_short"] = float(sums[0, 0] / (n * ns[0]))
        if nb:
            r["short_bins01_frac"] = float(hist[0, :2].sum() / hist[0].sum())
        res[label] = r
    # a long lag: 2 000 steps of dt = 0.005 (q |del| up to ~10^1-10^2 rad here; the cos cost does not depend on it below
    # 2^30 rad, the branch point of ocml's fp64 range reduction)
    dev.dyn_setup(1, 1, q, r_max, nbins)
    dev.dyn_origin(0)
    dev.run(2000, 0.005)
    res["full"]["sample_long_ms"] = timed(dev, lambda: dev.dyn_sample([0], [0]), nsamp)
    ns, sums, hist = dev.dyn_read()
    res["full"]["msd_long"] = float(sums[0, 0] / (n * ns[0]))
    res["full"]["long_bins01_frac"] = float(hist[0, :2].sum() / max(hist[0].sum(), 1))
    res["full"]["origin_long_ms"] = timed(dev, lambda: dev.dyn_origin(0), nsamp)   # (slots now far from id order)
    out["device"] = res
    # bytes one sample moves: k_export reads pos (32 B) + images (12 B) + id (4 B), writes x (24 B) + images (12 B); the
    # sample kernel reads both frames (2 x 36 B)
    out["sample_bytes"] = n * (32 + 12 + 4 + 36 + 72)
    out["origin_bytes"] = n * (32 + 12 + 4 + 36)
    xs = dev.download()[0]

# run_simulation three ways (NVE, thermo every 1000th step, no trajectory file), same start, alternated
params = md.Parameters(rho, n, 0.001, md.LennardJones())
walls = {}
with tempfile.TemporaryDirectory() as tmp:
    cwd = os.getcwd()
    os.chdir(tmp)                                    # (log_times writes new-log-times.txt into the working directory)
    try:
        for r in range(rounds):
            for label in ("dynamics", "log_times", "plain"):
                st = md.initialize_state(params, None, cutoff=2.5, positions=xs, diameters=np.ones(n), unitcell=L)
                st.velocities = v.copy()
                dyn = md.SelfDynamics(q=q) if label == "dynamics" else None
                t0 = time.perf_counter()
                md.run_simulation(st, params, md.NVE(), steps, 1000, os.path.join(tmp, label), write_trajectory=False,
                                  log_times=label == "log_times", dynamics=dyn)
                walls.setdefault(label, []).append(time.perf_counter() - t0)
                st.system.device.close()
                for f in os.listdir(os.path.join(tmp, label)):
                    if f.startswith("snapshot."):
                        os.remove(os.path.join(tmp, label, f))
    finally:
        os.chdir(cwd)
out["run_simulation"] = dict(steps=steps, frequency=1000, walls=walls, best={k: min(w) for k, w in walls.items()})
print(json.dumps(out), flush=True)
