"""Time the device pressure-tensor sampler (md_stress_*) on the bench system: N = 2^20 LJ, rho = 0.897, d = 3, after a short
equilibration -- one md_stress_sample beside one md_compute_forces on the same handle and box (both walk the outer rows;
md_compute_forces also waits and reads its scalars back, so its figure is per synchronised call), synchronised wall clock
over `nsamples` calls, `rounds` times alternated.  With MDHIP_NO_TILES=1 in the environment it times the global-gather twin.
Prints one JSON line.
python scripts/probe/stress_rate.py [N] [nsamples] [rounds] [nlags]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np

from moleculardynamics.jl_amd import MDDevice, _lib, lattice_positions, initialize_velocities

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 20
nsamp = int(sys.argv[2]) if len(sys.argv) > 2 else 50
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
nlags = int(sys.argv[4]) if len(sys.argv) > 4 else 1000
rho = 0.897
L = (n / rho) ** (1.0 / 3.0)
box = np.full(3, L)
x = lattice_positions(n, box, 3, np.random.default_rng(12345))
v = initialize_velocities(1.4737, np.random.default_rng(67890), n, 3)
out = dict(n=n, rho=rho, nlags=nlags, nsamples=nsamp)

with MDDevice(3, n, box, 2.5) as dev:
    dev.set_potential(_lib.MD_POT_LJ, [1.0, 1.0, 2.5])
    dev.upload(x, v, np.zeros_like(x), np.zeros((n, 3), np.int32), np.ones(n))
    dev.run(200, 0.001)
    dev.stress_setup(nlags)
    for _ in range(3):
        dev.stress_sample()
        dev.compute_forces()
    res = dict(sample_ms=[], sample_sync_ms=[], compute_forces_ms=[])
    for _ in range(rounds):
        dev.stress_read()                                # waits for the stream
        t0 = time.perf_counter()
        for _ in range(nsamp):
            dev.stress_sample()
        dev.stress_read()
        res["sample_ms"].append((time.perf_counter() - t0) * 1e3 / nsamp)
        t0 = time.perf_counter()
        for _ in range(nsamp):
            dev.stress_sample()
            dev.stress_tensor()                          # a wait per call, as md_compute_forces has
        res["sample_sync_ms"].append((time.perf_counter() - t0) * 1e3 / nsamp)
        t0 = time.perf_counter()
        for _ in range(nsamp):
            dev.compute_forces()
        res["compute_forces_ms"].append((time.perf_counter() - t0) * 1e3 / nsamp)
    kin, vir = dev.stress_tensor()
    _, w = dev.compute_forces()
    st = dev.stats()
    out.update(res)
    out["best"] = {k: min(val) for k, val in res.items()}
    out["ratio_sync"] = out["best"]["sample_sync_ms"] / out["best"]["compute_forces_ms"]
    out["tiled"] = st["tiled"]
    out["walked_outer"] = st["walked_outer"]
    out["trace_minus_W_rel"] = float(abs((vir[0] + vir[1]) + vir[2] - w) / abs(w))
    out["pressure"] = float((kin[:3].sum() + vir[:3].sum()) / (3.0 * L ** 3))
print(json.dumps(out), flush=True)
