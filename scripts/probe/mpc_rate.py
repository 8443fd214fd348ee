"""Time the device marked-pair-correlation sampler (md_mpc_*) on the bench system: N = 2^20 LJ, rho = 0.897, d = 3, after
a short run -- md_mpc_sample at r_max = 4, 400 bins for NC = 1 and NC = 2 (user marks) and NC = 14 (the bond-order frame,
l = 6), each beside md_rdf_sample on the same handle in the same process: rdf is the same walk without marks, so it is
the yardstick.  Synchronised wall clock: a warm-up sample and a blocking read, then K samples and one blocking read;
repeated R times, the median reported with the spread.  Prints one JSON line.
python scripts/probe/mpc_rate.py"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from moleculardynamics.jl_amd import MDDevice, lattice_positions, initialize_velocities  # noqa: E402

N, rho, R_MAX, NBINS, K, R = 1 << 20, 0.897, 4.0, 400, 10, 5
box = np.full(3, (N / rho) ** (1.0 / 3.0))
x0 = lattice_positions(N, box, 3, np.random.default_rng(12345))
v0 = initialize_velocities(1.0, np.random.default_rng(67890), N, 3)
out = {"N": N, "r_max": R_MAX, "nbins": NBINS, "samples_per_repeat": K, "repeats": R}
dev = MDDevice(3, N, box, 2.5)
dev.set_potential(0, [1.0, 1.0, 2.5])
dev.upload(x0, v0, np.zeros_like(x0), np.zeros((N, 3), np.int32), np.ones(N))
dev.run(300, 0.002)                                     # melt the jittered lattice a little


def timed(sample, read):
    sample()
    read()                                              # warm-up, and the stream is idle
    ms = []
    for _ in range(R):
        t0 = time.perf_counter()
        for _ in range(K):
            sample()
        read()
        ms.append((time.perf_counter() - t0) / K * 1e3)
    return float(np.median(ms)), float(min(ms)), float(max(ms))


dev.rdf_setup(R_MAX, NBINS)
out["rdf_ms"], out["rdf_ms_min"], out["rdf_ms_max"] = timed(dev.rdf_sample, dev.rdf_read)
counts, ns = dev.rdf_read()
out["pairs_per_sample"] = int(counts.sum() // ns)
rng = np.random.default_rng(1)
for nc in (1, 2):
    dev.mpc_setup(R_MAX, NBINS, weights=np.ones(nc), tmax=float(nc))
    dev.mpc_marks(rng.uniform(-1.0, 1.0, (N, nc)))
    key = "mpc_nc%d" % nc
    out[key + "_ms"], out[key + "_ms_min"], out[key + "_ms_max"] = timed(dev.mpc_sample, dev.mpc_read)
    out[key + "_over_rdf"] = out[key + "_ms"] / out["rdf_ms"]
    assert dev.mpc_read()[5] == 0 and dev.mpc_last()[0].sum() == out["pairs_per_sample"]
dev.boo_setup(1.5, 6, 100, 0.7, 7, 0)
dev.boo_sample()
dev.mpc_setup(R_MAX, NBINS)
out["mpc_nc14_ms"], out["mpc_nc14_ms_min"], out["mpc_nc14_ms_max"] = timed(dev.mpc_sample, dev.mpc_read)
out["mpc_nc14_over_rdf"] = out["mpc_nc14_ms"] / out["rdf_ms"]
ns, cnt, tot, own, tmax, err = dev.mpc_read()
assert err == 0 and cnt.sum() == ns * out["pairs_per_sample"]
G = tot * 2.0 ** -31 / np.maximum(cnt, 1)
out["G6_at_r_1.1"], out["G6_at_r_3.9"] = float(G[110]), float(G[390])
out["mean_q6_squared"] = own * 2.0 ** -31 / ns / N
# rdf once more at the end: the yardstick did not drift
out["rdf_ms_after"] = timed(dev.rdf_sample, dev.rdf_read)[0]
dev.close()
print(json.dumps(out), flush=True)
