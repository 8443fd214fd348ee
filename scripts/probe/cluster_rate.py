"""Time the device cluster sampler (md_cluster_*) on the bench system: N = 2^20 LJ, rho = 0.897, d = 3, after a short run
-- one md_cluster_sample in ALL mode at r_bond = 1.0 (sparse) and 1.5 (the liquid is one giant component: the worst
contention on one root) and in SOLID mode after a bond-order sample, beside one ordinary md_run step and one
md_boo_sample on the same handle (synchronised wall clock: the calls, then one blocking read), and an independent
baseline: the frame downloaded, a pair list built on the host (scipy cKDTree on the periodic box) and
scipy.sparse.csgraph.connected_components on it, compared with the device's labels.  Prints one JSON line per stage.
python scripts/probe/cluster_rate.py [--profile]
--profile: only the steps and a few samples, no host baseline -- the run to put under `rocprofv3 --kernel-trace --stats`
for the per-kernel times (a run of its own: tracing slows the host)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
profile = "--profile" in sys.argv
from moleculardynamics.jl_amd import MDDevice, lattice_positions, initialize_velocities  # noqa: E402

N, rho = 1 << 20, 0.897
box = np.full(3, (N / rho) ** (1.0 / 3.0))
x0 = lattice_positions(N, box, 3, np.random.default_rng(12345))
v0 = initialize_velocities(1.0, np.random.default_rng(67890), N, 3)
out = {"N": N}
dev = MDDevice(3, N, box, 2.5)
dev.set_potential(0, [1.0, 1.0, 2.5])
dev.upload(x0, v0, np.zeros_like(x0), np.zeros((N, 3), np.int32), np.ones(N))
dev.run(300, 0.002)                                     # melt the jittered lattice a little, settle the list schedule
t0 = time.perf_counter()
dev.run(200, 0.002)
out["step_ms"] = (time.perf_counter() - t0) / 200 * 1e3
out["tiled"] = dev.stats()["tiled"]
K = 5 if profile else 20

dev.boo_setup(1.5, 6, 100, 0.7, 7, 0)
dev.boo_sample()
dev.boo_read()
t0 = time.perf_counter()
for _ in range(K):
    dev.boo_sample()
_, bfr, *_ = dev.boo_read()
out["boo_sample_ms"] = (time.perf_counter() - t0) / K * 1e3


def timed(tag, r_bond, members):
    dev.cluster_setup(r_bond, members, 1024, 0)
    dev.cluster_sample()
    dev.cluster_read()
    t0 = time.perf_counter()
    for _ in range(K):
        dev.cluster_sample()
    ns, fr, _, _ = dev.cluster_read()
    out["cluster_%s_ms" % tag] = (time.perf_counter() - t0) / K * 1e3
    out["cluster_%s_fr" % tag] = [int(v) for v in fr // ns]


timed("all_r1.0", 1.0, 0)
timed("all_r1.5", 1.5, 0)
timed("solid_r1.5", 1.5, 1)
print(json.dumps(out), flush=True)
if profile:
    sys.exit(0)

# ---- host baseline: download, pair list, scipy connected components ---------------------------------------------------
from scipy.sparse import coo_matrix  # noqa: E402
from scipy.sparse.csgraph import connected_components  # noqa: E402
from scipy.spatial import cKDTree  # noqa: E402

for r_bond in (1.0, 1.5):
    dev.cluster_setup(r_bond, 0, 1024, 0)
    dev.cluster_sample()
    label, size = dev.cluster_particles()
    t0 = time.perf_counter()
    x = dev.download()[0]
    t1 = time.perf_counter()
    pairs = cKDTree(np.mod(x, box), boxsize=box).query_pairs(r_bond, output_type="ndarray")
    t2 = time.perf_counter()
    g = coo_matrix((np.ones(len(pairs), dtype=np.int8), (pairs[:, 0], pairs[:, 1])), shape=(N, N))
    ncomp, comp = connected_components(g, directed=False)
    t3 = time.perf_counter()
    smallest = np.full(ncomp, N, dtype=np.int64)
    np.minimum.at(smallest, comp, np.arange(N))
    res = {"r_bond": r_bond, "host_download_ms": (t1 - t0) * 1e3, "host_pairs_ms": (t2 - t1) * 1e3,
           "host_components_ms": (t3 - t2) * 1e3, "host_total_ms": (t3 - t0) * 1e3, "pairs": int(len(pairs)),
           "components": int(ncomp), "labels_identical": bool(np.array_equal(smallest[comp], label)),
           "sizes_identical": bool(np.array_equal(np.bincount(comp)[comp], size))}
    print(json.dumps(res), flush=True)
dev.close()
