"""Time the device cage-relative dynamics sampler (md_cage_*) on the bench system: N = 2^20 LJ, rho = 0.897, d = 3,
r_neigh = 1.5, max_neigh = 16, nq = 4, after a short run -- one md_cage_origin and one md_cage_sample at a short and at a
long lag beside one ordinary md_run step on the same handle (synchronised wall clock: the calls, then one blocking read),
and an independent baseline in the same process: a chunked fp64 torch evaluation of Del^CR and the surviving-bond count
from a prebuilt padded neighbour tensor (md_neighbor_pairs of a handle with list cutoff r_neigh on the origin frame),
compared with the device's values.  Prints one JSON line per stage.
python scripts/probe/cage_rate.py [--profile]
--profile: only the steps, a few origins and samples, no torch -- the run to put under `rocprofv3 --kernel-trace --stats`
for the per-kernel times (a run of its own: tracing slows the host)."""
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
profile = "--profile" in sys.argv
if not profile:
    import torch                                        # (torch first, as bench.py does: it must find the device itself)
    torch.cuda.set_device(0)
    torch.zeros(1, device="cuda")
from moleculardynamics.jl_amd import MDDevice, lattice_positions, initialize_velocities  # noqa: E402

N, rho = 1 << 20, 0.897
R_N, R_B, MAXN = 1.5, 1.7, 16
Q = [2.0 * math.pi, 4.0, 7.0, 11.3]
SHORT, LONG = 10, 400
box = np.full(3, (N / rho) ** (1.0 / 3.0))
x0 = lattice_positions(N, box, 3, np.random.default_rng(12345))
v0 = initialize_velocities(1.0, np.random.default_rng(67890), N, 3)
out = {"N": N, "max_neigh": MAXN, "nq": len(Q)}
dev = MDDevice(3, N, box, 2.5)
dev.set_potential(0, [1.0, 1.0, 2.5])
dev.upload(x0, v0, np.zeros_like(x0), np.zeros((N, 3), np.int32), np.ones(N))
dev.run(300, 0.002)                                     # melt the jittered lattice a little, settle the list schedule
t0 = time.perf_counter()
dev.run(200, 0.002)
out["step_ms"] = (time.perf_counter() - t0) / 200 * 1e3
out["tiled"] = dev.stats()["tiled"]
dev.cage_setup(1, 2, R_N, R_B, False, MAXN, Q)
out["table_MB"] = N * MAXN * 28 / 1e6
K = 3 if profile else 10
dev.cage_origin(0)
dev.cage_read()
t0 = time.perf_counter()
for _ in range(K):
    dev.cage_origin(0)
dev.cage_read()
out["origin_ms"] = (time.perf_counter() - t0) / K * 1e3
for row, (name, steps) in enumerate((("short", SHORT), ("long", LONG - SHORT))):
    dev.run(steps, 0.002)
    dev.cage_sample([0], [row])
    dev.cage_read()
    dev.cage_reset()
    t0 = time.perf_counter()
    for _ in range(K):
        dev.cage_sample([0], [row])
    ns, sums, counts, hist, overflow = dev.cage_read()
    out["sample_ms_" + name] = (time.perf_counter() - t0) / K * 1e3
    out["msd_cr_" + name] = sums[row, 0] / counts[row, 0]
    out["C_B_" + name] = counts[row, 2] / counts[row, 1]
out["overflow"] = int(overflow)                         # (a liquid has particles with more than 16 neighbours within 1.5)
print(json.dumps(out), flush=True)
if profile:
    sys.exit(0)

# ---- torch baseline: Del^CR and the surviving bonds from a padded neighbour tensor, fp64, chunked ---------------------
# (max_neigh = 32 on the device for the comparison, so that no neighbour is dropped; a new origin on the same handle)
dev.cage_setup(1, 1, R_N, R_B, False, 32, Q)
dev.cage_origin(0)
f0 = dev.download()
dev.run(LONG, 0.002)
f1 = dev.download()
dev.cage_sample([0], [0])
nnb_dev, d2_dev, broken_dev = dev.cage_particles()
_, sums, counts, _, overflow = dev.cage_read()
dev.close()
z = np.zeros_like(x0)
d2h = MDDevice(3, N, box, R_N)
d2h.set_potential(0, [1.0, 1.0, R_N])
d2h.upload(f0[0], z, z, np.zeros(x0.shape, np.int32), np.ones(N))
pairs = d2h.neighbor_pairs()                            # d2 <= r_n^2: the bond test below is the strict one
d2h.close()
g = torch.device("cuda")
X0 = torch.from_numpy(f0[0]).to(g)
L = torch.tensor(box, dtype=torch.float64, device=g)
DEL = torch.from_numpy((f1[0] - f0[0]) + (f1[3] - f0[3]).astype(np.float64) * box).to(g)
P = torch.from_numpy(pairs.astype(np.int64)).to(g)
bi = torch.cat([P[:, 0], P[:, 1]])
bj = torch.cat([P[:, 1], P[:, 0]])
order = torch.argsort(bi, stable=True)
bi, bj = bi[order], bj[order]
cnt = torch.bincount(bi, minlength=N)
start = torch.cumsum(cnt, 0) - cnt
col = torch.arange(len(bi), device=g) - start[bi]
W = int(cnt.max().item())
idx = torch.full((N, W), -1, dtype=torch.int64, device=g)
idx[bi, col] = bj


def cage_torch(chunk=1 << 17):
    d2 = torch.empty(N, dtype=torch.float64, device=g)
    alive = torch.zeros((), dtype=torch.int64, device=g)
    nn = torch.empty(N, dtype=torch.int64, device=g)
    for a in range(0, N, chunk):
        ii = idx[a:a + chunk]
        jj = ii.clamp(min=0)
        de = X0[jj] - X0[a:a + chunk, None, :]
        de = de - L * torch.round(de / L)
        bond = (ii >= 0) & ((de * de).sum(-1) < R_N * R_N)
        w = bond.to(torch.float64)
        n = w.sum(-1)
        dj = DEL[jj]
        di = DEL[a:a + chunk]
        mean = (dj * w[..., None]).sum(1) / n.clamp(min=1.0)[:, None]
        cr = torch.where((n > 0)[:, None], di - mean, torch.zeros_like(di))
        d2[a:a + chunk] = (cr * cr).sum(-1)
        b = de + (dj - di[:, None, :])
        alive = alive + (bond & ((b * b).sum(-1) < R_B * R_B)).sum()
        nn[a:a + chunk] = n.to(torch.int64)
    return d2, alive, nn


d2t, alive, nn = cage_torch()
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(5):
    d2t, alive, nn = cage_torch()
torch.cuda.synchronize()
out2 = {"torch_cage_ms": (time.perf_counter() - t0) / 5 * 1e3, "torch_pad_width": W}
out2["torch_vs_device_max_abs_d2"] = float(np.abs(d2t.cpu().numpy() - d2_dev).max())
out2["torch_nnb_equal"] = bool(np.array_equal(nn.cpu().numpy(), nnb_dev))
out2["torch_surviving"], out2["device_surviving"] = int(alive.item()), int(counts[0, 2])
out2["device_overflow_at_32"] = int(overflow)
out2["ratio_torch_over_sample_long"] = out2["torch_cage_ms"] / out["sample_ms_long"]
print(json.dumps(out2), flush=True)
