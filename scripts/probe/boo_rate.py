"""Time the device bond-order sampler (md_boo_*) on the bench system: N = 2^20 LJ, rho = 0.897, d = 3, r_n = 1.5, after a
short run -- one md_boo_sample for l = 6 and l = 4 beside one ordinary md_run step on the same handle (synchronised wall
clock: the calls, then one blocking read), and an independent baseline in the same process: a chunked fp64 torch
evaluation of q_6(i) alone from a padded neighbour index tensor built from md_neighbor_pairs of a handle with list cutoff
r_n, compared with the device's q_6.  Prints one JSON line per stage.
python scripts/probe/boo_rate.py [--profile]
--profile: only the steps and a few samples, no torch -- the run to put under `rocprofv3 --kernel-trace --stats` for the
per-kernel times (a run of its own: tracing slows the host)."""
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
st = dev.stats()
out["tiled"], out["max_halo"] = st["tiled"], st.get("max_halo")
for l in (6, 4):
    dev.boo_setup(1.5, l, 100, 0.7, 7, 64)
    dev.boo_sample()
    dev.boo_read()
    K = 5 if profile else 20
    t0 = time.perf_counter()
    for _ in range(K):
        dev.boo_sample()
    ns, fr, *_ = dev.boo_read()
    out["sample_ms_l%d" % l] = (time.perf_counter() - t0) / K * 1e3
    out["mean_q%d" % l] = fr[0] / ns / N
    out["mean_n"] = fr[4] / ns / N
    out["solid_fraction_l%d" % l] = fr[6] / ns / N
print(json.dumps(out), flush=True)
if profile:
    sys.exit(0)

# ---- torch baseline: q_6(i) from a padded neighbour index tensor, fp64, chunked -------------------------------------
dev.boo_setup(1.5, 6, 100, 0.7, 7, 0)
dev.boo_sample()
nnb_dev, q_dev, _, _ = dev.boo_particles()
x = dev.download()[0]
dev.close()
d2 = MDDevice(3, N, box, 1.5)
d2.set_potential(0, [1.0, 1.0, 1.5])
z = np.zeros_like(x)
d2.upload(x, z, z, np.zeros(x.shape, np.int32), np.ones(N))
pairs = d2.neighbor_pairs()
d2.close()
g = torch.device("cuda")
X = torch.from_numpy(x).to(g)
L = torch.tensor(box, dtype=torch.float64, device=g)
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
coef = [(-1) ** m * math.sqrt(13.0 / (4 * math.pi) * math.factorial(6 - m) / math.factorial(6 + m)) for m in range(7)]


def q6_torch(chunk=1 << 17):
    res = torch.empty(N, dtype=torch.float64, device=g)
    for a in range(0, N, chunk):
        ii = idx[a:a + chunk]
        valid = ii >= 0
        de = X[ii.clamp(min=0)] - X[a:a + chunk, None, :]
        de = de - L * torch.round(de / L)
        r2 = (de * de).sum(-1)
        hit = valid & (r2 < 2.25)
        rinv = torch.rsqrt(torch.where(hit, r2, torch.ones_like(r2)))
        w = hit.to(torch.float64)
        u = de * rinv[..., None]
        zc, z2 = u[..., 2], u[..., 2] ** 2
        D = [(((231 * z2 - 315) * z2 + 105) * z2 - 5) / 16, ((693 * z2 - 630) * z2 + 105) * zc / 8,
             ((3465 * z2 - 1890) * z2 + 105) / 8, (3465 * z2 - 945) * zc / 2, (10395 * z2 - 945) / 2, 10395 * zc,
             torch.full_like(zc, 10395.0)]
        e = torch.complex(u[..., 0], u[..., 1])
        p = torch.complex(w, torch.zeros_like(w))
        n = w.sum(-1).clamp(min=1.0)
        tot = torch.zeros(ii.shape[0], dtype=torch.float64, device=g)
        for m in range(7):
            if m:
                p = p * e
            qm = coef[m] * (D[m] * p).sum(-1) / n
            tot = tot + (1.0 if m == 0 else 2.0) * (qm.real ** 2 + qm.imag ** 2)
        res[a:a + chunk] = torch.sqrt(4 * math.pi / 13.0 * tot)
    return res


q = q6_torch()
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(5):
    q = q6_torch()
torch.cuda.synchronize()
out["torch_q6_ms"] = (time.perf_counter() - t0) / 5 * 1e3
out["torch_pad_width"] = W
out["torch_vs_device_max_abs"] = float(np.abs(q.cpu().numpy() - q_dev).max())
out["torch_nnb_equal"] = bool(np.array_equal(cnt.cpu().numpy(), nnb_dev))
out["ratio_torch_q6_over_sample_l6"] = out["torch_q6_ms"] / out["sample_ms_l6"]
print(json.dumps(out), flush=True)
