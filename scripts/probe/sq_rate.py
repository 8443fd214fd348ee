"""Time the device density-mode sampler (md_sq_*) on the bench system: N = 2^20 LJ, rho = 0.897, d = 3, 1024 wave vectors
up to q_max = 8, after a short equilibration -- synchronised wall clock per md_sq_sample over `frames` frames after a
warm-up, static only and with one correlation plus an origin store.  In the same process, an independent baseline: the
same nvec x N sums by chunked fp64 torch on the device (cos / sin of f @ n^T, in chunks that fit memory), which also checks
the sampler's rho.  Prints one JSON line.
python scripts/probe/sq_rate.py [N] [nvec] [frames]
Per-kernel split: rocprofv3 --kernel-trace --stats -- python scripts/probe/sq_rate.py ..."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch

from moleculardynamics.jl_amd import MDDevice, _lib, initialize_velocities, lattice_positions, select_wave_vectors

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 20
nvec = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
frames = int(sys.argv[3]) if len(sys.argv) > 3 else 20
rho_n, q_max = 0.897, 8.0
L = (n / rho_n) ** (1.0 / 3.0)
box = np.full(3, L)
x = lattice_positions(n, box, 3, np.random.default_rng(12345))
v = initialize_velocities(1.4737, np.random.default_rng(67890), n, 3)
t0 = time.perf_counter()
vec, qlen, _ = select_wave_vectors(np.diag(box), q_max)
select_s = time.perf_counter() - t0
if vec.shape[0] < nvec:
    raise SystemExit(f"only {vec.shape[0]} vectors up to q_max = {q_max}")
keep = np.sort(np.random.default_rng(1).permutation(vec.shape[0])[:nvec])       # spread over all |q|
vec = vec[keep]
out = dict(n=n, rho=rho_n, nvec=nvec, q_max=q_max, frames=frames, select_wave_vectors_s=select_s,
           max_n1=int(np.abs(vec).sum(axis=1).max()), terms_per_frame=n * nvec)


def timed(dev, fn, k):
    dev.sq_read()                                    # waits for the stream
    t0 = time.perf_counter()
    for _ in range(k):
        fn()
    dev.sq_read()
    return (time.perf_counter() - t0) * 1e3 / k


with MDDevice(3, n, box, 2.5) as dev:
    dev.set_potential(_lib.MD_POT_LJ, [1.0, 1.0, 2.5])
    dev.upload(x, v, np.zeros_like(x), np.zeros((n, 3), np.int32), np.ones(n))
    dev.run(200, 0.001)
    dev.sq_setup(vec, 1, 1)
    dev.sq_sample(True, [], [], 0)
    for _ in range(3):
        dev.sq_sample(True, [0], [0])
    out["sample_static_ms"] = timed(dev, lambda: dev.sq_sample(True), frames)
    out["sample_full_ms"] = timed(dev, lambda: dev.sq_sample(True, [0], [0], 0), frames)
    out["sample_static_ms_repeat"] = timed(dev, lambda: dev.sq_sample(True), frames)
    rho_dev = dev.sq_rho()
    frame = dev.download()[0]

    # the baseline: f = x / L on the device once, then per chunk of particles cos / sin of 2 pi (f @ n^T) summed over particles
    g = torch.device("cuda")
    nt = torch.as_tensor(vec.astype(np.float64), device=g).T.contiguous()      # 3 x nvec
    chunk = 1 << 16                                                             # 65536 x 1024 doubles = 512 MiB per temporary

    f = torch.as_tensor(frame, device=g) / L

    def baseline():
        re = torch.zeros(nvec, dtype=torch.float64, device=g)
        im = torch.zeros(nvec, dtype=torch.float64, device=g)
        for i0 in range(0, n, chunk):
            ph = (2.0 * np.pi) * (f[i0:i0 + chunk] @ nt)
            re += torch.cos(ph).sum(dim=0)
            im += torch.sin(ph).sum(dim=0)
        return re, im

    for _ in range(2):
        re, im = baseline()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    kb = max(frames // 4, 3)
    for _ in range(kb):
        re, im = baseline()
    torch.cuda.synchronize()
    out["torch_baseline_ms"] = (time.perf_counter() - t0) * 1e3 / kb
    rho_t = re.cpu().numpy() + 1j * im.cpu().numpy()
    # the baseline forms 2 pi n.f without the exact reduction, so it is the less accurate of the two
    out["max_abs_rho_difference"] = float(np.abs(rho_dev - rho_t).max())
    out["max_abs_rho"] = float(np.abs(rho_dev).max())

out["speedup_vs_torch"] = out["torch_baseline_ms"] / out["sample_static_ms"]
out["paper_estimate_ms"] = 1.1
out["ratio_to_paper_estimate"] = out["sample_static_ms"] / 1.1
out["terms_per_s"] = out["terms_per_frame"] / (out["sample_static_ms"] * 1e-3)
out["faster_than_baseline"] = bool(out["sample_static_ms"] < out["torch_baseline_ms"])
print(json.dumps(out), flush=True)
if not out["faster_than_baseline"]:
    raise SystemExit("md_sq_sample is slower than the chunked torch baseline")
