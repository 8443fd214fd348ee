"""Time the device current sampler (md_cur_*) against the density-mode sampler (md_sq_*) on the bench system: N = 2^20 LJ,
rho = 0.897, d = 3, 1024 wave vectors up to q_max = 8, after a short equilibration -- synchronised wall clock per
md_cur_sample and per md_sq_sample over `frames` frames after a warm-up, the two alternated in the same process on the
same frame and vectors, three rounds.  The yardstick is md_sq_sample of the same run; the expectation is the ratio of
fp64 instructions per term of the two compiled loops (scripts/isa_budget.py).  In the same process, an independent
baseline: the same d x nvec x N sums by chunked fp64 torch on the device, which also checks the sampler's j.  Prints one
JSON line.
python scripts/probe/cur_rate.py [N] [nvec] [frames]
Per-kernel split: rocprofv3 --kernel-trace --stats -- python scripts/probe/cur_rate.py ... (a run of its own)"""
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
rho_n, q_max, rounds = 0.897, 8.0, 3
L = (n / rho_n) ** (1.0 / 3.0)
box = np.full(3, L)
x = lattice_positions(n, box, 3, np.random.default_rng(12345))
v = initialize_velocities(1.4737, np.random.default_rng(67890), n, 3)
vec, qlen, _ = select_wave_vectors(np.diag(box), q_max)
if vec.shape[0] < nvec:
    raise SystemExit(f"only {vec.shape[0]} vectors up to q_max = {q_max}")
keep = np.sort(np.random.default_rng(1).permutation(vec.shape[0])[:nvec])       # spread over all |q|
vec = vec[keep]
qc = 2.0 * np.pi * vec.astype(np.float64) / L
e = qc / np.linalg.norm(qc, axis=1)[:, None]
out = dict(n=n, rho=rho_n, nvec=nvec, q_max=q_max, frames=frames, rounds=rounds,
           max_n1=int(np.abs(vec).sum(axis=1).max()), terms_per_frame=n * nvec)


def timed(read, fn, k):
    read()                                           # waits for the stream
    t0 = time.perf_counter()
    for _ in range(k):
        fn()
    read()
    return (time.perf_counter() - t0) * 1e3 / k


with MDDevice(3, n, box, 2.5) as dev:
    dev.set_potential(_lib.MD_POT_LJ, [1.0, 1.0, 2.5])
    dev.upload(x, v, np.zeros_like(x), np.zeros((n, 3), np.int32), np.ones(n))
    dev.run(200, 0.001)
    dev.sq_setup(vec, 1, 1)
    dev.cur_setup(vec, e, 1, 1, vacf=False)
    dev.sq_sample(True, [], [], 0)
    dev.cur_sample(True, [], [], 0)
    for _ in range(3):
        dev.sq_sample(True, [0], [0])
        dev.cur_sample(True, [0], [0])
    sq_ms, cur_ms, cur_full_ms = [], [], []
    for _ in range(rounds):                          # alternated: the same frame, the same vectors, the same clocks
        sq_ms.append(timed(dev.sq_read, lambda: dev.sq_sample(True), frames))
        cur_ms.append(timed(dev.cur_read, lambda: dev.cur_sample(True), frames))
        cur_full_ms.append(timed(dev.cur_read, lambda: dev.cur_sample(True, [0], [0], 0), frames))
    out["sq_sample_ms"], out["cur_sample_ms"], out["cur_sample_full_ms"] = sq_ms, cur_ms, cur_full_ms
    out["ratio_cur_to_sq"] = [c / s for c, s in zip(cur_ms, sq_ms)]
    out["sq_spread"] = (max(sq_ms) - min(sq_ms)) / min(sq_ms)
    out["cur_spread"] = (max(cur_ms) - min(cur_ms)) / min(cur_ms)
    # the VACF on top: one static Z and one lag pair per call, velocities stored with the origin
    dev.cur_setup(vec, e, 1, 1, vacf=True)
    dev.cur_sample(True, [], [], 0)
    dev.cur_sample(True, [0], [0], 0)
    out["cur_sample_full_vacf_ms"] = timed(dev.cur_read, lambda: dev.cur_sample(True, [0], [0], 0), frames)
    dev.cur_setup(None, None, 1, 1, vacf=True)
    dev.cur_sample(True, [], [], 0)
    out["vacf_only_ms"] = timed(dev.cur_read, lambda: dev.cur_sample(True, [0], [0], 0), frames)
    dev.cur_setup(vec, e, 0, 0, vacf=False)
    dev.cur_sample(True)
    j_dev = dev.cur_last()
    frame_x, frame_v = dev.download()[:2]

    # the baseline: f = x / L on the device once, then per chunk of particles cos / sin of 2 pi (f @ n^T), times v^T
    g = torch.device("cuda")
    nt = torch.as_tensor(vec.astype(np.float64), device=g).T.contiguous()      # 3 x nvec
    chunk = 1 << 16                                                             # 65536 x 1024 doubles = 512 MiB per temporary
    f = torch.as_tensor(frame_x, device=g) / L
    vt = torch.as_tensor(frame_v, device=g)

    def baseline():
        re = torch.zeros((nvec, 3), dtype=torch.float64, device=g)
        im = torch.zeros((nvec, 3), dtype=torch.float64, device=g)
        for i0 in range(0, n, chunk):
            ph = (2.0 * np.pi) * (f[i0:i0 + chunk] @ nt)
            re += torch.cos(ph).T @ vt[i0:i0 + chunk]
            im += torch.sin(ph).T @ vt[i0:i0 + chunk]
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
    j_t = re.cpu().numpy() + 1j * im.cpu().numpy()
    # the baseline forms 2 pi n.f without the exact reduction, so it is the less accurate of the two
    out["max_abs_j_difference"] = float(np.abs(j_dev - j_t).max())
    out["max_abs_j"] = float(np.abs(j_dev).max())

out["speedup_vs_torch"] = out["torch_baseline_ms"] / min(out["cur_sample_ms"])
out["terms_per_s"] = out["terms_per_frame"] / (min(out["cur_sample_ms"]) * 1e-3)
print(json.dumps(out), flush=True)
