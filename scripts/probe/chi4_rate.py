"""Time the device four-point sampler (md_chi4_*) on the bench system: N = 2^20 LJ, rho = 0.897, d = 3, nvec wave vectors up
to q_max = 8, after a short equilibration -- synchronised wall clock per md_chi4_sample (one (slot, row) per call, as the
log-time schedule makes them) over `frames` calls after a warm-up, at a short lag (Q ~ N) and at a lag where about 30 %
of the particles are still slow (`a` is set to that quantile of the displacements of a first pass).  In the same process:
md_sq_sample (static only) on the same vectors, and -- with vectors -- the same masked sums by chunked fp64 torch on the
device, which also checks W.  Prints one JSON line.
python scripts/probe/chi4_rate.py [N] [nvec] [frames]
Per-kernel split: rocprofv3 --kernel-trace --stats -- python scripts/probe/chi4_rate.py ..."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch

from moleculardynamics.jl_amd import MDDevice, _lib, initialize_velocities, lattice_positions, select_wave_vectors

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 20
nvec = int(sys.argv[2]) if len(sys.argv) > 2 else 128
frames = int(sys.argv[3]) if len(sys.argv) > 3 else 20
rho_n, q_max, long_lag, dt = 0.897, 8.0, 300, 0.002
L = (n / rho_n) ** (1.0 / 3.0)
box = np.full(3, L)
x = lattice_positions(n, box, 3, np.random.default_rng(12345))
v = initialize_velocities(1.4737, np.random.default_rng(67890), n, 3)
vec = None
if nvec > 0:
    vec, _, _ = select_wave_vectors(np.diag(box), q_max)
    if vec.shape[0] < nvec:
        raise SystemExit(f"only {vec.shape[0]} vectors up to q_max = {q_max}")
    vec = vec[np.sort(np.random.default_rng(1).permutation(vec.shape[0])[:nvec])]       # spread over all |q|
out = dict(n=n, rho=rho_n, nvec=nvec, q_max=q_max, frames=frames, long_lag=long_lag, terms_per_sample_at_q_n=n * nvec)


def timed(wait, fn, k):
    wait()                                           # waits for the stream
    t0 = time.perf_counter()
    for _ in range(k):
        fn()
    wait()
    return (time.perf_counter() - t0) * 1e3 / k


with MDDevice(3, n, box, 2.5) as dev:
    dev.set_potential(_lib.MD_POT_LJ, [1.0, 1.0, 2.5])
    dev.upload(x, v, np.zeros_like(x), np.zeros((n, 3), np.int32), np.ones(n))
    dev.run(200, dt)
    start = dev.download()
    dev.run(long_lag, dt)
    x1, _, _, i1 = dev.download()
    d2 = np.sum(((x1 - start[0]) + (i1 - start[3]) * L) ** 2, axis=1)
    a = float(np.sqrt(np.quantile(d2, 0.3)))
    out["a"] = a
    dev.upload(*start)
    dev.chi4_setup(a, vec, 1, 2)
    dev.chi4_origin(0)
    frame0 = start[0]
    for row, lag in ((0, 2), (1, long_lag - 2)):
        dev.run(lag, dt)
        for _ in range(3):
            dev.chi4_sample([0], [row])
        key = "short" if row == 0 else "long"
        out[f"sample_{key}_ms"] = timed(dev.chi4_read, lambda: dev.chi4_sample([0], [row]), frames)
        out[f"sample_{key}_ms_repeat"] = timed(dev.chi4_read, lambda: dev.chi4_sample([0], [row]), frames)
        q, w, slow = dev.chi4_last()
        out[f"q_over_n_{key}"] = q / n
        out[f"zero_mask_words_{key}"] = float(np.mean(slow.reshape(-1, 64).max(axis=1) == 0)) if n % 64 == 0 else None
    if nvec > 0:
        dev.sq_setup(vec)
        for _ in range(3):
            dev.sq_sample(True)
        out["sq_sample_static_ms"] = timed(dev.sq_read, lambda: dev.sq_sample(True), frames)
        out["sq_sample_static_ms_repeat"] = timed(dev.sq_read, lambda: dev.sq_sample(True), frames)
        # the baseline: the masked sums of the last sample (the long lag) by chunked fp64 torch
        g = torch.device("cuda")
        nt = torch.as_tensor(vec.astype(np.float64), device=g).T.contiguous()      # 3 x nvec
        chunk = max(1 << 12, (1 << 26) // nvec)                                     # 2^26 doubles = 512 MiB per temporary
        f = torch.as_tensor(frame0, device=g) / L
        m = torch.as_tensor(slow.astype(np.float64), device=g)

        def baseline():
            re = torch.zeros(nvec, dtype=torch.float64, device=g)
            im = torch.zeros(nvec, dtype=torch.float64, device=g)
            for i0 in range(0, n, chunk):
                ph = (2.0 * np.pi) * (f[i0:i0 + chunk] @ nt)
                re += m[i0:i0 + chunk] @ torch.cos(ph)
                im += m[i0:i0 + chunk] @ torch.sin(ph)
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
        out["max_abs_w_difference"] = float(np.abs(w - (re.cpu().numpy() + 1j * im.cpu().numpy())).max())
        out["max_abs_w"] = float(np.abs(w).max())
        out["terms_per_s_short"] = n * nvec / (out["sample_short_ms"] * 1e-3)
        out["sq_terms_per_s"] = n * nvec / (out["sq_sample_static_ms"] * 1e-3)
        out["speedup_vs_torch_long"] = out["torch_baseline_ms"] / out["sample_long_ms"]
print(json.dumps(out), flush=True)
