"""Time the Hessian apply (md_hess_apply) on the bench system: N = 2^20 LJ, rho = 0.897, d = 3, after a short equilibration
-- blocks of m = 1 and m = 8 vectors beside one md_compute_forces on the same handle and frame (all three walk the outer
rows and wait), synchronised wall clock over `ncalls` calls, `rounds` times alternated.  md_hess_apply takes and returns host
arrays, so its wall clock includes staging m N d doubles each way; the kernels alone are read from a kernel trace of this
script (rocprofv3 --kernel-trace --stats -- python scripts/probe/hess_rate.py ...).  Prints one JSON line and writes it, with
the derived ratios, to `out` (default profiles/hess_apply_rate.txt).
python scripts/probe/hess_rate.py [N] [ncalls] [rounds] [out]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np

from moleculardynamics.jl_amd import MDDevice, _lib, lattice_positions, initialize_velocities

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 20
ncalls = int(sys.argv[2]) if len(sys.argv) > 2 else 10
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
path = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "hess_apply_rate.txt")
rho = 0.897
L = (n / rho) ** (1.0 / 3.0)
box = np.full(3, L)
x = lattice_positions(n, box, 3, np.random.default_rng(12345))
v = initialize_velocities(1.4737, np.random.default_rng(67890), n, 3)
out = dict(n=n, rho=rho, ncalls=ncalls)

with MDDevice(3, n, box, 2.5) as dev:
    dev.set_potential(_lib.MD_POT_LJ, [1.0, 1.0, 2.5])
    dev.upload(x, v, np.zeros_like(x), np.zeros((n, 3), np.int32), np.ones(n))
    dev.run(200, 0.001)
    dev.hess_setup()
    X8 = np.random.default_rng(1).standard_normal((8, n, 3))
    X1 = X8[:1].copy()
    for _ in range(2):
        dev.hess_apply(X1)
        dev.hess_apply(X8)
        dev.compute_forces()
    res = dict(apply_m1_ms=[], apply_m8_ms=[], compute_forces_ms=[])
    for _ in range(rounds):
        for key, call in (("apply_m1_ms", lambda: dev.hess_apply(X1)), ("apply_m8_ms", lambda: dev.hess_apply(X8)),
                          ("compute_forces_ms", dev.compute_forces)):
            t0 = time.perf_counter()
            for _ in range(ncalls):
                call()
            res[key].append((time.perf_counter() - t0) * 1e3 / ncalls)
    Y8 = dev.hess_apply(X8)
    Y1 = dev.hess_apply(X1)
    st = dev.stats()
    out.update(res)
    out["best"] = {k: min(val) for k, val in res.items()}
    out["wall_ratio_m1_to_forces"] = out["best"]["apply_m1_ms"] / out["best"]["compute_forces_ms"]
    out["wall_gain_m8_vs_8x_m1"] = 8.0 * out["best"]["apply_m1_ms"] / out["best"]["apply_m8_ms"]
    out["tiled"] = st["tiled"]
    out["walked_outer"] = st["walked_outer"]
    out["column_0_same_bits"] = bool(np.array_equal(Y8[0], Y1[0]))
    out["translation_residual"] = float(np.abs(Y8.sum(axis=1)).max() / np.abs(Y8).max())     # sum_i (H X)_i = 0
line = json.dumps(out)
print(line, flush=True)
os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
with open(path, "w") as fh:
    fh.write("scripts/probe/hess_rate.py %d %d %d (wall clock per call, host arrays in and out; ms)\n%s\n" % (n, ncalls, rounds, line))
